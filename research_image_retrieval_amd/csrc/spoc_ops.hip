// spoc_ops.hip — the SpoC head's kernels (gfx950): the spatial pyramid of
// max-pools in one launch, the gated half of the refine conv (the 1x1 conv over
// cat[x a, ctx] with the attention gate applied in the epilogue), and a linear
// whose product is needed only as a per-image max over region rows.
//
// Reference (models/spoc.py): SpatialPyramidPooling.forward :20-49
// (pool_type 'max'), ContextualAttention.forward :83-92 (attention_conv +
// sigmoid, the multiply, the cat, feature_refine) and feature_aggregation
// :131-136 (Conv1d + BatchNorm1d + ReLU + AdaptiveMaxPool1d(1)).
#include <cmath>

#include "heads_common.hpp"

namespace rr {

constexpr int kSpocThreads = 256;         // 4 waves per workgroup
constexpr int kSpocTile = 64;             // rows and columns of a workgroup's product tile
constexpr int kSpocStep = 32;             // k per step
constexpr int kSpocLd = kSpocStep + 4;    // staged row stride: rows 36 words apart, lanes (lq, lg) hit 64 banks
constexpr int kSpocTs = kSpocTile + 4;    // staged output tile row stride (16-B aligned rows)
constexpr int kSppMaxLevels = 8;

// The pyramid as the kernel reads it: level l pools kh x kw windows at stride
// (kh, kw) into oh x ow regions, the first of them region start[l].
struct SppPlan {
  int n;
  int kh[kSppMaxLevels], kw[kSppMaxLevels], ow[kSppMaxLevels], start[kSppMaxLevels];
};

// The reference's windows (:27-35): kernel = stride = (H // L, W // L), no
// padding, floor mode.  Returns the region count, or -1 for a level that is
// < 1 or above hgt or wid (the reference: "stride should not be zero").
inline long long spp_plan(int hgt, int wid, const int* levels, int nlevels, SppPlan* plan) {
  if (hgt < 1 || wid < 1 || !levels || nlevels < 1 || nlevels > kSppMaxLevels) return -1;
  long long r = 0;
  for (int l = 0; l < nlevels; ++l) {
    const int lv = levels[l];
    if (lv < 1 || lv > hgt || lv > wid) return -1;
    const int kh = hgt / lv, kw = wid / lv;
    const int oh = hgt / kh, ow = wid / kw;
    if (r > 0x7fffffffLL) return -1;
    if (plan) {
      plan->kh[l] = kh;
      plan->kw[l] = kw;
      plan->ow[l] = ow;
      plan->start[l] = (int)r;
    }
    r += (long long)oh * ow;
  }
  if (r > 0x7fffffffLL) return -1;
  if (plan) plan->n = nlevels;
  return r;
}

// One workgroup per (image, region): a thread takes 16 B of channels and walks
// the window, the max starting from the window's first element.  The level of
// a region is found by constant-index compares (no indexed copy of the plan).
__global__ __launch_bounds__(kSpocThreads) void spp_max_kernel(const float* __restrict__ x, int hgt, int wid, int c,
                                                               SppPlan plan, int regions, float* __restrict__ out) {
  const int img = blockIdx.x / regions, r = blockIdx.x - img * regions;
  int kh = 1, kw = 1, ow = 1, start = 0;
#pragma unroll
  for (int l = 0; l < kSppMaxLevels; ++l)
    if (l < plan.n && r >= plan.start[l]) {
      kh = plan.kh[l];
      kw = plan.kw[l];
      ow = plan.ow[l];
      start = plan.start[l];
    }
  const int q = r - start;
  const int oy = q / ow, ox = q - oy * ow;
  const float* base = x + (((long long)img * hgt + (long long)oy * kh) * wid + (long long)ox * kw) * c;
  float* orow = out + (long long)blockIdx.x * c;
  for (int c4 = threadIdx.x; c4 < (c >> 2); c4 += kSpocThreads) {
    const float* p = base + c4 * 4;
    f32x4 m = *reinterpret_cast<const f32x4*>(p);
    for (int dy = 0; dy < kh; ++dy) {
      const float* prow = p + (long long)dy * wid * c;
#pragma unroll 4
      for (int dx = 0; dx < kw; ++dx) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(prow + (long long)dx * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
      }
    }
    *reinterpret_cast<f32x4*>(orow + c4 * 4) = m;
  }
}

// The 64 x 64 product tile both GEMM kernels share: acc = A B^T over k, A
// [rows_a][lda] and B [rows_b][ldb] with k contiguous (rows past rows_a /
// rows_b and k past the end read as 0; k % 4 == 0).  A step takes 32 of k: the
// thread's two 16-B pieces of A and of B travel global -> registers (issued one
// step ahead) -> As / Bs [row][k], then v_mfma_f32_16x16x4_f32, wave (wi, wj)
// owning the 32 x 32 quadrant.  LOGIT: logit[i] also receives w_att . A[row]
// for the thread's rows row0 + 32 i — its eight k-pieces as one fmaf chain in k
// order, the eight threads of a row added by xor 1, 2, 4 (commutative at every
// level: the eight hold the same bits) — an order that depends on k alone, so
// every column tile of a row tile computes the same bits.
// After the call lane (lq, lg) of wave (wi, wj) holds in acc[i][j][r] the
// element (row 32 wi + 16 i + 4 lg + r, column 32 wj + 16 j + lq).
template <bool LOGIT>
__device__ __forceinline__ void spoc_tile_product(const float* __restrict__ A, long long lda, int rows_a,
                                                  const float* __restrict__ B, long long ldb, int rows_b, int k,
                                                  const float* __restrict__ w_att, float* lds, f32x4 (&acc)[2][2],
                                                  float (&logit)[2]) {
  float* As = lds;
  float* Bs = lds + kSpocTile * kSpocLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int wi = wave & 1, wj = wave >> 1;
  const int c4 = tid & 7, row0 = tid >> 3;
  const int steps = (k + kSpocStep - 1) / kSpocStep;

  f32x4 ra[2], rb[2], wv;
  auto load_step = [&](int st) {
    const int kk = st * kSpocStep + c4 * 4;
    const bool okk = kk < k;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = row0 + 32 * i;
      ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      rb[i] = ra[i];
      if (okk && row < rows_a) ra[i] = *reinterpret_cast<const f32x4*>(A + (long long)row * lda + kk);
      if (okk && row < rows_b) rb[i] = *reinterpret_cast<const f32x4*>(B + (long long)row * ldb + kk);
    }
    if (LOGIT) {
      wv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (okk) wv = *reinterpret_cast<const f32x4*>(w_att + kk);
    }
  };
  load_step(0);

#pragma unroll
  for (int i = 0; i < 2; ++i) {
    logit[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int st = 0; st < steps; ++st) {
    __syncthreads();  // the previous step's readers are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<f32x4*>(As + (row0 + 32 * i) * kSpocLd + c4 * 4) = ra[i];
      *reinterpret_cast<f32x4*>(Bs + (row0 + 32 * i) * kSpocLd + c4 * 4) = rb[i];
      if (LOGIT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) logit[i] = fmaf(ra[i][e], wv[e], logit[i]);
      }
    }
    if (st + 1 < steps) load_step(st + 1);
    __syncthreads();
    const float* pa = As + (32 * wi + lq) * kSpocLd + lg;
    const float* pb = Bs + (32 * wj + lq) * kSpocLd + lg;
#pragma unroll
    for (int kk = 0; kk < kSpocStep / 4; ++kk) {
      const float a0 = pa[4 * kk], a1 = pa[16 * kSpocLd + 4 * kk];
      const float b0 = pb[4 * kk], b1 = pb[16 * kSpocLd + 4 * kk];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  if (LOGIT) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      logit[i] += __shfl_xor(logit[i], 1, 64);
      logit[i] += __shfl_xor(logit[i], 2, 64);
      logit[i] += __shfl_xor(logit[i], 4, 64);
    }
  }
}

// y[row][:] = a_row u[row][:] + ctx_row w_c^T + bias, a_row = sigmoid(ctx_row .
// w_att + b_att).  Workgroup (row tile, column tile), column tile fastest: the
// product over dc on the MFMA, the logit beside it from the staged rows, the
// tile staged in LDS and the gate applied in the epilogue on 16-B pieces, each
// read from u and written to y by the same thread (y may alias u).  Column
// tile 0 writes att.
__global__ __launch_bounds__(kSpocThreads) void spoc_refine_kernel(const float* u, const float* __restrict__ ctx,
                                                                   int m, int c, int dc,
                                                                   const float* __restrict__ w_att, float b_att,
                                                                   const float* __restrict__ w_c,
                                                                   const float* __restrict__ bias,
                                                                   float* __restrict__ att, float* y, int tiles_n) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kSpocTile * kSpocLd];
  __shared__ float arow[kSpocTile];
  static_assert(kSpocTile * kSpocTs <= 2 * kSpocTile * kSpocLd, "the staged tile reuses the step buffers");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int wi = wave & 1, wj = wave >> 1;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const long long m0 = (long long)tm * kSpocTile;
  const int n0 = tn * kSpocTile;
  const int rows_a = m - m0 < kSpocTile ? (int)(m - m0) : kSpocTile;
  const int rows_b = c - n0 < kSpocTile ? c - n0 : kSpocTile;

  f32x4 acc[2][2];
  float logit[2];
  spoc_tile_product<true>(ctx + m0 * dc, dc, rows_a, w_c + (long long)n0 * dc, dc, rows_b, dc, w_att, lds, acc, logit);

  if ((tid & 7) == 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (tid >> 3) + 32 * i;
      const float a = 1.f / (1.f + expf(-(logit[i] + b_att)));
      arow[row] = a;
      if (att != nullptr && tn == 0 && row < rows_a) att[m0 + row] = a;
    }
  }
  __syncthreads();  // every read of As / Bs is done: the tile takes their place
  float* Ts = lds;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) Ts[(32 * wi + 16 * i + 4 * lg + r) * kSpocTs + 32 * wj + 16 * j + lq] = acc[i][j][r];
  __syncthreads();
#pragma unroll
  for (int e = tid; e < kSpocTile * (kSpocTile / 4); e += kSpocThreads) {
    const int row = e >> 4, col = (e & 15) * 4;
    if (row < rows_a && col < rows_b) {
      const long long off = (m0 + row) * c + n0 + col;
      const f32x4 uv = *reinterpret_cast<const f32x4*>(u + off);
      const f32x4 t = *reinterpret_cast<const f32x4*>(Ts + row * kSpocTs + col);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + n0 + col);
      const float a = arow[row];
      f32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = fmaf(a, uv[q], t[q] + bv[q]);
      *reinterpret_cast<f32x4*>(y + off) = o;
    }
  }
}

// out[img][col] = max_{j < r} act(x[img r + j] . w[col] + bias[col]).
// Workgroup (image, column tile): the image's r <= 64 rows are the tile's rows,
// rows past r are loaded as 0 and LEFT OUT of the max (a zero row would give
// act(bias), which beats a true maximum of 0 where bias > 0); the max starts at
// -inf, runs over the lane's accumulators, the lanes 16 and 32 apart, then the
// two row halves through LDS.  A max has no order: the same bits however it is
// grouped, an image alone or in a batch.
__global__ __launch_bounds__(kSpocThreads) void linear_groupmax_kernel(const float* __restrict__ x, int r, int k,
                                                                       const float* __restrict__ w,
                                                                       const float* __restrict__ bias, int n, int act,
                                                                       float* __restrict__ out, int tiles_n) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kSpocTile * kSpocLd];
  __shared__ float red[2][kSpocTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int wi = wave & 1, wj = wave >> 1;
  const int img = blockIdx.x / tiles_n, tn = blockIdx.x - img * tiles_n;
  const int n0 = tn * kSpocTile;
  const int rows_b = n - n0 < kSpocTile ? n - n0 : kSpocTile;

  f32x4 acc[2][2];
  float unused[2];
  spoc_tile_product<false>(x + (long long)img * r * k, k, r, w + (long long)n0 * k, k, rows_b, k, nullptr, lds, acc,
                           unused);

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = 32 * wj + 16 * j + lq;
    const float bv = (bias != nullptr && col < rows_b) ? bias[n0 + col] : 0.f;
    float v = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 32 * wi + 16 * i + 4 * lg + q;
        float t = acc[i][j][q] + bv;
        if (act == 1) t = fmaxf(t, 0.f);
        if (row < r) v = fmaxf(v, t);
      }
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    if (lg == 0) red[wi][col] = v;
  }
  __syncthreads();
  if (tid < rows_b) out[(long long)img * n + n0 + tid] = fmaxf(red[0][tid], red[1][tid]);
}

}  // namespace rr

using namespace rr;

extern "C" int rr_spp_regions(int hgt, int wid, const int* levels, int nlevels) {
  return (int)spp_plan(hgt, wid, levels, nlevels, nullptr);
}

extern "C" int rr_spp_max(rr_handle_t h, const float* x, int b, int hgt, int wid, int c, const int* levels, int nlevels,
                          float* out, void* stream) {
  RR_ENTRY(h);
  SppPlan plan = {};
  long long regions = -1;
  if (x && out && levels && b >= 0 && c >= 4 && !(c & 3) && !((uintptr_t)x & 15) && !((uintptr_t)out & 15))
    regions = spp_plan(hgt, wid, levels, nlevels, &plan);
  if (regions < 1)
    return set_error(h, RR_EINVAL,
                     "rr_spp_max: bad argument (1 <= nlevels <= 8, 1 <= level <= min(hgt, wid), c % 4 == 0, 16-B "
                     "aligned)");
  if (b == 0) return RR_OK;
  if ((long long)b * regions > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_spp_max: too many regions");
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch tl(h, kTimeElem, s);
  hipLaunchKernelGGL(spp_max_kernel, dim3((unsigned)(b * regions)), dim3(kSpocThreads), 0, s, x, hgt, wid, c, plan,
                     (int)regions, out);
  return check_hip(h, hipGetLastError(), "spp_max launch");
}

extern "C" int rr_spoc_refine(rr_handle_t h, const float* u, const float* ctx, int m, int c, int dc,
                              const float* w_att, float b_att, const float* w_c, const float* bias, float* att,
                              float* y, void* stream) {
  RR_ENTRY(h);
  if (!u || !ctx || !w_att || !w_c || !bias || !y || m < 0 || c < 4 || (c & 3) || dc < 32 || dc > 2048 || (dc & 31) ||
      ((uintptr_t)u & 15) || ((uintptr_t)ctx & 15) || ((uintptr_t)w_att & 15) || ((uintptr_t)w_c & 15) ||
      ((uintptr_t)bias & 15) || ((uintptr_t)att & 15) || ((uintptr_t)y & 15))
    return set_error(h, RR_EINVAL,
                     "rr_spoc_refine: bad argument (dc % 32 == 0, 32 <= dc <= 2048, c % 4 == 0, m >= 0, 16-B aligned)");
  if (m == 0) return RR_OK;
  const long long tiles_m = ((long long)m + kSpocTile - 1) / kSpocTile;
  const int tiles_n = (c + kSpocTile - 1) / kSpocTile;
  if (tiles_m * tiles_n > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_spoc_refine: too many tiles");
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch tl(h, kTimeGemm, s);
  hipLaunchKernelGGL(spoc_refine_kernel, dim3((unsigned)(tiles_m * tiles_n)), dim3(kSpocThreads), 0, s, u, ctx, m, c,
                     dc, w_att, b_att, w_c, bias, att, y, tiles_n);
  return check_hip(h, hipGetLastError(), "spoc_refine launch");
}

extern "C" int rr_linear_groupmax(rr_handle_t h, const float* x, int b, int r, int k, const float* w,
                                  const float* bias, int n, int act, float* out, void* stream) {
  RR_ENTRY(h);
  if (!x || !w || !out || b < 0 || r < 1 || r > kSpocTile || k < 4 || (k & 3) || n < 1 || act < 0 || act > 1 ||
      ((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)out & 15))
    return set_error(h, RR_EINVAL,
                     "rr_linear_groupmax: bad argument (1 <= r <= 64, k % 4 == 0, n >= 1, act 0 or 1, b >= 0, 16-B "
                     "aligned)");
  if (b == 0) return RR_OK;
  const int tiles_n = (n + kSpocTile - 1) / kSpocTile;
  if ((long long)b * tiles_n > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_linear_groupmax: too many tiles");
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch tl(h, kTimeGemm, s);
  hipLaunchKernelGGL(linear_groupmax_kernel, dim3((unsigned)(b * tiles_n)), dim3(kSpocThreads), 0, s, x, r, k, w, bias,
                     n, act, out, tiles_n);
  return check_hip(h, hipGetLastError(), "linear_groupmax launch");
}
