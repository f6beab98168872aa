// token_ops.hip — the Token head's three kernels (gfx950): multi-head attention
// at head width 128 with separate query and key counts, the object-token
// pooling, and the exact (erf) GELU.
//
// Reference (networks/RetrievalNet.py): Attention.forward :117-126 (8 heads of
// 128 over mid_dim 1024, self-attention over the map's positions,
// cross-attention from the 4 object tokens to the positions, self-attention
// over the tokens), Token_Refine.forward :180-182 (softmax over the objects,
// attns @ x) and GELU :67-72 (F.gelu, the erf form).
#include <cmath>

#include "heads_common.hpp"

namespace rr {

// ---- rr_attention_hd128 ---------------------------------------------------
constexpr int kHdDim = 128;        // head width
constexpr int kHdLd = kHdDim + 4;  // LDS row: 16-B reads by key row and 4-B reads of four key rows are conflict-free
constexpr int kHdWaves = 4;

// Two forms, chosen by nq alone:
//  KSPLIT = false (nq > 16): a workgroup is (image, head, 64 queries); wave w
//   owns queries [16 w, 16 w + 16) of them and the whole head width.  16-key
//   K and V tiles (2 x 16 x 132 floats = 16.5 KiB of LDS) stream past; the
//   four waves share each tile and never exchange anything else.
//  KSPLIT = true (nq <= 16, the object tokens): a workgroup is (image, head,
//   the 16-query tile); the streamed tile is 64 keys deep (66 KiB) and wave w
//   owns keys [16 w, 16 w + 16) of every tile with its own running max, sum and
//   output; after the last tile the four waves' (m, l, O) are merged through
//   LDS in wave order.
// Either way a wave's step on 16 queries x 16 keys is soa_ops.hip's: lane l =
// (lq = l & 15, lg = l >> 4); v_mfma_f32_16x16x4_f32 with A[row lq][k lg],
// B[k lg][col lq], D[row 4 lg + reg][col lq].
//  scores S^T = K . Q^T: A = the K tile (row = key, one 16-B LDS read per 16
//   channels), B = the wave's Q fragments (registers, loaded once); four
//   accumulators, one per 4-channel phase, added in a fixed order.  Lane
//   (lq, lg) ends with S[query lq][key 4 lg + reg].
//  softmax step: online_softmax_step (a wave only enters a tile whose first
//   key is < nk).
//  O^T += V^T . P^T: A = the V tile read at [key 4 lg + r][channel 16 j + lq],
//   B = p[r] as it sits in the lane; D: lane (lq, lg) holds O[query lq]
//   [channel 16 j + 4 lg + reg].
// A query's arithmetic does not depend on its image, head, tile or wave, nor on
// the strides: the same bits from dense or stacked buffers, alone or in a batch.
template <bool KSPLIT>
__global__ __launch_bounds__(kHdWaves * 64) void attention_hd128_kernel(
    const float* __restrict__ q, long long ldq, const float* __restrict__ k, long long ldk, const float* __restrict__ v,
    long long ldv, int nq, int nk, int heads, int qblocks, float scale, float* __restrict__ out) {
  constexpr int NJ = kHdDim / 16, R = KSPLIT ? 64 : 16, NI = R * (kHdDim / 4) / (kHdWaves * 64);
  extern __shared__ __attribute__((aligned(16))) float hd_lds[];
  float* Ks = hd_lds;
  float* Vs = Ks + R * kHdLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int qb = blockIdx.x % qblocks;
  const int ih = blockIdx.x / qblocks;
  const int head = ih % heads, img = ih / heads;
  const int q0 = KSPLIT ? qb * 16 : qb * 64 + wave * 16;  // the wave's first query
  const int qi = q0 + lq;
  const bool qok = qi < nq;  // a query past nq computes on zeros and is not stored

  f32x4 qf[NJ], o[NJ];
  {
    const float* qp = q + ((long long)img * nq + (qok ? qi : 0)) * ldq + head * kHdDim + 4 * lg;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(qp + 16 * j);
      qf[j] = qok ? t : f32x4{0.f, 0.f, 0.f, 0.f};
      o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  float m = -__builtin_inff(), l = 0.f;
  const float* kb = k + (long long)img * nk * ldk + head * kHdDim;
  const float* vb = v + (long long)img * nk * ldv + head * kHdDim;
  const int ntiles = (nk + R - 1) / R;
  // A tile's K and V rows (zero past nk) travel global -> registers -> LDS,
  // thread t taking 16-B group t + 256 i of the tile's R x 32; the next tile's
  // loads are issued before this tile's arithmetic.
  f32x4 kv[NI], vv[NI];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int idx = tid + i * (kHdWaves * 64);
      const int row = idx >> 5, c4 = idx & 31;
      const int key = kt * R + row;
      kv[i] = vv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (key < nk) {
        kv[i] = *reinterpret_cast<const f32x4*>(kb + (long long)key * ldk + c4 * 4);
        vv[i] = *reinterpret_cast<const f32x4*>(vb + (long long)key * ldv + c4 * 4);
      }
    }
  };
  load_tile(0);
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();  // the previous tile's readers are done
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int idx = tid + i * (kHdWaves * 64);
      const int row = idx >> 5, c4 = idx & 31;
      *reinterpret_cast<f32x4*>(Ks + row * kHdLd + c4 * 4) = kv[i];
      *reinterpret_cast<f32x4*>(Vs + row * kHdLd + c4 * 4) = vv[i];
    }
    if (kt + 1 < ntiles) load_tile(kt + 1);
    __syncthreads();

    const int r0 = KSPLIT ? wave * 16 : 0;  // the wave's 16 keys inside the tile
    const int key0 = kt * R + r0;
    if (key0 >= nk || q0 >= nq) continue;  // wave-uniform: nothing of this tile is this wave's
    const float* Kw = Ks + r0 * kHdLd;
    const float* Vw = Vs + r0 * kHdLd;

    f32x4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const f32x4 kf = *reinterpret_cast<const f32x4*>(Kw + lq * kHdLd + 16 * j + 4 * lg);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], qf[j][e], acc[e], 0, 0, 0);
    }
    const SoftmaxTile st = online_softmax_step((acc[0] + acc[1]) + (acc[2] + acc[3]), key0, nk, scale, lg, m, l);
    const f32x4 p = st.p;
    const float alpha = st.alpha;
    l = st.l;
    m = st.m;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      o[j] *= alpha;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(Vw[(4 * lg + r) * kHdLd + 16 * j + lq], p[r], o[j], 0, 0, 0);
    }
  }

  if (KSPLIT) {
    // merge the four key streams in wave order.  Wave 0 saw key 0, so its m is
    // finite and so is the merged max M; a wave that saw no tile has m = -inf,
    // l = 0, O = 0 and weight exp(-inf - M) = 0.
    float* Ml = hd_lds;                                // [3][2][64]
    float* Ol = hd_lds + (kHdWaves - 1) * 2 * 64;      // [3][NJ][64] float4
    __syncthreads();  // every wave is done with the last tile
    if (wave > 0) {
      Ml[((wave - 1) * 2 + 0) * 64 + lane] = m;
      Ml[((wave - 1) * 2 + 1) * 64 + lane] = l;
#pragma unroll
      for (int j = 0; j < NJ; ++j) *reinterpret_cast<f32x4*>(Ol + (((wave - 1) * NJ + j) * 64 + lane) * 4) = o[j];
    }
    __syncthreads();
    if (wave > 0) return;
    float M = m;
#pragma unroll
    for (int w = 0; w < kHdWaves - 1; ++w) M = fmaxf(M, Ml[(w * 2 + 0) * 64 + lane]);
    const float f0 = expf(m - M);
    l *= f0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) o[j] *= f0;
#pragma unroll
    for (int w = 0; w < kHdWaves - 1; ++w) {
      const float fw = expf(Ml[(w * 2 + 0) * 64 + lane] - M);
      l += Ml[(w * 2 + 1) * 64 + lane] * fw;
#pragma unroll
      for (int j = 0; j < NJ; ++j) o[j] += *reinterpret_cast<const f32x4*>(Ol + ((w * NJ + j) * 64 + lane) * 4) * fw;
    }
  }
  if (qok) {
    float* op = out + ((long long)img * nq + qi) * ((long long)heads * kHdDim) + head * kHdDim + 4 * lg;
#pragma unroll
    for (int j = 0; j < NJ; ++j) *reinterpret_cast<f32x4*>(op + 16 * j) = o[j] / l;
  }
}

template <bool KSPLIT>
static hipError_t launch_hd128(const float* q, long long ldq, const float* k, long long ldk, const float* v,
                               long long ldv, int nq, int nk, int heads, int qblocks, float scale, float* out,
                               unsigned blocks, hipStream_t s) {
  const size_t lds = (size_t)2 * (KSPLIT ? 64 : 16) * kHdLd * sizeof(float);
  return launch_dyn_lds(attention_hd128_kernel<KSPLIT>, blocks, kHdWaves * 64, lds, s, q, ldq, k, ldk, v, ldv, nq, nk,
                        heads, qblocks, scale, out);
}

// ---- rr_token_pool --------------------------------------------------------
constexpr int kTokWaves = 4;            // waves per workgroup (256 threads)
constexpr int kTokMaxObj = 8;           // most object queries
constexpr int kTokMinPixels = 16;       // fewest positions a workgroup takes when an image is split
constexpr int kTokTargetBlocks = 1024;  // workgroups wanted before images stop being split

// One wave owns a position's row of C = 256 NV channels as rr_dolg_local_pool
// does: lane l holds channels 256 j + 4 l .. + 3 (j < NV).  The n_obj query
// rows sit in LDS.  From the row in registers: the n_obj logits (wave_sum, a
// fixed order), their softmax over the objects with the max subtracted, and
// weight_o * row into the lane's accumulators of object o.  Workgroup
// blockIdx.x = image * splits + s takes positions [s chunk, (s + 1) chunk),
// wave w of it every kTokWaves-th position; the waves' accumulators are added
// through LDS in wave order.  splits == 1: dst is out[image]; otherwise
// part[image][s] (at most kTokTargetBlocks slabs of n_obj c floats, 32 MiB),
// which slab_sum_kernel<false> adds in a fixed order.
template <int NV>
__global__ __launch_bounds__(kTokWaves * 64) void token_pool_kernel(const float* __restrict__ x, int hw, int chunk,
                                                                    int splits, const float* __restrict__ query,
                                                                    int n_obj, float* __restrict__ dst) {
  constexpr int C = NV * 256;
  extern __shared__ __attribute__((aligned(16))) float tok_lds[];  // [n_obj][C]: the queries, then the reduction slab
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x / splits, s = blockIdx.x - img * splits;
  const int p0 = s * chunk;
  const int p1 = p0 + chunk < hw ? p0 + chunk : hw;
  const float* xi = x + (long long)img * hw * C + lane * 4;

  for (int i = tid; i < n_obj * (C / 4); i += kTokWaves * 64)
    *reinterpret_cast<f32x4*>(tok_lds + i * 4) = *reinterpret_cast<const f32x4*>(query + i * 4);
  __syncthreads();

  f32x4 acc[kTokMaxObj][NV], cur[NV], nxt[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    cur[j] = nxt[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ob = 0; ob < kTokMaxObj; ++ob) acc[ob][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int p = p0 + wave;  // wave-uniform
  if (p < p1) {
#pragma unroll
    for (int j = 0; j < NV; ++j) cur[j] = *reinterpret_cast<const f32x4*>(xi + (long long)p * C + j * 256);
  }
  for (; p < p1; p += kTokWaves) {
    const int pn = p + kTokWaves;
    if (pn < p1) {  // the next row's loads fly under this row's arithmetic
#pragma unroll
      for (int j = 0; j < NV; ++j) nxt[j] = *reinterpret_cast<const f32x4*>(xi + (long long)pn * C + j * 256);
    }
    float lg[kTokMaxObj];
    float mx = -__builtin_inff();
#pragma unroll
    for (int ob = 0; ob < kTokMaxObj; ++ob) {
      lg[ob] = -__builtin_inff();
      if (ob < n_obj) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const f32x4 qv = *reinterpret_cast<const f32x4*>(tok_lds + ob * C + j * 256 + lane * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) d = fmaf(qv[e], cur[j][e], d);
        }
        lg[ob] = wave_sum(d);
        mx = fmaxf(mx, lg[ob]);
      }
    }
    float den = 0.f;
#pragma unroll
    for (int ob = 0; ob < kTokMaxObj; ++ob) {
      lg[ob] = ob < n_obj ? expf(lg[ob] - mx) : 0.f;
      den += lg[ob];
    }
#pragma unroll
    for (int ob = 0; ob < kTokMaxObj; ++ob) {
      if (ob < n_obj) {
        const float wgt = lg[ob] / den;
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[ob][j] += wgt * cur[j];
      }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) cur[j] = nxt[j];
  }

  // waves 1..3 hand their sums to wave 0 through the one slab, in wave order
  for (int w = 1; w < kTokWaves; ++w) {
    __syncthreads();  // the queries (w == 1) or wave w - 1's slab have been read
    if (wave == w) {
#pragma unroll
      for (int ob = 0; ob < kTokMaxObj; ++ob)
        if (ob < n_obj) {
#pragma unroll
          for (int j = 0; j < NV; ++j) *reinterpret_cast<f32x4*>(tok_lds + ob * C + j * 256 + lane * 4) = acc[ob][j];
        }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int ob = 0; ob < kTokMaxObj; ++ob)
        if (ob < n_obj) {
#pragma unroll
          for (int j = 0; j < NV; ++j)
            acc[ob][j] += *reinterpret_cast<const f32x4*>(tok_lds + ob * C + j * 256 + lane * 4);
        }
    }
  }
  if (wave == 0) {
    float* o = dst + (long long)blockIdx.x * n_obj * C + lane * 4;  // out[img] (splits == 1) or part[img][s]
#pragma unroll
    for (int ob = 0; ob < kTokMaxObj; ++ob)
      if (ob < n_obj) {
#pragma unroll
        for (int j = 0; j < NV; ++j) *reinterpret_cast<f32x4*>(o + ob * C + j * 256) = acc[ob][j];
      }
  }
}

template <int NV>
static void launch_token_pool(const float* x, int hw, int chunk, int splits, const float* query, int n_obj, float* dst,
                              unsigned blocks, hipStream_t s) {
  const size_t lds = (size_t)n_obj * NV * 256 * sizeof(float);
  hipLaunchKernelGGL(token_pool_kernel<NV>, dim3(blocks), dim3(kTokWaves * 64), lds, s, x, hw, chunk, splits, query, n_obj,
                     dst);
}

// ---- rr_gelu --------------------------------------------------------------
__global__ __launch_bounds__(256) void gelu_kernel(const float* x, long long n, float* y) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const float t = x[i];
    // -inf: the limit x Phi(x) -> -0 (the product form alone would give inf . 0 = NaN)
    y[i] = t == -__builtin_inff() ? -0.f : 0.5f * t * (1.f + erff(t * 0.70710678118654752440f));
  }
}

}  // namespace rr

using namespace rr;

extern "C" int rr_attention_hd128(rr_handle_t h, const float* q, long long ldq, const float* k, long long ldk,
                                  const float* v, long long ldv, int b, int nq, int nk, int heads, float* out,
                                  void* stream) {
  RR_ENTRY(h);
  const long long w = (long long)heads * kHdDim;
  if (!q || !k || !v || !out || b < 0 || nq < 1 || nq > 65535 || nk < 1 || nk > 65535 || heads < 1 || ldq < w ||
      ldk < w || ldv < w || (ldq & 3) || (ldk & 3) || (ldv & 3) || ((uintptr_t)q & 15) || ((uintptr_t)k & 15) ||
      ((uintptr_t)v & 15) || ((uintptr_t)out & 15))
    return set_error(h, RR_EINVAL,
                     "rr_attention_hd128: bad argument (1 <= nq, nk <= 65535, heads >= 1, ld >= 128 heads, ld % 4 == 0, "
                     "16-B aligned)");
  if (b == 0) return RR_OK;
  const bool ksplit = nq <= 16;
  const int qblocks = ksplit ? 1 : (nq + 63) / 64;
  const long long blocks = (long long)b * heads * qblocks;
  if (blocks > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_attention_hd128: too many images x heads");
  // torch multiplies the fp32 scores by the Python float 128 ** -0.5 rounded to fp32 (:99, :123)
  const float scale = (float)std::pow((double)kHdDim, -0.5);
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch tl(h, kTimeAttn, s);
  hipError_t e = ksplit ? launch_hd128<true>(q, ldq, k, ldk, v, ldv, nq, nk, heads, qblocks, scale, out, (unsigned)blocks, s)
                        : launch_hd128<false>(q, ldq, k, ldk, v, ldv, nq, nk, heads, qblocks, scale, out, (unsigned)blocks, s);
  return check_hip(h, e, "attention_hd128 launch");
}

extern "C" int rr_token_pool(rr_handle_t h, const float* x, int b, int hw, int c, const float* query, int n_obj,
                             float* out, void* stream) {
  RR_ENTRY(h);
  if (!x || !query || !out || b < 0 || hw < 1 || c < 256 || c > 1024 || (c & 255) || n_obj < 1 || n_obj > kTokMaxObj ||
      ((uintptr_t)x & 15) || ((uintptr_t)query & 15) || ((uintptr_t)out & 15))
    return set_error(h, RR_EINVAL,
                     "rr_token_pool: bad argument (c % 256 == 0, 256 <= c <= 1024, 1 <= n_obj <= 8, hw >= 1, 16-B aligned)");
  if (b == 0) return RR_OK;
  const auto [splits, chunk] = split_positions(b, hw, kTokMinPixels, kTokTargetBlocks);
  const long long blocks = (long long)b * splits;
  const long long len = (long long)n_obj * c;
  if (blocks > 0x7fffffffLL || (long long)b * (len >> 8) > 0x7fffffffLL)
    return set_error(h, RR_EINVAL, "rr_token_pool: too many images");
  hipStream_t s = (hipStream_t)stream;
  float* dst = out;
  if (splits > 1) {
    void* p = nullptr;
    if (int rc = stream_scratch(h, s, (size_t)blocks * len * sizeof(float), &p, "rr_token_pool")) return rc;
    dst = (float*)p;
  }
  TimedLaunch tl(h, kTimeElem, s);
  switch (c >> 8) {
    case 1: launch_token_pool<1>(x, hw, chunk, splits, query, n_obj, dst, (unsigned)blocks, s); break;
    case 2: launch_token_pool<2>(x, hw, chunk, splits, query, n_obj, dst, (unsigned)blocks, s); break;
    case 3: launch_token_pool<3>(x, hw, chunk, splits, query, n_obj, dst, (unsigned)blocks, s); break;
    default: launch_token_pool<4>(x, hw, chunk, splits, query, n_obj, dst, (unsigned)blocks, s); break;
  }
  if (int rc = check_hip(h, hipGetLastError(), "token_pool launch")) return rc;
  if (splits > 1)
    return check_hip(h, launch_slab_sum<false>(dst, b, splits, (int)len, hw, out, s), "token_pool_sum launch");
  return RR_OK;
}

extern "C" int rr_gelu(rr_handle_t h, const float* x, long long n, float* y, void* stream) {
  RR_ENTRY(h);
  if (!x || !y || n < 0) return set_error(h, RR_EINVAL, "rr_gelu: bad argument");
  if (n == 0) return RR_OK;
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch tl(h, kTimeElem, s);
  long long blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, n, y);
  return check_hip(h, hipGetLastError(), "gelu launch");
}
