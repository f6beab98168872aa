// sos_ops.hip — the SoSNet head's kernels (gfx950): the attention-weighted,
// centred covariance of the projected rows as its packed upper triangle, and
// the split-K form of the skinny linear that follows it (rr_linear_splitk; with a
// residual, rr_linear_splitk_ex, for the token aggregator's folded last layer).
//
// Reference (models/sosnet.py): SimilarityAttention.forward :76-92 (the last
// Linear + Sigmoid and the multiply), SecondOrderPooling.forward :27-55 (mean,
// centring, bmm / (N - 1), triu_indices gather, F.normalize) and feature_proj's
// first Linear(c (c + 1) / 2, 2048) + ReLU (:131-136).
#include <cmath>

#include "heads_common.hpp"

namespace rr {

constexpr int kSosThreads = 256;      // 4 waves per workgroup
constexpr int kSosTile = 64;          // channels per covariance tile side
constexpr int kSosStep = 32;          // positions per step
constexpr int kSosLd = kSosTile + 16; // Ys row stride: rows 4 apart land 16 banks apart (4-B reads conflict-free)
constexpr int kSosTs = kSosTile + 1;  // staged output tile row stride
constexpr int kSosMinPos = 64;        // fewest positions a workgroup takes when an image is split
constexpr int kSosTargetBlocks = 64;  // split images while b is below this
constexpr float kSosEps = 1e-12f;     // F.normalize's eps (:53)

// a_p = sigmoid(w3 . hid_p + b3), one wave per position (hid == nullptr: 1).
__global__ __launch_bounds__(kSosThreads) void sos_att_kernel(const float* __restrict__ hid, int dh,
                                                              const float* __restrict__ w3, float b3,
                                                              long long rows, float* __restrict__ att,
                                                              float* __restrict__ att_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long p = (long long)blockIdx.x * (kSosThreads / 64) + wave;
  if (p >= rows) return;  // wave-uniform
  float a = 1.f;
  if (hid != nullptr) {
    const int d4 = dh >> 2;
    float s = 0.f;
    for (int f = lane; f < d4; f += 64) {
      const f32x4 hv = *reinterpret_cast<const f32x4*>(hid + p * dh + f * 4);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w3 + f * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(hv[e], wv[e], s);
    }
    s = wave_sum(s) + b3;
    a = 1.f / (1.f + expf(-s));
  }
  if (lane == 0) {
    att[p] = a;
    if (att_out != nullptr) att_out[p] = a;
  }
}

// mean[img][ch] = (1 / n) sum_p a_p z_p[ch]: workgroup (image, 64 channels),
// thread (16-B group c4, position group pg of 16) adds positions pg, pg + 16,
// ... in that order, then the 16 partial sums are added through LDS in order.
__global__ __launch_bounds__(kSosThreads) void sos_mean_kernel(const float* __restrict__ z, int n, int c,
                                                               const float* __restrict__ att,
                                                               float* __restrict__ mean) {
  __shared__ __attribute__((aligned(16))) float red[16 * kSosTile];
  const int groups = (c + kSosTile - 1) / kSosTile;
  const int img = blockIdx.x / groups, g = blockIdx.x - img * groups;
  const int tid = threadIdx.x, c4 = tid & 15, pg = tid >> 4;
  const int ch = g * kSosTile + c4 * 4;
  const float* zi = z + (long long)img * n * c;
  const float* ai = att + (long long)img * n;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (ch < c) {
#pragma unroll 4
    for (int p = pg; p < n; p += 16) {
      const float a = ai[p];
      const f32x4 v = *reinterpret_cast<const f32x4*>(zi + (long long)p * c + ch);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = fmaf(a, v[e], s[e]);
    }
  }
  *reinterpret_cast<f32x4*>(red + pg * kSosTile + c4 * 4) = s;
  __syncthreads();
  if (tid < kSosTile && g * kSosTile + tid < c) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += red[i * kSosTile + tid];
    mean[(long long)img * c + g * kSosTile + tid] = t / (float)n;
  }
}

// tile pair index -> (ti, tj), ti <= tj, row-major over the upper triangle
__device__ __forceinline__ void sos_pair(int pair, int nt, int& ti, int& tj) {
  ti = 0;
  while (pair >= nt - ti) {
    pair -= nt - ti;
    ++ti;
  }
  tj = ti + pair;
}

// The staged 64 x 64 tile of sums Ts -> cov = sum / (n - 1) at its place in the
// image's packed triangle (4-B stores, lanes along a row: a packed row starts
// at any 4-B offset), and the tile's sum of squares to ssq (threads' values in
// element order, the wave sums of wave_sum, the four waves in order).
__device__ __forceinline__ void sos_emit_tile(const float* Ts, float* red, int ti, int tj, int c, int n,
                                              float* __restrict__ orow, float* __restrict__ ssq) {
  const int tid = threadIdx.x;
  const float den = (float)(n - 1);
  float ss = 0.f;
#pragma unroll 4
  for (int e = tid; e < kSosTile * kSosTile; e += kSosThreads) {
    const int r = e >> 6, cc = e & 63;
    const int gi = ti * kSosTile + r, gj = tj * kSosTile + cc;
    if (gi < c && gj < c && gj >= gi) {
      const float v = Ts[r * kSosTs + cc] / den;
      const long long off = (long long)gi * c - ((long long)gi * (gi - 1)) / 2 + (gj - gi);
      orow[off] = v;
      ss = fmaf(v, v, ss);
    }
  }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  if (tid == 0) *ssq = ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup = (image, tile pair ti <= tj, chunk of the image's positions).
// A step takes 32 positions: the rows' two 64-channel slices travel global ->
// registers (issued one step ahead) -> y = a_p z_p - mean (0 past the chunk and
// past channel c) -> Ya / Yb; then sum_p y_p[i] y_p[j] on
// v_mfma_f32_16x16x4_f32, wave (wi, wj) owning the 32 x 32 quadrant of the tile
// (a diagonal tile's quadrant below the diagonal is skipped).  The tile is
// staged in LDS and either emitted (splits == 1) or stored whole to part for
// the fixed-order adding of sos_reduce_kernel.
__global__ __launch_bounds__(kSosThreads) void sos_cov_kernel(const float* __restrict__ z, int n, int c, int chunk,
                                                              int splits, const float* __restrict__ att,
                                                              const float* __restrict__ mean,
                                                              float* __restrict__ part, float* __restrict__ out,
                                                              float* __restrict__ ssq) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kSosStep * kSosLd];
  __shared__ float red[4];
  static_assert(kSosTile * kSosTs <= 2 * kSosStep * kSosLd, "the staged tile reuses the step buffers");
  float* Ya = lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int nt = (c + kSosTile - 1) / kSosTile, pairs = nt * (nt + 1) / 2;
  const int sp = blockIdx.x % splits;
  const int ip = blockIdx.x / splits;
  const int img = ip / pairs, pair = ip - img * pairs;
  int ti, tj;
  sos_pair(pair, nt, ti, tj);
  const bool diag = ti == tj;
  float* Yb = diag ? Ya : lds + kSosStep * kSosLd;
  const int p0 = sp * chunk;
  const int p1 = p0 + chunk < n ? p0 + chunk : n;
  const int steps = (p1 - p0 + kSosStep - 1) / kSosStep;
  const float* zi = z + (long long)img * n * c;
  const float* ai = att + (long long)img * n;

  // the thread's two rows of a step (row0, row0 + 16) and its 16-B column
  const int c4 = tid & 15, row0 = tid >> 4;
  const int cha = ti * kSosTile + c4 * 4, chb = tj * kSosTile + c4 * 4;
  const bool oka = cha < c, okb = chb < c && !diag;
  f32x4 ma = f32x4{0.f, 0.f, 0.f, 0.f}, mb = ma;
  if (oka) ma = *reinterpret_cast<const f32x4*>(mean + (long long)img * c + cha);
  if (okb) mb = *reinterpret_cast<const f32x4*>(mean + (long long)img * c + chb);

  f32x4 ra[2], rb[2];
  float av[2];
  auto load_step = [&](int st) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = p0 + st * kSosStep + row0 + 16 * i;
      ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      rb[i] = ra[i];
      av[i] = 0.f;
      if (p < p1) {
        av[i] = ai[p];
        if (oka) ra[i] = *reinterpret_cast<const f32x4*>(zi + (long long)p * c + cha);
        if (okb) rb[i] = *reinterpret_cast<const f32x4*>(zi + (long long)p * c + chb);
      }
    }
  };
  load_step(0);

  const int wi = wave & 1, wj = wave >> 1;
  const bool skip = diag && wi > wj;  // wave-uniform: the quadrant lies below the diagonal
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int st = 0; st < steps; ++st) {
    __syncthreads();  // the previous step's readers are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = p0 + st * kSosStep + row0 + 16 * i;
      const bool live = p < p1;
      f32x4 ya = f32x4{0.f, 0.f, 0.f, 0.f}, yb = ya;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (live && oka) ya[e] = fmaf(av[i], ra[i][e], -ma[e]);
        if (live && okb) yb[e] = fmaf(av[i], rb[i][e], -mb[e]);
      }
      *reinterpret_cast<f32x4*>(Ya + (row0 + 16 * i) * kSosLd + c4 * 4) = ya;
      if (!diag) *reinterpret_cast<f32x4*>(Yb + (row0 + 16 * i) * kSosLd + c4 * 4) = yb;
    }
    if (st + 1 < steps) load_step(st + 1);
    __syncthreads();
    if (!skip) {
      const float* pa = Ya + lg * kSosLd + 32 * wi + lq;
      const float* pb = Yb + lg * kSosLd + 32 * wj + lq;
#pragma unroll
      for (int kk = 0; kk < kSosStep / 4; ++kk) {
        const float a0 = pa[4 * kk * kSosLd], a1 = pa[4 * kk * kSosLd + 16];
        const float b0 = pb[4 * kk * kSosLd], b1 = pb[4 * kk * kSosLd + 16];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }

  // stage the tile: lane (lq, lg) holds rows 4 lg + r, column lq of each 16 x 16
  __syncthreads();
  float* Ts = lds;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Ts[(32 * wi + 16 * i + 4 * lg + r) * kSosTs + 32 * wj + 16 * j + lq] = skip ? 0.f : acc[i][j][r];
  __syncthreads();
  if (splits == 1) {
    const long long tri = (long long)c * (c + 1) / 2;
    sos_emit_tile(Ts, red, ti, tj, c, n, out + (long long)img * tri, ssq + ip);
  } else {
    float* dst = part + (long long)blockIdx.x * (kSosTile * kSosTile);
#pragma unroll 4
    for (int e = tid; e < kSosTile * kSosTile; e += kSosThreads) dst[e] = Ts[(e >> 6) * kSosTs + (e & 63)];
  }
}

// A split image's tile: the chunks' partial tiles added in index order, then
// emitted as sos_cov_kernel emits an unsplit one.  One workgroup per (image,
// tile pair).
__global__ __launch_bounds__(kSosThreads) void sos_reduce_kernel(const float* __restrict__ part, int splits, int n,
                                                                 int c, float* __restrict__ out,
                                                                 float* __restrict__ ssq) {
  __shared__ float Ts[kSosTile * kSosTs];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int nt = (c + kSosTile - 1) / kSosTile, pairs = nt * (nt + 1) / 2;
  const int img = blockIdx.x / pairs, pair = blockIdx.x - img * pairs;
  int ti, tj;
  sos_pair(pair, nt, ti, tj);
  const float* pp = part + (long long)blockIdx.x * splits * (kSosTile * kSosTile);
  for (int e = tid; e < kSosTile * kSosTile; e += kSosThreads) {
    float t = 0.f;
#pragma unroll 4
    for (int s = 0; s < splits; ++s) t += pp[(long long)s * (kSosTile * kSosTile) + e];
    Ts[(e >> 6) * kSosTs + (e & 63)] = t;
  }
  __syncthreads();
  const long long tri = (long long)c * (c + 1) / 2;
  sos_emit_tile(Ts, red, ti, tj, c, n, out + (long long)img * tri, ssq + blockIdx.x);
}

// inv_norm[img] = 1 / max(sqrt(sum of the image's tiles' sums of squares, in
// tile order), 1e-12), one thread per image
__global__ __launch_bounds__(256) void sos_inv_norm_kernel(const float* __restrict__ ssq, int b, int pairs,
                                                           float* __restrict__ inv_norm) {
  const int img = blockIdx.x * 256 + threadIdx.x;
  if (img >= b) return;
  float s = 0.f;
  for (int i = 0; i < pairs; ++i) s += ssq[(long long)img * pairs + i];
  inv_norm[img] = 1.f / fmaxf(sqrtf(s), kSosEps);
}

// y[i][j] = act(row_scale[i] * sum_s part[i][s][j] + bias[j] + residual[i][j]),
// the slices added in index order; one thread per output
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int splits, int n,
                                                            long long total, const float* __restrict__ row_scale,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ residual, int act,
                                                            float* __restrict__ y) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long long i = e / n;
  const int j = (int)(e - i * n);
  const float* pp = part + i * splits * n + j;
  float t = 0.f;
#pragma unroll 4
  for (int s = 0; s < splits; ++s) t += pp[(long long)s * n];
  if (row_scale != nullptr) t *= row_scale[i];
  if (bias != nullptr) t += bias[j];
  if (residual != nullptr) t += residual[e];
  if (act == 1) t = fmaxf(t, 0.f);
  else if (act == 2) t = t / (1.f + expf(-1.702f * t));  // QuickGELU, x sigmoid(1.702 x)
  y[e] = t;
}

// The k-slices of rr_linear_splitk: enough (row tile, column tile, slice)
// workgroups of the fp32 core's 128 x 128 tile for four per compute unit, each
// slice at least 512 deep and a multiple of 32 (the core's k-tile); a function
// of (m, k, n) and the CU count only.
struct SplitKPlan {
  int splits, k_split;
};
inline SplitKPlan splitk_plan(int m, int k, int n, int n_cu) {
  const long long tiles = (long long)((m + 127) / 128) * ((n + 127) / 128);
  long long want = (4LL * n_cu + tiles - 1) / tiles;
  const long long most = (k + 511) / 512;
  if (want > most) want = most;
  if (want < 1) want = 1;
  const int k_split = (int)(((k + want - 1) / want + 31) / 32 * 32);
  return {(k + k_split - 1) / k_split, k_split};
}

}  // namespace rr

using namespace rr;

extern "C" int rr_sos_cov(rr_handle_t h, const float* z, int b, int n, int c, const float* hid, int dh,
                          const float* w3, float b3, float* att_out, float* out, float* inv_norm, void* stream) {
  RR_ENTRY(h);
  bool bad = !z || !out || !inv_norm || b < 0 || n < 2 || n > 65535 || c < 32 || c > 512 || (c & 31) ||
             ((uintptr_t)z & 15) || ((uintptr_t)out & 15) || ((uintptr_t)inv_norm & 15) || ((uintptr_t)att_out & 15);
  if (hid != nullptr)
    bad = bad || !w3 || dh < 4 || dh > 512 || (dh & 3) || ((uintptr_t)hid & 15) || ((uintptr_t)w3 & 15);
  if (bad)
    return set_error(h, RR_EINVAL,
                     "rr_sos_cov: bad argument (c % 32 == 0, 32 <= c <= 512, dh % 4 == 0, 4 <= dh <= 512, 2 <= n <= "
                     "65535, 16-B aligned)");
  if (b == 0) return RR_OK;
  const auto [splits, chunk] = split_positions(b, n, kSosMinPos, kSosTargetBlocks);
  const int nt = (c + kSosTile - 1) / kSosTile, pairs = nt * (nt + 1) / 2;
  const long long rows = (long long)b * n;
  const long long tiles = (long long)b * pairs;
  const long long blocks = tiles * splits;
  if (blocks > 0x7fffffffLL || (rows + 3) / 4 > 0x7fffffffLL)
    return set_error(h, RR_EINVAL, "rr_sos_cov: too many images");
  hipStream_t s = (hipStream_t)stream;
  // scratch: att [b n], mean [b c], ssq [b pairs], then the split images' partial tiles
  auto al = [](size_t v) { return (v + 63) & ~(size_t)63; };  // in floats: 256-B sections
  const size_t off_mean = al((size_t)rows);
  const size_t off_ssq = off_mean + al((size_t)b * c);
  const size_t off_part = off_ssq + al((size_t)tiles);
  const size_t total = off_part + (splits > 1 ? (size_t)blocks * kSosTile * kSosTile : 0);
  void* p = nullptr;
  if (int rc = stream_scratch(h, s, total * sizeof(float), &p, "rr_sos_cov")) return rc;
  float* att = (float*)p;
  float* mean = att + off_mean;
  float* ssq = att + off_ssq;
  float* part = att + off_part;
  TimedLaunch tl(h, kTimeElem, s);
  hipLaunchKernelGGL(sos_att_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(kSosThreads), 0, s, hid, dh, w3, b3, rows,
                     att, att_out);
  hipLaunchKernelGGL(sos_mean_kernel, dim3((unsigned)(b * nt)), dim3(kSosThreads), 0, s, z, n, c, att, mean);
  hipLaunchKernelGGL(sos_cov_kernel, dim3((unsigned)blocks), dim3(kSosThreads), 0, s, z, n, c, chunk, splits, att,
                     mean, part, out, ssq);
  if (splits > 1)
    hipLaunchKernelGGL(sos_reduce_kernel, dim3((unsigned)tiles), dim3(kSosThreads), 0, s, part, splits, n, c, out,
                       ssq);
  hipLaunchKernelGGL(sos_inv_norm_kernel, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, s, ssq, b, pairs,
                     inv_norm);
  return check_hip(h, hipGetLastError(), "sos_cov launch");
}

// rr_linear_splitk and rr_linear_splitk_ex (residual == nullptr: the former)
static int linear_splitk(rr_handle_t h, const char* who, const float* x, int m, int k, const float* w, int n,
                         const float* row_scale, const float* bias, const float* residual, int act, float* y,
                         void* stream) {
  if (!x || !w || !y || m < 0 || k <= 0 || n <= 0 || (k & 3) || act < 0 || act > 2)
    return set_error(h, RR_EINVAL, std::string(who) + ": bad argument (k % 4 == 0, act 0, 1 or 2)");
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 15))
    return set_error(h, RR_EINVAL, std::string(who) + ": x/w must be 16-byte aligned");
  if (m == 0) return RR_OK;
  const auto [splits, k_split] = splitk_plan(m, k, n, device_cu_count(h));
  const long long total = (long long)m * n;
  if ((total + 255) / 256 > 0x7fffffffLL) return set_error(h, RR_EINVAL, std::string(who) + ": too many outputs");
  hipStream_t s = (hipStream_t)stream;
  void* p = nullptr;
  if (int rc = stream_scratch(h, s, (size_t)total * splits * sizeof(float), &p, who)) return rc;
  GemmArgs g;
  g.A = x;
  g.lda = k;
  g.M = m;
  g.K = k;
  g.B = w;
  g.ldb = k;
  g.N = n;
  g.C = (float*)p;
  g.ldc = (long long)splits * n;
  g.k_split = k_split;
  g.c_split_stride = n;
  if (int rc = launch_gemm(h, A_DENSE, E_STORE, g, s, kTimeGemm)) return rc;
  TimedLaunch tl(h, kTimeGemm, s);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)p,
                     splits, n, total, row_scale, bias, residual, act, y);
  return check_hip(h, hipGetLastError(), "splitk_reduce launch");
}

extern "C" int rr_linear_splitk(rr_handle_t h, const float* x, int m, int k, const float* w, int n,
                                const float* row_scale, const float* bias, int act, float* y, void* stream) {
  RR_ENTRY(h);
  return linear_splitk(h, "rr_linear_splitk", x, m, k, w, n, row_scale, bias, nullptr, act, y, stream);
}

extern "C" int rr_linear_splitk_ex(rr_handle_t h, const float* x, int m, int k, const float* w, int n,
                                   const float* row_scale, const float* bias, const float* residual, int act,
                                   float* y, void* stream) {
  RR_ENTRY(h);
  return linear_splitk(h, "rr_linear_splitk_ex", x, m, k, w, n, row_scale, bias, residual, act, y, stream);
}
