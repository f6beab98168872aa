// how_ops.hip — the HOW head's aggregation kernels (gfx950): VLAD pooling with
// a soft assignment and ASMK's thresholded nearest-centroid histogram, both
// from the raw local_proj rows.
//
// Reference (models/how_vlad.py): HOWModel.extract_local_descriptors :162
// (F.normalize over the descriptor), VLADPooling.forward :36-55 (cdist,
// softmax(-alpha dist), the loop over the centroids) and ASMKPooling.forward
// :80-99 (cdist, argmin, gather, mean + std threshold, the double loop).
#include <cmath>

#include "heads_common.hpp"

namespace rr {

constexpr int kHowWaves = 4;            // waves per workgroup (256 threads)
constexpr int kHowThreads = kHowWaves * 64;
constexpr int kHowMinPos = 64;          // fewest positions a workgroup takes when an image is split
constexpr int kHowTargetBlocks = 256;   // workgroups wanted before images stop being split
constexpr float kHowEps = 1e-12f;       // F.normalize's eps (:162)

// LDS layout in floats for k centroids padded to KT16 = 16 ceil(k / 16) rows of
// width d, and P positions per step:
//  Cs [KT16][d + 4]  the centroids (rows >= k zero)
//  cn [KT16]         their squared norms
//  Xs [P][d + 4]     the step's normalised descriptors (rows past the chunk zero)
//  xn [P]            their squared norms
//  As [P][KT16 + 4]  the step's x . c, then the assignment weights in place
//  sa [KT16]         sum over the workgroup's positions of the weights
// Rows of d + 4 and KT16 + 4 floats: 16-B reads by row and 4-B reads of rows
// four apart are both conflict-free (token_ops.hip's kHdLd).
struct HowLds {
  int ldc, lda, cs, cn, xs, xn, as, sa, total;
  __host__ __device__ HowLds(int kt16, int d, int p) {
    ldc = d + 4;
    lda = kt16 + 4;
    cs = 0;
    cn = cs + kt16 * ldc;
    xs = cn + kt16;
    xn = xs + p * ldc;
    as = xn + p;
    sa = as + p * lda;
    total = sa + kt16;
  }
};

__device__ __forceinline__ float how_group_sum(float v, int width) {
  // butterfly over `width` (8 or 16) neighbouring lanes: every lane of the
  // group ends with the same bits
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  if (width == 16) v += __shfl_xor(v, 8, 64);
  return v;
}

// One workgroup = (image, chunk of its positions).  KTMAX bounds the centroid
// tiles (k <= 16 KTMAX), NJ the 16-channel column tiles a wave owns (d <= 64 NJ).
// A step takes P = 32 positions (16 where the largest centroid table leaves LDS
// for no more):
//  0. the step's rows travel global -> registers (issued one step ahead) ->
//     x / max(||x||, 1e-12) -> Xs, with ||x^||^2 (TPP = 256 / P threads a row);
//  1. S = X^ . C^T on v_mfma_f32_16x16x4_f32, the (position tile, centroid
//     tile) pairs dealt over the waves; rows = centroids, columns = positions:
//     lane (lq, lg) ends with S[position lq][centroid 16 kt + 4 lg + reg] and
//     stores those four to As;
//  2. per position (TPP threads): dist = sqrt(max(||x^||^2 + ||c||^2 - 2 S, 0)),
//     VLAD: softmax over the centroids of -alpha dist with the max subtracted,
//     written over S (0 for rows past the chunk and columns >= k);
//     ASMK: the smallest dist and its lowest centroid index, to global memory;
//  3. VLAD: V += A^T . X^ on the same MFMA, wave w owning channel tiles w, w + 4,
//     ... of every centroid tile; the column sums of A ride along in the lanes.
// The epilogue subtracts (sum_n a[n][c]) c and stores the k x d block to dst
// (out[image], or part[image][split] for token_pool-style fixed-order adding).
// A position's arithmetic depends on neither its image nor its chunk.
template <int KTMAX, int NJ, bool ASMK>
__global__ __launch_bounds__(kHowThreads) void how_pool_kernel(const float* __restrict__ x, int n, int d, int chunk,
                                                                int splits, const float* __restrict__ cent, int k,
                                                                float alpha, float* __restrict__ dst,
                                                                int* __restrict__ dst_idx) {
  constexpr int P = (KTMAX == 8 && NJ == 4) ? 16 : 32;  // positions per step
  constexpr int NPT = P / 16;                            // position tiles per step
  constexpr int TPP = kHowThreads / P;                   // threads per position (phases 0 and 2)
  constexpr int NV = (NJ * 16 + TPP - 1) / TPP;          // 16-B groups of a row per thread
  constexpr int NC = (KTMAX * 16 + TPP - 1) / TPP;       // centroids per thread in phase 2
  extern __shared__ __attribute__((aligned(16))) float how_lds[];
  const int KT = (k + 15) >> 4, DT = d >> 4, d4 = d >> 2;
  const HowLds L(KT * 16, d, P);
  float* Cs = how_lds + L.cs;
  float* cn = how_lds + L.cn;
  float* Xs = how_lds + L.xs;
  float* xn = how_lds + L.xn;
  float* As = how_lds + L.as;
  float* sa = how_lds + L.sa;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int img = blockIdx.x / splits, sp = blockIdx.x - img * splits;
  const int p0 = sp * chunk;
  const int p1 = p0 + chunk < n ? p0 + chunk : n;
  const int steps = (p1 - p0 + P - 1) / P;
  const float* xi = x + (long long)img * n * d;
  const int prow = tid / TPP, psub = tid - prow * TPP;  // phases 0 and 2: the thread's row of the step

  f32x4 xr[NV];
  auto load_step = [&](int st) {
    const int p = p0 + st * P + prow;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = psub + i * TPP;
      xr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p < p1 && f < d4) xr[i] = *reinterpret_cast<const f32x4*>(xi + (long long)p * d + f * 4);
    }
  };
  load_step(0);

  // the centroids and their squared norms (two threads a centroid, halves
  // added in one order: identical centroids get identical norms)
  for (int i = tid; i < KT * 16 * d4; i += kHowThreads) {
    const int row = i / d4, c4 = i - row * d4;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row < k) v = *reinterpret_cast<const f32x4*>(cent + (long long)row * d + c4 * 4);
    *reinterpret_cast<f32x4*>(Cs + row * L.ldc + c4 * 4) = v;
  }
  __syncthreads();
  {
    const int c = tid >> 1, half = tid & 1, dh = d >> 1;
    float s = 0.f;
    if (c < KT * 16)
      for (int j = 0; j < dh; ++j) {
        const float v = Cs[c * L.ldc + half * dh + j];
        s = fmaf(v, v, s);
      }
    s += __shfl_xor(s, 1, 64);
    if (c < KT * 16 && half == 0) cn[c] = s;
  }

  f32x4 acc[KTMAX][NJ];
  float psum[KTMAX];
#pragma unroll
  for (int kt = 0; kt < KTMAX; ++kt) {
    psum[kt] = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[kt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int st = 0; st < steps; ++st) {
    __syncthreads();  // the previous step's readers of Xs and As are done (first step: cn is written)
    // ---- 0: normalise the step's rows into Xs
    {
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = fmaf(xr[i][e], xr[i][e], ss);
      ss = how_group_sum(ss, TPP);
      const float den = fmaxf(sqrtf(ss), kHowEps);
      float s2 = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int f = psub + i * TPP;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = xr[i][e] / den;
          s2 = fmaf(v[e], v[e], s2);
        }
        if (f < d4) *reinterpret_cast<f32x4*>(Xs + prow * L.ldc + f * 4) = v;
      }
      s2 = how_group_sum(s2, TPP);
      if (psub == 0) xn[prow] = s2;
    }
    if (st + 1 < steps) load_step(st + 1);
    __syncthreads();

    // ---- 1: S = X^ . C^T
    {
      const int pt = wave % NPT;
#pragma unroll
      for (int i = 0; i < (KTMAX * NPT + kHowWaves - 1) / kHowWaves; ++i) {
        const int kt = wave / NPT + i * (kHowWaves / NPT);
        if (kt < KT) {  // wave-uniform
          f32x4 a4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) a4[e] = f32x4{0.f, 0.f, 0.f, 0.f};
          const float* cp = Cs + (16 * kt + lq) * L.ldc + 4 * lg;
          const float* xp = Xs + (16 * pt + lq) * L.ldc + 4 * lg;
          for (int j = 0; j < DT; ++j) {
            const f32x4 cf = *reinterpret_cast<const f32x4*>(cp + 16 * j);
            const f32x4 xf = *reinterpret_cast<const f32x4*>(xp + 16 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) a4[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(cf[e], xf[e], a4[e], 0, 0, 0);
          }
          const f32x4 s = (a4[0] + a4[1]) + (a4[2] + a4[3]);
          *reinterpret_cast<f32x4*>(As + (16 * pt + lq) * L.lda + 16 * kt + 4 * lg) = s;
        }
      }
    }
    __syncthreads();

    // ---- 2: distances; the assignment (VLAD) or the nearest centroid (ASMK)
    {
      const int p = p0 + st * P + prow;
      const float xx = xn[prow];
      float* ar = As + prow * L.lda;
      float v[NC];
      float mx = -__builtin_inff();  // VLAD: the largest logit; ASMK: unused
      float best = __builtin_inff();
      int bi = 0x7fffffff;
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const int c = psub + i * TPP;
        v[i] = -__builtin_inff();
        if (c < k) {
          const float d2 = fmaxf(xx + cn[c] - 2.f * ar[c], 0.f);  // rounding may leave it below 0
          const float dist = sqrtf(d2);
          if (ASMK) {
            if (dist < best) {  // c ascends: the lowest index among the thread's equals
              best = dist;
              bi = c;
            }
          } else {
            v[i] = -alpha * dist;
            mx = fmaxf(mx, v[i]);
          }
        }
      }
      if (ASMK) {
#pragma unroll
        for (int o = 1; o < TPP; o <<= 1) {
          const float ob = __shfl_xor(best, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (ob < best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
          }
        }
        if (psub == 0 && p < p1) {
          dst[(long long)img * n + p] = best;
          dst_idx[(long long)img * n + p] = bi;
        }
      } else {
#pragma unroll
        for (int o = 1; o < TPP; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float den = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
          v[i] = expf(v[i] - mx);  // exp(-inf) = 0 for c >= k; mx is finite (k >= 1)
          den += v[i];
        }
        den = how_group_sum(den, TPP);
        const float keep = p < p1 ? 1.f : 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
          const int c = psub + i * TPP;
          if (c < KT * 16) ar[c] = keep * (v[i] / den);
        }
      }
    }
    if (ASMK) continue;
    __syncthreads();

    // ---- 3: V += A^T . X^ (rows = centroids, columns = channels, summed over positions)
    if (wave < DT) {
#pragma unroll
      for (int g = 0; g < NPT; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * g + 4 * lg + r;
          float av[KTMAX];
#pragma unroll
          for (int kt = 0; kt < KTMAX; ++kt) {
            av[kt] = kt < KT ? As[row * L.lda + 16 * kt + lq] : 0.f;
            psum[kt] += av[kt];
          }
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int ct = wave + kHowWaves * j;
            if (ct < DT) {
              const float xv = Xs[row * L.ldc + 16 * ct + lq];
#pragma unroll
              for (int kt = 0; kt < KTMAX; ++kt)
                if (kt < KT) acc[kt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kt], xv, acc[kt][j], 0, 0, 0);
            }
          }
        }
    }
  }
  if (ASMK) return;

  // ---- epilogue: V[c][:] -= (sum_n a[n][c]) c, then the store
#pragma unroll
  for (int kt = 0; kt < KTMAX; ++kt) {
    psum[kt] += __shfl_xor(psum[kt], 16, 64);
    psum[kt] += __shfl_xor(psum[kt], 32, 64);
    if (wave == 0 && lg == 0 && kt < KT) sa[16 * kt + lq] = psum[kt];
  }
  __syncthreads();
  float* o = dst + (long long)blockIdx.x * k * d;
#pragma unroll
  for (int kt = 0; kt < KTMAX; ++kt)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ct = wave + kHowWaves * j;
      if (kt < KT && ct < DT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 16 * kt + 4 * lg + r, ch = 16 * ct + lq;
          if (c < k) o[(long long)c * d + ch] = fmaf(-sa[c], Cs[c * L.ldc + ch], acc[kt][j][r]);
        }
      }
    }
}

// out[img][:] = sum_s part[img][s][:] over rows of len floats, slab after slab
// in index order (one thread per 16-B group).
__global__ __launch_bounds__(256) void how_sum_kernel(const float* __restrict__ part, int splits, int len4,
                                                      long long total4, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const long long img = i / len4;
  const int g = (int)(i - img * len4);
  const float* pp = part + (img * splits * len4 + g) * 4;
  f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int s = 0; s < splits; ++s) t += *reinterpret_cast<const f32x4*>(pp + (long long)s * len4 * 4);
  *reinterpret_cast<f32x4*>(out + i * 4) = t;
}

// ASMK's second pass, one workgroup per image over its n (smallest distance,
// centroid) pairs: mean and unbiased variance in double (sums in a fixed
// order; n == 1 gives 0 / 0 = NaN, so nothing passes the threshold, as
// torch.std of one value), integer counts in LDS, one multiply by the weight.
__global__ __launch_bounds__(256) void how_asmk_count_kernel(const float* __restrict__ minv,
                                                             const int* __restrict__ mini, int n, int k,
                                                             const float* __restrict__ w, float* __restrict__ out) {
  __shared__ double red[256];
  __shared__ int cnt[128];
  const int tid = threadIdx.x;
  const float* mv = minv + (long long)blockIdx.x * n;
  const int* mi = mini + (long long)blockIdx.x * n;
  auto block_sum = [&](double v) {
    __syncthreads();  // red's previous readers are done
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    return red[0];
  };
  double s = 0.0;
  for (int i = tid; i < n; i += 256) s += (double)mv[i];
  const double mean = block_sum(s) / (double)n;
  double q = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double t = (double)mv[i] - mean;
    q += t * t;
  }
  const double thr = mean + sqrt(block_sum(q) / (double)(n - 1));
  if (tid < 128) cnt[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 256)
    if ((double)mv[i] < thr && (unsigned)mi[i] < (unsigned)k) atomicAdd(&cnt[mi[i]], 1);  // a NaN row has no index
  __syncthreads();
  if (tid < k) out[(long long)blockIdx.x * k + tid] = w[tid] * (float)cnt[tid];
}

template <int KTMAX, int NJ, bool ASMK>
static hipError_t launch_how_pool(const float* x, int n, int d, int chunk, int splits, const float* cent, int k,
                                  float alpha, float* dst, int* dst_idx, unsigned blocks, hipStream_t s) {
  constexpr int P = (KTMAX == 8 && NJ == 4) ? 16 : 32;
  const size_t lds = (size_t)HowLds(((k + 15) >> 4) * 16, d, P).total * sizeof(float);
  return launch_dyn_lds(how_pool_kernel<KTMAX, NJ, ASMK>, blocks, kHowThreads, lds, s, x, n, d, chunk, splits, cent, k,
                        alpha, dst, dst_idx);
}

template <bool ASMK>
static hipError_t dispatch_how_pool(const float* x, int n, int d, int chunk, int splits, const float* cent, int k,
                                    float alpha, float* dst, int* dst_idx, unsigned blocks, hipStream_t s) {
  if (k <= 64)
    return d <= 128 ? launch_how_pool<4, 2, ASMK>(x, n, d, chunk, splits, cent, k, alpha, dst, dst_idx, blocks, s)
                    : launch_how_pool<4, 4, ASMK>(x, n, d, chunk, splits, cent, k, alpha, dst, dst_idx, blocks, s);
  return d <= 128 ? launch_how_pool<8, 2, ASMK>(x, n, d, chunk, splits, cent, k, alpha, dst, dst_idx, blocks, s)
                  : launch_how_pool<8, 4, ASMK>(x, n, d, chunk, splits, cent, k, alpha, dst, dst_idx, blocks, s);
}

static bool how_bad_shape(int b, int n, int d, int k) {
  return b < 0 || n < 1 || n > 65535 || d < 32 || d > 256 || (d & 31) || k < 1 || k > 128;
}

}  // namespace rr

using namespace rr;

extern "C" int rr_how_vlad(rr_handle_t h, const float* x, int b, int n, int d, const float* centroids, int k,
                           float alpha, float* out, void* stream) {
  RR_ENTRY(h);
  if (!x || !centroids || !out || how_bad_shape(b, n, d, k) || ((uintptr_t)x & 15) || ((uintptr_t)centroids & 15) ||
      ((uintptr_t)out & 15))
    return set_error(h, RR_EINVAL,
                     "rr_how_vlad: bad argument (1 <= k <= 128, d % 32 == 0, 32 <= d <= 256, 1 <= n <= 65535, 16-B "
                     "aligned)");
  if (b == 0) return RR_OK;
  const auto [splits, chunk] = split_positions(b, n, kHowMinPos, kHowTargetBlocks);
  const long long blocks = (long long)b * splits;
  const long long len = (long long)k * d;
  const long long total4 = (long long)b * (len >> 2);
  if (blocks > 0x7fffffffLL || (total4 + 255) / 256 > 0x7fffffffLL)
    return set_error(h, RR_EINVAL, "rr_how_vlad: too many images");
  hipStream_t s = (hipStream_t)stream;
  float* dst = out;
  if (splits > 1) {
    void* p = nullptr;
    if (int rc = stream_scratch(h, s, (size_t)blocks * len * sizeof(float), &p, "rr_how_vlad")) return rc;
    dst = (float*)p;
  }
  TimedLaunch tl(h, kTimeElem, s);
  if (int rc = check_hip(h, dispatch_how_pool<false>(x, n, d, chunk, splits, centroids, k, alpha, dst, nullptr,
                                                     (unsigned)blocks, s),
                         "how_vlad launch"))
    return rc;
  if (splits > 1) {
    hipLaunchKernelGGL(how_sum_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, dst, splits,
                       (int)(len >> 2), total4, out);
    return check_hip(h, hipGetLastError(), "how_sum launch");
  }
  return RR_OK;
}

extern "C" int rr_how_asmk(rr_handle_t h, const float* x, int b, int n, int d, const float* centroids,
                           const float* weights, int k, float* out, void* stream) {
  RR_ENTRY(h);
  if (!x || !centroids || !weights || !out || how_bad_shape(b, n, d, k) || ((uintptr_t)x & 15) ||
      ((uintptr_t)centroids & 15) || ((uintptr_t)weights & 15) || ((uintptr_t)out & 15))
    return set_error(h, RR_EINVAL,
                     "rr_how_asmk: bad argument (1 <= k <= 128, d % 32 == 0, 32 <= d <= 256, 1 <= n <= 65535, 16-B "
                     "aligned)");
  if (b == 0) return RR_OK;
  const auto [splits, chunk] = split_positions(b, n, kHowMinPos, kHowTargetBlocks);
  const long long blocks = (long long)b * splits;
  if (blocks > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_how_asmk: too many images");
  hipStream_t s = (hipStream_t)stream;
  // [b n] smallest distances, then [b n] centroid indices
  const size_t cells = (size_t)b * n;
  void* p = nullptr;
  if (int rc = stream_scratch(h, s, cells * (sizeof(float) + sizeof(int)), &p, "rr_how_asmk")) return rc;
  float* minv = (float*)p;
  int* mini = (int*)(minv + cells);
  TimedLaunch tl(h, kTimeElem, s);
  if (int rc = check_hip(h, dispatch_how_pool<true>(x, n, d, chunk, splits, centroids, k, 0.f, minv, mini,
                                                    (unsigned)blocks, s),
                         "how_asmk launch"))
    return rc;
  hipLaunchKernelGGL(how_asmk_count_kernel, dim3((unsigned)b), dim3(256), 0, s, minv, mini, n, k, weights, out);
  return check_hip(h, hipGetLastError(), "how_asmk_count launch");
}
