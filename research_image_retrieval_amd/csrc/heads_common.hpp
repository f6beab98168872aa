// heads_common.hpp — what the extractor heads' files (dolg_ops.hip,
// soa_ops.hip, token_ops.hip, how_ops.hip, sos_ops.hip) share: the split of an image's
// positions over workgroups, the per-stream scratch their partial sums pass
// through, the fixed-order adding kernel, the online-softmax tile step and the
// launch with more than 64 KiB of dynamic LDS.
//
// Not here on purpose: how_sum_kernel (how_ops.hip).  It adds an image's slabs
// strictly in index order and an image at b = 1 has up to 256 of them, where
// slab_sum_kernel's 16-wave order gives the same bits only up to 16 slabs; its
// rows are k d floats, not always a multiple of 256 (k = 1, d = 32).  Folding
// it in would change results.
#pragma once

#include <utility>

#include "rr_internal.hpp"

namespace rr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// An image's n positions are split over workgroups only while whole images
// leave the chip short of work (b < target_blocks): into about target_blocks / b
// chunks of at least min_positions each.  The split depends on (b, n) alone,
// so with partial sums added in a fixed order a result is the same bits on
// every run.
struct SplitPlan {
  int splits, chunk;
};
inline SplitPlan split_positions(int b, int n, int min_positions, int target_blocks) {
  if (b >= target_blocks) return {1, n};
  const int want = (target_blocks + b - 1) / b;
  const int most = (n + min_positions - 1) / min_positions;
  const int splits = want < most ? want : most;
  const int chunk = (n + splits - 1) / splits;
  return {(n + chunk - 1) / chunk, chunk};
}

// The heads' scratch (the partial slabs of split images, ASMK's per-position
// minima): one buffer per stream, owned by the handle and freed by rr_destroy.
// rr_dolg_local_pool, rr_token_pool, rr_how_vlad, rr_how_asmk, rr_sos_cov (its
// a_p, means, tile sums of squares and partial tiles) and rr_linear_splitk (its
// k-slices' partial products) share the
// buffer of their stream: launches on one stream are ordered, so the adding
// (or counting) kernel of one call has read the buffer before the next call's
// pooling kernel writes it; two streams never share one.  It grows on demand:
// a buffer that is too small is freed only after its stream has drained.  No
// lock: a handle is not shared between threads (rr.h).
inline int stream_scratch(rr_handle_s* h, hipStream_t s, size_t bytes, void** out, const char* who) {
  auto& e = h->scratch[s];
  if (e.second < bytes) {
    if (e.first) {
      if (int rc = check_hip(h, hipStreamSynchronize(s), "stream scratch sync")) return rc;
      (void)hipFree(e.first);
      e = {nullptr, 0};
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess)
      return set_error(h, RR_EWORKSPACE, std::string(who) + ": cannot allocate the per-stream scratch");
    e = {p, bytes};
  }
  *out = e.first;
  return RR_OK;
}

// out[img][:] = sum_s part[img][s][:] over rows of len floats (len % 256 == 0)
// in a fixed order: workgroup (image, 256-float group), wave w adds slabs w,
// w + 16, ... in that order (1 KiB per wave load), then the waves' sums are
// added through LDS in wave order.  MEAN: the sum is divided by hw.
constexpr int kSumWaves = 16;
template <bool MEAN>
__global__ __launch_bounds__(kSumWaves * 64) void slab_sum_kernel(const float* __restrict__ part, int splits, int len,
                                                                  int hw, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float red[(kSumWaves - 1) * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int groups = len >> 8;
  const int img = blockIdx.x / groups, g = blockIdx.x - img * groups;
  const float* pp = part + (long long)img * splits * len + g * 256 + lane * 4;
  f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int s = wave; s < splits; s += kSumWaves) t += *reinterpret_cast<const f32x4*>(pp + (long long)s * len);
  if (wave > 0) *reinterpret_cast<f32x4*>(red + (wave - 1) * 256 + lane * 4) = t;
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < kSumWaves - 1; ++w) t += *reinterpret_cast<const f32x4*>(red + w * 256 + lane * 4);
    *reinterpret_cast<f32x4*>(out + (long long)img * len + g * 256 + lane * 4) = MEAN ? t / (float)hw : t;
  }
}

// b (len / 256) workgroups; the caller has checked that the count fits an int
template <bool MEAN>
inline hipError_t launch_slab_sum(const float* part, int b, int splits, int len, int hw, float* out, hipStream_t s) {
  hipLaunchKernelGGL(slab_sum_kernel<MEAN>, dim3((unsigned)(b * (len >> 8))), dim3(kSumWaves * 64), 0, s, part, splits,
                     len, hw, out);
  return hipGetLastError();
}

// One wave's online-softmax step on a 16-query x 16-key score tile.  Lane
// (lq, lg) passes s[r] = S[query lq][key key0 + 4 lg + r], its four partial
// accumulators added as (0 + 1) + (2 + 3), with the running max m and sum l.
// Scale, mask keys >= nk to -inf, tile max and sum over the lane's 4 keys and
// its partner lanes (xor 16, 32), then the new m and l.  m starts at -inf and a
// wave only takes a tile whose first key is < nk, so the tile max is finite and
// alpha = exp(m - m_new) is exp(-inf) = 0 on the first tile, never
// (-inf) - (-inf).  Returned beside m and l: p[r] = exp(s[r] - m_new), and
// alpha, by which the caller scales its output accumulators before adding this
// tile's P.V.
// The form is the one in which both attention kernels compile to the
// instructions they had with this step written inline (tools/
// kernel_body_diff.py): values in and out, no references (a referenced m or l
// reaches registers only after inlining, which reorders the k-loop's phis);
// the partial accumulators added by the caller (four vector arguments make
// soa_attention_kernel's four LDS loads precede its first add); p written out
// and alpha's exp after it, where the compiler had sunk it.
struct SoftmaxTile {
  f32x4 p;
  float alpha, m, l;
};
__device__ __forceinline__ SoftmaxTile online_softmax_step(f32x4 s, int key0, int nk, float scale, int lg, float m,
                                                           float l) {
  float tmax = -__builtin_inff();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    s[r] = key0 + 4 * lg + r < nk ? s[r] * scale : -__builtin_inff();
    tmax = fmaxf(tmax, s[r]);
  }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  const float mn = fmaxf(m, tmax);
  const float d = m - mn;
  const f32x4 p = {expf(s[0] - mn), expf(s[1] - mn), expf(s[2] - mn), expf(s[3] - mn)};
  const float alpha = expf(d);
  float ps = (p[0] + p[1]) + (p[2] + p[3]);
  ps += __shfl_xor(ps, 16, 64);
  ps += __shfl_xor(ps, 32, 64);
  return {p, alpha, mn, l * alpha + ps};
}

// Launch of a kernel whose dynamic LDS may pass the 64 KiB a kernel gets by
// default: the limit is raised first where it has to be.
template <typename... P, typename... A>
inline hipError_t launch_dyn_lds(void (*kernel)(P...), unsigned blocks, unsigned threads, size_t lds_bytes,
                                 hipStream_t s, A... args) {
  if (lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds_bytes, s, args...);
  return hipGetLastError();
}

}  // namespace rr
