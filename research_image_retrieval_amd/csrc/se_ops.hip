// se_ops.hip — the Squeeze-and-Excitation block's two streaming kernels
// (gfx950): the per-channel spatial mean of conv3's output, and the gate (the
// second FC + sigmoid) applied with the identity add and the ReLU in one pass.
// The first FC + ReLU between them is rr_linear_splitk (b rows over a long k).
//
// Reference (models/senet_g2.py): SEBlock.forward :25-29 (AdaptiveAvgPool2d(1),
// fc = Linear, ReLU, Linear, Sigmoid, x * y.expand_as(x)) and
// SEBottleneck.forward :64-70 (se, out += residual, relu).
#include <cmath>

#include "gemm_epilogue.hpp"
#include "heads_common.hpp"

namespace rr {

constexpr int kSeWaves = 4;              // waves per workgroup (256 threads), both kernels
constexpr int kSeMinPos = 8;             // fewest positions a squeeze workgroup takes when an image is split
constexpr int kSeTargetBlocks = 1024;    // squeeze workgroups (per channel group) wanted before images stop being split
constexpr int kSeSlab = 64;              // channels of an apply workgroup
constexpr int kSeMinRows = 32;           // fewest rows an apply workgroup streams when an image is split
constexpr int kSeApplyTarget = 2048;     // apply workgroups wanted before images stop being split
constexpr int kSeDepth = 4;              // rows an apply thread has in flight (8 16-B loads with the identity)

// Workgroup blockIdx.x = (image * splits + s) * groups + g takes positions
// [s chunk, (s + 1) chunk) of its image and channels 256 g .. + 255: lane l of
// every wave holds channels 256 g + 4 l .. + 3, so a wave load is 1 KiB
// contiguous; wave w adds every kSeWaves-th position from s chunk + w in
// position order, and the waves' sums are added through LDS in wave order.
// splits == 1: dst = mean, the sum divided by hw.  Otherwise dst = part
// [image][s][c] and slab_sum_kernel<true> adds an image's slabs and divides.
__global__ __launch_bounds__(kSeWaves * 64) void se_squeeze_kernel(const float* __restrict__ y, int hw, int c, int chunk,
                                                                   int splits, int groups, float* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) float red[(kSeWaves - 1) * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int is = blockIdx.x / groups, g = blockIdx.x - is * groups;
  const int img = is / splits, s = is - img * splits;
  const int p0 = s * chunk;
  const int p1 = p0 + chunk < hw ? p0 + chunk : hw;
  const float* yi = y + (long long)img * hw * c + g * 256 + lane * 4;
  f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int p = p0 + wave; p < p1; p += kSeWaves) t += *reinterpret_cast<const f32x4*>(yi + (long long)p * c);
  if (wave > 0) *reinterpret_cast<f32x4*>(red + (wave - 1) * 256 + lane * 4) = t;
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < kSeWaves - 1; ++w) t += *reinterpret_cast<const f32x4*>(red + w * 256 + lane * 4);
    if (splits == 1) t = t / (float)hw;
    *reinterpret_cast<f32x4*>(dst + (long long)is * c + g * 256 + lane * 4) = t;
  }
}

// Workgroup blockIdx.x = (image * slabs + sl) * chunks + rc: channels 64 sl ..
// + 63, rows [rc chunk, (rc + 1) chunk) of its image.
// Gates: thread (ch = tid >> 2, q = tid & 3) adds the 16-B pieces q, q + 4, ...
// of w2[64 sl + ch] . hidden[image] as one fmaf chain in k order, the four
// threads of a channel are added by xor 1, 2 (commutative at both levels: the
// four hold the same bits): an order that depends on cr alone.  The gate goes
// to LDS; row chunk 0 writes gate_out.
// Rows: thread (r = tid >> 4, c4 = tid & 15) owns 16 B of the slab in rows
// r, r + 16, ..., taken kSeDepth rows at a time: all of a batch's loads go out
// before its first store (a thread reads and writes its own elements only, so
// out may alias y or identity).
__global__ __launch_bounds__(kSeWaves * 64) void se_apply_kernel(const float* y, const float* __restrict__ hidden,
                                                                 const float* __restrict__ w2, const float* identity,
                                                                 int hw, int c, int cr, int relu, int chunk, int chunks,
                                                                 int slabs, float* __restrict__ gate_out, float* out,
                                                                 uint32_t* __restrict__ out_amax) {
  __shared__ float gate[kSeSlab];
  __shared__ float wave_am[kSeWaves];
  const int tid = threadIdx.x;
  const int isl = blockIdx.x / chunks, rc = blockIdx.x - isl * chunks;
  const int img = isl / slabs, sl = isl - img * slabs;
  {
    const int ch = tid >> 2, q = tid & 3;
    const float* wr = w2 + (long long)(sl * kSeSlab + ch) * cr;
    const float* hr = hidden + (long long)img * cr;
    float z = 0.f;
    // (unrolled: the pieces' loads go out together; the chain's order stays k's)
#pragma unroll 8
    for (int k = q * 4; k < cr; k += 16) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k);
      const f32x4 hv = *reinterpret_cast<const f32x4*>(hr + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) z = fmaf(wv[e], hv[e], z);
    }
    z += __shfl_xor(z, 1, 64);
    z += __shfl_xor(z, 2, 64);
    // exp(-z) = +inf for z <= -89 gives 1 / inf = 0; exp(-z) = 0 for z >= 104 gives 1
    const float gt = 1.f / (1.f + expf(-z));
    if (q == 0) {
      gate[ch] = gt;
      if (gate_out != nullptr && rc == 0) gate_out[(long long)img * c + sl * kSeSlab + ch] = gt;
    }
  }
  __syncthreads();

  const int c4 = tid & 15, r0 = tid >> 4;
  const f32x4 gv = *reinterpret_cast<const f32x4*>(gate + c4 * 4);
  const int p0 = rc * chunk;
  const int p1 = p0 + chunk < hw ? p0 + chunk : hw;
  const long long base = (long long)img * hw * c + sl * kSeSlab + c4 * 4;
  const bool has_id = identity != nullptr;
  float am = 0.f;
  for (int p = p0 + r0; p < p1; p += 16 * kSeDepth) {
    f32x4 vy[kSeDepth], vi[kSeDepth];
#pragma unroll
    for (int u = 0; u < kSeDepth; ++u) {
      const int pu = p + 16 * u;
      vy[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      vi[u] = vy[u];
      if (pu < p1) {
        vy[u] = *reinterpret_cast<const f32x4*>(y + base + (long long)pu * c);
        if (has_id) vi[u] = *reinterpret_cast<const f32x4*>(identity + base + (long long)pu * c);
      }
    }
#pragma unroll
    for (int u = 0; u < kSeDepth; ++u) {
      const int pu = p + 16 * u;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = fmaf(vy[u][e], gv[e], vi[u][e]);
        if (relu) v = fmaxf(v, 0.f);
        o[e] = v;
      }
      if (pu < p1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) am = amax_acc(am, o[e]);
        *reinterpret_cast<f32x4*>(out + base + (long long)pu * c) = o;
      }
    }
  }
  // One atomic per workgroup, not per wave: the waves' maxima (non-negative, so
  // their bit patterns order as the floats) meet in LDS and wave 0 publishes.
  // (every lane of every wave arrives here: the reductions run across the wave)
  if (out_amax != nullptr) {
    const float wm = amax_reduce(__float_as_uint(am));
    if ((tid & 63) == 0) wave_am[tid >> 6] = wm;
    __syncthreads();
    if (tid < 64) {
      float m = wave_am[0];
#pragma unroll
      for (int w = 1; w < kSeWaves; ++w) m = fmaxf(m, wave_am[w]);
      amax_publish(out_amax, m, blockIdx.x);
    }
  }
}

}  // namespace rr

using namespace rr;

extern "C" int rr_se_squeeze(rr_handle_t h, const float* y, int b, int hw, int c, float* mean, void* stream) {
  RR_ENTRY(h);
  if (!y || !mean || b < 0 || hw < 1 || c < 256 || (c & 255) || ((uintptr_t)y & 15) || ((uintptr_t)mean & 15))
    return set_error(h, RR_EINVAL, "rr_se_squeeze: bad argument (c % 256 == 0, hw >= 1, b >= 0, 16-B aligned)");
  if (b == 0) return RR_OK;
  const auto [splits, chunk] = split_positions(b, hw, kSeMinPos, kSeTargetBlocks);
  const int groups = c >> 8;
  const long long blocks = (long long)b * splits * groups;
  if (blocks > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_se_squeeze: too many workgroups");
  hipStream_t s = (hipStream_t)stream;
  float* dst = mean;
  if (splits > 1) {
    void* p = nullptr;
    if (int rc = stream_scratch(h, s, (size_t)b * splits * c * sizeof(float), &p, "rr_se_squeeze")) return rc;
    dst = (float*)p;
  }
  TimedLaunch tl(h, kTimeElem, s);
  hipLaunchKernelGGL(se_squeeze_kernel, dim3((unsigned)blocks), dim3(kSeWaves * 64), 0, s, y, hw, c, chunk, splits, groups,
                     dst);
  if (int rc = check_hip(h, hipGetLastError(), "se_squeeze launch")) return rc;
  if (splits > 1) return check_hip(h, launch_slab_sum<true>(dst, b, splits, c, hw, mean, s), "se_squeeze_sum launch");
  return RR_OK;
}

extern "C" int rr_se_apply(rr_handle_t h, const float* y, const float* hidden, const float* w2, const float* identity,
                           int b, int hw, int c, int cr, int relu, float* gate_out, float* out, unsigned* out_amax,
                           void* stream) {
  RR_ENTRY(h);
  if (!y || !hidden || !w2 || !out || b < 0 || hw < 1 || c < kSeSlab || (c % kSeSlab) || cr < 4 || cr > 512 || (cr & 3) ||
      ((uintptr_t)y & 15) || ((uintptr_t)hidden & 15) || ((uintptr_t)w2 & 15) || ((uintptr_t)identity & 15) ||
      ((uintptr_t)gate_out & 15) || ((uintptr_t)out & 15) || ((uintptr_t)out_amax & 15))
    return set_error(h, RR_EINVAL,
                     "rr_se_apply: bad argument (c % 64 == 0, cr % 4 == 0, 4 <= cr <= 512, hw >= 1, b >= 0, 16-B aligned)");
  if (b == 0) return RR_OK;
  const int slabs = c / kSeSlab;
  const long long units = (long long)b * slabs;
  if (units > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_se_apply: too many workgroups");
  const auto [chunks, chunk] = split_positions((int)units, hw, kSeMinRows, kSeApplyTarget);
  const long long blocks = units * chunks;
  if (blocks > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_se_apply: too many workgroups");
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch tl(h, kTimeElem, s);
  hipLaunchKernelGGL(se_apply_kernel, dim3((unsigned)blocks), dim3(kSeWaves * 64), 0, s, y, hidden, w2, identity, hw, c, cr,
                     relu, chunk, chunks, slabs, gate_out, out, (uint32_t*)out_amax);
  return check_hip(h, hipGetLastError(), "se_apply launch");
}
