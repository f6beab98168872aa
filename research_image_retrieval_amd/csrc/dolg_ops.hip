// dolg_ops.hip — the DOLG head's two fused kernels (gfx950): the local branch's
// attention-weighted pooling in one read of the conv1+BN map, and the
// orthogonal fusion of the pooled local vector with the global one.
//
// Reference (networks/RetrievalNet.py:409-474, with_aspp=False):
//   fmn = y / max(||y||_2, 1e-12); att = softplus(conv2(relu(y)));
//   fl = att * fmn; proj = fg (fg . fl_p) / ||fg||^2; fo = mean_p (fl - proj)
// proj is linear in fl, so fo = m - fg (fg . m) / (fg . fg) with m = mean_p fl:
// neither fl nor proj is ever stored.
#include "heads_common.hpp"

namespace rr {

constexpr int kPoolWaves = 4;        // waves per workgroup (256 threads)
constexpr int kPoolMinPixels = 8;    // fewest pixels a workgroup takes when an image is split
constexpr int kPoolTargetBlocks = 1024;  // workgroups wanted before images stop being split

// One wave owns a pixel row of C = 256 NV channels: lane l holds channels
// 256 j + 4 l .. + 3 (j < NV) as NV float4s, so a wave load is 1 KiB
// contiguous.  From those registers: sum y^2 and sum w2 relu(y) (wave_sum, a
// fixed order), the scalar softplus(. + b2) / max(sqrt(sum y^2), 1e-12), and
// scalar * y into the lane's channel accumulators.  Workgroup blockIdx.x =
// image * splits + s takes pixels [s chunk, (s + 1) chunk) of its image, wave
// w of it every kPoolWaves-th pixel from s chunk + w; the waves' accumulators
// are added through LDS in wave order.  splits == 1: out[image] = sum / hw.
// Otherwise the sum goes to part[image][s] and slab_sum_kernel<true> adds an
// image's slabs in a fixed order: the same bits on every run (no float atomics).
template <int NV>
__global__ __launch_bounds__(kPoolWaves * 64) void dolg_local_pool_kernel(const float* __restrict__ y, int hw, int chunk,
                                                                          int splits, const float* __restrict__ w2,
                                                                          float b2, float* __restrict__ dst) {
  constexpr int C = NV * 256;
  extern __shared__ __attribute__((aligned(16))) float dolg_lds[];  // [kPoolWaves - 1][C]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int img = blockIdx.x / splits, s = blockIdx.x - img * splits;
  const int p0 = s * chunk;
  const int p1 = p0 + chunk < hw ? p0 + chunk : hw;
  const float* yi = y + (long long)img * hw * C + lane * 4;

  f32x4 wv[NV], acc[NV], cur[NV], nxt[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    wv[j] = *reinterpret_cast<const f32x4*>(w2 + j * 256 + lane * 4);
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    cur[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    nxt[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int p = p0 + wave;  // wave-uniform
  if (p < p1) {
#pragma unroll
    for (int j = 0; j < NV; ++j) cur[j] = *reinterpret_cast<const f32x4*>(yi + (long long)p * C + j * 256);
  }
  for (; p < p1; p += kPoolWaves) {
    const int pn = p + kPoolWaves;
    if (pn < p1) {  // the next row's loads fly under this row's arithmetic
#pragma unroll
      for (int j = 0; j < NV; ++j) nxt[j] = *reinterpret_cast<const f32x4*>(yi + (long long)pn * C + j * 256);
    }
    float ss = 0.f, dot = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = cur[j][e];
        ss = fmaf(v, v, ss);
        dot = fmaf(wv[j][e], fmaxf(v, 0.f), dot);
      }
    ss = wave_sum(ss);
    dot = wave_sum(dot);
    const float logit = dot + b2;
    const float att = logit > 20.f ? logit : log1pf(expf(logit));  // nn.Softplus(beta=1, threshold=20)
    const float sc = att / fmaxf(sqrtf(ss), 1e-12f);               // F.normalize: the clamp is on the norm
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      acc[j] += sc * cur[j];
      cur[j] = nxt[j];
    }
  }

  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
      *reinterpret_cast<f32x4*>(dolg_lds + (wave - 1) * C + j * 256 + lane * 4) = acc[j];
  }
  __syncthreads();
  if (wave == 0) {
    const float den = (float)hw;
    float* o = dst + (long long)blockIdx.x * C + lane * 4;  // out[img] (splits == 1) or part[img][s]
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      f32x4 t = acc[j];
#pragma unroll
      for (int w = 0; w < kPoolWaves - 1; ++w) t += *reinterpret_cast<const f32x4*>(dolg_lds + w * C + j * 256 + lane * 4);
      if (splits == 1) t = t / den;
      *reinterpret_cast<f32x4*>(o + j * 256) = t;
    }
  }
}

// One wave per row: out[r] = [fg | m - fg (fg . m) / (fg . fg)].  No epsilon on
// fg . fg: a zero fg row gives NaN, as the reference's division does.
__global__ __launch_bounds__(256) void dolg_orth_fuse_kernel(const float* __restrict__ fg, const float* __restrict__ m,
                                                             int b, int c, float* __restrict__ out) {
  const int row = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= b) return;  // wave-uniform
  const float* g = fg + (long long)row * c;
  const float* mr = m + (long long)row * c;
  float* o = out + (long long)row * 2 * c;
  float gm = 0.f, gg = 0.f;
  for (int i = lane * 4; i < c; i += 256) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
    const f32x4 mv = *reinterpret_cast<const f32x4*>(mr + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      gm = fmaf(gv[e], mv[e], gm);
      gg = fmaf(gv[e], gv[e], gg);
    }
  }
  gm = wave_sum(gm);
  gg = wave_sum(gg);
  const float k = gm / gg;
  for (int i = lane * 4; i < c; i += 256) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
    const f32x4 mv = *reinterpret_cast<const f32x4*>(mr + i);
    *reinterpret_cast<f32x4*>(o + i) = gv;
    *reinterpret_cast<f32x4*>(o + c + i) = mv - gv * k;
  }
}

template <int NV>
static void launch_pool(const float* y, int hw, int chunk, int splits, const float* w2, float b2, float* dst,
                        unsigned blocks, hipStream_t s) {
  const size_t lds = (size_t)(kPoolWaves - 1) * NV * 256 * sizeof(float);
  hipLaunchKernelGGL(dolg_local_pool_kernel<NV>, dim3(blocks), dim3(kPoolWaves * 64), lds, s, y, hw, chunk, splits, w2, b2,
                     dst);
}

}  // namespace rr

using namespace rr;

extern "C" int rr_dolg_local_pool(rr_handle_t h, const float* y, int b, int hw, int c, const float* w2, float b2,
                                  float* out, void* stream) {
  RR_ENTRY(h);
  if (!y || !w2 || !out || b < 0 || hw <= 0 || c <= 0 || (c & 255) || c > 2048 || ((uintptr_t)y & 15) ||
      ((uintptr_t)out & 15) || ((uintptr_t)w2 & 15))
    return set_error(h, RR_EINVAL, "rr_dolg_local_pool: bad argument (c % 256 == 0, c <= 2048, hw > 0, 16-B aligned)");
  if (b == 0) return RR_OK;
  const auto [splits, chunk] = split_positions(b, hw, kPoolMinPixels, kPoolTargetBlocks);
  const long long blocks = (long long)b * splits;
  if (blocks > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_dolg_local_pool: too many images");
  hipStream_t s = (hipStream_t)stream;
  float* dst = out;
  if (splits > 1) {
    void* p = nullptr;
    if (int rc = stream_scratch(h, s, (size_t)blocks * c * sizeof(float), &p, "rr_dolg_local_pool")) return rc;
    dst = (float*)p;
  }
  TimedLaunch tl(h, kTimeElem, s);
  switch (c >> 8) {
    case 1: launch_pool<1>(y, hw, chunk, splits, w2, b2, dst, (unsigned)blocks, s); break;
    case 2: launch_pool<2>(y, hw, chunk, splits, w2, b2, dst, (unsigned)blocks, s); break;
    case 3: launch_pool<3>(y, hw, chunk, splits, w2, b2, dst, (unsigned)blocks, s); break;
    case 4: launch_pool<4>(y, hw, chunk, splits, w2, b2, dst, (unsigned)blocks, s); break;
    case 5: launch_pool<5>(y, hw, chunk, splits, w2, b2, dst, (unsigned)blocks, s); break;
    case 6: launch_pool<6>(y, hw, chunk, splits, w2, b2, dst, (unsigned)blocks, s); break;
    case 7: launch_pool<7>(y, hw, chunk, splits, w2, b2, dst, (unsigned)blocks, s); break;
    default: launch_pool<8>(y, hw, chunk, splits, w2, b2, dst, (unsigned)blocks, s); break;
  }
  if (int rc = check_hip(h, hipGetLastError(), "dolg_local_pool launch")) return rc;
  if (splits > 1) return check_hip(h, launch_slab_sum<true>(dst, b, splits, c, hw, out, s), "dolg_pool_sum launch");
  return RR_OK;
}

extern "C" int rr_dolg_orth_fuse(rr_handle_t h, const float* fg, const float* m, int b, int c, float* out,
                                 void* stream) {
  RR_ENTRY(h);
  if (!fg || !m || !out || b < 0 || c <= 0 || (c & 3) || ((uintptr_t)fg & 15) || ((uintptr_t)m & 15) ||
      ((uintptr_t)out & 15))
    return set_error(h, RR_EINVAL, "rr_dolg_orth_fuse: bad argument (c % 4 == 0, 16-B aligned rows)");
  if (b == 0) return RR_OK;
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch tl(h, kTimeElem, s);
  const long long threads = (long long)b * 64;
  hipLaunchKernelGGL(dolg_orth_fuse_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, fg, m, b, c, out);
  return check_hip(h, hipGetLastError(), "dolg_orth_fuse launch");
}
