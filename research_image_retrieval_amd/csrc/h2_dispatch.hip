// h2_dispatch.hip — the f16x2 split GEMM core's host side: launch_gemm_s3
// validates, asks h2_route (h2_route.hpp) which kernel instance serves the
// GEMM, and launches it (h2_tile.hip, h2_stream.hip, h2_stream256.hip,
// h2_halo.hip), in row chunks where the route says so; and the two small
// kernels every layer needs: the weight split and the max-|x| record.
#include <algorithm>

#include "gemm_epilogue.hpp"
#include "h2_route.hpp"

namespace rr {

int launch_gemm_s3(rr_handle_s* h, int amode, const GemmArgs& g, hipStream_t s, int timer_cls) {
  if (const char* err = h2_shape_error(amode, g)) return set_error(h, RR_EINVAL, err);
  if (amode != A_CONV && ((uintptr_t)g.A & 15)) return set_error(h, RR_EINVAL, "gemm_s3: dense / NHWC4 A needs 16-B alignment");
  if ((uintptr_t)g.B & 15) return set_error(h, RR_EINVAL, "gemm_s3: B planes need 16-B alignment");
  if (g.col_scale == nullptr || g.a_amax == nullptr || ((uintptr_t)g.col_scale & 15))
    return set_error(h, RR_EINVAL, "gemm_h2: needs 16-B aligned column scales and the A max-|x| record");
  if (g.M == 0) return RR_OK;
  // default stagger: the residual layers only (their 256 KB-per-tile epilogue
  // is the HBM-heavy phase): 256->1024 x23 -5 %, the other residual layers
  // -1 %, the rest neutral to +2 % (tools/ab_trunk.sh stagger, profiles/r02f_s3_stagger.txt)
  const int st = h->tune.s3_stagger >= 0 ? h->tune.s3_stagger : (g.residual != nullptr ? 8 : 0);
  const H2Route r = h2_route(amode, g, h2_tune(h->tune, g.residual != nullptr));
  const int n_cu = device_cu_count(h);
  hipError_t e = hipSuccess;
  {
    TimedLaunch tl(h, timer_cls, s);
    // row chunks of a 256-row multiple keep the one launch's tiling: every
    // row is computed as the one launch would
    const long long per = r.chunk_rows ? r.chunk_rows : g.M;
    for (long long m0 = 0; m0 < g.M && e == hipSuccess; m0 += per) {
      GemmArgs c = g;
      c.M = (int)std::min<long long>(per, g.M - m0);
      c.A = g.A + m0 * g.lda;
      c.C = g.C + m0 * g.ldc;
      if (g.residual != nullptr) c.residual = g.residual + m0 * g.ldc;
      switch (r.family) {  // what the route names
        case H2_STREAM256: e = launch_s3q(r, c, s, n_cu, st); break;
        case H2_STREAM: e = launch_s3p(c, s, n_cu, st); break;
        case H2_TILE: e = launch_h2_tile(r, amode, c, s, n_cu, st); break;
        default: e = launch_h2_halo(r, c, s, n_cu);
      }
    }
  }
  return check_hip(h, e, "gemm_h2 launch");
}

// ---- weight split, f16x2: row n of w [rows][k] at scale 2^e_n (h2_exp of
// the row's max |w|) -> planes [2][rows][kpad] (zero past k), iscale[n] ----
__global__ __launch_bounds__(256) void split2h_kernel(const float* __restrict__ w, int rows, int k, int kpad,
                                                      uint16_t* __restrict__ planes, float* __restrict__ iscale) {
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* wr = w + (long long)n * k;
  float am = 0.f;
  for (int i = tid; i < k; i += 256) am = amax_acc(am, wr[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o));
  if ((tid & 63) == 0) red[tid >> 6] = am;
  __syncthreads();
  am = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const int e = h2_exp(am);
  const float sc = __builtin_amdgcn_ldexpf(1.f, e);
  if (tid == 0) iscale[n] = __builtin_amdgcn_ldexpf(1.f, -e);
  const long long plane = (long long)rows * kpad;
  uint16_t* p0 = planes + (long long)n * kpad;
  for (int i = tid; i < kpad; i += 256) {
    const float v = i < k ? wr[i] * sc : 0.f;
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    p0[i] = __builtin_bit_cast(uint16_t, hi);
    p0[plane + i] = __builtin_bit_cast(uint16_t, lo);
  }
}

int launch_split2h(rr_handle_s* h, const float* w, int rows, int k, int kpad, uint16_t* planes, float* iscale,
                   hipStream_t s) {
  if (rows <= 0) return RR_OK;
  hipLaunchKernelGGL(split2h_kernel, dim3((unsigned)rows), dim3(256), 0, s, w, rows, k, kpad, planes, iscale);
  return check_hip(h, hipGetLastError(), "split2h launch");
}

// ---- max |x| of a tensor into its RR_AMAX_SLOTS-word record ----
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, long long n, uint32_t* slots) {
  float am = 0.f;
  const long long gs = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (((uintptr_t)x & 15) == 0) {
    const long long n4 = n >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    for (long long i = i0; i < n4; i += gs) {
      const f32x4 v = x4[i];
      am = amax_acc(amax_acc(am, v[0]), v[1]);
      am = amax_acc(amax_acc(am, v[2]), v[3]);
    }
    for (long long i = (n4 << 2) + i0; i < n; i += gs) am = amax_acc(am, x[i]);
  } else {
    for (long long i = i0; i < n; i += gs) am = amax_acc(am, x[i]);
  }
  amax_publish(slots, am, blockIdx.x * 4 + (threadIdx.x >> 6));
}

int launch_amax(rr_handle_s* h, const float* x, long long n, uint32_t* slots, hipStream_t s) {
  if (n <= 0) return RR_OK;
  const long long blocks = std::min<long long>((n / 4 + 255) / 256 + 1, 2048);
  hipLaunchKernelGGL(amax_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, n, slots);
  return check_hip(h, hipGetLastError(), "amax launch");
}

#if RR_S3_PHASES  // (undefined in the product build)
// diagnostic build (h2_common.hpp): read and clear the phase sums, one row
// of 8 per kernel file ([4][8] cycles)
int h2_tile_phases(unsigned long long* out);
int h2_stream_phases(unsigned long long* out);
int h2_stream256_phases(unsigned long long* out);
int h2_halo_phases(unsigned long long* out);
#endif

}  // namespace rr

#if RR_S3_PHASES  // (undefined in the product build)
extern "C" int rr_debug_phases(unsigned long long* out) {
  if (const int e = rr::h2_tile_phases(out)) return e;
  if (const int e = rr::h2_stream_phases(out + 8)) return e;
  if (const int e = rr::h2_stream256_phases(out + 16)) return e;
  return rr::h2_halo_phases(out + 24);
}
#endif
