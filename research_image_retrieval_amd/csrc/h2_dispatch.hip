// h2_dispatch.hip — the f16x2 split GEMM core's host side: which kernel of
// the family serves a GEMM (h2_tile.hip: the split and the tile-config table;
// h2_stream.hip config 8, h2_stream256.hip config 15, h2_halo.hip configs 13 /
// 14), the ≥4 GB row chunking, and the two small kernels every layer needs:
// the weight split and the max-|x| record.
#include <algorithm>

#include "gemm_epilogue.hpp"
#include "rr_internal.hpp"

namespace rr {

// The pick among the tile configs (table: h2_tile.hip).
// rr_set_tuning(RR_TUNE_S3_CFG) forces a config (tests, tools); a forced 1, 2,
// 5 or 6 (no instance) runs the pick.
static int pick_s3(const GemmArgs& g, int forced) {
  if (forced >= 1 && forced <= 8) return forced;
  if ((g.N % 256) == 0) return 4;
  // rounds of resident blocks x tile area per CU / relative per-FLOP speed
  auto cost = [&](long long bm, long long bn, long long per_cu, double speed) {
    const long long slots = 256 * per_cu;
    const long long t = ((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn);
    return (double)((t + slots - 1) / slots) * bm * bn * per_cu / speed;
  };
  double best = cost(128, 128, 2, 1.0);
  int cfg = 1;
  if (cost(256, 128, 1, 1.15) < best) best = cost(256, 128, 1, 1.15), cfg = 3;
  if (cost(256, 64, 2, 1.0) < best) best = cost(256, 64, 2, 1.0), cfg = 7;
  return cfg;
}
// config 1 (no instance) -> 3 where it tiles no worse than 7
static int pick_h2(const GemmArgs& g, int forced) {
  if (forced == 9) return (g.N % 256) == 0 ? 9 : pick_h2(g, 0);
  if (forced == 10) return (g.N % 256) == 0 ? 10 : pick_h2(g, 0);
  if (forced == 11) return (g.N % 128) == 0 ? 11 : pick_h2(g, 0);
  if (forced == 12) return (g.N % 256) == 0 ? 12 : pick_h2(g, 0);
  // N == 128: two 128x128 blocks per CU (config 11) run the R101 N = 128
  // layers 4-7 % faster than the 256x128 tile (profiles/r03l_h2_cfg_sweep.txt);
  // the dense K >= 256 ones take config 15's persistent 256x128 form before
  // this pick (profiles/r05ae_s3q128_ab/)
  if (forced == 0 && g.N == 128) return 11;
  int cfg = pick_s3(g, forced);
  if (cfg == 3 || cfg == 4 || cfg == 7 || cfg == 8) return cfg;
  cfg = pick_s3(g, 0);
  if (cfg == 1) cfg = (g.N % 128) == 0 ? 3 : 7;
  return cfg;
}

// config 8 serves dense A (1x1 convs), N % 256 == 0, any residual / ReLU
// combination; the rest falls back to the library's pick
static bool s3_persist_ok(const GemmArgs& g, int amode) { return (g.N % 256) == 0 && amode == A_DENSE; }

static hipError_t launch_h2_am(int am, const GemmArgs& g, hipStream_t s, int forced, int n_cu, int st) {
  // the N = 64 halo tile as a persistent stream: the default (s3_cfg 13
  // forces the one-tile form); 64@56 3x3 1.212 -> 1.161 ms, bit-identical
  // (profiles/r05w_sweep.txt; the embed 68.26 / 68.22 ms, r05w_e2e.txt)
  const bool hpers = forced == 0;
  // dense A past config 15's 32-bit byte offsets (A or C of 4 GB or more:
  // C2's 1024-px gallery batches at layer 1, 6.4 GB at batch 128) ran config
  // 7 / 11 instead: the GEMM now goes in row chunks that fit, each a config-15
  // launch on offset pointers (chunks of 256-row multiples keep the one-launch
  // tiling, so every row is the one launch's).  256->64 at 128 x 256 x 192:
  // 1.738 -> 1.575 ms, 256->128 2.204 -> 2.136 (profiles/r06ze_dense4gb_ab.txt)
  if (am == A_DENSE && (forced == 15 || forced == 0) && s3q_shape(g) && !s3q_fits(g)) {
    const long long per = ((1LL << 32) - 1) / (4LL * std::max(g.lda, g.ldc)) / 256 * 256;
    if (per >= 256) {
      for (long long m0 = 0; m0 < g.M; m0 += per) {
        GemmArgs c = g;
        c.M = (int)std::min<long long>(per, g.M - m0);
        c.A = g.A + m0 * g.lda;
        c.C = g.C + m0 * g.ldc;
        if (g.residual != nullptr) c.residual = g.residual + m0 * g.ldc;
        if (const hipError_t e = launch_h2_am(am, c, s, forced, n_cu, st)) return e;
      }
      return hipSuccess;
    }
  }
  // config 15 (config 12 as a persistent k-stream): the pick for dense A
  // with config 12's shape condition (forced 15: the same, every other GEMM
  // on the library's pick; forced 12 runs config 12).  Measured at 1280
  // images (profiles/r05f_cfg15_sweep.txt, interleaved): 256->1024 + residual
  // x22 0.704 -> 0.569 ms, 512->2048 0.513 -> 0.432, 1024->256 0.409 ->
  // 0.384, 2048->512 0.357 -> 0.351; the bench's embed 70.49 -> 69.05 ms
  // (r05f_cfg15_e2e.txt; residual layers only: 69.17)
  if (forced == 15 || forced == 0) {
    if (am == A_DENSE && s3q_shape(g) && s3q_fits(g)) return launch_s3q(g, s, n_cu, st);
    if (forced == 15) forced = 0;
  }
  // the halo-A tile (configs 13 / 14) is the pick for N % 256 == 0 and N == 64: the 3x3
  // 256@14 and 512@7 layers 2.7 % / 1.6 % faster than config 12 at 1280
  // images (profiles/r03t_h2_cfg_sweep.txt)
  if (am == A_CONV) {
    // (N == 64 too: the 256x64 instance with three taps per barrier runs the
    // 64@56 3x3 layers 1.455 -> 1.297 ms; the 256x128 one lost on 128@28,
    // 0.888 -> 0.922 ms, and stays opt-in; profiles/r03w_h2_cfg_sweep.txt)
    // The 256x256 instance (hr 288, the N % 256 layers) runs on
    // v_mfma_f32_16x16x32_f16 by default: 256@14 0.716 -> 0.675 ms, 512@7
    // 0.671 -> 0.606; the 256x64 one lost on 64@56 (1.225 -> 1.334 ms) and
    // keeps the 32x32x16 form (profiles/r04c_h2_cfg_sweep.txt).  Forcing 13
    // selects the 32x32x16 form everywhere, 14 the 16x16x32 form everywhere.
    // Round 6: N = 128 too (the 256x128 instance on 16x16x32): 128@28 1.035 ->
    // 0.931 ms against config 11 at 1280 images, after the halo tiles' taps
    // became compile-time (profiles/r06w_halo128_ab.txt)
    // halo_2d: the 2-D block tiles where no raster halo holds the map (-1),
    // wherever one serves (1), never (0)
    if (forced == 0 && g.halo_2d != 0 && h2_halo_2d_ok(g) && (g.halo_2d == 1 || !h2_halo_rows(g)))
      return launch_h2_halo_2d(g, s);
    if (forced == 13 || forced == 14 || (forced == 0 && ((g.N % 256) == 0 || g.N == 64 || g.N == 128))) {
      if (const int hr = h2_halo_rows(g))
        return launch_h2_halo(g, s, hr,
                              forced == 14 ? 1 : forced == 13 ? 0 : g.halo_mf >= 0 ? g.halo_mf : (hr == 288 || hr == 320 ? 1 : 0),
                              hpers, n_cu);
    }
  }
  if (forced == 13 || forced == 14) forced = 0;
  int cfg = pick_h2(g, forced);
  // (dense A: config 15 above, config 12 as a persistent k-stream)
  // N % 256 == 0: the 256x256 one-accumulator tile (config 12) everywhere but
  // the short-K residual expansions (K < 256: their epilogue dominates and the
  // persistent k-stream, config 8, hides part of it).  Measured per R101 layer
  // at 1280 images (profiles/r03p_h2_cfg_sweep.txt): 3x3 256@14 0.848 -> 0.794
  // ms, 1024->256 0.432 -> 0.400, 512@7 0.778 -> 0.707, 2048->512 0.393 ->
  // 0.350, 256->1024 (residual) 0.690 -> 0.676; 128->512 / 64->256 (residual,
  // K 128 / 64) 17 % / 8 % slower, so those keep config 8.  K < 256 without a
  // residual keeps the two-accumulator tiles too: on a K = 64 conv the single
  // accumulator's max error (2.7e-7 Sigma|ab|) exceeded the exact-fp32 core's
  // (2.2e-7), the bar of tests/test_gpu_h2.py (no such layer in the R101
  // trunk: its K = 64 projection runs fused, rr_bottleneck_out_h2).
  const bool big = (g.N % 256) == 0 && g.K >= 256;
  if (forced == 0 && big) cfg = 12;
  else if (forced == 0 && s3_persist_ok(g, am)) cfg = 8;
  if (cfg == 8) {
    if (s3_persist_ok(g, am)) return launch_s3p(g, s, n_cu, st);
    cfg = pick_h2(g, 0);
  }
  return launch_h2_tile(cfg, am, g, s, n_cu, st);  // 4, 7, 9-12, otherwise 3
}

int launch_gemm_s3(rr_handle_s* h, int amode, const GemmArgs& g, hipStream_t s, int timer_cls) {
  if (g.M < 0 || g.N <= 0 || g.K <= 0) return set_error(h, RR_EINVAL, "gemm_s3: bad shape");
  if (g.K % 32) return set_error(h, RR_EINVAL, "gemm_s3: K must be a multiple of 32");
  if (amode == A_DENSE && ((g.lda & 3) || ((uintptr_t)g.A & 15)))
    return set_error(h, RR_EINVAL, "gemm_s3: dense A needs lda % 4 == 0 and 16-B alignment");
  if (amode == A_CONV && (g.Cin % 32)) return set_error(h, RR_EINVAL, "gemm_s3: conv A needs Cin % 32 == 0");
  if (amode == A_CONV_C4 && (g.Cin != 4 || g.K < g.KH * g.KW * 4 || ((uintptr_t)g.A & 15)))
    return set_error(h, RR_EINVAL, "gemm_s3: NHWC4 A needs Cin == 4, K >= KH*KW*4, 16-B alignment");
  if (amode != A_DENSE && amode != A_CONV && amode != A_CONV_C4)
    return set_error(h, RR_EINVAL, "gemm_s3: unsupported A mode");
  if ((g.ldb & 7) || (g.b_plane & 7) || ((uintptr_t)g.B & 15))
    return set_error(h, RR_EINVAL, "gemm_s3: B planes need ldb % 8 == 0, plane stride % 8 == 0, 16-B alignment");
  if (g.col_scale == nullptr || g.a_amax == nullptr || ((uintptr_t)g.col_scale & 15))
    return set_error(h, RR_EINVAL, "gemm_h2: needs 16-B aligned column scales and the A max-|x| record");
  if (g.relu == 2 || g.out_bf16 || (g.N & 3) || (g.ldc & 3))
    return set_error(h, RR_EINVAL, "gemm_h2: fp32 output, ReLU or none, N % 4 == 0");
  if (g.M == 0) return RR_OK;
  // default stagger: the residual layers only (their 256 KB-per-tile epilogue
  // is the HBM-heavy phase): 256->1024 x23 -5 %, the other residual layers
  // -1 %, the rest neutral to +2 % (tools/ab_trunk.sh stagger, profiles/r02f_s3_stagger.txt)
  const int st = h->tune.s3_stagger >= 0 ? h->tune.s3_stagger : (g.residual != nullptr ? 8 : 0);
  hipError_t e;
  {
    TimedLaunch tl(h, timer_cls, s);
    const int f = (g.residual != nullptr && h->tune.s3_cfg_res > 0) ? h->tune.s3_cfg_res : h->tune.s3_cfg;
    const int n_cu = device_cu_count(h);
    {
      // conv_il (opt-in): every R101 layer the 256x256 tile serves ran 1-3 %
      // faster alone at 1280 images (256->1024 0.681 -> 0.668 ms; profiles/
      // r04g_h2_cfg_il.txt, r04h_h2_cfg_il.txt), but the bench's whole embed
      // ran 0.5 % slower with it (71.77 -> 72.11 ms, r04j_e2e_ab.txt; limited
      // to the GEMMs without a residual, 1.0 % slower, r04s_e2e_conv_il.txt).
      // It also selects the halo tile's 16x16x32 form with its B DMA spread.
      GemmArgs g2 = g;
      g2.issue_spread = h->tune.conv_il == 1;
      g2.halo_mf = h->tune.halo_mf;
      g2.halo_2d = h->tune.halo_2d;
      e = launch_h2_am(amode, g2, s, f, n_cu, st);
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
