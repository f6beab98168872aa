// h2_route.hpp — which kernel instance of the f16x2 split core serves a GEMM.
// One pure host function, h2_route: no HIP call, no handle, no pointer read
// (a pointer is only compared with null).  launch_gemm_s3 (h2_dispatch.hip)
// launches exactly what it names; rr_h2_route (rr.h) reports it, and
// tests/test_h2_route.py holds its table for the ResNet trunks on the CPU.
#pragma once

#include <algorithm>

#include "rr_internal.hpp"

namespace rr {

enum H2Family { H2_TILE = 0, H2_STREAM = 1, H2_STREAM256 = 2, H2_HALO = 3, H2_HALO_2D = 4 };

// One kernel instantiation and how it is launched.  The tuple is the kernel
// template's, as far as the family has the parameter (0 where it has not).
struct H2Route {
  int family = H2_TILE, cfg = 0;       // cfg: the tile table's number (h2_tile.hip): 3, 4, 7-15
  int wm = 0, wn = 0, fm = 0, fn = 0;  // WM x WN waves of FM x FN 32x32 MFMA tiles
  int bk = 0, hr = 0, tpk = 0;         // k-tile depth; halo tiles: the buffer's rows (HALO_HR), taps per barrier
  int mf16 = 0, nstg = 0, acc = 0;     // 1: v_mfma_f32_16x16x32_f16 (0: 32x32x16); LDS stages; accumulator sets (1: ACC1 / !ACC2)
  int il = 0, pers = 0, t2 = 0;        // loads spread among the MFMAs; 1: persistent stream (halo 2: one buffer at 256 rows); 2-D tile columns
  long long chunk_rows = 0;            // rows per launch (operands of 4 GB or more); 0: one launch
};

// rr_set_tuning's values that steer the route
struct H2Tune {
  int forced = 0;    // s3_cfg, or s3_cfg_res for a GEMM with a residual
  int halo_mf = -1;  // -1 the pick; 0 / 1 the MFMA form; N = 64: 2 the 512-row tile, 3 the persistent stream; N = 128: 4 two buffers
  int halo_2d = -1;  // the 2-D halo tiles: -1 where no raster halo holds the map, 1 wherever one serves, 0 never
  int conv_il = -1;  // 1: the IL instances of config 12 and of the 288-row halo tile
};
inline H2Tune h2_tune(const rr_handle_s::Tuning& t, bool residual) {
  return {(residual && t.s3_cfg_res > 0) ? t.s3_cfg_res : t.s3_cfg, t.halo_mf, t.halo_2d, t.conv_il};
}

// ---- shape predicates: what launch_gemm_s3 rejects by shape alone (nullptr: none) ...
inline const char* h2_shape_error(int amode, const GemmArgs& g) {
  if (g.M < 0 || g.N <= 0 || g.K <= 0) return "gemm_s3: bad shape";
  if (g.K % 32) return "gemm_s3: K must be a multiple of 32";
  if (amode != A_DENSE && amode != A_CONV && amode != A_CONV_C4) return "gemm_s3: unsupported A mode";
  if (amode == A_DENSE && (g.lda & 3)) return "gemm_s3: dense A needs lda % 4 == 0";
  if (amode == A_CONV && (g.Cin % 32)) return "gemm_s3: conv A needs Cin % 32 == 0";
  if (amode == A_CONV_C4 && (g.Cin != 4 || g.K < g.KH * g.KW * 4)) return "gemm_s3: NHWC4 A needs Cin == 4, K >= KH*KW*4";
  if ((g.ldb & 7) || (g.b_plane & 7)) return "gemm_s3: B planes need ldb % 8 == 0, plane stride % 8 == 0";
  if (g.relu == 2 || g.out_bf16 || (g.N & 3) || (g.ldc & 3)) return "gemm_h2: fp32 output, ReLU or none, N % 4 == 0";
  return nullptr;
}
// config 8 serves dense A at N % 256 == 0, any residual / ReLU combination
inline bool s3_persist_ok(const GemmArgs& g, int amode) { return (g.N % 256) == 0 && amode == A_DENSE; }
// config 15 serves dense A at N % 256 == 0 or N == 128 with K >= 256 (the
// 256x256 and 256x128 forms), and N == 64 with K >= 64 (the 256x64 form)
inline bool s3q_shape(const GemmArgs& g) {
  return ((g.N % 256) == 0 && g.K >= 256) || (g.N == 128 && g.K >= 256) || (g.N == 64 && g.K >= 64);
}
// config 15 addresses A and the residual by 32-bit byte offsets
inline bool s3q_fits(const GemmArgs& g) {
  const long long lim = 1LL << 32;
  return (long long)g.M * g.lda * 4 < lim && (long long)g.M * g.ldc * 4 < lim;
}
// the halo tiles' convolution: 3x3, stride 1, pad 1 (output = input size), Cin % 32 == 0
inline bool h2_halo_conv(const GemmArgs& g) {
  return g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 && g.OH == g.H && g.OW == g.W && (g.Cin % 32) == 0 &&
         g.K == 9 * g.Cin;
}
// the raster halo tile's buffer rows (288: 256x256, 320: 256x128, 384: 256x64),
// which must hold the 256 + 2 (W + 1) input rows of a tile; 0: none serves g
inline int h2_halo_rows(const GemmArgs& g) {
  if (!h2_halo_conv(g)) return 0;
  const int need = 256 + 2 * (g.W + 1);
  if ((g.N % 256) == 0) return need <= 288 ? 288 : 0;
  if ((g.N % 128) == 0) return need <= 320 ? 320 : 0;
  if ((g.N % 64) == 0) return need <= 384 ? 384 : 0;
  return 0;
}
// whether a 2-D block halo tile serves g: whole images, no residual epilogue
// (the trunk's 3x3s have none), N % 256 == 0, 128 or 64
inline bool h2_halo_2d_ok(const GemmArgs& g) {
  return h2_halo_conv(g) && g.H > 0 && g.W > 0 && (g.M % (g.H * g.W)) == 0 && g.residual == nullptr &&
         ((g.N % 256) == 0 || g.N == 128 || g.N == 64);
}
// the N = 128 2-D tile (16 x 16 outputs) has a block per CU of a 256-CU device
inline bool h2_halo_2d_fills(const GemmArgs& g) {
  return g.N != 128 || (long long)(g.M / (g.H * g.W)) * ((g.H + 15) / 16) * ((g.W + 15) / 16) >= 256;
}

// ---- the instances.  h2_tile.hip's (tile shapes described there): config, WM, WN, FM, FN, BK,
// MINB, MF16, NSTG, ACC1, IL.  h2_tile_route and the file's launcher both read this table.
#define RR_H2_TILE_INSTANCES(X)         \
  X(3, 4, 2, 2, 2, 32, 1, 0, 2, 0, 0)   \
  X(4, 2, 4, 2, 2, 32, 1, 1, 2, 0, 0)   \
  X(7, 8, 1, 1, 2, 16, 4, 0, 2, 0, 0)   \
  X(9, 2, 4, 2, 2, 32, 1, 1, 3, 0, 0)   \
  X(10, 2, 4, 2, 2, 32, 1, 1, 2, 1, 0)  \
  X(11, 2, 2, 2, 2, 32, 2, 1, 2, 1, 0)  \
  X(12, 2, 4, 4, 2, 32, 1, 0, 2, 1, 0)  \
  X(12, 2, 4, 4, 2, 32, 1, 0, 2, 1, 1) /* conv_il; not on NHWC4 A */
inline H2Route h2_tile_route(int cfg, bool il = false) {
#define RR_X(CFG, WM, WN, FM, FN, BK, MINB, MF16, NSTG, ACC1, IL) \
  if (cfg == CFG && il == (bool)IL) return {H2_TILE, CFG, WM, WN, FM, FN, BK, 0, 0, MF16, NSTG, ACC1 ? 1 : 2, IL};
  RR_H2_TILE_INSTANCES(RR_X)
#undef RR_X
  return {};  // (cfg 0: the launcher refuses it)
}
// config 8: config 4's tile as a persistent k-stream
inline H2Route h2_stream_route() { return {H2_STREAM, 8, 2, 4, 2, 2, 32, 0, 0, 1, 2, 2, 0, 1}; }
// config 15: the 256x256, 256x128 (N == 128) and 256x64 (N == 64, two accumulator sets) forms
inline H2Route h2_stream256_route(int n, long long chunk_rows) {
  H2Route r = n == 64    ? H2Route{H2_STREAM256, 15, 4, 2, 2, 1, 32, 0, 0, 0, 2, 2, 0, 1}
              : n == 128 ? H2Route{H2_STREAM256, 15, 2, 4, 4, 1, 32, 0, 0, 0, 2, 1, 0, 1}
                         : H2Route{H2_STREAM256, 15, 2, 4, 4, 2, 32, 0, 0, 0, 2, 1, 0, 1};
  r.chunk_rows = chunk_rows;
  return r;
}
// h2_halo.hip's instances: WM, WN, FM, FN, HR, TPK, MF, IL, PERS, T2 (its launcher reads this table)
#define RR_H2_HALO_INSTANCES(X)                                                                                  \
  X(2, 4, 4, 2, 288, 1, 0, 0, 0, 0)  /* 256x256, N % 256 == 0, W <= 15 (the 14x14 / 7x7 layers) */              \
  X(2, 4, 4, 2, 288, 1, 1, 0, 0, 0)  /*  on 16x16x32 */                                                          \
  X(2, 4, 4, 2, 288, 1, 1, 1, 0, 0)  /*  with its B DMA spread among the MFMAs */                                \
  X(4, 2, 2, 2, 320, 1, 0, 0, 0, 0)  /* 256x128, N % 128 == 0, W <= 31 (28x28) */                                \
  X(4, 2, 2, 2, 320, 1, 1, 0, 0, 0)  /*  on 16x16x32 */                                                          \
  X(4, 2, 2, 2, 320, 3, 1, 0, 2, 0)  /*  one halo buffer: its LDS holds three taps' B stages per barrier */      \
  X(4, 2, 2, 1, 384, 3, 0, 0, 0, 0)  /* 256x64, N % 64 == 0, W <= 63 (56x56), three taps per barrier */          \
  X(4, 2, 2, 1, 384, 3, 1, 0, 0, 0)  /*  on 16x16x32 */                                                          \
  X(4, 2, 2, 1, 384, 3, 0, 0, 1, 0)  /*  N == 64 as a persistent stream (one column tile) */                     \
  X(8, 1, 2, 2, 640, 3, 0, 0, 0, 0)  /* 512x64, N == 64, W <= 63: one halo buffer, waves of 64 x 64 */            \
  X(2, 4, 4, 2, 324, 1, 1, 0, 0, 16) /* 2-D, 16 x 16 outputs (18 x 18 halo rows), 256x256 */                     \
  X(4, 2, 2, 2, 324, 3, 1, 0, 2, 16) /* 2-D, 16 x 16 outputs, 256x128 (N == 128) */                              \
  X(8, 1, 2, 2, 640, 3, 0, 0, 0, 32) /* 2-D, 16 x 32 outputs (18 x 34 = 612 rows), 512x64 (N == 64) */
// configs 13 (32x32x16) / 14 (16x16x32): the halo tiles, one accumulator set
inline H2Route h2_halo_route(int wm, int wn, int fm, int fn, int hr, int tpk, int mf, int il = 0, int pers = 0, int t2 = 0) {
  return {t2 ? H2_HALO_2D : H2_HALO, mf ? 14 : 13, wm, wn, fm, fn, 32, hr, tpk, mf, 0, 1, il, pers, t2};
}

// The pick among the one-tile configs 3, 4 and 7.  N % 256 == 0: 4.  N % 128
// == 0: 3 (the 256x64 tiling has the same rounds there at 1 / 1.15 of the
// speed, and at least the bar's, so the cost rule always gave 3).  Ragged N:
// 3 where its rounds of resident blocks x tile area per CU / relative per-FLOP
// speed are below the bar -- the same area in 128x128 steps at two blocks per
// CU -- and no more than config 7's; else 7.
inline int h2_pick_tile(const GemmArgs& g) {
  if ((g.N % 256) == 0) return 4;
  if ((g.N % 128) == 0) return 3;
  auto cost = [&](long long bm, long long bn, long long per_cu, double speed) {
    const long long slots = 256 * per_cu;
    const long long t = ((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn);
    return (double)((t + slots - 1) / slots) * bm * bn * per_cu / speed;
  };
  const double bar = cost(128, 128, 2, 1.0), c3 = cost(256, 128, 1, 1.15), c7 = cost(256, 64, 2, 1.0);
  return (c3 < bar && c3 <= c7) ? 3 : 7;
}

// The routes forced 0 picks, first match wins (times per R101 layer at 1280 images unless noted)
//  dense A (1x1 stride 1)
//   15, 256x256  N % 256 == 0, K >= 256: 256->1024 + residual 0.704 -> 0.569 ms, 512->2048 0.513 -> 0.432
//                against 12 (profiles/r05f_cfg15_sweep.txt; the embed 70.49 -> 69.05 ms, r05f_cfg15_e2e.txt)
//   15, 256x128  N == 128, K >= 256 (profiles/r05ae_s3q128_ab/); 256x64: N == 64, K >= 64, config 7's
//                two accumulator sets (profiles/r05ah_s3q64_ab/, r05al_s3q64_acc2/)
//   15 in chunks A or C of 4 GB or more (its 32-bit byte offsets): chunks of a 256-row multiple; 256->64
//                at 128 x 256 x 192 1.738 -> 1.575 ms against 7 (profiles/r06ze_dense4gb_ab.txt)
//   8            N % 256 == 0, K < 256: the short-K residual expansions, 128->512 / 64->256 17 % / 8 %
//                faster than 12 (profiles/r03p_h2_cfg_sweep.txt); without a residual two accumulator
//                sets keep a K = 64 GEMM's error at the exact-fp32 core's (tests/test_gpu_h2.py)
//  3x3 stride 1 pad 1 (conv A)
//   2-D halo     no raster halo holds the map (halo_2d 1: wherever one serves; 0: never); N == 128
//                only at a block per CU, below that 11 spreads further: 35 blocks 0.040 -> 0.045 ms,
//                64 x 128@128x96 0.811 -> 0.685 (profiles/r06zb_halo2d_ab.txt)
//   halo 288     N % 256 == 0, W <= 15, 256x256 on 16x16x32: 256@14 0.716 -> 0.675 ms, 512@7 0.671 ->
//                0.606 (profiles/r04c_h2_cfg_sweep.txt); against 12 2.7 % / 1.6 % (r03t_h2_cfg_sweep.txt)
//   halo 320     N == 128, W <= 31, 256x128 on 16x16x32, one halo buffer, three taps per barrier:
//                128@28 1.035 -> 0.931 ms against 11 (profiles/r06w_halo128_ab.txt), 0.924 -> 0.897
//                against the two-buffer form (r06z2_halo128_sb_ab.txt; halo_mf 4 keeps that form)
//   halo 640     N == 64, W <= 63, the 512-row single-buffer tile: 64@56 1.193 -> 1.059 ms
//                (profiles/r06r_halo512_ab.txt) against the persistent 256-row stream (halo_mf 3;
//                1.212 -> 1.161 against the one-tile 256x64 form, r05w_sweep.txt, which s3_cfg 13 /
//                15 select; 32x32x16: 16x16x32 lost, 1.225 -> 1.334, r04c_h2_cfg_sweep.txt)
//   forced 13 / 14: the raster halo tile of g's N % 64 == 0 on 32x32x16 / 16x16x32; none serves: as forced 0
//  everything else, and a forced config on a shape it does not serve
//   12           N % 256 == 0, K >= 256 (conv A without a halo): 256@14 0.848 -> 0.794 ms, 2048->512
//                0.393 -> 0.350 against 4 (profiles/r03p_h2_cfg_sweep.txt); conv_il 1: its IL instance,
//                1-3 % faster alone, the embed 0.5 % slower (profiles/r04g_h2_cfg_il.txt, r04j_e2e_ab.txt)
//   11           N == 128: 4-7 % faster than 3 (profiles/r03l_h2_cfg_sweep.txt)
//   4 / 3 / 7    h2_pick_tile (7 against the 4-wave 256x64 tile: profiles/r02f_s3_cfg7.txt)
//  Forced 3, 4, 7: that tile.  Forced 8 to 12 and 15: that config where it serves the shape (8, 9, 10,
//  12: N % 256 == 0; 11: N % 128 == 0; 15: dense A, as picked), else 11 at N == 128, else h2_pick_tile.
//  Forced 1, 2, 5, 6 (no such tile): h2_pick_tile.
inline H2Route h2_route(int amode, const GemmArgs& g, const H2Tune& t) {
  int f = t.forced;
  if (amode == A_DENSE && (f == 0 || f == 15) && s3q_shape(g)) {
    if (s3q_fits(g)) return h2_stream256_route(g.N, 0);
    const long long per = ((1LL << 32) - 1) / (4LL * std::max(g.lda, g.ldc)) / 256 * 256;
    if (per >= 256) return h2_stream256_route(g.N, per);
  }
  const bool picked = f == 0;  // (a forced 15 is the pick from here on, but for the N = 64 halo form)
  if (f == 15) f = 0;
  if (amode == A_CONV) {
    if (f == 0 && t.halo_2d != 0 && h2_halo_2d_ok(g) &&
        (t.halo_2d == 1 || (h2_halo_2d_fills(g) && !h2_halo_rows(g)))) {
      if (g.N == 64) return h2_halo_route(8, 1, 2, 2, 640, 3, 0, 0, 0, 32);
      if (g.N == 128) return h2_halo_route(4, 2, 2, 2, 324, 3, 1, 0, 2, 16);
      return h2_halo_route(2, 4, 4, 2, 324, 1, 1, 0, 0, 16);
    }
    const int hr = h2_halo_rows(g);
    if (hr && (f == 13 || f == 14 || (f == 0 && ((g.N % 256) == 0 || g.N == 64 || g.N == 128)))) {
      const int form = f == 14 ? 1 : f == 13 ? 0 : t.halo_mf >= 0 ? t.halo_mf : (hr == 384 ? 0 : 1);
      const int mf = form == 1 || form == 4;
      if (hr == 288) return h2_halo_route(2, 4, 4, 2, 288, 1, mf, mf && t.conv_il == 1);
      if (hr == 320) return form == 1 ? h2_halo_route(4, 2, 2, 2, 320, 3, 1, 0, 2) : h2_halo_route(4, 2, 2, 2, 320, 1, mf);
      if (g.N == 64 && (form == 2 || (form == 0 && picked)) && 512 + 2 * (g.W + 1) <= 640)
        return h2_halo_route(8, 1, 2, 2, 640, 3, 0);
      if (g.N == 64 && !mf && (picked || form == 3)) return h2_halo_route(4, 2, 2, 1, 384, 3, 0, 0, 1);
      return h2_halo_route(4, 2, 2, 1, 384, 3, mf);
    }
  }
  if (f == 13 || f == 14) f = 0;  // no halo tile serves g: the pick
  const int pick = g.N == 128 ? 11 : h2_pick_tile(g);
  const bool il12 = t.conv_il == 1 && amode != A_CONV_C4;
  switch (f) {
    case 0:
      if ((g.N % 256) == 0 && g.K >= 256) return h2_tile_route(12, il12);
      [[fallthrough]];
    case 8: return s3_persist_ok(g, amode) ? h2_stream_route() : h2_tile_route(pick);
    case 3:
    case 4:
    case 7: return h2_tile_route(f);
    case 9:
    case 10: return h2_tile_route((g.N % 256) == 0 ? f : pick);
    case 11: return h2_tile_route((g.N % 128) == 0 ? 11 : pick);
    case 12: return (g.N % 256) == 0 ? h2_tile_route(12, il12) : h2_tile_route(pick);
    default: return h2_tile_route(h2_pick_tile(g));  // 1, 2, 5, 6
  }
}

}  // namespace rr
