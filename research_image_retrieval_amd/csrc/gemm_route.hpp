// gemm_route.hpp — which kernel instance serves a GEMM that goes through
// launch_gemm: the exact-fp32 core (gemm_f32.hip) and the bf16 / fp8 kernels
// (gemm_lp.hip, gemm_lpp.hip, gemm_8p.hip, sweep16.hip).  One pure host
// function, gemm_route: no HIP call, no handle, no pointer read (a pointer is
// only compared with null, and A / B are tested for 16-byte alignment).
// launch_gemm (gemm_f32.hip) launches exactly what it names; rr_gemm_route
// (rr.h) reports it, and tests/test_gemm_route.py holds its table for the
// project's own GEMMs on the CPU.
#pragma once

#include <algorithm>

#include "gemm_epilogue.hpp"
#include "rr_internal.hpp"

namespace rr {

enum GemmFamily {
  GF_NONE = -1,     // no instance serves it: launch_gemm reports hipErrorInvalidValue
  GF_F32 = 0,       // gemm_f32.hip, one tile per block
  GF_LP = 1,        // gemm_lp.hip, one tile per block
  GF_LPP = 2,       // gemm_lpp.hip, the persistent 256x256 k-stream
  GF_LPP3 = 3,      //  its three-A-stage form
  GF_8P = 4,        // gemm_8p.hip, the 256x256 8-phase pipeline
  GF_SWEEP128 = 5,  // sweep16.hip on 128-B LDS rows
  GF_SWEEP64 = 6    //  on 64-B rows
};

// One kernel instantiation.  The tuple is the kernel template's, as far as the
// family has the parameter (0 where it has not; epi -1).
struct GemmRoute {
  int family = GF_NONE;
  int cfg = 0;                         // fp32: 22 / 41 / 88; low precision: 1-5 (the k-streams 3, sweep16 4: their tile)
  int wm = 0, wn = 0, fm = 0, fn = 0;  // WM x WN waves of FM x FN 32x32 MFMA tiles
  int bk = 0, minb = 0;                // fp32: k-tile depth; blocks per CU (launch bounds)
  int gl = 0, mf16 = 0, il = 0;        // low precision: 1 LDS-DMA staging; 1 / 2: v_mfma_f32_16x16x32_bf16; DMA spread among the MFMAs
  int epi = -1;                        // the compiled-in epilogue flag set (gemm_epilogue.hpp EP_*); -1: read at run time
};

// rr_set_tuning's values that steer the route
struct GemmTune {
  int gemm_cfg = 0;     // fp32: 22, 41 or 88; 0 the pick
  int gemm_bk = 0;      // fp32 k-tile depth: 16 or 32; 0 the pick
  int lp_cfg = 0;       // low precision: 1-5 the configs below, 6 the three-A-stage k-stream; 0 the pick
  int sweep_form = -1;  // bf16 filter sweeps: 0 gemm_lp.hip's tiles, 1 / 2 sweep16.hip on 128-B / 64-B rows; -1 the pick
  int sweep_mf16 = -1;  // the 256x320 bf16 filter tile on 16x16x32 (1) or 32x32x16 (0); -1 the pick (0)
  int sweep_il = -1;    // filter sweeps: the next k-tile's DMA spread among the MFMAs (1) or one burst (0); -1 the pick
};
inline GemmTune gemm_tune(const rr_handle_s::Tuning& t) {
  return {t.gemm_cfg, t.gemm_bk, t.lp_cfg, t.sweep_form, t.sweep_mf16, t.sweep_il};
}

// ---- what launch_gemm rejects by shape alone (nullptr: nothing; M == 0 or N == 0 launches nothing) ----
inline const char* gemm_shape_error(int amode, int emode, int dt, const GemmArgs& g) {
  if (g.M < 0 || g.N < 0 || g.K <= 0) return "gemm: bad shape";
  if (dt != DT_F32) {
    if (amode != A_DENSE) return "gemm: low-precision GEMM needs dense A";
    const int vec = dt == DT_BF16 ? 8 : 16;  // elements per 16-B staging load
    if ((g.K % vec) || (g.lda % vec) || (g.ldb % vec)) return "gemm: low-precision K / lda / ldb must be multiples of 16 bytes";
    if (emode == E_SCORES_T && (g.ldc & 3)) return "gemm: ldc must be a multiple of 4";
    if (dt == DT_FP8 && emode == E_STORE) return "gemm: fp8 has no stored-C GEMM";
    return nullptr;
  }
  if (amode != A_CONV_GENERIC && (g.K & 3) != 0) return "gemm: K must be a multiple of 4";
  if (amode == A_DENSE && (g.lda & 3)) return "gemm: lda must be a multiple of 4";
  if (amode != A_CONV_GENERIC && (g.ldb & 3) != 0) return "gemm: ldb must be a multiple of 4";
  if (emode == E_SCORES_T && (g.ldc & 3)) return "gemm: ldc must be a multiple of 4";
  if (amode == A_CONV && (g.Cin % 32) != 0) return "gemm: A_CONV needs Cin % 32 == 0";
  if ((g.k_split > 0 || g.sym) && (amode != A_DENSE || emode != E_STORE))
    return "gemm: split-K / symmetric mode needs dense A and a stored C";
  if (g.k_split > 0 && (g.k_split % 32) != 0) return "gemm: k_split must be a multiple of 32";
  if (g.M > 0 && g.N > 0 && emode != E_STORE && amode != A_DENSE) return "gemm: unsupported mode combination";
  return nullptr;
}

// ---- the instances ----
// gemm_f32.hip's: config, WM, WN, FM, FN, BK, MINB, and the (AM, EM) it is compiled for.  BK = 32: 64 KB
// LDS per 128x128 block, 2 blocks (2 waves/SIMD) per CU; BK = 16: 32 KB, 3 blocks per CU, twice the barriers.
#define RR_GEMM_F32_INSTANCES(X)                                                      \
  X(22, 2, 2, 2, 2, 16, 3, true) /* 128x128, 4 waves of 64x64 */                       \
  X(41, 4, 1, 2, 2, 16, 3, true) /* 256x64 */                                          \
  X(22, 2, 2, 2, 2, 32, 2, true)                                                       \
  X(41, 4, 1, 2, 2, 32, 2, true)                                                       \
  X(88, 2, 4, 4, 2, 32, 1, EM == E_STORE && (AM == A_DENSE || AM == A_CONV)) /* 256x256, 8 waves of 128x64, 1 block per CU */
inline GemmRoute f32_tile_route(int AM, int EM, int cfg, int bk) {
#define RR_X(CFG, WM, WN, FM, FN, BK, MINB, WHEN) \
  if (cfg == CFG && bk == BK && (WHEN)) return {GF_F32, CFG, WM, WN, FM, FN, BK, MINB};
  RR_GEMM_F32_INSTANCES(RR_X)
#undef RR_X
  return {};
}
// gemm_lp.hip's: config, WM, WN, FM, FN, MINB, GL, MF16, IL, and the (EM, DT) it is compiled for
// (waves WM x WN, MFMA tiles per wave FM x FN, blocks per CU):
//   1: 128x128, 4 waves of 64x64, 2/CU      2: 256x64, 4 waves of 64x64, 2/CU
//   3: 256x256, 8 waves of 128x64, 1/CU (128 KB LDS) — the large GEMMs
//   4: 256x320, 8 waves of 64x160, 1/CU (144 KB) — a 320-query batch in one tile column: the streamed
//      gallery is read exactly once (bf16 filter and score sweeps only; fp8's 256x320 form spills the
//      dequantisation)
//   (5: 256x256 on the 8-phase LDS-DMA pipeline of gemm_8p.hip)
// bf16 runs on four v_mfma_f32_16x16x32_bf16 per 32x32 tile (MF16 1; measured: ViT-B/16 linears +4-7 %,
// 128x128 cosine sweeps +2-5 % over 32x32x16), except the 256x320 sweep tile, whose 16x16 fragments
// spill (180 B/lane) in that form; MF16 2 is its own 16x16x32 form.  Configs 3 and 4 stage by LDS-DMA
// (GL 1): whole k-tiles only.
#define RR_GEMM_LP_INSTANCES(X)                                       \
  X(1, 2, 2, 2, 2, 2, 0, 1, 0, DT == DT_BF16)                         \
  X(1, 2, 2, 2, 2, 2, 0, 0, 0, DT == DT_FP8)                          \
  X(2, 4, 1, 2, 2, 2, 0, 1, 0, DT == DT_BF16)                         \
  X(2, 4, 1, 2, 2, 2, 0, 0, 0, DT == DT_FP8)                          \
  X(3, 2, 4, 4, 2, 1, 1, 1, 0, DT == DT_BF16)                         \
  X(3, 2, 4, 4, 2, 1, 1, 0, 0, DT == DT_FP8)                          \
  X(3, 2, 4, 4, 2, 1, 1, 1, 1, DT == DT_BF16 && EM == E_FILTER)       \
  X(3, 2, 4, 4, 2, 1, 1, 0, 1, DT == DT_FP8 && EM == E_FILTER)        \
  X(4, 4, 2, 2, 5, 1, 1, 0, 0, DT == DT_BF16 && EM != E_STORE)        \
  X(4, 4, 2, 2, 5, 1, 1, 0, 1, DT == DT_BF16 && EM == E_FILTER)       \
  X(4, 4, 2, 2, 5, 1, 1, 2, 0, DT == DT_BF16 && EM == E_FILTER)       \
  X(4, 4, 2, 2, 5, 1, 1, 2, 1, DT == DT_BF16 && EM == E_FILTER)
// The epilogue flag sets compiled into the bf16 stored-C kernels (the ViT linears: QKV bias -> bf16,
// out-proj / fc2 bias + residual, fc1 bias + QuickGELU -> bf16, and the LayerNorm fold's producer and
// consumers): flags, FOLD (1: of gemm_lp.hip's tiles only the 256-column MF16 1 one has it), A3 (1: the
// three-A-stage k-stream has it; the fold's consumers need its LDS).  The k-stream of gemm_lpp.hip has
// all six; gemm_lp.hip's tiles read any other set at run time (EPI -1).
#define RR_GEMM_EPI_SETS(X)                       \
  X(EP_BIAS | EP_BF16, 0, 1)                      \
  X(EP_BIAS | EP_RES, 0, 1)                       \
  X(EP_BIAS | EP_GELU | EP_BF16, 0, 1)            \
  X(EP_BIAS | EP_RES | EP_STATS, 1, 1)            \
  X(EP_BIAS | EP_BF16 | EP_LNFOLD, 1, 0)          \
  X(EP_BIAS | EP_GELU | EP_BF16 | EP_LNFOLD, 1, 0)
// the compiled-in set that serves flag set f, -1: none (a3: of the three-A-stage form; no_fold: of a
// tile without the fold)
inline int gemm_epi_set(int f, bool a3 = false, bool no_fold = false) {
#define RR_X(FLAGS, FOLD, A3) \
  if (f == (FLAGS) && (!a3 || A3) && (!no_fold || !FOLD)) return f;
  RR_GEMM_EPI_SETS(RR_X)
#undef RR_X
  return -1;
}
inline GemmRoute lp_tile_route(int EM, int DT, const GemmArgs& g, int cfg, int mf16, int il) {
  GemmRoute r;
#define RR_X(CFG, WM, WN, FM, FN, MINB, GL, MF16, IL, WHEN) \
  if (cfg == CFG && mf16 == MF16 && il == IL && (WHEN)) r = {GF_LP, CFG, WM, WN, FM, FN, 0, MINB, GL, MF16, IL, -1};
  RR_GEMM_LP_INSTANCES(RR_X)
#undef RR_X
  if (r.family == GF_LP && EM == E_STORE) {
    const int f = ep_flags(g);
    r.epi = gemm_epi_set(f, false, !(32 * r.fn * r.wn == 256 && r.mf16 == 1));
    if (r.epi < 0 && (f & (EP_STATS | EP_LNFOLD))) return {};  // the fold has no run-time form
  }
  return r;
}

// ---- shape predicates of the kernels beside the one-tile ones ----
// gemm_lpp.hip: the bf16 stored-C GEMM as a persistent 256x256 k-stream, for the compiled-in flag sets
inline bool lpp_eligible(const GemmArgs& g) {
  return g.M > 0 && (g.N % 256) == 0 && (g.K % 64) == 0 && g.K <= 1024 && g.k_split <= 0 && !g.sym &&
         gemm_epi_set(ep_flags(g)) >= 0;
}
inline bool lpp3_eligible(const GemmArgs& g) {
  return g.M > 0 && (g.N % 256) == 0 && (g.K % 64) == 0 && g.k_split <= 0 && !g.sym && gemm_epi_set(ep_flags(g), true) >= 0;
}
// gemm_8p.hip: dense A and B, K a multiple of two k-tiles (bf16 128, fp8 256), 16-B aligned rows, no
// split-K / symmetric; row scales only for fp8
inline bool gemm_8p_eligible(const GemmArgs& g, int dt) {
  const int ktp = dt == DT_FP8 ? 256 : 128;
  return (dt == DT_BF16 || dt == DT_FP8) && (g.K % ktp) == 0 && g.k_split == 0 && !g.sym &&
         (dt == DT_FP8 || (g.scale_a == nullptr && g.scale_b == nullptr)) && (((uintptr_t)g.A | (uintptr_t)g.B) & 15) == 0;
}
// sweep16.hip: 256 gallery rows x 320 queries per block; unscaled bf16 rows, 32-bit byte offsets within a tile
constexpr int SW_BM = 256, SW_BN = 320;
inline bool sweep16_eligible(const GemmArgs& g) {
  return g.K > 0 && (g.K % 32) == 0 && (g.lda % 8) == 0 && (g.ldb % 8) == 0 && g.scale_a == nullptr &&
         g.scale_b == nullptr && ((uintptr_t)g.A & 15) == 0 && ((uintptr_t)g.B & 15) == 0 &&
         (long long)SW_BM * g.lda * 2 < (1LL << 31) && (long long)SW_BN * g.ldb * 2 < (1LL << 31);
}

// fp32 k-tile depth.  Measured on MI355X (same device, interleaved A/B): BK = 16 (3 blocks per CU) is
// +2.5 % on the long-K, huge-grid cosine GEMM, BK = 32 (2 blocks per CU) is +4.8 % on the ResNet convs.
inline int f32_pick_bk(int emode, const GemmTune& t) {
  if (t.gemm_bk == 16 || t.gemm_bk == 32) return t.gemm_bk;
  return emode == E_STORE ? 32 : 16;
}
// The low-precision cost model: rounds x tile area / relative per-FLOP speed (a round of `slots`
// resident blocks lasts ~ tile area x blocks per CU), over configs 1-5.
inline int lp_pick_cfg(const GemmArgs& g, int emode, bool bf16) {
  auto cost = [&](long long bm, long long bn, long long slots, double speed) {
    const long long t = ((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn);
    return (double)((t + slots - 1) / slots) * bm * bn * (slots / 256) / speed;
  };
  double best = cost(128, 128, 512, 1.0);
  int cfg = 1;
  if (cost(256, 64, 512, 1.0) < best) best = cost(256, 64, 512, 1.0), cfg = 2;
  if (emode == E_STORE && cost(256, 256, 256, 1.25) < best) best = cost(256, 256, 256, 1.25), cfg = 3;
  if (emode == E_FILTER && (g.K < 1024 || g.scale_a != nullptr) && cost(256, 256, 256, 1.25) < best)
    best = cost(256, 256, 256, 1.25), cfg = 3;
  if (emode != E_STORE && g.K >= 1024 && g.scale_a == nullptr && cost(256, 320, 256, 1.35) < best)
    best = cost(256, 320, 256, 1.35), cfg = 4;
  if (emode != E_STORE && bf16 && g.K >= 1024 && (g.K % 128) == 0 && cost(256, 256, 256, 1.35 * 1.03) < best * 0.97)
    best = cost(256, 256, 256, 1.35 * 1.03), cfg = 5;
  return cfg;
}

// Picked when, first match wins.
//  fp32 (gemm_f32.hip; every config is 4 waves and 2 (BK 32) or 3 (BK 16) blocks per CU but 88)
//   BK           gemm_bk 16 / 32, else 32 for a stored C and 16 for the rankers (f32_pick_bk)
//   gemm_cfg 22 / 41: that tile.  88: 88 at BK 32 with a stored C, else 22.
//   88, 256x256  stored C, no split-K, no residual, K >= 1024, N % 256 == 0, BK 32, t88 = tiles >= 240 (~a
//                full round of one block per CU) and its rounds x area / 1.05 below twice the better of
//                22 and 41 (per CU: 1 block against 2).  Measured per R101 layer: +3-7 % on long-K GEMMs
//                without a residual (3x3 256@14, 1024->512/2048), -5..-30 % on residual epilogues and
//                short K, -40 % when the grid leaves CUs idle.  Only dense and conv A have the
//                instance: the generic-gather and NHWC4 A modes run 22 where 88 is picked or forced.
//   41 / 22      the lower rounds x tile area, rounds = ceil(tiles / slots), slots 512 (BK 16: 768): this
//                charges both the padding of N (e.g. 320 queries on 128-wide tiles) and the last
//                partially-filled round (wave quantization); 22 on a tie
//  bf16 stored C (the ViT linears)
//   lpp3         the flag sets without the fold's consumers, N % 256 == 0, K % 64 == 0, no split-K / sym, K <=
//                1024 (lp_cfg 6: at any K): out-proj 0.579 -> 0.546 ms against the two-stage form
//                (r05u_vitlin.txt); at K = 3072 (c_proj) it ran 1.313 ms against the one-tile kernel's
//                1.257, so lp_cfg 6 (tests) is the only way there.  Per block of linears 4.51 -> 4.35 ms
//                (profiles/r05u_vitlin.txt)
//   lpp          lp_cfg 0 / 6, the six flag sets, the same shapes, K <= 1024 (c_proj, K = 3072, ran 11 %
//                slower than the one-tile kernel): the C4 embed 62.29 -> 61.54 ms (r05q_e2e_c4.txt).
//                lp_cfg 3 forces the one-tile kernel
//  low precision, the config: lp_cfg 1-3; 4 and 5 for the sweeps (3 for a stored C); else lp_pick_cfg
//   (measured, tools/lp_bench.py: the 8-wave tiles run ViT linears 1.2-1.3x faster than 128x128; the
//   320-query tile runs the bf16 d=2048 sweep 1.35x faster, but not d=512 or fp8, where 4-wave tiles win):
//   3            stored C; and filter sweeps with K < 1024 or row scales, where the 8-wave 256x256 tile
//                wins at >= 1024 queries (measured at 1280 queries x 1.6 M rows: bf16 d = 512 3.27 -> 2.39
//                ms, fp8 d = 2048 11.2 -> 8.1 ms per C5 step); at 320 queries the cost model keeps 128x128
//   4            sweeps with K >= 1024 and no row scales
//   5            bf16 sweeps, K >= 1024, K % 128 == 0, where it wins by padding: measured (tools/sweep_ab.py,
//                random queries x 1.6 M x 2048) 1.22-1.25x the 256x320 tile at 256 / 512 / 768 queries
//                (no padded query columns), 1.03x at 1280 and slower at 320 (256 + 64 padded)
//   Not kept: the 8-phase pipeline for the ViT linears (2-4 % slower: short K) and the
//   256x320 tile on a 4-stage 64-B-row LDS-DMA ring (7.59 vs 6.94 ms per C3 sweep).
//   Then: the LayerNorm fold (stats_in / stats_out) takes 3, its 256-column tiles; 3 and 4 on a partial
//   k-tile (K % 64 bf16, K % 128 fp8) take 1: the LDS-DMA staging has no zero fill.
//  bf16 filter sweeps
//   sweep16      sweep_form 1 / 2 (128-B rows at K % 64 == 0, else and for 2 the 64-B rows), else K >= 1024
//                with K % 64 == 0 (the C3 prefilter's 1.6 M x 2048 sweep), where sweep16_eligible.
//                Measured against the 256x320 tile (tools/prefilter_ab.py, 1280 queries,
//                profiles/r06m_*): random queries 9.57 -> 7.26 ms, near-parallel 7.39 -> 7.04, and 6.86 ->
//                7.01 on identical queries (the bench's random-weight descriptors); at K = 512 (C4) 2.43
//                -> 2.49 ms, so short K keeps the tile
//  sweeps, config 5
//   8-phase      where gemm_8p_eligible; else config 3 -- and config 1 on a partial k-tile.  The parent of
//                this table applied the k-tile rule only before this fallback, so a forced lp_cfg 5 at
//                bf16 K % 64 != 0 or fp8 K % 128 != 0 reached the LDS-DMA tile, whose staging reads whole
//                128-B rows past K (gemm_lp_kernel glds_tile): the one deliberate change of route
//  filter sweeps, the form of configs 3 and 4
//   IL           sweep_il 1, or -1 on the 256x320 bf16 tile and on fp8: the next k-tile's DMA spread among
//                the MFMAs.  On the C3 bench's own descriptors (tools/e2e_ab.py,
//                profiles/r04j_e2e_ab.txt): 7.15 -> 6.81 ms; the 16x16x32 form is 7.71 ms there (7.08 with
//                the spread), though it won on synthetic near-parallel queries (r04f_sweep_il_ab.txt).
//                C5's fp8 sweeps 7.70 -> 7.53 ms per step on the bench (profiles/r04k_c5_*.json).  On the
//                ViT linears' stored-C tile it made the C4 embed slower, 61.3 -> 62.4 ms
//                (profiles/r04k_e2e_c4_il.txt), and was removed.  fp8 under a forced lp_cfg 4 runs the
//                256x256 tile without it.  Bit-identical rankings in every form
//   MF16 2       sweep_mf16 1, the 256x320 bf16 filter tile only
//  the epilogue: a bf16 stored C takes the compiled-in set that matches its flags (RR_GEMM_EPI_SETS),
//  else the run-time form; a fold flag set without a compiled-in instance has no route (GF_NONE)
inline GemmRoute gemm_route(int amode, int emode, int dt, const GemmArgs& g, const GemmTune& t) {
  if (dt == DT_F32) {
    const int bk = f32_pick_bk(emode, t);
    int cfg = t.gemm_cfg;
    if (cfg == 88 && !(emode == E_STORE && bk == 32)) cfg = 22;
    if (cfg == 0) {
      const long long slots = bk == 16 ? 768 : 512;
      const long long t22 = ((g.M + 127) / 128) * ((g.N + 127) / 128);
      const long long t41 = ((g.M + 255) / 256) * ((g.N + 63) / 64);
      const long long c22 = ((t22 + slots - 1) / slots) * 128 * 128;
      const long long c41 = ((t41 + slots - 1) / slots) * 256 * 64;
      cfg = c41 < c22 ? 41 : 22;
      if (emode == E_STORE && g.k_split == 0 && g.residual == nullptr && g.K >= 1024 && (g.N % 256) == 0 && bk == 32) {
        const long long t88 = ((g.M + 255) / 256) * (g.N / 256);
        const long long c88 = ((t88 + 255) / 256) * 256 * 256;
        if (t88 >= 240 && (double)c88 / 1.05 < (double)std::min(c22, c41) * 2.0) cfg = 88;
      }
    }
    if (cfg == 88 && amode != A_DENSE && amode != A_CONV) cfg = 22;
    return f32_tile_route(amode, emode, cfg, bk);
  }
  const bool bf16 = dt == DT_BF16;
  if (bf16 && emode == E_STORE) {
    const int f = ep_flags(g);
    if (lpp3_eligible(g) && (t.lp_cfg == 6 || (t.lp_cfg == 0 && g.K <= 1024))) return {GF_LPP3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, f};
    if ((t.lp_cfg == 0 || t.lp_cfg == 6) && lpp_eligible(g)) return {GF_LPP, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, f};
  }
  const int epr = bf16 ? 64 : 128;  // elements per 128-B k-tile row
  int cfg = t.lp_cfg >= 1 && t.lp_cfg <= 3              ? t.lp_cfg
            : t.lp_cfg == 4 || t.lp_cfg == 5            ? (emode == E_STORE ? 3 : t.lp_cfg)
                                                        : lp_pick_cfg(g, emode, bf16);
  if (g.stats_out != nullptr || g.stats_in != nullptr) cfg = 3;
  if ((cfg == 3 || cfg == 4) && (g.K % epr) != 0) cfg = 1;
  if (emode == E_FILTER && bf16) {
    const int form = t.sweep_form >= 0 ? t.sweep_form : (g.K >= 1024 && (g.K % 64) == 0 ? 1 : 0);
    if ((form == 1 || form == 2) && sweep16_eligible(g))
      return {form == 1 && (g.K % 64) == 0 ? GF_SWEEP128 : GF_SWEEP64, 4};
  }
  const bool mf16_sweep = emode == E_FILTER && t.sweep_mf16 > 0;
  const bool spread = emode == E_FILTER && (t.sweep_il > 0 || (t.sweep_il < 0 && ((cfg == 4 && bf16) || !bf16)));
  if (cfg == 5) {
    if (emode != E_STORE && gemm_8p_eligible(g, dt)) return {GF_8P, 5};
    cfg = (g.K % epr) != 0 ? 1 : 3;
  }
  if (cfg == 4 && !bf16) return lp_tile_route(emode, dt, g, 3, 0, 0);
  if (cfg == 4) return lp_tile_route(emode, dt, g, 4, mf16_sweep ? 2 : 0, spread);
  return lp_tile_route(emode, dt, g, cfg, bf16, cfg == 3 && spread);
}

}  // namespace rr
