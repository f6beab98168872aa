// h2_halo.hip — halo-staged A for stride-1 3x3 convolutions (configs 13 / 14)
// of the f16x2 split GEMM core (h2_tile.hip: the split and the tile table).
//
// The implicit-GEMM A loader of gemm_s3_kernel (h2_tile.hip) fetches every input pixel once
// per filter tap: nine fetches of each activation on a 3x3 conv.  Every tile
// here on this chip is bound by the bytes each CU fetches per MFMA cycle
// (the per-CU fill rate), and on the 3x3 256@14 layer the A operand
// is half of them: per output, 4 K / Nt B of A plus 4 K / Mt B of B planes =
// 36 + 36 B at the 256x256 tile.  Here a 256-row tile (256 consecutive output
// pixels in NHWC raster order) loads, per 32-channel slice of Cin, the raster
// range of input pixels its nine taps can touch — 256 + 2 (W + 1) rows, one
// fetch each — splits it once into the two fp16 planes of an LDS halo buffer,
// and runs the slice's nine k-tiles (one per tap) on it: output row r reads
// halo row r + kh W + kw, or a zero row when the tap falls outside its image
// (padding) or r is past M.  A fetch per output drops to (256 + 2W + 2) / 256
// x 4 Cin / Nt (4.5 B at 256@14), the split VALU to one per slice instead of
// one per k-tile.  k order: slice-major, tap-minor (k-tile (c, t) = weight
// columns t Cin + 32 c ..); B planes by LDS-DMA one k-tile ahead as config 12;
// 256x256 tile, 8 waves of 128x64 on v_mfma_f32_32x32x16_f16, one accumulator
// set (ACC1, config 12's arithmetic per product); the next slice's halo goes
// to the other buffer one 128-row pass per k-tile during the slice's first
// four.  Instances (waves WM x WN of FM x FN 32x32 tiles, halo rows HR): the
// table RR_H2_HALO_INSTANCES in h2_route.hpp; the 256x64 tile takes three taps
// per k-step (and barrier): its 12 MFMAs per wave and tap are too few to
// carry a barrier each.  Row HR of each halo plane is the zero row.
// Halo rows are read 32 at a time from any row offset r0 + kh W + kw, not from
// 32-aligned groups, so the row-group swizzle of the other tiles (pswz<32>)
// conflicts there (PMC: 3.5e7 SQ_LDS_BANK_CONFLICT on the 3x3 256@14 layer,
// profiles/r03pmc_layer3_sq_counters.txt).  slot ^ ((row >> 2) & 3) keeps every
// ds_read_b128 lane group on 16 distinct bank quads for every offset: the four
// rows of a group that share row & 3 differ by {0, 12, 20, 24} or {4, 8, 16,
// 28}, whose (row >> 2) & 3 are four distinct values whatever the offset.
#include <algorithm>

#include "h2_common.hpp"
#include "h2_route.hpp"

namespace rr {

__device__ __forceinline__ int hswz(int row, int slot) { return slot ^ ((row >> 2) & 3); }

// MF = 1: v_mfma_f32_16x16x32_f16 (one 32-deep k-step per k-tile; each 32x32
// tile of a wave is four 16x16 sub-tiles, the acc_row / acc_col<true> map),
// which the chip holds at a higher clock than 32x32x16 in MFMA-dense loops
// (MI355X_MICROARCH.md 'DVFS give-back' item 7; profiles/r04b_fetch_ceiling.txt:
// register-only 0.875 vs 0.725 of the bf16 peak at two waves per SIMD).  A row
// half's A fragments are read once, the B fragments once per row half.
// IL (16x16x32, one tap per barrier): the next k-tile's B DMA goes out one
// instruction at a time among the k-tile's first MFMAs instead of as one
// burst before them (the halo pass load stays at the top: it comes from HBM).
// T2 (round 6): 2-D block tiles for maps too wide for a raster halo.  The
// tile is TH x T2 output pixels of one image (TH = BM / T2); its halo is the
// (TH + 2) x (T2 + 2) input block around them, out-of-image pixels loaded as
// zeros, so every tap of an in-map row is live (no tap masks) and output row
// r = (oy, ox) reads halo row (oy + kh)(T2 + 2) + ox + kw; rows outside the
// map are neither computed from (the zero row) nor stored (Rows2D).  Same
// products in the same order as the raster tile: bit-identical to it.
template <int EPI, int WM, int WN, int FM, int FN, int HALO_HR, int TPK = 1, int MF = 0, int IL = 0, int PERS = 0,
          int T2 = 0>
__global__ __launch_bounds__(512, 1) void gemm_h2_halo_kernel(GemmArgs g, int tiles_n) {
  constexpr int NP = 2, BK = 32, NT = 512, NW = 8;
  constexpr int WTM = 32 * FM, WTN = 32 * FN, BM = WTM * WM, BN = WTN * WN, SL = BK / 8;
  static_assert(WM * WN == NW && (BM == 256 || BM == 512), "8 waves, 256- or 512-row tiles");
  // SB (the 512-row tile): ONE halo buffer.  The next slice's passes wait in
  // registers through the slice's taps and are split into the buffer at the
  // top of the next slice, behind a barrier of their own.
  // (PERS 2: the one-tile form with one halo buffer at 256 rows too: room for
  // three taps' B stages per barrier where two halo buffers left none)
  constexpr bool SB = BM == 512 || PERS == 2;
  constexpr bool PST = PERS == 1;  // the persistent stream
  static_assert(!SB || (!PST && !IL && (BM == 256 || !MF)), "single-buffer halo: the one-tile form");
  constexpr int NHB = SB ? 1 : 2;  // halo buffers
  constexpr int TH = T2 ? BM / T2 : 1, HWD = T2 + 2;  // T2: the tile's output rows, the halo's width
  constexpr int NHR = T2 ? (TH + 2) * HWD : HALO_HR;   // halo rows a tile loads
  static_assert(!T2 || (BM % T2 == 0 && T2 % (MF ? 16 : 32) == 0 && NHR <= HALO_HR && !PST && !IL), "2-D tile");
  constexpr int HRA = HALO_HR + 1;                  // rows per A plane (+ the zero row)
  constexpr int A_EL = NP * HRA * BK;               // u16 per halo buffer
  constexpr int B_TAP = NP * BN * BK;               // u16 of one tap's B planes
  constexpr int B_EL = TPK * B_TAP;                 // u16 per B stage (TPK taps per barrier)
  constexpr int B_RPI = 64 / SL;                    // plane rows per LDS-DMA wave instruction
  constexpr int B_INS = NP * BN / B_RPI / NW;       // LDS-DMA instructions per wave per k-tile (4 / 2 / 1)
  constexpr int A_PASS = (HALO_HR + NT / SL - 1) / (NT / SL);  // 128-row passes over the halo (3)
  constexpr int LDS_U16 = NHB * A_EL + 2 * B_EL;
  static_assert(B_INS * NW * B_RPI == NP * BN, "B staging must tile the block");
  __shared__ __attribute__((aligned(16))) uint16_t lds[LDS_U16];
  typedef f16x8 frag_t;

  const uint32_t a_amax_w = amax_load_slot(g.a_amax);
  float a_sc = 1.f, a_isc = 1.f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int lr = lane & 31, lh = lane >> 5;

  static_assert(!PST || (TPK > 1 && !IL), "persistent halo tile: the all-passes-at-once instance");
  const int nwg = gridDim.x, bid = blockIdx.x;
  // PERS: one block per CU walks the row tiles bid + t nwg (tiles_n == 1, so
  // the weights never change), remapped per virtual block as config 8 / 15
  const int ntiles = PST ? (g.M + BM - 1) / BM * tiles_n : nwg;
  auto tile_m0 = [&](int tl) __attribute__((always_inline)) {
    const int v = bid + tl * nwg;
    const int xcd = v & 7, q8 = ntiles >> 3, r8 = ntiles & 7;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (v >> 3);
    return (wgid / tiles_n) * BM;
  };
  int m0, n0;
  {
    const int xcd = bid & 7, q8 = ntiles >> 3, r8 = ntiles & 7;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    m0 = (wgid / tiles_n) * BM;
    n0 = (wgid % tiles_n) * BN;
  }
  // 3x3 only (h2_halo_rows): the tap -> (kh, kw) split and the group count
  // are compile-time constants
  const int W = g.W, H = g.H;
  constexpr int KW = 3, KH = 3, ntap = KH * KW;
  const int nch = g.Cin / BK, ngrp = ntap / TPK, nk = nch * ngrp;  // k-step kt = (slice, group of TPK taps)
  const int hoff = g.pad * W + g.pad;  // halo row 0 = input raster index m0 - hoff
  // T2: the tile's image (its first output row) and top-left output pixel
  int t_img = 0, t_y0 = 0, t_x0 = 0;
  if constexpr (T2 != 0) {
    const int mt = m0 / BM, tx_n = (W + T2 - 1) / T2, tpi = (H + TH - 1) / TH * tx_n;
    const int im = mt / tpi, rem = mt - im * tpi, ty = rem / tx_n;
    t_img = im * H * W;
    t_y0 = ty * TH;
    t_x0 = (rem - ty * tx_n) * T2;
  }
  // the halo row (tap (0, 0)) of tile row rb + l (rb a multiple of the
  // fragment height, l below it, so l stays an offset: T2 % 32 == 0 for the
  // 32x32 fragments), and the halo-row step of kh
  auto hrow = [&](int rb, int l) __attribute__((always_inline)) { return T2 ? (rb / T2) * HWD + rb % T2 + l : rb + l; };
  const int tstep = T2 ? HWD : W;

  // ---- halo loader: thread -> (row t / 4 + 128 pass, 16-B slot pair t % 4);
  // one 128-row pass at a time (8 registers), so the halo of the next slice
  // never holds more than one pass beside the accumulators ----
  // (TPK > 1: the narrow tiles have the registers to hold every pass at once)
  const int a_slot = tid % SL, a_row = tid / SL;
  constexpr int RA_N = (TPK == 1 && !SB) ? 1 : A_PASS;
  f32x4 ra[RA_N][2];
  auto load_pass_to = [&](int c, int p, f32x4(&r)[2], int mb) {
    const int hr = a_row + p * (NT / SL);
    long long q;
    bool ok;
    if constexpr (T2 != 0) {
      // (from an opaque row: hoisted out of the k-loop, the three passes'
      // addresses and bounds would be held beside the accumulators)
      const int ho = s3_opaque(hr), hy = ho / HWD, iy = t_y0 - 1 + hy, ix = t_x0 - 1 + (ho - hy * HWD);
      q = (long long)t_img + iy * W + ix;
      ok = hr < NHR && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    } else {
      q = (long long)mb - hoff + hr;
      ok = hr < HALO_HR && q >= 0 && q < g.M;
    }
    const f32x4* src = ok ? reinterpret_cast<const f32x4*>(g.A + q * g.Cin + c * BK + a_slot * 8) : s3_zero_page();
    s3_load2<1>(src, r);
  };
  auto load_pass = [&](int c, int p) { load_pass_to(c, p, ra[RA_N == 1 ? 0 : p], m0); };
  auto launder_pass = [&]() {
#pragma unroll
    for (int p = 0; p < RA_N; ++p) {
      s3_launder(ra[p][0]);
      s3_launder(ra[p][1]);
    }
  };
  auto store_pass_from = [&](int buf, int p, const f32x4(&r)[2]) {
    const int hr = a_row + p * (NT / SL);
    u32x4 p0, p1;
    split2h8(r, a_sc, p0, p1);
    if (hr < HALO_HR) {
      uint16_t* la = lds + buf * A_EL;
      const int off = hr * BK + hswz(hr, a_slot) * 8;
      *reinterpret_cast<u32x4*>(la + off) = p0;
      *reinterpret_cast<u32x4*>(la + HRA * BK + off) = p1;
    }
  };
  auto store_pass = [&](int buf, int p) { store_pass_from(buf, p, ra[RA_N == 1 ? 0 : p]); };

  // ---- B planes: LDS-DMA, instruction i of a wave fills plane rows
  // prow = (i NW + wave) B_RPI + lane / 4 of the [2][BN] stage (N % BN == 0:
  // every row real).  256 columns: plane i / 2, rows 128 (i & 1) + prow % 128
  // off one pointer (rows r and r + 128 share their swizzle); narrower tiles
  // keep a pointer per instruction ----
  const int b_r = wave * B_RPI + lane / SL;
  const uint16_t* Bp = reinterpret_cast<const uint16_t*>(g.B);
  static_assert(NW * B_RPI == 128, "one DMA round = 128 plane rows");
  const uint16_t* b_src[BN == 256 ? 1 : B_INS];
  if constexpr (BN == 256) {
    b_src[0] = Bp + (long long)(n0 + b_r) * g.ldb + pswz<BK>(b_r, lane % SL) * 8;
  } else {
#pragma unroll
    for (int i = 0; i < B_INS; ++i) {
      const int prow = i * 128 + b_r, p = prow / BN, r = prow - p * BN;
      b_src[i] = Bp + p * g.b_plane + (long long)(n0 + r) * g.ldb + pswz<BK>(r, lane % SL) * 8;
    }
  }
  auto glds_b = [&](int kt, int buf) {
    const int c = kt / ngrp, t0 = (kt - c * ngrp) * TPK;
#pragma unroll
    for (int u = 0; u < TPK; ++u) {
      const long long koff = (long long)(t0 + u) * g.Cin + c * BK;
      uint16_t* lb = lds + NHB * A_EL + buf * B_EL + u * B_TAP;
#pragma unroll
      for (int i = 0; i < B_INS; ++i) {
        const uint16_t* src = BN == 256 ? b_src[0] + (i >> 1) * g.b_plane + (long long)(i & 1) * (BN / 2) * g.ldb
                                        : b_src[BN == 256 ? 0 : i];
        __builtin_amdgcn_global_load_lds((const void*)(src + koff),
                                         (__attribute__((address_space(3))) void*)(lb + (i * NW + wave) * B_RPI * BK),
                                         16, 0, 0);
      }
    }
  };

  static_assert(!IL || (MF && TPK == 1 && B_INS <= FM * FN), "IL: the 16x16x32 one-tap-per-barrier tile");
  // IL: DMA instruction i of glds_b(kt, buf), before a0b0 MFMA number
  // i * IL_STEP of the k-tile's first (row half, column half) block
  constexpr int IL_STEP = (FM * FN) / B_INS;
  auto glds_b_due = [&](int kt, int buf, int idx) {
    if constexpr (IL) {
      const int c = kt / ngrp, t0 = kt - c * ngrp;
      const long long koff = (long long)t0 * g.Cin + c * BK;
      uint16_t* lb = lds + NHB * A_EL + buf * B_EL;
#pragma unroll
      for (int i = 0; i < B_INS; ++i) {
        if (i * IL_STEP != idx) continue;
        const uint16_t* src = BN == 256 ? b_src[0] + (i >> 1) * g.b_plane + (long long)(i & 1) * (BN / 2) * g.ldb
                                        : b_src[BN == 256 ? 0 : i];
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_global_load_lds((const void*)(src + koff),
                                         (__attribute__((address_space(3))) void*)(lb + (i * NW + wave) * B_RPI * BK),
                                         16, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  // ---- the lanes' fragment rows: a 9-bit mask of the taps that stay inside
  // the row's image (bit kh KW + kw), empty past M ----
  // (MF: the lane's rows are i * 32 + 16 a + (lane & 15), a = 0, 1)
  constexpr int RPT = MF ? 2 : 1;
  const int l16 = lane & 15, lg = lane >> 4;
  int tmask[FM][RPT];
  auto masks = [&](int mb) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int a = 0; a < RPT; ++a) {
        const int m = mb + wm * WTM + i * 32 + (MF ? 16 * a + l16 : lr);
        if constexpr (T2 != 0) {
          // every tap reads the halo (zeros off the image); rows off the map
          // compute from it too, finite, and are not stored (Rows2D)
          tmask[i][a] = (1 << ntap) - 1;
          continue;
        }
        const int rem = m % (H * W), oh = rem / W, ow = rem - oh * W;
        int mk = 0;
        for (int kh = 0; kh < KH; ++kh)
          for (int kw = 0; kw < KW; ++kw)
            if ((unsigned)(oh + kh - g.pad) < (unsigned)H && (unsigned)(ow + kw - g.pad) < (unsigned)W)
              mk |= 1 << (kh * KW + kw);
        tmask[i][a] = m < g.M ? mk : 0;
      }
  };
  masks(m0);

  f32x16 acc[FM][FN];
  f32x4 acc4[MF ? FM : 1][MF ? FN : 1][4];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  if constexpr (MF) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc4[i][j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // one k-tile: tap t of halo buffer hb, B stage bs; two 16-deep k-steps, each
  // a0b0 first, then a0b1 + a1b0 (config 12's per-accumulator order)
  // kt_next: the k-tile whose B DMA an IL tile issues among these MFMAs
  auto compute = [&](int hb, int bs, int t, int u, int kt_next = 0) {
    const int kh = t / KW, kw = t - kh * KW;
    const uint16_t* la = lds + hb * A_EL;
    const uint16_t* lb = lds + NHB * A_EL + bs * B_EL + u * B_TAP;
    if constexpr (MF) {
      // one 32-deep k-step: lane group lg holds k 8 lg .. +7 (16-B slot lg)
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        frag_t fa[NP][FM];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int ar = ((tmask[i][a] >> t) & 1) ? hrow(wm * WTM + i * 32 + 16 * a, l16) + kh * tstep + kw : HALO_HR;
#pragma unroll
          for (int p = 0; p < NP; ++p)
            fa[p][i] = *reinterpret_cast<const frag_t*>(la + (p * HRA + ar) * BK + hswz(ar, lg) * 8);
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          frag_t fb[NP][FN];
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            const int row = wn * WTN + j * 32 + 16 * b + l16;
#pragma unroll
            for (int p = 0; p < NP; ++p)
              fb[p][j] = *reinterpret_cast<const frag_t*>(lb + (p * BN + row) * BK + pswz<BK>(row, lg) * 8);
          }
          // config 12's per-accumulator order: a0b0, then a0b1 + a1b0
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) {
              if constexpr (IL) {
                if (a == 0 && b == 0) glds_b_due(kt_next, bs ^ 1, i * FN + j);
              }
              acc4[i][j][2 * a + b] = s3_mf16(fa[0][i], fb[0][j], acc4[i][j][2 * a + b]);
            }
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) {
              acc4[i][j][2 * a + b] = s3_mf16(fa[0][i], fb[1][j], acc4[i][j][2 * a + b]);
              acc4[i][j][2 * a + b] = s3_mf16(fa[1][i], fb[0][j], acc4[i][j][2 * a + b]);
            }
        }
      }
      return;
    }
    int ar[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i)
      ar[i] = ((tmask[i][0] >> t) & 1) ? hrow(wm * WTM + i * 32, lr) + kh * tstep + kw : HALO_HR;
#pragma unroll
    for (int st = 0; st < BK / 16; ++st) {
      frag_t a[NP][FM], b[NP][FN];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int i = 0; i < FM; ++i)
          a[p][i] = *reinterpret_cast<const frag_t*>(la + (p * HRA + ar[i]) * BK + hswz(ar[i], 2 * st + lh) * 8);
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int row = wn * WTN + j * 32 + lr;
          b[p][j] = *reinterpret_cast<const frag_t*>(lb + (p * BN + row) * BK + pswz<BK>(row, 2 * st + lh) * 8);
        }
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = s3_mf32(a[0][i], b[0][j], acc[i][j]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          acc[i][j] = s3_mf32(a[0][i], b[1][j], acc[i][j]);
          acc[i][j] = s3_mf32(a[1][i], b[0][j], acc[i][j]);
        }
    }
  };

  // ---- prologue: the zero rows, slice 0's halo (pass by pass), k-tile 0's B ----
  RR_PH_DECL
  if (tid < 8 * NHB) {
    // row HALO_HR of both planes of every halo buffer: 64 B per plane, 16 B per thread
    const int buf = tid >> 3, p = (tid >> 2) & 1, sl = tid & 3;
    *reinterpret_cast<u32x4*>(lds + buf * A_EL + (p * HRA + HALO_HR) * BK + sl * 8) = u32x4{0u, 0u, 0u, 0u};
  }
  glds_b(0, 0);
  {
    // slice 0's halo: every pass's loads first, one wait (three waits in
    // turn cost a tile three HBM round trips before its first MFMA); the
    // accumulators are still constant zeros here, so the registers are free
    f32x4 rp[A_PASS][2];
#pragma unroll
    for (int p = 0; p < A_PASS; ++p) load_pass_to(0, p, rp[p], m0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int p = 0; p < A_PASS; ++p) {
      s3_launder(rp[p][0]);
      s3_launder(rp[p][1]);
    }
    {
      // the record's wave max, with shuffle addresses from an opaque lane id:
      // amax_reduce's would be shared with the epilogue's amax_publish and held
      // (spilled) through the whole k-loop
      uint32_t u = a_amax_w;
      const int lo = s3_opaque(lane);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute((lo ^ o) << 2, (int)u);
        u = v > u ? v : u;
      }
      const int e = __builtin_amdgcn_readfirstlane(h2_exp(__uint_as_float(u)));
      a_sc = __int_as_float((127 + e) << 23);
      a_isc = __int_as_float((127 - e) << 23);
    }
#pragma unroll
    for (int p = 0; p < A_PASS; ++p) store_pass_from(0, p, rp[p]);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // ---- k-loop: k-tile kt = (slice c, tap t); B stage kt & 1, halo buffer c & 1.
  // The next slice's halo: pass p loaded in tap p's k-tile (after its B DMA,
  // landed by the end-of-tile wait) and split into the other buffer at the
  // start of tap p + 1's (that buffer's last reader was slice c - 1) ----
  static_assert(A_PASS < 9, "the halo passes must fit in one slice's taps");
  if constexpr (PST) {
    // ---- the persistent stream: k-step q of the block = k-step q % nk of
    // local tile q / nk, B stage q & 1, halo buffer sg & 1 (sg: the block's
    // slice counter).  The next slice -- the tile's next, or after the
    // tile's last the next tile's slice 0 -- loads in a slice's first group
    // and splits into the other buffer in its second (with that buffer's
    // zero rows: an epilogue may have staged C over them); the next k-step's
    // B DMA may belong to the next tile (the same weights).  After a tile's
    // last k-step its epilogue stages C through the halo buffer that slice
    // released, in 128-row slabs ----
    const int my_tiles = (ntiles - bid + nwg - 1) / nwg;
    const int Q = my_tiles * nk;
    // the group whose top splits the next slice into the other buffer: the
    // slice's third (its passes, loaded in the first group, then have two
    // groups' MFMAs to arrive from HBM; the first group's end waits only for
    // the B DMA issued before them), or the second with fewer groups
    const int st_g = ngrp >= 3 ? 2 : 1;
    int tl = 0, c = 0, tg = 0, kt = 0, sg = 0;
    int m_next = my_tiles > 1 ? tile_m0(1) : m0;
    for (int q = 0; q < Q; ++q) {
      const bool last_slice = c + 1 == nch;
      const bool more = !last_slice || tl + 1 < my_tiles;
      if (q + 1 < Q) glds_b(kt + 1 == nk ? 0 : kt + 1, (q + 1) & 1);
      if (more && tg == st_g) {
        const int nb = (sg + 1) & 1;
#pragma unroll
        for (int p = 0; p < A_PASS; ++p) store_pass(nb, p);
        if (tid < 8) {
          const int pl = tid >> 2, sl = tid & 3;
          *reinterpret_cast<u32x4*>(lds + nb * A_EL + (pl * HRA + HALO_HR) * BK + sl * 8) = u32x4{0u, 0u, 0u, 0u};
        }
      }
      if (more && tg == 0) {
#pragma unroll
        for (int p = 0; p < A_PASS; ++p) load_pass_to(last_slice ? 0 : c + 1, p, ra[p], last_slice ? m_next : m0);
      }
#pragma unroll
      for (int u = 0; u < TPK; ++u) compute(sg & 1, q & 1, tg * TPK + u, u);
      if (more && tg == 0 && st_g == 2)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * A_PASS) : "memory");  // the next B (older than the passes)
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next B (and the next slice's passes)
      launder_pass();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (++tg == ngrp) {
        tg = 0;
        ++c;
        ++sg;
      }
      if (++kt == nk) {
        if constexpr (MF) {
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
              for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][4 * t + e] = acc4[i][j][t][e];
        }
        epilogue_store<WM, WN, FM, FN, A_EL / 2, (bool)MF, EPI>(
            g, g.C, acc, reinterpret_cast<float*>(lds + ((sg - 1) & 1) * A_EL), m0, n0, a_isc);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
            if constexpr (MF) {
#pragma unroll
              for (int t = 0; t < 4; ++t) acc4[i][j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
          }
        kt = 0;
        c = 0;
        ++tl;
        m0 = m_next;
        m_next = tl + 1 < my_tiles ? tile_m0(tl + 1) : m0;
        masks(m0);
      }
    }
    return;
  }
  int c = 0, tg = 0;
  RR_PH(7);
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = c + 1 < nch;
    if constexpr (!IL) glds_b(min(kt + 1, nk - 1), (kt + 1) & 1);
    if constexpr (TPK == 1 && !SB) {
      if (more && tg >= 1 && tg <= A_PASS) store_pass((c + 1) & 1, tg - 1);
      if (more && tg < A_PASS) load_pass(c + 1, tg);
    } else if constexpr (SB) {
      // one halo buffer: slice c's passes (loaded during slice c - 1) split
      // into it once every wave is done with slice c - 1 (the last group's
      // barrier), then a barrier before any tap reads them
      if (c > 0 && tg == 0) {
#pragma unroll
        for (int p = 0; p < A_PASS; ++p) store_pass(0, p);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      if (more && tg == 0) {
#pragma unroll
        for (int p = 0; p < A_PASS; ++p) load_pass(c + 1, p);
      }
    } else {
      // every pass loaded in the slice's first group, split in its second
      if (more && tg == 1) {
#pragma unroll
        for (int p = 0; p < A_PASS; ++p) store_pass((c + 1) & 1, p);
      }
      if (more && tg == 0) {
#pragma unroll
        for (int p = 0; p < A_PASS; ++p) load_pass(c + 1, p);
      }
    }
    RR_PH(0);
#pragma unroll
    for (int u = 0; u < TPK; ++u) compute(SB ? 0 : (c & 1), kt & 1, tg * TPK + u, u, min(kt + 1, nk - 1));
    RR_PH(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next B (and a halo pass)
    launder_pass();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    RR_PH(2);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    RR_PH(3);
    if (++tg == ngrp) {
      tg = 0;
      ++c;
    }
  }
  __syncthreads();
  if constexpr (MF) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][4 * t + e] = acc4[i][j][t][e];
  }
  if constexpr (T2 != 0)
    epilogue_store<WM, WN, FM, FN, LDS_U16 / 2, (bool)MF, EPI, Rows2D<T2>>(
        g, g.C, acc, reinterpret_cast<float*>(lds), 0, n0, a_isc, nullptr, Rows2D<T2>{t_img, t_y0, t_x0, H, W});
  else
    epilogue_store<WM, WN, FM, FN, LDS_U16 / 2, (bool)MF, EPI>(g, g.C, acc, reinterpret_cast<float*>(lds), m0, n0,
                                                               a_isc);
  RR_PH(6);
  RR_PH_FLUSH();
}

template <int EPI, int WM, int WN, int FM, int FN, int HR, int TPK, int MF, int IL = 0, int PERS = 0, int T2 = 0>
static hipError_t launch_h2_halo_t(const GemmArgs& g, hipStream_t s, int n_cu = 256) {
  constexpr int BN = 32 * FN * WN, BM = 32 * FM * WM;
  // (T2: images x row blocks x column blocks of the map)
  const long long tiles_m = T2 ? (long long)(g.M / (g.H * g.W)) * ((g.H + BM / T2 - 1) / (BM / T2)) * ((g.W + T2 - 1) / T2)
                               : (g.M + BM - 1) / BM,
                  tiles_n = g.N / BN;
  const long long nblk = tiles_m * tiles_n;
  if (nblk <= 0) return hipSuccess;
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  // PERS: one block per CU walking the row tiles (tiles_n == 1; a block that
  // owns several stays on its XCD: grid a multiple of 8)
  const int slots = std::max(8, n_cu & ~7);
  const long long grid = PERS == 1 ? (nblk <= slots ? nblk : slots) : nblk;
  hipLaunchKernelGGL((gemm_h2_halo_kernel<EPI, WM, WN, FM, FN, HR, TPK, MF, IL, PERS, T2>), dim3((unsigned)grid), dim3(512),
                     0, s, g, (int)tiles_n);
  return hipGetLastError();
}
// The raster instances with the four residual / ReLU epilogues; the 2-D block
// tiles (T2: maps too wide for a raster halo, C2's 1024-px layers 1-3) with
// the two that have no residual (the trunk's 3x3s have none).
template <int WM, int WN, int FM, int FN, int HR, int TPK, int MF, int IL, int PERS, int T2>
static hipError_t launch_h2_halo_i(const GemmArgs& g, hipStream_t s, int n_cu) {
  if constexpr (T2 != 0) {
    if ((ep_flags(g) & EP_RES) != 0) return hipErrorInvalidValue;
    if ((ep_flags(g) & EP_RELU) != 0)
      return launch_h2_halo_t<H2_EP | EP_RELU, WM, WN, FM, FN, HR, TPK, MF, 0, PERS, T2>(g, s);
    return launch_h2_halo_t<H2_EP, WM, WN, FM, FN, HR, TPK, MF, 0, PERS, T2>(g, s);
  } else {
    return h2_ep_dispatch<false>(g, [&](auto ep) {
      return launch_h2_halo_t<decltype(ep)::value, WM, WN, FM, FN, HR, TPK, MF, IL, PERS>(g, s, n_cu);
    });
  }
}
// the route's tuple -> the instance (the table: h2_route.hpp)
hipError_t launch_h2_halo(const H2Route& r, const GemmArgs& g, hipStream_t s, int n_cu) {
#define RR_X(WM, WN, FM, FN, HR, TPK, MF, IL, PERS, T2)                                                             \
  if (r.wm == WM && r.wn == WN && r.fm == FM && r.fn == FN && r.hr == HR && r.tpk == TPK && r.mf16 == MF && r.il == IL && \
      r.pers == PERS && r.t2 == T2)                                                                                 \
    return launch_h2_halo_i<WM, WN, FM, FN, HR, TPK, MF, IL, PERS, T2>(g, s, n_cu);
  RR_H2_HALO_INSTANCES(RR_X)
#undef RR_X
  return hipErrorInvalidValue;
}

#if RR_S3_PHASES
int h2_halo_phases(unsigned long long* out) { return s3_phases_take(out); }
#endif

}  // namespace rr
