// h2_tile.hip — the one-tile-per-block kernel of the f16x2 split GEMM core
// (gemm_s3_kernel: tile configs 3, 4, 7, 9-12, table below) and the fused
// implicit-GEMM stem + max-pool instance of it.
//
// gfx950 has no xf32/TF32 MFMA, and its f32-input MFMA runs at 1/16 of the
// bf16 rate (MI355X_MICROARCH.md: 157 vs 2500 TF/s dense).  Every fp32
// operand is scaled by a power of two and split into two fp16 pieces,
// x 2^e = x0 + x1 + r with |r| <= 2^-22 |x 2^e|; a.b keeps a0b0 (its own
// accumulator) + a0b1 + a1b0 (h2_common.hpp; DESIGN.md, f16x2 split core):
// three fp16 MFMAs per fp32 product with exact products and fp32
// accumulation, error vs float64 at the exact-fp32 MFMA chain's
// (tests/test_gpu_h2.py).  (The split core this one replaced: DESIGN.md,
// "Removed from the library in round 6".)
//
// Operands: A = fp32 activations (dense rows or the implicit im2col of an
// NHWC map with Cin % 32 == 0), split in registers while staging into LDS;
// B = weights pre-split once into fp16 planes [2][N][K] (rr_split2_f16),
// copied global -> LDS by LDS-DMA (global_load_lds).  16-B slots of the LDS
// rows are XOR-swizzled so the fragment ds_read_b128 are conflict-free.
// The other kernels of the family: h2_stream.hip (config 8), h2_stream256.hip
// (15), h2_halo.hip (13 / 14), h2_stem.hip; h2_route.hpp picks among them.
#include <algorithm>

#include "h2_common.hpp"
#include "h2_route.hpp"

namespace rr {

// MF16 (BK = 32): each 32x32 tile is four v_mfma_f32_16x16x32_f16
// tiles (one 32-deep k-step per k-tile instead of two 16-deep ones; the
// 16x16 shape holds a higher clock on random operands, MI355X_MICROARCH.md
// 'DVFS give-back' item 7).  The k-tile's MFMAs go in two parts around the A
// split: a0b1 + a1b0 (mf_lo1), then a0b0 among the split's VALU (mf_rest).
// IL (the 32x32x16 two-stage loop, dense or Cin % 32 == 0 conv A): the next
// k-tiles' B DMA and A loads are not issued as one burst at the top of the
// k-tile but one instruction group at a time among the first MFMAs of its
// first k-step (see gemm_lp.hip IL: a burst of every wave's loads at once
// fills the vector-memory issue queue and stalls the MFMAs behind it).
template <int WM, int WN, int FM, int FN, int BK, int AMODE, int MINB, int MF16, int EPI, int NSTG = 2, int POOL = 0,
          int ACC1 = 0, int IL = 0>
__global__ __launch_bounds__(64 * WM * WN, MINB) void gemm_s3_kernel(GemmArgs g, int tiles_n) {
  static_assert(!POOL || (AMODE == A_CONV_C4 && WM * 32 * FM == 256), "stem + max-pool: 256-row NHWC4 tile");
  static_assert(NSTG == 2 || (NSTG == 3 && MF16), "three LDS stages: the 16x16x32 tile");
  static_assert(!IL || (!MF16 && NSTG == 2 && !POOL), "IL: the 32x32x16 two-stage loop");
  static_assert(!MF16 || BK == 32, "MF16: BK 32");
  static_assert(EPI >= 0 && (EPI & EP_SCALE), "f16x2: scaled epilogue");
  typedef f16x8 frag_t;
  constexpr int NP = 2;                      // planes per operand
  constexpr int NT = 64 * WM * WN, NW = WM * WN;
  constexpr int WTM = 32 * FM, WTN = 32 * FN;
  constexpr int BM = WTM * WM, BN = WTN * WN;
  constexpr int SL = BK / 8;                 // 16-B slots per plane row
  constexpr int A_EL = NP * BM * BK;         // 16-bit elements per stage: A planes
  constexpr int BUF = A_EL + NP * BN * BK;   // 16-bit elements per stage: A + B planes
  constexpr int A_RPP = NT / SL;             // A rows staged per pass
  constexpr int A_CH = BM / A_RPP;           // A chunks (8 k each) per thread
  constexpr int B_RPI = 64 / SL;             // plane rows per LDS-DMA wave instruction
  constexpr int B_TI = NP * BN / B_RPI;      // LDS-DMA wave instructions per k-tile
  constexpr int B_INS = (B_TI + NW - 1) / NW; // ... per wave (the last round may be partial)
  static_assert(BM % A_RPP == 0 && (NP * BN) % B_RPI == 0, "staging must tile the block");
  static_assert(BK == 16 || BK == 32, "BK");
  // one block per CU: room for the whole fp32 C tile, so the epilogue
  // stages it in one slab
  // (rows padded by 4 / 8 floats, epilogue_store)
  constexpr int CT_F = BM * (BN + (MF16 ? 4 : 8));
  // (the fused stem + max-pool stages its whole C tile at any MINB)
  constexpr int LDS_U16 = ((MINB == 1 || POOL) && 2 * CT_F > NSTG * BUF && 2 * CT_F <= 80 * 1024) ? 2 * CT_F : NSTG * BUF;
  __shared__ __attribute__((aligned(16))) uint16_t lds[LDS_U16];

  // the A operand's split scale: its max-|x| record is loaded first, so it
  // has landed by the prologue's first counted wait
  const uint32_t a_amax_w = amax_load_slot(g.a_amax);

  // round stagger (GemmArgs): half of the first round's blocks start later,
  // so in every later round half the CUs run their k-loop while the other
  // half run their HBM-heavy epilogue (blocks b, b+8, ... share an XCD, so
  // (b >> 3) & 1 halves every XCD).  At two blocks per CU the later half is
  // the second resident of every CU (blocks n_cu .. 2 n_cu - 1: the
  // dispatcher fills every CU's first slot first), so each CU's two blocks
  // alternate between k-loop and epilogue.
  if (g.stagger_sleeps > 0 && (int)blockIdx.x < g.stagger_blocks &&
      (MINB >= 2 ? (int)blockIdx.x >= g.stagger_blocks / 2 : ((blockIdx.x >> 3) & 1)))
    for (int i = 0; i < g.stagger_sleeps; ++i) __builtin_amdgcn_s_sleep(32);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float a_sc = 1.f, a_isc = 1.f;
  const int wm = wave % WM, wn = wave / WM;
  const int lr = lane & 31, lh = lane >> 5;

  // XCD-aware bijective block remap (blocks b, b+8, ... share an XCD)
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int tn = wgid % tiles_n, tm = wgid / tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int nk = g.K / BK;  // K % BK == 0 (checked on the host)

  // ---- A: per-chunk row state (fp32, register-staged, split on store) ----
  const int a_slot = tid % SL, a_row = tid / SL;
  const float* a_ptr[A_CH];
  int a_ih0[A_CH], a_iw0[A_CH];
  bool a_ok[A_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    const int m = m0 + a_row + i * A_RPP;
    a_ok[i] = m < g.M;
    const int mm = a_ok[i] ? m : 0;
    if constexpr (POOL) {
      // tile tm = (image, pr, pc); local row lr -> conv output pixel
      // (16 pr - 1 + lr / 15, 14 pc - 1 + lr % 15), lr < 255; rows outside the
      // conv map load the zero page and are left out of every window
      const int tpi = g.pool_tr * g.pool_tc;
      const int b = tm / tpi, t2 = tm - b * tpi, pr = t2 / g.pool_tc, pc = t2 - pr * g.pool_tc;
      const int tr = a_row + i * A_RPP, q = tr / 15;
      const int oh = 16 * pr - 1 + q, ow = 14 * pc - 1 + (tr - 15 * q);
      a_ok[i] = tr < 255 && (unsigned)oh < (unsigned)g.OH && (unsigned)ow < (unsigned)g.OW;
      a_ih0[i] = oh * g.stride - g.pad;
      a_iw0[i] = ow * g.stride - g.pad;
      a_ptr[i] = g.A + (((long long)b * g.H + a_ih0[i]) * g.W + a_iw0[i]) * g.Cin;
    } else if constexpr (AMODE == A_DENSE) {
      a_ptr[i] = g.A + (long long)mm * g.lda + a_slot * 8;
      a_ih0[i] = a_iw0[i] = 0;
    } else {
      const int ohw = g.OH * g.OW;
      const int b = mm / ohw, rem = mm - b * ohw;
      const int oh = rem / g.OW, ow = rem - oh * g.OW;
      a_ih0[i] = oh * g.stride - g.pad;
      a_iw0[i] = ow * g.stride - g.pad;
      // the (possibly padded, out-of-image) top-left tap pixel; a k-tile adds a
      // block-uniform offset (kh*W + kw)*Cin + cin0
      a_ptr[i] = g.A + (((long long)b * g.H + a_ih0[i]) * g.W + a_iw0[i]) * g.Cin + (AMODE == A_CONV ? a_slot * 8 : 0);
    }
  }
  // conv tap of the k-tile the A loader is at, advanced incrementally (the
  // loader requests k-tiles in non-decreasing order, one step at a time):
  // no per-tile integer divisions
  int tp_kt = 0, tp_kh = 0, tp_kw = 0, tp_cin = 0;
  long long tp_off = 0;  // (kh * W + kw) * Cin + cin0
  auto tap_to = [&](int kt) {
    while (tp_kt < kt) {
      ++tp_kt;
      tp_off += BK;
      tp_cin += BK;
      if (tp_cin == g.Cin) {
        tp_cin = 0;
        if (++tp_kw == g.KW) {
          tp_kw = 0;
          ++tp_kh;
          tp_off += (long long)(g.W - g.KW) * g.Cin;
        }
      }
    }
  };
  f32x4 ra2[2][A_CH][2];
  auto load_a = [&](int kt, int rb) {
    f32x4(&ra)[A_CH][2] = ra2[rb];
    const int k0 = kt * BK;
    if constexpr (AMODE == A_DENSE) {
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        // every load is issued (the counted vmcnt of the k-loop assumes A_LD
        // loads per tile); out-of-range rows read the zero page, so the
        // loaded registers are used as they are, no select after the load
        // (a select right after it makes hipcc wait for the load at once)
        const f32x4* p = a_ok[i] ? reinterpret_cast<const f32x4*>(a_ptr[i] + k0) : s3_zero_page();
        s3_load2<1>(p, ra[i]);
      }
    } else if constexpr (AMODE == A_CONV_C4) {
      // NHWC4 stem (RGB + a zero channel): a k-tile is BK/4 filter taps of 4
      // channels, a thread's 8-k chunk the taps (BK/4) kt + 2 slot + {0, 1},
      // one 16-B load each; taps past KH*KW (K padded to a multiple of 32) and
      // padding pixels read the zero page
      const int tb = kt * (BK / 4), khb = tb / g.KW, kwb = tb - khb * g.KW;
      const f32x4* p[A_CH][2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        int kh = khb, kw = kwb + 2 * a_slot + e;
        while (kw >= g.KW) kw -= g.KW, ++kh;
        const bool tap_ok = kh < g.KH;
        const long long toff = (long long)(kh * g.W + kw) * 4;
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
          const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
          const bool ok = tap_ok && a_ok[i] && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
          p[i][e] = ok ? reinterpret_cast<const f32x4*>(a_ptr[i] + toff) : s3_zero_page();
        }
      }
#pragma unroll
      for (int i = 0; i < A_CH; ++i) s3_load1x2<1>(p[i][0], p[i][1], ra[i]);
    } else {
      // Cin % 32 == 0: the whole k-tile lies in one (kh, kw) filter tap
      tap_to(kt);
      const int kh = tp_kh, kw = tp_kw;
      const long long toff = tp_off;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
        const bool ok = a_ok[i] && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
        const f32x4* p = ok ? reinterpret_cast<const f32x4*>(a_ptr[i] + toff) : s3_zero_page();
        s3_load2<1>(p, ra[i]);
      }
    }
  };
  // IL: chunk i of load_a(kt, rb) alone (dense or Cin % 32 == 0 conv A)
  auto load_a_chunk = [&](int kt, int rb, int i) {
    static_assert(!IL || AMODE == A_DENSE || AMODE == A_CONV, "IL: dense or Cin % 32 == 0 conv A");
    f32x4(&ra)[A_CH][2] = ra2[rb];
    if constexpr (AMODE == A_DENSE) {
      const f32x4* p = a_ok[i] ? reinterpret_cast<const f32x4*>(a_ptr[i] + kt * BK) : s3_zero_page();
      s3_load2<1>(p, ra[i]);
    } else if constexpr (AMODE == A_CONV) {
      tap_to(kt);
      const int ih = a_ih0[i] + tp_kh, iw = a_iw0[i] + tp_kw;
      const bool ok = a_ok[i] && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
      const f32x4* p = ok ? reinterpret_cast<const f32x4*>(a_ptr[i] + tp_off) : s3_zero_page();
      s3_load2<1>(p, ra[i]);
    }
  };
  // split the staged fp32 chunks into the two packed fp16 planes
  u32x4 pk[A_CH][NP];
  auto split_a = [&](int rb) {
    const f32x4(&ra)[A_CH][2] = ra2[rb];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) split2h8(ra[i], a_sc, pk[i][0], pk[i][1]);
  };
  auto write_a = [&](int buf) {
    uint16_t* la = lds + buf * BUF;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int row = a_row + i * A_RPP;
      const int off = row * BK + pswz<BK>(row, a_slot) * 8;
#pragma unroll
      for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x4*>(la + p * BM * BK + off) = pk[i][p];
    }
  };
  auto store_a = [&](int rb, int buf) {
    split_a(rb);
    write_a(buf);
  };

  // ---- B: two fp16 planes, LDS-DMA (64 lanes x 16 B = B_RPI whole plane
  // rows per instruction; the swizzle moves to the source slot) ----
  const uint16_t* b_src[B_INS];
  const uint16_t* Bp = reinterpret_cast<const uint16_t*>(g.B);
#pragma unroll
  for (int i = 0; i < B_INS; ++i) {
    const int prow = min(i * NW + wave, B_TI - 1) * B_RPI + lane / SL;
    const int p = prow / BN, r = prow - p * BN;
    const int n = min(n0 + r, g.N - 1);  // rows past N feed only unstored columns
    b_src[i] = Bp + p * g.b_plane + (long long)n * g.ldb + pswz<BK>(r, lane % SL) * 8;
  }
  auto glds_b = [&](int kt, int buf) {
    uint16_t* lb = lds + buf * BUF + A_EL;
    // every wave issues B_INS (the counted vmcnt assumes it): in a partial
    // last round the surplus waves repeat the last row group (same source,
    // same LDS destination)
#pragma unroll
    for (int i = 0; i < B_INS; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(b_src[i] + (long long)kt * BK),
                                       (__attribute__((address_space(3))) void*)(lb + min(i * NW + wave, B_TI - 1) * B_RPI * BK),
                                       16, 0, 0);
  };

  auto glds_b_one = [&](int kt, int buf, int i) {
    uint16_t* lb = lds + buf * BUF + A_EL;
    __builtin_amdgcn_global_load_lds((const void*)(b_src[i] + (long long)kt * BK),
                                     (__attribute__((address_space(3))) void*)(lb + min(i * NW + wave, B_TI - 1) * B_RPI * BK),
                                     16, 0, 0);
  };
  // IL: the iteration's load groups in issue order (B DMA of kt + 1, then the
  // A chunks of kt + 2: the counted waits assume that order), group q before
  // MFMA number 2q of the first k-step, each fenced in place
  constexpr int IL_GROUPS = B_INS + A_CH;
  // every group's MFMA number exists: 0 .. FM FN - 1 (a0b0), then FM FN + 2m
  static_assert(!IL || ((FM * FN) % 2 == 0 && 2 * (IL_GROUPS - 1) < 3 * FM * FN), "IL: a slot for every load group");
  auto il_issue = [&](int kt, int cur, int idx) {
    if constexpr (IL) {
#pragma unroll
      for (int q = 0; q < IL_GROUPS; ++q) {
        if (2 * q != idx) continue;
        __builtin_amdgcn_sched_barrier(0);
        if (q < B_INS) glds_b_one(min(kt + 1, nk - 1), cur ^ 1, q);
        else load_a_chunk(min(kt + 2, nk - 1), cur, q - B_INS);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  f32x16 hi[FM][FN];
  f32x16 lo[ACC1 ? 1 : FM][ACC1 ? 1 : FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        hi[i][j][r] = 0.f;
        if constexpr (!ACC1) lo[i][j][r] = 0.f;
      }

  // IL, first k-step: iteration kt_il's loads go out among the MFMAs
  auto compute_st = [&](int cur, int st, int kt_il = 0) {
    const uint16_t* la = lds + cur * BUF;
    const uint16_t* lb = la + A_EL;
    {
      frag_t a[NP][FM], b[NP][FN];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int row = wm * WTM + i * 32 + lr;
          a[p][i] = *reinterpret_cast<const frag_t*>(la + (p * BM + row) * BK + pswz<BK>(row, 2 * st + lh) * 8);
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int row = wn * WTN + j * 32 + lr;
          b[p][j] = *reinterpret_cast<const frag_t*>(lb + (p * BN + row) * BK + pswz<BK>(row, 2 * st + lh) * 8);
        }
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          if constexpr (IL) {
            if (st == 0) il_issue(kt_il, cur, i * FN + j);
          }
          hi[i][j] = s3_mf32(a[0][i], b[0][j], hi[i][j]);
        }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          if constexpr (IL) {
            if (st == 0) il_issue(kt_il, cur, FM * FN + 2 * (i * FN + j));
          }
          f32x16& L = ACC1 ? hi[i][j] : lo[ACC1 ? 0 : i][ACC1 ? 0 : j];
          L = s3_mf32(a[0][i], b[1][j], L);
          L = s3_mf32(a[1][i], b[0][j], L);
        }
    }
  };
  // ---- MF16: 16x16x32 tiles, sub-tile t = 2a + b (row half a, column half b) ----
  f32x4 hi4[MF16 ? FM : 1][MF16 ? FN : 1][4], lo4[MF16 && !ACC1 ? FM : 1][MF16 && !ACC1 ? FN : 1][4];
  frag_t fa[MF16 ? NP : 1][MF16 ? FM : 1][2], fb[MF16 ? NP : 1][MF16 ? FN : 1][2];
  if constexpr (MF16) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          hi4[i][j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
          if constexpr (!ACC1) lo4[i][j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
  }
  // ACC1: the plane-1 products go to the a0b0 accumulator (one accumulator set)
#define RR_LO(i, j, t) (*(ACC1 ? &hi4[i][j][t] : &lo4[ACC1 ? 0 : i][ACC1 ? 0 : j][t]))
  const int l16 = lane & 15, lg = lane >> 4;
  // plane p fragments of one 32-deep k-tile: lane group lg holds k = 8lg..8lg+7
  // (16-B slot lg) of row l16 of each 16-row half
  auto rd_mf = [&](int cur, int p) {
    // three stages: the stage offset (up to 96 KB) does not fit the 16-bit
    // ds_read offset, so each stage would need its own address registers;
    // an opaque per-call base keeps one set
    const uint16_t* la = lds + (NSTG == 3 ? s3_opaque(cur * BUF) : cur * BUF);
    const uint16_t* lb = la + A_EL;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = wm * WTM + i * 32 + h * 16 + l16;
        fa[MF16 ? p : 0][i][h] = *reinterpret_cast<const frag_t*>(la + (p * BM + row) * BK + pswz<BK>(row, lg) * 8);
      }
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = wn * WTN + j * 32 + h * 16 + l16;
        fb[MF16 ? p : 0][j][h] = *reinterpret_cast<const frag_t*>(lb + (p * BN + row) * BK + pswz<BK>(row, lg) * 8);
      }
  };
#define RR_MF16(a, b, c) c = s3_mf16(a, b, c)
  // k-tile of MFMAs in two parts.  lo1: the plane-1 products (a0b1, a1b0)
  // into lo; rest: a0b0 into hi — the same per-accumulator order as one pass —
  // with the A split + LDS store of the next stage interleaved (the plane-1
  // fragments are dead by then, which leaves the registers for it).
  auto mf_lo1 = [&](int cur) {
    if constexpr (MF16) {
      rd_mf(cur, 0);
      rd_mf(cur, 1);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            RR_MF16(fa[0][i][t >> 1], fb[1][j][t & 1], RR_LO(i, j, t));
            RR_MF16(fa[1][i][t >> 1], fb[0][j][t & 1], RR_LO(i, j, t));
          }
    }
  };
  // rbn: the register buffer holding the next A k-tile; stn: the stage it goes to
  auto mf_rest = [&](int cur, int rbn, int stn) {
    if constexpr (MF16) {
      split_a(rbn);
      write_a(stn);  // that stage is free since the last barrier
      // with two A chunks per thread, or the conv A loader's state, there is
      // no room to hold the plane-0 fragments across the split (2 registers
      // spilled): re-read them (ACC1 leaves the registers to hold them)
      if constexpr (!ACC1 && (A_CH >= 2 || AMODE != A_DENSE)) rd_mf(cur, 0);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int t = 0; t < 4; ++t) RR_MF16(fa[0][i][t >> 1], fb[0][j][t & 1], hi4[i][j][t]);
      // the split's VALU (about 3 per element) two per MFMA gap
#pragma unroll
      for (int x = 0; x < FM * FN * 4; ++x) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // 2 VALU
      }
    }
  };
#undef RR_MF16

  constexpr int A_LD = 2 * A_CH;  // A global loads per tile per thread
  {
    // Pipelined k-loop with asynchronous A loads (s3_load2<1>), two register
    // buffers: A(j) lives in buffer j&1.  Iteration kt issues the B DMA of
    // tile kt+1 and the A loads of tile kt+2 (into the buffer A(kt) left),
    // computes tile kt, then waits for everything but the A loads of kt+2
    // (so A(kt+1) and B(kt+1) have landed), splits A(kt+1) into the other
    // stage and crosses a raw barrier.  An A load thus has almost two
    // iterations to land instead of one; its split runs between the MFMAs of
    // the second 16-deep step.  The loop is unrolled by two so the stage and
    // buffer indices are constants.
    auto launder_a = [&](int rb) {
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        s3_launder(ra2[rb][i][0]);
        s3_launder(ra2[rb][i][1]);
      }
    };
    if constexpr (NSTG == 3) {
      // Three LDS stages (config 9): the B DMA of k-tile kt+2 and the A
      // loads of kt+2 go out at the start of iteration kt, so B has two
      // iterations to land instead of one; A(kt+1) is split into stage
      // (kt+1) % 3 among the MFMAs as before.  Its counted wait also covers
      // B(kt+1) (issued before it), so the iteration ends on the barrier
      // alone.  Unrolled by six: stage (kt % 3) and register buffer (kt % 2)
      // indices are constants.
      load_a(0, 0);
      glds_b(0, 0);
      glds_b(nk > 1 ? 1 : 0, 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * B_INS) : "memory");  // A(0) landed
      launder_a(0);
      {
        const int e = __builtin_amdgcn_readfirstlane(h2_exp(amax_reduce(a_amax_w)));
        a_sc = __int_as_float((127 + e) << 23);
        a_isc = __int_as_float((127 - e) << 23);
      }
      store_a(0, 0);
      load_a(nk > 1 ? 1 : 0, 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD + B_INS) : "memory");  // B(0) landed
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      auto iter3 = [&](int kt, int cur, int rb) __attribute__((always_inline)) {
        glds_b(min(kt + 2, nk - 1), (cur + 2) % 3);
        load_a(min(kt + 2, nk - 1), rb);
        mf_lo1(cur);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD + B_INS) : "memory");  // A(kt+1), B(kt+1) landed
        launder_a(rb ^ 1);
        mf_rest(cur, rb ^ 1, (cur + 1) % 3);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      };
      for (int kt = 0; kt < nk; kt += 6) {
        iter3(kt, 0, 0);
        if (kt + 1 < nk) iter3(kt + 1, 1, 1);
        if (kt + 2 < nk) iter3(kt + 2, 2, 0);
        if (kt + 3 < nk) iter3(kt + 3, 0, 1);
        if (kt + 4 < nk) iter3(kt + 4, 1, 0);
        if (kt + 5 < nk) iter3(kt + 5, 2, 1);
      }
    } else {
      RR_PH_DECL
      load_a(0, 0);
      glds_b(0, 0);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(B_INS) : "memory");  // A(0) landed
      launder_a(0);
      {
        // uniform: the exponent and both powers of two stay in scalar registers
        const int e = __builtin_amdgcn_readfirstlane(h2_exp(amax_reduce(a_amax_w)));
        a_sc = __int_as_float((127 + e) << 23);
        a_isc = __int_as_float((127 - e) << 23);
      }
      store_a(0, 0);
      load_a(nk > 1 ? 1 : 0, 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD) : "memory");  // B(0) landed
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      auto iter = [&](int kt, int cur) __attribute__((always_inline)) {
        if constexpr (!IL) {
          glds_b(min(kt + 1, nk - 1), cur ^ 1);
          load_a(min(kt + 2, nk - 1), cur);
        }
        if constexpr (MF16) {
          RR_PH(0);
          mf_lo1(cur);
          RR_PH(1);
          // A(kt+1) landed (the B DMA of kt+1 and the A loads of kt+2 may not
          // have): split and stored among the remaining MFMAs of tile kt
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD + B_INS) : "memory");
          launder_a(cur ^ 1);
          RR_PH(2);
          mf_rest(cur, cur ^ 1, cur ^ 1);
          RR_PH(3);
        } else {
          compute_st(cur, 0, kt);
          // A(kt+1) landed: its split overlaps the remaining MFMAs of tile kt
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD + B_INS) : "memory");
          launder_a(cur ^ 1);
          split_a(cur ^ 1);
        }
        if constexpr (!MF16) {
  #pragma unroll
          for (int st = 1; st < BK / 16; ++st) compute_st(cur, st);
          write_a(cur ^ 1);
        }
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD) : "memory");  // B DMA of kt+1 landed
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        RR_PH(4);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        RR_PH(5);
      };
      RR_PH(7);
      for (int kt = 0; kt < nk; kt += 2) {
        iter(kt, 0);
        if (kt + 1 < nk) iter(kt + 1, 1);
      }
      if constexpr (MF16) RR_PH_FLUSH();
    }
    // the clamped tail loads are still in flight: keep both buffers live
    // until they have landed, so no later value is allocated to them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    launder_a(0);
    launder_a(1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  if constexpr (MF16) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) hi[i][j][4 * t + e] = ACC1 ? hi4[i][j][t][e] : hi4[i][j][t][e] + RR_LO(i, j, t)[e];
  } else {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        if constexpr (!ACC1) hi[i][j] += lo[i][j];
  }
  if constexpr (POOL) {
    // stage the raw 256 x 64 accumulator tile, then every pooled output of
    // the tile: the max over the window's in-map conv outputs of the raw
    // accumulators, then scale, bias, ReLU once (all monotone: the same bits
    // as pooling the stored conv outputs)
    constexpr int CS = BN + (MF16 ? 4 : 8);
    static_assert(BM * CS <= LDS_U16 / 2, "stem + max-pool: the C tile must fit the LDS");
    float* ct = reinterpret_cast<float*>(lds);
    {
      const int wm = wave % WM, wn = wave / WM;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            ct[(wm * WTM + acc_row<(bool)MF16>(i, r, lane)) * CS + wn * WTN + acc_col<(bool)MF16>(j, r, lane)] =
                hi[i][j][r];
    }
    __syncthreads();
    const int tpi = g.pool_tr * g.pool_tc;
    const int b = tm / tpi, t2 = tm - b * tpi, pr = t2 / g.pool_tc, pc = t2 - pr * g.pool_tc;
    constexpr int C4 = BN / 4;
    float am = 0.f;
    for (int it = tid; it < 56 * C4; it += NT) {
      const int qd = it / C4, c4 = it - qd * C4, pi = qd / 7, pj = qd - 7 * pi;
      const int ph = 8 * pr + pi, pw = 7 * pc + pj;
      if (ph >= g.POH || pw >= g.POW) continue;
      f32x4 mx = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
      for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
        for (int dc = -1; dc <= 1; ++dc) {
          const int oh = 2 * ph + dr, ow = 2 * pw + dc;
          if ((unsigned)oh >= (unsigned)g.OH || (unsigned)ow >= (unsigned)g.OW) continue;
          const f32x4 v = *reinterpret_cast<const f32x4*>(ct + ((2 * pi + dr + 1) * 15 + 2 * pj + dc + 1) * CS + c4 * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) mx[e] = __builtin_fmaxf(mx[e], v[e]);
        }
      const f32x4 sc = *reinterpret_cast<const f32x4*>(g.col_scale + c4 * 4) * a_isc;
      const f32x4 bv = g.bias != nullptr ? *reinterpret_cast<const f32x4*>(g.bias + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = __builtin_fmaxf(mx[e] * sc[e] + bv[e], 0.f);
        am = amax_acc(am, o[e]);
      }
      *reinterpret_cast<f32x4*>(g.pool_out + (((long long)b * g.POH + ph) * g.POW + pw) * BN + c4 * 4) = o;
    }
    if (g.c_amax != nullptr) amax_publish(g.c_amax, am, blockIdx.x * NW + wave);
  } else {
    epilogue_store<WM, WN, FM, FN, LDS_U16 / 2, (bool)MF16, EPI>(g, g.C, hi, reinterpret_cast<float*>(lds), m0, n0,
                                                                   a_isc);
  }
}

template <int WM, int WN, int FM, int FN, int BK, int AM, int MINB, int MF16, int EPI, int NSTG = 2, int POOL = 0,
          int ACC1 = 0, int IL = 0>
static hipError_t launch_s3_t(GemmArgs g, hipStream_t s, int n_cu, int stagger) {
  constexpr int BM = 32 * FM * WM, BN = 32 * FN * WN;
  const long long tiles_m = (g.M + BM - 1) / BM, tiles_n = (g.N + BN - 1) / BN;
  const long long nblk = tiles_m * tiles_n;
  if (nblk <= 0) return hipSuccess;
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  // resident blocks per CU: MINB is the launch bound's minimum waves per SIMD
  constexpr int PER_CU = (MINB * 4) / (WM * WN) > 1 ? (MINB * 4) / (WM * WN) : 1;
  g.stagger_blocks = n_cu * PER_CU;
  g.stagger_sleeps = nblk > 2LL * n_cu * PER_CU ? stagger : 0;  // only grids of several rounds
  hipLaunchKernelGGL((gemm_s3_kernel<WM, WN, FM, FN, BK, AM, MINB, MF16, EPI, NSTG, POOL, ACC1, IL>), dim3((unsigned)nblk),
                     dim3(64 * WM * WN), 0, s, g, (int)tiles_n);
  return hipGetLastError();
}

// Tile configs (waves WMxWN, MFMA tiles per wave FMxFN, BK, blocks per CU,
// LDS of the two stages).  Which one serves a GEMM, and the measurements
// behind that: h2_route.hpp.
//   3: 256x128, 8 waves of 64x64, BK 32, 1/CU (96 KB)
//   4: 128x256, 8 waves of 64x64, BK 32, 1/CU (96 KB), v_mfma_f32_16x16x32_f16
//   7: 256x64,  8 waves of 32x64, BK 16, 2/CU (40 KB), 4 waves per SIMD
//   9: config 4 with three LDS stages (144 KB): the B DMA two k-tiles ahead
//  10: config 4 with one accumulator set (ACC1: the plane-1 products
//      accumulate with a0b0; error vs float64 still at the exact-fp32
//      core's, profiles/r03j_acc1_ab.txt; 196 instead of 254 VGPRs)
//  11: 128x128, 4 waves of 64x64, BK 32, 2/CU (64 KB), 16x16x32, ACC1
//  12: 256x256, 8 waves of 128x64, BK 32, 1/CU (128 KB), 32x32x16, ACC1
//      (254 VGPRs -- two accumulator sets do not fit this tile): half the
//      operand bytes per FLOP of config 4
// (8 and 15: configs 4 and 12 as persistent k-streams, h2_stream.hip and
// h2_stream256.hip, bit-identical to them; 13 / 14: the halo tiles,
// h2_halo.hip).  The 16x16 shape holds a higher clock on random operands
// (MI355X_MICROARCH.md 'DVFS give-back' item 7); it spills in config 3's tile.

// The tile configs with the ResNet's epilogues compiled in: the four residual
// / ReLU combinations of H2_EP (conv + BN + ReLU, + residual + ReLU,
// projection conv + BN, ...).
template <int WM, int WN, int FM, int FN, int BK, int AM, int MINB, int MF16, int NSTG = 2, int ACC1 = 0, int IL = 0>
static hipError_t launch_s3_ep(const GemmArgs& g, hipStream_t s, int n_cu, int st) {
  return h2_ep_dispatch<false>(g, [&](auto ep) {
    return launch_s3_t<WM, WN, FM, FN, BK, AM, MINB, MF16, decltype(ep)::value, NSTG, 0, ACC1, IL>(g, s, n_cu, st);
  });
}

// the route's tuple -> the instance (the table: h2_route.hpp)
template <int AM>
static hipError_t launch_h2_tile_am(const H2Route& r, const GemmArgs& g, hipStream_t s, int n_cu, int st) {
#define RR_X(CFG, WM, WN, FM, FN, BK, MINB, MF16, NSTG, ACC1, IL)                                                       \
  if constexpr (!(IL && AM == A_CONV_C4)) {                                                                             \
    if (r.cfg == CFG && r.wm == WM && r.wn == WN && r.fm == FM && r.fn == FN && r.bk == BK && r.mf16 == MF16 &&        \
        r.nstg == NSTG && r.acc == (ACC1 ? 1 : 2) && r.il == IL)                                                        \
      return launch_s3_ep<WM, WN, FM, FN, BK, AM, MINB, MF16, NSTG, ACC1, IL>(g, s, n_cu, st);                          \
  }
  RR_H2_TILE_INSTANCES(RR_X)
#undef RR_X
  return hipErrorInvalidValue;
}

hipError_t launch_h2_tile(const H2Route& r, int amode, const GemmArgs& g, hipStream_t s, int n_cu, int st) {
  return amode == A_DENSE  ? launch_h2_tile_am<A_DENSE>(r, g, s, n_cu, st)
         : amode == A_CONV ? launch_h2_tile_am<A_CONV>(r, g, s, n_cu, st)
                           : launch_h2_tile_am<A_CONV_C4>(r, g, s, n_cu, st);
}

// the implicit-GEMM stem + max-pool (config 7 on NHWC4 with POOL; q.M = 256 rows per tile)
hipError_t launch_h2_tile_stem_pool(const GemmArgs& q, hipStream_t s, int n_cu) {
  return launch_s3_t<8, 1, 1, 2, 16, A_CONV_C4, 4, 0, H2_EP | EP_RELU, 2, 1>(q, s, n_cu, 0);
}

#if RR_S3_PHASES
int h2_tile_phases(unsigned long long* out) { return s3_phases_take(out); }
#endif

}  // namespace rr
