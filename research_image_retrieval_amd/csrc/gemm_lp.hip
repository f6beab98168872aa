// gemm_lp.hip — the bf16 / fp8 one-tile-per-block GEMM core for gfx950 (CDNA4).
//
// C[M,N] = A[M,K] . B[N,K]^T, A and B dense and K-contiguous, fp32 accumulate:
// the low-precision cosine rankers' seed (E_SCORES_T) and filter (E_FILTER)
// sweeps, and the ViT linears' stored C (E_STORE, bf16 only) where the
// persistent streams of gemm_lpp.hip do not apply.  launch_gemm
// (gemm_f32.hip) launches the instance gemm_route names through launch_gemm_lp
// below.
//
// Tiling as the fp32 core's: a workgroup is WM x WN waves, a wave owns FM x FN
// MFMA tiles of 32x32, each k-tile of A and B is a double-buffered LDS image
// of 128-byte rows (64 bf16 / 128 fp8) whose 16-byte slots are XOR-swizzled
// (gemm_tile.hpp swz), and block ids are remapped so consecutive tiles of one
// XCD share the A panel.  The k-tile reaches LDS register-staged (GL = 0) or
// by LDS-DMA (GL = 1, whole k-tiles only).
#include "gemm_route.hpp"
#include "gemm_tile.hpp"

namespace rr {

// MF16 (bf16 only): each 32x32 tile of a wave's block is computed as four
// v_mfma_f32_16x16x32_bf16 tiles (same cycles per FLOP as 32x32x16; the
// 16x16 shape holds a higher clock on random operands, MI355X_MICROARCH.md
// 'DVFS give-back' item 7).  Register r of tile (i, j) then maps through
// acc_row / acc_col<true> (gemm_epilogue.hpp) instead of the 32x32 map.
// IL (LDS-DMA bf16 filter sweeps): the next k-tile's DMA is not issued as one
// burst at the top of the k-tile but chunk by chunk among the first SPAN
// MFMAs (18 of 40 on 32x32x16, 36 of 80 on 16x16x32): a burst of 9
// instructions from all 8 waves at once fills the vector-memory issue queue
// and stalls the waves' MFMAs behind it (tools/fetch_ceiling.hip, r04e:
// 0.481 -> 0.525 of peak on the bare 32x32x16 sweep loop).
template <int WM, int WN, int FM, int FN, int EMODE, int DT, int MINB, int GL, int MF16 = 0, int EPI = -1, int IL = 0>
__global__ __launch_bounds__(64 * WM * WN, MINB) void gemm_lp_kernel(GemmArgs g, int tiles_n) {
  using ET = typename ElemT<DT>::T;
  static_assert(DT == DT_BF16 || DT == DT_FP8, "the low-precision core");
  static_assert(!MF16 || DT == DT_BF16, "MF16: bf16 only");
  constexpr int BK = 32;  // floats per 128-B LDS row
  constexpr int ES = (int)sizeof(ET);
  constexpr int EPR = BK * 4 / ES;  // elements per LDS row (= k per k-tile)
  constexpr int CH = 16 / ES;       // elements per 16-byte staging chunk
  constexpr int NT = 64 * WM * WN;
  constexpr int WTM = 32 * FM, WTN = 32 * FN;  // one wave's output block
  constexpr int BM = WTM * WM, BN = WTN * WN;
  constexpr int SLOTS = BK / 4;
  constexpr int ROWS_PER_PASS = NT / SLOTS;
  constexpr int A_CH = BM / ROWS_PER_PASS;
  constexpr int B_CH = BN / ROWS_PER_PASS;
  static_assert(A_CH >= 1 && B_CH >= 1, "tile too small for block");
  static_assert(BM % ROWS_PER_PASS == 0 && BN % ROWS_PER_PASS == 0, "staging passes must tile the block");
  constexpr int BUF = (BM + BN) * BK;  // floats per LDS buffer
  // EP_LNFOLD: the tile's rows' LayerNorm (mean, rstd) beside the stages
  constexpr bool LNF = EPI >= 0 && (EPI & EP_LNFOLD) != 0;
  __shared__ __attribute__((aligned(16))) float lds[2 * BUF + (LNF ? LN_ROW * BM + LN_TMAX * BN : 0)];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;

  // XCD-aware block -> tile order (rr_internal.hpp tile_coords)
  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int slot = tid % SLOTS;
  const int crow = tid / SLOTS;
  int K = g.K;
  long long koff = 0;
  float* const Cb = g.C + (g.k_split > 0 ? (long long)blockIdx.y * g.c_split_stride : 0LL);
  if (g.k_split > 0) {
    koff = (long long)blockIdx.y * g.k_split;
    K = (int)(g.K - koff < g.k_split ? g.K - koff : g.k_split);
  }
  if (g.sym && m0 > n0 + BN - 1) return;  // block-uniform, before any barrier
  const int nk = (K + EPR - 1) / EPR;

  // ---- per-chunk row state ----
  const ET* a_ptr[A_CH];
  bool a_ok[A_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    const int m = m0 + crow + i * ROWS_PER_PASS;
    a_ok[i] = m < g.M;
    a_ptr[i] = reinterpret_cast<const ET*>(g.A) + (long long)(a_ok[i] ? m : 0) * g.lda + koff;
  }
  const ET* b_ptr[B_CH];
  bool b_ok[B_CH];
#pragma unroll
  for (int i = 0; i < B_CH; ++i) {
    const int n = n0 + crow + i * ROWS_PER_PASS;
    b_ok[i] = n < g.N;
    b_ptr[i] = reinterpret_cast<const ET*>(g.B) + (long long)(b_ok[i] ? n : 0) * g.ldb + koff;
  }

  // register staging (GL = 0): one 16-byte chunk per lane and pass, zero past
  // M / N / K
  f32x4 ra[A_CH], rb[B_CH];
  auto load_tile = [&](int kt) {
    const int k = kt * EPR + slot * CH;
    const bool kok = k < K;
#pragma unroll
    for (int i = 0; i < A_CH; ++i)
      ra[i] = (a_ok[i] && kok) ? *reinterpret_cast<const f32x4*>(a_ptr[i] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < B_CH; ++i)
      rb[i] = (b_ok[i] && kok) ? *reinterpret_cast<const f32x4*>(b_ptr[i] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto store_tile = [&](int buf) {
    float* la = lds + buf * BUF;
    float* lb = la + BM * BK;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int row = crow + i * ROWS_PER_PASS;
      *reinterpret_cast<f32x4*>(la + row * BK + swz(row, slot) * 4) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int row = crow + i * ROWS_PER_PASS;
      *reinterpret_cast<f32x4*>(lb + row * BK + swz(row, slot) * 4) = rb[i];
    }
  };

  // LDS-DMA staging (GL): global_load_lds writes a wave's 64 x 16 B lane-
  // linearly = 8 whole 128-B rows; the XOR swizzle moves to the SOURCE slot
  // (it is an involution, so the fragment reads below stay as they are).
  // Needs K % EPR == 0 (no partial k-tile to zero-fill).
  auto glds_tile = [&](int kt, int buf) {
    float* la = lds + buf * BUF;
    float* lb = la + BM * BK;
    const int wv = tid >> 6;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int row = crow + i * ROWS_PER_PASS;
      __builtin_amdgcn_global_load_lds(
          (const void*)(a_ptr[i] + (long long)kt * EPR + swz(row, slot) * CH),
          (__attribute__((address_space(3))) void*)(la + (i * ROWS_PER_PASS + wv * (64 / SLOTS)) * BK), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int row = crow + i * ROWS_PER_PASS;
      __builtin_amdgcn_global_load_lds(
          (const void*)(b_ptr[i] + (long long)kt * EPR + swz(row, slot) * CH),
          (__attribute__((address_space(3))) void*)(lb + (i * ROWS_PER_PASS + wv * (64 / SLOTS)) * BK), 16, 0, 0);
    }
  };

  // IL: chunk c (A rows, then B rows) of glds_tile(kt, buf), due before MFMA
  // number idx; past the last k-tile it re-fetches the last one (an L2 hit)
  // into the drained buffer, so every iteration issues the same DMAs
  static_assert(!IL || (GL && (MF16 == 1 || EMODE == E_FILTER)), "IL: LDS-DMA bf16 / fp8 filter sweeps, or the PIPE16 tiles");
  constexpr int NCH = A_CH + B_CH;
  // (PIPE16: the chunks go among the last k-step's MFMAs, one every
  // 4 FM FN / NCH, right after the barrier that frees their buffer)
  // (fp8: the first k-step's FM FN MFMAs, one chunk each)
  constexpr int IL_SPAN = IL ? (MF16 == 2 ? 36 : MF16 == 1 ? 4 * FM * FN : DT == DT_FP8 ? FM * FN : 18) : 0;
  static_assert(IL_SPAN <= (MF16 ? 4 * FM * FN * (BK / 16) : DT == DT_FP8 ? FM * FN * (BK / 16) : FM * FN * (BK / 8)),
                "IL: every chunk before an MFMA of the k-tile");
  auto glds_due = [&](int kt, int buf, int idx) {
    if constexpr (IL) {
      const int kc = kt < nk ? kt : nk - 1;
      float* la = lds + buf * BUF;
      float* lb = la + BM * BK;
      const int wv = tid >> 6;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if ((c * IL_SPAN) / NCH != idx) continue;
        const bool is_a = c < A_CH;
        const int i = is_a ? c : c - A_CH;
        const int row = crow + i * ROWS_PER_PASS;
        const ET* src = (is_a ? a_ptr[is_a ? i : 0] : b_ptr[is_a ? 0 : i]) + (long long)kc * EPR + swz(row, slot) * CH;
        __builtin_amdgcn_global_load_lds((const void*)src,
                                         (__attribute__((address_space(3))) void*)((is_a ? la : lb) +
                                                                                   (i * ROWS_PER_PASS + wv * (64 / SLOTS)) * BK),
                                         16, 0, 0);
      }
    }
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // MF16: sub-tile t = 2a + b (row half a, column half b) of tile (i, j)
  f32x4 acc4[MF16 ? FM : 1][MF16 ? FN : 1][4];
  if constexpr (MF16) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc4[i][j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int lr = lane & 31, lh = lane >> 5;

  // EP_LNFOLD: each of the tile's rows combines its producer's partials once,
  // before the k-loop (the prologue's barrier publishes them to the epilogue)
  if constexpr (LNF) {
    if (tid < BM) {
      const f32x4 r = m0 + tid < g.M ? ln_row_stats(g.stats_in, m0 + tid, g.stats_k, g.ln_eps) : f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(lds + 2 * BUF + LN_ROW * tid) = r;
    }
    // the tile's column sums per k tile (colsum [T][N]), zero past N and T
    const int T = (g.stats_k + 255) >> 8;
    for (int i = tid; i < LN_TMAX * BN / 4; i += NT) {
      const int t = i / (BN / 4), c = (i - t * (BN / 4)) * 4;
      const f32x4 v = (t < T && n0 + c < g.N) ? *reinterpret_cast<const f32x4*>(g.colsum + (long long)t * g.N + n0 + c)
                                              : f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(lds + 2 * BUF + LN_ROW * BM + t * BN + c) = v;
    }
  }

  constexpr bool PIPE16 = GL && MF16 == 1;
  if constexpr (PIPE16) {
    // ---- the PIPE16 k-loop: bf16 16x16x32 with LDS-DMA ----
    // The barrier of k-tile kt sits inside its last k-step, after that step's
    // fragments are in registers: wait for tile kt+1's DMA, barrier, DMA tile
    // kt+2 into the buffer just drained, read tile kt+1's first fragments,
    // THEN the last step's MFMAs — they hide the post-barrier LDS latency that
    // otherwise idles both waves of every SIMD at each k-tile.
    constexpr int S = BK / 16;
    static_assert(S % 2 == 0, "PIPE16: an even number of k-steps per k-tile");
    const int l16 = lane & 15, lg = lane >> 4;
    bf16x8 af[2][FM][2], bf[2][FN][2];
    // (the 16x16x32 fragment read is written out in each of the three k-loops
    // that use it: shared as a helper or a lambda it came out as different code)
    auto rd = [&](int buf, int st, bf16x8 (*a)[2], bf16x8 (*b)[2]) {
      const float* la = lds + buf * BUF;
      const float* lb = la + BM * BK;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int row = wm * WTM + i * 32 + h * 16 + l16;
          a[i][h] = *reinterpret_cast<const bf16x8*>(la + row * BK + swz(row, 4 * st + lg) * 4);
        }
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int row = wn * WTN + j * 32 + h * 16 + l16;
          b[j][h] = *reinterpret_cast<const bf16x8*>(lb + row * BK + swz(row, 4 * st + lg) * 4);
        }
    };
    glds_tile(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (nk > 1) glds_tile(1, 1);
    rd(0, 0, af[0], bf[0]);
    __builtin_amdgcn_s_setprio(1);
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      auto mfmas = [&](int st) {
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t)
              acc4[i][j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[st & 1][i][t >> 1], bf[st & 1][j][t & 1],
                                                                      acc4[i][j][t], 0, 0, 0);
      };
#pragma unroll
      for (int st = 0; st < S; ++st) {
        if (st + 1 < S) {
          // next step's reads between this step's MFMAs
          mfmas(st);
          rd(cur, st + 1, af[(st + 1) & 1], bf[(st + 1) & 1]);
          interleave<2 * (FM + FN), 4 * FM * FN>();
        } else {
          // this step's fragments: waited for and redefined by an empty asm
          // on both paths, so the MFMAs below (one copy: two spill the
          // accumulators) wait for nothing — not for the next tile's reads
          auto settle = [&]() {
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
              for (int h = 0; h < 2; ++h) asm volatile("" : "+v"(af[st & 1][i][h]));
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
              for (int h = 0; h < 2; ++h) asm volatile("" : "+v"(bf[st & 1][j][h]));
          };
          __builtin_amdgcn_sched_barrier(0);  // the previous step's MFMAs stay above the wait
          settle();
          if constexpr (IL) {
            // tile kt+2's DMA chunk by chunk among this step's MFMAs, into the
            // buffer the barrier just freed.  Past the last tile it fetches the
            // last tile again (an L2 hit); in the last iteration (no barrier:
            // other waves may still read buffer cur) into buffer cur ^ 1, free
            // since the previous iteration's barrier.  The epilogue's
            // __syncthreads retires it.
            if (kt + 1 < nk) {
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              __builtin_amdgcn_s_barrier();
              rd(cur ^ 1, 0, af[0], bf[0]);
            }
            // issued as one burst in the source; the scheduler spreads it
            // (interleave_il's VMEM groups: one DMA per 4 FM FN / NCH MFMAs)
            glds_tile(min(kt + 2, nk - 1), kt + 1 < nk ? cur : cur ^ 1);
            mfmas(st);
            interleave_il<4 * FM * FN, IL_SPAN, NCH>(0, 0);
          } else {
            if (kt + 1 < nk) {
              // every wave is done with buffer cur; tile kt+1's DMA has landed
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              __builtin_amdgcn_s_barrier();
              if (kt + 2 < nk) glds_tile(kt + 2, cur);
              rd(cur ^ 1, 0, af[0], bf[0]);
            }
            mfmas(st);
          }
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    if constexpr (IL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last spread DMA
    __syncthreads();  // every wave's last reads done: the epilogue reuses the LDS
  } else {
    // ---- the general k-loop: one barrier per k-tile, the next tile's global
    // loads (or DMA) in flight under this tile's MFMAs ----
    if constexpr (GL) {
      glds_tile(0, 0);
      __syncthreads();
    } else {
      load_tile(0);
      store_tile(0);
      __syncthreads();
    }

    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (!IL && kt + 1 < nk) {
        if constexpr (GL) glds_tile(kt + 1, cur ^ 1);
        else load_tile(kt + 1);
      }
      const float* la = lds + cur * BUF;
      const float* lb = la + BM * BK;
      if constexpr (MF16 == 2) {
        // MF16 = 2 (the 256x320 filter sweep on v_mfma_f32_16x16x32_bf16): one
        // fragment set per 32-deep k-step, read whole before its MFMAs (two sets
        // do not fit beside the 160 accumulator registers); the partner wave on
        // the SIMD covers the read latency.  Same lane -> k map as below.
        constexpr int S = BK / 16;
        const int l16 = lane & 15, lg = lane >> 4;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int st = 0; st < S; ++st) {
          bf16x8 af[FM][2], bf[FN][2];
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int row = wm * WTM + i * 32 + h * 16 + l16;
              af[i][h] = *reinterpret_cast<const bf16x8*>(la + row * BK + swz(row, 4 * st + lg) * 4);
            }
#pragma unroll
          for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int row = wn * WTN + j * 32 + h * 16 + l16;
              bf[j][h] = *reinterpret_cast<const bf16x8*>(lb + row * BK + swz(row, 4 * st + lg) * 4);
            }
#pragma unroll
          for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                glds_due(kt + 1, cur ^ 1, st * 4 * FM * FN + (j * FM + i) * 4 + t);
                acc4[i][j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][t >> 1], bf[j][t & 1], acc4[i][j][t], 0, 0, 0);
              }
          if constexpr (IL) interleave_il<4 * FM * FN, IL_SPAN, NCH>(st * 4 * FM * FN, 0);
        }
        __builtin_amdgcn_s_setprio(0);
      } else if constexpr (MF16) {
        // BK/16 k-steps of 32; lane group g = lane>>4 holds k = 32s + 8g .. +7
        // = 16-B slot 4s + g of rows (lane & 15) of each 16-row half.
        constexpr int S = BK / 16;
        const int l16 = lane & 15, lg = lane >> 4;
        bf16x8 af[2][FM][2], bf[2][FN][2];
        auto rd = [&](int st, bf16x8 (*a)[2], bf16x8 (*b)[2]) {
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int row = wm * WTM + i * 32 + h * 16 + l16;
              a[i][h] = *reinterpret_cast<const bf16x8*>(la + row * BK + swz(row, 4 * st + lg) * 4);
            }
#pragma unroll
          for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int row = wn * WTN + j * 32 + h * 16 + l16;
              b[j][h] = *reinterpret_cast<const bf16x8*>(lb + row * BK + swz(row, 4 * st + lg) * 4);
            }
        };
        rd(0, af[0], bf[0]);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int st = 0; st < S; ++st) {
          if (st + 1 < S) rd(st + 1, af[(st + 1) & 1], bf[(st + 1) & 1]);
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
              for (int t = 0; t < 4; ++t)
                acc4[i][j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[st & 1][i][t >> 1], bf[st & 1][j][t & 1],
                                                                        acc4[i][j][t], 0, 0, 0);
          if (st + 1 < S) interleave<2 * (FM + FN), 4 * FM * FN>();
        }
        __builtin_amdgcn_s_setprio(0);
      } else if constexpr (DT == DT_BF16) {
        // BK/8 k-steps of 16; lane half h holds k = 16s + 8h .. +7 = 16-B slot 2s + h.
        // Fragments are double-buffered in registers: step s+1's ds_reads are
        // issued before step s's MFMAs, so LDS latency hides under the MFMAs.
        constexpr int S = BK / 8;
        bf16x8 af[2][FM], bf[2][FN];
        auto rd = [&](int st, bf16x8* a, bf16x8* b) {
#pragma unroll
          for (int i = 0; i < FM; ++i) {
            const int row = wm * WTM + i * 32 + lr;
            a[i] = *reinterpret_cast<const bf16x8*>(la + row * BK + swz(row, 2 * st + lh) * 4);
          }
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            const int row = wn * WTN + j * 32 + lr;
            b[j] = *reinterpret_cast<const bf16x8*>(lb + row * BK + swz(row, 2 * st + lh) * 4);
          }
        };
        rd(0, af[0], bf[0]);
        // MFMA cluster at raised priority (cdna_hip_programming.md T5; measured
        // +2 % on the ViT linears and the bf16 sweep)
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int st = 0; st < S; ++st) {
          if (st + 1 < S) rd(st + 1, af[(st + 1) & 1], bf[(st + 1) & 1]);
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) {
              glds_due(kt + 1, cur ^ 1, st * FM * FN + i * FN + j);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[st & 1][i], bf[st & 1][j], acc[i][j], 0, 0, 0);
            }
          if constexpr (IL) interleave_il<FM * FN, IL_SPAN, NCH>(st * FM * FN, st + 1 < S ? FM + FN : 0);
          else if (st + 1 < S) interleave<FM + FN, FM * FN>();
        }
        __builtin_amdgcn_s_setprio(0);
      } else {
        // fp8 on the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 both
        // operands, every E8M0 block scale = 127 = 1.0; the per-row fp32 scales
        // stay in the epilogue): 2x the k per clock of the non-scaled
        // 32x32x16_fp8 form.  BK/16 k-steps of 64; lane half h holds the 32
        // bytes of 16-B slots 4s+2h, 4s+2h+1.  A and B fragments are read by
        // the same lane->k map, so each dot product covers every k once.
        constexpr int S = BK / 16;
        i32x8 af[2][FM], bf[2][FN];
        auto rd32 = [&](const float* base, int row, int st) {
          const i32x4 lo = *reinterpret_cast<const i32x4*>(base + row * BK + swz(row, 4 * st + 2 * lh) * 4);
          const i32x4 hi = *reinterpret_cast<const i32x4*>(base + row * BK + swz(row, 4 * st + 2 * lh + 1) * 4);
          return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        };
        auto rd = [&](int st, i32x8* a, i32x8* b) {
#pragma unroll
          for (int i = 0; i < FM; ++i) a[i] = rd32(la, wm * WTM + i * 32 + lr, st);
#pragma unroll
          for (int j = 0; j < FN; ++j) b[j] = rd32(lb, wn * WTN + j * 32 + lr, st);
        };
        rd(0, af[0], bf[0]);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int st = 0; st < S; ++st) {
          // IL: the next k-tile's DMA as one burst in the source, spread by the
          // scheduler among the first k-step's MFMAs (past the last k-tile: the
          // last one again, into the drained buffer)
          if (IL && st == 0) glds_tile(min(kt + 1, nk - 1), cur ^ 1);
          if (st + 1 < S) rd(st + 1, af[(st + 1) & 1], bf[(st + 1) & 1]);
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[st & 1][i], bf[st & 1][j], acc[i][j],
                                                                           0, 0, 0, 127, 0, 127);
          if constexpr (IL) {
            if (st == 0) interleave_il<FM * FN, IL_SPAN, NCH, 2>(0, st + 1 < S ? FM + FN : 0);
            else if (st + 1 < S) interleave2<FM + FN, FM * FN>();
          } else if (st + 1 < S) {
            interleave2<FM + FN, FM * FN>();
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
      if constexpr (!GL) {
        if (kt + 1 < nk) store_tile(cur ^ 1);
      }
      __syncthreads();  // with GL: also the vmcnt(0) that retires the DMA
    }
  }
  if constexpr (MF16) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][4 * t + r] = acc4[i][j][t][r];
  }

  // ---- epilogue ----
  // 32x32 C/D map: col (N index) = lane & 31, row (M index) = (r&3) + 8(r>>2) + 4(lane>>5)
  // per-row dequantisation (fp8 only; bf16 rows are unscaled — compiled into
  // those kernels, this block's 160 hoisted scale loads spilled ~150 VGPRs
  // of the 256x320 bf16 sweep tile).  Row scales one at a time, the FN column
  // scales held.
  if constexpr (DT == DT_FP8) {
    if (g.scale_a != nullptr || g.scale_b != nullptr) {
      float sb[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn * WTN + j * 32 + lr;
        sb[j] = (g.scale_b != nullptr && n < g.N) ? g.scale_b[n] : 1.f;
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const float sa = (g.scale_a != nullptr && m < g.M) ? g.scale_a[m] : 1.f;
#pragma unroll
          for (int j = 0; j < FN; ++j) acc[i][j][r] = acc[i][j][r] * sa * sb[j];
        }
    }
  }
  if constexpr (MF16 && EMODE == E_SCORES_T) {
    // sub-tile t: rows acc_row(i, 4t) .. +3 (consecutive), one column
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n0 + wn * WTN + acc_col<true>(j, 4 * q, lane);
          const int mb = m0 + wm * WTM + acc_row<true>(i, 4 * q, lane);
          store_rows4(g, n < g.N, acc[i][j], 4 * q, n, mb);
        }
  } else if constexpr (MF16 && EMODE == E_FILTER) {
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int n = n0 + wn * WTN + acc_col<true>(j, 4 * b, lane);
        const bool nok = n < g.N;
        const float t = nok ? g.tau[n] : __builtin_inff();
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = 8 * a + 4 * b + e;
              const int m = m0 + wm * WTM + acc_row<true>(i, r, lane);
              filter_emit(g, nok, acc[i][j][r], t, n, m);
            }
      }
  } else {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + wn * WTN + j * 32 + lr;
      const bool nok = n < g.N;
      if constexpr (EMODE == E_STORE) {
        // handled below through LDS (the loop stays for E_STORE: without this
        // first read of g.N the stored-C kernels compile to different code)
      } else if constexpr (EMODE == E_SCORES_T) {
#pragma unroll
        for (int i = 0; i < FM; ++i) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int mb = m0 + wm * WTM + i * 32 + 8 * q + 4 * lh;
            store_rows4(g, nok, acc[i][j], 4 * q, n, mb);
          }
        }
      } else {  // E_FILTER (gemm_tile.hpp filter_emit)
        const float t = nok ? g.tau[n] : __builtin_inff();
#pragma unroll
        for (int i = 0; i < FM; ++i) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            filter_emit(g, nok, acc[i][j][r], t, n, m);
          }
        }
      }
    }
  }

  // E_STORE: through LDS (gemm_epilogue.hpp)
  if constexpr (EMODE == E_STORE)
    epilogue_store<WM, WN, FM, FN, 2 * BUF, (bool)MF16, EPI>(g, Cb, acc, lds, m0, n0, 1.f, LNF ? lds + 2 * BUF : nullptr);
}

template <int WM, int WN, int FM, int FN, int EM, int DT, int MINB, int GL = 0, int MF16 = 0, int EPI = -1, int IL = 0>
static hipError_t launch_t1(const GemmArgs& g, hipStream_t s) {
  return launch_tiles<32 * FM * WM, 32 * FN * WN, 64 * WM * WN>(gemm_lp_kernel<WM, WN, FM, FN, EM, DT, MINB, GL, MF16, EPI, IL>, g,
                                                                 s);
}

// the instance of RR_GEMM_LP_INSTANCES and RR_GEMM_EPI_SETS that the route names, for one (epilogue, dtype)
template <int EM, int DT>
static hipError_t launch_lp(const GemmRoute& r, const GemmArgs& g, hipStream_t s) {
#define RR_E(FLAGS, FOLD, A3)                                                      \
  if constexpr (EM == E_STORE && (!FOLD || (32 * FN_ * WN_ == 256 && MF16_ == 1))) \
    if (r.epi == (FLAGS)) return launch_t1<WM_, WN_, FM_, FN_, EM, DT, MINB_, GL_, MF16_, (FLAGS), IL_>(g, s);
#define RR_X(CFG, WM, WN, FM, FN, MINB, GL, MF16, IL, WHEN)                                                        \
  if constexpr (WHEN) {                                                                                            \
    if (r.cfg == CFG && r.wm == WM && r.wn == WN && r.fm == FM && r.fn == FN && r.bk == 0 && r.minb == MINB &&     \
        r.gl == GL && r.mf16 == MF16 && r.il == IL) {                                                              \
      constexpr int WM_ = WM, WN_ = WN, FM_ = FM, FN_ = FN, MINB_ = MINB, GL_ = GL, MF16_ = MF16, IL_ = IL;        \
      RR_GEMM_EPI_SETS(RR_E)                                                                                       \
      return r.epi == -1 ? launch_t1<WM, WN, FM, FN, EM, DT, MINB, GL, MF16, -1, IL>(g, s) : hipErrorInvalidValue; \
    }                                                                                                              \
  }
  RR_GEMM_LP_INSTANCES(RR_X)
#undef RR_X
#undef RR_E
  return hipErrorInvalidValue;
}

hipError_t launch_gemm_lp(const GemmRoute& r, int emode, int dt, const GemmArgs& g, hipStream_t s) {
  if (dt == DT_BF16 && emode == E_STORE) return launch_lp<E_STORE, DT_BF16>(r, g, s);
  if (dt == DT_BF16 && emode == E_SCORES_T) return launch_lp<E_SCORES_T, DT_BF16>(r, g, s);
  if (dt == DT_BF16 && emode == E_FILTER) return launch_lp<E_FILTER, DT_BF16>(r, g, s);
  if (dt == DT_FP8 && emode == E_SCORES_T) return launch_lp<E_SCORES_T, DT_FP8>(r, g, s);
  if (dt == DT_FP8 && emode == E_FILTER) return launch_lp<E_FILTER, DT_FP8>(r, g, s);
  return hipErrorInvalidValue;  // fp8 has no stored-C GEMM
}

}  // namespace rr
