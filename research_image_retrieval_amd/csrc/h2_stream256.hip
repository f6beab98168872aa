// h2_stream256.hip — the persistent 256x256 one-accumulator tile (config 15)
// of the f16x2 split GEMM core (h2_tile.hip: the split and the tile table).
//
// Config 12 (8 waves of 128x64 on v_mfma_f32_32x32x16_f16, one accumulator
// set, BK 32, dense A) as one block per CU walking its tiles as ONE k-stream,
// as config 8 does for config 4: the B DMA one k-tile and the A loads two
// k-tiles ahead across tile boundaries, so a tile's epilogue runs with the
// next tile's first k-tile in LDS and its second in flight, and a fresh tile
// never pays the cold prologue of a new block.  The epilogue goes in four
// 64-row slabs (slab s = MFMA row tile s of every wave: rows 32 s + [0, 32)
// and 128 + 32 s + [0, 32), so all eight waves stage every slab) through the
// stage buffer the tile's last k-tile released, and slab s + 1's residual rows
// are in flight while slab s is staged and stored: one exposed residual round
// trip per tile instead of config 12's two (its two 128-row slabs each load
// their residual after staging, and only half the waves stage each slab).
// Same per-accumulator k order (per 16-deep k-step: a0b0, a0b1, a1b0) and
// epilogue arithmetic as config 12: bit-identical to it.  FN = 1: the 256x128
// form (waves of 128x32, two B DMA instructions per wave, 96 KB of LDS) for
// N = 128; FN = 1, WM = 4: the 256x64 form (waves 4 x 2 of 64x32, one B DMA
// instruction per wave spanning both planes, slabs of four 32-row bands, 80
// KB) for N = 64, with config 7's two accumulator sets (ACC2: its arithmetic
// at K = 64, where one accumulator's error passes the exact-fp32 core's).
// Every column of the 256x128 form is config 12's column bit for bit, the
// 256x64 form's output config 7's.
// Counted waits rely only on loads returning in issue order among
// themselves: each names how many younger loads may remain, and stores are
// never counted (a wait issued after stores also covers them, which makes it
// longer, never shorter); where fewer loads were issued (rows past M) the
// wait is longer, never shorter.
#include <algorithm>

#include "h2_common.hpp"
#include "h2_route.hpp"

namespace rr {

template <int EPI, int FN = 2, int WM = 2, int ACC2 = 0>
__global__ __launch_bounds__(512, 1) void gemm_s3q_kernel(GemmArgs g, int tiles_n, int ntiles) {
  static_assert((EPI & EP_SCALE) != 0, "f16x2: scaled epilogue");
  static_assert((WM == 2 && (FN == 1 || FN == 2)) || (WM == 4 && FN == 1), "256x256, 256x128 or 256x64");
  typedef f16x8 frag_t;
  constexpr int NP = 2, FM = 8 / WM, BK = 32, NT = 512, NW = 8, WN = NW / WM;
  constexpr int WTM = 32 * FM, WTN = 32 * FN, BM = 256, BN = WN * WTN, SL = BK / 8;
  constexpr int A_EL = NP * BM * BK, BUF = A_EL + NP * BN * BK;
  // stage stride: a stage also holds one 64-row slab of C (rows padded by 8
  // floats: the 32x32 accumulator writes hit distinct banks)
  constexpr int CS = BN + 8;
  constexpr int STG = BUF > WM * 32 * CS * 2 ? BUF : WM * 32 * CS * 2;
  constexpr int B_INS = NP * BN / (64 / SL) / NW;  // LDS-DMA instructions per wave per k-tile (4 / 2)
  constexpr int IPP = BN >= 128 ? BN / 128 : 1;     // of them per plane (64 columns: one spans both)
  constexpr int A_RPP = NT / SL, A_CH = BM / A_RPP;  // 128 rows per pass, 2 chunks per thread
  constexpr int A_LD = 2 * A_CH;                     // A loads per thread per k-tile
  static_assert(B_INS * NW * (64 / SL) == NP * BN && A_CH * A_RPP == BM, "staging must tile the block");
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * STG];
  const uint32_t a_amax_w = amax_load_slot(g.a_amax);
  float a_sc = 1.f, a_isc = 1.f, am = 0.f;

  // round stagger: every block is resident from the start, so half of them
  // (every other XCD slot) start later and the halves stay out of phase
  if (g.stagger_sleeps > 0 && ((blockIdx.x >> 3) & 1))
    for (int i = 0; i < g.stagger_sleeps; ++i) __builtin_amdgcn_s_sleep(32);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int lr = lane & 31, lh = lane >> 5;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);  // (scalar: the amax slot at the end)
  const int G = gridDim.x, bid = blockIdx.x;
  const int nk = g.K / BK;
  const int my_tiles = (ntiles - bid + G - 1) / G;
  const int J = my_tiles * nk;  // k-tiles in this block's stream
  // local tile tl -> origin (as config 8: virtual block bid + tl G keeps the
  // block's XCD, then the bijective XCD remap)
  auto tile_origin = [&](int tl, int& m0, int& n0) __attribute__((always_inline)) {
    const int v = bid + tl * G;
    const int xcd = v & 7, q8 = ntiles >> 3, r8 = ntiles & 7;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (v >> 3);
    const int tn = wgid % tiles_n, tm = wgid / tiles_n;
    m0 = tm * BM;
    n0 = tn * BN;
  };

  // ---- A loader: two 8-k chunks per thread (rows t / 4 and 128 + t / 4),
  // two k-tiles ahead of the MFMAs, advancing along the stream; past the
  // stream's end it runs into a virtual tile whose rows clamp to M - 1 ----
  // (32-bit byte offsets from the uniform base, saddr form: 64-bit row
  // pointers spilled this kernel; the host keeps A and C below 4 GB)
  uint32_t a_off[A_CH];
  int a_kt = 0, a_tl = 0;
  auto a_tile = [&](int tl) __attribute__((always_inline)) {
    int m0, n0;
    tile_origin(tl, m0, n0);
    const int t = s3_opaque(tid);
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int m = min(m0 + t / SL + i * A_RPP, g.M - 1);
      a_off[i] = ((uint32_t)m * (uint32_t)g.lda + (uint32_t)(t % SL) * 8u) * 4u;
    }
  };
  a_tile(0);
  f32x4 ra2[2][A_CH][2];
  auto load_a = [&](int rb) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i)
      asm volatile("global_load_dwordx4 %0, %2, %3\n\tglobal_load_dwordx4 %1, %2, %3 offset:16"
                   : "=&v"(ra2[rb][i][0]), "=&v"(ra2[rb][i][1])
                   : "v"(a_off[i] + (uint32_t)(a_kt * BK * 4)), "s"(g.A)
                   : "memory");
    if (++a_kt == nk) {
      a_kt = 0;
      a_tile(++a_tl);
    }
  };
  u32x4 pk[A_CH][NP];
  auto split_a = [&](int rb) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) split2h8(ra2[rb][i], a_sc, pk[i][0], pk[i][1]);
  };
  auto write_a = [&](int buf) __attribute__((always_inline)) {
    uint16_t* la = lds + buf * STG;
    const int a_slot = tid % SL, a_row = tid / SL;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int row = a_row + i * A_RPP;
      const int off = row * BK + pswz<BK>(row, a_slot) * 8;
#pragma unroll
      for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x4*>(la + p * BM * BK + off) = pk[i][p];
    }
  };
  auto launder_a = [&](int rb) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      s3_launder(ra2[rb][i][0]);
      s3_launder(ra2[rb][i][1]);
    }
  };

  // ---- B loader (as config 8): instruction i of a wave DMAs plane i / IPP,
  // plane rows 128 (i % IPP) + 16 wave + lane / 4 ----
  const uint16_t* Bp = reinterpret_cast<const uint16_t*>(g.B);
  const int b_r = wave * (64 / SL) + lane / SL;
  const int b_sw = pswz<BK>(b_r, lane % SL) * 8;  // the same for every i
  const uint16_t* b_src = Bp;
  int b_kt = 0, b_tl = 0;
  auto b_tile = [&](int tl) __attribute__((always_inline)) {
    int m0, n0;
    tile_origin(tl, m0, n0);
    b_src = Bp + (long long)(b_r / BN) * g.b_plane + (long long)(n0 + b_r % BN) * g.ldb + b_sw;
  };
  b_tile(0);
  auto glds_b = [&](int buf) __attribute__((always_inline)) {
    uint16_t* lb = lds + buf * STG + A_EL;
#pragma unroll
    for (int i = 0; i < B_INS; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(b_src + (i / IPP) * g.b_plane + (long long)(i % IPP) * 128 * g.ldb +
                                                     b_kt * BK),
                                       (__attribute__((address_space(3))) void*)(lb + (i * NW + wave) * (64 / SL) * BK),
                                       16, 0, 0);
    if (++b_kt == nk) {
      b_kt = 0;
      b_tile(++b_tl);
    }
  };

  // ---- MFMAs: config 12's 16-deep k-step (st = 0, 1 of the k-tile) ----
  // ACC2: config 7's two accumulator sets (a0b0 in acc, a0b1 + a1b0 in lo,
  // summed before the epilogue)
  f32x16 acc[FM][FN], lo[ACC2 ? FM : 1][ACC2 ? FN : 1];
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc[i][j][r] = 0.f;
          if constexpr (ACC2) lo[i][j][r] = 0.f;
        }
  };
  zero_acc();
  auto compute_st = [&](int cur, int st) __attribute__((always_inline)) {
    const uint16_t* la = lds + cur * STG;
    const uint16_t* lb = la + A_EL;
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
      for (int j = 0; j < FN; ++j) acc[i][j] = s3_mf32(a[0][i], b[0][j], acc[i][j]);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        f32x16& L = ACC2 ? lo[ACC2 ? i : 0][ACC2 ? j : 0] : acc[i][j];
        L = s3_mf32(a[0][i], b[1][j], L);
        L = s3_mf32(a[1][i], b[0][j], L);
      }
  };

  // ---- epilogue of local tile tl through stage buffer `buf` (free) ----
  // Eight 32-row bands, band b = rows 128 (b & 1) + 32 (b >> 1) + [0, 32);
  // bands 2s and 2s + 1 form slab s (MFMA row tile s of every wave), staged
  // together.  Band b's residual rows are loaded two bands ahead (issued
  // before band b - 2 is stored): at most three bands (48 registers) in
  // flight -- a whole slab ahead (64) spilled the k-loop.
  constexpr int C4 = BN / 4, HITERS = 32 * C4 / NT;  // 4 / 2 / 1 row chunks per thread and band
  static_assert(HITERS * 2 <= 16 && (HITERS == 1 || HITERS % 2 == 0), "the counted waits' immediates");
  constexpr int NB = WM * FM, RD = 2;                  // bands, residual look-ahead (bands)
  RR_PH_DECL
  auto epilogue = [&](int tl, int buf) __attribute__((always_inline)) {
    int m0, n0;
    tile_origin(tl, m0, n0);
    const int te = s3_opaque(tid);
    const int c40 = te % C4;
    f32x4 bias_v[1] = {f32x4{0.f, 0.f, 0.f, 0.f}}, sc_v[1];
    f32x4 res[RD + 1][HITERS];  // ring of bands
    auto band_row0 = [&](int bb) { return (bb % WM) * WTM + (bb / WM) * 32; };
    auto load_band = [&](int bb) __attribute__((always_inline)) {
      if constexpr ((EPI & EP_RES) != 0) {
        // (addresses from an opaque thread index per band: hoisted, every
        // band's addresses would be live through the epilogue and spill)
        const int tq = s3_opaque(tid);
        const int cq = tq % C4, rq = tq / C4;
#pragma unroll
        for (int it = 0; it < HITERS; ++it) {
          const int m = min(m0 + band_row0(bb) + rq + it * (NT / C4), g.M - 1);
          const uint32_t o = ((uint32_t)m * (uint32_t)g.ldc + (uint32_t)(n0 + cq * 4)) * 4u;
          if constexpr ((EPI & EP_SC1) != 0)  // streamed: nt
            asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=&v"(res[bb % (RD + 1)][it]) : "v"(o), "s"(g.residual) : "memory");
          else
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(res[bb % (RD + 1)][it]) : "v"(o), "s"(g.residual) : "memory");
        }
      }
    };
    float* ct = reinterpret_cast<float*>(lds + buf * STG);  // [2 bands x 32 rows][CS]
    // (wave and lane from the opaque index too: the staging addresses are
    // loop-invariant and would otherwise be held through the k-loop)
    const int le = te & 63, we = te >> 6;
    auto stage = [&](int sl) __attribute__((always_inline)) {
      float* cw = ct + ((we % WM) * 32) * CS + (we / WM) * WTN;
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          cw[acc_row<false>(0, r, le) * CS + acc_col<false>(j, r, le)] =
              ACC2 ? acc[sl][j][r] + lo[ACC2 ? sl : 0][ACC2 ? j : 0][r] : acc[sl][j][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      RR_PH(4);
    };
    // the bias / column scales first, by inline asm as well (a plain load's
    // use would make hipcc wait vmcnt(0), the look-ahead bands included):
    // older than every band, so band 0's wait covers them
    if ((EPI & EP_BIAS) && g.bias != nullptr)
      asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(bias_v[0]) : "v"(g.bias + n0 + c40 * 4) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(sc_v[0]) : "v"(g.col_scale + n0 + c40 * 4) : "memory");
    load_band(0);
    load_band(1);
    // band bb's wait: vmcnt(the loads issued after it: bands bb + 1 ..
    // bb + RD, HITERS each).  The stores issued after it (bands bb - RD ..
    // bb - 1) are not counted: loads return in order among themselves, but
    // nothing is assumed about stores against loads, so the wait also covers
    // those stores (measured free: 0.584 vs 0.590 ms counting them,
    // profiles/r05j_probe.txt)
#pragma unroll
    for (int bb = 0; bb < NB; ++bb) {
      if (bb % WM == 0) stage(bb / WM);
      if (bb + RD < NB) load_band(bb + RD);
      if constexpr ((EPI & EP_RES) != 0) {
        const int ahead = (NB - 1 - bb < RD ? NB - 1 - bb : RD);
        const int younger = HITERS * ahead;
        // (s_waitcnt needs an immediate: the few values this unrolled loop produces)
        switch (younger) {
#define RR_VMW(n) \
  case n: asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory"); break;
          RR_VMW(0) RR_VMW(1) RR_VMW(2) RR_VMW(3) RR_VMW(4) RR_VMW(6) RR_VMW(8) RR_VMW(10) RR_VMW(12) RR_VMW(14)
#undef RR_VMW
          default: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
        }
#pragma unroll
        for (int it = 0; it < HITERS; ++it) asm volatile("" : "+v"(res[bb % (RD + 1)][it]));
      } else if (bb == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      RR_PH(5);
      if (bb == 0) {
        asm volatile("" : "+v"(bias_v[0]));
        asm volatile("" : "+v"(sc_v[0]));
        sc_v[0] *= a_isc;
      }
      store_slab<EPI, 2, HITERS, NT, C4, CS, 1>(g, g.C, ct + (bb % WM) * 32 * CS, bias_v, res[bb % (RD + 1)], te,
                                                m0 + band_row0(bb), n0, sc_v, am);
      if (bb % WM == WM - 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // every LDS read of the slab done (the last also frees `buf`)
        asm volatile("" ::: "memory");
      }
      RR_PH(6);
    }
    zero_acc();
  };

  // ---- the stream: k-tile j of the block = k-tile j % nk of local tile j / nk ----
  load_a(0);
  glds_b(0);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(B_INS) : "memory");  // A(0) landed
  launder_a(0);
  {
    // uniform: the exponent and both powers of two stay in scalar registers
    const int e = __builtin_amdgcn_readfirstlane(h2_exp(amax_reduce(a_amax_w)));
    a_sc = __int_as_float((127 + e) << 23);
    a_isc = __int_as_float((127 - e) << 23);
  }
  split_a(0);
  write_a(0);
  load_a(1);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD) : "memory");  // B(0) landed
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  int c_kt = 0, c_tl = 0;
  // iteration j (stage cur = j & 1 holds k-tile j, register buffer cur ^ 1
  // holds A(j+1)): B DMA of j+1, A loads of j+2, the first k-step, the split
  // of A(j+1) under the second, then -- after a tile's last k-tile -- its
  // epilogue through stage cur.  A(j+1) of a tile's first k-tile was issued
  // before the previous epilogue, whose waits already covered it: that
  // iteration skips the A wait (it would wait for the epilogue's stores).
  auto iter = [&](int cur, int j) __attribute__((always_inline)) {
    glds_b(cur ^ 1);
    load_a(cur);
    compute_st(cur, 0);
    RR_PH(0);
    if (c_kt != 0 || c_tl == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD + B_INS) : "memory");  // A(j+1) landed
    launder_a(cur ^ 1);
    RR_PH(1);
    split_a(cur ^ 1);
    compute_st(cur, 1);
    write_a(cur ^ 1);
    RR_PH(2);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD) : "memory");  // B DMA of j+1 landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    RR_PH(3);
    if (++c_kt == nk) {
      c_kt = 0;
      epilogue(c_tl++, cur);
    }
    // the stream's last k-tile: the clamped tail loads (into buffer cur) are
    // still in flight; that buffer stays live until they have landed, so no
    // later value is allocated to it (laundering both buffers after the loop
    // instead kept 32 registers live through every epilogue and spilled)
    if (j == J - 1) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      launder_a(cur);
    }
  };
  RR_PH(7);
  for (int j = 0; j < J; j += 2) {
    iter(0, j);
    if (j + 1 < J) iter(1, j + 1);
  }
  RR_PH_FLUSH();
  if constexpr ((EPI & EP_AMAX) != 0) {
    if (g.c_amax != nullptr) amax_publish(g.c_amax, am, bid * NW + wave_u);
  }
}

template <int EPI, int FN = 2, int WM = 2, int ACC2 = 0>
static hipError_t launch_s3q_t(GemmArgs g, hipStream_t s, int n_cu, int stagger) {
  const long long tiles_m = (g.M + 255) / 256, tiles_n = g.N / (32 * FN * (8 / WM));
  const long long ntiles = tiles_m * tiles_n;
  if (ntiles <= 0) return hipSuccess;
  if (ntiles * (g.K / 32) > 0x7fffffffLL) return hipErrorInvalidValue;
  // 32-bit byte offsets (checked by the caller, s3q_fits)
  const int slots = std::max(8, n_cu & ~7);
  const int grid = ntiles <= slots ? (int)ntiles : slots;
  g.stagger_blocks = grid;
  g.stagger_sleeps = ntiles > 2LL * grid ? stagger : 0;
  hipLaunchKernelGGL((gemm_s3q_kernel<EPI, FN, WM, ACC2>), dim3((unsigned)grid), dim3(512), 0, s, g, (int)tiles_n, (int)ntiles);
  return hipGetLastError();
}
// the route's form (h2_stream256_route; s3q_shape and s3q_fits hold for g)
hipError_t launch_s3q(const H2Route& r, const GemmArgs& g, hipStream_t s, int n_cu, int st) {
  // residual epilogues streamed (EP_SC1): output stores sc1, residual
  // loads nt -- neither keeps XCD L2 lines the row tile's other column
  // tiles still re-read (256->1024 + residual 0.604 -> 0.579 ms, 512->2048
  // 0.470 -> 0.466; the embed 69.82 -> 69.47 ms with every config-15
  // layer streamed).  Without a residual the plain policy stays: streamed
  // stores there ran 1024->256 0.395 -> 0.406 ms (profiles/r05i_sweep.txt,
  // r05j_probe2.txt)
  return h2_ep_dispatch<true>(g, [&](auto ep) {
    constexpr int EPI = decltype(ep)::value;
    if (r.wm == 4 && r.fn == 1 && r.acc == 2) return launch_s3q_t<EPI, 1, 4, 1>(g, s, n_cu, st);
    if (r.wm == 2 && r.fn == 1 && r.acc == 1) return launch_s3q_t<EPI, 1>(g, s, n_cu, st);
    if (r.wm == 2 && r.fn == 2 && r.acc == 1) return launch_s3q_t<EPI>(g, s, n_cu, st);
    return hipErrorInvalidValue;
  });
}

#if RR_S3_PHASES
int h2_stream256_phases(unsigned long long* out) { return s3_phases_take(out); }
#endif

}  // namespace rr
