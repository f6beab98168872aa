// h2_stream.hip — the persistent 128x256 tile (config 8) of the f16x2 split
// GEMM core (h2_tile.hip: the split and the tile table) and its two-segment
// form (launch_gemm_h2_seg2).
//
// The config-4 tile (8 waves of 64x64, BK 32, v_mfma_f32_16x16x32_f16, dense
// A or the Cin % 32 == 0 conv A) as one block per CU that walks its tiles as
// ONE continuous k-stream: the B DMA runs one k-tile and the A loads two
// k-tiles ahead ACROSS tile boundaries, so while a tile's epilogue runs the
// next tile's first k-tile already sits in LDS and its second is in flight
// (a fresh block pays that round trip before its first MFMA), and the
// epilogue's stores drain under the next tile's first k-tiles.  The epilogue
// stages C through the stage buffer the tile's last k-tile just released (two
// 64-row slabs of 64 KB), with every bias / residual load issued before the
// staging.  Same per-accumulator k order and epilogue arithmetic as config 4:
// the results are bit-identical to it.
// (s3_opaque: per-thread address math built from it inside a tile loop's
// epilogue / loader switch cannot be hoisted out of the loop -- its results
// would then be live through the whole k-loop and spill it)
#include <algorithm>

#include "h2_common.hpp"

namespace rr {

template <int EPI, int SEG2 = 0>
__global__ __launch_bounds__(512, 1) void gemm_s3p_kernel(GemmArgs g, int tiles_n, int ntiles) {
  static_assert((EPI & EP_SCALE) != 0, "f16x2: scaled epilogue");
  typedef f16x8 frag_t;
  constexpr int NP = 2;
  constexpr int WM = 2, FM = 2, FN = 2, BK = 32, NT = 512, NW = 8;
  constexpr int WTM = 64, WTN = 64, BM = 128, BN = 256, SL = BK / 8;
  constexpr int A_EL = NP * BM * BK, BUF = A_EL + NP * BN * BK;
  // stage stride: a stage also stages one 64-row slab of C in the epilogue
  // (rows padded by 4 floats: the 16x16 accumulator writes hit distinct banks)
  constexpr int CS = BN + 4;
  constexpr int STG = BUF > 64 * CS * 2 ? BUF : 64 * CS * 2;
  constexpr int B_INS = NP * BN / (64 / SL) / NW;  // LDS-DMA instructions per wave per k-tile (4)
  constexpr int A_LD = 2;                          // A loads per thread per k-tile
  static_assert(B_INS * NW * (64 / SL) == NP * BN, "B staging must tile the block");
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * STG];
  uint32_t a_amax_w = amax_load_slot(g.a_amax);
  if constexpr (SEG2) {  // one split scale for both segments: the larger max
    const uint32_t w2 = amax_load_slot(g.a2_amax);
    a_amax_w = w2 > a_amax_w ? w2 : a_amax_w;
  }
  float a_sc = 1.f, a_isc = 1.f, am = 0.f;

  // round stagger: every block is resident from the start, so half of them
  // (every other XCD slot) start later and the halves stay out of phase
  if (g.stagger_sleeps > 0 && ((blockIdx.x >> 3) & 1))
    for (int i = 0; i < g.stagger_sleeps; ++i) __builtin_amdgcn_s_sleep(32);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int G = gridDim.x, bid = blockIdx.x;
  const int nk = g.K / BK;
  const int my_tiles = (ntiles - bid + G - 1) / G;
  const int J = my_tiles * nk;  // k-tiles in this block's stream
  // local tile tl -> origin: virtual block v = bid + tl*G keeps this block's
  // XCD (G % 8 == 0 whenever a block owns more than one tile), then the same
  // bijective XCD remap as the one-tile-per-block kernel
  auto tile_origin = [&](int tl, int& m0, int& n0) {
    const int v = bid + tl * G;
    const int xcd = v & 7, q8 = ntiles >> 3, r8 = ntiles & 7;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (v >> 3);
    const int tn = wgid % tiles_n, tm = wgid / tiles_n;
    m0 = tm * BM;
    n0 = tn * BN;
  };

  // ---- A loader (one 8-k chunk of one row per thread), two k-tiles ahead
  // of the MFMAs; load_a() issues the loader's k-tile and advances it one
  // k-tile along the stream (into the next tile after a tile's last).  Past
  // the stream's end the loaders run on into one virtual tile v >= ntiles,
  // which the remap sends to another block's tile or past M (A then reads
  // row M - 1; B's column tile is always a real one): every address stays
  // valid, nothing reads what they stage, and every iteration issues the same
  // loads, as the counted waits assume ----
  // rows past M load row M - 1 (only their own, unstored, output rows see it)
  const float* a_ptr = g.A;
  int a_kt = 0, a_tl = 0;
  auto a_tile = [&](int tl) {
    int m0, n0;
    tile_origin(tl, m0, n0);
    const int t = s3_opaque(tid);
    const int m = min(m0 + t / SL, g.M - 1);
    a_ptr = g.A + (long long)m * g.lda + (t % SL) * 8;
  };
  // SEG2: from k-tile K1 / BK on, the row's pointer moves to its sampled
  // pixel of A2 (minus K1, so a_ptr + a_kt * BK stays the element address)
  auto a_seg2 = [&](int tl) {
    int m0, n0;
    tile_origin(tl, m0, n0);
    const int t = s3_opaque(tid);
    const int m = min(m0 + t / SL, g.M - 1);
    const int ohw = g.OH * g.OW;
    const int b = m / ohw, r = m - b * ohw, oh = r / g.OW, ow = r - oh * g.OW;
    const long long pix = ((long long)b * g.H2 + (long long)oh * g.s2) * g.W2 + (long long)ow * g.s2;
    a_ptr = g.A2 + pix * g.lda2 + (t % SL) * 8 - g.K1;
  };
  a_tile(0);
  f32x4 ra2[2][2];
  auto load_a = [&](int rb) {
    s3_load2<1>(reinterpret_cast<const f32x4*>(a_ptr + a_kt * BK), ra2[rb]);
    if (++a_kt == nk) {
      a_kt = 0;
      a_tile(++a_tl);
    } else if (SEG2 && a_kt * BK == g.K1) {
      a_seg2(a_tl);
    }
  };
  u32x4 pk[NP];
  auto split_a = [&](int rb) { split2h8(ra2[rb], a_sc, pk[0], pk[1]); };
  auto write_a = [&](int buf) {
    uint16_t* la = lds + buf * STG;
    const int a_slot = tid % SL, a_row = tid / SL;
    const int off = a_row * BK + pswz<BK>(a_row, a_slot) * 8;
#pragma unroll
    for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x4*>(la + p * BM * BK + off) = pk[p];
  };
  auto launder_a = [&](int rb) {
    s3_launder(ra2[rb][0]);
    s3_launder(ra2[rb][1]);
  };

  // ---- B loader: instruction i of a wave DMAs plane i/2, plane rows
  // 128 (i&1) + 16 wave + lane/4 (N % 256 == 0: no row past N) ----
  const uint16_t* Bp = reinterpret_cast<const uint16_t*>(g.B);
  const int b_r = wave * (64 / SL) + lane / SL;
  const int b_sw = pswz<BK>(b_r, lane % SL) * 8;  // the same for every i
  const uint16_t* b_src = Bp;
  int b_kt = 0, b_tl = 0;
  auto b_tile = [&](int tl) {
    int m0, n0;
    tile_origin(tl, m0, n0);
    b_src = Bp + (long long)(n0 + b_r) * g.ldb + b_sw;
  };
  b_tile(0);
  auto glds_b = [&](int buf) {
    uint16_t* lb = lds + buf * STG + A_EL;
#pragma unroll
    for (int i = 0; i < B_INS; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(b_src + (i >> 1) * g.b_plane + (long long)(i & 1) * (BN / 2) * g.ldb +
                                                     b_kt * BK),
                                       (__attribute__((address_space(3))) void*)(lb + (i * NW + wave) * (64 / SL) * BK),
                                       16, 0, 0);
    if (++b_kt == nk) {
      b_kt = 0;
      b_tile(++b_tl);
    }
  };

  // ---- MFMAs: four 16x16x32 sub-tiles per 32x32 tile, as config 4 ----
  f32x4 hi4[FM][FN][4], lo4[FM][FN][4];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          hi4[i][j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
          lo4[i][j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
  };
  zero_acc();
  frag_t fa[NP][FM][2], fb[NP][FN][2];
  const int l16 = lane & 15, lg = lane >> 4;
  auto rd_mf = [&](int cur, int p) {
    const uint16_t* la = lds + cur * STG;
    const uint16_t* lb = la + A_EL;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = wm * WTM + i * 32 + h * 16 + l16;
        fa[p][i][h] = *reinterpret_cast<const frag_t*>(la + (p * BM + row) * BK + pswz<BK>(row, lg) * 8);
      }
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = wn * WTN + j * 32 + h * 16 + l16;
        fb[p][j][h] = *reinterpret_cast<const frag_t*>(lb + (p * BN + row) * BK + pswz<BK>(row, lg) * 8);
      }
  };
#define RR_MF16(a, b, c) c = s3_mf16(a, b, c)
  auto mf_hi = [&]() {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) RR_MF16(fa[0][i][t >> 1], fb[0][j][t & 1], hi4[i][j][t]);
  };
  auto mf_lo1 = [&]() {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          RR_MF16(fa[0][i][t >> 1], fb[1][j][t & 1], lo4[i][j][t]);
          RR_MF16(fa[1][i][t >> 1], fb[0][j][t & 1], lo4[i][j][t]);
        }
  };
#undef RR_MF16

  // ---- epilogue of local tile tl through stage buffer `buf` (free) ----
  // Two slabs by MFMA row tile i: slab s = rows 64 wm + 32 s + [0, 32) of every
  // wave, so staging slab 0 frees half of every wave's accumulators before
  // slab 1's residual is loaded (both slabs' residuals in registers at once
  // beside all accumulators spilled the k-loop).  Residual rows are loaded by
  // inline asm (rows past M clamped to M - 1; never stored), so one explicit
  // vmcnt(0) covers both slabs: slab 1's loads fly while slab 0 is staged.
  constexpr int C4 = BN / 4, HITERS = 32 * C4 / NT;  // 4 row chunks per thread and 32-row band
  auto epilogue = [&](int tl, int buf) {
    // the two accumulator tiles summed first (128 registers -> 64)
    f32x16 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][4 * t + e] = hi4[i][j][t][e] + lo4[i][j][t][e];
    int m0, n0;
    tile_origin(tl, m0, n0);
    const int te = s3_opaque(tid);
    const int c40 = te % C4, r0 = te / C4;
    f32x4 bias_v[1] = {f32x4{0.f, 0.f, 0.f, 0.f}}, sc_v[1];
    // the bias / column scales load after slab 0's residual rows go out and
    // are waited for (redefined by an empty asm) only after slab 0 is staged:
    // waited for up front, as before, they cost a full memory round trip (a
    // vmcnt(0), the next tile's prefetch included) ahead of the residual loads
    auto load_bias = [&]() {
      if ((EPI & EP_BIAS) && g.bias != nullptr) bias_v[0] = *reinterpret_cast<const f32x4*>(g.bias + n0 + c40 * 4);
      if constexpr ((EPI & EP_SCALE) != 0) sc_v[0] = *reinterpret_cast<const f32x4*>(g.col_scale + n0 + c40 * 4);
    };
    auto launder_bias = [&]() {
      asm volatile("" : "+v"(bias_v[0]));
      if constexpr ((EPI & EP_SCALE) != 0) {
        asm volatile("" : "+v"(sc_v[0]));
        sc_v[0] *= a_isc;
      }
    };
    f32x4 res[2][2][HITERS];  // [slab][band][row chunk]
    auto load_res = [&](int sl) {
      if constexpr ((EPI & EP_RES) != 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int it = 0; it < HITERS; ++it) {
            const int m = min(m0 + q * 64 + sl * 32 + r0 + it * (NT / C4), g.M - 1);
            const float* p = g.residual + (long long)m * g.ldc + n0 + c40 * 4;
            if constexpr ((EPI & EP_SC1) != 0)  // streamed (EP_SC1): nt
              asm volatile("global_load_dwordx4 %0, %1, off nt" : "=&v"(res[sl][q][it]) : "v"(p) : "memory");
            else
              asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(res[sl][q][it]) : "v"(p) : "memory");
          }
      }
    };
    float* ct = reinterpret_cast<float*>(lds + buf * STG);  // [2 bands x 32 rows][CS]
    const int le = te & 63;
    auto stage = [&](int sl) {
      float* cw = ct + (wm * 32) * CS + wn * WTN;
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) cw[acc_row<true>(0, r, le) * CS + acc_col<true>(j, r, le)] = acc[sl][j][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    };
    auto store = [&](int sl) {
      if constexpr ((EPI & EP_RES) != 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int it = 0; it < HITERS; ++it) asm volatile("" : "+v"(res[sl][q][it]));
      }
#pragma unroll
      for (int q = 0; q < 2; ++q)
        store_slab<EPI, 2, HITERS, NT, C4, CS, 1>(g, g.C, ct + q * 32 * CS, bias_v, res[sl][q], te,
                                                  m0 + q * 64 + sl * 32, n0, sc_v, am);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every LDS read of the slab done
      asm volatile("" ::: "memory");
    };
    load_res(0);
    load_bias();
    stage(0);
    load_res(1);
    // every load issued so far has landed, the next tile's A(j+1) included:
    // the next iteration's skipped A wait (wait_a) relies on this explicit
    // wait, not on the one hipcc places for the plain bias / scale loads
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    launder_bias();
    store(0);
    stage(1);
    store(1);  // its barrier also frees `buf` for the next k-tiles
    zero_acc();  // here, not at the sum: 128 registers of zeros held through the stores spilled
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
  RR_PH_DECL
  // iteration j (stage cur = j & 1 holds k-tile j, register buffer cur ^ 1
  // holds A(j+1)): B DMA of j+1, A loads of j+2, the k-tile's MFMAs with the
  // split of A(j+1) among them (the dense-A order of config 4), then — after
  // the last k-tile of a tile — its epilogue through stage cur.  The
  // epilogue's stores are issued after A(j+2) and before the next loads: the
  // next A wait (vmcnt(A_LD + B_INS)) counts only loads after it, so it is
  // exact if the stores retire in order and waits longer (never shorter) if
  // they do not.
  auto iter = [&](int cur) __attribute__((always_inline)) {
    glds_b(cur ^ 1);
    load_a(cur);
    RR_PH(0);
    rd_mf(cur, 0);
    rd_mf(cur, 1);
    // (a tile's first k-tile skips the A wait: its A(j+1) was issued before
    // the previous epilogue, whose waits -- the residual's vmcnt(0), or the
    // bias / scale loads' -- covered it; waiting here would wait for that
    // epilogue's stores as well)
    const bool wait_a = c_kt != 0 || c_tl == 0;
    // the plane-1 products, then a0b0 with the split of A(j+1) two VALU per
    // MFMA gap (same per-accumulator order as config 4)
    mf_lo1();
    RR_PH(1);
    if (wait_a) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD + B_INS) : "memory");  // A(j+1) landed
    launder_a(cur ^ 1);
    RR_PH(2);
    split_a(cur ^ 1);
    mf_hi();
#pragma unroll
    for (int x = 0; x < FM * FN * 4; ++x) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // 2 VALU
    }
    write_a(cur ^ 1);
    RR_PH(3);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD) : "memory");  // B DMA of j+1 landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    RR_PH(4);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    RR_PH(5);
    if (++c_kt == nk) {
      c_kt = 0;
      epilogue(c_tl++, cur);
      RR_PH(6);
    }
  };
  RR_PH(7);
  for (int j = 0; j < J; j += 2) {
    iter(0);
    if (j + 1 < J) iter(1);
  }
  // the clamped tail loads are still in flight: keep both buffers live until
  // they have landed, so no later value is allocated to them
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  launder_a(0);
  launder_a(1);
  if constexpr ((EPI & EP_AMAX) != 0) {
    if (g.c_amax != nullptr) amax_publish(g.c_amax, am, bid * NW + wave);
  }
  RR_PH_FLUSH();
}

template <int EPI, int SEG2 = 0>
static hipError_t launch_s3p_t(GemmArgs g, hipStream_t s, int n_cu, int stagger) {
  const long long tiles_m = (g.M + 127) / 128, tiles_n = g.N / 256;
  const long long ntiles = tiles_m * tiles_n;
  if (ntiles <= 0) return hipSuccess;
  if (ntiles * (g.K / 32) > 0x7fffffffLL) return hipErrorInvalidValue;
  // one block per CU; a block that owns several tiles must stay on its XCD
  // (grid a multiple of 8)
  const int slots = std::max(8, n_cu & ~7);
  const int grid = ntiles <= slots ? (int)ntiles : slots;
  g.stagger_blocks = grid;
  g.stagger_sleeps = ntiles > 2LL * grid ? stagger : 0;
  hipLaunchKernelGGL((gemm_s3p_kernel<EPI, SEG2>), dim3((unsigned)grid), dim3(512), 0, s, g, (int)tiles_n,
                     (int)ntiles);
  return hipGetLastError();
}

// config 8: dense A, N % 256 == 0 (s3_persist_ok, h2_route.hpp)
hipError_t launch_s3p(const GemmArgs& g, hipStream_t s, int n_cu, int st) {
  // residual epilogues streamed (EP_SC1, as config 15's): 128->512 + residual
  // x3 0.908 -> 0.877 ms, 64->256 x2 1.701 -> 1.707; the embed 69.09 -> 69.06
  // ms (profiles/r05k_sweep.txt, r05k_e2e.txt)
  return h2_ep_dispatch<true>(g, [&](auto ep) { return launch_s3p_t<decltype(ep)::value>(g, s, n_cu, st); });
}

int launch_gemm_h2_seg2(rr_handle_s* h, const GemmArgs& g, hipStream_t s, int timer_cls) {
  if (g.M < 0 || g.N <= 0 || g.K <= 0 || g.K1 <= 0 || g.K1 >= g.K || (g.K % 32) || (g.K1 % 32) || (g.N % 256))
    return set_error(h, RR_EINVAL, "gemm_h2_seg2: K1, K - K1 multiples of 32 and N % 256 == 0");
  if ((g.lda & 3) || (g.lda2 & 3) || ((uintptr_t)g.A & 15) || ((uintptr_t)g.A2 & 15) || g.OH <= 0 || g.OW <= 0 ||
      g.s2 <= 0 || (long long)(g.OH - 1) * g.s2 >= g.H2 || (long long)(g.OW - 1) * g.s2 >= g.W2)
    return set_error(h, RR_EINVAL, "gemm_h2_seg2: bad A / A2 layout");
  if (g.col_scale == nullptr || g.a_amax == nullptr || g.a2_amax == nullptr || g.residual != nullptr ||
      g.relu != 1 || g.out_bf16 || (g.ldb & 7) || (g.b_plane & 7) || ((uintptr_t)g.B & 15) ||
      ((uintptr_t)g.col_scale & 15))
    return set_error(h, RR_EINVAL, "gemm_h2_seg2: ReLU epilogue, scales and both max-|x| records");
  if (g.M == 0) return RR_OK;
  hipError_t e;
  {
    TimedLaunch tl(h, timer_cls, s);
    e = launch_s3p_t<H2_EP | EP_RELU, 1>(g, s, device_cu_count(h), h->tune.s3_stagger >= 0 ? h->tune.s3_stagger : 0);
  }
  return check_hip(h, e, "gemm_h2_seg2 launch");
}

#if RR_S3_PHASES
int h2_stream_phases(unsigned long long* out) { return s3_phases_take(out); }
#endif

}  // namespace rr
