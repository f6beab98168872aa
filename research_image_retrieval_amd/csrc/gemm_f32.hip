// gemm_f32.hip — fp32 MFMA GEMM core for gfx950 (CDNA4).
//
// C[M,N] = A[M,K] . B[N,K]^T with A and B both K-contiguous ("NT" layout).
// One core serves three reference call sites:
//   * cosine ranker  : A = gallery rows, B = query rows  (iris_evaluate.py:383)
//   * conv layers    : A = implicit im2col of an NHWC map, B = weights
//                      [Cout][KH][KW][Cin]               (networks/backbone.py:103-109)
//   * projections    : A = pooled descriptors, B = W     (networks/RetrievalNet.py:342,
//                                                         models/gem_pooling.py:68)
//
// Arithmetic: v_mfma_f32_32x32x2_f32 (exact f32 in, f32 accumulate; every
// output element is a k-ordered fmaf chain).  Within each 16-deep k chunk the
// lane half h of MFMA e supplies k = 16c + 8h + e, so the chain visits
// k = 16c+0, 16c+8, 16c+1, 16c+9, ..., 16c+7, 16c+15 — oracle/cosine_topk.c
// restates exactly this order, which makes GPU scores bit-identical to the
// oracle's.
//
// Tiling: a wave owns a 64x64 output block (2x2 MFMA tiles of 32x32, 64
// accumulator registers); a workgroup is WM x WN waves.  BK = 32: each k-tile
// of A and B is register-staged (one float4 per lane-chunk, coalesced along
// K) into a double-buffered LDS image of 128-byte rows whose 16-byte slots are
// XOR-swizzled by (row>>1)&7, which makes the fragment ds_read_b128 (lane
// groups of 16 distinct rows, same slot) bank-conflict free.  One barrier per
// k-tile; the next tile's global loads are in flight under the MFMAs.
// Block ids are remapped so consecutive tiles of one XCD share the A panel
// (the streamed gallery / activation rows) in that XCD's L2.
//
// launch_gemm is the one entry point of the GEMM cores: it launches the
// instance gemm_route (gemm_route.hpp) names, here or in gemm_lp.hip,
// gemm_lpp.hip, gemm_8p.hip and sweep16.hip.
#include "gemm_route.hpp"
#include "gemm_tile.hpp"

namespace rr {

template <int WM, int WN, int FM, int FN, int AMODE, int EMODE, int BK, int MINB>
__global__ __launch_bounds__(64 * WM * WN, MINB) void gemm_f32_kernel(GemmArgs g, int tiles_n) {
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
  __shared__ __attribute__((aligned(16))) float lds[2 * BUF];

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
  const int nk = (K + BK - 1) / BK;

  // ---- per-chunk A row state ----
  const float* a_ptr[A_CH];
  int a_ih0[A_CH], a_iw0[A_CH];
  bool a_ok[A_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    const int m = m0 + crow + i * ROWS_PER_PASS;
    a_ok[i] = m < g.M;
    if constexpr (AMODE == A_DENSE) {
      a_ptr[i] = g.A + (long long)(a_ok[i] ? m : 0) * g.lda + koff;
      a_ih0[i] = 0;
      a_iw0[i] = 0;
    } else {
      const int mm = a_ok[i] ? m : 0;
      const int ohw = g.OH * g.OW;
      const int b = mm / ohw;
      const int rem = mm - b * ohw;
      const int oh = rem / g.OW;
      const int ow = rem - oh * g.OW;
      a_ptr[i] = g.A + (long long)b * g.H * g.W * g.Cin;
      a_ih0[i] = oh * g.stride - g.pad;
      a_iw0[i] = ow * g.stride - g.pad;
    }
  }
  const float* b_ptr[B_CH];
  bool b_ok[B_CH];
#pragma unroll
  for (int i = 0; i < B_CH; ++i) {
    const int n = n0 + crow + i * ROWS_PER_PASS;
    b_ok[i] = n < g.N;
    b_ptr[i] = g.B + (long long)(b_ok[i] ? n : 0) * g.ldb + koff;
  }

  f32x4 ra[A_CH], rb[B_CH];

  auto load_tile = [&](int kt) {
    const int k = kt * BK + slot * 4;
    const bool kok = k < K;
    if constexpr (AMODE == A_DENSE) {
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        ra[i] = (a_ok[i] && kok) ? *reinterpret_cast<const f32x4*>(a_ptr[i] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else if constexpr (AMODE == A_CONV) {
      // Cin % 32 == 0: the whole 32-deep k-tile lies in one (kh, kw) tap.
      const int k0 = kt * BK;
      const int khw = k0 / g.Cin;
      const int cin0 = k0 - khw * g.Cin;
      const int kh = khw / g.KW;
      const int kw = khw - kh * g.KW;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
        const bool ok = a_ok[i] && kok && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
        ra[i] = ok ? *reinterpret_cast<const f32x4*>(a_ptr[i] + ((long long)ih * g.W + iw) * g.Cin + cin0 + slot * 4)
                   : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else if constexpr (AMODE == A_CONV_C4) {
      // Cin == 4 (RGB + zero pad channel): each float4 is one filter tap
      const int tap = k >> 2;
      const int kh = tap / g.KW;
      const int kw = tap - kh * g.KW;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
        const bool ok = a_ok[i] && kok && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
        ra[i] = ok ? *reinterpret_cast<const f32x4*>(a_ptr[i] + ((long long)ih * g.W + iw) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
      // generic gather (small / odd Cin)
      const int kwc = g.KW * g.Cin;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kk = k + e;
          if (a_ok[i] && kk < K) {
            const int kh = kk / kwc;
            const int r2 = kk - kh * kwc;
            const int kw = r2 / g.Cin;
            const int c = r2 - kw * g.Cin;
            const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
            if ((unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
              v[e] = a_ptr[i][((long long)ih * g.W + iw) * g.Cin + c];
          }
        }
        ra[i] = v;
      }
    }
    if constexpr (AMODE == A_CONV_GENERIC) {
      // K need not be a multiple of 4 here (stem: 7*7*3 = 147): scalar loads
#pragma unroll
      for (int i = 0; i < B_CH; ++i) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (b_ok[i] && k + e < K) v[e] = b_ptr[i][k + e];
        rb[i] = v;
      }
    } else {
#pragma unroll
      for (int i = 0; i < B_CH; ++i) {
        rb[i] = (b_ok[i] && kok) ? *reinterpret_cast<const f32x4*>(b_ptr[i] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };

  auto store_tile = [&](int buf) {
    float* la = lds + buf * BUF;
    float* lb = la + BM * BK;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int row = crow + i * ROWS_PER_PASS;
      *reinterpret_cast<f32x4*>(la + row * BK + swz<BK>(row, slot) * 4) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int row = crow + i * ROWS_PER_PASS;
      *reinterpret_cast<f32x4*>(lb + row * BK + swz<BK>(row, slot) * 4) = rb[i];
    }
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int lr = lane & 31, lh = lane >> 5;

  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    const float* la = lds + cur * BUF;
    const float* lb = la + BM * BK;
#pragma unroll
    for (int c2 = 0; c2 < BK / 16; ++c2) {
      f32x4 af[FM][2], bf[FN][2];
      const int s0 = c2 * 4 + 2 * lh;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int row = wm * WTM + i * 32 + lr;
        af[i][0] = *reinterpret_cast<const f32x4*>(la + row * BK + swz<BK>(row, s0) * 4);
        af[i][1] = *reinterpret_cast<const f32x4*>(la + row * BK + swz<BK>(row, s0 + 1) * 4);
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int row = wn * WTN + j * 32 + lr;
        bf[j][0] = *reinterpret_cast<const f32x4*>(lb + row * BK + swz<BK>(row, s0) * 4);
        bf[j][1] = *reinterpret_cast<const f32x4*>(lb + row * BK + swz<BK>(row, s0 + 1) * 4);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e >> 2][e & 3], bf[j][e >> 2][e & 3], acc[i][j], 0, 0, 0);
      }
    }
    if (kt + 1 < nk) store_tile(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue ----
  // 32x32 C/D map: col (N index) = lane & 31, row (M index) = (r&3) + 8(r>>2) + 4(lane>>5)
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

  // E_STORE: through LDS (gemm_epilogue.hpp), the flags read at run time
  if constexpr (EMODE == E_STORE) epilogue_store<WM, WN, FM, FN, 2 * BUF, false, -1>(g, Cb, acc, lds, m0, n0, 1.f, nullptr);
}

// the instance of RR_GEMM_F32_INSTANCES that the route names, for one (A mode, epilogue)
template <int AM, int EM>
static hipError_t launch_f32(const GemmRoute& r, const GemmArgs& g, hipStream_t s) {
#define RR_X(CFG, WM, WN, FM, FN, BK, MINB, WHEN)                                                               \
  if constexpr (WHEN) {                                                                                         \
    if (r.cfg == CFG && r.wm == WM && r.wn == WN && r.fm == FM && r.fn == FN && r.bk == BK && r.minb == MINB)   \
      return launch_tiles<32 * FM * WM, 32 * FN * WN, 64 * WM * WN>(gemm_f32_kernel<WM, WN, FM, FN, AM, EM, BK, MINB>, g, s); \
  }
  RR_GEMM_F32_INSTANCES(RR_X)
#undef RR_X
  return hipErrorInvalidValue;
}

static hipError_t launch_gemm_f32(const GemmRoute& r, int amode, int emode, const GemmArgs& g, hipStream_t s) {
  if (amode == A_DENSE && emode == E_STORE) return launch_f32<A_DENSE, E_STORE>(r, g, s);
  if (amode == A_DENSE && emode == E_SCORES_T) return launch_f32<A_DENSE, E_SCORES_T>(r, g, s);
  if (amode == A_DENSE && emode == E_FILTER) return launch_f32<A_DENSE, E_FILTER>(r, g, s);
  if (amode == A_CONV && emode == E_STORE) return launch_f32<A_CONV, E_STORE>(r, g, s);
  if (amode == A_CONV_GENERIC && emode == E_STORE) return launch_f32<A_CONV_GENERIC, E_STORE>(r, g, s);
  if (amode == A_CONV_C4 && emode == E_STORE) return launch_f32<A_CONV_C4, E_STORE>(r, g, s);
  return hipErrorInvalidValue;
}

// The one door of the GEMM cores: validate, route (gemm_route.hpp), launch what the route names.
int launch_gemm(rr_handle_s* h, int amode, int emode, const GemmArgs& g, hipStream_t s, int timer_cls, int dt) {
  if (const char* err = gemm_shape_error(amode, emode, dt, g)) return set_error(h, RR_EINVAL, err);
  if (g.M == 0 || g.N == 0) return RR_OK;
  const GemmRoute r = gemm_route(amode, emode, dt, g, gemm_tune(h->tune));
  hipError_t e = hipErrorInvalidValue;  // GF_NONE
  {
    TimedLaunch tl(h, timer_cls, s);
    switch (r.family) {
      case GF_F32: e = launch_gemm_f32(r, amode, emode, g, s); break;
      case GF_LP: e = launch_gemm_lp(r, emode, dt, g, s); break;
      case GF_LPP:
      case GF_LPP3: e = launch_gemm_lpp(r, g, s, device_cu_count(h)); break;
      case GF_8P: e = launch_gemm_8p(r, emode, dt, g, s); break;
      case GF_SWEEP128:
      case GF_SWEEP64: e = launch_sweep16(r, g, s); break;
      default: break;
    }
  }
  return check_hip(h, e, "gemm launch");
}

}  // namespace rr
