// h2_stem.hip — the stem (7x7 / 2, pad 3, NHWC4) + ReLU + 3x3 / 2 max-pool
// as a halo tile of the f16x2 split GEMM core (h2_tile.hip: the split).
//
// The implicit-GEMM stem (h2_tile.hip, POOL) reads each input pixel's 16 B once per filter tap
// that covers it (~12x at stride 2) plus the 64 x 224 weight planes for every
// 256-row tile (more bytes than the tile's whole input patch).  Here one
// persistent block per CU keeps both weight planes resident in LDS (loaded
// once) and, per tile, stages the tile's input patch once: the tile is the
// same 17 x 15 patch of conv outputs (8 x 7 pooled outputs plus their window
// halo) as the fused config-7 stem, so its input is a 39 x 35-pixel patch,
// fetched once (one 16-B load per pixel, zero outside the image) and split
// into two fp16 planes of 4 channels (8 B per pixel).  The k-loop then reads
// only LDS and has no barrier: k-step s = taps 4s .. 4s + 3 (16 k), lane half
// h supplies taps 4s + 2h, 4s + 2h + 1 (one ds_read_b64 each per plane), taps
// past 49 read a zero pixel (their weight columns are zero as well).  Same
// per-accumulator products and order as the fused config-7 stem (a0b0 into
// one set; a0b1, a1b0 into the other; 32x32x16 f16) over taps 0..51 instead of
// 0..55 (the four dropped k-steps add exact zeros).  The next tile's patch is
// loaded into registers under the k-loop; the pool epilogue stages the raw
// accumulators through LDS exactly as the config-7 stem does.
// Round 6 (PMC on this launch alone, profiles/r06y_halo_stem_pmc.txt: MFMA
// busy 0.36, 3.3 LDS bank-conflict cycles per MFMA, four barriers per tile):
//  - the C staging has its own LDS region (B 58 KB + patch 22 KB + C 68 KB),
//    so tile i's pool epilogue (its LDS reads, the max / scale / bias / ReLU
//    and the stores) runs inside tile i + 1's k-loop, between its k-steps,
//    instead of after it with the matrix cores idle; two barriers per tile;
//  - patch row hr keeps its even columns in slots 0..17 and its odd ones in
//    18..34 (row stride 36 slots): a lane row reads every other pixel of a
//    patch row, so consecutive lanes now read consecutive 8-B slots, where
//    the raster layout put them 16 B apart (two lanes per bank pair).
// Same products, order and epilogue arithmetic: bit-identical output.
// NW = 4: four waves of 64 rows x 64 columns instead of eight of 32 x 64
// (every wave reads the whole B operand each k-step: 32 KB of fragments per
// k-step through LDS instead of 48 KB for the same MFMAs).  Bit-identical, and
// measured slower: 2.20 vs 1.68 ms at 1280 images (one wave per SIMD leaves
// nothing to cover the LDS latency; profiles/r06m_stem_4wave_ab.txt), so the
// launch keeps NW = 8.
// BREG: the weights in registers instead of LDS.  8 waves as 4 row groups of
// 64 rows x 2 column groups of 32: a wave's B fragments for all 13 k-steps
// (its 32 columns, both planes: 104 VGPRs) are loaded once per block, so the
// k-loop reads only the patch from LDS, 4 KB of fragments per wave and k-step
// instead of 6 KB for the same six MFMAs.  Same products and order per
// accumulator: bit-identical.  BREG 1 spills (33 VGPRs; 16 even with the
// pool items out of the k-loop).  BREG 2, the launch's form: only the high
// plane in registers (52 VGPRs; it feeds two of the three products), the low
// plane still read from LDS, 5 KB per wave and k-step; 256 VGPRs, no spill.
// 1.759 -> 1.715 ms at 1280 images, bit-identical
// (profiles/r06zd_stem_breg_ab.txt).
#include <algorithm>

#include "h2_common.hpp"

namespace rr {

template <int EPI, int NW = 8, int BREG = 0>
__global__ __launch_bounds__(64 * NW, 1) void stem_pool_halo_kernel(GemmArgs g, int ntiles) {
  constexpr int NT = 64 * NW, BN = 64, HR = 39, HC = 35, HP = HR * HC;  // 1365 patch pixels
  constexpr int WR = BREG ? 64 : 256 / NW, FM = WR / 32;  // rows per wave, 32-row MFMA tiles per wave
  constexpr int JN = BREG ? 1 : 2;                        // 32-column MFMA tiles per wave
  static_assert(NW == 8 || (NW == 4 && !BREG), "8 waves of 32 rows or 4 of 64");
  constexpr int HS = 36, HPS = HR * HS;       // patch slots per row / in all (even | odd columns), zero slot HPS
  constexpr int KP = 224, BS = KP + 8;        // weight row (k) length; LDS row stride (u16, padded)
  constexpr int NKS = 13;                     // k-steps of 4 taps (taps 0..51)
  constexpr int B_U16 = BREG == 1 ? 0 : 2 * BN * BS;  // both weight planes
  constexpr int A_U16 = 2 * (HPS + 1) * 4;    // both patch planes + the zero slot
  constexpr int CS = BN + 4;                  // C staging row stride (floats)
  constexpr int C_U16 = 256 * CS * 2;
  constexpr int A_PASS = (HP + NT - 1) / NT;  // 3
  constexpr int C4 = BN / 4, NPOOL = 56 * C4;  // pool work items per tile (896)
  constexpr int QI = (NPOOL + NT - 1) / NT;     // pool items per thread (2 / 4), the last one partial
  constexpr int PS = NKS / QI;                  // k-steps between them
  __shared__ __attribute__((aligned(16))) uint16_t lds[B_U16 + A_U16 + C_U16];
  uint16_t* lb = lds;
  uint16_t* la = lds + B_U16;
  float* ct = reinterpret_cast<float*>(lds + B_U16 + A_U16);
  typedef f16x8 frag_t;
  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int wrg = BREG ? wave % 4 : wave, wn = BREG ? wave / 4 : 0;  // the wave's row / column group
  const uint32_t a_amax_w = amax_load_slot(g.a_amax);
  float a_sc, a_isc;
  {
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

  // ---- both weight planes into LDS, once: [plane][n][k], rows padded
  // (BREG: the wave's own fragments into registers) ----
  constexpr int BRP = BREG == 1 ? 2 : 1;  // weight planes in registers
  frag_t breg[BREG ? NKS : 1][BRP];
  if constexpr (BREG != 0) {
    const uint16_t* Bp = reinterpret_cast<const uint16_t*>(g.B) + (long long)(32 * wn + lr) * g.ldb + 8 * lh;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int p = 0; p < BRP; ++p) breg[ks][p] = *reinterpret_cast<const frag_t*>(Bp + p * g.b_plane + 16 * ks);
  }
  if constexpr (BREG != 1) {
    const uint16_t* Bp = reinterpret_cast<const uint16_t*>(g.B);
    for (int i = tid; i < 2 * BN * (KP / 8); i += NT) {
      const int row = i / (KP / 8), c8 = i - row * (KP / 8);  // row = plane * 64 + n
      const int p = row / BN, n = row - p * BN;
      *reinterpret_cast<u32x4*>(lb + row * BS + c8 * 8) =
          *reinterpret_cast<const u32x4*>(Bp + p * g.b_plane + (long long)n * g.ldb + c8 * 8);
    }
  }

  const int tpi = g.pool_tr * g.pool_tc;
  // the patch of tile tl: pixel p -> input (32 pr - 5 + p / 35, 28 pc - 5 + p % 35)
  f32x4 px[A_PASS];
  auto load_patch = [&](int tl) {
    const int b = tl / tpi, t2 = tl - b * tpi, pr = t2 / g.pool_tc, pc = t2 - pr * g.pool_tc;
#pragma unroll
    for (int q = 0; q < A_PASS; ++q) {
      const int p = tid + q * NT, hr = p / HC, hc = p - hr * HC;
      const int ih = 32 * pr - 5 + hr, iw = 28 * pc - 5 + hc;
      const bool ok = tl < ntiles && p < HP && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
      const f32x4* src = ok ? reinterpret_cast<const f32x4*>(g.A + (((long long)b * g.H + ih) * g.W + iw) * 4)
                            : s3_zero_page();
      asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(px[q]) : "v"(src) : "memory");
    }
  };
  auto store_patch = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int q = 0; q < A_PASS; ++q) {
      asm volatile("" : "+v"(px[q]));
      const int p = tid + q * NT, hr = p / HC, hc = p - hr * HC;
      const int slot = hr * HS + (hc & 1) * (HS / 2) + (hc >> 1);
      const f32x4 v = px[q] * a_sc;
      const f16x4 hi = __builtin_convertvector(v, f16x4);
      const f16x4 lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x4), f16x4);
      if (p < HP) {
        *reinterpret_cast<f16x4*>(la + slot * 4) = hi;
        *reinterpret_cast<f16x4*>(la + (HPS + 1) * 4 + slot * 4) = lo;
      }
    }
    if (tid < 2) *reinterpret_cast<uint2*>(la + tid * (HPS + 1) * 4 + HPS * 4) = uint2{0u, 0u};  // the zero slot
  };

  // lane rows: wave w owns tile rows WR w .. +WR-1 (MFMA row tile i: WR w + 32 i
  // + lane & 31); row r -> conv output (q, c) = (r / 15, r % 15) of the patch,
  // input pixel of tap (kh, kw) = (2q + kh, 2c + kw), slot (2q + kh) 36 +
  // (kw & 1) 18 + c + (kw >> 1)
  int sbase[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int row = wrg * WR + 32 * i + lr, rq = row / 15, rc = row - rq * 15;
    sbase[i] = row < 255 ? (2 * rq) * HS + rc : -1;
  }

  // ---- pool work item `it` of tile tl (C staged in ct): the pooled output
  // (8 pr + it / 16 / 7, 7 pc + it / 16 % 7), channels 4 (it % 16) .. +3: max
  // over the window's in-map conv outputs of the raw accumulators, then
  // scale, bias, ReLU (all monotone) ----
  float am = 0.f;
  auto pool_item = [&](int tl, int it) __attribute__((always_inline)) {
    const int b = tl / tpi, t2 = tl - b * tpi, pr = t2 / g.pool_tc, pc = t2 - pr * g.pool_tc;
    const int qd = it / C4, c4 = it - qd * C4, pi = qd / 7, pj = qd - 7 * pi;
    const int ph = 8 * pr + pi, pw = 7 * pc + pj;
    if (ph >= g.POH || pw >= g.POW) return;
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
  };

  const int G = gridDim.x;
  int tl = blockIdx.x;
  int prev = -1;  // the tile whose C is staged in ct (its pool still to run)
  load_patch(tl);
  store_patch();
  __syncthreads();
  for (; tl < ntiles; tl += G) {
    load_patch(tl + G);  // the next tile's patch lands under this tile's k-loop
    f32x16 hi[FM][JN], lo[FM][JN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < JN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) hi[i][j][r] = lo[i][j][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      frag_t a[2][FM], b[2][2];
      const int t0 = 4 * ks + 2 * lh;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        int pix[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int t = t0 + u, kh = t / 7, kw = t - kh * 7;
          pix[u] = (sbase[i] >= 0 && t < 49) ? sbase[i] + kh * HS + (kw & 1) * (HS / 2) + (kw >> 1) : HPS;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const uint16_t* pl = la + p * (HPS + 1) * 4;
          const f16x4 x0 = *reinterpret_cast<const f16x4*>(pl + pix[0] * 4);
          const f16x4 x1 = *reinterpret_cast<const f16x4*>(pl + pix[1] * 4);
          a[p][i] = __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7);
        }
      }
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < JN; ++j)
          b[p][j] = (BREG == 1 || (BREG == 2 && p == 0))
                        ? breg[ks][BREG == 1 ? p : 0]
                        : *reinterpret_cast<const frag_t*>(lb + (p * BN + 32 * (j + wn) + lr) * BS + 16 * ks + 8 * lh);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j) hi[i][j] = s3_mf32(a[0][i], b[0][j], hi[i][j]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j) {
          lo[i][j] = s3_mf32(a[0][i], b[1][j], lo[i][j]);
          lo[i][j] = s3_mf32(a[1][i], b[0][j], lo[i][j]);
        }
      // the previous tile's pool epilogue, one work item at a time, among the MFMAs
      if (prev >= 0) {
#pragma unroll
        for (int q = 0; q < QI; ++q)
          if (ks == q * PS + PS / 2 && tid + q * NT < NPOOL) pool_item(prev, tid + q * NT);
      }
    }
    __syncthreads();  // every wave done with the patch and with ct's previous tile
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < JN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          ct[(wrg * WR + 32 * i + acc_row<false>(0, r, lane)) * CS + 32 * wn + acc_col<false>(j, r, lane)] =
              hi[i][j][r] + lo[i][j][r];
    store_patch();
    prev = tl;
    __syncthreads();
  }
  if (prev >= 0) {  // the last tile's pool
#pragma unroll
    for (int q = 0; q < QI; ++q)
      if (tid + q * NT < NPOOL) pool_item(prev, tid + q * NT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr ((EPI & EP_AMAX) != 0) {
    if (g.c_amax != nullptr) amax_publish(g.c_amax, am, blockIdx.x * NW + wave);
  }
}

int launch_stem_pool_h2(rr_handle_s* h, const GemmArgs& g, hipStream_t s, int timer_cls) {
  if (g.N != 64 || g.Cin != 4 || g.K % 32 || g.K < g.KH * g.KW * 4 || g.relu != 1 || g.residual != nullptr ||
      g.col_scale == nullptr || g.a_amax == nullptr || g.pool_out == nullptr || g.POH <= 0 || g.POW <= 0 ||
      g.pool_tr != (g.POH + 7) / 8 || g.pool_tc != (g.POW + 6) / 7 || ((uintptr_t)g.A & 15) || (g.ldb & 7) ||
      (g.b_plane & 7) || ((uintptr_t)g.B & 15) || ((uintptr_t)g.col_scale & 15) || ((uintptr_t)g.pool_out & 15))
    return set_error(h, RR_EINVAL, "stem_pool_h2: NHWC4 input, 64 output channels, ReLU, aligned operands");
  GemmArgs q = g;
  const long long tiles = (long long)(g.M / ((long long)g.OH * g.OW)) * g.pool_tr * g.pool_tc;
  if (tiles * 256 > 0x7fffffffLL) return set_error(h, RR_EINVAL, "stem_pool_h2: too many tiles");
  if (tiles == 0) return RR_OK;
  q.M = (int)(tiles * 256);  // 256 rows per tile (255 used)
  hipError_t e;
  {
    TimedLaunch tl(h, timer_cls, s);
    // the halo stem (7x7 / 2, pad 3; s3_cfg 7 forces the implicit-GEMM one)
    if (h->tune.s3_cfg != 7 && g.KH == 7 && g.KW == 7 && g.stride == 2 && g.pad == 3 && g.K == 224 && g.ldb == 224) {
      const int grid = (int)std::min<long long>(tiles, device_cu_count(h));
      hipLaunchKernelGGL((stem_pool_halo_kernel<H2_EP | EP_RELU, 8, 2>), dim3((unsigned)grid), dim3(512), 0, s, g, (int)tiles);
      e = hipGetLastError();
    } else {
      e = launch_h2_tile_stem_pool(q, s, device_cu_count(h));
    }
  }
  return check_hip(h, e, "stem_pool_h2 launch");
}

}  // namespace rr
