// tokagg_ops.hip — the token aggregator's kernel (gfx950): the last encoder
// layer's attention for the global token alone, with the K and V projections
// folded into the query and the output weights ("The token
// aggregator").
//
// Reference (models/token_based.py): TokenAggregator.forward :60-86 — the
// nn.TransformerEncoder of :45-52 returns every row, :81 keeps x[0].
#include "heads_common.hpp"

namespace rr {

constexpr int kCapThreads = 512;  // 8 waves per workgroup
constexpr int kCapWaves = kCapThreads / 64;
constexpr int kCapRows = 4;       // rows a wave scores per step
constexpr int kCapMaxHeads = 16;
constexpr int kCapMaxSeq = 256;

// 16-lane row sum by DPP row_shr 1/2/4/8 (out-of-row sources read 0): lane 15
// of each row holds the row's total, added in the same order on every call.
__device__ __forceinline__ float row_sum16(float x) {
  auto shr = [](float v, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), decltype(ctrl)::value, 0xf, 0xf, true));
  };
  x += shr(x, std::integral_constant<int, 0x111>{});
  x += shr(x, std::integral_constant<int, 0x112>{});
  x += shr(x, std::integral_constant<int, 0x114>{});
  x += shr(x, std::integral_constant<int, 0x118>{});
  return x;
}

// Four per-lane values -> their four 64-lane sums in one pass: lanes 32 apart
// fold a0 | a1 and a2 | a3, lanes 16 apart fold the two results, row_sum16 adds
// the 16 columns.  Lane 15 of 16-lane row r then holds the sum of value
// ((r & 1) << 1) | (r >> 1).  A fixed order: the same bits on every call.
__device__ __forceinline__ float wave_sum4(float a0, float a1, float a2, float a3, int lane) {
  const bool hi = lane & 32, q = lane & 16;
  const float b0 = (hi ? a1 : a0) + __shfl_xor(hi ? a0 : a1, 32, 64);
  const float b1 = (hi ? a3 : a2) + __shfl_xor(hi ? a2 : a3, 32, 64);
  const float c = (q ? b1 : b0) + __shfl_xor(q ? b0 : b1, 16, 64);
  return row_sum16(c);
}

// One workgroup per image, all heads: the image's rows leave HBM once (the
// second pass reads them from cache), and a head's sums never depend on the
// batch.  Dynamic LDS, in floats: qt [heads][d], then sc [heads][seq] (scores,
// then p); the slabs of the last step, red [rg][heads][d], reuse it from 0.
//  1. scores: wave w takes rows 4 g .. 4 g + 3 for g = w, w + 8, ...; a lane
//     holds the rows' columns 4 (lane + 64 k) .. + 3 (k < KC) and adds
//     qt_h . x_j over them in column order; wave_sum4 adds the lanes.
//  2. softmax: wave w takes heads w, w + 8; a lane holds rows lane + 64 i; the
//     maximum is subtracted before exp, the sum is wave_sum's.
//  3. out: thread (c4, rg) adds p_hj x_j[4 c4 .. + 3] over rows j = rg, rg + RG,
//     ... (RG = 512 / (d / 4)) for every head; the RG slabs are added in index
//     order through LDS.
// (Eight rows per step in 1 and eight loads in flight in 3 measured the same
// time, 47 us per image at seq = 197, d = 512, at 206 registers for 79: the
// time is not in the global loads.  DESIGN.md has both.)
template <int KC>
__global__ __launch_bounds__(kCapThreads) void cls_attn_pool_kernel(const float* __restrict__ x, int seq, int d,
                                                                    const float* __restrict__ qt, int heads,
                                                                    float* __restrict__ p_out,
                                                                    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float cap_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d4 = d >> 2;
  const long long img = blockIdx.x;
  const float* xi = x + img * seq * d;
  const float* qi = qt + img * heads * d;
  float* qs = cap_lds;
  float* sc = cap_lds + heads * d;

  for (int e = tid; e < heads * d4; e += kCapThreads)
    *reinterpret_cast<f32x4*>(qs + e * 4) = *reinterpret_cast<const f32x4*>(qi + e * 4);
  __syncthreads();

  // 1. scores
  const int groups = (seq + kCapRows - 1) / kCapRows;
  for (int g = wave; g < groups; g += kCapWaves) {
    f32x4 xv[kCapRows][KC];
#pragma unroll
    for (int r = 0; r < kCapRows; ++r)
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const int j = g * kCapRows + r, c4 = lane + 64 * k;
        xv[r][k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j < seq && c4 < d4) xv[r][k] = *reinterpret_cast<const f32x4*>(xi + (long long)j * d + c4 * 4);
      }
    for (int h = 0; h < heads; ++h) {
      float a[kCapRows] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const int c4 = lane + 64 * k;
        f32x4 qv = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c4 < d4) qv = *reinterpret_cast<const f32x4*>(qs + h * d + c4 * 4);
#pragma unroll
        for (int r = 0; r < kCapRows; ++r)
#pragma unroll
          for (int e = 0; e < 4; ++e) a[r] = fmaf(qv[e], xv[r][k][e], a[r]);
      }
      const float t = wave_sum4(a[0], a[1], a[2], a[3], lane);
      const int row = lane >> 4;
      const int j = g * kCapRows + (((row & 1) << 1) | (row >> 1));
      if ((lane & 15) == 15 && j < seq) sc[h * seq + j] = t;
    }
  }
  __syncthreads();

  // 2. softmax over the rows, per head
  for (int h = wave; h < heads; h += kCapWaves) {
    float s[kCapMaxSeq / 64];
    float m = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < kCapMaxSeq / 64; ++i) {
      const int j = lane + 64 * i;
      s[i] = j < seq ? sc[h * seq + j] : -__builtin_inff();
      m = fmaxf(m, s[i]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
#pragma unroll
    for (int i = 0; i < kCapMaxSeq / 64; ++i) s[i] = lane + 64 * i < seq ? expf(s[i] - m) : 0.f;
    const float l = wave_sum((s[0] + s[1]) + (s[2] + s[3]));
#pragma unroll
    for (int i = 0; i < kCapMaxSeq / 64; ++i) {
      const int j = lane + 64 * i;
      if (j < seq) {
        const float pj = s[i] / l;
        sc[h * seq + j] = pj;
        if (p_out != nullptr) p_out[(img * heads + h) * seq + j] = pj;
      }
    }
  }
  __syncthreads();

  // 3. out = p . x
  const int rgs = kCapThreads / d4;  // 2 .. 32 row groups
  const int c4 = tid % d4, rg = tid / d4;
  f32x4 acc[kCapMaxHeads];
#pragma unroll
  for (int h = 0; h < kCapMaxHeads; ++h) acc[h] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (rg < rgs) {
#pragma unroll 2
    for (int j = rg; j < seq; j += rgs) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xi + (long long)j * d + c4 * 4);
#pragma unroll
      for (int h = 0; h < kCapMaxHeads; ++h)
        if (h < heads) {
          const float pj = sc[h * seq + j];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[h][e] = fmaf(pj, xv[e], acc[h][e]);
        }
    }
  }
  __syncthreads();  // every read of sc is done: the slabs take its place
  float* red = cap_lds;
  if (rg < rgs) {
#pragma unroll
    for (int h = 0; h < kCapMaxHeads; ++h)
      if (h < heads) *reinterpret_cast<f32x4*>(red + ((long long)(rg * heads + h) * d4 + c4) * 4) = acc[h];
  }
  __syncthreads();
  float* oi = out + img * heads * d;
  for (int e = tid; e < heads * d4; e += kCapThreads) {
    f32x4 t = *reinterpret_cast<const f32x4*>(red + e * 4);
    for (int s = 1; s < rgs; ++s) t += *reinterpret_cast<const f32x4*>(red + ((long long)s * heads * d4 + e) * 4);
    *reinterpret_cast<f32x4*>(oi + e * 4) = t;
  }
}

}  // namespace rr

using namespace rr;

extern "C" int rr_cls_attn_pool(rr_handle_t h, const float* x, int b, int seq, int d, const float* qt, int heads,
                                float* p, float* out, void* stream) {
  RR_ENTRY(h);
  if (!x || !qt || !out || b < 0 || seq < 1 || seq > kCapMaxSeq || d < 64 || d > 1024 || (d & 63) || heads < 1 ||
      heads > kCapMaxHeads || ((uintptr_t)x & 15) || ((uintptr_t)qt & 15) || ((uintptr_t)out & 15) ||
      ((uintptr_t)p & 15))
    return set_error(h, RR_EINVAL,
                     "rr_cls_attn_pool: bad argument (d % 64 == 0, 64 <= d <= 1024, 1 <= heads <= 16, 1 <= seq <= 256, "
                     "16-B aligned)");
  if (b == 0) return RR_OK;
  hipStream_t s = (hipStream_t)stream;
  const int d4 = d >> 2, rgs = kCapThreads / d4;
  const size_t a_floats = (size_t)heads * d + (size_t)heads * seq;
  const size_t r_floats = (size_t)rgs * heads * d;
  const size_t lds = (a_floats > r_floats ? a_floats : r_floats) * sizeof(float);  // <= 128 KiB
  TimedLaunch tl(h, kTimeAttn, s);
  hipError_t e;
  switch ((d4 + 63) >> 6) {
    case 1: e = launch_dyn_lds(cls_attn_pool_kernel<1>, (unsigned)b, kCapThreads, lds, s, x, seq, d, qt, heads, p, out); break;
    case 2: e = launch_dyn_lds(cls_attn_pool_kernel<2>, (unsigned)b, kCapThreads, lds, s, x, seq, d, qt, heads, p, out); break;
    case 3: e = launch_dyn_lds(cls_attn_pool_kernel<3>, (unsigned)b, kCapThreads, lds, s, x, seq, d, qt, heads, p, out); break;
    default: e = launch_dyn_lds(cls_attn_pool_kernel<4>, (unsigned)b, kCapThreads, lds, s, x, seq, d, qt, heads, p, out); break;
  }
  return check_hip(h, e, "cls_attn_pool launch");
}
