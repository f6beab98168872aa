// soa_ops.hip — SOLAR's second-order attention block as one fused kernel
// (gfx950): single-head self-attention over the H*W positions of the last
// feature map with a head as wide as the map's mid channels (c = 1024).
//
// Reference (networks/RetrievalNet.py:558-565, SOABlock_GeM.forward):
//   z = bmm(f^T, g); attn = softmax(c^-0.5 z, dim=-1); out = bmm(attn, h^T)
// with f, g after their ReLU.  Here the N x N scores never leave the chip:
// key tiles stream past a 16-query tile with a running max and running sum
// (online softmax), both products on the exact-fp32 MFMA.
#include <cmath>

#include "heads_common.hpp"

namespace rr {

constexpr int kSoaTile = 16;  // queries per workgroup = keys per streamed tile
constexpr int kSoaWaves = 4;  // waves per workgroup; wave w owns channels [w c/4, (w + 1) c/4)

// LDS: g tile [16][C + 4], h tile [16][C + 4], partial scores [4][16][16].
// Rows of C + 4 floats: the score step's 16-B reads (lane = key row) and the
// P.V step's 4-B reads (four key rows per wave read) are then conflict-free.
constexpr size_t soa_lds_bytes(int c) {
  return ((size_t)2 * kSoaTile * (c + 4) + kSoaWaves * kSoaTile * kSoaTile) * sizeof(float);
}

// Workgroup blockIdx.x = image * qtiles + query tile; C = 256 NV channels.
// Lane l = (lq = l & 15, lg = l >> 4).  v_mfma_f32_16x16x4_f32 maps: A[row lq]
// [k lg], B[k lg][col lq], D[row 4 lg + reg][col lq].
//
//  scores, per wave over its channel slice:  S^T = relu(g) . relu(f)^T, A = the
//   g tile (row = key), B = the wave's Q fragments (col = query), so lane
//   (lq, lg) ends with S[query lq][key 4 lg + reg].  MFMA step (j, e) sums
//   channel 16 j + 4 lg + e of the slice in both operands (one 16-B load per
//   j); four accumulators (one per e) keep the 40-cycle dependent latency off
//   the chain and are added in a fixed order.
//  the four waves' partial tiles are added through LDS in wave order; every
//   wave then does the same softmax step for all 16 queries (same operations,
//   same bits): online_softmax_step (a tile's first key is < hw).
//  O^T += h^T . P^T over the wave's own 256 NV / 4 output channels: A = the h
//   tile read at [key 4 lg + r][channel lq] (row = channel), B = p[r] as it
//   sits in the lane (k = key 4 lg + r, col = query lq): no lane movement.
//   D: lane (lq, lg) holds O[query lq][channel 16 j + 4 lg + reg], scaled by
//   the lane's own alpha before each tile and divided by its own l at the end.
// A query with relu(f) == 0 has every logit 0 and p == 1: O is the plain
// fp32 sum of the h rows in key order and l == hw.
template <int NV>
__global__ __launch_bounds__(kSoaWaves * 64) void soa_attention_kernel(const float* __restrict__ fgh, int hw, int qtiles,
                                                                       float scale, float* __restrict__ out) {
  constexpr int C = NV * 256, CS = C / kSoaWaves, NJ = CS / 16, LD = C + 4, G4 = C / 4;
  extern __shared__ __attribute__((aligned(16))) float soa_lds[];
  float* Gs = soa_lds;
  float* Hs = Gs + kSoaTile * LD;
  float* Sp = Hs + kSoaTile * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int img = blockIdx.x / qtiles, qt = blockIdx.x - img * qtiles;
  const float* base = fgh + (long long)img * hw * (3 * C);
  const int q = qt * kSoaTile + lq;
  const int c0 = wave * CS;

  f32x4 qf[NJ], o[NJ];
  {
    const bool ok = q < hw;  // a query past the map computes on zeros and is not stored
    const float* qp = base + (long long)(ok ? q : 0) * (3 * C) + c0 + 4 * lg;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      f32x4 v = *reinterpret_cast<const f32x4*>(qp + 16 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) qf[j][e] = ok ? fmaxf(v[e], 0.f) : 0.f;
      o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  float m = -__builtin_inff(), l = 0.f;
  const int ntiles = (hw + kSoaTile - 1) / kSoaTile;
  // A key tile's g and h rows (zero past hw) travel global -> registers ->
  // LDS, thread t taking 16-B group t + 256 i of the tile's 16 x C / 4.  The
  // next tile's loads are issued before this tile's arithmetic and waited
  // for only at the next store, so their latency hides under the MFMAs.
  constexpr int NI = kSoaTile * G4 / (kSoaWaves * 64);
  f32x4 gv[NI], hv[NI];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int idx = tid + i * (kSoaWaves * 64);
      const int row = idx / G4, c4 = idx - row * G4;
      const int key = kt * kSoaTile + row;
      gv[i] = hv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (key < hw) {
        const float* p = base + (long long)key * (3 * C) + c4 * 4;
        gv[i] = *reinterpret_cast<const f32x4*>(p + C);
        hv[i] = *reinterpret_cast<const f32x4*>(p + 2 * C);
      }
    }
  };
  load_tile(0);
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();  // the previous tile's readers are done with Gs / Hs / Sp
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int idx = tid + i * (kSoaWaves * 64);
      const int row = idx / G4, c4 = idx - row * G4;
      f32x4 gr;
#pragma unroll
      for (int e = 0; e < 4; ++e) gr[e] = fmaxf(gv[i][e], 0.f);
      *reinterpret_cast<f32x4*>(Gs + row * LD + c4 * 4) = gr;
      *reinterpret_cast<f32x4*>(Hs + row * LD + c4 * 4) = hv[i];
    }
    if (kt + 1 < ntiles) load_tile(kt + 1);
    __syncthreads();

    f32x4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const f32x4 kf = *reinterpret_cast<const f32x4*>(Gs + lq * LD + c0 + 16 * j + 4 * lg);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], qf[j][e], acc[e], 0, 0, 0);
    }
    *reinterpret_cast<f32x4*>(Sp + wave * (kSoaTile * kSoaTile) + lq * kSoaTile + 4 * lg) =
        (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();

    const float* sp = Sp + lq * kSoaTile + 4 * lg;
    const f32x4 s = (*reinterpret_cast<const f32x4*>(sp) + *reinterpret_cast<const f32x4*>(sp + 256)) +
                    (*reinterpret_cast<const f32x4*>(sp + 512) + *reinterpret_cast<const f32x4*>(sp + 768));
    const SoftmaxTile st = online_softmax_step(s, kt * kSoaTile, hw, scale, lg, m, l);
    const f32x4 p = st.p;
    const float alpha = st.alpha;
    l = st.l;
    m = st.m;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      o[j] *= alpha;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(Hs[(4 * lg + r) * LD + c0 + 16 * j + lq], p[r], o[j], 0, 0, 0);
    }
  }
  if (q < hw) {
    float* op = out + ((long long)img * hw + q) * C + c0 + 4 * lg;
#pragma unroll
    for (int j = 0; j < NJ; ++j) *reinterpret_cast<f32x4*>(op + 16 * j) = o[j] / l;
  }
}

template <int NV>
static hipError_t launch_soa(const float* fgh, int hw, int qtiles, float scale, float* out, unsigned blocks,
                             hipStream_t s) {
  return launch_dyn_lds(soa_attention_kernel<NV>, blocks, kSoaWaves * 64, soa_lds_bytes(NV * 256), s, fgh, hw, qtiles,
                        scale, out);
}

}  // namespace rr

using namespace rr;

extern "C" int rr_soa_attention(rr_handle_t h, const float* fgh, int b, int hw, int c, float* out, void* stream) {
  RR_ENTRY(h);
  if (!fgh || !out || b < 0 || hw < 1 || hw > 65535 || c < 256 || c > 1024 || (c & 255) || ((uintptr_t)fgh & 15) ||
      ((uintptr_t)out & 15))
    return set_error(h, RR_EINVAL,
                     "rr_soa_attention: bad argument (c % 256 == 0, 256 <= c <= 1024, 1 <= hw <= 65535, 16-B aligned)");
  if (b == 0) return RR_OK;
  const int qtiles = (hw + kSoaTile - 1) / kSoaTile;
  const long long blocks = (long long)b * qtiles;
  if (blocks > 0x7fffffffLL) return set_error(h, RR_EINVAL, "rr_soa_attention: too many images");
  // torch multiplies the fp32 scores by the Python float c ** -0.5 rounded to fp32 (:563)
  const float scale = (float)std::pow((double)c, -0.5);
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch tl(h, kTimeAttn, s);
  hipError_t e;
  switch (c >> 8) {
    case 1: e = launch_soa<1>(fgh, hw, qtiles, scale, out, (unsigned)blocks, s); break;
    case 2: e = launch_soa<2>(fgh, hw, qtiles, scale, out, (unsigned)blocks, s); break;
    case 3: e = launch_soa<3>(fgh, hw, qtiles, scale, out, (unsigned)blocks, s); break;
    default: e = launch_soa<4>(fgh, hw, qtiles, scale, out, (unsigned)blocks, s); break;
  }
  return check_hip(h, e, "soa_attention launch");
}
