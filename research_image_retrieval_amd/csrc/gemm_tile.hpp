// gemm_tile.hpp — what the GEMM kernels on 128-byte LDS rows share around
// their k-loops (gemm_f32.hip, gemm_lp.hip, gemm_lpp.hip, gemm_8p.hip): the
// LDS slot swizzle, the MFMA / DS-read schedule pins, the filter epilogue's
// inner step, the four-row E_SCORES_T store and the one-tile-per-block launch.
// Every device helper is forced inline and each call site keeps its own loop
// order, so candidates reach the buffer in the order the site's loops visit
// the accumulator.
//
// Only what left every kernel's machine code as it was is shared
// (tools/kernel_body_diff.py).  Still written out at each site, because the
// helper (with GemmArgs by value too) changed some kernel's code: the 16x16x32
// bf16 fragment read (gemm_lp.hip three times, gemm_lpp.hip twice), the
// filter step in gemm_8p.hip (twice), sweep16.hip's swizzle arithmetic, the
// 32x32 rank epilogue loop and the LayerNorm-fold staging of gemm_lp.hip.
#pragma once

#include "gemm_epilogue.hpp"
#include "rr_internal.hpp"

namespace rr {

// input element type of A/B: DT_F32 (v_mfma_f32_32x32x2_f32), DT_BF16
// (v_mfma_f32_32x32x16_bf16), DT_FP8 (OCP e4m3, v_mfma_scale_f32_32x32x64_f8f6f4
// with unit block scales).
// LDS rows are 128 B for all three (32 fp32 / 64 bf16 / 128 fp8 per k-tile),
// so staging, swizzle and epilogues are shared.
template <int DT> struct ElemT { using T = float; };
template <> struct ElemT<DT_BF16> { using T = uint16_t; };
template <> struct ElemT<DT_FP8> { using T = uint8_t; };

// 16-byte-slot XOR swizzle of a [rows][BK] fp32 LDS image, conflict-free for
// the fragment ds_read_b128 (16 lanes = 16 rows distinct mod 16, one slot):
// BK = 32 (8 slots per 128-B row): slot ^ ((row >> 1) & 7);
// BK = 16 (4 slots per 64-B row):  slot ^ ((row >> 2) & 3).
template <int BK = 32>
__device__ __forceinline__ int swz(int row, int slot) {
  if constexpr (BK == 32) return slot ^ ((row >> 1) & 7);
  else return slot ^ ((row >> 2) & 3);
}

// Pin the scheduler to alternate MFMAs with the next k-step's LDS fragment
// reads (NR reads, NM >= NR MFMAs in the region): MFMA, read, MFMA, read,
// ..., then the remaining MFMAs, so the reads' latency runs under MFMAs.
template <int NR, int NM>
__device__ __forceinline__ void interleave() {
#pragma unroll
  for (int x = 0; x < NR; ++x) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
  }
  if constexpr (NM > NR) __builtin_amdgcn_sched_group_barrier(0x008, NM - NR, 0);
}

// interleave<nr, NM> with the next k-tile's LDS-DMA chunks spread among the
// MFMAs (IL sweeps): chunk c of NCH goes out before MFMA number (c * SPAN) /
// NCH of the k-tile; base = the k-tile's MFMA number of this region's first
// (base and nr constant once the caller's k-step loop is unrolled).
template <int NM, int SPAN, int NCH, int DSPER = 1>
__device__ __forceinline__ void interleave_il(int base, int nr) {
#pragma unroll
  for (int x = 0; x < NM; ++x) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if ((c * SPAN) / NCH == base + x) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM (the DMA)
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                      // 1 MFMA
    if (x < nr) __builtin_amdgcn_sched_group_barrier(0x100, DSPER, 0);                      // DSPER DS reads
  }
}

// Same with two DS reads per MFMA (NP pairs, NM >= NP MFMAs): the fp8 k-step
// reads 32 bytes (two ds_read_b128) per fragment.
template <int NP, int NM>
__device__ __forceinline__ void interleave2() {
  static_assert(NM >= NP, "interleave2: fewer MFMAs than read pairs");
#pragma unroll
  for (int x = 0; x < NP; ++x) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // 2 DS reads
  }
  if constexpr (NM > NP) __builtin_amdgcn_sched_group_barrier(0x008, NM - NP, 0);
}

// E_FILTER, one accumulator value: score v of gallery row m for query n (nok:
// n < N) is kept if it lies strictly above the query's threshold t (as
// !(v <= t): a NaN score, or every score under a NaN threshold, is kept; the
// NaN keys rank last in select_final, see ord_f32).  Rows past M and the
// padding query columns are excluded explicitly: a NaN gallery row gives NaN
// there too, and no counter exists for them.  (g by value: through a reference
// to the kernel's argument struct hipcc generated different code.)
__device__ __forceinline__ void filter_emit(const GemmArgs g, bool nok, float v, float t, int n, int m) {
  if (nok && m < g.M && !(v <= t)) {
    const int pos = atomicAdd(g.cnt + n, 1);
    if (pos < g.cap) g.cand[(long long)n * g.cap + pos] = make_key(v, (uint32_t)(g.row_offset + m));
  }
}

// E_SCORES_T, four consecutive rows mb .. mb + 3 of query n (nok: n < N) from
// the accumulator's elements r0 .. r0 + 3: one 16-byte store where all four
// are rows of A, else row by row.  (g by value, as filter_emit.)
template <class V>
__device__ __forceinline__ void store_rows4(const GemmArgs g, bool nok, const V& a, int r0, int n, int mb) {
  if (!nok) return;
  float* dst = g.C + (long long)n * g.ldc + mb;
  if (mb + 3 < g.M) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{a[r0], a[r0 + 1], a[r0 + 2], a[r0 + 3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (mb + e < g.M) dst[e] = a[r0 + e];
  }
}

// One block of NT threads per BM x BN tile (blockIdx.y: the split-K part).
template <int BM, int BN, int NT>
hipError_t launch_tiles(void (*kernel)(GemmArgs, int), const GemmArgs& g, hipStream_t s) {
  const long long tiles_m = (g.M + BM - 1) / BM;
  const long long tiles_n = (g.N + BN - 1) / BN;
  const long long nblk = tiles_m * tiles_n;
  if (nblk <= 0) return hipSuccess;
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  const unsigned splits = g.k_split > 0 ? (unsigned)((g.K + g.k_split - 1) / g.k_split) : 1u;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblk, splits), dim3(NT), 0, s, g, (int)tiles_n);
  return hipGetLastError();
}

}  // namespace rr
