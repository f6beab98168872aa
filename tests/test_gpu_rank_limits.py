"""The rankers at the limits include/rr.h documents, which the shapes of
tests/test_gpu_rank.py (written around the benchmark's) never reach:

* k in (8192, 16384]: topk.hip sorts pow2(k) * 8 bytes of keys in dynamic LDS;
  above k = 8192 that is 128 KB beside the static SelShared, raised through
  hipFuncSetAttribute (select_dense_seed, select_final, merge, and the
  prefilter's threshold + rescore between the first two);
* n at and one past the threshold-seeding sample (the filter GEMM with M = 1),
  d = 4 and d = 20 (the fmaf chain zero-padded to 16), idx_offset >= 2^32;
* rr_topk_merge with one part, k_in = 1, nothing but padding, fewer valid
  entries than k_out, indices up to 2^32 - 2;
* NaN descriptors (extract_vectors yields them when every scale is dropped,
  utils/helpfunc.py:39-44) through every filter sweep and both low-precision
  rankers, fp8 quantisation included.

Reference: oracle/cosine_topk.c (iris_evaluate.py:383 torch.mm + :386
np.argsort with a stable tie-break), bit for bit, for the exact rankers; the
float64 dot products of the dequantised rows for the low-precision ones."""
import functools

import numpy as np
import pytest
import torch

import oracle
from research_image_retrieval_amd import ops
from research_image_retrieval_amd.search import search

pytestmark = pytest.mark.gpu


def _normed(rs, n, d):
    x = rs.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def _planted(seed, nq, n, d):
    """Unit rows with two exact duplicates of each query planted in the gallery
    (equal scores: the tie-break on the index decides their order)."""
    rs = np.random.RandomState(seed)
    q, g = _normed(rs, nq, d), _normed(rs, n, d)
    for i in range(nq):
        j = int(rs.randint(n))
        g[j] = q[i]
        g[(j + 3) % n] = q[i]
    return q, g


def _dev(cuda, *arrays):
    return [torch.from_numpy(a).to(cuda) for a in arrays]


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _prefilter(qd, gd, k, **kw):
    gb, _ = ops.quantize_rows(gd, "bf16")
    return ops.cosine_topk_prefilter(qd, gd, gb, ops.prefilter_gallery_bound(gd, gb), k, **kw)


# ---- A1: k in (8192, 16384], exact rankers ---------------------------------

@functools.lru_cache(maxsize=None)
def _large_k_case():
    q, g = _planted(101, 3, 20000, 64)
    s_ref, i_ref = oracle.cosine_topk(q, g, 16384)  # a top-k list is a prefix of every longer one
    return q, g, s_ref, i_ref


@pytest.mark.parametrize("k", [8192, 8193, 16384])
def test_large_k_exact_rankers_match_oracle(cuda, k):
    """k = 8192 is the last size whose 64 KB of keys needs no attribute, 8193
    the first that sorts 16384 keys (128 KB), 16384 the documented maximum.
    The exhaustive ranker equals the oracle, the prefilter the exhaustive
    ranker, scores and indices bit for bit."""
    q, g, s_ref, i_ref = _large_k_case()
    qd, gd = _dev(cuda, q, g)
    s, i = ops.cosine_topk(qd, gd, k)
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref[:, :k])
    np.testing.assert_array_equal(_bits(s), s_ref[:, :k].view(np.int32))
    s1, i1 = _prefilter(qd, gd, k)
    assert torch.equal(i1, i) and torch.equal(s1.view(torch.int32), s.view(torch.int32))


def test_large_k_exceeds_gallery(cuda):
    """n = 12000 < k = 16384: the first n entries are the full stable ranking,
    the tail is (-inf, -1); both exact rankers."""
    n, k = 12000, 16384
    q, g = _planted(102, 3, n, 64)
    s_ref, i_ref = oracle.cosine_topk(q, g, n)
    qd, gd = _dev(cuda, q, g)
    s, i = ops.cosine_topk(qd, gd, k)
    s1, i1 = _prefilter(qd, gd, k)
    for ss, ii in ((s, i), (s1, i1)):
        ss, ii = ss.cpu().numpy(), ii.cpu().numpy()
        np.testing.assert_array_equal(ii[:, :n], i_ref)
        np.testing.assert_array_equal(ss[:, :n].view(np.int32), s_ref.view(np.int32))
        assert (ii[:, n:] == -1).all() and np.isneginf(ss[:, n:]).all()


def test_search_full_ranking_above_8192_rows(cuda):
    """search(k=None) on 8193..16384 gallery rows (search.MAX_FULL_RANK) ranks
    with k = N: the oracle's stable full ranking, int64 [N, Q]."""
    q, g = _planted(103, 5, 12000, 64)
    ranks, scores = search(q, g, k=None, return_scores=True, device=cuda, normalize=False)
    sim = oracle.cosine_scores(q, g)
    order = oracle.argsort_stable_desc(sim)
    assert ranks.shape == (12000, 5) and ranks.dtype == np.int64
    np.testing.assert_array_equal(ranks, order.T)
    np.testing.assert_array_equal(scores.view(np.int32), np.take_along_axis(sim, order, 1).view(np.int32))


# ---- A2: k = 16384, low precision -----------------------------------------

@pytest.mark.parametrize("dtype,d", [("bf16", 64), ("fp8", 128)])
def test_large_k_lowp_vs_dequantised(cuda, dtype, d):
    """rr_cosine_topk_lp at k = 16384, checked as
    test_gpu_lowp.py::test_lowp_topk_many_queries_vs_dequantised checks k =
    100, at its tolerances: the scores are the dot products of the dequantised
    rows (float64 here), descending, and every returned row scores at least
    the reference's k-th best minus 1e-5."""
    k, nq, n = 16384, 3, 20000
    rs = np.random.RandomState(104 + d)
    qd, gd = _dev(cuda, _normed(rs, nq, d), _normed(rs, n, d))
    gl, gs = ops.quantize_rows(gd, dtype)
    ql, qs = ops.quantize_rows(qd, dtype)
    s, i = ops.cosine_topk_lp(ql, qs, gl, gs, k, dtype)
    if dtype == "bf16":
        gf, qf = gl.cpu().double(), ql.cpu().double()
    else:
        gf = gl.cpu().view(torch.float8_e4m3fn).double() * gs.cpu().double()[:, None]
        qf = ql.cpu().view(torch.float8_e4m3fn).double() * qs.cpu().double()[:, None]
    ref = qf @ gf.t()
    s, i = s.cpu(), i.cpu()
    assert int(i.min()) >= 0 and all(len(set(r.tolist())) == k for r in i)  # k distinct rows per query
    got = torch.gather(ref, 1, i)
    torch.testing.assert_close(s.double(), got, rtol=1e-4, atol=1e-5)
    assert bool((s[:, :-1] >= s[:, 1:]).all())
    kth = torch.topk(ref, k, dim=1).values[:, -1:]
    assert bool((s.double() >= kth - 1e-5).all())


# ---- A3: rr_topk_merge -----------------------------------------------------

def _merge_vs_oracle(cuda, ps, pi, kout):
    so, io = ops.topk_merge(torch.from_numpy(ps).to(cuda), torch.from_numpy(pi).to(cuda), kout)
    sr, ir = oracle.topk_merge(ps, pi, kout)
    so, io = so.cpu().numpy(), io.cpu().numpy()
    np.testing.assert_array_equal(io, ir)
    np.testing.assert_array_equal(so.view(np.int32), sr.view(np.int32))
    return so, io


def test_merge_large_k(cuda):
    """Three parts of 8000 into k_out = 16384 (128 KB of keys): 24000 entries
    minus padding, cross-part exact ties, more valid entries than k_out."""
    rs = np.random.RandomState(105)
    P, nq, kin = 3, 2, 8000
    ps = rs.standard_normal((P, nq, kin)).astype(np.float32)
    pi = rs.permutation(P * nq * kin).reshape(P, nq, kin).astype(np.int64)
    ps[1, :, :50] = ps[0, :, :50]
    pi[2, :, -100:] = -1
    so, io = _merge_vs_oracle(cuda, ps, pi, 16384)
    assert (io >= 0).all()


def test_merge_shape_edges(cuda):
    """One part; k_in = 1 over eight parts; nothing but padding; k_out above
    the number of valid entries; indices 2^32 - 2 and 2^32 - 3 (rr.h: < 2^32 -
    1) with equal scores, the smaller index first."""
    rs = np.random.RandomState(106)
    # one part, unsorted input, k_out < k_in and k_out > k_in
    ps = rs.standard_normal((1, 3, 70)).astype(np.float32)
    pi = rs.permutation(3 * 70).reshape(1, 3, 70).astype(np.int64)
    _merge_vs_oracle(cuda, ps, pi, 20)
    so, io = _merge_vs_oracle(cuda, ps, pi, 100)
    assert (io[:, 70:] == -1).all() and np.isneginf(so[:, 70:]).all()
    # k_in = 1, eight parts
    ps = rs.standard_normal((8, 5, 1)).astype(np.float32)
    pi = rs.permutation(40).reshape(8, 5, 1).astype(np.int64)
    ps[3], ps[6] = ps[1], ps[1]  # ties across parts
    _merge_vs_oracle(cuda, ps, pi, 1)
    _merge_vs_oracle(cuda, ps, pi, 8)
    _merge_vs_oracle(cuda, ps, pi, 11)
    # every entry padding
    ps = rs.standard_normal((2, 3, 9)).astype(np.float32)
    pi = np.full((2, 3, 9), -1, np.int64)
    so, io = _merge_vs_oracle(cuda, ps, pi, 7)
    assert (io == -1).all() and np.isneginf(so).all()
    # 37 valid entries, k_out = 100
    ps = rs.standard_normal((4, 1, 25)).astype(np.float32)
    pi = np.full((4, 1, 25), -1, np.int64)
    flat = rs.permutation(100)[:37]
    pi.reshape(-1)[flat] = rs.permutation(10_000)[:37]
    so, io = _merge_vs_oracle(cuda, ps, pi, 100)
    assert (io[0, :37] >= 0).all() and (io[0, 37:] == -1).all() and np.isneginf(so[0, 37:]).all()
    # the largest indices the key holds, equal scores
    ps = np.array([[[0.5, 0.25]], [[0.5, 0.5]]], np.float32)  # [2][1][2]
    pi = np.array([[[2**32 - 2, 7]], [[2**32 - 3, 2**32 - 4]]], np.int64)
    so, io = _merge_vs_oracle(cuda, ps, pi, 4)
    assert io[0].tolist() == [2**32 - 4, 2**32 - 3, 2**32 - 2, 7]
    assert so[0].tolist() == [0.5, 0.5, 0.5, 0.25]


# ---- A4: size edges --------------------------------------------------------

@pytest.mark.parametrize("nq,n,d,k,prefilter", [(5, 4096, 64, 10, True), (5, 4097, 64, 10, True),
                                               (1, 5000, 4, 3, False), (257, 5000, 20, 7, False)])
def test_rank_size_edges(cuda, nq, n, d, k, prefilter):
    """n = the seed sample exactly (no filter pass) and one row past it (the
    filter GEMM with M = 1; the planted best match of query 0 is that row);
    d = 4 and d = 20 (the chain's 16-deep chunks zero-padded; these do not
    meet the prefilter's d % 8 == 0); 257 queries (a third 128-wide tile
    column holding one query).  idx_offset = 2^33 + 5 shifts the indices and
    nothing else."""
    q, g = _planted(107 + n + d, nq, n, d)
    g[n - 1] = q[0]
    s_ref, i_ref = oracle.cosine_topk(q, g, k)
    qd, gd = _dev(cuda, q, g)
    s, i = ops.cosine_topk(qd, gd, k)
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(_bits(s), s_ref.view(np.int32))
    off = 2**33 + 5
    s2, i2 = ops.cosine_topk(qd, gd, k, idx_offset=off)
    assert torch.equal(i2, i + off) and torch.equal(s2.view(torch.int32), s.view(torch.int32))
    if prefilter:
        s1, i1 = _prefilter(qd, gd, k)
        assert torch.equal(i1, i) and torch.equal(s1.view(torch.int32), s.view(torch.int32))
        s3, i3 = _prefilter(qd, gd, k, idx_offset=off)
        assert torch.equal(i3, i + off) and torch.equal(s3.view(torch.int32), s.view(torch.int32))


# ---- A5: NaN descriptors through every sweep -------------------------------

NAN_ROWS = (5, 15000, 16000)  # gallery rows of _nan_case holding a NaN
NAN_Q = 4                     # its all-NaN query


@functools.lru_cache(maxsize=None)
def _nan_case(nq, d):
    """The data of test_gpu_rank.py::test_nan_rows_and_queries_rank_last at
    (nq, d): an all-NaN row inside the seed sample (the first 4096 rows), one
    NaN element in row 15000, a copy of the NaN row at 16000, an all-NaN
    query; and a 40-row gallery with two NaN rows (5, and one element of 33)
    for k = 60.  The oracle's scores and stable rankings are computed once per
    (nq, d) and shared by every parametrisation.  Returns q, g, g40, the
    expected (order, scores) at k = 100 on g and at k = 60 on g40, and the
    100th-best finite exact score per query."""
    rs = np.random.RandomState(17 + nq + d)
    n = 20000
    g, q = _normed(rs, n, d), _normed(rs, nq, d)
    g[5] = np.nan
    g[15000, 7] = np.nan
    g[16000] = g[5]
    q[NAN_Q] = np.nan
    g40 = g[:40].copy()
    g40[33, 2] = np.nan
    expect = []
    for gal, k in ((g, 100), (g40, 60)):
        sim = oracle.cosine_scores(q, gal)
        order = oracle.argsort_stable_desc(sim)[:, :k]
        expect.append((order, np.take_along_axis(sim, order, 1)))
    s100 = expect[0][1][:, 99]  # NaN ranks last: the 100th entry is the 100th-best finite score
    return q, g, g40, expect, s100


def _assert_nan_expectation(s, i, order, ref_s, kk):
    """(s, i) of an exact ranker against the oracle's stable order and scores
    (first kk columns; the rest padding): NaN scores last, by index; the NaN
    query returns 0..kk-1."""
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert np.array_equal(i[:, :kk], order[:, :kk]), np.argwhere(i[:, :kk] != order[:, :kk])[:5]
    assert np.array_equal(np.isnan(s[:, :kk]), np.isnan(ref_s))
    fin = ~np.isnan(ref_s)
    assert np.array_equal(s[:, :kk][fin], ref_s[fin])
    assert (i[:, kk:] == -1).all() and np.isneginf(s[:, kk:]).all()
    assert list(i[NAN_Q, :kk]) == list(range(kk)) and np.isnan(s[NAN_Q, :kk]).all()


@pytest.mark.parametrize("nq,d,tune", [
    (6, 128, dict(sweep_form=0)), (6, 128, dict(sweep_form=1)), (6, 128, dict(sweep_form=2)),
    (256, 256, dict(sweep_form=0)), (256, 256, dict(sweep_form=1)), (256, 256, dict(sweep_form=2)),
    (256, 256, dict(sweep_form=0, lp_cfg=3)), (256, 256, dict(sweep_form=0, lp_cfg=4)),
    (256, 256, dict(sweep_form=0, lp_cfg=5)),
    (33, 192, dict(sweep_form=0, lp_cfg=2)), (33, 192, dict(sweep_form=0, lp_cfg=4, sweep_il=0)),
    (33, 192, dict(sweep_form=0, lp_cfg=4, sweep_mf16=1, sweep_il=0)),
    (33, 192, dict(sweep_form=0, lp_cfg=4, sweep_mf16=1)),
], ids=lambda v: "-".join(f"{a}{b}" for a, b in v.items()) if isinstance(v, dict) else str(v))
def test_nan_rank_last_prefilter_every_sweep(cuda, nq, d, tune):
    """The expectation of test_nan_rows_and_queries_rank_last (NaN scores rank
    after every number, by index; the NaN query returns 0..k-1; k > #rows pads
    with (-inf, -1)) for the exact prefilter ranker under every bf16 filter
    sweep.  Which kernel runs pass 2 (and, for the gemm core's configs, the
    seed scores) is gemm_route's answer (csrc/gemm_route.hpp), asserted for these
    parameter sets in tests/test_gemm_route.py::test_claims_of_the_gpu_tests:

    * sweep_form 0 at the default lp_cfg: the cost model (lp_pick_cfg) gives the
      128x128 tile of gemm_lp_kernel (16x16x32 bf16 MFMA) at both (6, 128) and
      (256, 256) over 20000 rows;
    * sweep_form 1: sweep128_kernel of csrc/sweep16.hip (128-B LDS rows, K %
      64 == 0: both d qualify); sweep_form 2: sweep16_kernel<8> (64-B rows);
      nq = 256 leaves 64 of the tile's 320 query columns as padding, whose
      threshold is +inf;
    * lp_cfg 3: gemm_lp_kernel's 8-wave 256x256 tile (LDS-DMA, K % 64 == 0);
      lp_cfg 4: its 256x320 tile on 32x32x16 MFMA (<4, 2, 2, 5>),
      by default with the next k-tile's DMA spread among the MFMAs; sweep_il 0:
      as one burst; sweep_mf16 1: the tile's 16x16x32 form, with either DMA
      issue; lp_cfg 2: the 4-wave 256x64 tile.  These four run 33 queries
      (a ragged query tile) at d = 192 (three whole 64-deep k-tiles: both LDS
      buffers, an odd tile count);
    * lp_cfg 5: the 8-phase pipeline of csrc/gemm_8p.hip (K % 128 == 0), its
      E_FILTER and, for the seed, E_SCORES_T epilogues; 256 queries = one
      full panel.
    Each of the three files has its own copy of the !(s <= tau) filter."""
    q, g, g40, expect, _ = _nan_case(nq, d)
    for (gal, k), (order, ref_s) in zip(((g, 100), (g40, 60)), expect):
        qd, gd = _dev(cuda, q, gal)
        with ops.tuning(cuda.index, **tune):
            s, i = _prefilter(qd, gd, k)
        _assert_nan_expectation(s, i, order, ref_s, min(k, gal.shape[0]))


@pytest.mark.parametrize("cfg,bk", [(22, 16), (22, 32), (41, 16), (41, 32)])
def test_nan_rank_last_exact_every_f32_tile(cuda, cfg, bk):
    """The same expectation for rr_cosine_topk on each tile of the fp32 core
    (gemm_f32_kernel, csrc/gemm_f32.hip) that serves the rankers: 128x128
    (gemm_cfg 22) and 256x64 (41) at k-tile depth 16 and 32, their E_SCORES_T
    (the seed sample) and E_FILTER (the rows past it) epilogues.  The default
    pick only reaches 22 / 16 at these sizes.  33 queries at d = 192: a ragged
    query tile, 12 or 6 k-tiles."""
    q, g, g40, expect, _ = _nan_case(33, 192)
    for (gal, k), (order, ref_s) in zip(((g, 100), (g40, 60)), expect):
        qd, gd = _dev(cuda, q, gal)
        with ops.tuning(cuda.index, gemm_cfg=cfg, gemm_bk=bk):
            s, i = ops.cosine_topk(qd, gd, k)
        _assert_nan_expectation(s, i, order, ref_s, min(k, gal.shape[0]))


@pytest.mark.parametrize("dtype,nq,d,tune", [
    ("bf16", 6, 128, dict(sweep_form=0, lp_cfg=0)), ("bf16", 6, 128, dict(sweep_form=1)),
    ("bf16", 6, 128, dict(sweep_form=2)), ("bf16", 256, 256, dict(sweep_form=0, lp_cfg=0)),
    ("bf16", 256, 256, dict(sweep_form=1)), ("bf16", 256, 256, dict(sweep_form=2)),
    ("bf16", 256, 256, dict(sweep_form=0, lp_cfg=5)),
    ("fp8", 6, 128, dict(lp_cfg=0)), ("fp8", 256, 256, dict(lp_cfg=0)), ("fp8", 256, 256, dict(lp_cfg=3)),
    ("fp8", 256, 256, dict(lp_cfg=5)), ("fp8", 33, 384, dict(lp_cfg=2)),
], ids=lambda v: "-".join(f"{a}{b}" for a, b in v.items()) if isinstance(v, dict) else str(v))
def test_nan_rank_last_lowp_every_sweep(cuda, dtype, nq, d, tune):
    """NaN rows and a NaN query through rr_cosine_topk_lp.  Kernels (gemm_route,
    asserted in tests/test_gemm_route.py): bf16 takes the same sweeps as the prefilter's pass 2
    (sweep_form 0 + lp_cfg 0: gemm_lp_kernel's 128x128 tile; sweep_form 1 / 2:
    sweep128_kernel / sweep16_kernel<8> of csrc/sweep16.hip; lp_cfg 5: the
    8-phase bf16 pipeline of csrc/gemm_8p.hip, K % 128 == 0).  fp8 has no
    sweep16 form (it carries row scales): lp_cfg 0 is gemm_lp_kernel's 128x128
    tile dequantising in its epilogue, lp_cfg 2 its 256x64 tile (33 queries,
    d = 384: a ragged query tile, three whole 128-deep k-tiles), lp_cfg 3 its
    8-wave 256x256 tile on the block-scaled MFMA, lp_cfg 5 gemm_8p.hip's fp8 pipeline on the 32x32x64
    block-scaled MFMA (K % 256 == 0, hence d = 256) with its own scale and
    filter epilogue.

    The low-precision scores are not the oracle's, so:
    1. at k = 100 the finite queries' output equals, bit for bit, that of the
       same call on a gallery whose NaN rows are zero rows; every returned
       score is > 0, which puts the zero rows (score +-0) outside the top 100,
       so this says the NaN rows displaced nothing.  (The exact 100th-best
       score is checked > 0.1 on the CPU, far above the quantisation error,
       so the > 0 assertion is not a coincidence of the seed.)
    2. on the 40-row gallery at k = 60 the finite rows come first, then the NaN
       rows by index with NaN scores, then (-inf, -1);
    3. the NaN query returns 0..k-1 with NaN scores."""
    q, g, g40, _, s100 = _nan_case(nq, d)
    finite_q = [r for r in range(nq) if r != NAN_Q]
    assert (s100[finite_q] > 0.1).all(), s100[finite_q].min()
    clean = g.copy()
    clean[list(NAN_ROWS)] = 0.0

    def run(gal, k):
        qd, gd = _dev(cuda, q, gal)
        gl, gs = ops.quantize_rows(gd, dtype)
        ql, qs = ops.quantize_rows(qd, dtype)
        with ops.tuning(cuda.index, **tune):
            s, i = ops.cosine_topk_lp(ql, qs, gl, gs, k, dtype)
        return s.cpu().numpy(), i.cpu().numpy()

    s, i = run(g, 100)
    s0, i0 = run(clean, 100)
    assert np.array_equal(i[finite_q], i0[finite_q]), np.argwhere(i != i0)[:5]
    assert np.array_equal(s[finite_q].view(np.int32), s0[finite_q].view(np.int32))
    assert (s[finite_q] > 0).all(), s[finite_q].min()
    assert not np.isin(i[finite_q], NAN_ROWS).any()
    assert list(i[NAN_Q]) == list(range(100)) and np.isnan(s[NAN_Q]).all()

    s, i = run(g40, 60)
    nan40 = [5, 33]
    for r in finite_q:
        assert sorted(i[r, :38]) == [j for j in range(40) if j not in nan40]
        assert np.isfinite(s[r, :38]).all() and (s[r, :37] >= s[r, 1:38]).all()
        assert list(i[r, 38:40]) == nan40 and np.isnan(s[r, 38:40]).all()
    assert list(i[NAN_Q, :40]) == list(range(40)) and np.isnan(s[NAN_Q, :40]).all()
    assert (i[:, 40:] == -1).all() and np.isneginf(s[:, 40:]).all()


def test_fp8_quantize_keeps_nan(cuda):
    """rr_quantize_rows fp8 (rr.h): a row holding a NaN gets a NaN scale, so
    each of its elements dequantises to NaN (byte an e4m3 NaN, or scale NaN);
    its finite elements are still quantised at amax(finite) / 448 and meet the
    bound of test_gpu_lowp.py::test_fp8_quantize_and_scores against that
    scale; rows without a NaN keep their bytes and scale (checked against the
    quantisation of the same rows in a batch that holds no NaN)."""
    rs = np.random.RandomState(108)
    x = _normed(rs, 50, 512)
    bad = x.copy()
    bad[3] = np.nan          # every element
    bad[17, 100] = np.nan    # one element
    bad[40, ::2] = np.nan    # every lane holds some
    nan_rows = [3, 17, 40]
    xq, xs = ops.quantize_rows(torch.from_numpy(x).to(cuda), "fp8")
    bq, bs = ops.quantize_rows(torch.from_numpy(bad).to(cuda), "fp8")
    xq, xs, bq, bs = xq.cpu(), xs.cpu(), bq.cpu(), bs.cpu()
    keep = [r for r in range(50) if r not in nan_rows]
    assert torch.equal(bq[keep], xq[keep]) and torch.equal(bs[keep].view(torch.int32), xs[keep].view(torch.int32))
    f8 = bq.view(torch.float8_e4m3fn).float()
    deq = f8 * bs[:, None]
    badt = torch.from_numpy(bad)
    assert bool(torch.isnan(deq[torch.isnan(badt)]).all())
    assert bool(torch.isfinite(deq[keep]).all())
    for r in (17, 40):
        fin = ~torch.isnan(badt[r])
        scale = badt[r][fin].abs().max() / 448.0  # fp32, as the kernel computes it
        err = (f8[r][fin] * scale - badt[r][fin]).abs()
        # e4m3: 3 mantissa bits -> half-ulp 2^-4 relative; subnormals 2^-10 absolute (in scaled units)
        assert bool((err <= badt[r][fin].abs() * 2.0 ** -4 + 2.0 ** -10 * scale).all()), (r, err.max())
