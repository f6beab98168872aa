"""Token on the GPU: rr_attention_hd128, rr_token_pool and rr_gelu against the
float64 evaluation of tests/token_ref.py (pinned to the reference's own output
by tests/test_token_host.py), and networks.Token / RetrievalNet end to end and
head-only against tests/golden/token.npz (the reference's Token.forward_test and
Token_Refine, make_golden_token.py).

The kernel bar, per case: max over rows of max|got - ref| / ||ref row||_2 <=
max(1e-6, 4 e32), e32 the same quantity for the float32 torch evaluation
(computed here and printed), as tests/test_gpu_solar.py.  The descriptor bar:
max(2e-6, 4 x the float32 restatement's distance from the float64 one)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from research_image_retrieval_amd import _lib, ops
from research_image_retrieval_amd import weights as W
from research_image_retrieval_amd.extract import extract_vectors
from research_image_retrieval_amd.networks import ConvDimReduction, GeMPCAw, RetrievalNet, Token

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
import inputs as I  # noqa: E402
import token_ref  # noqa: E402

BAR = 1e-6
ATT_SHAPES = [(1, 1, 1, 1), (2, 4, 4, 8), (2, 15, 15, 8), (1, 16, 16, 1), (1, 17, 17, 8), (3, 33, 33, 2),
              (2, 49, 49, 8), (1, 65, 130, 8), (64, 49, 49, 8), (1, 323, 323, 8), (1, 1024, 1024, 8),
              (2, 4, 49, 8), (3, 4, 35, 8), (1, 4, 1024, 8), (1, 1, 17, 8)]
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19))


def _row_err(got, ref):
    """max over rows of max|got - ref| / ||ref row||_2"""
    return ((got.double() - ref.double()).abs().amax(dim=-1) / ref.double().norm(dim=-1)).max().item()


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- rr_attention_hd128 ----------------------------------------------------
def _att_case(b, nq, nk, heads, plant=True, gain=2.0):
    """q, k, v = N(0,1) with q and k scaled by 2 (logits N(0, 4^2): they reach
    10-20; the unplanted cases pass gain 1.5, logits N(0, 2.25^2) that reach 10
    at the larger shapes, so that no row is a one-hot).  Planted where nk >= 8:
    one all-zero query (uniform attention: the mean of the v rows), and in head 0 one key equal to 3 x another query (a
    logit of ~135: weight > 0.999, the running max jumps).  Where the only
    query must serve both (b == nq == 1) the zero query keeps head 0."""
    rs = np.random.RandomState(100000 * b + 1000 * nq + nk + heads)
    w = heads * 128
    q = rs.standard_normal((b, nq, w)).astype(np.float32) * np.float32(gain)
    k = rs.standard_normal((b, nk, w)).astype(np.float32) * np.float32(gain)
    v = rs.standard_normal((b, nk, w)).astype(np.float32)
    special = {}
    if plant and nk >= 8:
        zq, dq, dk = (0, nq // 3), (1 % b, nq // 2), nk - 2
        h0 = 1 if zq == dq else 0
        k[dq[0], dk, :128] = 3.0 * q[dq[0], dq[1], :128]
        q[zq[0], zq[1], 128 * h0:] = 0.0
        special = {"zero_query": zq, "zero_from_head": h0, "dominant": (dq, dk)}
    return torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(v), special


def _att_ref(q, k, v, heads, dtype):
    return token_ref.mha(q.to(dtype), k.to(dtype), v.to(dtype), heads)


def _att_weights(q, k, heads, img, qi, head):
    qh = q[img, qi, 128 * head:128 * head + 128].double()
    kh = k[img, :, 128 * head:128 * head + 128].double()
    return torch.softmax((kh @ qh) * (128 ** -0.5), dim=0)


def _run_dense(q, k, v, heads, dev):
    b, nq, w = q.shape
    nk = k.shape[1]
    return ops.attention_hd128(q.reshape(b * nq, w).to(dev), k.reshape(b * nk, w).to(dev), v.reshape(b * nk, w).to(dev),
                               b, nq, nk, heads).view(b, nq, w)


def _run_stacked(q, k, v, heads, dev):
    """q at column 0 of an ld = 3 w buffer; k and v at column offsets 2 w and
    3 w of an ld = 4 w buffer (the rest filled with NaN: it must not be read)."""
    b, nq, w = q.shape
    nk = k.shape[1]
    qb = torch.full((b * nq, 3 * w), float("nan"), device=dev)
    kvb = torch.full((b * nk, 4 * w), float("nan"), device=dev)
    qb[:, :w] = q.reshape(b * nq, w).to(dev)
    kvb[:, 2 * w:3 * w] = k.reshape(b * nk, w).to(dev)
    kvb[:, 3 * w:] = v.reshape(b * nk, w).to(dev)
    return ops.attention_hd128(qb[:, :w], kvb[:, 2 * w:3 * w], kvb[:, 3 * w:], b, nq, nk, heads).view(b, nq, w)


@pytest.mark.parametrize("b,nq,nk,heads", ATT_SHAPES)
def test_attention_hd128_vs_float64(cuda, b, nq, nk, heads):
    q, k, v, special = _att_case(b, nq, nk, heads)
    ref, ref32 = _att_ref(q, k, v, heads, torch.float64), _att_ref(q, k, v, heads, torch.float32)
    got = _run_dense(q, k, v, heads, cuda)
    stacked = _run_stacked(q, k, v, heads, cuda)
    assert _bits_equal(got, stacked)
    got = got.cpu()
    assert got.shape == (b, nq, heads * 128) and bool(torch.isfinite(got).all())
    # per (query, head) rows of 128
    rows = lambda t: t.reshape(b, nq, heads, 128)  # noqa: E731
    err, e32 = _row_err(rows(got), rows(ref)), _row_err(rows(ref32), rows(ref))
    bar = max(BAR, 4 * e32)
    print(f"hd128 ({b},{nq},{nk},{heads}): kernel {err:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}  (of the row norm)")
    if special:
        (zi, zq), h0, ((di, dq), dk) = special["zero_query"], special["zero_from_head"], special["dominant"]
        wd = float(_att_weights(q, k, heads, di, dq, 0)[dk])
        assert wd > 0.999
        mean_v = v[zi].double().mean(dim=0).reshape(heads, 128)[h0:]
        gz = got[zi, zq].double().reshape(heads, 128)[h0:]
        e_mean = ((gz - mean_v).abs().amax(dim=-1) / mean_v.norm(dim=-1)).max().item() if heads > h0 else 0.0
        print(f"   zero query -> mean of v rows: {e_mean:.3e}; dominant key weight {wd:.6f}")
        assert e_mean <= BAR
    assert err <= bar


@pytest.mark.parametrize("b,nq,nk,heads", [(1, 17, 17, 8), (1, 323, 323, 8), (1, 4, 1024, 8)])
def test_attention_hd128_unplanted_vs_float64(cuda, b, nq, nk, heads):
    q, k, v, _ = _att_case(b, nq, nk, heads, plant=False, gain=1.5)
    ref, ref32 = _att_ref(q, k, v, heads, torch.float64), _att_ref(q, k, v, heads, torch.float32)
    got = _run_dense(q, k, v, heads, cuda).cpu()
    rows = lambda t: t.reshape(b, nq, heads, 128)  # noqa: E731
    err, e32 = _row_err(rows(got), rows(ref)), _row_err(rows(ref32), rows(ref))
    bar = max(BAR, 4 * e32)
    top = max(float(_att_weights(q, k, heads, 0, i, h).max()) for i in range(nq) for h in range(heads))
    print(f"hd128 unplanted ({b},{nq},{nk},{heads}): kernel {err:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}; "
          f"largest attention weight {top:.4f}")
    assert top < 0.999  # no row is a one-hot
    assert err <= bar


@pytest.mark.parametrize("b,nq,nk,heads", [(3, 33, 33, 2), (2, 4, 49, 8), (1, 65, 130, 8)])
def test_attention_hd128_reruns_bit_identical(cuda, b, nq, nk, heads):
    q, k, v, _ = _att_case(b, nq, nk, heads)
    assert _bits_equal(_run_dense(q, k, v, heads, cuda), _run_dense(q, k, v, heads, cuda))


@pytest.mark.parametrize("nq,nk", [(33, 33), (4, 49), (65, 130)])
def test_attention_hd128_image_and_head_alone(cuda, nq, nk):
    """An image alone equals that image in a batch of 3; a head alone (heads =
    1 on its column slice, through the stride) equals that head among 8."""
    q, k, v, _ = _att_case(3, nq, nk, 8)
    qd, kd, vd = (t.reshape(-1, 1024).to(cuda) for t in (q, k, v))
    whole = ops.attention_hd128(qd, kd, vd, 3, nq, nk, 8).view(3, nq, 1024)
    for i in range(3):
        one = ops.attention_hd128(qd[i * nq:(i + 1) * nq], kd[i * nk:(i + 1) * nk], vd[i * nk:(i + 1) * nk], 1, nq, nk, 8)
        assert _bits_equal(one, whole[i])
    for h in (0, 5, 7):
        c = slice(128 * h, 128 * h + 128)
        one = ops.attention_hd128(qd[:, c], kd[:, c], vd[:, c], 3, nq, nk, 1).view(3, nq, 128)
        assert _bits_equal(one, whole[:, :, c])


def test_attention_hd128_at_the_key_limit(cuda):
    """nk = 65535, the most rr.h allows (1024 tiles of 64 keys, the last one 63
    deep, each wave's last tile partly or wholly past nk)."""
    nq, nk = 3, 65535
    rs = np.random.RandomState(65535)
    q = torch.from_numpy(rs.standard_normal((1, nq, 128)).astype(np.float32) * 2.0)
    k = torch.from_numpy(rs.standard_normal((1, nk, 128)).astype(np.float32) * 2.0)
    v = torch.from_numpy(rs.standard_normal((1, nk, 128)).astype(np.float32))
    got = _run_dense(q, k, v, 1, cuda).cpu()
    ref, ref32 = _att_ref(q, k, v, 1, torch.float64), _att_ref(q, k, v, 1, torch.float32)
    err, e32 = _row_err(got, ref), _row_err(ref32, ref)
    bar = max(BAR, 4 * e32)
    print(f"hd128 (1,{nq},{nk},1): kernel {err:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}")
    assert err <= bar


def test_attention_hd128_offsets_past_2_31_elements(cuda):
    """11000 images x 49 keys x 4096 columns = 2.2e9 elements: the last image's
    keys lie past 2^31 elements.  First and last image must come out as the
    same bits as the image alone."""
    b, nq, nk, ld = 11000, 4, 49, 4096
    assert (b - 1) * nk * ld > 2 ** 31
    g = torch.Generator(device=cuda).manual_seed(7)
    kv = torch.randn((b * nk, ld), device=cuda, generator=g)
    q = torch.randn((b * nq, 1024), device=cuda, generator=g)
    kk, vv = kv[:, 2048:3072], kv[:, 3072:]
    whole = ops.attention_hd128(q, kk, vv, b, nq, nk, 8).view(b, nq, 1024)
    for i in (0, b - 1):
        one = ops.attention_hd128(q[i * nq:(i + 1) * nq], kk[i * nk:(i + 1) * nk], vv[i * nk:(i + 1) * nk], 1, nq, nk, 8)
        assert bool(torch.isfinite(one).all()) and float(one.abs().max()) > 0
        assert _bits_equal(one, whole[i])
    del kv, kk, vv, whole, one
    torch.cuda.empty_cache()  # 8.8 GB back to the device for the tests that follow


def test_attention_hd128_argument_errors(cuda):
    L = _lib.lib()
    hd = _lib.handle(0)
    t = torch.zeros(8192, device=cuda)
    out = torch.full((4096,), 7.0, device=cuda)
    p, po = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(out.data_ptr())
    p4 = ctypes.c_void_p(t.data_ptr() + 4)
    f = L.rr_attention_hd128
    assert f(hd, p, 128, p, 256, p, 256, 1, 2, 2, 2, po, None) == _lib.RR_EINVAL    # ldq < heads * 128
    assert f(hd, p, 256, p, 128, p, 256, 1, 2, 2, 2, po, None) == _lib.RR_EINVAL    # ldk
    assert f(hd, p, 256, p, 256, p, 255, 1, 2, 2, 2, po, None) == _lib.RR_EINVAL    # ldv
    assert f(hd, p, 130, p, 128, p, 128, 1, 2, 2, 1, po, None) == _lib.RR_EINVAL    # ld % 4
    assert f(hd, p4, 128, p, 128, p, 128, 1, 2, 2, 1, po, None) == _lib.RR_EINVAL   # misaligned q
    assert f(hd, p, 128, p, 128, p4, 128, 1, 2, 2, 1, po, None) == _lib.RR_EINVAL   # misaligned v
    assert f(hd, p, 128, p, 128, p, 128, 1, 2, 2, 1, ctypes.c_void_p(out.data_ptr() + 4), None) == _lib.RR_EINVAL
    assert f(hd, p, 128, p, 128, p, 128, 1, 0, 2, 1, po, None) == _lib.RR_EINVAL    # nq = 0
    assert f(hd, p, 128, p, 128, p, 128, 1, 2, 65536, 1, po, None) == _lib.RR_EINVAL
    assert f(hd, p, 128, p, 128, p, 128, 1, 2, 2, 0, po, None) == _lib.RR_EINVAL    # heads = 0
    assert f(hd, None, 128, p, 128, p, 128, 1, 2, 2, 1, po, None) == _lib.RR_EINVAL
    assert b"rr_attention_hd128" in L.rr_last_error(hd)
    assert f(hd, p, 128, p, 128, p, 128, 0, 2, 2, 1, po, None) == _lib.RR_OK        # b = 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # out untouched
    z = torch.zeros((4, 128), device=cuda)
    with pytest.raises(ValueError):
        ops.attention_hd128(z, z, z, 1, 4, 4, 2)          # width does not fit heads
    with pytest.raises(ValueError):
        ops.attention_hd128(z.t(), z, z, 1, 4, 4, 1)      # columns not contiguous
    with pytest.raises(ValueError):
        ops.attention_hd128(z, z, z, 1, 0, 4, 1)
    assert ops.attention_hd128(z[:0], z[:0], z[:0], 0, 4, 4, 1).shape == (0, 128)


# ---- rr_token_pool ---------------------------------------------------------
POOL_SHAPES = [(1, 1, 256, 1), (2, 15, 256, 4), (3, 49, 1024, 4), (64, 49, 1024, 4), (1, 1024, 1024, 4),
               (1, 4096, 1024, 4), (2, 323, 768, 8)]


def _pool_case(b, hw, c, n_obj):
    """x = N(0,1), query = N(0, 4/c) (logits N(0, 2^2)).  Planted where n_obj >=
    4: query rows 0 and 1 identical (equal weights, bit-equal output rows), row
    3 = -row 2, and one position along row 2 whose logits are +100 and -100."""
    rs = np.random.RandomState(10000 * b + hw + c + n_obj)
    x = rs.standard_normal((b, hw, c)).astype(np.float32)
    qy = (rs.standard_normal((n_obj, c)) * (2.0 / np.sqrt(c))).astype(np.float32)
    planted = n_obj >= 4
    if planted:
        qy[1] = qy[0]
        qy[3] = -qy[2]
        x[b - 1, hw // 2] = qy[2] * np.float32(100.0 / float(np.dot(qy[2].astype(np.float64), qy[2])))
    return torch.from_numpy(x), torch.from_numpy(qy), planted


def _pool_ref(x, qy, dtype):
    x, qy = x.to(dtype), qy.to(dtype)
    a = torch.softmax(torch.matmul(qy, x.permute(0, 2, 1)), dim=1)
    return a, torch.bmm(a, x)


@pytest.mark.parametrize("b,hw,c,n_obj", POOL_SHAPES)
def test_token_pool_vs_float64(cuda, b, hw, c, n_obj):
    x, qy, planted = _pool_case(b, hw, c, n_obj)
    (a, ref), (_, ref32) = _pool_ref(x, qy, torch.float64), _pool_ref(x, qy, torch.float32)
    xd, qd = x.to(cuda), qy.to(cuda)
    got = ops.token_pool(xd, qd)
    assert got.shape == (b, n_obj, c)
    assert _bits_equal(got, ops.token_pool(xd, qd))  # reruns
    got = got.cpu()
    err, e32 = _row_err(got, ref), _row_err(ref32, ref)
    bar = max(BAR, 4 * e32)
    print(f"token_pool ({b},{hw},{c},{n_obj}): kernel {err:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}")
    if planted:
        assert _bits_equal(got[:, 0], got[:, 1])
        wp = a[b - 1, :, hw // 2]
        print(f"   planted position's weights {wp.tolist()}")
        assert float(wp[2]) > 0.999 and float(wp[3]) < 1e-80
    assert err <= bar


@pytest.mark.parametrize("hw,c,n_obj", [(49, 1024, 4), (323, 768, 8), (15, 256, 4)])
def test_token_pool_image_alone_equals_image_in_batch(cuda, hw, c, n_obj):
    """The position split is a function of (b, hw); at these sizes b = 1 and
    b = 3 choose the same one."""
    x, qy, _ = _pool_case(3, hw, c, n_obj)
    xd, qd = x.to(cuda), qy.to(cuda)
    whole = ops.token_pool(xd, qd)
    for i in range(3):
        assert _bits_equal(ops.token_pool(xd[i:i + 1].contiguous(), qd)[0], whole[i])
    maps = ops.token_pool(xd.reshape(3, 1, hw, c), qd)
    assert _bits_equal(maps, whole)


def test_token_pool_argument_errors(cuda):
    L = _lib.lib()
    hd = _lib.handle(0)
    t = torch.zeros(16384, device=cuda)
    out = torch.full((8192,), 7.0, device=cuda)
    p, po = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(out.data_ptr())
    p4 = ctypes.c_void_p(t.data_ptr() + 4)
    f = L.rr_token_pool
    assert f(hd, p, 1, 1, 100, p, 1, po, None) == _lib.RR_EINVAL
    assert f(hd, p, 1, 1, 128, p, 1, po, None) == _lib.RR_EINVAL
    assert f(hd, p, 1, 1, 1280, p, 1, po, None) == _lib.RR_EINVAL   # c > 1024
    assert f(hd, p, 1, 1, 256, p, 0, po, None) == _lib.RR_EINVAL
    assert f(hd, p, 1, 1, 256, p, 9, po, None) == _lib.RR_EINVAL    # n_obj > 8
    assert f(hd, p, 1, 0, 256, p, 1, po, None) == _lib.RR_EINVAL    # hw = 0
    assert f(hd, p, -1, 1, 256, p, 1, po, None) == _lib.RR_EINVAL
    assert f(hd, p4, 1, 1, 256, p, 1, po, None) == _lib.RR_EINVAL
    assert f(hd, p, 1, 1, 256, p4, 1, po, None) == _lib.RR_EINVAL
    assert f(hd, p, 1, 1, 256, p, 1, ctypes.c_void_p(out.data_ptr() + 4), None) == _lib.RR_EINVAL
    assert f(hd, None, 1, 1, 256, p, 1, po, None) == _lib.RR_EINVAL
    assert b"rr_token_pool" in L.rr_last_error(hd)
    assert f(hd, p, 0, 4, 256, p, 1, po, None) == _lib.RR_OK
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError):
        ops.token_pool(torch.zeros((1, 4, 300), device=cuda), torch.zeros((4, 300), device=cuda))
    with pytest.raises(ValueError):
        ops.token_pool(torch.zeros((1, 4, 256), device=cuda), torch.zeros((9, 256), device=cuda))
    with pytest.raises(ValueError):
        ops.token_pool(torch.zeros((1, 4, 256), device=cuda), torch.zeros((4, 512), device=cuda))


# ---- rr_gelu ---------------------------------------------------------------
SPECIAL = [0.0, -0.0, 1e-8, -1e-8, 6.0, -6.0, 40.0, -40.0, float("inf"), float("-inf"), float("nan")]


@pytest.mark.parametrize("n", [1, 3, 255, 2048 * 4, 2 ** 20 + 1])
def test_gelu_vs_float64(cuda, n):
    """N(0, 3) values; per element max(1e-6 max(1, |ref|), 4 |torch float32
    gelu - float64|).  Out of place and in place give the same bits."""
    rs = np.random.RandomState(n)
    x = torch.from_numpy((rs.standard_normal(n) * 3.0).astype(np.float32))
    ref = torch.nn.functional.gelu(x.double())
    t32 = torch.nn.functional.gelu(x)
    xd = x.to(cuda)
    got = ops.gelu(xd)
    assert torch.equal(xd.cpu(), x)  # the input is left alone
    inplace = xd.clone()
    assert ops.gelu(inplace, out=inplace) is inplace
    assert _bits_equal(got, inplace)
    bar = torch.maximum(1e-6 * ref.abs().clamp(min=1.0), 4 * (t32.double() - ref).abs())
    err = (got.cpu().double() - ref).abs()
    print(f"gelu n={n}: max err {err.max().item():.3e}; torch float32 {(t32.double() - ref).abs().max().item():.3e}")
    assert bool((err <= bar).all())


def test_gelu_special_values(cuda):
    x = torch.tensor(SPECIAL, dtype=torch.float32)
    got = ops.gelu(x.to(cuda)).cpu()
    ref = torch.nn.functional.gelu(x.double())
    print("gelu specials:", dict(zip(SPECIAL, got.tolist())), "; torch float64:", ref.tolist())
    assert bool(torch.isnan(got[10]))                                   # NaN stays NaN
    assert float(got[8]) == float("inf")                                # +inf -> +inf
    assert float(got[9]) == 0.0 and bool(torch.signbit(got[9]))         # -inf -> -0 (the limit; never NaN)
    assert float(got[0]) == 0.0 and not bool(torch.signbit(got[0]))
    assert float(got[1]) == 0.0 and bool(torch.signbit(got[1]))
    fin = [2, 3, 4, 5, 6, 7]
    err = (got[fin].double() - ref[fin]).abs()
    assert bool((err <= 1e-6 * ref[fin].abs().clamp(min=1.0)).all())
    assert float(got[6]) == 40.0 and float(got[7]) == 0.0
    L = _lib.lib()
    hd = _lib.handle(0)
    assert L.rr_gelu(hd, None, 4, None, None) == _lib.RR_EINVAL
    t = torch.zeros(4, device=cuda)
    assert L.rr_gelu(hd, ctypes.c_void_p(t.data_ptr()), -1, ctypes.c_void_p(t.data_ptr()), None) == _lib.RR_EINVAL
    assert L.rr_gelu(hd, ctypes.c_void_p(t.data_ptr()), 0, ctypes.c_void_p(t.data_ptr()), None) == _lib.RR_OK


# ---- networks.Token --------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "token.npz"))


@pytest.fixture(scope="module")
def sd(fx):
    """One reference-keyed checkpoint: backbone.* in ResNet_DOLG layout (stride
    on the 1x1) + the tr.* head."""
    d = {"backbone." + k: v
         for k, v in W.to_dolg_keys(W.synthetic_resnet_state_dict("resnet101", int(fx["weight_seed"]))).items()}
    d.update(W.synthetic_token_head(int(fx["head_seed"])))
    return d


@pytest.fixture(scope="module")
def nets(sd):
    made = {}

    def get(conv_math):
        if conv_math not in made:
            made[conv_math] = Token(state_dict=sd, device="cuda:0", conv_math=conv_math, stride_on="1x1")
        return made[conv_math]
    return get


@pytest.fixture(scope="module")
def head_refs(fx):
    """float64 and float32 restatements of the head-only cases, computed once."""
    head = W.token_head_from_state_dict(W.synthetic_token_head(int(fx["head_seed"])))
    out = {}
    for c in HEAD_CASES:
        x = torch.from_numpy(I.feature_map(9000 + c[1] * c[2], c[0], 2048, c[1], c[2]))
        out[c] = (x, token_ref.head_forward(x, head, torch.float64), token_ref.head_forward(x, head, torch.float32))
    return out


@pytest.mark.parametrize("case", HEAD_CASES)
def test_token_head_vs_reference(cuda, fx, nets, head_refs, case):
    """Token_Refine + F.normalize alone on maps where every piece matters
    (test_token_host.py: each degenerate piece moves these descriptors by >=
    100 x this bar).  Measured on the MI355X: see DESIGN.md, "Token head"."""
    b, h, w = case
    tag = f"head_b{b}_{h}x{w}"
    x4, r64, r32 = head_refs[case]
    d32 = (r32["out"].double() - r64["out"]).abs().max().item()
    bar = max(2e-6, 4 * d32)
    x = x4.permute(0, 2, 3, 1).contiguous().to(cuda)
    for cm in ("f32", "h2"):
        net = nets(cm)
        taps = {}
        got = net.tail(net.tr(x, taps=taps)).cpu()
        err = np.abs(got.numpy() - fx[tag + "_out"]).max()
        e64 = (got.double() - r64["out"]).abs().max().item()
        print(f"Token {tag} {cm}: descriptor max|err| vs the reference {err:.3e}, vs float64 {e64:.3e}; float32 "
              f"restatement vs float64 {d32:.3e}; bar {bar:.3e}")
        rows = {}
        for k in ("X", "T0", "tn", "dec0", "dec1"):
            e32k = _row_err(r32[k], r64[k])
            rows[k] = (_row_err(taps[k].cpu(), r64[k]), max(BAR, 4 * e32k))
            stored = f"{tag}_{k}"
            if stored in fx.files:
                es = _row_err(taps[k].cpu(), torch.from_numpy(fx[stored]))
                print(f"   {k}: vs the stored reference {es:.3e}, vs float64 {rows[k][0]:.3e}, bar {rows[k][1]:.3e}")
                assert es <= rows[k][1], k
            else:
                print(f"   {k}: vs float64 {rows[k][0]:.3e}, bar {rows[k][1]:.3e}")
        assert got.shape == (b, 1024)
        assert err <= bar
        if case == (1, 5, 9):
            for k, (e, kb) in rows.items():
                assert e <= kb, k


def _e2e_err(net, fx, tag):
    seed, b, h, w = (int(v) for v in fx[tag + "_case"])
    got = net.forward_test(I.trunk_input(seed, b, h, w).to("cuda:0")).cpu().numpy()
    assert got.shape == (b, 1024) == (b, net.outputdim) and net.meta == {"outputdim": 1024}
    return np.abs(got - fx[tag + "_out"]).max()


@pytest.mark.parametrize("tag", ["b2_224", "b1_odd"])
def test_token_vs_reference(cuda, fx, nets, tag):
    """End to end (wiring).  The bar's float32 term comes from the head
    restatement on the reference trunk's saved x4."""
    tr = np.load(os.path.join(GOLD, "resnet_dolg.npz"))
    head = W.token_head_from_state_dict(W.synthetic_token_head(int(fx["head_seed"])))
    x4 = torch.from_numpy(tr[tag + "_x4"])
    d32 = (token_ref.head_forward(x4, head, torch.float32)["out"].double() -
           token_ref.head_forward(x4, head, torch.float64)["out"]).abs().max().item()
    bar = max(2e-6, 4 * d32)
    e32 = _e2e_err(nets("f32"), fx, tag)
    eh2 = _e2e_err(nets("h2"), fx, tag)
    print(f"Token {tag}: descriptor max|err| f32 {e32:.3e}  h2 {eh2:.3e}; float32 restatement vs float64 {d32:.3e}; "
          f"bar {bar:.3e}")
    assert e32 <= bar
    assert eh2 <= bar


def test_retrievalnet_same_bits_as_token(cuda, sd, nets):
    net = RetrievalNet(1000, state_dict=sd, device="cuda:0", conv_math="h2", stride_on="1x1")
    assert net.outputdim == 1024 and net.meta == {"outputdim": 1024}
    x = I.trunk_input(91, 2, 96, 128).to(cuda)
    assert _bits_equal(net.forward_test(x), nets("h2").forward_test(x))


def test_token_entry_points_agree(cuda, nets):
    """forward_test == forward_test_u8 == extract_vectors (batches of 2,
    multi-scale) on 4 images of 96 x 128."""
    net = nets("h2")
    rs = np.random.RandomState(17)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(4, 96, 128, 3), dtype=np.uint8))
    x = ops.preprocess_u8(imgs.to(cuda))
    a = net.forward_test(x.permute(0, 3, 1, 2).contiguous())
    assert a.shape == (4, 1024)
    assert _bits_equal(a, net.forward_test_u8(imgs.to(cuda)))
    assert _bits_equal(extract_vectors(net, [imgs[:2], imgs[2:]], ms=[1], device=cuda, print_freq=0).to(cuda),
                       torch.cat([net.forward_test_u8(imgs[:2].to(cuda)), net.forward_test_u8(imgs[2:].to(cuda))]))
    ms = [1, 2 ** -0.5, 0.5]
    got = extract_vectors(net, [imgs[:2], imgs[2:]], ms=ms, device=cuda, print_freq=0)
    parts = []
    for batch in (imgs[:2], imgs[2:]):
        xb = ops.preprocess_u8(batch.to(cuda))
        acc = None
        for s in ms:
            xs = xb if s == 1 else ops.resize_bilinear(xb, int(96 * s), int(128 * s), scale_factor=s)
            f = net.forward_test_nhwc(xs)
            acc = f.clone() if acc is None else acc.add_(f)
        acc.div_(len(ms))
        parts.append(ops.l2_normalize(acc, 1e-12).cpu())
    assert got.shape == (4, 1024)
    assert _bits_equal(got.cpu(), torch.cat(parts))
    # batch-1 variable size
    one = extract_vectors(net, [imgs[:1, :64, :96]], ms=[1], device=cuda, print_freq=0)
    assert one.shape == (1, 1024) and abs(float(one.norm()) - 1.0) < 1e-5


def test_token_image_alone_equals_image_in_batch_f32(cuda, nets):
    net = nets("f32")
    rs = np.random.RandomState(29)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(3, 96, 128, 3), dtype=np.uint8)).to(cuda)
    whole = net.forward_test_u8(imgs)
    for i in range(3):
        assert _bits_equal(net.forward_test_u8(imgs[i:i + 1])[0], whole[i])


def test_gempcaw_on_token(cuda, nets):
    net = nets("h2")
    pw = ConvDimReduction(1024, 256, device=cuda)
    w, b = W.synthetic_linear(256, 1024, 8, scale=1.0 / np.sqrt(1024))
    pw.set_params(w, b)
    ext = GeMPCAw(net, pw)
    rs = np.random.RandomState(31)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(2, 96, 128, 3), dtype=np.uint8)).to(cuda)
    f = ext.forward_test_u8(imgs)
    assert f.shape == (2, 256) == (2, ext.outputdim)
    assert bool(((f.double().norm(dim=1) - 1.0).abs() < 1e-5).all())
