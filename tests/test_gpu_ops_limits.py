"""The row and pointwise kernels at the limits include/rr.h documents and at
every size where they take another path, against float64 torch of the same
operation (kernels that only move data: torch.equal).  tests/test_gpu_ops.py
and tests/test_gpu_vit.py run each of them at one shape:

* layernorm_kernel's four PER_LANE instances (4, 12, 16, 64 registers per lane,
  d <= 256 / 768 / 1024 / 4096) and the two vectorised ones (d = 512, 768 on
  16-B aligned rows), fp32 and bf16 output, and the fused token assembly's;
* alpha_qe_kernel past one wave's worth of columns (d = 1024: all 256 threads;
  1028 and 2048: a second trip of the column loop);
* the grid-stride step of gem / resize / nchw_to_nhwc / preprocess_u8 (grids
  are capped at 4096 x 256 threads = 1,048,576);
* l2norm_kernel at d below, at and above one wave and at the documented eps.

Tolerances are those of the existing test of each op."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from research_image_retrieval_amd import _lib, ops

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- B1: LayerNorm -----------------------------------------------------------

def _ln_data(d, rows=5, seed=0):
    g = _gen(1000 + d + seed)
    x = torch.randn(rows, d, generator=g) * 2.0 + 0.5  # a mean the first pass has to remove
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g)
    ref = F.layer_norm(x.double(), (d,), w.double(), b.double(), 1e-5)
    return x, w, b, ref


def _assert_bf16_within_one_ulp(got_bf16, want_f32):
    """got (bf16) equals want rounded to bf16, up to one bf16 ulp (8 significand
    bits: ulp = 2^(e - 7) for |x| in [2^e, 2^(e+1)))."""
    a, b = got_bf16.float(), want_f32.to(torch.bfloat16).float()
    _, e = torch.frexp(torch.maximum(a.abs(), b.abs()))  # |x| = m 2^e, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(a), e - 8)
    bad = (a - b).abs() > ulp
    assert not bool(bad.any()), ((a - b).abs() / ulp).max().item()


@pytest.mark.parametrize("d", [1, 63, 200, 257, 512, 768, 769, 1024, 1025, 2048, 4096])
def test_layernorm_every_instance(cuda, d):
    """d -> kernel (launch_ln in csrc/vit_ops.hip): 1, 63, 200: PER_LANE 4;
    257: 12; 769, 1024: 16; 1025, 2048, 4096 (rr.h's maximum): 64; 512 and
    768 on aligned rows: layernorm_vec_kernel<2> / <3>.  d = 1 has variance 0:
    the output is beta."""
    x, w, b, ref = _ln_data(d)
    out = ops.layernorm(x.to(cuda), w.to(cuda), b.to(cuda)).cpu()
    print(f"layernorm d={d}: max |err| {(out.double() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(out, ref.float(), rtol=1e-5, atol=1e-5)
    if d == 1:
        assert torch.equal(out, b.expand(5, 1))


def test_layernorm_unaligned_stride_takes_generic_instance(cuda):
    """d = 768 with a row stride of 769 floats (not a multiple of 4): launch_ln
    leaves the vectorised kernel for layernorm_kernel<12>.  Same tolerance
    against float64; against the vectorised run of the same rows only that
    tolerance (the two sum in different orders)."""
    d, rows, ld = 768, 5, 769
    g = _gen(7)
    buf = torch.randn(rows * ld, generator=g) * 2.0 + 0.5
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g)
    x = torch.stack([buf[r * ld:r * ld + d] for r in range(rows)])
    ref = F.layer_norm(x.double(), (d,), w.double(), b.double(), 1e-5).float()
    bufd = torch.zeros(rows + 1, d, device=cuda)  # (rows + 1) d >= rows ld floats; row r starts at float r ld
    bufd.view(-1)[:rows * ld] = buf.to(cuda)
    strided = ops.layernorm(bufd, w.to(cuda), b.to(cuda), rows=rows, row_stride=ld).cpu()
    dense = ops.layernorm(x.to(cuda), w.to(cuda), b.to(cuda)).cpu()
    torch.testing.assert_close(strided, ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dense, ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(strided, dense, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("d", [200, 768, 4096])
def test_layernorm_bf16_output(cuda, d):
    """rr_layernorm_ex out_dtype 1 (generic instances 4 and 64, vectorised
    768): the fp32 output rounded to bf16, up to one bf16 ulp (the two
    template instances may contract the last multiply-add differently); the
    fp32 output itself is within the fp32 tolerance of float64."""
    x, w, b, ref = _ln_data(d, seed=1)
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    out32 = ops.layernorm(xd, wd, bd).cpu()
    out16 = ops.layernorm_bf16(xd, wd, bd).cpu()
    assert out16.dtype == torch.bfloat16 and out16.shape == (5, d)
    torch.testing.assert_close(out32, ref.float(), rtol=1e-5, atol=1e-5)
    _assert_bf16_within_one_ulp(out16, out32)


@pytest.mark.parametrize("width", [1000, 4096])
def test_vit_tokens_ln_fused_wide(cuda, width):
    """The fused token assembly's PER_LANE 16 (width 1000) and 64 (4096, the
    maximum) instances: bit-identical to vit_tokens followed by layernorm, as
    tests/test_gpu_vit.py::test_vit_tokens_ln_pre_fused asserts for widths up
    to 768, and within 1e-5 of float64."""
    b, npatch = 2, 3
    g = _gen(width)
    pt = torch.randn(b * npatch, width, generator=g)
    cls, pos = torch.randn(width, generator=g), torch.randn(npatch + 1, width, generator=g)
    gm, bt = torch.randn(width, generator=g), torch.randn(width, generator=g)
    d = [t.to(cuda) for t in (pt, cls, pos, gm, bt)]
    plain = ops.vit_tokens(d[0], b, d[1], d[2])
    fused = ops.vit_tokens(d[0], b, d[1], d[2], ln=(d[3], d[4]))
    two = ops.layernorm(plain, d[3], d[4])
    assert torch.equal(fused.cpu(), two.cpu())
    tok = torch.cat([cls.expand(b, 1, width), pt.view(b, npatch, width)], 1) + pos
    assert torch.equal(plain.cpu(), tok.reshape(-1, width))
    ref = F.layer_norm(tok.double(), (width,), gm.double(), bt.double(), 1e-5).float()
    torch.testing.assert_close(fused.cpu(), ref.reshape(-1, width), rtol=1e-5, atol=1e-5)


def test_layernorm_rejects_rows_wider_than_4096(cuda):
    """rr.h: d <= 4096 (a lane holds at most 64 elements): 4097 is RR_EINVAL
    for rr_layernorm, rr_layernorm_ex and the fused rr_vit_tokens_ex, which
    still assembles tokens of that width without the LayerNorm."""
    d = 4097
    L, h = _lib.lib(), _lib.handle(cuda.index)
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    x = torch.randn(2 * 4, d, device=cuda)
    w, b = torch.randn(d, device=cuda), torch.randn(d, device=cuda)
    y = torch.full((2 * 5, d), 7.0, device=cuda)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.rr_layernorm(h, p(x), d, 2, d, p(w), p(b), 1e-5, p(y), st) == _lib.RR_EINVAL
    assert b"d <= 4096" in L.rr_last_error(h)
    assert L.rr_layernorm_ex(h, p(x), d, 2, d, p(w), p(b), 1e-5, 1, p(y), st) == _lib.RR_EINVAL
    pos = torch.randn(5, d, device=cuda)
    assert L.rr_vit_tokens_ex(h, p(x), 2, 4, d, p(w), p(pos), p(w), p(b), 1e-5, p(y), st) == _lib.RR_EINVAL
    assert b"width <= 4096" in L.rr_last_error(h)
    assert bool((y == 7.0).all())  # nothing was launched
    assert L.rr_vit_tokens_ex(h, p(x), 2, 4, d, p(w), p(pos), None, None, 0.0, p(y), st) == _lib.RR_OK
    tok = torch.cat([w.expand(2, 1, d), x.view(2, 4, d)], 1) + pos
    assert torch.equal(y, tok.reshape(-1, d))


# ---- B2: alpha-QE --------------------------------------------------------------

def _qe_data(d, nq=3, n_rows=500, k=10):
    rs = np.random.RandomState(200 + d)
    g = rs.standard_normal((n_rows, d)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    q = rs.standard_normal((nq, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    s, i = oracle.cosine_topk(q, g, k)
    return q, g, s, i


def _qe(cuda, q, g, i, s, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    return ops.alpha_qe(t(q), t(g), t(i), t(s), **kw).cpu().numpy()


@pytest.mark.parametrize("d", [4, 1024, 1028, 2048])
def test_alpha_qe_widths(cuda, d):
    """d = 4: one float4, one thread; 1024: every thread of the block once;
    1028: thread 0 alone takes a second trip; 2048 (C5's): every thread takes
    two.  Against oracle.alpha_qe (float64 accumulation) at the existing
    test's atol 2e-6."""
    q, g, s, i = _qe_data(d)
    out = _qe(cuda, q, g, i, s, n=5, alpha=3.0)
    ref = oracle.alpha_qe(q, g, i, s, n=5, alpha=3.0)
    np.testing.assert_allclose(out, ref, rtol=0, atol=2e-6)
    np.testing.assert_allclose(np.linalg.norm(out.astype(np.float64), axis=1), 1.0, rtol=0, atol=1e-6)


def test_alpha_qe_edges_at_2048(cuda):
    """n = 0 and a list without a positive score give the normalised query;
    n = k uses the whole list; alpha = 0 weighs every positive score 1."""
    q, g, s, i = _qe_data(2048)
    q = q * np.float32(2.5)  # not unit norm: the final normalisation has work to do
    qn = (q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    np.testing.assert_allclose(_qe(cuda, q, g, i, s, n=0, alpha=3.0), qn, rtol=0, atol=2e-6)
    np.testing.assert_allclose(_qe(cuda, q, g, i, s, n=10, alpha=3.0), oracle.alpha_qe(q, g, i, s, n=10, alpha=3.0),
                               rtol=0, atol=2e-6)
    assert (s > 0).all()  # top-10 of 500 random unit rows: alpha = 0 then weighs each row 1
    ref0 = q.astype(np.float64) + g[i[:, :4]].astype(np.float64).sum(1)
    ref0 /= np.linalg.norm(ref0, axis=1, keepdims=True)
    out0 = _qe(cuda, q, g, i, s, n=4, alpha=0.0)
    np.testing.assert_allclose(out0, ref0.astype(np.float32), rtol=0, atol=2e-6)
    np.testing.assert_allclose(out0, oracle.alpha_qe(q, g, i, s, n=4, alpha=0.0), rtol=0, atol=2e-6)
    s_neg = -np.abs(s)
    s_neg[:, 0] = 0.0
    s_neg[:, 1] = -0.0
    np.testing.assert_allclose(_qe(cuda, q, g, i, s_neg, n=10, alpha=3.0), qn, rtol=0, atol=2e-6)


# ---- B3: GeM ---------------------------------------------------------------------

def _gem_ref(x, p, eps):
    return x.double().clamp(min=eps).pow(p).mean(dim=1).pow(1.0 / p)


@pytest.mark.parametrize("p", [3.0, 2.5])
@pytest.mark.parametrize("b,hw,c", [(520, 2, 2048), (3, 1, 2048), (3, 1024, 8)])
def test_gem_shapes(cuda, p, b, hw, c):
    """[520, 2, 2048]: b x c = 1,064,960 outputs, past the 1,048,576 threads
    of the capped grid, so the last 16,384 are second trips of the grid-stride
    loop; hw = 1; hw = 1024 (a 1024-term fp32 sum per output).  Channels 1 and
    c - 1 lie entirely below eps: the clamp decides them, and the output there
    is eps itself."""
    eps = 1e-6
    x = torch.randn(b, hw, c, generator=_gen(b + hw + c))
    x[:, :, 1] = -x[:, :, 1].abs()
    x[:, :, c - 1] = 3e-7
    ref = _gem_ref(x, p, eps)
    out = ops.gem_pool(x.to(cuda), p, eps).cpu()
    assert out.shape == (b, c)
    rel = ((out.double() - ref).abs() / ref).max().item()
    print(f"gem p={p} [{b},{hw},{c}]: max rel err {rel:.3e}")
    torch.testing.assert_close(out, ref.float(), rtol=2e-6, atol=1e-7)
    # The clamped channels are ~1e-6, where atol 1e-7 alone would allow 10 %.
    # (eps^p)^(1/p) in fp32: |ln eps^p| <= 42, times the 2^-24 rounding of 1 / p,
    # is 2.5e-6 relative, plus a few ulp (6e-8 each) of the two powf: within 4e-6.
    for ch in (1, c - 1):
        assert bool(((out[:, ch].double() - eps).abs() <= 4e-6 * eps).all()), out[:, ch]


# ---- B4: L2 normalise -------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 4, 63, 64, 65, 2048])
def test_l2_normalize_widths_and_eps(cuda, d):
    """One wave per row, lanes striding by 64: d below, at and one past the
    wave, and 2048.  eps = 1e-3: an all-zero row stays exactly 0, a row whose
    norm is below eps is divided by eps (F.normalize semantics).  m = 1 and m =
    1000 (250 blocks), out of place and in place."""
    eps = 1e-3
    g = _gen(300 + d)
    for m in (1, 1000):
        x = torch.randn(m, d, generator=g)
        if m > 2:
            x[0] = 0.0
            x[1] = 1e-5 * torch.randn(d, generator=g)  # norm ~ 1e-5 sqrt(d) <= 5e-4
            assert x[1].double().norm().item() < eps
        ref = x.double() / x.double().norm(dim=1, keepdim=True).clamp_min(eps)
        xd = x.to(cuda)
        out = ops.l2_normalize(xd, eps)
        assert torch.equal(xd.cpu(), x)  # the input is left alone
        torch.testing.assert_close(out.cpu(), ref.float(), rtol=1e-5, atol=1e-6)
        same = ops.l2_normalize(xd, eps, out=xd)
        assert same.data_ptr() == xd.data_ptr() and torch.equal(xd.cpu(), out.cpu())
        if m > 2:
            assert bool((out[0] == 0).all())
            torch.testing.assert_close(out[1].cpu(), (x[1].double() / eps).float(), rtol=1e-5, atol=1e-6)


# ---- B5: bilinear resize ----------------------------------------------------------

def _resize_ref(x_nhwc, oh, ow):
    return F.interpolate(x_nhwc.permute(0, 3, 1, 2).double(), size=(oh, ow), mode="bilinear",
                         align_corners=False).permute(0, 2, 3, 1)


def test_resize_past_one_grid(cuda):
    """2 x 37 x 41 x 3 -> 420 x 440: 1,108,800 outputs, 60,224 of them second
    trips of the grid-stride loop; the size is given without a scale factor,
    so the source index uses in / out."""
    x = torch.randn(2, 37, 41, 3, generator=_gen(41))
    ref = _resize_ref(x, 420, 440)
    out = ops.resize_bilinear(x.to(cuda), 420, 440).cpu()
    err = (out.double() - ref).abs()
    print(f"resize 37x41 -> 420x440: max |err| {err.max().item():.3e}, "
          f"over the bar by {(err - (1e-5 + 1e-5 * ref.abs())).max().item():.3e}")
    torch.testing.assert_close(out, ref.float(), rtol=1e-5, atol=1e-5)


def test_resize_identity_and_degenerate_inputs(cuda):
    """Same size in and out: every source index is an integer and the output
    is the input, bit for bit.  A 1 x 1 input and a 1-row input clamp the
    second tap onto the first (h1 = h0 at the last row)."""
    x = torch.randn(2, 9, 11, 5, generator=_gen(9))
    assert torch.equal(ops.resize_bilinear(x.to(cuda), 9, 11).cpu(), x)
    one = torch.randn(2, 1, 1, 3, generator=_gen(1))
    out = ops.resize_bilinear(one.to(cuda), 4, 7).cpu()
    torch.testing.assert_close(out, one.expand(2, 4, 7, 3), rtol=1e-5, atol=1e-5)  # v lw0 + v lw1 may round
    row = torch.randn(1, 1, 6, 4, generator=_gen(6))
    for oh, ow in ((3, 13), (1, 4), (2, 6)):
        out = ops.resize_bilinear(row.to(cuda), oh, ow).cpu()
        torch.testing.assert_close(out, _resize_ref(row, oh, ow).float(), rtol=1e-5, atol=1e-5)


# ---- B6: relayout and preprocess past one grid ---------------------------------------

def test_nchw_to_nhwc_past_one_grid(cuda):
    """[2, 3, 500, 400]: 1.2 M outputs (1.6 M padded to four channels)."""
    x = torch.randn(2, 3, 500, 400, generator=_gen(500))
    xd = x.to(cuda)
    assert torch.equal(ops.nchw_to_nhwc(xd).cpu(), x.permute(0, 2, 3, 1))
    y4 = ops.nchw_to_nhwc(xd, out_c=4).cpu()
    assert torch.equal(y4[..., :3], x.permute(0, 2, 3, 1)) and bool((y4[..., 3] == 0).all())


def test_preprocess_u8_past_one_grid(cuda):
    """[2, 800, 700, 3]: 1.12 M pixels, one thread each."""
    rng = np.random.RandomState(800)
    t = torch.from_numpy(rng.randint(0, 256, size=(2, 800, 700, 3), dtype=np.uint8))
    mean = torch.tensor([0.485, 0.456, 0.406])
    std = torch.tensor([0.229, 0.224, 0.225])
    ref = (t.float().div(255) - mean) / std  # ToTensor + Normalize (HWC view)
    a = ops.preprocess_u8(t.to(cuda)).cpu()
    assert torch.equal(a, ref)
    b4 = ops.preprocess_u8(t.to(cuda), out_c=4).cpu()
    assert torch.equal(b4[..., :3], ref) and bool((b4[..., 3] == 0).all())
