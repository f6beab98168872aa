"""Every template instance of the three fused attention kernels
(csrc/vit_ops.hip: rr_attention_ex, rr_attention_bf16, rr_attention_bf16_qkv16)
against float64 softmax(q k^T / 8) v per head on the CPU.

Each entry dispatches on NC = ceil(seq / 32) to one of eight instances, times
two output types.  test_gpu_vit.py runs NC = 1, 2, 7 and 8 on randn inputs,
never a seq that is a multiple of 32 (no masked key, no padded query lane),
never seq = 1, and the bf16 kernels only with bf16 output.  Here every
instance runs at both ends of its seq range with both output types, on peaked
rows (logits of +-100 next to the -inf mask), inside guarded buffers, and with
a NaN planted in one head.

b = 2 and heads = 3 throughout: blockIdx -> (image, head) uses both the
division and the remainder.  The entries are called through ctypes: ops.py has
no wrapper for the bf16 kernels' fp32 output."""
import ctypes
import functools

import pytest
import torch

from research_image_retrieval_amd import _lib

pytestmark = pytest.mark.gpu

B, HEADS, HD = 2, 3, 64
WIDTH = HEADS * HD
ENTRIES = ("rr_attention_ex", "rr_attention_bf16", "rr_attention_bf16_qkv16")
PAIRS = [(e, od) for e in ENTRIES for od in (0, 1)]
SEQS = [1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _rc(entry, qkv, b, seq, heads, head_dim, out_dtype, out):
    """The raw C call: the return code, nothing raised."""
    dev = out.device
    return getattr(_lib.lib(), entry)(_lib.handle(dev.index), _p(qkv), b, seq, heads, head_dim, out_dtype, _p(out),
                                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))


def _run(entry, qkv, seq, out_dtype, out=None):
    """qkv: fp32 device rows (bf16 rows for the qkv16 entry); returns out."""
    assert qkv.dtype == (torch.bfloat16 if entry.endswith("qkv16") else torch.float32) and qkv.is_contiguous()
    if out is None:
        out = torch.empty(B * seq, WIDTH, dtype=torch.bfloat16 if out_dtype else torch.float32, device=qkv.device)
    rc = _rc(entry, qkv, B, seq, HEADS, HD, out_dtype, out)
    assert rc == _lib.RR_OK, (entry, seq, out_dtype, rc)
    return out


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _attn(x, seq):
    """softmax(q k^T / 8) v per head of qkv rows x [B*seq][3*WIDTH], in x's dtype."""
    q, k, v = x.view(B, seq, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
    o = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v
    return o.permute(0, 2, 1, 3).reshape(B * seq, WIDTH)


@functools.lru_cache(maxsize=None)
def _case(seq, peaked=False):
    """Inputs and float64 references, computed once per seq and left unchanged:
    (qkv fp32, ref64 of qkv, ref64 of the bf16-rounded qkv)."""
    g = torch.Generator().manual_seed(1000 * int(peaked) + seq)
    qkv = torch.randn(B * seq, 3 * WIDTH, generator=g)
    if peaked:
        # q, k ~ N(0, 40) element-wise: logits q.k / 8 with a standard deviation of ~40
        qkv[:, :2 * WIDTH] *= 40.0 ** 0.5
    return qkv, _attn(qkv.double(), seq), _attn(qkv.bfloat16().double(), seq)


def _inputs(qkv, cuda):
    d32 = qkv.to(cuda)
    return {"rr_attention_ex": d32, "rr_attention_bf16": d32, "rr_attention_bf16_qkv16": qkv.bfloat16().to(cuda)}


@pytest.mark.parametrize("seq", SEQS)
def test_every_instance_both_output_types(cuda, seq):
    """NC = 1..8 at the first and last seq of each instance (and seq = 1), the
    six (entry, out_dtype) pairs each, on randn rows, at the bars
    test_gpu_vit.py sets: the fp32 kernel within rtol = atol = 1e-5 of float64;
    the bf16 kernels per-head-row cosine >= 0.9999 and max |err| <= 1e-2 of
    the float64 attention of the bf16-rounded rows; bf16 output = the same
    kernel's fp32 output rounded RNE, bit for bit; the qkv16 entry = the
    fp32-input bf16 kernel, bit for bit."""
    qkv, ref32, ref16 = _case(seq)
    x = _inputs(qkv, cuda)
    out = {(e, od): _run(e, x[e], seq, od).cpu() for e, od in PAIRS}
    for (e, od), o in out.items():
        assert o.dtype == (torch.bfloat16 if od else torch.float32) and bool(torch.isfinite(o.float()).all()), (e, od)
    # fp32 kernel
    torch.testing.assert_close(out["rr_attention_ex", 0], ref32.float(), rtol=1e-5, atol=1e-5)
    # the bf16 kernels
    for e in ENTRIES[1:]:
        for od in (0, 1):
            o = out[e, od].double()
            cos = torch.nn.functional.cosine_similarity(o.view(-1, HD), ref16.view(-1, HD), dim=1)
            err = (o - ref16).abs().max().item()
            print(f"seq {seq} {e} out_dtype {od}: max|err| {err:.3g} min cos {cos.min().item():.6f}")
            assert cos.min().item() >= 0.9999 and err <= 1e-2, (e, od, cos.min().item(), err)
    # the cast at the store, and the bf16-rows entry
    for e in ENTRIES:
        assert torch.equal(_bits(out[e, 1]), _bits(out[e, 0].bfloat16())), e
    for od in (0, 1):
        assert torch.equal(_bits(out["rr_attention_bf16_qkv16", od]), _bits(out["rr_attention_bf16", od])), od


@pytest.mark.parametrize("seq", [97, 160, 256])
def test_peaked_rows_within_derived_bound(cuda, seq):
    """q, k ~ N(0, 40) element-wise and v ~ N(0, 1): logits with a standard
    deviation of ~40, row maxima past 88 (exp before the max subtraction
    overflows) and masked keys next to scores of +-100.  The bound comes from
    the inputs, not from the kernels: with A = max_(query, key) sum_i |q_i||k_i|
    / 8 and V = max |v|, the fp32 scores and the exp2 argument are off by at
    most D = 68 2^-24 A, a softmax whose logits move by D moves its output by
    at most 2 D V, and P.V plus the division add (seq + 16) 2^-24 V:
        fp32 kernel, fp32 output: |out - ref| <= (136 A + seq + 16) 2^-24 V
        bf16 kernels: + 2^-8 V (P rounded to bf16, the row sum not)
        bf16 output:  + 2^-8 (|ref| + the bound above)
    (the bf16 kernels against the float64 attention of the bf16-rounded rows,
    A and V of those rows).  The bf16-output term was first written 2^-9 |ref|;
    that is half of what RNE allows: bf16 has 8 significand bits, so the
    spacing in [2^e, 2^(e+1)) is 2^(e-7) and |bf16(y) - y| <= 2^(e-8) <= 2^-8
    |y|, reached just above a power of two; and the value rounded is the
    kernel's y, |y| <= |ref| + bound.  (test_gpu_linear_edges.py measures
    err = 1.98 x 2^-9 |ref| on plain bf16 stores.)
    "cpu32" is the same attention evaluated by torch in float32 on the CPU.
    Measured on MI355X, max |out - ref|, fp32 output (bound; cpu32):
        seq  97: fp32 kernel 5.7e-5 (1.36e-2; 5.7e-5), bf16 kernels 2.6e-3 (3.10e-2; 1.0e-5)
        seq 160: fp32 kernel 3.6e-5 (1.40e-2; 2.7e-5), bf16 kernels 3.4e-3 (3.21e-2; 1.6e-5)
        seq 256: fp32 kernel 5.2e-5 (1.57e-2; 4.6e-5), bf16 kernels 3.2e-3 (3.57e-2; 1.8e-5)
    and with bf16 output 1.41e-2 / 8.99e-3 / 1.35e-2 (fp32 kernel) and 1.22e-2
    / 1.50e-2 / 8.5e-3 (bf16 kernels): the output rounding, 2^-8 of |ref| ~ 3.
    The qkv16 entry equals rr_attention_bf16 in every figure."""
    qkv, ref32, ref16 = _case(seq, True)
    x = _inputs(qkv, cuda)

    def bound_terms(rows):
        q, k, v = rows.double().view(B, seq, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
        a = (q.abs() @ k.abs().transpose(-1, -2) / 8.0).max().item()
        vmax = v.abs().max().item()
        return a, vmax, (136.0 * a + seq + 16) * 2.0 ** -24 * vmax

    q64, k64 = qkv.double().view(B, seq, 3, HEADS, HD).permute(2, 0, 3, 1, 4)[:2]
    logits = q64 @ k64.transpose(-1, -2) / 8.0
    # the inputs are what the case is about: a bare exp overflows, and +-100 sits among the keys
    assert logits.amax(-1).median() > 88 and logits.max() > 100 and logits.min() < -100
    for e, od in PAIRS:
        bf = e != "rr_attention_ex"
        ref = ref16 if bf else ref32
        a, vmax, base = bound_terms(qkv.bfloat16() if bf else qkv)
        pre = base + (2.0 ** -8 * vmax if bf else 0.0)
        bound = pre + (2.0 ** -8 * (ref.abs() + pre) if od else 0.0)
        o = _run(e, x[e], seq, od).cpu().double()
        cpu32 = _attn((qkv.bfloat16().float() if bf else qkv), seq).double()
        err = (o - ref).abs()
        print(f"seq {seq} {e} out_dtype {od}: A {a:.1f} max|v| {vmax:.2f} max|err| {err.max().item():.3e} "
              f"bound {pre:.3e}{' + 2^-8 (|ref| + that)' if od else ''} "
              f"cpu32 max|err| {(cpu32 - ref).abs().max().item():.3e}")
        assert bool(torch.isfinite(o).all()), (e, od)
        assert bool((err <= bound).all()), (e, od, err.max().item(), (err - bound).max().item())


GUARD_VAL = -768.0  # exact in bf16


def _guarded(t, front, back, fill):
    """t's values in the middle of a larger device buffer filled with `fill`;
    returns (buffer, view of the middle)."""
    buf = torch.full((front + t.numel() + back,), fill, dtype=t.dtype, device=t.device)
    mid = buf[front:front + t.numel()].view(t.shape)
    mid.copy_(t)
    return buf, mid


@pytest.mark.parametrize("seq", [97, 129])
def test_guarded_buffers_nan_isolation_and_repeatability(cuda, seq):
    """seq = 97 and 129 (31 padded rows in the last key tile; one row past four
    tiles).  Input guard: qkv ends a larger buffer whose other elements are
    NaN -- the 32 rows that would follow the last image, and the rows before
    the first -- and out sits between sentinels: the results equal those from
    plain buffers bit for bit and no sentinel changes, so rows >= seq of the
    last image neither reach a result nor are written.  NaN isolation: a NaN in
    one (image, head)'s K makes exactly that head's output block non-finite,
    one in its V exactly one column of that block; every other value keeps the
    clean run's bits.  Two runs on the same inputs give the same bits."""
    qkv, _, _ = _case(seq)
    x = _inputs(qkv, cuda)
    ld = 3 * WIDTH
    for e, od in PAIRS:
        plain = _run(e, x[e], seq, od)
        assert torch.equal(_bits(_run(e, x[e], seq, od)), _bits(plain)), (e, od)  # repeatability
        # guards: whole 16-B units, so the views stay as aligned as the kernels' vector loads need
        qbuf, qv = _guarded(x[e], 8 * ld, 32 * ld, float("nan"))
        obuf, ov = _guarded(torch.empty_like(plain), 4096, 32 * WIDTH, GUARD_VAL)
        ov.fill_(GUARD_VAL)
        _run(e, qv, seq, od, out=ov)
        assert torch.equal(_bits(ov), _bits(plain)), (e, od)
        assert bool((obuf[:4096] == GUARD_VAL).all()) and bool((obuf[4096 + ov.numel():] == GUARD_VAL).all()), (e, od)
        assert bool(torch.isnan(qbuf[:8 * ld]).all()) and bool(torch.isnan(qbuf[8 * ld + qv.numel():]).all())
        assert torch.equal(_bits(qv), _bits(x[e]))
        # NaN isolation
        bi, hi, row, col = 1, 1, seq - 2, 37
        blk = (slice(bi * seq, (bi + 1) * seq), slice(hi * HD, (hi + 1) * HD))
        for part in (1, 2):  # K, V
            xn = x[e].clone()
            xn[bi * seq + row, part * WIDTH + hi * HD + col] = float("nan")
            o = _run(e, xn, seq, od)
            bad = ~torch.isfinite(o.float())
            want = torch.zeros_like(bad)
            if part == 1:
                want[blk] = True
            else:
                want[blk[0], hi * HD + col] = True
            assert torch.equal(bad, want), (e, od, part, int(bad.sum()), int(want.sum()))
            assert torch.equal(_bits(o)[~want], _bits(plain)[~want]), (e, od, part)


def test_argument_checks(cuda):
    """seq = 0, seq = 257, head_dim = 32 and out_dtype = 2 are RR_EINVAL on all
    three entries; b = 0 is RR_OK and writes nothing."""
    seq = 40
    qkv, _, _ = _case(seq)
    x = _inputs(qkv, cuda)
    big = _inputs(torch.zeros(B * 257, 3 * WIDTH), cuda)  # large enough for whatever a missing check would launch
    for e in ENTRIES:
        out = torch.full((B * 257, WIDTH), GUARD_VAL, device=cuda)
        assert _rc(e, big[e], B, 0, HEADS, HD, 0, out) == _lib.RR_EINVAL, e
        assert _rc(e, big[e], B, 257, HEADS, HD, 0, out) == _lib.RR_EINVAL, e
        assert _rc(e, big[e], B, seq, HEADS, 32, 0, out) == _lib.RR_EINVAL, e
        assert _rc(e, big[e], B, seq, HEADS, HD, 2, out) == _lib.RR_EINVAL, e
        for od in (0, 1):
            assert _rc(e, x[e], 0, seq, HEADS, HD, od, out) == _lib.RR_OK, (e, od)
        assert bool((out == GUARD_VAL).all()), e
