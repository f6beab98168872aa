"""Plain-torch restatement of the SoSNet head (models/sosnet.py:12-183), a test
helper.  head_forward writes the reference's own sequence, LITERALLY: the
attention MLP per position and the multiply (:76-92), the 1x1 projection WITH
its bias on the attended map, mean, centring, bmm / (N - 1), the triu_indices
gather, F.normalize (:27-55), feature_proj (Linear, ReLU, Linear, :131-136) and
F.normalize (:182), on the weight format of weights.sos_head_from_state_dict,
in any dtype.  It is independent of the three identities the kernels use;
head_rearranged writes those (the projection of the RAW rows times a_p, no
bias, the L2 of the packed vector applied after the first Linear).
tests/test_sos_host.py pins both to the reference's own output
(tests/golden/sos.npz), so the GPU tests may use them at other shapes and in
float64.
"""
import torch
import torch.nn.functional as F


def triu_offset(i, j, c):
    """Place of (i, j), i <= j, in the row-major packed upper triangle."""
    return i * c - i * (i - 1) // 2 + (j - i)


def attention(x, head, dtype=torch.float64):
    """SimilarityAttention's weights (:84) for rows x [B,N,Cin]: (a [B,N], hid
    [B,N,H/2], the ReLU'd second layer)."""
    x = x.to(dtype)
    h1 = F.relu(F.linear(x, head["att_w1"].to(dtype), head["att_b1"].to(dtype)))
    hid = F.relu(F.linear(h1, head["att_w2"].to(dtype), head["att_b2"].to(dtype)))
    a = torch.sigmoid(hid @ head["att_w3"].to(dtype) + head["att_b3"].to(dtype))
    return a, hid


def pack(cov, order="triu"):
    """cov [B,c,c] -> the packed triangle.  order: "triu" (the reference, :48-49),
    "tril" (lower triangle, row-major) or "colmajor" (upper triangle walked by
    columns) — the last two are the sensitivity tests' wrong packings."""
    c = cov.shape[-1]
    if order == "triu":
        i = torch.triu_indices(c, c, offset=0)
        return cov[:, i[0], i[1]]
    if order == "tril":
        i = torch.tril_indices(c, c, offset=0)
        return cov[:, i[0], i[1]]
    if order == "colmajor":
        i = torch.triu_indices(c, c, offset=0)
        key = torch.argsort(i[1] * c + i[0])
        return cov[:, i[0][key], i[1][key]]
    raise ValueError(order)


def covariance(y, center=True, unbiased=True):
    """SecondOrderPooling's covariance (:41-45) of rows y [B,N,c]: [B,c,c]."""
    n = y.shape[1]
    yc = y - y.mean(dim=1, keepdim=True) if center else y
    return torch.bmm(yc.transpose(1, 2), yc) / ((n - 1) if unbiased else n)


def head_forward(x4, head, dtype=torch.float64, attend=True, center=True, order="triu", unbiased=True, relu=True):
    """Everything after the trunk on x4 [B,Cin,H,W] (NCHW), literal form: dict(att
    [B,N] (ones without attention), hid, y (the projected rows), cov (the packed
    triangle BEFORE its L2), vhat (after it), hidden, features, out [B,F]).
    The switches each disable one piece (the sensitivity tests): attend=False
    (a = 1), center=False, order "tril" / "colmajor", unbiased=False (/ N),
    relu=False (no ReLU in feature_proj)."""
    b, cin, h, w = x4.shape
    x = x4.to(dtype).permute(0, 2, 3, 1).reshape(b, h * w, cin)
    got = {}
    if "att_w1" in head and attend:
        got["att"], got["hid"] = attention(x, head, dtype)
    else:
        got["att"] = torch.ones(b, h * w, dtype=dtype)
    xa = x * got["att"].unsqueeze(2)                                               # :90
    got["y"] = F.linear(xa, head["proj_w"].to(dtype), head["proj_b"].to(dtype))   # :33
    got["cov"] = pack(covariance(got["y"], center, unbiased), order)              # :41-49
    got["vhat"] = F.normalize(got["cov"], p=2, dim=1)                             # :53
    hid = F.linear(got["vhat"], head["fp0_w"].to(dtype), head["fp0_b"].to(dtype))
    got["hidden"] = F.relu(hid) if relu else hid
    got["features"] = F.linear(got["hidden"], head["fp3_w"].to(dtype), head["fp3_b"].to(dtype))
    got["out"] = F.normalize(got["features"], p=2, dim=1)
    return got


def cov_from_rows(z, att, dtype=torch.float64):
    """What rr_sos_cov computes from RAW projection rows z [B,N,c] and weights
    att [B,N] (None: ones): (cov, the un-normalised packed triangle of the
    centred covariance of a_p z_p; inv_norm [B] = 1 / max(||cov row||, 1e-12))."""
    y = z.to(dtype)
    if att is not None:
        y = y * att.to(dtype).unsqueeze(2)
    v = pack(covariance(y))
    return v, 1.0 / v.norm(dim=1).clamp_min(1e-12)


def head_rearranged(x4, head, dtype=torch.float32):
    """The head as the kernels compute it: y_p = a_p (Wp x_p) with no bias (it
    cancels under the centring), and W0' v^ = (W0' v) / max(||v||, 1e-12).
    Same keys as head_forward, plus inv_norm."""
    b, cin, h, w = x4.shape
    x = x4.to(dtype).permute(0, 2, 3, 1).reshape(b, h * w, cin)
    got = {}
    att = None
    if "att_w1" in head:
        att, got["hid"] = attention(x, head, dtype)
    got["att"] = att if att is not None else torch.ones(b, h * w, dtype=dtype)
    z = F.linear(x, head["proj_w"].to(dtype))
    got["cov"], got["inv_norm"] = cov_from_rows(z, att, dtype)
    got["vhat"] = got["cov"] * got["inv_norm"].unsqueeze(1)
    lin = F.linear(got["cov"], head["fp0_w"].to(dtype)) * got["inv_norm"].unsqueeze(1) + head["fp0_b"].to(dtype)
    got["hidden"] = F.relu(lin)
    got["features"] = F.linear(got["hidden"], head["fp3_w"].to(dtype), head["fp3_b"].to(dtype))
    got["out"] = F.normalize(got["features"], p=2, dim=1)
    return got
