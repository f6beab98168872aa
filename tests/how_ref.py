"""Plain-torch restatement of the HOW head (models/how_vlad.py:14-199), a test
helper.  It writes the reference's own sequence (the 1x1 local_proj, F.normalize
per position, torch.cdist, softmax(-alpha dist) and the residual sum, or argmin /
gather / mean + std threshold / the masked histogram, F.normalize, final_proj,
F.normalize) on the weight format of weights.how_head_from_state_dict, in any
dtype.  tests/test_how_host.py pins it to the reference's own output
(tests/golden/how.npz), so the GPU tests may use it at other shapes and in
float64.
"""
import torch
import torch.nn.functional as F

ALPHA = 100.0  # VLADPooling's default (:17)


def vlad(x, cent, alpha=ALPHA, dtype=torch.float64, normalize=True, hard=False, subtract=True):
    """VLADPooling.forward :36-55 (before its F.normalize) on RAW rows x [B,N,D]
    after HOWModel's :162: dict(desc [B,N,D], assign [B,N,K], vlad [B, K D]).
    The degenerate switches (the sensitivity tests): normalize=False skips
    :162, hard=True puts a one-hot at the nearest centroid in place of the
    softmax, subtract=False drops the centroid from the residual."""
    x, cent = x.to(dtype), cent.to(dtype)
    desc = F.normalize(x, p=2, dim=2) if normalize else x
    b = x.shape[0]
    dist = torch.cdist(desc, cent.unsqueeze(0).expand(b, -1, -1))
    a = F.softmax(-alpha * dist, dim=2)
    if hard:
        a = F.one_hot(dist.argmin(dim=2), cent.shape[0]).to(dtype)
    # sum_n a[n,k] (x_n - c_k), the loop :44-52 written as two products
    v = torch.einsum("bnk,bnd->bkd", a, desc)
    if subtract:
        v = v - a.sum(dim=1).unsqueeze(2) * cent.unsqueeze(0)
    return {"desc": desc, "assign": a, "vlad": v.reshape(b, -1)}


def asmk(x, cent, weights, dtype=torch.float64, mask=True):
    """ASMKPooling.forward :80-99 (before its F.normalize) on RAW rows x
    [B,N,D]: dict(desc, dist [B,N,K], nearest [B,N], mind [B,N], thr [B,1],
    mask [B,N], count [B,K] (int64), asmk [B,K] = weights x count).
    mask=False keeps every position (the sensitivity tests)."""
    x, cent, weights = x.to(dtype), cent.to(dtype), weights.to(dtype)
    desc = F.normalize(x, p=2, dim=2)
    b, k = x.shape[0], cent.shape[0]
    dist = torch.cdist(desc, cent.unsqueeze(0).expand(b, -1, -1))
    nearest = torch.argmin(dist, dim=2)
    mind = torch.gather(dist, 2, nearest.unsqueeze(2)).squeeze(2)
    thr = mind.mean(dim=1, keepdim=True) + mind.std(dim=1, keepdim=True)
    keep = mind < thr if mask else torch.ones_like(mind, dtype=torch.bool)
    count = torch.zeros(b, k, dtype=torch.int64)
    count.scatter_add_(1, nearest, keep.to(torch.int64))
    return {"desc": desc, "dist": dist, "nearest": nearest, "mind": mind, "thr": thr, "mask": keep, "count": count,
            "asmk": weights.unsqueeze(0) * count.to(dtype)}


def local_rows(x4, head, dtype=torch.float64):
    """local_proj on x4 [B,Cin,H,W] (NCHW) as rows: [B, H W, D] (:155-159)."""
    b, cin, h, w = x4.shape
    x = x4.to(dtype).permute(0, 2, 3, 1).reshape(b, h * w, cin)
    return x @ head["local_w"].to(dtype).t() + head["local_b"].to(dtype)


def head_forward(x4, head, dtype=torch.float64, pooling=None, **switches):
    """Everything after the trunk: dict(out [B,2048], features, pooled (after
    its F.normalize), local (raw rows), desc, and the pooling's own
    intermediates).  pooling: "vlad" or "asmk" (default: what the head holds).
    switches: vlad's normalize / hard / subtract / alpha, asmk's mask, and
    ones=True (all-ones ASMK weights)."""
    pooling = pooling or ("asmk" if "weights" in head else "vlad")
    y = local_rows(x4, head, dtype)
    if pooling == "vlad":
        got = vlad(y, head["centroids"], switches.pop("alpha", ALPHA), dtype, **switches)
        pooled = got["vlad"]
    else:
        wts = head["weights"]
        if switches.pop("ones", False):
            wts = torch.ones_like(wts)
        got = asmk(y, head["centroids"], wts, dtype, **switches)
        pooled = got["asmk"]
    got["local"] = y
    got["pooled"] = F.normalize(pooled, p=2, dim=1)
    got["features"] = F.linear(got["pooled"], head["final_w"].to(dtype), head["final_b"].to(dtype))
    got["out"] = F.normalize(got["features"], p=2, dim=1)
    return got


def margins(x, cent, weights=None):
    """The float64 decision margins of ASMK on RAW rows x [B,N,D]: per position
    the second-nearest minus the nearest distance (inf for one centroid) and
    |min-dist - threshold| (inf where the threshold is NaN, n = 1): (argmin
    margin [B,N], threshold margin [B,N])."""
    r = asmk(x, cent, torch.ones(cent.shape[0]) if weights is None else weights, torch.float64)
    d = r["dist"].sort(dim=2).values
    am = d[..., 1] - d[..., 0] if d.shape[2] > 1 else torch.full_like(d[..., 0], float("inf"))
    tm = (r["mind"] - r["thr"]).abs()
    tm = torch.where(torch.isnan(tm), torch.full_like(tm, float("inf")), tm)
    return am, tm
