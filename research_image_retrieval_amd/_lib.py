"""ctypes binding of librr.so (include/rr.h).

The library is built in-tree (``make -C research_image_retrieval_amd/csrc``,
or ``__graft_entry__.build()``).  There is no fallback: if librr.so is missing
or cannot be loaded every op raises, so a GPU run can never silently take a
CPU or eager-PyTorch path.
"""
import ctypes
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# RR_LIB_PATH: load an alternative build (A/B experiments on one device)
LIB_PATH = os.environ.get("RR_LIB_PATH") or os.path.join(_HERE, "librr.so")
CSRC = os.path.join(_HERE, "csrc")

RR_OK, RR_EINVAL, RR_EHIP, RR_EWORKSPACE, RR_EOVERFLOW = 0, -1, -2, -3, -4
ABI_VERSION = 9  # RR_ABI_VERSION of include/rr.h these signatures follow
AMAX_SLOTS = 64  # RR_AMAX_SLOTS

# timing classes (rr_timing_enable / rr_timing_collect)
TIME_COSINE, TIME_GEMM, TIME_SELECT, TIME_ELEM, TIME_COSINE_SEED, TIME_ATTN = 0, 1, 2, 3, 4, 5
# rr_set_tuning: name -> (key, the default: the library's own pick)
# (keys 6, 7 and 12 -- sweep_order, sweep_pf, lp_il -- were retired in ABI 5)
TUNING = {"gemm_cfg": (1, 0), "gemm_bk": (2, 0), "lp_cfg": (3, 0), "s3_cfg": (4, 0), "s3_stagger": (5, -1),
          "sweep_mf16": (8, -1), "sweep_il": (9, -1), "conv_il": (10, -1), "halo_mf": (11, -1), "s3_cfg_res": (13, 0),
          "sweep_form": (14, -1), "halo_2d": (15, -1), "trunk_parts": (16, -1)}
globals().update({"TUNE_" + _name.upper(): _key for _name, (_key, _) in TUNING.items()})  # TUNE_GEMM_CFG = 1, ...
TRUNK_MAX_STAGES = 8  # RR_TRUNK_MAX_STAGES


class TrunkConv(ctypes.Structure):
    """rr_trunk_conv_t"""
    _fields_ = [("w2", ctypes.c_void_p), ("w_iscale", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("cin", ctypes.c_int), ("cout", ctypes.c_int), ("kh", ctypes.c_int), ("kw", ctypes.c_int),
                ("stride", ctypes.c_int), ("pad", ctypes.c_int), ("residual", ctypes.c_int), ("relu", ctypes.c_int)]


class TrunkDesc(ctypes.Structure):
    """rr_trunk_desc_t"""
    _fields_ = [("n_stages", ctypes.c_int), ("blocks", ctypes.c_int * TRUNK_MAX_STAGES),
                ("fuse_entry", ctypes.c_int * TRUNK_MAX_STAGES), ("stride_on", ctypes.c_int),
                ("fuse_stem_pool", ctypes.c_int), ("lag", ctypes.c_int), ("mean", ctypes.c_float * 3),
                ("std", ctypes.c_float * 3), ("n_convs", ctypes.c_int), ("convs", ctypes.POINTER(TrunkConv))]

_lib = None
_lock = threading.RLock()

_vp = ctypes.c_void_p
_i = ctypes.c_int
_ll = ctypes.c_longlong
_f = ctypes.c_float
_sz = ctypes.c_size_t

# name -> (restype, argtypes): exactly the symbols include/rr.h declares
SIGNATURES = {
    "rr_version": (ctypes.c_char_p, []),
    "rr_abi_version": (_i, []),
    "rr_create": (_i, [_i, ctypes.POINTER(_vp)]),
    "rr_destroy": (_i, [_vp]),
    "rr_last_error": (ctypes.c_char_p, [_vp]),
    "rr_timing_enable": (_i, [_vp, _i]),
    "rr_timing_collect": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_ll)]),
    "rr_timing_collect_ex": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(_ll)]),
    "rr_trunk_h2_create": (_i, [_vp, _vp, ctypes.POINTER(_vp)]),
    "rr_trunk_h2_destroy": (_i, [_vp, _vp]),
    "rr_trunk_h2_workspace_size": (_sz, [_vp, _i, _i, _i, _i]),
    "rr_trunk_h2_parts": (_i, [_vp, _vp, _i, _i, _i]),
    "rr_trunk_h2_counters": (_i, [_vp, ctypes.POINTER(_ll)]),
    "rr_trunk_h2_forward_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "rr_get_device": (_i, [_vp, ctypes.POINTER(_i)]),
    "rr_set_tuning": (_i, [_vp, _i, _i]),
    "rr_cosine_topk_workspace_size": (_sz, [_i, _ll, _i, _i]),
    "rr_cosine_topk_workspace_size_cap": (_sz, [_i, _ll, _i, _i, _ll]),
    "rr_cosine_topk_cap_for": (_ll, [_i, _ll, _i, _i, _sz]),
    "rr_cosine_topk_counts_offset": (_sz, [_i, _ll, _i, _i]),
    "rr_cosine_topk_overflow_offset": (_sz, [_i, _ll, _i, _i]),
    "rr_cosine_topk": (_i, [_vp, _vp, _i, _vp, _ll, _i, _i, _ll, _vp, _vp, _vp, _sz, _vp]),
    "rr_cosine_scores": (_i, [_vp, _vp, _i, _vp, _ll, _i, _vp, _vp]),
    "rr_topk_merge": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "rr_preprocess_u8": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "rr_nchw_to_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "rr_preprocess_u8_ex": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "rr_nchw_to_nhwc_ex": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rr_conv2d": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "rr_conv2d_h2": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "rr_split2_f16": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "rr_stem_pool_h2": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "rr_bottleneck_out_h2": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp,
                                  _vp, _vp]),
    "rr_amax_f32": (_i, [_vp, _vp, _ll, _vp, _vp]),
    "rr_resize_bilinear": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp]),
    "rr_maxpool2d": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "rr_gem_pool": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _vp, _vp]),
    "rr_linear": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "rr_l2_normalize": (_i, [_vp, _vp, _i, _i, _f, _vp, _vp]),
    "rr_dolg_local_pool": (_i, [_vp, _vp, _i, _i, _i, _vp, _f, _vp, _vp]),
    "rr_dolg_orth_fuse": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "rr_soa_attention": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "rr_attention_hd128": (_i, [_vp, _vp, _ll, _vp, _ll, _vp, _ll, _i, _i, _i, _i, _vp, _vp]),
    "rr_token_pool": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "rr_gelu": (_i, [_vp, _vp, _ll, _vp, _vp]),
    "rr_how_vlad": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _f, _vp, _vp]),
    "rr_how_asmk": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "rr_sos_cov": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _f, _vp, _vp, _vp, _vp]),
    "rr_linear_splitk": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "rr_linear_splitk_ex": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "rr_cls_attn_pool": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "rr_spp_regions": (_i, [_i, _i, _vp, _i]),
    "rr_h2_route": (_i, [_vp, _vp, _vp]),
    "rr_gemm_route": (_i, [_vp, _vp, _vp]),
    "rr_spp_max": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "rr_spoc_refine": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    "rr_linear_groupmax": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "rr_se_squeeze": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "rr_se_apply": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "rr_linear_ex": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "rr_layernorm": (_i, [_vp, _vp, _ll, _i, _i, _vp, _vp, _f, _vp, _vp]),
    "rr_patchify": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rr_vit_tokens": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "rr_patchify_ex": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "rr_vit_tokens_ex": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp]),
    "rr_attention": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "rr_attention_ex": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rr_attention_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rr_attention_bf16_qkv16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rr_layernorm_ex": (_i, [_vp, _vp, _ll, _i, _i, _vp, _vp, _f, _i, _vp, _vp]),
    "rr_linear_bf16": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "rr_linear_bf16_ln": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp]),
    "rr_ln_partials_bf16": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "rr_alpha_qe": (_i, [_vp, _vp, _i, _vp, _ll, _i, _vp, _vp, _i, _i, _f, _ll, _vp, _vp]),
    "rr_prefilter_gallery_bound": (_i, [_vp, _vp, _vp, _ll, _i, _vp, _vp]),
    "rr_cosine_topk_prefilter_workspace_size": (_sz, [_i, _ll, _i, _i]),
    "rr_cosine_topk_prefilter_counts_offset": (_sz, [_i, _ll, _i, _i]),
    "rr_cosine_topk_prefilter_overflow_offset": (_sz, [_i, _ll, _i, _i]),
    "rr_cosine_topk_prefilter_workspace_size_cap": (_sz, [_i, _ll, _i, _i, _ll]),
    "rr_cosine_topk_prefilter_cap_for": (_ll, [_i, _ll, _i, _i, _sz]),
    "rr_cosine_topk_prefilter": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _ll, _i, _i, _ll, _vp, _vp, _vp, _sz, _vp]),
    "rr_pcaw_gram_workspace_size": (_sz, [_ll, _i]),
    "rr_pcaw_gram": (_i, [_vp, _vp, _ll, _i, _vp, _sz, _vp, _vp, _vp]),
    "rr_quantize_rows": (_i, [_vp, _vp, _ll, _i, _i, _vp, _vp, _vp]),
    "rr_cosine_topk_lp": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _ll, _i, _i, _i, _ll, _vp, _vp, _vp, _sz, _vp]),
}


class RRError(RuntimeError):
    pass


def build(force=False):
    """Compile librr.so for gfx950 with hipcc (in-tree)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", CSRC, "-j4"], check=True)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RRError(
                    f"librr.so not found at {LIB_PATH}: build it with `make -C {CSRC}` "
                    "(there is deliberately no CPU/eager fallback)")
            L = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                if os.environ.get("RR_LIB_PATH") and not hasattr(L, name):
                    continue  # A/B against an older build: bind what it has
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            if not os.environ.get("RR_LIB_PATH") and L.rr_abi_version() != ABI_VERSION:
                raise RRError(f"librr.so ABI {L.rr_abi_version()} != {ABI_VERSION} this binding was written "
                              f"against: rebuild it with `make -C {CSRC}`")
            _lib = L
    return _lib


_handles = {}


def handle(device_index):
    """Per-device librr handle (created once)."""
    h = _handles.get(device_index)
    if h is None:
        with _lock:
            h = _handles.get(device_index)
            if h is None:
                out = _vp()
                rc = lib().rr_create(int(device_index), ctypes.byref(out))
                if rc != RR_OK:
                    raise RRError(f"rr_create(device={device_index}) failed with {rc}")
                h = out.value
                _handles[device_index] = h
    return h


def check(rc, h, what):
    if rc != RR_OK:
        msg = lib().rr_last_error(h)
        raise RRError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
