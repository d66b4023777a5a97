"""ctypes binding of libdissc_hip.so (C ABI: include/dissc_hip.h).

torch is imported first on purpose: the library's DT_NEEDED libamdhip64.so.7 then
resolves to the HIP runtime PyTorch already loaded, so device pointers and
hipStream_t handles are shared between PyTorch (allocator, streams, RCCL) and the
kernels.  If the library is missing this module raises -- there is no fallback.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL load, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libdissc_hip.so"


def library_path():
    # DISSC_HIP_LIB: development hook for A/B-ing an alternative build of the same library
    return os.environ.get("DISSC_HIP_LIB") or os.path.join(_HERE, _LIB_NAME)


class DisscError(RuntimeError):
    pass


class DisscTensor(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p),
                ("shape", ctypes.c_int64 * 4), ("ndim", ctypes.c_int32)]


MAX_UPS, MAX_RK = 8, 4


class DisscGenConfig(ctypes.Structure):
    _fields_ = [("model_in_dim", ctypes.c_int32), ("upsample_initial_channel", ctypes.c_int32),
                ("num_upsamples", ctypes.c_int32), ("upsample_rates", ctypes.c_int32 * MAX_UPS),
                ("upsample_kernel_sizes", ctypes.c_int32 * MAX_UPS), ("num_kernels", ctypes.c_int32),
                ("resblock_kernel_sizes", ctypes.c_int32 * MAX_RK),
                ("resblock_dilations", (ctypes.c_int32 * 3) * MAX_RK),
                ("num_embeddings", ctypes.c_int32), ("embedding_dim", ctypes.c_int32),
                ("num_speakers", ctypes.c_int32), ("has_f0", ctypes.c_int32), ("has_spkr", ctypes.c_int32)]


class DisscConvLaunch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("family", "cfg", "bm", "bn", "rows", "p0", "np", "ntap", "pad_left")]


class DisscBf3Info(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bm", "bn", "small_grid", "tile", "cols", "h4", "pad")]


class DisscChainInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("wout", "span", "halo", "lds_bytes", "tiles_per_wave")]


class DisscWino8Plan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("mi", "ni", "wps", "r", "ns", "unit", "ot", "cpr", "gx", "gy")]


class DisscWinoPlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("ns", "dilation", "cpr", "rh", "tw", "shv", "unit", "ot", "gx", "gy", "wgs", "lds_bytes")]


def _load():
    path = library_path()
    if not os.path.exists(path):
        raise DisscError(
            f"{path} not found: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()').  "
            "dissc_amd has no CPU fallback.")
    L = ctypes.CDLL(path)
    vp, i32, i64p = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    L.dissc_last_error.restype = ctypes.c_char_p
    L.dissc_abi_version.restype = i32
    L.dissc_device_count.restype = i32
    L.dissc_device_name.argtypes = [i32, ctypes.c_char_p, ctypes.c_size_t]
    L.dissc_gen_create.argtypes = [ctypes.POINTER(DisscGenConfig), ctypes.POINTER(DisscTensor),
                                   ctypes.c_size_t, ctypes.POINTER(vp)]
    L.dissc_gen_create_ex.argtypes = [ctypes.POINTER(DisscGenConfig), ctypes.POINTER(DisscTensor),
                                      ctypes.c_size_t, i32, ctypes.POINTER(vp)]
    L.dissc_gen_create_rb.argtypes = [ctypes.POINTER(DisscGenConfig), ctypes.POINTER(DisscTensor),
                                      ctypes.c_size_t, i32, i32, ctypes.POINTER(vp)]
    L.dissc_gen_destroy.argtypes = [vp]
    L.dissc_gen_destroy.restype = None
    L.dissc_gen_hop.argtypes = [vp]
    L.dissc_gen_workspace_bytes.argtypes = [vp, i32, i32]
    L.dissc_gen_workspace_bytes.restype = ctypes.c_size_t
    L.dissc_gen_flops.argtypes = [vp, ctypes.c_int64]
    L.dissc_gen_flops.restype = ctypes.c_double
    L.dissc_gen_flops_executed.argtypes = [vp, ctypes.c_int64]
    L.dissc_gen_flops_executed.restype = ctypes.c_double
    L.dissc_gen_forward.argtypes = [vp, i64p, vp, i64p, vp, i32, i32, vp, vp, ctypes.c_size_t, vp]
    L.dissc_conv1d.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32,
                               ctypes.c_float, vp]
    L.dissc_conv_transpose1d.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32,
                                         ctypes.c_float, vp]
    L.dissc_conv1d_prec.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, ctypes.c_float, i32, vp]
    L.dissc_conv_transpose1d_prec.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, ctypes.c_float, i32, vp]
    L.dissc_pred_create.argtypes = [i32, ctypes.POINTER(DisscTensor), ctypes.c_size_t, ctypes.POINTER(vp)]
    L.dissc_pred_destroy.argtypes = [vp]
    L.dissc_pred_destroy.restype = None
    L.dissc_pred_workspace_bytes.argtypes = [vp, i32, i32]
    L.dissc_pred_workspace_bytes.restype = ctypes.c_size_t
    L.dissc_len_set_norm.argtypes = [vp, ctypes.c_float, ctypes.c_float]
    L.dissc_len_forward.argtypes = [vp, vp, vp, vp, i32, i32, vp, i32, vp, ctypes.c_size_t, vp]
    L.dissc_pitch_forward.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, i32, vp, i32, vp,
                                      ctypes.c_size_t, vp]
    L.dissc_dedup.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
    L.dissc_len_carryover.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.dissc_expand.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp]
    L.dissc_hubert_create.argtypes = [i32, ctypes.POINTER(DisscTensor), ctypes.c_size_t, vp, i32,
                                      ctypes.POINTER(vp)]
    L.dissc_hubert_create_ex.argtypes = [i32, ctypes.POINTER(DisscTensor), ctypes.c_size_t, vp, i32, i32,
                                         ctypes.POINTER(vp)]
    L.dissc_hubert_precision.argtypes = [vp]
    L.dissc_hubert_destroy.argtypes = [vp]
    L.dissc_hubert_destroy.restype = None
    L.dissc_hubert_frames.argtypes = [i32]
    L.dissc_hubert_workspace_bytes.argtypes = [vp, i32, i32]
    L.dissc_hubert_workspace_bytes.restype = ctypes.c_size_t
    L.dissc_hubert_forward.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, ctypes.c_size_t, vp]
    L.dissc_kmeans_assign.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.dissc_mfma_peak.argtypes = [i32, ctypes.POINTER(ctypes.c_float)]
    L.dissc_erf_check.argtypes = [vp, vp, i32, vp]
    L.dissc_attention.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    L.dissc_layernorm_cf.argtypes = [vp, vp, vp, vp, i32, i32, i32, ctypes.c_float, vp, vp]
    L.dissc_set_option.argtypes = [ctypes.c_char_p, i32]
    L.dissc_get_option.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    L.dissc_conv_bench.argtypes = [i32] * 9 + [ctypes.POINTER(ctypes.c_float)]
    L.dissc_conv1d_s2.argtypes = [vp, vp, vp, vp, vp] + [i32] * 9 + [vp]
    L.dissc_conv1d_s2_prec.argtypes = [vp, vp, vp, vp, vp] + [i32] * 9 + [vp]
    L.dissc_linear_prec.argtypes = [vp, vp, vp, vp, vp, vp] + [i32] * 7 + [vp]
    L.dissc_conv_s2_bench.argtypes = [i32] * 5 + [ctypes.POINTER(ctypes.c_float)]
    L.dissc_pair_bench.argtypes = [i32] * 8 + [ctypes.POINTER(ctypes.c_float)]
    L.dissc_pair_info.argtypes = [i32] * 3 + [ctypes.POINTER(ctypes.c_int)] * 2
    L.dissc_resblock2_bench.argtypes = [i32] * 9 + [ctypes.POINTER(ctypes.c_float)]
    L.dissc_resblock2_info.argtypes = [i32] * 4 + [ctypes.POINTER(ctypes.c_int)] * 2
    L.dissc_resblock2_1d.argtypes = [vp] * 8 + [i32] * 7 + [ctypes.c_float, i32, ctypes.c_float, i32, vp]
    L.dissc_conv_info.argtypes = [i32] * 7 + [ctypes.POINTER(DisscConvLaunch), i32, ctypes.POINTER(ctypes.c_int)]
    L.dissc_wino8_info.argtypes = [i32] * 6 + [ctypes.POINTER(DisscWino8Plan)]
    if hasattr(L, "dissc_wino8_form"):  # (an older build loaded through DISSC_HIP_LIB for an A/B has none)
        L.dissc_wino8_form.argtypes = [i32] * 6 + [ctypes.POINTER(ctypes.c_int)]
    L.dissc_wino_info.argtypes = [i32] * 5 + [ctypes.POINTER(DisscWinoPlan)]
    L.dissc_resblock1d_bf3.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, i32, ctypes.c_float, i32, ctypes.c_float, i32, i32, vp]
    L.dissc_bf3_info.argtypes = [i32] * 6 + [vp, i32, i32, ctypes.POINTER(DisscBf3Info)]
    if hasattr(L, "dissc_reschain1d"):  # (an older build loaded through DISSC_HIP_LIB for an A/B, tools/lib_ab.sh, has none of the three)
        # x, w6, b6, y, acc, lengths | B, C, k | dil3 | ld, Lmax | slope | epi | mrf_div | mode | stream
        L.dissc_reschain1d.argtypes = [vp] * 6 + [i32] * 3 + [vp, i32, i32, ctypes.c_float, i32, ctypes.c_float, i32, vp]
        L.dissc_chain_info.argtypes = [i32, i32, vp, ctypes.POINTER(DisscChainInfo)]
        L.dissc_chain_bench.argtypes = [i32] * 6 + [ctypes.POINTER(ctypes.c_float)]
    L.dissc_respair1d.argtypes = [vp] * 8 + [i32] * 6 + [ctypes.c_float, i32, ctypes.c_float, i32, vp]
    L.dissc_wav_postprocess.argtypes = [vp, vp, i32, i32, vp]
    L.dissc_pitch_stats.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    i64 = ctypes.c_longlong
    L.dissc_pack_rows.argtypes = [vp, i64, vp, vp, i32, i32, vp, vp]
    L.dissc_comm_unique_id.argtypes = [ctypes.c_char_p]
    L.dissc_comm_create.argtypes = [ctypes.c_char_p, i32, i32, ctypes.POINTER(vp)]
    L.dissc_comm_destroy.argtypes = [vp]
    L.dissc_allgather_waves.argtypes = [vp, vp, ctypes.c_size_t, vp, vp]
    L.dissc_resample.argtypes = [vp, i32, vp, i32, ctypes.c_double, vp, vp, i32, i32, vp]
    return L


lib = _load()

# tuning hook: DISSC_OPTIONS="key=value,key=value" -> dissc_set_option (see include/dissc_hip.h)
for _kv in filter(None, os.environ.get("DISSC_OPTIONS", "").split(",")):
    _k, _v = _kv.split("=")
    if lib.dissc_set_option(_k.strip().encode(), int(_v)) != 0:
        raise DisscError(f"DISSC_OPTIONS: unknown option {_k}")


def check(rc, what=""):
    if rc != 0:
        msg = lib.dissc_last_error()
        raise DisscError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def current_stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def make_tensor_table(named):
    """{name: contiguous fp32 CPU tensor} -> (ctypes array, keep-alive list)."""
    arr = (DisscTensor * len(named))()
    keep = []
    for i, (k, t) in enumerate(named.items()):
        t = t.detach().to("cpu", torch.float32).contiguous()
        nb = k.encode()
        keep.append((t, nb))
        arr[i].name = nb
        arr[i].data = t.data_ptr()
        arr[i].ndim = t.dim()
        for d in range(t.dim()):
            arr[i].shape[d] = t.shape[d]
    return arr, keep


def conv_info(Cin, Cout, k, dilation=1, up=1, B=1, Lmax_out=1):
    """dissc_conv_info: the launches of dissc_conv1d (up = 1) / dissc_conv_transpose1d (up > 1) for the shape under the current
    option defaults, as a list of dicts (family, cfg, bm, bn, rows, p0, np, ntap, pad_left).  Host only."""
    out = (DisscConvLaunch * 16)()
    n = ctypes.c_int(0)
    check(lib.dissc_conv_info(Cin, Cout, k, dilation, up, B, Lmax_out, out, 16, ctypes.byref(n)), "dissc_conv_info")
    assert n.value <= 16
    return [{f: getattr(out[i], f) for f, _ in DisscConvLaunch._fields_} for i in range(n.value)]


def wino8_info(C, k, dilation, R, B, Lmax):
    """dissc_wino8_info: the conv_wino8_kernel instance and grid of the shape as F(6,3) (R = 3) or F(5,4) (R = 4) under the current
    option defaults, as a dict (mi, ni, wps, r, ns, unit, ot, cpr, gx, gy).  Host only."""
    out = DisscWino8Plan()
    check(lib.dissc_wino8_info(C, k, dilation, R, B, Lmax, ctypes.byref(out)), "dissc_wino8_info")
    return {f: getattr(out, f) for f, _ in DisscWino8Plan._fields_}


def wino8_form(C, k, dilation, R, B, Lmax):
    """dissc_wino8_form: 1 where that launch shares one input transform between the waves of a workgroup ("wino8_sv"), 0 where
    every wave forms its own tile.  Host only."""
    out = ctypes.c_int(-1)
    check(lib.dissc_wino8_form(C, k, dilation, R, B, Lmax, ctypes.byref(out)), "dissc_wino8_form")
    return out.value


def wino_info(C, k, dilation, B, Lmax):
    """dissc_wino_info: the conv_wino_kernel (F(4,3)) instance and grid of the shape under the current option defaults, as a dict
    (ns, dilation, cpr, rh, tw, shv, unit, ot, gx, gy, wgs, lds_bytes).  Host only."""
    out = DisscWinoPlan()
    check(lib.dissc_wino_info(C, k, dilation, B, Lmax, ctypes.byref(out)), "dissc_wino_info")
    return {f: getattr(out, f) for f, _ in DisscWinoPlan._fields_}


def bf3_conv_info(Cin, Cout, k, dilation=1, B=1, Lmax=1):
    """dissc_bf3_info for a conv: the conv_bf3_kernel tile of the layer (for a ConvTranspose phase group: Cout = its GEMM rows, k = its
    taps) under the current option defaults, as a dict (bm, bn, small_grid, tile).  Raises where the layer gets no split-bf16
    instance.  Host only."""
    out = DisscBf3Info()
    check(lib.dissc_bf3_info(Cout, Cin, k, dilation, B, Lmax, None, 0, 0, ctypes.byref(out)), "dissc_bf3_info")
    return {f: getattr(out, f) for f in ("bm", "bn", "small_grid", "tile")}


def bf3_block_info(C, k, dil, m0=0, m1=3):
    """dissc_bf3_info for pairs [m0, m1) of a ResBlock on resblock_bf3_kernel, as a dict (cols, pad, h4, bn).  Host only."""
    out = DisscBf3Info()
    d3 = (ctypes.c_int32 * 3)(*dil)
    check(lib.dissc_bf3_info(C, C, k, 1, 1, 1, d3, m0, m1, ctypes.byref(out)), "dissc_bf3_info")
    return {f: getattr(out, f) for f in ("cols", "pad", "h4", "bn")}


def get_option(key):
    v = ctypes.c_int(0)
    check(lib.dissc_get_option(key.encode(), ctypes.byref(v)), f"dissc_get_option({key})")
    return v.value


def set_option(key, value):
    check(lib.dissc_set_option(key.encode(), int(value)), f"dissc_set_option({key})")
