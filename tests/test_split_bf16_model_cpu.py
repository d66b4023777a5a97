"""The encoder's opt-in split-bf16 mode on the CPU: its public surface (option, C ABI, Python, command lines) against the
library as built, and the CPU model of its arithmetic (tests/split_bf16_model.py) that the GPU tests use as their yardstick.

The model's figures (worst per-frame l2 relative error of the layer-6 features against the float64 oracle):
    iid 2 s / 1 s: fp32 oracle 8.3e-7 / 8.4e-7, split model 1.6e-5 / 1.4e-5; identity control 3.0e-7, hi-only control 8.9e-3 (1 s)
    trained-like speech_like / speech_dc / dither: fp32 oracle 4.0e-8 / 4.4e-8 / 3.7e-8, split model 2.8e-7 / 2.9e-7 / 2.9e-7."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import hubert_ref as hr
import synthdata as synth
import split_bf16_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IID_UTTS = ((32000, 719), (16000, 7))
TL_UTTS = (("speech_like", 32000, 31), ("speech_dc", 16000, 32), ("dither", 8000, 33))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import dissc_amd
    return dissc_amd


# ---- public surface ---------------------------------------------------------------------------------------------------------
def test_enc_precision_option_round_trips_and_defaults_to_zero(built):
    L = built.lib
    v = ctypes.c_int(-7)
    assert L.dissc_get_option(b"enc_precision", ctypes.byref(v)) == 0
    assert v.value == 0
    try:
        assert L.dissc_set_option(b"enc_precision", 1) == 0
        assert L.dissc_get_option(b"enc_precision", ctypes.byref(v)) == 0 and v.value == 1
        p = ctypes.c_int(-7)  # the generator's option is another one
        assert L.dissc_get_option(b"precision", ctypes.byref(p)) == 0 and p.value == 0
    finally:
        assert L.dissc_set_option(b"enc_precision", 0) == 0
    assert L.dissc_get_option(b"enc_precision", ctypes.byref(v)) == 0 and v.value == 0


def test_create_ex_and_precision_are_declared_and_exported(built):
    src = open(os.path.join(ROOT, "include", "dissc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dissc_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(built.library_path())
    for s in ("dissc_hubert_create_ex", "dissc_hubert_precision", "dissc_conv1d_s2_prec", "dissc_linear_prec"):
        assert s in declared, s
        assert hasattr(L, s), s
    assert "enc_precision" in open(os.path.join(ROOT, "include", "dissc_hip.h")).read()


def test_create_ex_refuses_an_unknown_precision(built):
    """argument checks come before anything touches a device"""
    h = ctypes.c_void_p()
    for bad in (-2, 2, 8):
        assert built.lib.dissc_hubert_create_ex(6, None, 0, None, 0, bad, ctypes.byref(h)) != 0
        assert b"precision" in built.lib.dissc_last_error()
    assert built.lib.dissc_hubert_precision(None) == 0
    try:  # nor does a default handle quietly run fp32 under an option value that names no arithmetic
        assert built.lib.dissc_set_option(b"enc_precision", 5) == 0
        assert built.lib.dissc_hubert_create_ex(6, None, 0, None, 0, -1, ctypes.byref(h)) != 0
        assert b"enc_precision" in built.lib.dissc_last_error()
    finally:
        built.lib.dissc_set_option(b"enc_precision", 0)


def test_hubert_encoder_precision_vocabulary(built):
    from dissc_amd.hubert import HubertEncoder
    sd = synth.synth_hubert_state_dict(1)
    with pytest.raises(ValueError):
        HubertEncoder(sd, precision="fp8")
    with pytest.raises(ValueError):
        HubertEncoder(sd, precision=1)
    for p in (None, "fp32", "split_bf16"):
        assert HubertEncoder(sd, n_layers=1, precision=p).precision == p


def test_command_lines_take_precision(built):
    sys.path.insert(0, os.path.join(ROOT, "data"))
    try:
        import encode
    finally:
        sys.path.pop(0)
    import convert
    need = ["--base_dir", "w", "--output_dir", "o", "--id_to_spkr", "i", "--target_speakers", "t"]
    for parser, base in ((encode.build_parser(), []), (convert.build_parser(), need)):
        assert parser.parse_args(base).precision is None
        assert parser.parse_args(base + ["--precision", "split_bf16"]).precision == "split_bf16"
        assert parser.parse_args(base + ["--precision", "fp32"]).precision == "fp32"
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--precision", "fp8"])


# ---- the model --------------------------------------------------------------------------------------------------------------
def _frame_err(x, ref):
    x, ref = x.double(), ref.double()
    return float(((x - ref).norm(dim=1) / ref.norm(dim=1)).max())


@pytest.fixture(scope="module")
def cases(golden_dir):
    """name -> (sd fp32, centres, wav [1, N], float64 dense, float64 units)"""
    out = {}
    sd, c = synth.synth_hubert_state_dict(6), torch.as_tensor(synth.synth_kmeans_centers())
    sd64 = hr.to_double(sd)
    for n, seed in IID_UTTS:
        wav = torch.from_numpy(synth.synth_waveform(n, seed=seed))[None]
        u64, d64 = hr.encode(sd64, c, wav)
        out[f"iid_{n}"] = (sd, c, wav, d64, u64)
    sd, c = synth.synth_hubert_state_dict(6, kind="trained_like"), torch.from_numpy(np.load(os.path.join(golden_dir, "hubert_trainedlike.npz"))["centers"])
    sd64 = hr.to_double(sd)
    for kind, n, seed in TL_UTTS:
        wav = torch.from_numpy(synth.synth_waveform(n, seed=seed, kind=kind))[None]
        u64, d64 = hr.encode(sd64, c, wav)
        out[kind] = (sd, c, wav, d64, u64)
    return out


def test_split_model_costs_more_than_fp32_on_every_fixture(cases):
    """the arithmetic is not free: on all five utterances the model's error is above the fp32 oracle's (and finite, and far
    below plain bf16's: within 100 x the fp32 oracle's)"""
    for name, (sd, c, wav, d64, u64) in cases.items():
        u32, d32 = hr.encode(sd, c, wav)
        um, dm = sm.encode(sd, c, wav)
        assert hr.F is torch.nn.functional
        e32, em = _frame_err(d32, d64), _frame_err(dm, d64)
        print(f"{name}: fp32 oracle {e32:.2e}, split model {em:.2e} ({em / e32:.1f} x); flips vs float64: fp32 oracle "
              f"{int((u32 != u64).sum())}, model {int((um != u64).sum())} of {len(u64)}")
        assert dm.dtype == torch.float32 and torch.isfinite(dm).all()
        assert e32 < em < 100 * e32, (name, e32, em)


def test_model_controls_on_the_iid_utterance(cases):
    """split := identity -> no worse than the fp32 oracle (the shim changes nothing but the arithmetic); lo halves dropped ->
    >= 100 x the split model (measured 640 x): a missing cross term cannot pass a bar of 2 x the model"""
    sd, c, wav, d64, _ = cases["iid_16000"]
    e32 = _frame_err(hr.encode(sd, c, wav)[1], d64)
    e_id = _frame_err(sm.encode(sd, c, wav, sp=sm.split_identity)[1], d64)
    e_sp = _frame_err(sm.encode(sd, c, wav)[1], d64)
    e_hi = _frame_err(sm.encode(sd, c, wav, sp=sm.split_hi_only)[1], d64)
    print(f"fp32 oracle {e32:.2e}, identity {e_id:.2e}, split {e_sp:.2e}, hi only {e_hi:.2e} ({e_hi / e_sp:.0f} x)")
    assert e_id <= e32
    assert e_hi >= 100 * e_sp


def test_split_halves_reassemble_the_operand():
    x = torch.from_numpy(np.random.RandomState(0).standard_normal(4096).astype(np.float32)) * 37.0
    hi, lo = sm.split(x)
    assert (hi.float().bfloat16().double() == hi).all() and (lo.float().bfloat16().double() == lo).all()
    assert float(((hi + lo) - x.double()).abs().max() / x.abs().max()) <= 2.0 ** -16


def test_oracle_global_is_restored_after_an_exception(cases):
    sd, c, wav, _, _ = cases["iid_16000"]
    bad = dict(sd)
    del bad["post_extract_proj.weight"]
    with pytest.raises(KeyError):
        sm.encode(bad, c, wav)
    assert hr.F is torch.nn.functional
