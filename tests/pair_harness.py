"""What every test of the one-launch residual pairs y = x + conv_1(lrelu(conv_d(lrelu(x)))) (dissc_respair1d; reference
sr/models.py:34-41) shares: the shipped option values and a context manager that restores them, data / float64 reference / launch,
forms tied by dissc_pair_info to the kernel mode 3 builds (and the pins of that entry), tile-edge lengths from that instance's own
tile, the one check body, the one trained-like per-layer loop, and the trained-like context (float64 oracle taps) built once per
process.
`lib` is the dissc_amd._lib module throughout."""
import ctypes
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

import tile_harness
import trained_like_cases as ttl

DEV = "cuda:0"
# the values the library ships with.  pair_f23: bit 0 C = 32, bit 1 C = 16 (4 / 8: their k = 3 pairs); pair_tc6: 1 C = 32 k = 7,
# 2 C = 32 k = 11; pairw_chv: the F(4,3) kernel's workgroup shape (DISSC_EXPERIMENTAL=1 builds only)
SHIPPED = {"pair_f23": 3, "pair_tc6": 3, "pair_f23_c64": 1, "pairw_chv": 2}
F23, TC6, F43 = 1, 2, 0  # DevPairW::form, as dissc_pair_info reports it


def experimental(lib):
    v = ctypes.c_int(0)
    return lib.lib.dissc_get_option(b"experimental", ctypes.byref(v)) == 0 and v.value == 1


def shipped(lib):
    """SHIPPED without the keys only a DISSC_EXPERIMENTAL=1 build knows"""
    return {k: v for k, v in SHIPPED.items() if k != "pairw_chv" or experimental(lib)}


def options(lib, **kv):
    """sets the given options; restores the SHIPPED values (not the previous ones, and nothing else) on exit.  Setting and
    restoring both go through lib.set_option: a key the library refuses raises DisscError, on exit too"""
    return tile_harness.options(lib, restore=shipped(lib), **kv)


PairInfo = namedtuple("PairInfo", "form tile")


def pair_info(lib, C, k, d):
    """what mode 3 builds for the shape under the current options (form, outputs a workgroup owns), or None: no instance"""
    form, tile = ctypes.c_int(-1), ctypes.c_int(-1)
    if lib.lib.dissc_pair_info(C, k, d, ctypes.byref(form), ctypes.byref(tile)) != 0:
        return None
    return PairInfo(form.value, tile.value)


# ---- the pins of dissc_pair_info (tests/test_pair_info.py holds the entry to them, tests/test_pair_info_c64_tc6.py holds them
# untouched by "pair_tc6_c64") ----
DILS = (1, 3, 5)
# (C, k, options, form, tile at d = 1 / 3 / 5)
PINS = [
    (16, 11, {}, F23, (500, 492, 468)),
    (32, 11, {}, TC6, (360, 360, 348)),
    (32, 11, {"pair_tc6": 0}, F23, (500, 492, 468)),
    (32, 11, {"pair_tc6": 1}, F23, (500, 492, 468)),  # (bit 0 is k = 7's)
    (32, 7, {}, TC6, (376, 372, 352)),
    (32, 7, {"pair_tc6": 1}, TC6, (376, 372, 352)),
    (64, 3, {}, F23, (252, 248, 248)),
]
# DISSC_EXPERIMENTAL=1 builds: the k = 3 instances of the C = 32 / 16 F(2,3) kernels (bits 4 / 8 of "pair_f23"), and the F(4,3)
# pair kernel (no constant outside its kernel file names its tile: 0) wherever the options leave no register-only form
PINS_EXPERIMENTAL = [
    (32, 3, {"pair_f23": 15}, F23, (508, 508, 508)),
    (16, 3, {"pair_f23": 15}, F23, (508, 508, 508)),
    (32, 7, {"pair_f23": 0}, F43, (0, 0, 0)),
    (32, 11, {"pair_f23": 0}, F43, (0, 0, 0)),
    (64, 3, {"pair_f23": 0}, F43, (0, 0, 0)),
    (64, 3, {"pair_f23_c64": 0}, F43, (0, 0, 0)),
]
# no instance in a default build
NONE_DEFAULT = [(32, 7, {"pair_f23": 0}), (32, 11, {"pair_f23": 0}), (64, 3, {"pair_f23": 0}), (64, 3, {"pair_f23_c64": 0}),
                (32, 7, {"pair_f23": 2, "pair_tc6": 15}), (32, 3, {"pair_f23": 15}), (16, 3, {"pair_f23": 15})]
# no instance in either build
NONE_ANYWHERE = [(16, 11, {"pair_f23": 1}), (16, 7, {"pair_tc6": 15}), (32, 3, {}), (16, 3, {}), (128, 3, {}), (256, 11, {}), (32, 5, {})]


class Form(namedtuple("Form", "name mode options expect_form", defaults=({}, None))):
    """one way through dissc_respair1d: its mode, the options it runs under and, for mode 3, the form that must come of them"""


DIRECT_PAIR = Form("direct pair", 1)           # the fused direct pair (respair.hip)
DIRECT_LAUNCHES = Form("direct launches", 0)   # two direct conv launches
TL_DIRECT, TL_FUSED = Form("direct", 0), Form("fused", 1)  # the same two under the names of trained_like_cases._check


def form_tile(lib, form, C, k, d):
    with options(lib, **form.options):
        info = pair_info(lib, C, k, d)
    assert info is not None and info.form == form.expect_form, (form.name, C, k, d, info)
    return info.tile


def edge_lengths(tile):
    """lengths that end beside the first and second tile boundary of an instance (none for a form that names no tile)"""
    return [tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile + 1] if tile else []


# the F(2,3) tests' fixed lengths: the first tile boundary - 1 / 0 / + 1 of every C = 16 / 32 instance (k = 11 and k = 3), whichever
# one runs; each test adds edge_lengths of its own instance
F23_LENGTHS = [2000, 1, 7, 255, 467, 468, 469, 491, 492, 493, 499, 500, 501, 507, 508, 509, 1023, 1999, 12]


def tile_windows(tile):
    """(first column, length) of the windows of a trained-like tap that end beside an instance's tile boundaries"""
    return ((0, tile - 1), (5, tile), (9, tile + 1), (2, 2 * tile + 1))


def data(C, k, lengths, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(len(lengths), C, ld, generator=g) * 2 - 1).to(DEV)
    for i, n in enumerate(lengths):
        x[i, :, n:] = float("nan")  # never read
    sc = 0.9 / (C * k) ** 0.5
    w1 = (torch.rand(C, C, k, generator=g) * 2 - 1) * sc
    w2 = (torch.rand(C, C, k, generator=g) * 2 - 1) * sc
    b1 = (torch.rand(C, generator=g) * 2 - 1) * 0.1
    b2 = (torch.rand(C, generator=g) * 2 - 1) * 0.1
    return x, w1, b1, w2, b2


def reference(x, w1, b1, w2, b2, lengths, k, d, slope=0.1):
    """float64, one utterance at a time on its own samples (the reference runs B = 1: zero "same" padding at every layer)"""
    out = torch.zeros_like(x, dtype=torch.float64)
    for i, n in enumerate(lengths):
        xi = x[i:i + 1, :, :n].double()
        t = F.conv1d(F.leaky_relu(xi, slope), w1.double().to(x.device), b1.double().to(x.device), padding=(k - 1) * d // 2, dilation=d)
        y = F.conv1d(F.leaky_relu(t, slope), w2.double().to(x.device), b2.double().to(x.device), padding=(k - 1) // 2)
        out[i, :, :n] = xi[0] + y[0]
    return out


def run_pair(lib, mode, x, w1, b1, w2, b2, lengths, k, d, epi=1, acc=None, slope=0.1, div=3.0):
    """x / acc on the device, weights on the host; y starts as the sentinel -7"""
    B, C, ld = x.shape
    y = torch.full_like(x, -7.0)
    ln = torch.as_tensor(lengths, dtype=torch.int32, device=DEV)
    a = None if acc is None else acc.clone()
    lib.check(lib.lib.dissc_respair1d(x.data_ptr(), w1.contiguous().data_ptr(), b1.contiguous().data_ptr(),
                                      w2.contiguous().data_ptr(), b2.contiguous().data_ptr(), y.data_ptr(),
                                      None if a is None else a.data_ptr(), ln.data_ptr(), B, C, k, d, ld, int(max(lengths)),
                                      ctypes.c_float(slope), epi, ctypes.c_float(div), mode, None), f"dissc_respair1d mode {mode}")
    return y if epi == 1 else a


def run_form(lib, form, x, w1, b1, w2, b2, lengths, k, d, **kw):
    """run_pair under the form's options, after dissc_pair_info has confirmed the kernel form they select"""
    with options(lib, **form.options):
        if form.expect_form is not None:
            info = pair_info(lib, x.shape[1], k, d)
            assert info is not None and info.form == form.expect_form, (form.name, x.shape[1], k, d, info)
        return run_pair(lib, form.mode, x, w1, b1, w2, b2, lengths, k, d, **kw)


def check_pair(lib, form, baseline_form, C, k, d, lengths, seed, *, max_err=1e-5, alone=(3, 5)):
    """ragged lengths (row 0 is the longest: 2000), NaN beyond every utterance and a sentinel behind it, against float64 and the
    baseline form (max <= max_err, rms <= max(3 x the baseline's, 1e-6)); batch independence of the rows `alone`; the MRF modes.
    Returns the form's output."""
    ld = 2000
    x, w1, b1, w2, b2 = data(C, k, lengths, ld, seed)
    ref = reference(x, w1, b1, w2, b2, lengths, k, d)
    y = run_form(lib, form, x, w1, b1, w2, b2, lengths, k, d)
    yb = run_form(lib, baseline_form, x, w1, b1, w2, b2, lengths, k, d)
    worst = worst_b = 0.0
    for i, n in enumerate(lengths):
        assert torch.isfinite(y[i, :, :n]).all(), (i, n)
        assert (y[i, :, n:] == -7.0).all(), f"utterance {i}: wrote beyond its {n} samples"
        worst = max(worst, (y[i, :, :n].double() - ref[i, :, :n]).abs().max().item())
        worst_b = max(worst_b, (yb[i, :, :n].double() - ref[i, :, :n]).abs().max().item())
    r = float(((y[0, :, :2000].double() - ref[0]) ** 2).mean().sqrt())
    rb = float(((yb[0, :, :2000].double() - ref[0]) ** 2).mean().sqrt())
    print(f"C={C} k={k} d={d}: {form.name} pair max err {worst:.2e} rms {r:.2e}; {baseline_form.name} {worst_b:.2e} / {rb:.2e}")
    assert not torch.equal(y[0], yb[0])  # (not the baseline's kernel)
    assert worst <= max_err and r <= max(3.0 * rb, 1e-6)
    for i in alone:
        one = run_form(lib, form, x[i:i + 1].clone(), w1, b1, w2, b2, lengths[i:i + 1], k, d)
        assert torch.equal(one[0, :, :lengths[i]], y[i, :, :lengths[i]]), i
    acc0 = torch.rand(len(lengths), C, ld, device=DEV)
    for epi in (2, 3, 4):
        a = run_form(lib, form, x, w1, b1, w2, b2, lengths, k, d, epi=epi, acc=acc0)
        for i, n in enumerate(lengths):
            want = y[i, :, :n] if epi == 2 else acc0[i, :, :n] + y[i, :, :n]
            if epi == 4:
                # on the CPU like the reference's xs / num_kernels: a true division (torch's GPU kernel for a scalar divisor
                # multiplies by the reciprocal; the HIP kernels use __fdiv_rn)
                want = (want.cpu() / 3.0).to(DEV)
            assert torch.equal(a[i, :, :n], want), (epi, i)
            assert torch.equal(a[i, :, n:], acc0[i, :, n:])
    return y


def assert_no_instance(lib, C, k, opts):
    """under these options mode 3 has no register-only form for the shape: it refuses and writes nothing (a DISSC_EXPERIMENTAL=1
    build carries the F(4,3) pair kernel, which mode 3 then builds where that has an instance)"""
    lengths = [64]
    x, w1, b1, w2, b2 = data(C, k, lengths, 64, seed=3)
    with options(lib, **opts):
        info = pair_info(lib, C, k, 1)
        assert (info is None) == (not experimental(lib)) and (info is None or info.form == F43), info
        y = torch.full_like(x, -7.0)
        ln = torch.as_tensor(lengths, dtype=torch.int32, device=DEV)
        rc = lib.lib.dissc_respair1d(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y.data_ptr(), None,
                                     ln.data_ptr(), 1, C, k, 1, 64, 64, ctypes.c_float(0.1), 1, ctypes.c_float(3.0), 3, None)
        assert (rc != 0) == (info is None)
        assert rc == 0 or (y == -7.0).all()


# ------------------------------------------------------------------------------------------------------------------------
# trained-like data (tests/trained_like_cases.py: the rows, metrics and bars of tests/test_gpu_trained_like.py)
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tl_context():
    """the trained-like checkpoint and the float64 oracle's layer taps on a T = 99 utterance: built once per process, read-only"""
    from dissc_amd import _lib
    from oracle import generator_ref as gr
    import synthdata as synth
    sd = synth.synth_generator_state_dict(seed=0, kind="trained_like")
    folded = gr.fold_state_dict(sd)
    w64 = gr.to_double(folded)
    code, f0, spkr, _ = synth.synth_generator_inputs(1, 99, seed=199, kind="trained_like")
    x = gr.embed_concat(w64, torch.from_numpy(code), torch.from_numpy(f0), torch.from_numpy(spkr))
    taps, conv_taps = {}, {}
    gr.generator_forward(w64, synth.VCTK_CONFIG, x, taps=taps, conv_taps=conv_taps)
    # the pre-activation inputs (the kernels apply the leaky ReLU on load), as the fp32 data a kernel is fed
    inp = {k[:-2]: v[0].float() for k, v in conv_taps.items() if k.endswith(".x")}
    inp["conv_pre"] = x[0].float()
    for i in range(5):
        inp[f"ups.{i}"] = (taps["conv_pre"] if i == 0 else taps[f"mrf{i - 1}"])[0].float()
    return dict(lib=_lib.lib, _lib=_lib, gr=gr, synth=synth, sd=sd, folded=folded, inp=inp, experimental=experimental(_lib))


def register_only_forms(lib, C, k, d):
    """the register-only forms mode 3 can build for the shape: the one the shipped options select first (the default plan's), then
    the F(2,3) one "pair_tc6" = 0 leaves a six-point shape with"""
    forms = []
    for opts in ({}, {"pair_tc6": 0}):
        with options(lib, **opts):
            info = pair_info(lib, C, k, d)
        name = {F23: "F(2,3)", TC6: "TC6"}.get(info.form) if info is not None else None
        if name is not None and name not in [f.name for f in forms]:
            forms.append(Form(name, 3, opts, info.form))
    return forms


def trained_like_pair_layer(tl, C, k, d, p, m, forms, plan_form, unit_widths, seed, extra_rows=()):
    """pair m (dilation d) of ResBlock p through every form, on its float64-oracle input (a) and on (b): the adversarial rows
    (bursts after silence at every offset modulo unit_widths, spikes, ragged lengths) and windows of the tap of the
    (first column, length) in extra_rows; at m == 2 also the MRF epilogues (2: store, 3: accumulate, 4: accumulate / 3) of the
    chain's last pair.  Returns the broken bars of trained_like_cases._check: TD_RMS for plan_form, TD_CH and LEAK for all."""
    lib, folded = tl["_lib"], tl["folded"]
    w1, b1 = folded[f"{p}.convs1.{m}.weight"], folded[f"{p}.convs1.{m}.bias"]
    w2, b2 = folded[f"{p}.convs2.{m}.weight"], folded[f"{p}.convs2.{m}.bias"]
    tap = tl["inp"][f"{p}.convs1.{m}"]
    rows = [(tap, None)] + ttl._adversarial_rows(tap, unit_widths, seed=seed)
    rows += [(tap[:, c0:c0 + ln].clone(), None) for c0, ln in extra_rows]
    x, lens = ttl._batch(rows)
    xd = x.to(DEV)
    for i, n in enumerate(lens):
        xd[i, :, n:] = float("nan")  # never read
    pad = (k - 1) * d // 2 + (k - 1) // 2
    unit = F.leaky_relu(x, ttl.SLOPE).abs().amax((1, 2))
    s1 = float(w1.double().abs().sum((1, 2)).max())
    wsum = w2.double().abs().sum((1, 2)) * s1  # the gain of the pair's path from a loud input, per output channel
    refs = [ttl._ref_pair(x[i, :, :n], w1, b1, w2, b2, k, d, torch.float64) for i, n in enumerate(lens)]
    res, outs = {}, {}
    for form in [None] + forms:
        if form is None:
            name, y = "cpu", [ttl._ref_pair(x[i, :, :n], w1, b1, w2, b2, k, d, torch.float32) for i, n in enumerate(lens)]
        else:
            name, yb = form.name, run_form(lib, form, xd, w1, b1, w2, b2, lens, k, d, slope=ttl.SLOPE).cpu()
            for i, n in enumerate(lens):
                assert (yb[i, :, n:] == -7.0).all(), (p, m, name, i, "wrote beyond the utterance")
                assert torch.isfinite(yb[i, :, :n]).all(), (p, m, name, i)
            y = [yb[i, :, :n] for i, n in enumerate(lens)]
            outs[name] = yb
            if m == 2:  # exactly the pair's output stored / accumulated
                acc0 = torch.rand(x.shape, generator=torch.Generator().manual_seed(m))
                for epi in (2, 3, 4):
                    a = run_form(lib, form, xd, w1, b1, w2, b2, lens, k, d, slope=ttl.SLOPE, epi=epi, acc=acc0.to(DEV)).cpu()
                    for i, n in enumerate(lens):
                        want = yb[i, :, :n] if epi == 2 else acc0[i, :, :n] + yb[i, :, :n]
                        if epi == 4:
                            want = want / 3.0
                        assert torch.equal(a[i, :, :n], want), (p, name, epi, i)
                        assert torch.equal(a[i, :, n:], acc0[i, :, n:]), (p, name, epi, i)
        acc_a, acc_b = ttl._Acc(C), ttl._Acc(C)
        for i, (r, loud) in enumerate(rows):
            if i == 0:
                acc_a.add(y[i], refs[i])
            else:
                acc_b.add(y[i], refs[i], loud, pad, float(unit[i]) * wsum * ttl.U)
        res[name] = (acc_a.metrics(), acc_b.metrics())
    for form in forms:
        assert form.mode != 3 or not torch.equal(outs[form.name], outs["direct"]), (p, m, form.name, "the form did not run")
    return ttl._check(f"{p}.pair{m}", [f.name for f in forms], res, plan_form)
