"""The inference predictors (csrc/predictors.hip, dissc_amd/predictors.py) against float64 at tile-edge lengths.

One ragged batch of the edge rows of tests/predictor_cases.py per (kind, weight set) is held to the bars of that file --
e_gpu <= K max(e_torch_fp32, 2^-24 rms(ref64)) over all frames, the worst utterance and the edge frames -- with iid and with
trained-like BatchNorm statistics (the per-row affine epilogue: alpha up to 316 gamma, gamma over decades), the pitch heads also
through the two derived dicts that need no frame excluded.  The bits of that batch are then carried to every tile the launch rule
can pick: each row alone (B = 1), a 70-row batch of repeats and empty rows, a middle batch; the tile ids are asked of
dissc_conv_info and held to tests/plan_rules.py.  Further: a workspace poisoned with NaN, T = 850 (the last row of pe.pe), a
changed length normalisation on a live handle, the carry-over rounding on 1 / 64 / 65 / 130 rows, infer_batch against its stages.
Every predictor launch but infer_batch's goes through run(), which refuses a (B, Tmax) the tile test does not know.
Measured ratios: profiles/predictor_error.md."""
import functools

import numpy as np
import pytest
import torch

import plan_rules as R
import predictor_cases as C
from tile_harness import DEV, lib  # noqa: F401  (lib: the module fixture that builds the library)

pytestmark = pytest.mark.gpu

PITCH = [k for k in C.KINDS if k != "len"]
KEY = {True: "out", False: "out_hz"}

# Exceptions to K = 4 (predictor_cases.K; the rule of tests/test_gpu_conv_strided_grad.py's K_EXC): per (kind, weight set, case,
# bar), K = 2 x the measured worst ratio rounded up, never above predictor_cases.K_CAP = 19; the measured ratio stands beside it.
# Measured on an MI355X (profiles/predictor_error.md): every ratio of this file is at most 3.99 except
#   "new" / iid, frames 840-849 of the 850-frame row, natural dict: 5.33 -> 11.  The statistic rests on the 6 voiced frames of
#   those 10 (e_gpu 1.10e-6, torch 2.06e-7); the same row cut into its 66 windows of 10 frames with a voiced one gives ratios of
#   median 2.65, 90th percentile 8.7, with 15 windows above 5.33, while the row as a whole is at 2.09 and its 85-frame tenths at
#   1.1 - 3.2 with no trend towards the end: a ten-frame window is that noisy anywhere, the last rows of pe.pe do not stand out.
K_EXC = {("new", "iid", "T850/natural", b): 11.0 for b in "abc"}  # measured 5.33


def bars(kind, weights, case):
    return tuple(K_EXC.get((kind, weights, case, b), C.K) for b in "abc")


# ---- (B, Tmax) of every launch, and the tile each layer takes there (worked from plan_rules.rule_pick; asserted below) -----------
#          (B, Tmax): (128-row layers, 256-row head)
PLAN = {"pitch": {(20, 850): (2, 0), (1, None): (10, 10), (70, 513): (1, 0), (20, 385): (10, 2)},
        "len": {(19, 513): (10, None), (1, None): (10, None), (70, 513): (1, None), (40, 513): (2, None)}}
HEAD16 = R.DEFAULT16[16]  # the 128 -> 1 length head: one useful row in a tile of the 16-row family


def model(kind, weights, exposed="natural"):
    return _model(kind, weights, exposed)


@functools.lru_cache(maxsize=None)
def _model(kind, weights, exposed):
    from dissc_amd import predictors as P
    if kind == "len":
        m = P.LenPredictor(C.N_TOKENS, C.N_SPEAKERS)
        m.norm_mean, m.norm_std = C.LEN_NORM
    else:
        mean, std = C.pitch_stats()
        m = (P.PitchPredictor if kind == "new" else P.PitchPredictorBase)(C.N_TOKENS, C.N_SPEAKERS, id2pitch_mean=mean, id2pitch_std=std)
    m.to(DEV)
    m.load_state_dict(C.EXPOSED[exposed](C.state_dict(kind, weights)))
    return m.eval()


def run(m, kind, seq, spk, lengths, norm=True):
    """one launch -> float32 numpy [B, Tmax]; lengths None: the uniform call (lengths = NULL)"""
    B, T = seq.shape
    plan = PLAN["len" if kind == "len" else "pitch"]
    assert (B, T) in plan or (B == 1 and T <= C.T_PE), ("a (B, Tmax) the tile test does not cover", B, T)
    out = m(seq, spk, lengths=lengths) if kind == "len" else m.infer_freq(seq, spk, norm, lengths=lengths)
    assert tuple(out.shape) == (B, T) and out.dtype == torch.float32
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def edge_out(kind, weights, exposed="natural", norm=True):
    """the edge batch of (kind, weight set), once per module"""
    return _edge_out(kind, weights, exposed, norm)


@functools.lru_cache(maxsize=None)
def _edge_out(kind, weights, exposed, norm):
    lengths, seqs, spk = C.rows(kind)
    return run(model(kind, weights, exposed), kind, *C.batch(seqs, spk, range(len(lengths))), norm=norm)


def check_padding(got, lengths, what):
    assert np.isfinite(got).all(), (what, "not finite")
    for b, n in enumerate(lengths):
        assert not bits(got[b, n:]).any(), (what, "the output beyond a length is not exactly 0", b, n)


def hold(got, ref, key, lengths, tag, k, natural=False, frames=None):
    m = C.measure(got, ref, key, lengths, natural_pitch=natural, frames=frames)
    print(C.line(tag, m))
    return [(tag, v) for v in C.violations(m, k)]


# ---- the edge batch against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", C.WEIGHTS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_edge_batch_against_float64(lib, kind, weights):
    lengths, _, _ = C.rows(kind)
    ref = C.reference(kind, weights)
    bad = []
    for norm in ((True,) if kind == "len" else (True, False)):
        got = edge_out(kind, weights, "natural", norm)
        key = "lens" if kind == "len" else KEY[norm]
        assert got.shape == (len(lengths), max(lengths))
        check_padding(got, lengths, (kind, weights, key))  # (a row of length 0 is all zero)
        bad += hold(got, ref, key, lengths, f"edge {kind} {weights} {key}", bars(kind, weights, key), natural=kind != "len")
    assert not bad, bad


@pytest.mark.parametrize("exposed", ["reg_exposed", "cls_exposed"])
@pytest.mark.parametrize("weights", C.WEIGHTS)
@pytest.mark.parametrize("kind", PITCH)
def test_pitch_heads_exposed_against_float64(lib, kind, weights, exposed):
    """no frame excluded: reg_exposed puts the regression out at every frame; cls_exposed puts out max(cls, 0), continuous through
    zero, from rows 0-127 and 128-255 of the stacked head on the same weights"""
    lengths, _, _ = C.rows(kind)
    got = edge_out(kind, weights, exposed)
    check_padding(got, lengths, (kind, weights, exposed))
    if exposed == "cls_exposed":
        assert (got >= 0).all()
    bad = hold(got, C.reference(kind, weights, exposed), "out", lengths, f"edge {kind} {weights} {exposed}", bars(kind, weights, exposed))
    assert not bad, bad


@pytest.mark.parametrize("weights", C.WEIGHTS)
def test_last_rows_of_the_positional_encoding(lib, weights):
    """T = 850 for "new": frames 840-849 read the last rows of pe.pe"""
    lengths, _, _ = C.rows("new")
    frames = np.zeros((len(lengths), C.T_PE), dtype=bool)
    frames[lengths.index(C.T_PE), 840:] = True
    bad = []
    for exposed, natural in (("natural", True), ("reg_exposed", False)):
        bad += hold(edge_out("new", weights, exposed), C.reference("new", weights, exposed), "out", lengths,
                    f"T850 new {weights} {exposed} frames 840-849", bars("new", weights, "T850/" + exposed), natural=natural, frames=frames)
    assert not bad, bad


# ---- the workspace is torch.empty and reused ----------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", C.WEIGHTS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_poisoned_workspace(lib, kind, weights):
    m = model(kind, weights)
    first = edge_out(kind, weights)
    assert m._ws is not None and m._ws.dtype == torch.uint8
    m._ws.fill_(0xFF)  # every float of it a NaN
    ptr = m._ws.data_ptr()
    lengths, seqs, spk = C.rows(kind)
    again = run(m, kind, *C.batch(seqs, spk, range(len(lengths))))
    assert m._ws.data_ptr() == ptr, "the workspace was not reused"
    assert np.array_equal(bits(again), bits(first)), (kind, weights, "stale workspace contents reached the output")


# ---- alone = batch = repeated row, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", C.WEIGHTS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_alone_batch_and_repeated_rows_give_the_same_bits(lib, kind, weights):
    lengths, seqs, spk = C.rows(kind)
    m = model(kind, weights)
    for norm in ((True,) if kind == "len" else (True, False)):
        full = edge_out(kind, weights, "natural", norm)
        if norm:
            for i, n in enumerate(lengths):  # B = 1, lengths = NULL: the command-line tools
                if n:
                    seq, s, _ = C.batch(seqs, spk, [i])
                    one = run(m, kind, seq, s, None, norm)
                    assert np.array_equal(bits(one[0]), bits(full[i, :n])), (kind, weights, "alone", n)
        for name, index, shape in (("70 rows", C.big_batch_index(kind), (70, 513)),
                                   ("middle", C.mid_batch_index(kind), (40, 513) if kind == "len" else (20, 385))):
            seq, s, ln = C.batch(seqs, spk, index)
            got = run(m, kind, seq, s, ln, norm)
            assert got.shape == shape  # (513 is no multiple of 4: the row stride is 516)
            check_padding(got, [lengths[i] for i in index], (kind, weights, name))
            for b, i in enumerate(index):
                n = lengths[i]
                assert np.array_equal(bits(got[b, :n]), bits(full[i, :n])), (kind, weights, name, "row", b, "length", n)


# ---- every tile the rule can pick has run -------------------------------------------------------------------------------------
def test_every_tile_of_the_step_lists_has_run(lib):
    ran = {"len": {128: set(), 16: set()}, "pitch": {128: set(), 256: set()}}
    for group, plan in PLAN.items():
        for (B, T), (id128, id256) in plan.items():
            for Tmax in ([T] if T else [n for n in C.rows("new" if group == "pitch" else "len")[0] if n]):
                got = {}
                for cin, cout in ((64, 128), (128, 128), (128, 256), (128, 1)):
                    (g,) = lib.conv_info(cin, cout, 3, 1, 1, B, Tmax)
                    got[cin, cout] = (g["family"], g["cfg"])
                assert got[64, 128] == got[128, 128] == (32, id128) == (32, R.rule_pick(128, B, Tmax)), (group, B, Tmax, got)
                ran[group][128].add(id128)
                if group == "pitch":
                    assert got[128, 256] == (32, id256) == (32, R.rule_pick(256, B, Tmax)), (group, B, Tmax, got)
                    ran[group][256].add(id256)
                else:
                    assert got[128, 1] == (16, HEAD16) and R.TILES16[HEAD16] == (16, 256), (group, B, Tmax, got)
                    ran[group][16].add(HEAD16)
            print(f"PE tiles {group:5s} B {B:3d} Tmax {T or 'every edge length'}: 128-row layers id {id128}, "
                  + (f"256-row head id {id256}" if group == "pitch" else f"128 -> 1 head 16-row family id {HEAD16}"))
    assert ran["pitch"][128] == ran["len"][128] == set(R.STEPS[128]) == {1, 2, 10}
    assert ran["pitch"][256] == set(R.STEPS[256]) == {0, 2, 10} and ran["len"][16] == {HEAD16}


# ---- a changed length normalisation on a live handle --------------------------------------------------------------------------
@pytest.mark.parametrize("weights", C.WEIGHTS)
def test_changed_length_normalisation_on_a_live_handle(lib, weights):
    from dissc_amd import predictors as P
    lengths, seqs, spk = C.rows("len")
    args = C.batch(seqs, spk, range(len(lengths)))
    m = P.LenPredictor(C.N_TOKENS, C.N_SPEAKERS).to(DEV)
    m.load_state_dict(C.state_dict("len", weights))
    m.norm_mean, m.norm_std = C.LEN_NORM
    first = run(m, "len", *args)
    assert np.array_equal(bits(first), bits(edge_out("len", weights)))
    handle = m._handle.value
    m.norm_mean, m.norm_std = C.LEN_NORM_2
    second = run(m, "len", *args)
    assert m._handle.value == handle and not np.array_equal(bits(second), bits(first))
    check_padding(second, lengths, ("len", weights, "second pair"))
    bad = hold(second, C.reference("len", weights, "natural", True), "lens", lengths, f"norm2 len {weights} lens", bars("len", weights, "norm2"))
    m.norm_mean, m.norm_std = C.LEN_NORM
    assert np.array_equal(bits(run(m, "len", *args)), bits(first)), "the first pair set back does not give the first call's bits"
    assert not bad, bad


# ---- carry-over rounding: 64 rows per workgroup -------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_len_carryover_correction_rows(lib, B):
    from dissc_amd import predictors as P
    from oracle import predictors_ref as pr
    rs = np.random.RandomState(100 + B)
    L = 300
    n = rs.randint(0, L + 1, B)
    n[0] = L
    if B > 1:
        n[[1, B - 1]] = [0, 1]
    x = rs.uniform(-2.0, 8.0, (B, L))
    pick = rs.rand(B, L)
    x = np.where(pick < 0.25, np.round(x) + 0.5, x)              # exact .5 ties (torch.round: half to even)
    x = np.where((pick >= 0.25) & (pick < 0.35), rs.uniform(0.0, 1.0, (B, L)), x)  # below the clamp
    x = np.where((pick >= 0.35) & (pick < 0.37), 1e4, x)
    x = np.where((pick >= 0.37) & (pick < 0.38), 1e4 + 0.5, x)
    x = torch.from_numpy(x.astype(np.float32))
    assert (x < 0).any() and (x == 1e4).any() and ((x - x.floor()) == 0.5).any()
    got, totals = P.len_carryover_correction(x.to(DEV), torch.from_numpy(n.astype(np.int32)).to(DEV))
    got, totals = got.cpu(), totals.cpu()
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, L)
    for b in range(B):
        k = int(n[b])
        assert not got[b, k:].any(), (B, b, "wrote beyond a row's count")
        if k == 0:
            assert int(totals[b]) == 0
            continue
        want = pr.len_carryover_correction(x[b:b + 1, :k])
        assert torch.equal(got[b, :k].long(), want.long()), (B, b, k)
        assert int(totals[b]) == int(want.clamp(min=0).sum()), (B, b, k)


# ---- infer_batch = its stages, and F0 given those units against float64 -------------------------------------------------------
@pytest.mark.parametrize("kind", PITCH)
def test_infer_batch_on_the_edge_rows(lib, kind):
    """the trained-like models.  Units and integer lengths are those of running the stages one by one through the same module; F0
    meets the bars given those units (the rounding of the lengths is not compared across precisions)"""
    from dissc_amd import predictors as P
    lengths, seqs, spk = C.rows(kind)
    index = [i for i, n in enumerate(lengths) if n <= 513]
    units, s, ln = C.batch(seqs, spk, index)
    lm, pm = model("len", "trained_like"), model(kind, "trained_like")
    units, ln = units.to(DEV), ln.to(DEV)
    r = P.infer_batch(units, ln, s, lm, pm, norm_pitch=True)
    vals, _, n = P.dedup(units, ln)
    li, tot = P.len_carryover_correction(lm(vals, s, lengths=n).contiguous(), n)
    ex = P.expand(vals, li, n, int(tot.max()))
    assert torch.equal(r["units"], ex) and torch.equal(r["lengths"], tot) and torch.equal(r["lens_int"], li) and torch.equal(r["n"], n)
    tot = [int(t) for t in tot.cpu()]
    assert r["totals"].tolist() == tot and max(tot) <= C.T_PE and tot[lengths.index(0)] == 0 and min(tot[1:]) > 0
    f0 = r["f0"].cpu().numpy()
    assert f0.shape == (len(index), max(tot))
    check_padding(f0, tot, (kind, "infer_batch"))
    sd, ex = C.state_dict(kind, "trained_like"), ex.cpu()
    ref = [None if t == 0 else tuple({k: v.double().numpy() for k, v in C.forward(kind, sd, ex[b, :t], spk[i], dt).items() if k != "h"}
                                      for dt in (torch.float64, torch.float32)) for b, (i, t) in enumerate(zip(index, tot))]
    bad = hold(f0, ref, "out", tot, f"infer_batch {kind} trained_like out", bars(kind, "trained_like", "infer_batch"), natural=True)
    assert not bad, bad
