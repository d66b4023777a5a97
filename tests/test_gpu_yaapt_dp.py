"""The YAAPT device stages on constructed inputs that take every branch (tests/yaapt_dp_cases.py; what the cases cover and
why they may be compared exactly is checked without a GPU in tests/test_yaapt_dp_cases_cpu.py): the spec-track and
final-track kernels of csrc/yaapt_dp.hip against dissc_amd.f0's numpy stages, the NCCF kernel's candidate logic against
oracle crs_corr / cmp_rate, and the whole tracker on utterances of a few frames.  Every test prints the largest deviation
it saw against each of its bars."""
import warnings

import numpy as np
import pytest
import torch

import yaapt_dp_cases as C
from yaapt_cases import voiced

pytestmark = pytest.mark.gpu
F_SMALL = 520
NAN = float("nan")


@pytest.fixture(scope="module")
def trackers():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd.f0 import YaaptTracker
    made = {}

    def get(median=7):
        if median not in made:
            made[median] = YaaptTracker(device="cuda:0") if median == 7 else YaaptTracker(device="cuda:0", median_value=median)
        return made[median]
    return get


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():   # scipy.signal.medfilt says so when the window is wider than the data
        warnings.simplefilter("ignore")
        yield


def _poison(trk, B, F):
    """the cached workspace of the DP kernels, every byte 0xFF (NaN as a double, -1 as an int, state 255 as a back-pointer)"""
    with torch.cuda.device(trk.device):
        trk._track_workspace(B, F)
    trk._tws.fill_(0xFF)


def _bits(t):
    return t.reshape(-1).contiguous().view(torch.uint8).cpu()


# ---------------------------------------------------------------------------------------------------------------
# spec-track
# ---------------------------------------------------------------------------------------------------------------
def _launch_spec(trk, cases, F):
    B = len(cases)
    en, cp, cm = torch.full((B, F), NAN), torch.full((B, F, 4), NAN), torch.full((B, F, 4), NAN)
    for b, c in enumerate(cases):
        f = c["f"]
        assert f <= F and c["n_tda"] <= f
        en[b, :f], cp[b, :f], cm[b, :f] = (torch.from_numpy(c[k]) for k in ("energy", "cand_pitch", "cand_merit"))
    s = {"energy": en.cuda(), "cand_pitch": cp.cuda(), "cand_merit": cm.cuda()}
    _poison(trk, B, F)
    st = trk.spec_track(s, [c["f"] for c in cases], [c["n_tda"] for c in cases])
    torch.cuda.synchronize()
    return st


SPEC_OUT = ("en_norm", "vuv", "spec", "spec_std", "lag_min", "lag_max")


def _check_spec(st, b, c, worst):
    f, t, name = c["f"], c["n_tda"], c["name"]
    got = {k: st[k][b].cpu().numpy() for k in SPEC_OUT}
    want = C.spec_reference(c)
    np.testing.assert_allclose(got["en_norm"][:f], want["en_norm"], rtol=1e-12, atol=0, err_msg=name)
    np.testing.assert_array_equal(got["vuv"][:f].astype(bool), want["vuv"], err_msg=name)
    np.testing.assert_allclose(got["spec"][:f], want["spec"], rtol=1e-9, atol=0, err_msg=name)
    if f == 0:
        assert float(got["spec_std"]) == 1.0, name
    else:
        assert abs(float(got["spec_std"]) - want["spec_std"]) <= 1e-9 * want["spec_std"], name
    np.testing.assert_array_equal(got["lag_min"][:t], want["lag_min"], err_msg=name)
    np.testing.assert_array_equal(got["lag_max"][:t], want["lag_max"], err_msg=name)
    assert (got["lag_min"][t:] == 1).all() and (got["lag_max"][t:] == 2).all(), name
    assert not got["en_norm"][f:].any() and not got["vuv"][f:].any() and not got["spec"][f:].any(), name
    if f:
        nz = want["en_norm"] != 0
        worst["en_norm rel"] = max(worst.get("en_norm rel", 0.0), float(np.max(np.abs(got["en_norm"][:f] - want["en_norm"])[nz] /
                                                                              want["en_norm"][nz], initial=0.0)))
        worst["spec rel"] = max(worst.get("spec rel", 0.0), float(np.max(np.abs(got["spec"][:f] - want["spec"]) / want["spec"])))
        worst["spec_std rel"] = max(worst.get("spec_std rel", 0.0), abs(float(got["spec_std"]) - want["spec_std"]) / want["spec_std"])


def test_spec_track_takes_every_branch_like_the_host_stages(trackers):
    """all constructed spec-track cases of one median_value in one ragged launch (F = 520, NaN beyond each row's frames,
    workspace poisoned): en_norm rtol 1e-12, vuv equal, spec and spec_std 1e-9, lag ranges equal on [0, n_tda) and 1 / 2
    beyond, zeros on [f, F), spec_std == 1 for f == 0; each row launched alone gives the batch's bits"""
    worst = {}
    for median in C.MEDIANS:
        cases = [c for c in C.spec_cases() if c["median"] == median]
        assert cases and (median != 7 or len(cases) >= 30)
        trk = trackers(median)
        st = _launch_spec(trk, cases, F_SMALL)
        for b, c in enumerate(cases):
            _check_spec(st, b, c, worst)
        for b, c in enumerate(cases):
            alone = _launch_spec(trk, [c], F_SMALL)
            for k in SPEC_OUT:
                assert torch.equal(_bits(alone[k][0]), _bits(st[k][b])), (c["name"], k)
    print("spec-track, largest deviation:", {k: f"{v:.2e}" for k, v in worst.items()}, "(lag ranges, vuv: equal)")


# ---------------------------------------------------------------------------------------------------------------
# final-track
# ---------------------------------------------------------------------------------------------------------------
def _launch_final(trk, cases, F):
    B = len(cases)
    tabs = {k: torch.full((B, F, 3), NAN) for k in ("tp1", "tm1", "tp2", "tm2")}
    en, sp = torch.full((B, F), NAN, dtype=torch.float64), torch.full((B, F), NAN, dtype=torch.float64)
    vuv = torch.full((B, F), 0xFF, dtype=torch.uint8)
    std = torch.zeros(B, dtype=torch.float64)
    for b, c in enumerate(cases):
        t = c["t"]
        assert t <= F
        for k in tabs:
            tabs[k][b, :t] = torch.from_numpy(c[k])
        en[b, :t], sp[b, :t], vuv[b, :t] = torch.from_numpy(c["en_norm"]), torch.from_numpy(c["spec"]), torch.from_numpy(c["vuv"])
        std[b] = c["spec_std"]
    st = {"en_norm": en.cuda(), "vuv": vuv.cuda(), "spec": sp.cuda(), "spec_std": std.cuda(),
          "n_tda": torch.tensor([c["t"] for c in cases], dtype=torch.int32).cuda()}
    tabs = {k: v.cuda() for k, v in tabs.items()}
    _poison(trk, B, F)
    f0 = trk.final_track_device(st, (tabs["tp1"], tabs["tm1"]), (tabs["tp2"], tabs["tm2"]))
    torch.cuda.synchronize()
    return f0


def _check_final(f0, b, c):
    got, t = f0[b].cpu().numpy(), c["t"]
    want = np.float32(C.final_reference(c))
    differ = int((got[:t] != want).sum())
    assert differ == 0, (c["name"], differ, np.nonzero(got[:t] != want)[0][:8], got[:t][got[:t] != want][:8], want[got[:t] != want][:8])
    assert not got[t:].any(), c["name"]
    return differ


def test_final_track_takes_every_branch_like_the_host_stages(trackers):
    """all constructed final-track cases of one median_value in one ragged launch: the result is a selection among the
    inputs, so it equals np.float32(reference) bit for bit, and is zero on [t, F); each row alone gives the batch's bits"""
    frames = 0
    for median in C.MEDIANS:
        cases = [c for c in C.final_cases() if c["median"] == median]
        assert cases
        trk = trackers(median)
        f0 = _launch_final(trk, cases, F_SMALL)
        for b, c in enumerate(cases):
            _check_final(f0, b, c)
            frames += c["t"]
        for b, c in enumerate(cases):
            assert torch.equal(_bits(_launch_final(trk, [c], F_SMALL)[0]), _bits(f0[b])), c["name"]
    print(f"final-track: 0 of {frames} frames differ from np.float32(reference)")


# ---------------------------------------------------------------------------------------------------------------
# back-pointers outside LDS
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_back_pointers_in_the_workspace(trackers, which):
    """F = 38 401, B = 2 (row 0 full length, row 1 of 300 frames: the per-row offset into the byte workspace): both kernels
    keep their back-pointers in the workspace.  F = 19 201, B = 1: spec-track in LDS, final-track in the workspace.  Same
    bars as the small cases."""
    F, spec, final = C.big_launches()[which]
    assert F == (C.F_SPEC_WS, C.F_FINAL_WS)[which] and len(spec) == len(final) == (2, 1)[which]
    trk = trackers(7)
    worst = {}
    st = _launch_spec(trk, spec, F)
    for b, c in enumerate(spec):
        _check_spec(st, b, c, worst)
    f0 = _launch_final(trk, final, F)
    for b, c in enumerate(final):
        _check_final(f0, b, c)
    trk._tws = None   # 12 MB of workspace: not kept for the rest of the session
    print(f"F = {F}: spec-track largest deviation", {k: f"{v:.2e}" for k, v in worst.items()},
          f"; final-track 0 of {sum(c['t'] for c in final)} frames differ")


# ---------------------------------------------------------------------------------------------------------------
# NCCF candidate logic
# ---------------------------------------------------------------------------------------------------------------
def test_nccf_candidates_on_constructed_frames(trackers):
    """one launch over the constructed frames (NaN beyond each row's n_samples, degenerate lag ranges included): phi within
    5e-4 of oracle crs_corr on every frame, candidates on every frame whose decisions hold margin (d): pitch rtol 1e-5,
    merit atol 1e-3; degenerate ranges and the frames beyond a row's count give pitch 0 and merit 0.001"""
    trk = trackers(7)
    case = C.nccf_case()
    kept = C.margins(case)["kept"]
    rows = case["rows"]
    B = len(rows)
    sig = torch.full((B, C.NCCF_N), NAN)
    for b, r in enumerate(rows):
        sig[b, :r["ns"]] = torch.from_numpy(r["sig"][:r["ns"]])
    ns = torch.tensor([r["ns"] for r in rows], dtype=torch.int32).cuda()
    lag = np.array([r["lags"] for r in rows], dtype=np.int32)
    pit, mer, phi = (t.cpu().numpy() for t in trk.nccf(sig.cuda(), ns, lag[:, :, 0], lag[:, :, 1], want_phi=True))
    none_p, none_m = np.zeros(3, np.float32), np.full(3, np.float32(0.001))
    worst = {"phi abs": 0.0, "pitch rel": 0.0, "merit abs": 0.0}
    checked = 0
    for b, r in enumerate(rows):
        nfr = C.nccf_frames(r)
        for fr in range(C.NCCF_F):
            where = (r["name"], fr, r["lags"][fr])
            if fr >= nfr:
                assert np.array_equal(pit[b, fr], none_p) and np.array_equal(mer[b, fr], none_m), where
                continue
            want_phi, want_p, want_m = C.nccf_frame_reference(r, fr)
            err = float(np.abs(phi[b, fr] - want_phi).max())
            worst["phi abs"] = max(worst["phi abs"], err)
            assert err <= 5e-4, (where, err)
            if "nccf:no_peak" in C.nccf_frame_info(r, fr)[0] and kept[(r["name"], fr)]:
                assert not want_p.any()
                assert np.array_equal(pit[b, fr], none_p) and np.array_equal(mer[b, fr], none_m), where
            if kept[(r["name"], fr)]:
                checked += 1
                np.testing.assert_allclose(pit[b, fr], want_p, rtol=1e-5, atol=0, err_msg=str(where))
                np.testing.assert_allclose(mer[b, fr], want_m, rtol=0, atol=1e-3, err_msg=str(where))
                if want_p.any():
                    worst["pitch rel"] = max(worst["pitch rel"], float(np.max(np.abs(pit[b, fr] - want_p) / want_p)))
                worst["merit abs"] = max(worst["merit abs"], float(np.abs(mer[b, fr] - want_m).max()))
    assert checked >= 0.9 * sum(C.nccf_frames(r) for r in rows)
    print(f"NCCF, {checked} frames, largest deviation:", {k: f"{v:.2e}" for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------------------------
# the whole tracker on utterances of a few frames
# ---------------------------------------------------------------------------------------------------------------
def test_tracker_on_very_short_utterances(trackers):
    from dissc_amd.f0 import lib
    trk = trackers(7)
    x = voiced(np.full(320, 150.0))
    lens = [1, 79, 80, 81, 160, 240, 241, 320]
    sigs = [x[:n] for n in lens]
    dev = trk(sigs)
    host = trk(sigs, host_dp=True)
    for n, s, d, h in zip(lens, sigs, dev, host):
        assert len(d) == len(h) == lib.dissc_yaapt_frames(trk._h, n + 2 * (trk.flen // 2)), n
        assert np.isfinite(d).all() and (d >= 0).all(), n
        np.testing.assert_allclose(d, h, rtol=1e-6, atol=0, err_msg=str(n))
        np.testing.assert_array_equal(trk([s])[0], d, err_msg=str(n))   # alone == in the batch, bit for bit
    assert not dev[0].any() and not dev[1].any()   # 1 and 79 samples: a spectral frame, no time-domain frame
    assert [len(d) for d in dev[:3]] == [1, 1, 1]
