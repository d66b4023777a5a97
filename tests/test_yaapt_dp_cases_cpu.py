"""The constructed YAAPT cases of tests/yaapt_dp_cases.py, checked where no GPU is needed: dissc_amd.f0's host stages equal
the oracle's on every case, the cases together take every branch of ALL_BRANCHES, every case holds the margins under
which tests/test_gpu_yaapt_dp.py compares the device with float64 numpy exactly, and every seeded defect of the
reference changes at least one case beyond that test's bars while the unedited reference changes none."""
import os
import re
import warnings

import numpy as np
import pytest

import yaapt_dp_cases as C
from oracle import yaapt_ref as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():   # scipy.signal.medfilt says so when the window is wider than the data
        warnings.simplefilter("ignore")
        yield


def _big():
    return [c for _, a, b in C.big_launches() for c in a + b]


def test_thresholds_follow_the_kernel_source():
    src = open(os.path.join(ROOT, "dissc_amd", "csrc", "yaapt_dp.hip")).read()
    m = re.search(r"constexpr size_t kLdsBack = (\d+) \* 1024;", src)
    assert m and int(m.group(1)) * 1024 == C.LDS_BACK
    assert "const size_t lds = (size_t)4 * F;" in src and "const size_t lds = (size_t)8 * F;" in src
    assert (C.F_SPEC_WS, C.F_FINAL_WS) == (38401, 19201)
    assert re.search(r"constexpr int YA_MAXLIST = 64;", open(os.path.join(ROOT, "dissc_amd", "csrc", "yaapt.hip")).read())


def test_host_stages_equal_the_oracle_on_every_dp_case():
    # (of the long random cases the 19 201-frame launch and the short rows: the oracle's per-frame Python loops take
    # seconds on 38 401 frames, and the tables are drawn by the same builders)
    big = [c for c in _big() if c.get("f", c.get("t")) < C.F_SPEC_WS]
    for c in C.spec_cases() + big:
        if c["kind"] != "spec" or c["f"] == 0:
            continue
        p = dict(yr.PARAMS, median_value=c["median"])
        r = C.spec_reference(c)
        spec_o, std_o, _ = yr.spec_track_from_candidates(r["pit"].astype(np.float64), r["mer"].astype(np.float64), p)
        np.testing.assert_allclose(r["spec"], spec_o, rtol=1e-12, err_msg=c["name"])
        assert abs(r["spec_std"] - std_o) <= 1e-12 * std_o, c["name"]
        lo, hi = yr.lag_ranges(spec_o[:c["n_tda"]], std_o, C.FS, p)
        np.testing.assert_array_equal(r["lag_min"], lo, err_msg=c["name"])
        np.testing.assert_array_equal(r["lag_max"], hi, err_msg=c["name"])
    for c in C.final_cases() + big:
        if c["kind"] != "final" or c["t"] == 0:
            continue
        p = dict(yr.PARAMS, median_value=c["median"])
        # pitches as float64 (the oracle's table takes its dtype from them), merits as the float32 the NCCF kernel writes
        resh = [yr.reshape_merit(c[a].T.astype(np.float64), c[b].T, c["spec"], c["spec_std"], p)
                for a, b in (("tp1", "tm1"), ("tp2", "tm2"))]
        rp, rm = yr.refine(resh[0][0], resh[0][1], resh[1][0], resh[1][1], c["spec"], c["en_norm"], c["vuv"].astype(bool), p)
        np.testing.assert_allclose(C.final_reference(c), yr.dynamic(rp, rm, c["en_norm"], p), rtol=1e-12, err_msg=c["name"])


def test_the_cases_take_every_branch():
    seen = {}
    for c in C.spec_cases() + C.final_cases() + [C.nccf_case()]:
        for tag in C.branches(c):
            seen.setdefault(tag, []).append(c["name"])
    for F, spec, final in [(520, C.spec_cases(), C.final_cases())] + C.big_launches():
        for kind, cases in (("spec", spec), ("final", final)):
            for tag in C.launch_branches(F, kind):
                seen.setdefault(tag, []).append(f"{kind} launch at F = {F}")
    assert len(set(C.ALL_BRANCHES)) == len(C.ALL_BRANCHES)
    assert set(seen) == set(C.ALL_BRANCHES), (sorted(set(C.ALL_BRANCHES) - set(seen)), sorted(set(seen) - set(C.ALL_BRANCHES)))
    # the two long launches differ in where the kernels keep their back-pointers
    (F1, _, _), (F2, _, _) = C.big_launches()
    assert C.launch_branches(F1, "spec") == {"spec:back_in_workspace"} and C.launch_branches(F1, "final") == {"final:back_in_workspace"}
    assert C.launch_branches(F2, "spec") == {"spec:back_in_lds"} and C.launch_branches(F2, "final") == {"final:back_in_workspace"}
    assert C.launch_branches(F1 - 1, "spec") == {"spec:back_in_lds"} and C.launch_branches(F2 - 1, "final") == {"final:back_in_lds"}


def test_every_case_holds_its_margins():
    for c in C.spec_cases() + C.final_cases() + _big():
        m = C.margins(c)
        assert m["ok"], (c["name"], m["why"])
        for k in ("energy", "cand_pitch", "cand_merit", "tp1", "tm1", "tp2", "tm2"):
            assert k not in c or c[k].dtype == np.float32
    n = C.nccf_case()
    m = C.margins(n)
    assert m["ok"], m["why"]
    assert m["dropped"] <= 0.1 * m["frames"], (m["dropped"], m["frames"])
    print(f"NCCF case: {m['dropped']} of {m['frames']} frames dropped for margin (d)")


def _changed_by(defect):
    mod = C._variant(defect)
    hit = [c["name"] for c in C.spec_cases() if C.spec_differs(c, C.spec_reference(c, mod))]
    return hit + [c["name"] for c in C.final_cases() if C.final_differs(c, C.final_reference(c, mod))]


def test_the_unedited_reference_changes_no_case():
    assert C._variant(None).spectral_track is not C.f0m.spectral_track   # recompiled from source, not the same object
    assert _changed_by(None) == []


@pytest.mark.parametrize("defect", sorted(C.DEFECTS))
def test_every_seeded_defect_changes_a_case(defect):
    hit = _changed_by(defect)
    print(f"{defect} ({C.DEFECTS[defect][0]}): {len(hit)} cases, e.g. {hit[:4]}")
    assert hit, defect
