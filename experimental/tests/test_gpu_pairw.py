"""respair_wino.hip -- one residual pair y = x + conv_1(lrelu(conv_d(lrelu(x)))) (reference sr/models.py:34-41) per
launch with both convs in the Toom-Cook F(4,3) transform domain -- through the C ABI (dissc_respair1d): the checks of
tests/pair_harness.py against the two direct launches, and against the two-launch transform-domain path; and the register-only F(2,3)
kernels with the k = 3 instances only DISSC_EXPERIMENTAL=1 builds carry."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
import pair_harness as ph  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(32, 7, 1), (32, 7, 3), (32, 7, 5), (32, 11, 1), (32, 11, 3), (32, 11, 5), (64, 3, 1), (64, 3, 3), (64, 3, 5)]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd import _lib
    return _lib


@pytest.fixture(params=[1, 2], ids=["two-6-wave-workgroups-per-CU", "one-12-wave-workgroup-per-CU"])
def f43(request, experimental):  # (respair_wino_kernel failed its gate: DISSC_EXPERIMENTAL=1 builds only)
    """both workgroup shapes of the kernel (option "pairw_chv"); "pair_f23" off, so that mode 3 builds THIS kernel's form for
    every shape (the default is a register-only pair)"""
    return ph.Form("fused transform-domain", 3, {"pairw_chv": request.param, "pair_f23": 0}, ph.F43)


@pytest.mark.parametrize("C,k,d", SHAPES)
def test_fused_transform_domain_pair_matches_float64_and_the_other_paths(lib, f43, C, k, d):
    lengths = [2000, 1, 7, 255, 468, 469, 1023, 1999, 500, 12] + ph.edge_lengths(ph.form_tile(lib, f43, C, k, d))
    y3 = ph.check_pair(lib, f43, ph.Form("two direct launches", 0), C, k, d, lengths, C * 100 + k * 10 + d, max_err=2e-5,
                       alone=(3, 6))
    # the two-launch transform-domain path (the product path of the 64-channel stage) does the same arithmetic in the
    # same order -- except that a tile's last F(4,3) groups see zeros where the two-launch path sees the neighbouring
    # tile's t (contributions that cancel exactly only in exact arithmetic): equal to rounding, not bit for bit
    if C == 64:
        x, w1, b1, w2, b2 = ph.data(C, k, lengths, 2000, seed=C * 100 + k * 10 + d)
        y2 = ph.run_pair(lib, 2, x, w1, b1, w2, b2, lengths, k, d)
        for i, n in enumerate(lengths):
            assert (y2[i, :, :n] - y3[i, :, :n]).abs().max().item() <= 2e-6 if n else True


@pytest.mark.parametrize("C,k,d", [(32, 11, 3), (64, 3, 1), (32, 7, 5)])
def test_fused_transform_domain_pair_epilogue_modes(lib, f43, C, k, d):
    """MRF modes (acc = y | acc += y | acc = (acc + y) / 3) against the residual mode's y, on short rows"""
    lengths = [700, 300, 1]
    x, w1, b1, w2, b2 = ph.data(C, k, lengths, 700, seed=7)
    y = ph.run_form(lib, f43, x, w1, b1, w2, b2, lengths, k, d)
    acc0 = torch.rand(3, C, 700, device=ph.DEV)
    for epi in (2, 3, 4):
        a = ph.run_form(lib, f43, x, w1, b1, w2, b2, lengths, k, d, epi=epi, acc=acc0)
        for i, n in enumerate(lengths):
            want = y[i, :, :n] if epi == 2 else acc0[i, :, :n] + y[i, :, :n]
            if epi == 4:
                want = (want.cpu() / 3.0).to(ph.DEV)  # (a true division: pair_harness.check_pair)
            assert torch.equal(a[i, :, :n], want), (epi, i)
            assert torch.equal(a[i, :, n:], acc0[i, :, n:])


@pytest.mark.parametrize("k", [11, 3])
@pytest.mark.parametrize("C,d", [(32, 1), (32, 3), (32, 5), (16, 1), (16, 3), (16, 5)])
def test_register_only_f23_pair_matches_float64_and_the_direct_pair(lib, C, d, k):
    """respair32_f23_kernel / respair16_f23_kernel with every instance of this build switched on: k = 11 as in
    tests/test_gpu_pairs_f23.py, and k = 3 (bits 4 / 8 of "pair_f23")"""
    if k == 3 and not ph.experimental(lib):
        pytest.skip("the k = 3 instances measured neutral in the forward: DISSC_EXPERIMENTAL=1 builds only")
    f23 = ph.Form("F(2,3)", 3, {"pair_f23": 15, "pair_tc6": 0}, ph.F23)
    edges = [n for n in ph.edge_lengths(ph.form_tile(lib, f23, C, k, d)) if n not in ph.F23_LENGTHS]
    ph.check_pair(lib, f23, ph.DIRECT_PAIR, C, k, d, ph.F23_LENGTHS + edges, 900 + d + k, alone=(3, 5, 16, 17))
