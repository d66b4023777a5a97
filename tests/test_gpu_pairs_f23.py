"""The register-only Toom-Cook F(2,3) residual pairs of the default build (respair32_f23_kernel in respair_f23.hip,
respair16_f23_kernel in respair16_f23.hip; k = 11 at C = 32 / 16) through the C ABI (dissc_respair1d mode 3; at C = 32 under
"pair_tc6" = 0, which leaves the shape to this form): the checks of pair_harness.check_pair.  (The F(4,3) pair kernel and the
k = 3 instances: experimental/tests/test_gpu_pairw.py.)  Run with -s for the measured figures."""
import pytest
import torch

import pair_harness as ph

pytestmark = pytest.mark.gpu
F23 = ph.Form("F(2,3)", 3, {"pair_tc6": 0}, ph.F23)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dissc_amd import _lib
    return _lib


@pytest.mark.parametrize("k", [11])
@pytest.mark.parametrize("C,d", [(32, 1), (32, 3), (32, 5), (16, 1), (16, 3), (16, 5)])
def test_register_only_f23_pair_matches_float64_and_the_direct_pair(lib, C, d, k):
    edges = [n for n in ph.edge_lengths(ph.form_tile(lib, F23, C, k, d)) if n not in ph.F23_LENGTHS]
    ph.check_pair(lib, F23, ph.DIRECT_PAIR, C, k, d, ph.F23_LENGTHS + edges, 900 + d + k, alone=(3, 5, 16, 17))
