"""The CPU model of the generator's split-bf16 kernels (tests/split_bf16_model.py: conv1d_ref, conv_transpose1d_ref, pair_ref,
resblock_ref), the yardstick of tests/test_gpu_gen_split_bf16.py, and the two bars of that file:
  a single launch against float64 on the same split operands   <= KERNEL_RATIO x torch fp32's error on the unsplit operation;
  a pair or a block against float64 on the unsplit operands    <= MODEL_FACTOR x the model's error + FP32_RATIO x torch fp32's.
Errors: worst column, l2 over the channels, relative.  Nothing here runs on a device: what stands in for it is the model with
its three products accumulated in fp32 (torch's order), which must sit inside both bars, while the two ways to get the
arithmetic wrong -- hi halves only, and one cross term dropped -- must miss the block bar by >= 20 x.

Measured (C = 16 / 32 / 64 x k = 3 / 7 / 11, dilations (1, 3, 5), 600 columns, x uniform in [-1, 1), w ~ N(0, 1 / (C k))):
    torch fp32 2.1e-7 .. 6.2e-7, model 6.5e-6 .. 1.2e-5, fp32-accumulating emulation 0.42 .. 0.51 of the block bar,
    two-term control 142 .. 207 x the block bar, hi-only control 220 .. 269 x; one launch: emulation 0.12 .. 0.15 of the launch
    bar (torch's fp32 accumulation; the device's own order is what the GPU test measures), two-term control > 1 000 x."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_bf16_model as sm

DIL = (1, 3, 5)
N = 600
SLOPE = 0.1
CONTROL_MARGIN = 20.0


def block_data(C, k, n=N, seed=None):
    rs = np.random.RandomState(1000 * C + k if seed is None else seed)
    x = torch.from_numpy(rs.uniform(-1, 1, (C, n)).astype(np.float32))
    w6 = [torch.from_numpy((rs.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32)) for _ in range(6)]
    b6 = [torch.from_numpy(rs.uniform(-0.1, 0.1, C).astype(np.float32)) for _ in range(6)]
    return x, w6, b6


@pytest.fixture(scope="module", params=[(C, k) for C in (16, 32, 64) for k in (3, 7, 11)], ids=lambda p: f"C{p[0]}-k{p[1]}")
def block(request):
    C, k = request.param
    x, w6, b6 = block_data(C, k)
    r64 = sm.resblock_plain(x, w6, b6, k, DIL)
    e32 = float(sm.col_errs(sm.resblock_plain(x, w6, b6, k, DIL, dtype=torch.float32), r64).max())
    em = float(sm.col_errs(sm.resblock_ref(x, w6, b6, k, DIL), r64).max())
    return dict(C=C, k=k, x=x, w6=w6, b6=b6, r64=r64, e32=e32, em=em, bar=sm.block_bar(em, e32))


def test_identity_split_is_no_worse_than_fp32(block):
    """with split := identity the model is the chain with exact products and sums, rounded to fp32 once per conv: it changes
    nothing but the arithmetic"""
    e_id = float(sm.col_errs(sm.resblock_ref(block["x"], block["w6"], block["b6"], block["k"], DIL, sp=sm.split_identity), block["r64"]).max())
    print(f"\nGSM C {block['C']} k {block['k']}: identity {e_id:.2e}, torch fp32 {block['e32']:.2e}")
    assert e_id <= block["e32"]


def test_model_and_its_fp32_emulation_sit_inside_the_block_bar(block):
    b = block
    emu = sm.resblock_ref(b["x"], b["w6"], b["b6"], b["k"], DIL, dtype=torch.float32)
    e_emu = float(sm.col_errs(emu, b["r64"]).max())
    e_dist = float(sm.col_errs(emu, sm.resblock_ref(b["x"], b["w6"], b["b6"], b["k"], DIL)).max())
    print(f"\nGSM C {b['C']} k {b['k']}: torch fp32 {b['e32']:.2e}, model {b['em']:.2e}, block bar {b['bar']:.2e}; fp32-accumulating "
          f"emulation {e_emu:.2e} = {e_emu / b['bar']:.2f} of the bar, {e_dist:.2e} from the model")
    assert b["e32"] < b["em"] < 100 * b["e32"]  # the arithmetic is not free, and far from plain bf16
    assert b["em"] <= b["bar"] and e_emu <= b["bar"]


def test_controls_miss_the_block_bar_by_a_wide_margin(block):
    b = block
    out = {}
    for name, sp in (("two terms", sm.split_two_terms), ("hi only", sm.split_hi_only)):
        out[name] = float(sm.col_errs(sm.resblock_ref(b["x"], b["w6"], b["b6"], b["k"], DIL, sp=sp), b["r64"]).max()) / b["bar"]
    print(f"\nGSM C {b['C']} k {b['k']}: two-term control {out['two terms']:.0f} x the block bar, hi-only control {out['hi only']:.0f} x")
    assert out["two terms"] >= CONTROL_MARGIN and out["hi only"] >= out["two terms"]


@pytest.mark.parametrize("cin,cout,k,d,slope", [(257, 512, 7, 1, 1.0), (256, 256, 11, 5, SLOPE), (20, 40, 7, 3, SLOPE)])
def test_single_launch_emulation_sits_inside_the_launch_bar(cin, cout, k, d, slope):
    """one conv: float64 on the split operands against the same products accumulated in fp32, and the controls"""
    rs = np.random.RandomState(cin + k)
    x = torch.from_numpy(rs.uniform(-1, 1, (1, cin, 300)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32))
    ref = sm.conv1d_ref(x, w, b, k, d, slope)
    pad = (k - 1) * d // 2
    r64 = F.conv1d(F.leaky_relu(x.double(), slope), w.double(), b.double(), padding=pad, dilation=d)
    r32 = F.conv1d(F.leaky_relu(x, slope), w, b, padding=pad, dilation=d)
    bar = sm.launch_bar(float(sm.col_errs(r32, r64).max()))
    e_emu = float(sm.col_errs(sm.conv1d_ref(x, w, b, k, d, slope, dtype=torch.float32), ref).max())
    e_two = float(sm.col_errs(sm.conv1d_ref(x, w, b, k, d, slope, sp=sm.split_two_terms), ref).max())
    print(f"\nGSM conv {cin} -> {cout} k {k} d {d}: emulation {e_emu / bar:.2f} of the launch bar, two-term control {e_two / bar:.0f} x")
    assert e_emu <= bar and e_two >= CONTROL_MARGIN * bar


def test_conv_transpose_and_pair_models_agree_with_torch_on_unsplit_operands():
    """with the identity split the ConvTranspose and pair models are torch's float64 operation, to the fp32 roundings they keep
    from the device (the leaky ReLU on load, one per conv result)"""
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.uniform(-1, 1, (2, 32, 37)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((32, 16, 4)) / 8).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, 16).astype(np.float32))
    want = F.conv_transpose1d(F.leaky_relu(x.double(), SLOPE), w.double(), b.double(), stride=2, padding=1)
    assert float(sm.col_errs(sm.conv_transpose1d_ref(x, w, b, 2, SLOPE, sp=sm.split_identity), want).max()) < 1e-7
    assert float(sm.col_errs(sm.conv_transpose1d_ref(x, w, b, 2, SLOPE), want).max()) < 1e-4
    w1, w2 = (torch.from_numpy((rs.standard_normal((32, 32, 3)) / 10).astype(np.float32)) for _ in range(2))
    b1, b2 = (torch.from_numpy(rs.uniform(-0.1, 0.1, 32).astype(np.float32)) for _ in range(2))
    acc = torch.from_numpy(rs.uniform(0, 1, x.shape).astype(np.float32))
    t = F.conv1d(F.leaky_relu(x.double(), SLOPE), w1.double(), b1.double(), padding=3, dilation=3)
    y = x.double() + F.conv1d(F.leaky_relu(t, SLOPE), w2.double(), b2.double(), padding=1)
    for epi, ref in ((1, y), (2, y), (3, acc.double() + y), (4, (acc.double() + y) / 3.0)):
        got = sm.pair_ref(x, w1, b1, w2, b2, 3, 3, SLOPE, epi=epi, acc=acc, sp=sm.split_identity)
        assert got.dtype == torch.float32 and float(sm.col_errs(got, ref).max()) < 5e-7, epi
        assert float(sm.col_errs(sm.pair_ref(x, w1, b1, w2, b2, 3, 3, SLOPE, epi=epi, acc=acc), ref).max()) < 1e-4, epi


def test_partial_blocks_chain_to_the_whole_block():
    """pairs [0, 1), [1, 2), [2, 3) chained = the block in one piece, bit for bit, in the model as on the device"""
    x, w6, b6 = block_data(16, 7, n=97, seed=3)
    xk = x
    for m in range(3):
        xk = sm.resblock_ref(xk, w6, b6, 7, DIL, m, m + 1)
    assert torch.equal(xk, sm.resblock_ref(x, w6, b6, 7, DIL))


# ---- what would run: dissc_bf3_info (host only: no GPU is touched) --------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import _lib
    return _lib


def test_bf3_info_reports_the_launch_plans(lib):
    """the tile of conv_bf3_kernel by row class and the small-grid step-down (fewer than 256 x "small_grid" workgroups of the class
    tile), the windows of resblock_bf3_kernel (halo sum P2 (d + 1) over the pairs, rounded up to 4), and what has no instance"""
    assert lib.lib.dissc_abi_version() == 9
    before = lib.get_option("small_grid")
    try:
        lib.set_option("small_grid", 0)
        got = [lib.bf3_conv_info(64, m, 3, 1, 1, 100) for m in (32, 63, 64, 127, 128, 255, 256, 512)]
        assert [(g["tile"], g["bm"], g["bn"], g["small_grid"]) for g in got] == \
            [(0, 32, 256, 0)] * 2 + [(1, 64, 128, 0)] * 2 + [(2, 128, 256, 0)] * 2 + [(3, 256, 128, 0)] * 2
        lib.set_option("small_grid", 1)
        assert lib.bf3_conv_info(64, 64, 3, 1, 1, 100) == dict(bm=64, bn=128, small_grid=0, tile=1)  # below 128 rows: never
        # 256 rows on 256 x 128 tiles: B x ceil(Lmax / 128) workgroups; 255 of them step down, 256 do not
        assert lib.bf3_conv_info(256, 256, 3, 1, 255, 128) == dict(bm=64, bn=128, small_grid=1, tile=1)
        assert lib.bf3_conv_info(256, 256, 3, 1, 256, 128) == dict(bm=256, bn=128, small_grid=0, tile=3)
        assert lib.bf3_conv_info(256, 256, 3, 1, 128, 129) == dict(bm=256, bn=128, small_grid=0, tile=3)
        # 128 rows on 128 x 256 tiles
        assert lib.bf3_conv_info(128, 128, 7, 3, 85, 3 * 256) == dict(bm=64, bn=128, small_grid=1, tile=1)
        assert lib.bf3_conv_info(128, 128, 7, 3, 86, 3 * 256) == dict(bm=128, bn=256, small_grid=0, tile=2)
    finally:
        lib.set_option("small_grid", before)
    for C, cols in ((16, 512), (32, 512), (64, 256)):
        for k in (3, 7, 11):
            p2 = (k - 1) // 2
            for dil, m0, m1 in (((1, 3, 5), 0, 3), ((1, 3, 5), 0, 1), ((1, 3, 5), 1, 2), ((1, 3, 5), 2, 3), ((5, 5, 5), 0, 3), ((2, 4, 1), 1, 3)):
                h4 = (sum(p2 * (d + 1) for d in dil[m0:m1]) + 3) // 4 * 4
                pad = 32 if C == 16 else (p2 * 5 + 3) // 4 * 4
                assert lib.bf3_block_info(C, k, dil, m0, m1) == dict(cols=cols, pad=pad, h4=h4, bn=cols - 2 * h4), (C, k, dil, m0, m1)
    assert lib.bf3_block_info(64, 11, (5, 5, 5))["bn"] == 72
    for bad in ((64, 16, 3, 1), (64, 64, 11, 7), (512, 512, 1, 1), (64, 64, 3, 0)):  # 16 rows; span 70; a big 1x1 layer; dilation 0
        with pytest.raises(lib.DisscError):
            lib.bf3_conv_info(*bad, 4, 100)
    for bad in ((48, 3, (1, 3, 5), 0, 3), (32, 5, (1, 3, 5), 0, 3), (32, 3, (1, 3, 6), 0, 3), (32, 3, (1, 3, 5), 2, 2), (32, 3, (1, 3, 5), 0, 4)):
        with pytest.raises(lib.DisscError):
            lib.bf3_block_info(*bad)
    out = ctypes.c_int(0)
    assert lib.lib.dissc_get_option(b"precision", ctypes.byref(out)) == 0 and out.value == 0  # asking does not switch the mode on
