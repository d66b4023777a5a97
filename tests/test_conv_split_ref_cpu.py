"""Rehearsal of tests/conv_split_ref.py on the CPU (as tests/test_gen_split_bf16_model_cpu.py rehearses the generator's models):
the split-bf16 model of nn.conv1d reduces to float64 autograd under the identity split, the two controls (plain bf16; one
cross term dropped) miss the bars the GPU test holds the kernels to, and on every input set the GPU test uses the model is far
enough from unsplit float64 (>= 8 x torch fp32's own error) for that test's lower bound -- "the split arithmetic ran" -- to
tell it from an fp32 fallback."""
import pytest
import torch

import conv_split_ref as cs
import split_bf16_model as sm

NAMES = ("y", "gx", "gw")
FAR = 8.0  # the model's distance to unsplit float64, in units of torch fp32's own


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def refs(lib):
    """every input set of the GPU test with its three references, computed once"""
    out = {}
    for layer_ in cs.LAYERS:
        x, w, b, gy, lengths, ld = cs.inputs(lib, layer_)
        out[layer_] = (x, w, b, gy, lengths) + cs.references(x, w, b, gy, lengths, layer_[3])
    return out


def test_identity_split_is_float64_autograd(lib):
    for layer_ in cs.LAYERS[:3]:
        x, w, b, gy, lengths, ld = cs.inputs(lib, layer_)
        got = cs.layer(x, w, b, gy, lengths, layer_[3], cs.SLOPE, sp=sm.split_identity)
        want = cs.autograd64(x, w, b, torch.nan_to_num(gy), lengths, layer_[3], cs.SLOPE)
        for name, g, r in zip(NAMES + ("gb",), got, want):
            assert cs.rel_rms(g, r) < 1e-13, (layer_, name, cs.rel_rms(g, r))
            assert torch.isfinite(g).all()


def test_lengths_hold_every_edge(lib):
    for layer_ in cs.LAYERS[:-1]:
        lengths, ld = cs.lengths_for(lib, layer_)
        pad = (layer_[2] - 1) * layer_[3] // 2
        widths = cs.tile_widths(lib, *layer_, len(lengths), ld)
        assert {0, 1, 2, pad, pad + 1, *cs.STEP_EDGES} <= set(lengths) and ld in lengths and ld % 4 == 0 and ld == -(-max(lengths) // 4) * 4
        assert all(w + e in lengths for w in widths for e in (-1, 0, 1)), (layer_, widths)
        print(f"CSR {layer_}: tile widths {widths}, ld {ld}, {len(lengths)} utterances")
    assert set(w for l in cs.LAYERS[:-1] for w in cs.tile_widths(lib, *l, 22, 260)) == {128, 256}
    assert cs.lengths_for(lib, cs.LAYERS[-1]) == (cs.MPD_ROWS, 56)


@pytest.mark.parametrize("layer_", cs.LAYERS, ids=lambda l: "%d-%d-k%d-d%d" % l)
def test_controls_miss_the_bars_and_the_model_is_far_from_fp32(refs, layer_):
    x, w, b, gy, lengths, model, r64, r32 = refs[layer_]
    controls = {sp.__name__: cs.layer(x, w, b, gy, lengths, layer_[3], cs.SLOPE, sp=sp) for sp in (sm.split_hi_only, sm.split_two_terms)}
    for j, name in enumerate(NAMES):
        e_model, e32 = cs.rel_rms(model[j], r64[j]), cs.rel_rms(r32[j], r64[j])
        print(f"CSR {layer_} {name}: model to float64 {e_model:.3e}, torch fp32 to float64 {e32:.3e}, ratio {e_model / max(e32, sm.FLOOR):.1f}")
        for cname, c in controls.items():
            bad, fig = cs.bars(name, c[j], model[j], r64[j], r32[j])
            print(f"    control {cname}: {fig['e']:.3e} to the model, {fig['ratio']:.0f} x torch fp32's error (bar {sm.KERNEL_RATIO:g})")
            assert bad and fig["e"] > 32 * max(e32, sm.FLOOR), (layer_, name, cname, fig)  # (32: the most a K exception may ask)
        # the model itself is inside the bars it sets, trivially, and far from an fp32 result
        assert not cs.bars(name, model[j], model[j], r64[j], r32[j])[0]
        assert e_model >= FAR * max(e32, sm.FLOOR), (layer_, name, e_model, e32)
    assert cs.rel_rms(model[3], r64[3]) < 1e-13  # the bias gradient is plain
