"""dissc_amd.gan_train on the CPU: the segment sampler's law (interval_end, crop_host) element for element against the literal
restatement of CodeDataset.__getitem__ in tests/segment_ref.py, at every legal start of utterances of 1, F - 1, F, F + 1 and 3 F
frames; init_state_dicts' distributions and its keys and shapes against the three torch restatements."""
import math

import numpy as np
import pytest
import torch

import gen_train_ref as GT
from gan_train_cases import GenSkeleton
import mpd_cases as MP
import msd_cases as M
import segment_ref as SR


@pytest.fixture(scope="module")
def gt():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import gan_train
    return gan_train


@pytest.mark.parametrize("hop,segment", [(4, 20), (320, 8960), (1, 7), (3, 6)])
def test_sampler_law_at_every_legal_start(gt, hop, segment):
    F = segment // hop
    raw = SR.raw_corpus(hop, F, seed=hop)
    items = SR.prepared(raw, hop)
    assert [len(it["code"]) for it in items] == SR.lengths(F)
    for (audio, code, pitch, _), it in zip(raw, items):
        end = SR.getitem_crop(audio, code, pitch, segment, hop)[3]
        assert gt.interval_end(len(it["code"]), hop, segment) == end
        for s in range(end + 1):
            ya, ca, fa, _ = SR.getitem_crop(audio, code, pitch, segment, hop, s)
            yb, cb, fb = gt.crop_host(it, s, hop, segment)
            assert yb.dtype == np.float32 and cb.dtype == np.int64 and fb.dtype == np.float32
            assert np.array_equal(ya, yb) and np.array_equal(ca, cb) and np.array_equal(fa, fb), (len(it["code"]), s)


def test_refusals_by_name(gt):
    h = dict(GT.TINY_CONFIG, learning_rate=2e-4, adam_b1=0.8, adam_b2=0.99)
    for k in ("f0_median", "f0_vq_params", "code_vq_params"):
        with pytest.raises(NotImplementedError, match=k):
            gt.refuse_unsupported(dict(h, **{k: True}), environ={})
    with pytest.raises(NotImplementedError, match="num_gpus"):
        gt.refuse_unsupported(dict(h, num_gpus=2), environ={})
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        gt.refuse_unsupported(h, environ={"WORLD_SIZE": "2"})
    gt.refuse_unsupported(dict(h, num_gpus=1), environ={"WORLD_SIZE": "1"})  # what a launcher exports for a single-GPU job
    with pytest.raises(NotImplementedError, match="f0_median"):
        gt.SegmentSampler(dict(h, f0_median=True, code_hop_size=4, segment_size=20, batch_size=2), [])


@pytest.fixture(scope="module")
def fresh(gt):
    return gt.init_state_dicts(GT.SMALL_CONFIG, seed=5)


def test_init_distributions(gt, fresh):
    n_conv = 0
    for sd in fresh:
        for key, v in sd.items():
            if not (key.endswith(".weight_v") and v.dim() >= 3 or key.endswith(".weight_orig")):
                continue
            n_conv += 1
            pre = key.rsplit(".", 1)[0]
            # torch's fan_in: weight.size(1) * the receptive field -- for a ConvTranspose1d [Cin, Cout, k] that is Cout k
            bound = 1.0 / math.sqrt(v.shape[1] * v.shape[2])
            assert float(v.abs().max()) <= bound and float(sd[pre + ".bias"].abs().max()) <= bound, key
            if v.numel() >= 4096:  # uniform, not something narrower: the variance of U(-b, b) is b^2 / 3
                assert abs(float(v.var()) / (bound * bound / 3) - 1) < 0.1, key
            if key.endswith(".weight_v"):
                g = sd[pre + ".weight_g"]
                assert g.shape == (v.shape[0],) + (1,) * (v.dim() - 1)
                assert torch.equal(g.reshape(-1), v.reshape(v.shape[0], -1).norm(dim=1)), key
            else:
                u, w = sd[pre + ".weight_u"], sd[pre + ".weight_v"]
                assert u.shape == (v.shape[0],) and w.shape == (v.shape[1] * v.shape[2],)
                assert abs(float(u.norm()) - 1) < 1e-6 and abs(float(w.norm()) - 1) < 1e-6, key
    assert n_conv == len(fresh[0]) // 3 + 30 + 24  # every conv of the generator, 5 x 6 period convs, 3 x 8 scale convs
    for key in ("dict.weight", "spkr.weight"):
        t = fresh[0][key]
        assert abs(float(t.mean())) < 0.2 and abs(float(t.std()) - 1) < 0.15, key
    ups = fresh[0]["ups.0.weight_v"]  # [Cin 64, Cout 32, k 8]: fan_in 32 * 8, not 64 * 8
    assert ups.shape == (64, 32, 8) and float(ups.abs().max()) > 1.0 / math.sqrt(64 * 8)
    again = gt.init_state_dicts(GT.SMALL_CONFIG, seed=5)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(fresh, again) for k in a)
    other = gt.init_state_dicts(GT.SMALL_CONFIG, seed=6)
    assert not torch.equal(fresh[0]["conv_pre.weight_v"], other[0]["conv_pre.weight_v"])


def test_init_loads_into_the_torch_restatements(fresh):
    GenSkeleton(GT.SMALL_CONFIG).load_state_dict(fresh[0], strict=True)
    MP.TorchMPD().load_state_dict(fresh[1], strict=True)
    M.TorchMSD().load_state_dict(fresh[2], strict=True)
