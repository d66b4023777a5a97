"""The mel kernels (csrc/mel.hip through dissc_amd.mel) on the MI355X against tests/mel_ref.py.

Yardstick: mel_ref.mel in float64.  The bar is tied to the reference's own arithmetic, not to a constant: per frame
e = max_cell |mel - mel64| / max_cell mel64, and the kernel's worst frame may be at most 8 x the worst frame of mel_ref's
float32 path (torch.stft, the reference's precision) on the same signals.  Why 8: a 1 024-term fp32 dot product grows
rounding by about sqrt(1024) / log2(1024) = 3.2 x over a radix FFT; a CPU model (fp32 matmul DFT) read 2.2 to 4.9 x on
the four signal kinds; 8 leaves under 2 x over the worst, while a dropped tap, a wrong window or a wrong mirror index is
>= 1e-3.  The log-mel tolerance is that bar propagated to first order, per cell: bar_abs(frame) / max(mel64, 1e-5), no cell
left out; cells that clamp on both sides must be log(1e-5) exactly.  The fused L1 is held (a) to the float64 oracle within
the mean of the two signals' per-cell log tolerances (triangle inequality) and (b) to the float64 sum of the kernel's own
stored log-mels within 2^-23 of the sum of the terms (one fp32 rounding per cell, all additions in double).

Lengths: the smallest that reach every branch -- one frame with both mirrors in one tile (385), 640, 1023, 1024, one
sample either side of a full tile, two tiles and a bit, and 10 560 = 33 code hops of 320 (no multiple of 256) -- each alone
and all together as one ragged batch.  The measured ratios are printed (pytest -s) and recorded in profiles/mel.md.
"""
import numpy as np
import pytest
import torch

from mel_cases import FACTOR, KINDS, NARROW, ODD_HOP, SHIPPED, Ref, batch_of, ref_of, run_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG_FLOOR = np.float32(np.log(np.float64(np.float32(1e-5))))


@pytest.fixture(scope="module")
def melmod():
    from dissc_amd import mel
    return mel


def check_forward(ms, ref, label):
    alone_lin = [run_forward(ms, [w], True)[0] for w in ref.waves]
    alone_log = [run_forward(ms, [w], False)[0] for w in ref.waves]
    both_lin, both_log = run_forward(ms, ref.waves, True), run_forward(ms, ref.waves, False)
    worst = 0.0
    for i, w in enumerate(ref.waves):
        assert alone_lin[i].shape == ref.lin[i].shape, (label, len(w))
        assert np.array_equal(alone_lin[i], both_lin[i]) and np.array_equal(alone_log[i], both_log[i]), (label, len(w))
        e = ref.worst(i, alone_lin[i])
        worst = max(worst, e)
        print(f"mel linear {label} L={len(w)}: e_gpu {e:.3e}  e_torch32(set) {ref.e32:.3e}  ratio {e / ref.e32:.2f}")
    print(f"mel linear {label}: worst ratio {worst / ref.e32:.2f} (bar {FACTOR:.0f})")
    for i, w in enumerate(ref.waves):
        assert ref.worst(i, alone_lin[i]) <= ref.bar, (label, len(w), ref.worst(i, alone_lin[i]), ref.bar)
        err = np.abs(alone_log[i].astype(np.float64) - ref.log[i])
        over = err > ref.tol[i]
        assert not over.any(), (label, len(w), int(over.sum()), float((err / ref.tol[i]).max()))
        floor = (ref.lin[i] <= 1e-5) & (alone_lin[i] <= np.float32(1e-5))
        assert np.array_equal(alone_log[i][floor], np.full(int(floor.sum()), LOG_FLOOR, np.float32)), (label, len(w))
    return worst / ref.e32


@pytest.mark.parametrize("kind", KINDS)
def test_linear_and_log_mel_against_float64(melmod, kind):
    ms = melmod.MelSpectrogram(**SHIPPED).to(DEV)
    ref = ref_of(kind, SHIPPED)
    check_forward(ms, ref, kind)
    if kind in ("speech_like", "speech_dc"):  # the silences clamp: the exact-floor branch above was not vacuous
        assert any(((m <= 1e-5).any() for m in ref.lin))


@pytest.mark.parametrize("kind", ("iid", "speech_like"))
def test_second_parameter_set(melmod, kind):
    ms = melmod.MelSpectrogram(**NARROW).to(DEV)
    ref = ref_of(kind, NARROW)
    check_forward(ms, ref, kind + "/narrow")
    check_l1(ms, ref, Ref([w[::-1].copy() for w in ref.waves], NARROW), kind + "/narrow vs reversed")


def test_hop_that_is_no_multiple_of_four(melmod):
    """the scalar LDS read path: same bars"""
    ms = melmod.MelSpectrogram(**ODD_HOP).to(DEV)
    ref = ref_of("speech_like", ODD_HOP)
    check_forward(ms, ref, "speech_like/hop250")
    check_l1(ms, ref, ref_of("iid", ODD_HOP), "speech_like vs iid/hop250")


def check_l1(ms, ref_a, ref_b, label):
    """l1(a, b) for the ragged batch: (a) float64 oracle, (b) float64 sum of the kernel's own stored log-mels"""
    waves_a, waves_b = ref_a.waves, ref_b.waves
    xa, ns = batch_of(waves_a)
    xb, nsb = batch_of(waves_b)
    assert ns == nsb
    out = ms.l1(xa, xb, ns)
    total, cells, mean = out["sum"].cpu().numpy(), out["cells"].cpu().numpy(), out["mean"].cpu().numpy()
    la, lb = run_forward(ms, waves_a, False), run_forward(ms, waves_b, False)
    for i, n in enumerate(ns):
        assert cells[i] == ref_a.log[i].size == (n // ms.hop_size) * ms.num_mels
        want = float(np.abs(ref_a.log[i] - ref_b.log[i]).mean())
        bar = float((ref_a.tol[i] + ref_b.tol[i]).mean())
        print(f"mel l1 {label} L={n}: gpu {mean[i]:.9f} oracle {want:.9f} |d| {abs(mean[i] - want):.3e} bar {bar:.3e}")
        assert abs(mean[i] - want) <= bar, (label, n, mean[i], want, bar)
        terms = np.abs(la[i].astype(np.float64) - lb[i].astype(np.float64))
        assert abs(total[i] - terms.sum()) <= 2.0 ** -23 * terms.sum(), (label, n, total[i], terms.sum())
        assert mean[i] == total[i] / cells[i]
    return total


@pytest.mark.parametrize("kind", ("iid", "speech_dc"))
def test_fused_l1_against_a_noisy_copy(melmod, kind):
    ms = melmod.MelSpectrogram(**SHIPPED).to(DEV)
    ref = ref_of(kind, SHIPPED)
    rs = np.random.RandomState(7)
    noisy = [np.clip(w + 0.01 * rs.standard_normal(len(w)), -1, 1).astype(np.float32) for w in ref.waves]
    check_l1(ms, ref, Ref(noisy, SHIPPED), kind + " vs noisy")


def test_fused_l1_between_two_kinds(melmod):
    ms = melmod.MelSpectrogram(**SHIPPED).to(DEV)
    a, b = ref_of("speech_like", SHIPPED), ref_of("dither", SHIPPED)
    check_l1(ms, a, b, "speech_like vs dither")


def test_bit_reproducible_and_independent_of_the_batch(melmod):
    ms = melmod.MelSpectrogram(**SHIPPED).to(DEV)
    ref, other = ref_of("speech_like", SHIPPED), ref_of("iid", SHIPPED)
    me, me_b = ref.waves[7], other.waves[7]  # two tiles and a bit
    alone = run_forward(ms, [me], False)[0]
    alone_sum = ms.l1(me[None], me_b[None])["sum"].cpu().numpy()
    assert np.array_equal(alone_sum, ms.l1(me[None], me_b[None])["sum"].cpu().numpy())
    assert alone.tobytes() == run_forward(ms, [me], False)[0].tobytes()
    fill_a, fill_b = [ref.waves[8], ref.waves[0], ref.waves[5], ref.waves[3]], [other.waves[8], other.waves[0],
                                                                                  other.waves[5], other.waves[3]]
    for pos in (0, 2, 4):
        wa, wb = list(fill_a), list(fill_b)
        wa.insert(pos, me)
        wb.insert(pos, me_b)
        assert len(wa) == 5
        assert np.array_equal(run_forward(ms, wa, False)[pos], alone), pos
        xa, ns = batch_of(wa)
        xb, _ = batch_of(wb)
        assert ms.l1(xa, xb, ns)["sum"].cpu().numpy()[pos] == alone_sum[0], pos


def test_drop_in_function_and_errors(melmod):
    ref = ref_of("iid", SHIPPED)
    y = torch.from_numpy(ref.waves[3][None]).to(DEV)
    got = melmod.mel_spectrogram(y, 1024, 80, 16000, 256, 1024, 0, None).cpu().numpy()[0]
    assert got.shape == ref.log[3].shape and not (np.abs(got - ref.log[3]) > ref.tol[3]).any()
    with pytest.raises(NotImplementedError):
        melmod.mel_spectrogram(y, 1024, 80, 16000, 256, 1024, 0, None, center=True)
    ms = melmod.MelSpectrogram(**SHIPPED).to(DEV)
    with pytest.raises(melmod._lib.DisscError):
        ms.forward(np.zeros((1, 384), np.float32))  # n_samples <= (n_fft - hop) / 2: no mirror
    with pytest.raises(melmod._lib.DisscError):
        ms.l1(np.zeros((2, 4000), np.float32), np.zeros((2, 4000), np.float32), [4000, 384])
    for bad in (dict(n_fft=1000), dict(hop_size=255), dict(hop_size=2), dict(win_size=2048), dict(num_mels=129), dict(n_fft=2048, hop_size=2048)):
        with pytest.raises(melmod._lib.DisscError):
            melmod.MelSpectrogram(**dict(SHIPPED, **bad)).to(DEV).forward(np.zeros((1, 8000), np.float32))
