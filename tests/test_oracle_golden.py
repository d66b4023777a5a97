"""The CPU oracle (oracle/) against outputs of the reference itself.

tests/golden/gen_vctk.npz was produced by tests/golden/make_golden.py, which ran
the unmodified reference CodeGenerator (reference sr/models.py) in the build
container.  These tests pin the oracle before anything else trusts it."""
import os

import numpy as np
import pytest
import torch

from oracle import generator_ref as gr
import synthdata as synth
from kmeans_cases import kmeans_f32, kmeans_tie_cases


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "gen_vctk.npz"))


@pytest.fixture(scope="module")
def folded():
    return gr.fold_state_dict(synth.synth_generator_state_dict(seed=0))


def test_state_dict_layout():
    sd = synth.synth_generator_state_dict(seed=0)
    assert len(sd) == 293  # 97 convs x {bias, weight_g, weight_v} + dict + spkr
    assert sd["ups.0.weight_g"].shape == (512, 1, 1)  # per INPUT channel for ConvTranspose1d
    assert sd["resblocks.14.convs2.2.weight_v"].shape == (16, 16, 11)


def test_fold_matches_reference_bitwise(gold, folded):
    for name in ("conv_pre", "ups.0", "ups.3", "resblocks.0.convs1.2", "resblocks.14.convs2.0", "conv_post"):
        wt = folded[name + ".weight"].double()
        got = np.array([wt.sum().item(), wt.abs().sum().item(), (wt * wt).sum().item()])
        np.testing.assert_array_equal(got, gold[f"s0/fold/{name}"])
    np.testing.assert_array_equal(folded["ups.4.weight"].numpy(), gold["s0/fold/ups.4.weight"])


@pytest.mark.parametrize("T", [1, 2, 7, 33, 99])
def test_waveform_matches_reference(gold, folded, T):
    code, f0, spkr, _ = synth.synth_generator_inputs(1, T, seed=100 + T)
    taps = {}
    y = gr.code_generator(folded, synth.VCTK_CONFIG, code, f0, spkr, taps=taps).numpy()
    ref = gold[f"s0/T{T}/wav"]
    assert y.shape == ref.shape == (1, 1, 320 * T)
    # same ops in the same order on the same CPU backend: expect (near) bit equality
    assert np.abs(y - ref).max() <= 1e-6
    if T == 7:
        for k in ["conv_pre"] + [f"up{i}" for i in range(5)]:
            assert np.abs(taps[k].numpy() - gold[f"s0/T7/{k}"]).max() <= 1e-5, k
        for i in range(4):
            want = gold[f"s0/T7/lrelu_mrf{i}"]
            got = torch.nn.functional.leaky_relu(taps[f"mrf{i}"], 0.1).numpy()
            assert np.abs(got - want).max() <= 1e-5, i


@pytest.mark.parametrize("case", ["code_short", "f0_short", "code_short3"])
def test_upsample_branches_match_reference(golden_dir, folded, case):
    """CodeGenerator.forward's `_upsample` (reference sr/models.py:158-177,206-210): the SHORTER stream is repeated up to the longer one --
    the code stream too (round 5 verdict, missing #5), not only f0.  Goldens: the reference's own forward (make_golden.py upsample)."""
    g = np.load(os.path.join(golden_dir, "gen_upsample.npz"))
    x = gr.embed_concat(folded, torch.from_numpy(g[f"{case}/code"]), torch.from_numpy(g[f"{case}/f0"]), torch.from_numpy(g[f"{case}/spkr"]))
    y = gr.generator_forward(folded, synth.VCTK_CONFIG, x).numpy()
    assert y.shape == g[f"{case}/wav"].shape and np.abs(y - g[f"{case}/wav"]).max() <= 1e-6
    with pytest.raises(NotImplementedError):  # a non-integer ratio is refused like the reference does
        gr.embed_concat(folded, torch.from_numpy(g[f"{case}/code"][:, :5]), torch.from_numpy(g[f"{case}/f0"][:, :, :7]),
                        torch.from_numpy(g[f"{case}/spkr"]))


def test_resblocks_match_reference(gold, folded):
    x = torch.from_numpy(gold["s0/T7/up2"])
    for j, k in enumerate((3, 7, 11)):
        r = gr.resblock1(folded, f"resblocks.{2 * 3 + j}", x, k)
        assert np.abs(r.numpy() - gold[f"s0/T7/rb{6 + j}"]).max() <= 1e-5


def test_ragged_batch_is_per_utterance(gold, folded):
    code, f0, spkr, _ = synth.synth_generator_inputs(4, 40, seed=777)
    lengths = gold["s0/ragged/lengths"]
    y = gr.code_generator(folded, synth.VCTK_CONFIG, code, f0, spkr, lengths=lengths).numpy()
    for b in range(4):
        n = int(lengths[b]) * 320
        assert np.abs(y[b, :, :n] - gold[f"s0/ragged/wav{b}"][0]).max() <= 1e-6
        assert not y[b, :, n:].any()


def test_wav_postprocess_truncates_and_wraps():
    y = np.array([0.0, 0.99999, -0.99999, 1.0, -1.0, 0.5 / 32768, -0.5 / 32768, 3.7 / 32768, -3.7 / 32768],
                 dtype=np.float32)
    i16 = (y * 32768.0).astype("int16")  # what the reference does (numpy semantics)
    want = i16.astype(np.float32) / np.abs(i16.astype(np.float32)).max()
    np.testing.assert_array_equal(gr.wav_postprocess(y), want)
    assert gr.wav_postprocess(np.zeros(5, np.float32)).tolist() == [0.0] * 5


# ------------------------------------------------------------------------------------------
# predictors + infer.py sample logic (golden: tests/golden/pred.npz, made by running the
# reference's model/*.py and infer.py)
# ------------------------------------------------------------------------------------------
from oracle import predictors_ref as pr  # noqa: E402


@pytest.fixture(scope="module")
def pgold(golden_dir):
    return np.load(os.path.join(golden_dir, "pred.npz"))


def test_predictor_state_dict_layouts():
    assert len(synth.synth_len_state_dict()) == 53
    assert len(synth.synth_pitch_state_dict("new")) == 34
    assert len(synth.synth_pitch_state_dict("base")) == 78


def test_dedup_and_carryover_match_reference(pgold):
    for i in range(int(pgold["n_seqs"])):
        vals, counts = pr.dedup_seq(pgold[f"seq{i}"])
        np.testing.assert_array_equal(vals, pgold[f"dd_vals{i}"])
        np.testing.assert_array_equal(counts, pgold[f"dd_counts{i}"])
        got = pr.len_carryover_correction(torch.from_numpy(pgold[f"lens{i}"]))
        np.testing.assert_array_equal(got.numpy(), pgold[f"lens_int{i}"])
    for j in range(4):
        got = pr.len_carryover_correction(torch.from_numpy(pgold[f"carry_in{j}"]))
        np.testing.assert_array_equal(got.numpy(), pgold[f"carry_out{j}"])


def test_len_and_pitch_predictors_match_reference(pgold):
    len_sd = synth.synth_len_state_dict(100, 108)
    mean, std = synth.synth_len_norm_stats()
    id2m, id2s = torch.from_numpy(pgold["id2pitch_mean"]), torch.from_numpy(pgold["id2pitch_std"])
    for i in range(int(pgold["n_seqs"])):
        spk = torch.tensor([[int(pgold[f"spk{i}"])]])
        dd = torch.from_numpy(pgold[f"dd_vals{i}"]).unsqueeze(0)
        lens = pr.len_predictor(len_sd, dd, spk, mean, std)
        assert np.abs(lens.numpy() - pgold[f"lens{i}"]).max() <= 1e-6
        exp = torch.from_numpy(pgold[f"expanded{i}"])
        for kind in ("new", "base"):
            sd = synth.synth_pitch_state_dict(kind, 100, 108)
            f_n = pr.pitch_predictor(sd, exp, spk, kind, True)
            f_h = pr.pitch_predictor(sd, exp, spk, kind, False, id2m, id2s)
            assert np.abs(f_n.numpy() - pgold[f"f0_{kind}_norm{i}"]).max() <= 1e-6
            assert np.abs(f_h.numpy() - pgold[f"f0_{kind}_hz{i}"]).max() <= 1e-4
            # unvoiced frames are exactly zero
            assert ((f_n.numpy() == 0) == (pgold[f"f0_{kind}_norm{i}"] == 0)).all()


def test_infer_sample_matches_reference_infer_wild(pgold):
    len_sd = synth.synth_len_state_dict(100, 10)
    pitch_sd = synth.synth_pitch_state_dict("base", 100, 10)
    stats = synth.synth_len_norm_stats()
    import pickle
    spk_names = pickle.load(open(os.path.join(os.path.dirname(__file__), "golden", "esd_id_to_spkr.pkl"), "rb"))
    for t in pgold["wild/targets"]:
        spk = spk_names.index(str(t))
        for i in range(3):
            units, f0 = pr.infer_sample(pgold[f"wild/in{i}"], spk, len_sd, stats, pitch_sd, "base", True)
            np.testing.assert_array_equal(units, pgold[f"wild/{t}/{i}/units"])
            assert np.abs(np.array(f0) - pgold[f"wild/{t}/{i}/f0"]).max() <= 1e-6


# ------------------------------------------------------------------------------------------
# HuBERT unit encoder (golden: HF transformers.HubertModel + sklearn KMeans.predict;
# parity vs fairseq/textless itself is UNPINNED -- see oracle/hubert_ref.py header)
# ------------------------------------------------------------------------------------------
from oracle import hubert_ref as hr  # noqa: E402


@pytest.fixture(scope="module")
def hgold(golden_dir):
    return np.load(os.path.join(golden_dir, "hubert.npz"))


def test_hubert_frame_count():
    assert [hr.num_frames(n) for n in (399, 400, 719, 720, 32000, 160000)] == [0, 1, 1, 2, 99, 499]


@pytest.mark.parametrize("n", [400, 719, 4000, 16000, 32000])
def test_hubert_oracle_matches_hf_and_sklearn(hgold, n):
    sd = synth.synth_hubert_state_dict(6)
    centers = synth.synth_kmeans_centers()
    wav = torch.from_numpy(synth.synth_waveform(n, seed=n))[None]
    units, dense = hr.encode(sd, centers, wav)
    want = hgold[f"n{n}/dense"]
    assert dense.shape == want.shape
    assert np.abs(dense.numpy() - want).max() <= 2e-4 * max(1.0, np.abs(want).max())
    # unit indices: equal except where the measured feature difference explains the other unit (derived bound)
    mism, amb = hr.check_units(units.numpy(), hgold[f"n{n}/units"], want, centers, x_dev=dense.numpy(), tag=f"n={n}")
    assert amb <= 0.1 * len(want) + 1
    if n <= 4000:
        cnn = hr.conv_feature_extractor(sd, wav)
        assert np.abs(cnn.numpy() - hgold[f"n{n}/cnn"]).max() <= 1e-4


def test_score_rounding_model_holds(hgold):
    """oracle.hubert_ref.unit_flip_allowed models the fp32 rounding of a score as sqrt(D) u (|c|^2 + 2 |x|.|c|): the measured
    fp32-vs-fp64 difference of the scores on the golden features stays far inside it (and far inside the old worst case D u)"""
    c = synth.synth_kmeans_centers()
    worst = 0.0
    for n in (4000, 16000, 32000):
        x = torch.from_numpy(hgold[f"n{n}/dense"])
        s32 = (c * c).sum(1)[None, :] - 2.0 * (x @ c.t())
        s64 = (c.double() ** 2).sum(1)[None, :] - 2.0 * (x.double() @ c.double().t())
        mag = (c.double() ** 2).sum(1)[None, :] + 2.0 * (x.double().abs() @ c.double().abs().t())
        worst = max(worst, float(((s32.double() - s64).abs() / mag).max()))
    u = 2.0 ** -24
    print(f"score rounding: worst |fl(s) - s| / mag = {worst / u:.2f} u (model sqrt(768) u = {768 ** 0.5:.0f} u, worst case 768 u)")
    assert worst <= 0.25 * 768 ** 0.5 * u


# ------------------------------------------------------------------------------------------
# the C restatement (oracle/host_ref.c) of the integer host logic
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coracle():
    import ctypes
    import __graft_entry__ as ge
    path = ge.build_oracle()
    L = ctypes.CDLL(path)
    L.oracle_dedup.restype = ctypes.c_int
    return L


def test_c_oracle_matches_reference_goldens(coracle, pgold):
    import ctypes
    for i in range(int(pgold["n_seqs"])):
        seq = np.ascontiguousarray(pgold[f"seq{i}"], dtype=np.int64)
        vals = np.zeros(len(seq), np.int64)
        counts = np.zeros(len(seq), np.int32)
        m = coracle.oracle_dedup(seq.ctypes.data_as(ctypes.c_void_p), len(seq),
                                 vals.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p))
        np.testing.assert_array_equal(vals[:m], pgold[f"dd_vals{i}"])
        np.testing.assert_array_equal(counts[:m], pgold[f"dd_counts{i}"])
        lens = np.ascontiguousarray(pgold[f"lens{i}"][0], dtype=np.float32)
        out = np.zeros(len(lens), np.int32)
        coracle.oracle_len_carryover(lens.ctypes.data_as(ctypes.c_void_p), len(lens), out.ctypes.data_as(ctypes.c_void_p))
        np.testing.assert_array_equal(out, pgold[f"lens_int{i}"])
    for j in range(4):
        x = np.ascontiguousarray(pgold[f"carry_in{j}"][0], dtype=np.float32)
        out = np.zeros(len(x), np.int32)
        coracle.oracle_len_carryover(x.ctypes.data_as(ctypes.c_void_p), len(x), out.ctypes.data_as(ctypes.c_void_p))
        np.testing.assert_array_equal(out, pgold[f"carry_out{j}"])


def test_c_oracle_postprocess_and_kmeans(coracle, hgold):
    import ctypes
    rs = np.random.RandomState(1)
    y = np.tanh(rs.standard_normal(4000).astype(np.float32) * 2)
    y[:3] = [1.0, -1.0, 0.999999]
    out = np.zeros_like(y)
    coracle.oracle_wav_postprocess(y.ctypes.data_as(ctypes.c_void_p), len(y), out.ctypes.data_as(ctypes.c_void_p))
    np.testing.assert_array_equal(out, gr.wav_postprocess(y))
    dense = np.ascontiguousarray(hgold["n16000/dense"], dtype=np.float32)
    centers = np.ascontiguousarray(synth.synth_kmeans_centers().numpy())
    units = np.zeros(len(dense), np.int64)
    coracle.oracle_kmeans_assign(dense.ctypes.data_as(ctypes.c_void_p), len(dense), 768,
                                 centers.ctypes.data_as(ctypes.c_void_p), 100, units.ctypes.data_as(ctypes.c_void_p))
    np.testing.assert_array_equal(units, hgold["n16000/units"])  # == sklearn KMeans.predict


def test_c_oracle_kmeans_f32_is_sklearn_on_the_goldens_and_breaks_ties_low(coracle, hgold):
    centers = synth.synth_kmeans_centers().numpy()
    for n in (400, 719, 4000, 16000, 32000):
        np.testing.assert_array_equal(kmeans_f32(coracle, hgold[f"n{n}/dense"], centers), hgold[f"n{n}/units"])  # sklearn predict
    x, c = kmeans_tie_cases()
    u = kmeans_f32(coracle, x, c)
    assert u[0] == 5 and u[1] == 5 and u[2] == 60 and u[3] == 60 and u[4] == 30 and u[5] == 30, u[:6]
    assert not np.isin(u, (17, 99, 31)).any()       # the higher member of a tied pair never wins
    assert u[20] == 0                               # NaN row: nothing beats +inf
    # float64 argmin agrees wherever it is not an exact tie (the f32 chain and float64 can only differ at rounding-level margins)
    import ctypes
    u64 = np.zeros(len(x), np.int64)
    xs, cs = np.ascontiguousarray(x[:20]), np.ascontiguousarray(c)
    coracle.oracle_kmeans_assign(xs.ctypes.data_as(ctypes.c_void_p), 20, 768, cs.ctypes.data_as(ctypes.c_void_p), 100,
                                 u64.ctypes.data_as(ctypes.c_void_p))
    np.testing.assert_array_equal(u[:20], u64[:20])
