"""Shared by the predictor-training tests (tests/test_train_oracle.py, test_gpu_train.py, test_gpu_train_stages.py; not a test
module): the compact form the goldens store large tensors in, the biases whose gradient is rounding noise, the initial
checkpoints, and the comparison that tolerates a LeakyReLU branch flip."""
import numpy as np

import synthdata as synth


def compact(a):
    a = np.asarray(a)
    if a.size <= 4096:
        return a.copy()
    f = a.reshape(-1).astype(np.float64)
    return np.concatenate([[f.sum(), np.abs(f).sum(), (f * f).sum()], f[::max(1, f.size // 509)]])


BN_FED_BIASES = {"len": {"cnn1.bias"} | {f"cnn1{i}.bias" for i in range(1, 7)},
                 "new": {"cnn2.bias"},
                 "base": {"cnn1.bias", "cnn_class1.bias", "cnn_reg1.bias"} | {f"cnn1{i}.bias" for i in range(1, 8)}}


def initial_state(kind, n_spk=108):
    if kind == "len":
        return synth.synth_len_state_dict(100, n_spk)
    return synth.synth_pitch_state_dict(kind, 100, n_spk)


def _flip_tolerant(got, want, what, l2=0.03):
    """LeakyReLU's derivative jumps at 0, so an activation within fp32 rounding of 0 takes the other branch in one of
    the two implementations and perturbs the gradients that pass through it (a few rows, O(1 %) of the norm).  A real
    defect moves everything: require the typical (median) element to agree tightly and the whole tensor in the l2 sense."""
    a, b = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.median(np.abs(a - b)) <= 1e-3 * np.abs(b).max() + 1e-6, (what, float(np.median(np.abs(a - b))))
    assert np.linalg.norm(a - b) <= l2 * np.linalg.norm(b) + 1e-6, (what, np.linalg.norm(a - b) / np.linalg.norm(b))
