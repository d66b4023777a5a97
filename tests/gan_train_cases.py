"""Shared by the tests of dissc_amd.gan_train, sr/train.py and the optimiser state (not a test module): a torch skeleton of the reference generator's
parameters in its registration order and the trainer's tiny configuration (gen_train_ref.TINY_CONFIG at 80-sample segments with the
64-point mel of tests/test_gpu_msd.py's full alternation), a synthetic training tree on disk and sr/train.py as a module."""
import torch
from torch.nn.utils import weight_norm

import gen_train_ref as GT

# TINY_CONFIG's generator has hop 2: 40 frames per 80-sample segment
TRAIN_CONFIG = dict(GT.TINY_CONFIG, segment_size=80, code_hop_size=2, sampling_rate=16000, n_fft=64, num_mels=20, hop_size=16,
                    win_size=64, fmin=0, fmax=8000, fmax_for_loss=None, batch_size=2, learning_rate=2e-4, adam_b1=0.8, adam_b2=0.99,
                    lr_decay=0.999, seed=1234, num_gpus=0, f0_normalize=True)


class GenSkeleton(torch.nn.Module):
    """the parameters of the reference's CodeGenerator in its registration order (Generator.__init__: conv_pre, ups, resblocks,
    conv_post; CodeGenerator.__init__ then dict and spkr), weight-normed as sr/models.py does; no forward"""

    def __init__(self, h):
        super().__init__()
        c0, E, nk = h["upsample_initial_channel"], h["embedding_dim"], len(h["resblock_kernel_sizes"])
        self.conv_pre = weight_norm(torch.nn.Conv1d(h["model_in_dim"], c0, 7))
        self.ups = torch.nn.ModuleList(weight_norm(torch.nn.ConvTranspose1d(c0 >> i, c0 >> (i + 1), k, u))
                                       for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])))
        self.resblocks = torch.nn.ModuleList()
        for i in range(len(h["upsample_rates"])):
            ch = c0 >> (i + 1)
            for k in h["resblock_kernel_sizes"]:
                blk = torch.nn.Module()
                blk.convs1 = torch.nn.ModuleList(weight_norm(torch.nn.Conv1d(ch, ch, k)) for _ in range(3))
                blk.convs2 = torch.nn.ModuleList(weight_norm(torch.nn.Conv1d(ch, ch, k)) for _ in range(3))
                self.resblocks.append(blk)
        assert len(self.resblocks) == nk * len(h["upsample_rates"])
        self.conv_post = weight_norm(torch.nn.Conv1d(c0 >> len(h["upsample_rates"]), 1, 7))
        self.dict = torch.nn.Embedding(h["num_embeddings"], E)
        self.spkr = torch.nn.Embedding(200, E)



def write_tree(root, n_wavs=6):
    """a synthetic training tree: root/wav/p<k>_<i>.wav (int16, one shorter than a segment, a partial hop behind the last frame),
    root/train.txt and root/val.txt (one manifest line per wav: audio, units, f0), root/f0_stats.pkl -> the path of its config"""
    import json
    import os
    import pickle

    import numpy as np

    from dissc_amd import formats
    rs = np.random.RandomState(0)
    os.makedirs(os.path.join(root, "wav"), exist_ok=True)
    h = dict(TRAIN_CONFIG)
    hop, lines = h["code_hop_size"], []
    for i in range(n_wavs):
        T = (25, 40, 64, 90, 41, 130)[i % 6]  # frames; 25 < 40: doubled by the sampler
        name = f"p{i % 3}_{i:03d}.wav"
        wav = (rs.uniform(-0.5, 0.5, T * hop + (i % hop)) * 32767).astype(np.int16)
        formats.write_wav(os.path.join(root, "wav", name), h["sampling_rate"], wav)
        f0 = rs.uniform(80, 300, T + 1)
        f0[rs.uniform(size=T + 1) < 0.3] = 0.0
        lines.append(json.dumps({"audio": f"somewhere/else/{name}", "units": [int(c) for c in rs.randint(0, h["num_embeddings"], T + 1)],
                                 "f0": [float(x) for x in f0]}))
    for split, part in (("train.txt", lines), ("val.txt", lines[2:5])):
        with open(os.path.join(root, split), "w") as f:
            f.write("\n".join(part) + "\n")
    with open(os.path.join(root, "f0_stats.pkl"), "wb") as f:
        pickle.dump({"f0_mean": 180.0, "f0_std": 50.0, "p0": {"mean": 150.0, "std": 40.0}, "p1": {"mean": 200.0, "std": 60.0}}, f)
    h.update(input_training_file=os.path.join(root, "train.txt"), input_validation_file=os.path.join(root, "val.txt"),
             train_base_path=os.path.join(root, "wav"), val_base_path=os.path.join(root, "wav"), f0_stats=os.path.join(root, "f0_stats.pkl"))
    path = os.path.join(root, "config_in.json")
    with open(path, "w") as f:
        json.dump(h, f)
    return path


def load_train_cli():
    """sr/train.py as a module"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sr", "train.py")
    spec = importlib.util.spec_from_file_location("dissc_sr_train", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
