"""The vocoder's GAN trainer (reference sr/train.py): the segment sampler that makes a step's batch one gather launch from a
device-resident corpus (``dissc_segment_*``, csrc/segment_gather.hip), torch's default initialisation of the three modules, and
``GanTrainer``, which runs the reference's two lines per step on dissc_amd.nn's modules with nn.AdamW and reads and writes the
reference's ``g_*`` / ``do_*`` checkpoints.

    sampler = SegmentSampler(h, items, seed=1234)          # items: sr/validate.py's prepare_items on the training manifest
    trainer = GanTrainer(h, "cuda:0"); trainer.init(seed=h.seed)   # or trainer.load(checkpoint_dir)
    for batch in sampler: losses = trainer.step(batch)
    trainer.decay_lr(); trainer.save(checkpoint_dir, steps, epoch)
"""
import ctypes
import glob
import math
import os
import random

import numpy as np
import torch

from . import nn
from ._lib import DisscError, check, current_stream_ptr, lib
from .generator import AttrDict


def _bind():
    vp, i32, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.dissc_segment_max_batch.argtypes = []
    lib.dissc_segment_create.argtypes = [i32, ctypes.POINTER(ll), i32, vp, vp, vp, vp, ctypes.POINTER(vp)]
    lib.dissc_segment_destroy.argtypes, lib.dissc_segment_destroy.restype = [vp], None
    lib.dissc_segment_interval_end.argtypes = [vp, i32, i32, ctypes.POINTER(ll)]
    lib.dissc_segment_gather.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), i32, i32, vp, vp, vp, vp, vp]


_bind()

SEGMENT_MAX_BATCH = int(lib.dissc_segment_max_batch())  # rows one gather launch takes
# config options this trainer refuses by name (the modules refuse the VQ-VAE options they know themselves)
UNSUPPORTED = ("f0_median", "f0_vq_params", "code_vq_params")


def refuse_unsupported(h, environ=None):
    """the options out of scope, by name, before anything is built"""
    environ = os.environ if environ is None else environ
    if int(environ.get("WORLD_SIZE", 1) or 1) > 1 or int(h.get("num_gpus", 1) or 1) > 1:
        raise NotImplementedError("WORLD_SIZE / num_gpus > 1: the GAN trainer runs on one GPU (no gradient all-reduce)")
    for k in UNSUPPORTED:
        if h.get(k, None):
            raise NotImplementedError(f"config option '{k}' is not supported by the GAN trainer")


# ---- the sampler's law on the host (the GPU kernel does the same per element) -----------------------------------------------
def interval_end(frames, hop, segment):
    """the last legal start_step of an utterance of ``frames`` frames: N' / hop - segment / hop, N' = frames hop 2^j the length
    after CodeDataset.__getitem__'s doublings (reference sr/dataset.py:255-259, 209)"""
    if frames < 1 or hop < 1:
        raise DisscError(f"interval_end: {frames} frames of {hop} samples; need at least one of each")
    n = frames * hop
    while n < segment:
        n *= 2
    return n // hop - segment // hop


def crop_host(item, start_step, hop, segment):
    """one row of a batch on the host -> (y f32 [segment], code i64 [F], f0 f32 [F]): doubling is periodic, so sample i of the
    crop is sample (start_step hop + i) mod n and frame j is frame (start_step + j) mod T"""
    T = len(item["code"])
    i = (start_step * hop + np.arange(segment)) % (T * hop)
    j = (start_step + np.arange(segment // hop)) % T
    return (np.asarray(item["gt"], np.float32)[i], np.asarray(item["code"], np.int64)[j], np.asarray(item["f0"], np.float32)[j])


class SegmentSampler:
    """The training batches of the reference's single-GPU loader (CodeDataset with eval_mode False behind a DataLoader with
    shuffle=False, no sampler, drop_last=True) from a corpus that lives on the device: batch i is items [i B, (i + 1) B) in
    manifest order, each cropped to ``segment_size`` samples at a random whole number of code hops, in ONE launch.

    ``items``: sr/validate.py's ``prepare_items`` (prepared ground truth ``gt`` f32 [T hop], trimmed ``code`` [T],
    speaker-normalised ``f0`` [T], ``spkr``).  F0 normalisation is element-wise, so it commutes with the crop; ``f0_median``
    takes the crop's median in the reference and would not: refused.

    The law: the same distribution and order as the reference -- start_step = randint(0, interval_end) per item, in item order,
    from a private random.Random(seed).  The draw SEQUENCE is not the reference's: its validation set re-seeds the global
    generator (random.seed(1234) in CodeDataset.__init__) and shares it with the training set."""

    def __init__(self, h, items, seed=1234, device="cuda:0"):
        h = AttrDict(h)
        if h.get("f0_median", False):
            raise NotImplementedError("config option 'f0_median' is not supported by SegmentSampler: the reference takes the "
                                      "median of the CROP, which does not commute with cropping a prepared corpus")
        self.hop, self.segment, self.batch_size = int(h.code_hop_size), int(h.segment_size), int(h.batch_size)
        if self.segment % self.hop != 0 or self.segment < self.hop:
            raise DisscError(f"SegmentSampler: segment_size {self.segment} must be a positive multiple of code_hop_size {self.hop}")
        if not 1 <= self.batch_size <= SEGMENT_MAX_BATCH:
            raise DisscError(f"SegmentSampler: batch_size {self.batch_size}; one gather launch takes 1 .. {SEGMENT_MAX_BATCH} rows")
        if not items:
            raise DisscError("SegmentSampler: no items")
        self.device = torch.device(device)
        self.frames = [len(it["code"]) for it in items]
        for u, it in enumerate(items):
            if self.frames[u] < 1 or len(it["f0"]) != self.frames[u] or len(it["gt"]) != self.frames[u] * self.hop:
                raise DisscError(f"SegmentSampler: item {u} ({it.get('name', '?')}): {len(it['code'])} units, {len(it['f0'])} f0 values, "
                                 f"{len(it['gt'])} samples; need T >= 1, T and T * {self.hop}")
        audio = np.ascontiguousarray(np.concatenate([np.asarray(it["gt"], np.float32) for it in items]))
        codes = np.ascontiguousarray(np.concatenate([np.asarray(it["code"]) for it in items]).astype(np.int32))
        f0 = np.ascontiguousarray(np.concatenate([np.asarray(it["f0"], np.float32) for it in items]))
        spkr = np.ascontiguousarray(np.array([int(it["spkr"]) for it in items], np.int32))
        fr = (ctypes.c_longlong * len(items))(*self.frames)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.dissc_segment_create(len(items), fr, self.hop, audio.ctypes.data, codes.ctypes.data, f0.ctypes.data,
                                           spkr.ctypes.data, ctypes.byref(self._h)), "dissc_segment_create")
        self.n_items = len(items)
        self.rng = random.Random(seed)

    def __del__(self):
        try:
            lib.dissc_segment_destroy(self._h)
        except Exception:
            pass

    def __len__(self):
        """batches per epoch (drop_last)"""
        return self.n_items // self.batch_size

    def interval_end(self, u):
        out = ctypes.c_longlong(0)
        check(lib.dissc_segment_interval_end(self._h, int(u), self.segment, ctypes.byref(out)), "dissc_segment_interval_end")
        return out.value

    def draw(self, i):
        """the (utterance, start_step) table of batch i of an epoch: one randint per item, in item order"""
        return [(u, self.rng.randint(0, interval_end(self.frames[u], self.hop, self.segment)))
                for u in range(i * self.batch_size, (i + 1) * self.batch_size)]

    def gather(self, table, out=None):
        """table: (utterance, start_step) pairs -> {"y" f32 [B, 1, segment], "code" i64 [B, F], "f0" f32 [B, 1, F], "spkr" i64
        [B, 1]} on the device, new tensors or the four of ``out``; validated on the host, one launch"""
        B, F = len(table), self.segment // self.hop
        for b, row in enumerate(table):  # a ctypes int32 array wraps silently: 2^32 + k would pass the host validation as k
            if len(row) != 2 or not all(-2 ** 31 <= int(x) < 2 ** 31 for x in row):
                raise DisscError(f"SegmentSampler.gather: row {b}: {tuple(row)} is no (utterance, start_step) pair of int32")
        tab = (ctypes.c_int32 * max(2 * B, 1))(*[int(x) for row in table for x in row])
        if out is None:
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
            out = (mk((B, 1, self.segment), torch.float32), mk((B, F), torch.int64), mk((B, 1, F), torch.float32), mk((B, 1), torch.int64))
        y, code, f0, spkr = out
        for t, shape, dt, name in ((y, (B, 1, self.segment), torch.float32, "y"), (code, (B, F), torch.int64, "code"),
                                   (f0, (B, 1, F), torch.float32, "f0"), (spkr, (B, 1), torch.int64, "spkr")):
            if tuple(t.shape) != shape or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise DisscError(f"SegmentSampler.gather: out '{name}' must be a contiguous {dt} tensor {shape} on {self.device}")
        with torch.cuda.device(self.device):
            check(lib.dissc_segment_gather(self._h, tab, B, self.segment, y.data_ptr(), code.data_ptr(), f0.data_ptr(), spkr.data_ptr(),
                                           current_stream_ptr(self.device)), "dissc_segment_gather")
        return {"y": y, "code": code, "f0": f0, "spkr": spkr}

    def batch(self, i):
        return self.gather(self.draw(i))

    def __iter__(self):
        """one epoch"""
        for i in range(len(self)):
            yield self.batch(i)


# ---- fresh weights ------------------------------------------------------------------------------------------------------------
def init_state_dicts(h, seed):
    """(generator, mpd, msd) state dicts under the reference's keys, drawn on the CPU from torch's default initialisation: for a
    Conv1d / ConvTranspose1d / Conv2d, weight_v / weight_orig and bias uniform in +- 1 / sqrt(fan_in), fan_in = weight.size(1) *
    k as torch computes it (for a ConvTranspose1d that is out_channels * k); weight_g = the norm of its weight_v slice (what
    weight_norm sets when it wraps a layer); Embedding N(0, 1); unit-norm normal weight_u / weight_v for the spectral norm.
    The reference's init_weights (sr/models.py) writes normal(0, 0.01) into the RECOMPUTED .weight of a weight-normed conv,
    which the weight-norm hook overwrites at the next forward: it has no effect and is not reproduced.  Only the distributions
    are claimed, not torch's draws."""
    gen = torch.Generator().manual_seed(int(seed))
    uni = lambda shape, bound: (torch.rand(shape, generator=gen) * 2 - 1) * bound
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, generator=gen), dim=0, eps=1e-12)

    def conv(sd, name, shape, nb, tail=(), spectral=False):
        bound = 1.0 / math.sqrt(shape[1] * shape[2])
        w = uni(tuple(shape) + tail, bound)
        sd[name + ".bias"] = uni((nb,), bound)
        if spectral:
            sd[name + ".weight_orig"] = w
            sd[name + ".weight_u"], sd[name + ".weight_v"] = unit(shape[0]), unit(shape[1] * shape[2])
        else:
            sd[name + ".weight_g"] = w.reshape(shape[0], -1).norm(dim=1).reshape((shape[0],) + (1,) * (w.dim() - 1))
            sd[name + ".weight_v"] = w

    G, P, S = nn.CodeGenerator(h), nn.MultiPeriodDiscriminator(), nn.MultiScaleDiscriminator()
    g, p, s = {}, {}, {}
    for name, shape, nb in G.layers:
        conv(g, name, shape, nb)
    E = int(G.h.embedding_dim)
    g["dict.weight"] = torch.randn((int(G.h.num_embeddings), E), generator=gen)
    if G.multispkr:
        g["spkr.weight"] = torch.randn((G.N_SPEAKERS, E), generator=gen)
    for name, shape, nb in P.layers:
        conv(p, name, shape, nb, tail=(1,))
    for name, shape, nb in S.layers0:
        conv(s, name, shape, nb, spectral=True)
    for name, shape, nb in S.layers12:
        conv(s, name, shape, nb)
    return g, p, s


# ---- the trainer ----------------------------------------------------------------------------------------------------------------
def scan_checkpoint(cp_dir, prefix):
    """the latest checkpoint by sorted glob (reference sr/utils.py), or None"""
    cps = sorted(glob.glob(os.path.join(cp_dir, prefix + "????????")))
    return cps[-1] if cps else None


class GanTrainer:
    """The reference's training step (sr/train.py:142-191) on one MI355X: nn.CodeGenerator, nn.MultiPeriodDiscriminator and
    nn.MultiScaleDiscriminator, the fused losses, MelSpectrogram.l1_loss, and two nn.AdamW(lr=h.learning_rate, betas=(h.adam_b1,
    h.adam_b2)) -- optim_g over the generator's leaves, optim_d over msd's and then mpd's, the reference's order.
    precision: "fp32" or "split_bf16", handed to the three modules (their nn.conv1d layers; nn.conv1d says what it means).  A
    checkpoint does not record it: one written in either mode loads and resumes in the other."""

    def __init__(self, h, device="cuda:0", precision="fp32"):
        from .mel import MelSpectrogram
        self.h = AttrDict(h)
        refuse_unsupported(self.h)
        self.device = torch.device(device)
        self.precision = precision
        self.generator = nn.CodeGenerator(self.h, precision=precision).to(self.device)
        self.mpd = nn.MultiPeriodDiscriminator(precision=precision).to(self.device)
        self.msd = nn.MultiScaleDiscriminator(precision=precision).to(self.device)
        self.mel = MelSpectrogram.from_config(self.h, for_loss=True).to(self.device)
        self.optim_g = self.optim_d = None

    # -- weights ---------------------------------------------------------------------------------------------------------------
    def load_state_dicts(self, generator, mpd, msd):
        """the three modules from reference-format state dicts; fresh optimisers over their leaves"""
        self.generator.load_state_dict(generator)
        self.mpd.load_state_dict(mpd)
        self.msd.load_state_dict(msd)
        kw = dict(lr=float(self.h.learning_rate), betas=(float(self.h.adam_b1), float(self.h.adam_b2)))
        self.optim_g = nn.AdamW(self.generator.parameters(), **kw)
        self.optim_d = nn.AdamW(self.msd.parameters() + self.mpd.parameters(), **kw)
        return self

    def init(self, seed):
        """fresh weights: init_state_dicts(h, seed)"""
        return self.load_state_dicts(*init_state_dicts(self.h, seed))

    @property
    def lr(self):
        return self.optim_g.lr

    def decay_lr(self):
        """once per epoch: ExponentialLR's chainable form, lr *= h.lr_decay in Python double, both optimisers"""
        for opt in (self.optim_g, self.optim_d):
            opt.lr = opt.lr * float(self.h.lr_decay)

    # -- the step ----------------------------------------------------------------------------------------------------------------
    def step(self, batch):
        """batch: {"y" [B, 1, segment], "code", "f0", "spkr"} on the device (SegmentSampler's) -> the step's losses as device
        scalars {"loss_disc_all", "loss_gen_all", "loss_mel", "mel_error", ...}; the reference's lines in the reference's
        order: G forward; both discriminators on y_hat.detach(), (loss_disc_s + loss_disc_f).backward(), optim_d.step(); both
        discriminators with param_grads=False, loss_gen_s + loss_gen_f + loss_fm_s + loss_fm_f + 45 mel into backward(),
        optim_g.step()"""
        G, P, S = self.generator, self.mpd, self.msd
        y = batch["y"]
        x = {"code": batch["code"]}
        if G.f0:
            x["f0"] = batch["f0"]
        if G.multispkr:
            x["spkr"] = batch["spkr"]
        y_hat = G(**x)
        if y_hat.shape != y.shape:
            raise DisscError(f"GanTrainer.step: the generator's output {tuple(y_hat.shape)} is not the batch's y {tuple(y.shape)}")
        self.optim_d.zero_grad()
        loss_disc_f = nn.discriminator_loss(P(y, y_hat.detach()))[0]
        loss_disc_s = nn.discriminator_loss(S(y, y_hat.detach()))[0]
        loss_disc_all = loss_disc_s + loss_disc_f
        loss_disc_all.backward()
        self.optim_d.step()
        self.optim_g.zero_grad()
        mel_error = self.mel.l1_loss(y, y_hat)
        loss_mel = mel_error * 45
        out_f, out_s = P(y, y_hat, param_grads=False), S(y, y_hat, param_grads=False)
        loss_fm_f, loss_fm_s = nn.feature_loss(out_f), nn.feature_loss(out_s)
        loss_gen_f, loss_gen_s = nn.generator_loss(out_f)[0], nn.generator_loss(out_s)[0]
        loss_gen_all = loss_gen_s + loss_gen_f + loss_fm_s + loss_fm_f + loss_mel
        loss_gen_all.backward()
        self.optim_g.step()
        det = lambda t: t.detach()
        return {"loss_disc_all": det(loss_disc_all), "loss_disc_f": det(loss_disc_f), "loss_disc_s": det(loss_disc_s),
                "loss_gen_all": det(loss_gen_all), "loss_gen_f": det(loss_gen_f), "loss_gen_s": det(loss_gen_s),
                "loss_fm_f": det(loss_fm_f), "loss_fm_s": det(loss_fm_s), "loss_mel": det(loss_mel), "mel_error": det(mel_error)}

    # -- checkpoints ---------------------------------------------------------------------------------------------------------------
    def save(self, path, steps, epoch):
        """writes path/g_{steps:08d} = {'generator'} and path/do_{steps:08d} = {'mpd', 'msd', 'optim_g', 'optim_d', 'steps',
        'epoch'}, the optimiser states over the reference's per-layer parameters (nn.optimizer_state_to_reference)"""
        os.makedirs(path, exist_ok=True)
        g, do = os.path.join(path, f"g_{steps:08d}"), os.path.join(path, f"do_{steps:08d}")
        torch.save({"generator": self.generator.state_dict()}, g)
        torch.save({"mpd": self.mpd.state_dict(), "msd": self.msd.state_dict(),
                    "optim_g": nn.optimizer_state_to_reference(self.optim_g, [self.generator]),
                    "optim_d": nn.optimizer_state_to_reference(self.optim_d, [self.msd, self.mpd]),
                    "steps": int(steps), "epoch": int(epoch)}, do)
        return g, do

    def load(self, path):
        """the latest g_* / do_* of a directory -> {'steps', 'epoch'} as saved, or None where there is none (the caller resumes
        at steps + 1 and last_epoch = epoch, as the reference does); the learning rate comes from the checkpoint"""
        g, do = (scan_checkpoint(path, p) for p in ("g_", "do_")) if os.path.isdir(path) else (None, None)
        if g is None or do is None:
            return None
        sd_g, sd_do = torch.load(g, map_location="cpu"), torch.load(do, map_location="cpu")
        self.load_state_dicts(sd_g["generator"], sd_do["mpd"], sd_do["msd"])
        self.optim_g.load_state_dict(nn.optimizer_state_from_reference(sd_do["optim_g"], [self.generator]))
        self.optim_d.load_state_dict(nn.optimizer_state_from_reference(sd_do["optim_d"], [self.msd, self.mpd]))
        return {"steps": int(sd_do["steps"]), "epoch": int(sd_do["epoch"])}

    def sampler(self, items, seed=1234):
        return SegmentSampler(self.h, items, seed, self.device)

    def generator_state_dict(self):
        """the live generator under the reference's keys (what a g_* file holds): for sr/validate.py's scorer"""
        return self.generator.state_dict()
