"""Prosody metrics of reference eval.py on the MI355X: pitch earth-mover's distance, word / phone F0-frame-error and
the length errors, from F0 tracks that never leave the device.

    ev = ProsodyEvaluator(device='cuda:0')
    rows = ev.evaluate([(ref_wav, syn_wav, ref_grid, syn_grid_or_None), ...])   # one dict per job

The tracks come from dissc_amd.f0.YaaptTracker (the reference's get_yaapt, eval.py:26-33); the two kernels of
csrc/prosody_metrics.hip (C ABI ``dissc_track_emd`` / ``dissc_track_ffe``) turn them into one double per file / per
interval, and only those come back.  The host keeps what is bookkeeping in the reference too: the interval tables
(frame bounds in the reference's order of operations), the duration errors, the means over intervals.  Restated for
the tests in tests/eval_ref.py.  No CPU fallback.
"""
import ctypes
import time
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .audio import read_audio
from .f0 import YaaptTracker
from .textgrid import Interval, TextGrid

EMD_MAX_PAIR_FRAMES = 40000  # DISSC_EMD_MAX_PAIR_FRAMES
FFE_EMPTY_SYN, FFE_BAD_ENTRY = 1, 2


def _bind():
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.dissc_track_emd_workspace_bytes.argtypes = [i32, i32]
    lib.dissc_track_emd_workspace_bytes.restype = sz
    lib.dissc_track_emd.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, sz, vp]
    lib.dissc_track_ffe_workspace_bytes.argtypes = [i32]
    lib.dissc_track_ffe_workspace_bytes.restype = sz
    lib.dissc_track_ffe.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, sz, vp]


_bind()


def _tracks_and_table(tracks, table):
    if not (isinstance(tracks, torch.Tensor) and tracks.is_cuda and tracks.dtype == torch.float32 and tracks.dim() == 2):
        raise _lib.DisscError("dissc_amd.metrics works on a float32 [rows, frames] tensor on an MI355X")
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int32).reshape(-1, 6))
    return tracks.contiguous(), table, torch.from_numpy(table).to(tracks.device)


def _workspace(need, device):
    return torch.empty(max(int(need), 1), dtype=torch.uint8, device=device)


def track_emd(tracks, pairs):
    """tracks f32 [R, F] (device), pairs int [P, 6] rows (row_a, n_a, len_a, row_b, n_b, len_b): sample a is
    tracks[row_a, :n_a] followed by len_a - n_a zeros -> first Wasserstein distance per pair, f64 [P] (device)"""
    tracks, host, dev_table = _tracks_and_table(tracks, pairs)
    P = host.shape[0]
    out = torch.empty(P, dtype=torch.float64, device=tracks.device)
    if P == 0:
        return out
    most = int((host[:, 2].astype(np.int64) + host[:, 5]).max())
    with torch.cuda.device(tracks.device):
        need = lib.dissc_track_emd_workspace_bytes(P, min(max(most, 0), 2 ** 31 - 1))
        ws = _workspace(need, tracks.device)
        check(lib.dissc_track_emd(tracks.data_ptr(), tracks.shape[0], tracks.shape[1], dev_table.data_ptr(), P,
                                  min(max(most, 0), 2 ** 31 - 1), out.data_ptr(), ws.data_ptr(), need,
                                  _lib.current_stream_ptr(tracks.device)), "dissc_track_emd")
    return out


def track_ffe(tracks, intervals):
    """tracks f32 [R, F] (device), intervals int [S, 6] rows (row_ref, lo_ref, hi_ref, row_syn, lo_syn, hi_syn) with
    0 <= lo <= hi <= F -> (ffe f64 [S], status i32 [S]) on the device; status FFE_EMPTY_SYN marks an empty generated
    slice against a non-empty reference slice (the reference's ValueError), an empty reference slice gives NaN"""
    tracks, host, dev_table = _tracks_and_table(tracks, intervals)
    S = host.shape[0]
    ffe = torch.empty(S, dtype=torch.float64, device=tracks.device)
    status = torch.empty(S, dtype=torch.int32, device=tracks.device)
    if S == 0:
        return ffe, status
    with torch.cuda.device(tracks.device):
        need = lib.dissc_track_ffe_workspace_bytes(S)
        ws = _workspace(need, tracks.device)
        check(lib.dissc_track_ffe(tracks.data_ptr(), tracks.shape[0], tracks.shape[1], dev_table.data_ptr(), S,
                                  ffe.data_ptr(), status.data_ptr(), ws.data_ptr(), need,
                                  _lib.current_stream_ptr(tracks.device)), "dissc_track_ffe")
    return ffe, status


# ---------------------------------------------------------------------------------------------------------
# host bookkeeping (reference eval.py:50-57, 96-129)
# ---------------------------------------------------------------------------------------------------------
def frame_index(t, sr=16000):
    """TextGrid time -> index into the 5 ms track, left to right in double like the reference (int() truncates)"""
    return int(t * sr * 0.005 * 2.5 + 2)


def slice_bounds(t_min, t_max, n, sr=16000):
    """bounds of track[frame_index(t_min):frame_index(t_max)] on n frames as Python slices them: 0 <= lo <= hi <= n"""
    lo, hi, _ = slice(frame_index(t_min, sr), frame_index(t_max, sr)).indices(n)
    return lo, max(lo, hi)


def emd_lengths(n_ref_frames, n_syn_frames, n_ref_samples, n_syn_samples):
    """sizes (ref, syn) after the reference's zero extension (eval.py:98-101: the second branch tests the waveforms)"""
    if n_ref_frames > n_syn_frames:
        return n_ref_frames, n_ref_frames
    if n_ref_samples < n_syn_samples:
        return n_syn_frames, n_syn_frames
    return n_ref_frames, n_syn_frames


def tier_intervals(ref_tier, syn_tier, ref_max_time):
    """the marked intervals of one tier of both grids; without a generated grid, uniform pseudo-intervals"""
    ref_iv = [f for f in ref_tier if f.mark]
    if syn_tier is not None:
        return ref_iv, [f for f in syn_tier if f.mark]
    n = len(ref_tier) + 1
    return ref_iv, [Interval(ref_max_time / n * i, ref_max_time / n * (i + 1), inv.mark)
                    for i, inv in enumerate(ref_tier) if inv.mark]


def load_wav(path):
    """first channel as float32 in [-1, 1) and the sample rate (what torchaudio.load gives the reference)"""
    x, sr = read_audio(path)
    if x.ndim == 2:
        x = x[:, 0]
    return x.astype(np.float32), sr


def peak_normalize(w):
    """librosa.util.normalize(w) * 0.95 (reference eval.py:30) [3P-unverified]: divide by max |w|, silence stays silence"""
    w = np.asarray(w, dtype=np.float32)
    peak = np.max(np.abs(w)) if w.size else 0.0
    return (w / peak if peak > np.finfo(np.float32).tiny else w) * np.float32(0.95)


class ProsodyEvaluator:
    """jobs (ref_wav, syn_wav, ref_grid, syn_grid | None) -> one dict per job with 'len', 'emd' and those of 'p_len',
    'p_ffe', 'w_len', 'w_ffe' the reference appends for that file.  A waveform is a path or a 1-D array @16 kHz, a
    grid a path or a dissc_amd.textgrid.TextGrid.  Every distinct reference waveform (same path, or the same array
    object) is tracked once; the work is cut into batches of about ``batch_seconds`` of audio."""

    def __init__(self, device="cuda:0", batch_seconds=640.0, sr=16000):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DisscError("dissc_amd.metrics.ProsodyEvaluator runs on an MI355X only")
        self.sr = int(sr)
        self.batch_seconds = float(batch_seconds)
        self.tracker = YaaptTracker(device=self.device, fs=self.sr)
        self.timings = None  # set to {} to collect wall seconds per stage: 'read' (WAVs, TextGrids), 'track', 'metrics' (the two
        # launches + D2H); what is left of the wall time is the host's tables and means.  Synchronises after each stage

    def _timed(self, stage, fn, *args):
        if self.timings is None:
            return fn(*args)
        t0 = time.perf_counter()
        res = fn(*args)
        torch.cuda.synchronize(self.device)
        self.timings[stage] = self.timings.get(stage, 0.0) + time.perf_counter() - t0
        return res

    def _wave(self, w):
        if isinstance(w, (str, bytes)) or hasattr(w, "__fspath__"):
            x, sr = load_wav(w)
            if sr != self.sr:
                raise ValueError(f"{w}: {sr} Hz, expected {self.sr}")
            return x
        return np.asarray(w, dtype=np.float32)

    def _grid(self, g):
        if g is None or isinstance(g, TextGrid):
            return g
        if str(g) not in self._grids:  # a reference grid serves every source speaker's file
            self._grids[str(g)] = TextGrid.fromFile(g)
        return self._grids[str(g)]

    @staticmethod
    def _key(w):
        return str(w) if isinstance(w, (str, bytes)) or hasattr(w, "__fspath__") else id(w)

    def evaluate(self, jobs):
        jobs = list(jobs)
        out = [None] * len(jobs)
        self._grids = {}
        order = sorted(range(len(jobs)), key=lambda i: (str(type(self._key(jobs[i][0]))), self._key(jobs[i][0])))
        budget = self.batch_seconds * self.sr
        cache = {}  # reference key -> (device track [n], samples): the references of the previous batch
        i = 0
        while i < len(order):
            waves, rows, used, batch = [], [], 0, []  # rows: per job (ref slot, syn slot); slot = ('new', k) | ('old', key)
            new_refs = {}
            while i < len(order) and (not batch or used < budget):
                ref_w, syn_w = jobs[order[i]][0], jobs[order[i]][1]
                key = self._key(ref_w)
                if key in new_refs:
                    rslot = new_refs[key]
                elif key in cache:
                    rslot = ("old", key)
                else:
                    waves.append(self._timed("read", self._wave, ref_w))
                    used += len(waves[-1])
                    rslot = new_refs[key] = ("new", len(waves) - 1)
                waves.append(self._timed("read", self._wave, syn_w))
                used += len(waves[-1])
                rows.append((rslot, ("new", len(waves) - 1)))
                batch.append(order[i])
                i += 1
            cache = self._batch(jobs, batch, waves, rows, cache, out)
        return out

    def _batch(self, jobs, batch, waves, rows, cache, out):
        f0, counts = self._timed("track", lambda: self.tracker([peak_normalize(w) for w in waves], on_device=True))
        return self._score(jobs, batch, waves, rows, cache, out, f0, counts)

    @staticmethod
    def _launch(tracks, pairs, table):
        """the two launches and the copies of their results: all that crosses back from the device"""
        emd = track_emd(tracks, pairs)
        ffe, status = track_ffe(tracks, table)
        return emd.cpu().numpy(), ffe.cpu().numpy(), status.cpu().numpy()

    def _score(self, jobs, batch, waves, rows, cache, out, f0, counts):
        old = sorted({r[1] for r, _ in rows if r[0] == "old"}, key=str)
        if old:  # references tracked by the previous batch ride along as extra rows
            ld = max(f0.shape[1], max(cache[k][0].numel() for k in old))
            tracks = torch.zeros(f0.shape[0] + len(old), ld, dtype=torch.float32, device=self.device)
            tracks[:f0.shape[0], :f0.shape[1]] = f0
            for j, k in enumerate(old):
                tracks[f0.shape[0] + j, :cache[k][0].numel()] = cache[k][0]
        else:
            tracks = f0
        old_row = {k: f0.shape[0] + j for j, k in enumerate(old)}

        def place(slot):  # -> (row, frames, samples)
            if slot[0] == "new":
                return slot[1], counts[slot[1]], len(waves[slot[1]])
            return old_row[slot[1]], cache[slot[1]][0].numel(), cache[slot[1]][1]

        pairs, table, plan = [], [], []
        for job, (rslot, sslot) in zip(batch, rows):
            rrow, rn, rsamp = place(rslot)
            srow, sn, ssamp = place(sslot)
            res = {"len": abs(rsamp - ssamp)}
            lr, ls = emd_lengths(rn, sn, rsamp, ssamp)
            pairs.append((srow, sn, ls, rrow, rn, lr))
            ref_grid, syn_grid = (self._timed("read", self._grid, g) for g in jobs[job][2:4])
            tiers = []
            for key, tier in (("p", 1), ("w", 0)):
                try:
                    ref_iv, syn_iv = tier_intervals(ref_grid[tier], syn_grid[tier] if syn_grid else None, ref_grid.maxTime)
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")  # mean of an empty tier: NaN like the reference
                        res[key + "_len"] = np.abs(np.array([v.duration() for v in ref_iv]) -
                                                   np.array([v.duration() for v in syn_iv])).mean()
                except ValueError:  # unequal interval counts: the file leaves this tier's two lists
                    continue
                first = len(table)
                for k in range(len(ref_iv)):  # a shorter generated list raises IndexError here as in the reference
                    # sliced at the zero-EXTENDED lengths: the reference cuts its FFE slices from the tracks it padded
                    # for the EMD (rows are 0 beyond their frames, and lr, ls <= the row length)
                    table.append((rrow, *slice_bounds(ref_iv[k].minTime, ref_iv[k].maxTime, lr, self.sr),
                                  srow, *slice_bounds(syn_iv[k].minTime, syn_iv[k].maxTime, ls, self.sr)))
                tiers.append((key, first, len(table)))
            out[job] = res
            plan.append((job, tiers))
        emd, ffe, status = self._timed("metrics", self._launch, tracks, pairs, table)
        if np.any(status == FFE_BAD_ENTRY):
            raise _lib.DisscError("dissc_track_ffe refused an interval table entry")
        for n, (job, tiers) in enumerate(plan):
            out[job]["emd"] = emd[n]
            for key, lo, hi in tiers:
                if not np.any(status[lo:hi] == FFE_EMPTY_SYN):  # the reference's ValueError drops the file's FFE only
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        out[job][key + "_ffe"] = np.mean(ffe[lo:hi])
        keep = {}
        for (rslot, _), job in zip(rows, batch):
            key = self._key(jobs[job][0])
            if key not in keep:
                row, n, samp = place(rslot)
                keep[key] = (tracks[row, :n].clone(), samp)
        return keep
