"""What of the mel gradient (csrc/mel_grad.hip) can be held without a GPU.

A float64 numpy model of the kernel's INDEX arithmetic -- the mirrored staging, the transposed packing of the windowed
cosine / sine rows ([slab][cos | sin][q][lane][4], lane l, e -> frame sample 32 slab + (l & 31), bin 8 q + 4 (l >> 5) + e),
the operand maps of the 32 x 32 x 2 matrix instruction, the (row, column) walk of an accumulator into the overlap-add
strip of row stride hop | 1, the strips of overlapping tiles and the fold of both mirrors -- against float64 autograd
through tests/mel_ref.py, at hop 128 (four waves on four slabs at once) and hop 250 (the waves take turns; cells of one
accumulator wrap over strip rows).  Lengths: one frame with both mirrors inside it (n just above (n_fft - hop) / 2), and
two tiles and a bit.  The model is float64 throughout, so agreement is to rounding (1e-10 of the largest gradient).
Then the workspace size and the argument checks that need no device.
"""
import ctypes

import numpy as np
import pytest
import torch

import mel_ref

TF = 64
NARROW = dict(sr=16000, n_fft=512, num_mels=40, hop=128, win=400, fmin=50.0, fmax=7600.0)
ODD_HOP = dict(sr=16000, n_fft=512, num_mels=40, hop=250, win=512, fmin=0.0, fmax=None)


@pytest.fixture(scope="module")
def melmod():
    from dissc_amd import mel
    return mel


def model_vjp(x, cot, P, log):
    """grad of sum(cot * mel(x)) by the kernel's walk; x float64 [n], cot [num_mels, F]"""
    n_fft, hop, win, num_mels = P["n_fft"], P["hop"], P["win"], P["num_mels"]
    n, pad, F = len(x), (n_fft - hop) // 2, len(x) // hop
    fb = mel_ref.mel_filterbank(P["sr"], n_fft, num_mels, P["fmin"], P["fmax"]).astype(np.float32).astype(np.float64)
    used = np.nonzero(fb.any(axis=0))[0]
    b_lo, b_hi = int(used.min()), int(used.max())
    nblk, nmt = (b_hi - b_lo + 1 + 31) // 32, (num_mels + 31) // 32
    w_lo = (n_fft - win) // 2
    wnd = np.zeros(n_fft)
    wnd[w_lo:w_lo + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)
    s_lo, s_hi, nslab = w_lo // 32, (w_lo + win + 31) // 32, n_fft // 32
    rows, srs, SL = TF - 1 + (n_fft + hop - 1) // hop, hop | 1, (TF - 1) * hop + n_fft
    fast = hop % 32 == 0 and hop >= 128
    k = np.arange(n_fft)
    lane = np.arange(64)
    l31, hh = lane & 31, lane >> 5
    nt = (F + TF - 1) // TF
    strips = np.zeros((nt, SL))
    for tile in range(nt):
        i = np.arange(rows * hop)
        s = np.abs(tile * TF * hop - pad + i)
        s = np.where(s >= n, 2 * (n - 1) - s, s)
        stage = np.where((s >= 0) & (s < n), x[np.clip(s, 0, n - 1)], 0.0)
        frames = np.stack([stage[hop * f:hop * f + n_fft] for f in range(TF)], axis=1)  # [n_fft, TF]
        Ft = min(TF, F - tile * TF)
        # forward of the tile (for the log's factor), then G
        mel = np.zeros((nmt * 32, TF))
        spec = []
        for blk in range(nblk):
            bins = b_lo + blk * 32 + np.arange(32)
            live = (bins <= b_hi)[:, None]
            ph = 2 * np.pi * ((bins[:, None] * k[None, :]) % n_fft) / n_fft
            C, S = live * wnd * np.cos(ph), live * wnd * np.sin(ph)
            re, im = C @ frames, S @ frames
            mag = np.sqrt(re * re + im * im + 1e-9)
            basis = np.zeros((nmt * 32, 32))
            basis[:num_mels, live[:, 0]] = fb[:, bins[live[:, 0]]]
            mel += basis @ mag
            spec.append((C, S, re, im, mag, basis))
        G = np.zeros((nmt * 32, TF))
        G[:num_mels, :Ft] = cot[:, tile * TF:tile * TF + Ft]
        if log:
            G = G * np.where(mel > 1e-5, 1.0 / np.maximum(mel, 1e-300), 0.0)
        strip = np.zeros(rows * srs)
        for blk0 in range(0, nblk, 4):
            g = {}
            for wave in range(4):
                if blk0 + wave < nblk:
                    C, S, re, im, mag, basis = spec[blk0 + wave]
                    gm = basis.T @ G
                    # packed transposed rows of this block: [slab][cs][q][lane][e]
                    bidx = 8 * np.arange(4)[:, None, None] + 4 * hh[None, :, None] + np.arange(4)[None, None, :]  # [q][lane][e]
                    packT = np.stack([np.stack([W[bidx, 32 * sl + l31[None, :, None]] for W in (C, S)]) for sl in range(nslab)])
                    # accumulators as B operands: register 4 q + e of lane (j, h) holds bin 8 q + 4 h + e of frame j
                    breg = np.stack([(gm * re / mag), (gm * im / mag)])  # [cs][bin][frame]
                    g[wave] = (packT, breg)
            for step in range(s_lo - (3 if fast else 0), s_hi):
                touched = []
                for wave in sorted(g):
                    slab = step + wave if fast else step
                    if not s_lo <= slab < s_hi:
                        continue
                    packT, breg = g[wave]
                    A = packT[slab].reshape(2, 4, 2, 32, 4)  # [cs][q][h][i][e]
                    Bop = breg.reshape(2, 4, 2, 4, TF)       # bin 8 q + 4 h + e -> [cs][q][h][e][frame]
                    D = np.einsum("cqhie,cqhej->ij", A, Bop)  # [sample of the slab][frame]
                    cells = set()
                    for t in range(2):
                        for r in range(16):
                            for h in range(2):
                                q0 = 32 * slab + 4 * h
                                row0, c0 = q0 // hop, q0 % hop
                                c, row = c0 + (r & 3) + 8 * (r >> 2), row0
                                while c >= hop:
                                    c -= hop
                                    row += 1
                                at = (row + t * 32 + np.arange(32)) * srs + c
                                assert len(set(at)) == 32 and not (cells & set(at))
                                cells |= set(at)
                                strip[at] += D[(r & 3) + 8 * (r >> 2) + 4 * h, t * 32:(t + 1) * 32]
                    touched.append(cells)
                if fast:  # the waves of one step add without taking turns: their cells must be disjoint
                    for a in range(len(touched)):
                        for b in range(a + 1, len(touched)):
                            assert not (touched[a] & touched[b])
        ii = np.arange((Ft - 1) * hop + n_fft)
        strips[tile, :len(ii)] = strip[(ii // hop) * srs + ii % hop]
    ext = (F - 1) * hop + n_fft

    def cell(c):
        if c < 0 or c >= ext:
            return 0.0
        acc, t_hi = 0.0, min(c // (TF * hop), nt - 1)
        for t in range((c - SL) // (TF * hop) + 1 if c >= SL else 0, t_hi + 1):
            Ft, off = min(TF, F - t * TF), c - t * TF * hop
            if off < (Ft - 1) * hop + n_fft:
                acc += strips[t, off]
        return acc

    grad = np.zeros(n)
    for s in range(n):
        v = cell(s + pad)
        if 1 <= s <= pad:
            v += cell(pad - s)
        if n - 1 - pad <= s <= n - 2:
            v += cell(pad + 2 * (n - 1) - s)
        grad[s] = v
    return grad


@pytest.mark.parametrize("P", (NARROW, ODD_HOP), ids=("hop128", "hop250"))
@pytest.mark.parametrize("log", (False, True), ids=("linear", "log"))
def test_index_model_against_float64_autograd(P, log):
    pad = (P["n_fft"] - P["hop"]) // 2
    for n in (max(pad + 1, P["hop"]), pad + 7 + P["hop"], P["hop"] * TF + P["hop"] + 1):
        rs = np.random.RandomState(n)
        x = (0.3 * rs.standard_normal(n)).astype(np.float32).astype(np.float64)
        cot = rs.standard_normal((P["num_mels"], n // P["hop"]))
        xt = torch.from_numpy(x).requires_grad_(True)
        y = torch.nn.functional.pad(xt[None, None], (pad, pad), mode="reflect")[0, 0]
        basis = torch.from_numpy(mel_ref.mel_filterbank(P["sr"], P["n_fft"], P["num_mels"], P["fmin"], P["fmax"])).float().double()
        spec = torch.view_as_real(torch.stft(y[None], P["n_fft"], hop_length=P["hop"], win_length=P["win"],
                                             window=torch.hann_window(P["win"], dtype=torch.float64), center=False,
                                             return_complex=True))
        m = torch.matmul(basis, torch.sqrt(spec.pow(2).sum(-1) + 1e-9))
        if log:
            m = torch.log(torch.clamp(m, min=mel_ref.CLIP))
        (m[0] * torch.from_numpy(cot)).sum().backward()
        want = xt.grad.numpy()
        got = model_vjp(x, cot, P, log)
        e = np.abs(got - want).max() / np.abs(want).max()
        assert e < 1e-10, (n, e)


def test_tensor_restatement_equals_mel_ref():
    """mel_grad_ref.mel_t, which autograd can run through, is mel_ref.mel to the bit"""
    import mel_grad_ref
    rs = np.random.RandomState(3)
    x = (0.3 * rs.standard_normal((2, 3000))).astype(np.float32)
    for dtype in (torch.float32, torch.float64):
        for log in (True, False):
            assert torch.equal(mel_ref.mel(x, dtype=dtype, log=log), mel_grad_ref.mel_t(torch.from_numpy(x).to(dtype), log=log))
    kw = dict(n_fft=512, num_mels=40, sr=16000, hop=128, win=400, fmin=50.0, fmax=7600.0)
    assert torch.equal(mel_ref.mel(x, **kw), mel_grad_ref.mel_t(torch.from_numpy(x).double(), **kw))


def test_workspace_and_argument_checks_without_a_gpu(melmod):
    L = melmod.lib
    ms = melmod.MelSpectrogram()
    h = ms.handle()
    assert melmod.GRAD_TILE_FRAMES == 64
    a256 = lambda v: (v + 255) // 256 * 256
    for B, N in ((1, 385), (3, 64 * 256 + 1), (32, 160000)):
        tiles = B * ((N // 256 + 63) // 64)
        want = a256(max(tiles, 1) * 8) + a256(tiles * 96 * 64 * 4) + a256(tiles * (63 * 256 + 1024) * 4)
        assert L.dissc_mel_grad_workspace_bytes(h, B, N) == want
    assert L.dissc_mel_grad_workspace_bytes(None, 1, 1000) == 0 and L.dissc_mel_grad_workspace_bytes(h, 0, 1000) == 0
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused before anything is launched
    assert L.dissc_mel_backward(None, one, 1000, one, 1, one, 3, 0, one, 1000, one, 1 << 30, None) == -1
    assert L.dissc_mel_backward(h, None, 1000, one, 1, one, 3, 0, one, 1000, one, 1 << 30, None) == -1
    assert L.dissc_mel_backward(h, one, 1000, one, 1, None, 3, 0, one, 1000, one, 1 << 30, None) == -1
    assert L.dissc_mel_backward(h, one, 1000, one, 1, one, 3, 0, None, 1000, one, 1 << 30, None) == -1
    assert L.dissc_mel_backward(h, one, 1000, one, 1, one, 2, 0, one, 1000, one, 1 << 30, None) == -1  # ldF < ld / hop
    assert L.dissc_mel_backward(h, one, 1000, one, 1, one, 3, 2, one, 1000, one, 1 << 30, None) == -1  # unknown flag
    assert L.dissc_mel_backward(h, one, 1000, one, 1, one, 3, 0, one, 999, one, 1 << 30, None) == -1   # ldg < ld
    assert b"ldg" in L.dissc_last_error()
    assert L.dissc_mel_backward(h, one, 1000, one, 1, one, 3, 0, one, 1000, one, 100, None) == -2     # workspace too small
    assert b"workspace too small" in L.dissc_last_error()
    assert L.dissc_mel_backward(h, one, 1000, one, 1, one, 3, 0, one, 1000, None, 1 << 30, None) == -2
    assert L.dissc_mel_l1_grad(None, one, 1000, one, 1000, one, 1, one, one, one, 1000, one, 1 << 30, None) == -1
    assert L.dissc_mel_l1_grad(h, one, 1000, one, 1000, one, 1, None, one, one, 1000, one, 1 << 30, None) == -1
    assert L.dissc_mel_l1_grad(h, one, 1000, one, 1200, one, 1, one, one, one, 1100, one, 1 << 30, None) == -1  # ldg < ldb
    assert L.dissc_mel_l1_grad(h, one, 1000, one, 1000, one, 1, one, one, one, 1000, one, 8, None) == -2
    small = melmod.MelSpectrogram(hop_size=4, n_fft=64, win_size=64, num_mels=20)  # the forward takes hop 4, the gradient does not
    assert L.dissc_mel_backward(small.handle(), one, 1000, one, 1, one, 250, 0, one, 1000, one, 1 << 30, None) == -1
    assert b"hop >= 8" in L.dissc_last_error()
    with pytest.raises(melmod._lib.DisscError):
        melmod.MelSpectrogram().l1_loss(np.zeros((1, 4000), np.float32), np.zeros((1, 4000), np.float32))  # no device chosen
