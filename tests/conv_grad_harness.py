"""What the tests of the two differentiable conv layers (dissc_amd.nn.conv1d, nn.conv_transpose1d) share (not a test module):
the layer spec, seeded data, one forward + backward through a layer function, the ragged lengths around the chunk and a partial
boundary, and the two check bodies.  The bodies take ``run`` as a parameter -- on the GPU a partial of run() below, in
tests/test_conv_grad_cpu.py a CPU stand-in with seeded defects -- and the bars of the forward and the data gradient from the
caller, whose file keeps its K exception table."""
import collections
import functools

import numpy as np
import torch

import conv_grad_ref as R
from conv_transpose_grad_ref import valid_masks

DEV = "cuda:0"


class Spec(collections.namedtuple("Spec", "transpose cin cout k p")):
    """a layer: Conv1d with dilation p (weight [cout, cin, k]) or, transpose, ConvTranspose1d with stride p ([cin, cout, k])"""

    @property
    def mul(self):  # rows of y per row of x
        return self.p if self.transpose else 1

    @property
    def op(self):
        return R.conv_transpose_op(self.p) if self.transpose else R.conv_op(self.p)

    def __str__(self):
        return f"{self.cin} -> {self.cout} k {self.k} {'s' if self.transpose else 'd'} {self.p}"


def case(spec, B, ld, seed, bias=True):
    rs = np.random.RandomState(seed)
    cin, cout, k = spec.cin, spec.cout, spec.k
    x = torch.from_numpy(rs.randn(B, cin, ld).astype(np.float32))
    x[torch.from_numpy(rs.rand(B, cin, ld) < 0.02)] = 0.0  # exact zeros: the x = 0 branch is the slope
    wshape = (cin, cout, k) if spec.transpose else (cout, cin, k)
    w = torch.from_numpy((rs.uniform(-1, 1, wshape) / np.sqrt(cin * k / spec.mul)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32)) if bias else None
    gy = torch.from_numpy(rs.randn(B, cout, spec.mul * ld).astype(np.float32))
    return x, w, b, gy


def run(layer, spec, x, w, b, gy, lengths, slope, add=None, need=(True, True, True)):
    """one forward + backward of ``layer`` (nn.conv1d or nn.conv_transpose1d, as spec says) on the device; returns
    [y, gx, gw, gb, the gradient of add], None where there is none"""
    xd = x.to(DEV).requires_grad_(need[0])
    wd = w.to(DEV).requires_grad_(need[1])
    bd = None if b is None else b.to(DEV).requires_grad_(need[2])
    ad = None if add is None else add.to(DEV).requires_grad_(True)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    kw = {"stride": spec.p} if spec.transpose else {"dilation": spec.p, "add": ad}
    y = layer(xd, wd, bd, lengths=ln, in_slope=slope, **kw)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    out = [y.detach().cpu()] + [None if t is None or t.grad is None else t.grad.cpu() for t in (xd, wd, bd)]
    return out + [None if ad is None else ad.grad.cpu()]


def gpu_run(nn, spec):
    return functools.partial(run, nn.conv_transpose1d if spec.transpose else nn.conv1d, spec)


def partials(nn, spec, B, ld):
    if spec.transpose:
        return nn.wgrad_partials_transpose(B, ld, spec.cin, spec.cout, spec.k, spec.p)
    return nn.wgrad_partials(B, ld, spec.cin, spec.cout, spec.k)


def lengths_for(nn, spec):
    """1, 2, (Conv1d: pad, pad + 1; transposed: 3,) chunk - 1, chunk, chunk + 1, 2 chunk + 1, and, where the plan has one inside an
    utterance, a length on either side of a partial boundary (placed in the utterance the boundary falls in)"""
    T, pad = nn.WGRAD_CHUNK, (spec.k - 1) * spec.p // 2
    lengths = ([1, 2, 3] if spec.transpose else [1, 2, pad, pad + 1]) + [T - 1, T, T + 1, 2 * T + 1, T, 2 * T + 1]
    B, ld = len(lengths), (2 * T + 1 + 3) // 4 * 4
    P, pairs = partials(nn, spec, B, ld)
    nch = -(-ld // T)
    inside = [divmod(p * pairs, nch) for p in range(1, P) if (p * pairs) % nch]
    if inside:
        b, c = inside[len(inside) // 2]
        lengths[-2], lengths[-1] = c * T, c * T + 1
        lengths[b], lengths[-1] = lengths[-1], lengths[b]  # this utterance's chunk c belongs to the next partial
    return lengths, ld, (P, pairs)


def _bars(tag, got, r64, r32, k_y, k_gx):
    y, gx, gw, gb = got[:4]
    bad = R.check(tag + " y", "act", y, r64[0], r32[0], *k_y)
    bad += R.check(tag + " gx", "act", gx, r64[1], r32[1], *k_gx)
    bad += R.check(tag + " gw", "weight", gw, r64[2], r32[2])
    return bad + R.check(tag + " gb", "vec", gb, r64[3], r32[3])


def assert_layer_gradients(run, spec, lengths, ld, seed, k_y=(R.K_WHOLE, R.K_CH), k_gx=(R.K_WHOLE, R.K_CH), slope=0.1):
    """run(x, w, b, gy, lengths, slope, add=None, need=(True, True, True)) -> [y, gx, gw, gb, gadd].  The four bars on a ragged
    batch (Conv1d: with a residual ``add``); nothing beyond the lengths; every gradient bit-reproducible; poison beyond the
    lengths changes nothing; the five needs_input_grad combinations keep the others' bits; every utterance alone has the
    batch's gx bits and its own gw / gb inside the bars."""
    B, mul, op = len(lengths), spec.mul, spec.op
    x, w, b, gy = case(spec, B, ld, seed)
    vi, vo = valid_masks(lengths, ld, mul)
    add = None if spec.transpose else torch.from_numpy(np.random.RandomState(1).randn(B, spec.cout, ld).astype(np.float32))
    run = functools.partial(run, lengths=lengths, slope=slope, add=add)
    y, gx, gw, gb, gadd = run(x, w, b, gy)
    r64 = list(R.layer_ref(x, w, b, gy, lengths, op, slope, torch.float64))
    r32 = list(R.layer_ref(x, w, b, gy, lengths, op, slope, torch.float32))
    if add is not None:
        r64[0], r32[0] = r64[0] + add.double() * vo.double(), r32[0] + add * vo
        assert torch.equal(gadd, gy), "the gradient of add is gy itself"
    bad = _bars("batch", (y, gx, gw, gb), r64, r32, k_y, k_gx)
    assert not gx[(vi == 0).expand_as(gx)].any() and not y[(vo == 0).expand_as(y)].any(), "written or propagated beyond the lengths"
    again = run(x, w, b, gy)
    assert torch.equal(again[1], gx) and torch.equal(again[2], gw) and torch.equal(again[3], gb), "not bit-reproducible"
    xp, gyp = x.clone(), gy.clone()
    xp[(vi == 0).expand_as(x)] = 1e30
    gyp[(vo == 0).expand_as(gy)] = 1e30
    for name, t, q in zip(("y", "gx", "gw", "gb"), (y, gx, gw, gb), run(xp, w, b, gyp)):
        assert torch.equal(q, t), f"poison beyond the lengths changes {name}"
    for need in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, True)):
        for name, t, q, on in zip(("gx", "gw", "gb"), (gx, gw, gb), run(x, w, b, gy, need=need)[1:4], need):
            assert (torch.equal(q, t) if on else q is None), f"needs_input_grad {need}: {name}"
    worst = {}
    for i, n in enumerate(lengths):
        if n <= 0:
            continue
        sl = slice(i, i + 1)
        yi, gxi, gwi, gbi, _ = run(x[sl], w, b, gy[sl], lengths=[n], add=None)
        assert torch.equal(gxi, gx[sl]), ("alone gx differs from the batch's", i, n)
        if spec.transpose:  # (the Conv1d's alone runs are made without add)
            assert torch.equal(yi, y[sl]), ("alone y differs from the batch's", i, n)
        a64 = R.layer_ref(x[sl], w, b, gy[sl], [n], op, slope, torch.float64)
        a32 = R.layer_ref(x[sl], w, b, gy[sl], [n], op, slope, torch.float32)
        for name, kind, t, j in (("gw", "weight", gwi, 2), ("gb", "vec", gbi, 3)):
            m = R.compare(kind, t, a64[j], a32[j])
            bad += R.check(f"alone len {n} {name}", kind, t, a64[j], a32[j], verbose=False)
            for what in ("ratio", "ch_ratio"):
                worst[(name, what)] = max(worst.get((name, what), 0.0), m[what])
    print("CG alone, worst over the lengths:", {f"{a}/{b}": round(v, 3) for (a, b), v in worst.items()})
    assert not bad, bad


def assert_training_shape(run, spec, L, k_y, k_gx, slope=0.1):
    """B = 32 at a length L of the generator's own (28 frames), four utterances shorter: the four bars, every gradient
    bit-reproducible"""
    B = 32
    lengths = [L] * B
    for i, n in zip((1, 5, 17, 31), (L // 2 + 1, 1, L - 1, max(1, L // 3))):
        lengths[i] = n
    x, w, b, gy = case(spec, B, L, seed=L + spec.k)
    y, gx, gw, gb, _ = run(x, w, b, gy, lengths, slope)
    r64 = R.layer_ref(x, w, b, gy, lengths, spec.op, slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, spec.op, slope, torch.float32)
    bad = _bars("train", (y, gx, gw, gb), r64, r32, k_y, k_gx)
    assert not bad, bad
    again = run(x, w, b, gy, lengths, slope)
    assert torch.equal(again[1], gx) and torch.equal(again[2], gw) and torch.equal(again[3], gb), "not bit-reproducible"
