"""What the tests of the four differentiable conv layers (dissc_amd.nn.conv1d, conv_transpose1d, conv1d_strided, conv1d_grouped)
share (not a test module): the layer spec and everything that hangs on its kind, seeded data, one forward + backward through the
layer, the ragged lengths around the chunk and a partial boundary, the rule that admits a K exception, the two check bodies, the
packing read-back and the discriminators' loss.  The bodies take ``run`` as a parameter -- on the GPU a partial of run() below,
in tests/test_conv_grad_cpu.py a CPU stand-in with seeded defects -- and the bars of the forward and the data gradient from the
caller, whose file keeps its K exception table."""
import collections
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv_grad_ref as R

DEV = "cuda:0"
NAMES = ("y", "gx", "gw", "gb")


class Spec(collections.namedtuple("Spec", "kind cin cout k p groups")):
    """a layer by its kind: "conv1d" (p = dilation, weight [cout, cin, k]), "transposed" (ConvTranspose1d, p = stride,
    [cin, cout, k]), "strided" and "grouped" (Conv1d at p = stride in ``groups``, [cout, cin / groups, k])"""

    def __new__(cls, kind, cin, cout, k, p, groups=1):
        assert kind in ("conv1d", "transposed", "strided", "grouped") and (groups == 1 or kind == "grouped")
        return super().__new__(cls, kind, cin, cout, k, p, groups)

    @property
    def divides(self):  # the stride divides the length
        return self.kind in ("strided", "grouped")

    @property
    def down(self):
        return self.p if self.divides else 1

    @property
    def wshape(self):
        return (self.cin, self.cout, self.k) if self.kind == "transposed" else (self.cout, self.cin // self.groups, self.k)

    @property
    def fan_in(self):  # of the weight scale
        return self.cin // self.groups * self.k / (self.p if self.kind == "transposed" else 1)

    @property
    def op(self):
        return {"conv1d": R.conv_op, "transposed": R.conv_transpose_op}.get(self.kind, R.strided_op)(self.p, *self._g)

    @property
    def _g(self):
        return (self.groups,) if self.kind == "grouped" else ()

    def layer(self, nn):
        """(the nn layer function, its keyword arguments)"""
        return {"conv1d": (nn.conv1d, {"dilation": self.p}), "transposed": (nn.conv_transpose1d, {"stride": self.p}),
                "strided": (nn.conv1d_strided, {"stride": self.p}),
                "grouped": (nn.conv1d_grouped, {"stride": self.p, "groups": self.groups})}[self.kind]

    def partials(self, nn, B, ld):
        """(P, pairs): the weight gradient's plan"""
        if self.kind == "conv1d":
            return nn.wgrad_partials(B, ld, self.cin, self.cout, self.k)
        query = {"transposed": nn.wgrad_partials_transpose, "strided": nn.wgrad_partials_strided, "grouped": nn.wgrad_partials_grouped}
        return query[self.kind](B, ld, self.cin, self.cout, self.k, self.p, *self._g)

    def chunk(self, nn):  # the weight gradient's chunk, in input positions
        return nn.WGRAD_CHUNK * self.down

    @property
    def short(self):  # the kind's own short lengths: the padding; the stride; the halo and the kernel of k = 41
        pad, s = (self.k - 1) * self.p // 2, self.p
        return {"conv1d": [pad, pad + 1], "transposed": [3], "strided": [s, s + 1], "grouped": [s, s + 1, 20, 21, 41]}[self.kind]

    def chain(self, tensor):
        """the products in one output's sum: of y, or of gx"""
        up, down = (self.p if self.kind == "transposed" else 1), self.down
        return self.cin // self.groups * R.cdiv(self.k, up) if tensor == "y" else self.cout // self.groups * R.cdiv(self.k, down)

    def __str__(self):
        return f"{self.cin} -> {self.cout} k {self.k} {'d' if self.kind == 'conv1d' else 's'} {self.p}" + "".join(f" g {g}" for g in self._g)


def case(spec, B, ld, seed, bias=True):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.randn(B, spec.cin, ld).astype(np.float32))
    x[torch.from_numpy(rs.rand(B, spec.cin, ld) < 0.02)] = 0.0  # exact zeros: the x = 0 branch is the slope
    w = torch.from_numpy((rs.uniform(-1, 1, spec.wshape) / np.sqrt(spec.fan_in)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, spec.cout).astype(np.float32)) if bias else None
    gy = torch.from_numpy(rs.randn(B, spec.cout, R.y_ld(ld, spec.op)).astype(np.float32))
    return x, w, b, gy


def run(nn, spec, x, w, b, gy, lengths, slope, add=None, need=(True, True, True), nan_workspace=False):
    """one forward + backward of spec's layer on the device, with nan_workspace behind a workspace whose every float is a NaN;
    returns [y, gx, gw, gb, the gradient of add], None where there is none"""
    xd = x.to(DEV).requires_grad_(need[0])
    wd = w.to(DEV).requires_grad_(need[1])
    bd = None if b is None else b.to(DEV).requires_grad_(need[2])
    ad = None if add is None else add.to(DEV).requires_grad_(True)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    layer, kw = spec.layer(nn)
    y = layer(xd, wd, bd, lengths=ln, in_slope=slope, **kw, **({} if ad is None else {"add": ad}))
    if nan_workspace:
        for ws in nn._workspaces.values():
            ws.fill_(255)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    out = [y.detach().cpu()] + [None if t is None or t.grad is None else t.grad.cpu() for t in (xd, wd, bd)]
    return out + [None if ad is None else ad.grad.cpu()]


def gpu_run(nn, spec):
    return functools.partial(run, nn, spec)


def lengths_for(nn, spec, max_b=None):
    """INPUT lengths with T one chunk of the weight gradient: 1, 2, the kind's short ones, T - 1, T, T + 1, 2 T + 1, where a stride
    s divides the length one of each residue mod s next to 2 T, and, where the plan has one inside an utterance, a length on
    either side of a partial boundary (placed in the utterance the boundary falls in).  max_b = 4 (the widest layers): s + 1,
    2 T - 1 and the last two of the list."""
    T, s = spec.chunk(nn), spec.down
    residues = [2 * T - r for r in range(s)] if spec.divides else []
    lengths = [1, 2] + spec.short + [T - 1, T, T + 1, 2 * T + 1] + residues + [T, 2 * T + 1]
    if max_b is not None:
        assert max_b == 4
        lengths = [s + 1, 2 * T - 1, T, 2 * T + 1]
    B, ld = len(lengths), R.ceil4(2 * T + 1)
    P, pairs = spec.partials(nn, B, ld)
    nch = R.cdiv(ld, T)
    inside = [divmod(p * pairs, nch) for p in range(1, P) if (p * pairs) % nch]
    if inside:
        b, c = inside[len(inside) // 2]
        lengths[-2], lengths[-1] = c * T, c * T + 1  # c chunks exactly, and one position more
        lengths[b], lengths[-1] = lengths[-1], lengths[b]  # this utterance's chunk c belongs to the next partial
    return lengths, ld, (P, pairs)


def k_bars(exceptions, tensor, spec):
    """(whole, worst channel) for ``tensor`` of spec's layer: K = 4 unless ``exceptions`` has an entry, under (tensor, cin, cout,
    k, p[, groups]) or under the chain length n.  The rule every entry must meet (tests/train_stage_cases.py): only y or gx, only
    where the chain of one output has n >= 1 024 products, never above k_cap(n)."""
    n = spec.chain(tensor)
    kw, kc = exceptions.get((tensor,) + spec[1:5] + spec._g, exceptions.get(n, (R.K_WHOLE, R.K_CH)))
    assert tensor in ("y", "gx") and (max(kw, kc) <= 4 or (n >= 1024 and max(kw, kc) <= R.k_cap(n)))
    return kw, kc


def _bars(tag, got, r64, r32, k_y, k_gx):
    bad = R.check(tag + " y", "act", got[0], r64[0], r32[0], *k_y)
    bad += R.check(tag + " gx", "act", got[1], r64[1], r32[1], *k_gx)
    bad += R.check(tag + " gw", "weight", got[2], r64[2], r32[2])
    return bad + R.check(tag + " gb", "vec", got[3], r64[3], r32[3])


def _same_bits(got, want, what):
    for name, t, q in zip(NAMES, want, got):
        assert torch.equal(q, t), what.format(name)


def assert_layer_gradients(run, spec, lengths, ld, seed, k_y=(R.K_WHOLE, R.K_CH), k_gx=(R.K_WHOLE, R.K_CH), slope=0.1):
    """run(x, w, b, gy, lengths, slope, add=None, need=(True, True, True), nan_workspace=False) -> [y, gx, gw, gb, gadd].  The
    four bars on a ragged batch (Conv1d: with a residual ``add``); nothing beyond the lengths; every result bit-reproducible,
    also behind a workspace full of NaNs; poison beyond the lengths changes nothing; the five needs_input_grad combinations keep
    the others' bits; every utterance alone has the batch's y (but Conv1d, whose alone runs are made without add) and gx bits
    and its own gw / gb inside the bars."""
    B, op = len(lengths), spec.op
    x, w, b, gy = case(spec, B, ld, seed)
    vi, vo = R.valid_masks(lengths, ld, op)
    add = torch.from_numpy(np.random.RandomState(1).randn(B, spec.cout, ld).astype(np.float32)) if spec.kind == "conv1d" else None
    run = functools.partial(run, lengths=lengths, slope=slope, add=add)
    y, gx, gw, gb, gadd = got = run(x, w, b, gy)
    r64 = list(R.layer_ref(x, w, b, gy, lengths, op, slope, torch.float64))
    r32 = list(R.layer_ref(x, w, b, gy, lengths, op, slope, torch.float32))
    if add is not None:
        r64[0], r32[0] = r64[0] + add.double() * vo.double(), r32[0] + add * vo
        assert torch.equal(gadd, gy), "the gradient of add is gy itself"
    bad = _bars("batch", got, r64, r32, k_y, k_gx)
    assert not gx[(vi == 0).expand_as(gx)].any() and not y[(vo == 0).expand_as(y)].any(), "written or propagated beyond the lengths"
    _same_bits(run(x, w, b, gy), got, "{} is not bit-reproducible")
    _same_bits(run(x, w, b, gy, nan_workspace=True), got, "a workspace full of NaNs changes {}")
    xp, gyp = x.clone(), gy.clone()
    xp[(vi == 0).expand_as(x)] = 1e30
    gyp[(vo == 0).expand_as(gy)] = 1e30
    _same_bits(run(xp, w, b, gyp), got, "poison beyond the lengths changes {}")
    for need in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, True)):
        for name, t, q, on in zip(NAMES[1:], (gx, gw, gb), run(x, w, b, gy, need=need)[1:4], need):
            assert (torch.equal(q, t) if on else q is None), f"needs_input_grad {need}: {name}"
    worst = {}
    for i, n in enumerate(lengths):
        if n <= 0:
            continue
        sl = slice(i, i + 1)
        yi, gxi, gwi, gbi, _ = run(x[sl], w, b, gy[sl], lengths=[n], add=None)
        assert torch.equal(gxi, gx[sl]), ("alone gx differs from the batch's", i, n)
        assert add is not None or torch.equal(yi, y[sl]), ("alone y differs from the batch's", i, n)
        a64 = R.layer_ref(x[sl], w, b, gy[sl], [n], op, slope, torch.float64)
        a32 = R.layer_ref(x[sl], w, b, gy[sl], [n], op, slope, torch.float32)
        for name, kind, t, j in (("gw", "weight", gwi, 2), ("gb", "vec", gbi, 3)):
            m = R.compare(kind, t, a64[j], a32[j])
            bad += R.check(f"alone len {n} {name}", kind, t, a64[j], a32[j], verbose=False)
            for what in ("ratio", "ch_ratio"):
                worst[(name, what)] = max(worst.get((name, what), 0.0), m[what])
    print("CG alone, worst over the lengths:", {f"{a}/{b}": round(v, 3) for (a, b), v in worst.items()})
    assert not bad, bad


def training_lengths(B, L, short):
    """B rows of L, the rows ``short`` at L / 2 + 1, 1, L - 1, L / 3 in turn"""
    lengths = [L] * B
    for i, n in zip(short, (L // 2 + 1, 1, L - 1, max(1, L // 3))):
        lengths[i] = n
    return lengths


def assert_training_shape(run, spec, lengths, ld, seed, k_y, k_gx, slope=0.1):
    """the layer at one of the trainer's own row lengths, some rows shorter: the four bars, every result bit-reproducible"""
    x, w, b, gy = case(spec, len(lengths), ld, seed)
    got = run(x, w, b, gy, lengths, slope)
    r64 = R.layer_ref(x, w, b, gy, lengths, spec.op, slope, torch.float64)
    r32 = R.layer_ref(x, w, b, gy, lengths, spec.op, slope, torch.float32)
    bad = _bars("train", got, r64, r32, k_y, k_gx)
    _same_bits(run(x, w, b, gy, lengths, slope), got, "{} is not bit-reproducible")
    assert not bad, bad


def assert_device_packing(nn, spec, host_packing):
    """the two device-side packings of a strided or grouped spec's weight, read back through dissc_conv?grad_packed, bit for bit
    against host_packing(w, which)"""
    from dissc_amd import _lib
    kind = {"strided": nn.CONV1D_STRIDED, "grouped": nn.CONV1D_GROUPED}[spec.kind]
    packed = getattr(_lib.lib, kind.prefix + "_packed")
    packed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    packed.restype = ctypes.c_longlong
    w = case(spec, 1, 16, seed=spec.cin + spec.k)[1]
    h = nn._handle(kind, spec.cin, spec.cout, spec.k, spec.p, torch.device(DEV), spec.groups)
    wd = w.to(DEV)
    _lib.check(kind.set_weights(h, wd.data_ptr(), None, None), kind.names["set_weights"])
    for which in (0, 1):
        host = host_packing(w, which)
        n = packed(h, which, None, None)
        assert n == host.size
        dst = torch.full((n,), float("nan"), device=DEV)
        assert packed(h, which, dst.data_ptr(), None) == n
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy().view(np.uint32), host.reshape(-1).view(np.uint32))


def disc_loss(maps, hats, mask):
    """mean((1 - score)^2) over the valid scores + 2 sum_l mean |lrelu(f_l) - lrelu(fhat_l)| (the score map, the last one, as it
    is), torch ops"""
    last = len(maps) - 1
    loss = (((1 - maps[last]) ** 2) * mask[last]).sum() / mask[last].sum()
    for j, (f, fh) in enumerate(zip(maps, hats)):
        a, c = (f, fh) if j == last else (F.leaky_relu(f, R.SLOPE), F.leaky_relu(fh, R.SLOPE))
        loss = loss + 2 * (a - c).abs().sum() / (mask[j].sum() * f.shape[1])
    return loss
