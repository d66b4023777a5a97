"""What the tile-edge tests of the conv families share (tests/test_gpu_direct_conv_tiles.py, test_gpu_wino8_tiles.py,
test_gpu_wino_tiles.py, test_gpu_gen_split_bf16.py and the three test_*_plan_cpu.py files): the edge contract, once.
  options / lib          the option context manager that restores what it found, and the module fixture that builds the library;
  data and masks         make_x / make_case (NaN beyond every length), reference64, beyond_mask, edge_mask, edge_columns,
                         edge_lengths, check_edges (sentinel untouched beyond a length, nothing from beyond it inside), held;
  launches               run_conv (dissc_conv1d / dissc_conv1d_prec, ragged or uniform), walk_case, the ConvTranspose tables;
  sweep                  one batch of edge lengths through every tile setting of a Toom-Cook family (a Family below): same bits
                         in every setting, alone and uniform, and the float64 figures that assert_float64_bars holds to the bars;
  pair epilogues         pair_epilogues_every_setting, then check_pair_epilogues: dissc_respair1d's epilogues 1..4 at tile edges.
A family's own tables (tiles, option sets, shapes, bars) stay in its test file.  Nothing here touches the GPU at import; pytest
does not rewrite the asserts of this module, so each names its setting, instance and length itself.
`lib` is the dissc_amd._lib module throughout."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
SENTINEL = -7.0
SLOPE = 0.1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import _lib
    return _lib


@contextlib.contextmanager
def options(lib, restore=None, **kv):
    """sets options; on exit restores the values read at the start (dissc_get_option) -- or, where `restore` is given, sets
    exactly those {option: value} instead (tests/pair_harness.py: back to the shipped values whatever was in force)"""
    before = {k: lib.get_option(k) for k in kv} if restore is None else restore
    try:
        for k, v in kv.items():
            lib.set_option(k, v)
        yield
    finally:
        for k, v in before.items():
            lib.set_option(k, v)


# ---- data and masks -----------------------------------------------------------------------------------------------------
def edge_lengths(widths, pad, multiples=(1, 2), extra=()):
    """sorted: 0, 1, 2, pad, pad + 1, m W + e for every width (m in `multiples`; e = -1, 0, 1) and the lengths in `extra`"""
    return sorted({0, 1, 2, pad, pad + 1, *extra} | {m * w + e for w in widths for m in multiples for e in (-1, 0, 1)})


def make_x(rs, B, cin, ld, lengths):
    x = torch.from_numpy(rs.randn(B, cin, ld).astype(np.float32))
    x[torch.from_numpy(rs.rand(B, cin, ld) < 0.02)] = 0.0
    for i, n in enumerate(lengths):
        x[i, :, n:] = float("nan")  # never read
    return x


def make_case(C, k, lengths, seed, device=DEV):
    """x uniform in [-1, 1) with NaN beyond each length, weights and bias at the magnitudes of the Toom-Cook bars' own tests"""
    g = torch.Generator().manual_seed(seed)
    B, ld = len(lengths), (max(lengths) + 3) // 4 * 4
    x = torch.rand(B, C, ld, generator=g) * 2 - 1
    for i, n in enumerate(lengths):
        x[i, :, n:] = float("nan")  # never read
    w = (torch.rand(C, C, k, generator=g) * 2 - 1) * 0.025 * (256 / C) ** 0.5
    b = torch.rand(C, generator=g) * 0.2 - 0.1
    return x.to(device), w, b, ld


def reference64(x, w, b, lengths, k, d):
    """float64 F.conv1d on leaky_relu(x), every utterance on its own samples: zeros beyond a length are the "same" padding"""
    xz = torch.nan_to_num(x.double(), nan=0.0)
    return F.conv1d(F.leaky_relu(xz, SLOPE), w.double().to(x.device), b.double().to(x.device), padding=(k - 1) * d // 2, dilation=d)


def beyond_mask(lengths, ld, mul=1):
    m = torch.zeros(len(lengths), 1, ld, dtype=torch.bool)
    for i, n in enumerate(lengths):
        m[i, :, n * mul:] = True
    return m


def edge_mask(lengths, ld, unit, widths):
    """columns within one unit width of a boundary of the tiles of these widths or of the utterance's end"""
    c = torch.arange(ld)
    near = torch.zeros(ld, dtype=torch.bool)
    for w in widths:
        near |= (c % w < unit) | (c % w >= w - unit)
    m = torch.zeros(len(lengths), 1, ld, dtype=torch.bool)
    for i, n in enumerate(lengths):
        m[i, 0, :n] = near[:n] | (c[:n] >= n - unit)
    return m


def edge_columns(n, widths, reach, mul=1):
    """the columns of [0, n * mul) within `reach` (* mul) of an utterance end or of a boundary of a tile of one of the widths"""
    t = torch.arange(n * mul)
    m = (t < reach * mul) | (t >= (n - reach) * mul)
    for w in widths:
        for e in range(w, n + reach, w):
            m |= (t >= (e - reach) * mul) & (t < (e + reach) * mul)
    return m


def check_edges(y, beyond, what):
    """nothing written beyond an utterance (the sentinel is still there), nothing from beyond it inside (the input is NaN there)"""
    b = beyond.expand_as(y)
    assert (torch.where(b, y, torch.full_like(y, SENTINEL)) == SENTINEL).all(), ("wrote beyond an utterance", what)
    assert torch.isfinite(torch.where(b, torch.zeros_like(y), y)).all(), ("a sample from beyond an utterance's length reached its output", what)


def held(y, beyond):
    """the output with the sentinel columns beyond each utterance (asserted untouched) as zeros, on the CPU"""
    yb = torch.where(beyond.expand_as(y), y, torch.full_like(y, SENTINEL))
    assert (yb == SENTINEL).all(), "wrote beyond an utterance"
    return torch.where(beyond.expand_as(y), torch.zeros_like(y), y).cpu()


# ---- launches -----------------------------------------------------------------------------------------------------------
def run_conv(lib, x, w, b, lengths, k, d, slope, Lmax=None, prec=None):
    """dissc_conv1d (prec given: dissc_conv1d_prec) on device x [B, Cin, ld] (ld a multiple of 4) into an output prefilled with
    the sentinel.  lengths None or an int: the uniform call, lengths = NULL, every row that long (None: Lmax columns)"""
    B, cin, ld = x.shape
    cout = w.shape[0]
    assert ld % 4 == 0, ("the row stride must be a multiple of 4", ld)
    y = torch.full((B, cout, ld), SENTINEL, device=x.device)
    if lengths is None or isinstance(lengths, int):
        ln, Lmax = None, Lmax if lengths is None else lengths
    else:
        ln = torch.as_tensor(lengths, dtype=torch.int32, device=x.device)
        Lmax = int(max(lengths)) if Lmax is None else Lmax
    head = (x.data_ptr(), w.contiguous().data_ptr(), b.contiguous().data_ptr(), y.data_ptr(), None if ln is None else ln.data_ptr(),
            B, cin, cout, k, d, ld, ld, Lmax, ctypes.c_float(slope))
    if prec is None:
        lib.check(lib.lib.dissc_conv1d(*head, None), "dissc_conv1d")
    else:
        lib.check(lib.lib.dissc_conv1d_prec(*head, prec, None), "dissc_conv1d_prec")
    return y


def ragged_lengths(B, seed):
    rs = np.random.RandomState(seed)
    lengths = rs.randint(0, 301, B)
    lengths[[3, 64, B - 1]] = 0
    lengths[[0, 1, 63, 65, B - 2]] = [300, 77, 129, 1, 257]
    return [int(n) for n in lengths]


def walk_case(lib, shape, B, opts_list, alone):
    """B > 64 ragged utterances (empty ones at the round boundary of the prefix sum, index 64, and elsewhere) under every option
    set of opts_list bit for bit, the rows `alone` = those rows of the batch, the first two of them against float64"""
    cin, cout, k, d, slope = shape
    lengths = ragged_lengths(B, seed=B)
    ld = 300
    rs = np.random.RandomState(B + cin)
    x = make_x(rs, B, cin, ld, lengths).to(DEV)
    w = torch.from_numpy((rs.uniform(-1, 1, (cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, cout).astype(np.float32))
    beyond = beyond_mask(lengths, ld).to(DEV)
    first = None
    for opts in opts_list:
        with options(lib, **opts):
            y = run_conv(lib, x, w, b, lengths, k, d, slope)
        check_edges(y, beyond, opts)
        first = y if first is None else first
        assert torch.equal(y, first), ("differs from the first option set", opts)
    for i in alone:
        n = lengths[i]
        assert n > 0, (i, n)
        one = run_conv(lib, x[i:i + 1].clone(), w, b, [n], k, d, slope)
        assert torch.equal(one[0, :, :n], first[i, :, :n]), ("alone", i, n)
    # against torch on a few rows (the bits above carry it to the rest)
    for i in alone[:2]:
        n = lengths[i]
        ref = F.conv1d(F.leaky_relu(x[i:i + 1, :, :n].cpu().double(), slope), w.double(), b.double(), padding=(k - 1) * d // 2, dilation=d)
        err = float((first[i, :, :n].cpu().double() - ref[0]).abs().max())
        assert err <= 2e-5, ("against float64", i, n, err)


# ConvTranspose (Cin, Cout, k, stride), and where the paired float2 store of conv_epilogue32 runs (np, stride, p0 and the GEMM
# rows of every group all even)
UPS = [(512, 256, 11, 5), (256, 128, 8, 4), (128, 64, 8, 4), (64, 32, 4, 2), (32, 16, 4, 2), (96, 80, 9, 3)]
PAIRED = {(512, 256, 11, 5): False, (256, 128, 8, 4): True, (128, 64, 8, 4): True, (64, 32, 4, 2): True, (32, 16, 4, 2): True,
          (96, 80, 9, 3): False}


def paired_store(g, s):
    return g["np"] % 2 == 0 and s % 2 == 0 and g["p0"] % 2 == 0 and g["rows"] % 2 == 0


# ---- the sweep of a Toom-Cook family ------------------------------------------------------------------------------------
class Family:
    """One Toom-Cook conv family, as sweep needs it.  `form` is whatever tells the family's forms apart (the eight-point kernel:
    R = 3 / 4; F(4,3) has the one form None); an instance is the tuple the family's info entry identifies a kernel by.
      name                                              for messages
      forms(k)                                          the forms a kernel size runs in
      conv(form), direct                                the options that put dissc_conv1d on that form / on the direct kernel
      plan(lib, C, k, d, form, B, Lmax)                 (instance, plan dict) in force under the current options; asserts that the
                                                        plan can be launched
      shape_widths(lib, C, k, d, form)                  (unit width, {tile widths})
      tile_settings(lib, C, k, d, form, B, nb, Lmax)    [(options, rows, instance)]: the leading sub-batches and options that
                                                        reach every instance, a full batch first (nb: rows before repetition)
      alone_at_256(unit, w1, Lmax)                      the lengths that run alone at C >= 256 (w1: the narrowest tile)
      lmax_cap                                          the longest row the sweep may ask for"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def rows_for(lib, fam, C, k, d, rows):
    """the list of rows repeated until the full batch reaches the top tier ("small_grid" = 0) by the ladder itself, in every form"""
    Lmax = max(rows)
    for reps in (1, 2, 3, 4):
        ok = True
        for form in fam.forms(k):
            with options(lib, small_grid=0):
                top = fam.plan(lib, C, k, d, form, reps * len(rows), Lmax)[0]
            ok = ok and fam.plan(lib, C, k, d, form, reps * len(rows), Lmax)[0] == top
        if ok:
            return rows * reps
    raise AssertionError(("the ladder's top tier is out of reach", fam.name, C, k, d))


@functools.lru_cache(maxsize=None)
def sweep(lib, fam, C, k, d):
    """One batch per (C, k, d), shared by every form and tile: the edge lengths of every tile width any form has, longest first.
    Per form: the batch through every tile setting, every utterance alone (C >= 256: a subset at the edge lengths -- its
    instances are those of C = 128, where every row runs alone, and a call packs the weights on the host), two uniform calls; all
    bit-identical on an utterance's columns, the sentinel untouched beyond.  Returns dict(lengths, B, ran: the instances that ran,
    geo: {form: (unit, sorted widths)}, fig: {form: error figures against float64}); the figures are not asserted here."""
    forms = fam.forms(k)
    pad = (k - 1) * d // 2
    geo = {f: fam.shape_widths(lib, C, k, d, f) for f in forms}
    widths = set().union(*(ws for _, ws in geo.values()))
    base = set(edge_lengths(widths, pad, extra={u + e for u, _ in geo.values() for e in (-1, 1)}))
    # the longest first (Lmax is that of every leading sub-batch), then the edges of each form's narrowest tile: the rows the
    # small-grid tiers, which take the fewest rows, see in a batch
    narrow = {m * min(ws) + e for _, ws in geo.values() for m in (1, 2) for e in (-1, 0, 1)}
    base = [max(base)] + sorted(base - {max(base)}, key=lambda n: (n not in narrow, n))
    lengths = rows_for(lib, fam, C, k, d, base)
    nb, B, Lmax = len(base), len(lengths), max(lengths)
    assert lengths[0] == Lmax == 2 * max(widths) + 1 and Lmax <= fam.lmax_cap, (fam.name, C, k, d, lengths[0], Lmax)
    x, w, b, ld = make_case(C, k, base, seed=1000 * C + 10 * k + d)
    x = x.repeat(B // nb, 1, 1)  # (repeated rows carry the same data)
    beyond = beyond_mask(lengths, ld).to(DEV)
    valid = ~beyond.expand(B, C, ld)
    r64 = reference64(x, w, b, lengths, k, d)

    def errors(y, mask):
        e = torch.where(mask, y.double() - r64, torch.zeros_like(r64))
        return float(e.abs().max()), float((e.pow(2).sum() / mask.sum()).sqrt())

    with options(lib, **fam.direct):
        yd = run_conv(lib, x, w, b, lengths, k, d, SLOPE)
    check_edges(yd, beyond, (fam.name, "direct"))
    res = dict(lengths=base, B=B, ran=set(), geo={f: (u, sorted(ws)) for f, (u, ws) in geo.items()}, fig={})
    for form in forms:
        unit, ws = geo[form]
        first = first_inst = None
        for opts, rows, inst in fam.tile_settings(lib, C, k, d, form, B, nb, Lmax):
            with options(lib, **fam.conv(form), **opts):
                got = fam.plan(lib, C, k, d, form, rows, Lmax)[0]
                assert got == inst, (fam.name, form, opts, rows, "the plan moved", got, inst)
                y = run_conv(lib, x[:rows], w, b, lengths[:rows], k, d, SLOPE)
            check_edges(y, beyond[:rows], (fam.name, form, opts, rows, inst))
            if first is None:
                assert rows == B, (fam.name, form, "the first setting is not a full batch", rows, B)
                first, first_inst = y, inst
            assert torch.equal(y, first[:rows]), f"{fam.name} form {form}: instance {inst} ({opts}, {rows} rows) differs from instance {first_inst}"
            res["ran"].add(inst)
        for i in range(nb, B):  # a repeated row = its original
            assert torch.equal(first[i], first[i % nb]), (fam.name, form, "a repeated row differs from its original", i, lengths[i])
        assert not torch.equal(first, yd), (fam.name, form, "the direct kernel ran")
        w1 = min(ws)
        alone = range(nb) if C < 256 else [i for i, n in enumerate(base) if n in fam.alone_at_256(unit, w1, Lmax)]
        with options(lib, **fam.conv(form)):
            for i in alone:
                n = lengths[i]
                if n == 0:
                    continue
                res["ran"].add(fam.plan(lib, C, k, d, form, 1, n)[0])
                one = run_conv(lib, x[i:i + 1].clone(), w, b, [n], k, d, SLOPE)
                check_edges(one, beyond[i:i + 1], (fam.name, form, "alone", n))
                assert torch.equal(one[0, :, :n], first[i, :, :n]), (fam.name, form, "alone", n)
            for n in (min(ws) + 1, 2 * max(ws) - 1):  # uniform: two rows of that length, lengths = NULL
                i = lengths.index(n)
                res["ran"].add(fam.plan(lib, C, k, d, form, 2, n)[0])
                two = run_conv(lib, x[i:i + 1].expand(2, C, ld).contiguous(), w, b, n, k, d, SLOPE)
                check_edges(two, beyond[i:i + 1].expand(2, 1, ld), (fam.name, form, "uniform", n))
                assert torch.equal(two[0, :, :n], first[i, :, :n]) and torch.equal(two[1], two[0]), (fam.name, form, "uniform", n)
        fig = dict(all=errors(first, valid), direct=errors(yd, valid), edge=[])
        for wd in sorted(ws):  # per tile width (the narrowest tiles of d = 3 / 5 are one or two units wide, all of them edge)
            edge = edge_mask(lengths, ld, unit, [wd]).to(DEV).expand(B, C, ld) & valid
            assert 0 < int(edge.sum()) <= int(valid.sum()), (fam.name, form, "no edge columns", wd)
            fig["edge"].append((wd, float(edge.sum()) / float(valid.sum()), errors(first, edge), errors(yd, edge)))
        res["fig"][form] = fig
    return res


def figures_line(f):
    """the figures of one form as the tests print them"""
    (mx, rms), (dmx, drms) = f["all"], f["direct"]
    return (f"max {mx:.2e} rms {rms:.2e} (direct {dmx:.2e} / {drms:.2e}, ratio {rms / drms:.2f}); edge columns of "
            + ", ".join(f"w {wd} ({100 * sh:.0f} %): max {e[0]:.2e} rms {e[1]:.2e} ratio {e[1] / de[1]:.2f}" for wd, sh, e, de in f["edge"]))


def float64_bars(fig, max_err, k_rms, k_edge, rms_floor, edge_max=None):
    """a form's figures from sweep against the bars: per element max_err (the direct kernel's too), rms at most k_rms x the direct
    kernel's + rms_floor; over the edge columns of every tile width rms at most k_edge x the direct kernel's there + rms_floor
    and, where edge_max is given, that per element.  Returns the broken bars with their figures."""
    (mx, rms), (dmx, drms) = fig["all"], fig["direct"]
    bad = []
    if not (mx <= max_err and dmx <= max_err):
        bad.append(("max", mx, dmx))
    if not rms <= k_rms * drms + rms_floor:
        bad.append(("rms", rms, drms))
    for wd, _, (emx, erms), (_, derms) in fig["edge"]:
        if not ((edge_max is None or emx <= edge_max) and erms <= k_edge * derms + rms_floor):
            bad.append(("edge", wd, emx, erms, derms))
    return bad


def assert_float64_bars(figs, max_err, k_rms, k_edge, rms_floor, edge_max=None, what=""):
    """float64_bars over {form: figures} (sweep's "fig"): every form is measured before the test fails, and the message names
    `what`, the form and each broken bar"""
    bad = [(form,) + b for form, fig in figs.items() for b in float64_bars(fig, max_err, k_rms, k_edge, rms_floor, edge_max)]
    assert not bad, (what, bad)


# ---- the residual / MRF epilogues of a pair -----------------------------------------------------------------------------
def pair_epilogues_every_setting(lib, mode, pair, lengths, k, d, acc0, beyond, settings, inspect=None):
    """dissc_respair1d in `mode` on pair = (x, w1, b1, w2, b2) with epilogue 1..4 (2..4 on a copy of acc0) under every option set
    of `settings`: output and accumulator untouched beyond each length (`beyond`: [B, C, ld] on the device), nothing from beyond it
    inside, the same bits under every set.  inspect(options) runs under each set before its launches (to ask the info entry what
    runs); what it returns goes into the messages.  Returns {epilogue: output} of the first set."""
    import pair_harness as ph  # (it imports this module)
    first = {}
    for opts in settings:
        with options(lib, **opts):
            what = inspect(opts) if inspect else None
            outs = {epi: ph.run_pair(lib, mode, *pair, lengths, k, d, epi=epi, acc=None if epi == 1 else acc0) for epi in (1, 2, 3, 4)}
        for epi, o in outs.items():
            untouched = torch.full_like(o, SENTINEL) if epi == 1 else acc0
            assert torch.equal(torch.where(beyond, o, untouched), untouched), (opts, what, epi, "wrote beyond an utterance")
            assert torch.isfinite(torch.where(beyond, torch.zeros_like(o), o)).all(), (opts, what, epi, "read beyond an utterance")
            first.setdefault(epi, o)
            assert torch.equal(o, first[epi]), (opts, what, epi, "differs from the first setting")
    return first


def check_pair_epilogues(first, pair, lengths, k, d, acc0, beyond, head, y0=None):
    """first = pair_epilogues_every_setting(...): epilogue 1 against pair_harness.reference (float64 per utterance): finite, max
    error 1e-5 and, where y0 -- the output of the two direct launches, mode 0 -- is given, not its bits and rms at most
    max(3 x its rms, 1e-6); the MRF epilogues bit for bit: 2 stores the pair's output, 3 adds it to acc0, 4 divides that sum by
    3 (a true division, on the CPU like the reference's xs / num_kernels: torch's GPU kernel for a scalar divisor multiplies by
    the reciprocal).  Prints `head` and the figures before it asserts them."""
    import pair_harness as ph
    ref = ph.reference(*pair, lengths, k, d)
    y = first[1]
    for i, n in enumerate(lengths):
        assert torch.isfinite(y[i, :, :n]).all(), (head, "not finite", "utterance", i, "length", n)
    e = torch.where(beyond, torch.zeros_like(ref), y.double() - ref)
    worst = float(e.abs().max())
    if y0 is None:
        print(f"\n{head}max err {worst:.2e}, lengths {lengths}")
    else:
        e0 = torch.where(beyond, torch.zeros_like(ref), y0.double() - ref)
        rms, rms0 = float(e.pow(2).mean().sqrt()), float(e0.pow(2).mean().sqrt())
        print(f"\n{head}max err {worst:.2e}, rms {rms:.2e} (direct launches {rms0:.2e}), lengths {lengths}")
        assert not torch.equal(y, y0), (head, "the direct launches ran")
        assert rms <= max(3.0 * rms0, 1e-6), (head, "rms", rms, rms0)
    assert worst <= 1e-5, (head, "max err", worst)
    for i, n in enumerate(lengths):
        for epi in (2, 3, 4):
            want = y[i, :, :n] if epi == 2 else acc0[i, :, :n] + y[i, :, :n]
            if epi == 4:
                want = (want.cpu() / 3.0).to(want.device)
            assert torch.equal(first[epi][i, :, :n], want), (head, "epilogue", epi, "utterance", i, "length", n)
