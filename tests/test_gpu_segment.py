"""The segment gather on the GPU (csrc/segment_gather.hip through dissc_amd.gan_train.SegmentSampler): bit for bit against the
literal restatement of CodeDataset.__getitem__ in tests/segment_ref.py -- (hop 4, segment 20) at every legal start of utterances
of 1, F - 1, F, F + 1 and 3 F frames, (hop 320, segment 8 960) once, U = 1 and B = 1 --, nothing written outside the four outputs,
refusals with the error code and no launch, the sampler's batches and draws."""
import random

import numpy as np
import pytest
import torch

import segment_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -777.0


@pytest.fixture(scope="module")
def gt():
    import __graft_entry__ as ge
    ge.build()
    from dissc_amd import gan_train
    return gan_train


def config(hop, segment, batch_size=2):
    return dict(code_hop_size=hop, segment_size=segment, batch_size=batch_size)


def expect(raw, table, segment, hop):
    rows = [SR.getitem_crop(*raw[u][:3], segment, hop, s) for u, s in table]
    return (np.stack([r[0] for r in rows])[:, None, :], np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])[:, None, :],
            np.array([[raw[u][3]] for u, _ in table], np.int64))


def same(out, ref):
    for key, r in zip(("y", "code", "f0", "spkr"), ref):
        o = out[key].cpu().numpy()
        assert o.dtype == r.dtype and o.shape == r.shape and np.array_equal(o.view(np.int32), np.ascontiguousarray(r).view(np.int32)), key


def poisoned_out(B, segment, F):
    """the four outputs as views in the middle of poisoned buffers -> (out, check of the neighbours)"""
    pad = 64
    bufs = [torch.full((n + 2 * pad,), POISON if dt == torch.float32 else int(POISON), dtype=dt, device=DEV)
            for n, dt in ((B * segment, torch.float32), (B * F, torch.int64), (B * F, torch.float32), (B, torch.int64))]
    shapes = [(B, 1, segment), (B, F), (B, 1, F), (B, 1)]
    out = tuple(b[pad:b.numel() - pad].view(s) for b, s in zip(bufs, shapes))

    def untouched(inside_too=False):
        for b in bufs:
            edge = torch.cat([b[:pad], b[-pad:]]) if not inside_too else b
            assert bool((edge == b.new_tensor(POISON)).all())
    return out, untouched


def test_small_corpus_at_every_legal_start(gt):
    hop, segment = 4, 20
    raw = SR.raw_corpus(hop, 5, seed=1)
    s = gt.SegmentSampler(config(hop, segment), SR.prepared(raw, hop), device=DEV)
    table = []
    for u, r in enumerate(raw):
        end = SR.getitem_crop(*r[:3], segment, hop)[3]
        assert s.interval_end(u) == end
        table += [(u, k) for k in range(end + 1)]
    assert len(table) <= gt.SEGMENT_MAX_BATCH and table[0] == (0, 0) and table[-1][0] == len(raw) - 1
    out, untouched = poisoned_out(len(table), segment, 5)
    same(s.gather(table, out=out), expect(raw, table, segment, hop))
    untouched()
    same(s.gather(table[::-1]), expect(raw, table[::-1], segment, hop))  # rows in any order, an utterance many times


def test_real_segment_once(gt):
    hop, segment = 320, 8960
    raw = SR.raw_corpus(hop, 28, seed=2)
    s = gt.SegmentSampler(config(hop, segment), SR.prepared(raw, hop), device=DEV)
    ends = [SR.getitem_crop(*r[:3], segment, hop)[3] for r in raw]
    table = [(u, k) for u, e in enumerate(ends) for k in sorted({0, e // 2, e})]
    out, untouched = poisoned_out(len(table), segment, 28)
    same(s.gather(table, out=out), expect(raw, table, segment, hop))
    untouched()


def test_one_utterance_one_row(gt):
    hop, segment = 4, 20
    raw = SR.raw_corpus(hop, 5, seed=3, frames=[7])
    s = gt.SegmentSampler(config(hop, segment, 1), SR.prepared(raw, hop), device=DEV)
    for k in (0, 2):
        same(s.gather([(0, k)]), expect(raw, [(0, k)], segment, hop))


def test_refusals_return_the_code_before_any_launch(gt):
    hop, segment = 4, 20
    raw = SR.raw_corpus(hop, 5, seed=4)
    s = gt.SegmentSampler(config(hop, segment), SR.prepared(raw, hop), device=DEV)
    end = s.interval_end(2)
    for table, what in (([(0, 0), (len(raw), 0)], "row 1: utterance 5"), ([(-1, 0)], "row 0: utterance -1"),
                        ([(1, 0), (0, 0), (2, end + 1)], "row 2: start_step"), ([(2, -1)], "row 0: start_step"),
                        ([(0, 0)] * (gt.SEGMENT_MAX_BATCH + 1), "B = 257"), ([], "B = 0")):
        out, untouched = poisoned_out(max(len(table), 1), segment, 5)
        if not table:
            out = tuple(t[:0] for t in out)
        with pytest.raises(gt.DisscError, match=what):
            s.gather(table, out=out)
        torch.cuda.synchronize()
        untouched(inside_too=True)
    s.segment = 18
    with pytest.raises(gt.DisscError, match="multiple of code_hop_size"):
        s.gather([(0, 0)], out=(torch.empty(1, 1, 18, device=DEV), torch.empty(1, 4, dtype=torch.int64, device=DEV),
                                torch.empty(1, 1, 4, device=DEV), torch.empty(1, 1, dtype=torch.int64, device=DEV)))
    with pytest.raises(gt.DisscError, match="multiple of code_hop_size"):
        gt.SegmentSampler(config(4, 18), SR.prepared(raw, hop), device=DEV)
    with pytest.raises(gt.DisscError, match="item 1"):
        items = SR.prepared(raw, hop)
        items[1]["gt"] = items[1]["gt"][:-1]
        gt.SegmentSampler(config(hop, segment), items, device=DEV)


def test_batches_are_consecutive_items_with_private_seeded_draws(gt):
    hop, segment = 4, 20
    raw = SR.raw_corpus(hop, 5, seed=5)
    items = SR.prepared(raw, hop)
    a, b = (gt.SegmentSampler(config(hop, segment), items, seed=9, device=DEV) for _ in range(2))
    assert len(a) == 2  # five items, batches of two, drop_last
    random.seed(0)  # the global generator is not the sampler's
    ta = [a.draw(i) for i in range(len(a))]
    random.seed(1)
    tb = [b.draw(i) for i in range(len(b))]
    assert ta == tb and [[u for u, _ in t] for t in ta] == [[0, 1], [2, 3]]
    rng = random.Random(9)
    assert [k for t in ta for _, k in t] == [rng.randint(0, gt.interval_end(len(items[u]["code"]), hop, segment)) for u in range(4)]
    batches = list(b)
    assert len(batches) == 2 and batches[0]["y"].shape == (2, 1, segment) and batches[0]["spkr"].shape == (2, 1)


def test_rows_beyond_int32_are_refused_not_wrapped(gt):
    hop, segment = 4, 20
    s = gt.SegmentSampler(config(hop, segment), SR.prepared(SR.raw_corpus(hop, 5, seed=6), hop), device=DEV)
    for row in ((2 ** 32, 0), (0, 2 ** 32), (0,)):
        with pytest.raises(gt.DisscError, match="row 1"):
            s.gather([(0, 0), row])
