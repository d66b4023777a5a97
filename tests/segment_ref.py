"""Shared by the tests of the segment sampler (not a test module): a literal numpy restatement of what CodeDataset.__getitem__
does to one utterance with eval_mode False (reference sr/dataset.py:240-267: trim, double until long enough, _sample_interval
199-219 with the start step given instead of drawn), and small corpora at the lengths where the law can go wrong."""
import numpy as np


def getitem_crop(audio, code, pitch, segment, hop, start_step=None):
    """-> (audio [segment], code [F], pitch [F], interval_end); start_step None: only interval_end is meaningful (crop at 0)"""
    code_length = min(audio.shape[0] // hop, code.shape[0])
    code = code[:code_length]
    audio = audio[:code_length * hop]
    pitch = pitch[:code_length]
    assert audio.shape[0] // hop == code.shape[0]
    while audio.shape[0] < segment:
        audio = np.hstack([audio, audio])
        code = np.hstack([code, code])
        pitch = np.hstack([pitch, pitch])
    seqs = [audio[None], code, pitch]
    N = max(v.shape[-1] for v in seqs)
    hops = [N // v.shape[-1] for v in seqs]
    lcm = np.lcm.reduce(hops)
    interval_end = N // lcm - segment // lcm
    s = 0 if start_step is None else start_step
    assert 0 <= s <= interval_end
    out = []
    for i, v in enumerate(seqs):
        start = s * (lcm // hops[i])
        end = (s + segment // lcm) * (lcm // hops[i])
        out.append(v[..., start:end])
    return out[0][0], out[1], out[2], int(interval_end)


def lengths(F):
    """utterance lengths in frames: one frame, one below / at / above a segment, three segments"""
    return [1, F - 1, F, F + 1, 3 * F]


def raw_corpus(hop, F, seed, frames=None):
    """per utterance the UNTRIMMED (audio f32, code i64, pitch f32, speaker id): audio with a partial hop behind the last frame,
    every other utterance with more units than its audio has hops"""
    rs = np.random.RandomState(seed)
    out = []
    for u, T in enumerate(lengths(F) if frames is None else frames):
        extra = 2 if u % 2 else 0
        out.append((rs.uniform(-1, 1, T * hop + hop - 1).astype(np.float32), rs.randint(0, 100, T + extra).astype(np.int64),
                    rs.uniform(-2, 2, T + extra).astype(np.float32), int(rs.randint(0, 200))))
    return out


def prepared(raw, hop):
    """the items sr/validate.py's prepare_items would hand the sampler: ground truth cut to whole hops, code and F0 to its hops"""
    items = []
    for u, (audio, code, pitch, spkr) in enumerate(raw):
        T = min(len(audio) // hop, len(code))
        items.append(dict(name=f"u{u}", gt=audio[:T * hop].copy(), code=code[:T].copy(), f0=pitch[:T].copy(), spkr=spkr))
    return items
