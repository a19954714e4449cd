"""tests/golden/tantan_vectors.npz (tools/make_golden_tantan.py: tantan's float posteriors of the reference's own Masker, read
through its mask threshold) as the tantan tests read it, and the reading itself.

A residue is masked iff (double) p >= maskProb, p its float posterior.  For a float v with up(v) the next float above it, a residue
masked at maskProb = (double) v and not at (double) up(v) has p == v to the bit: anything that takes a threshold and returns
mask bytes shows its posteriors -- by bisection over the floats where nothing is known (recover), by two runs per distinct
value where expected posteriors exist (the tests)."""
import functools
import os

import numpy as np

from dbutil import GOLD

X = 20
C_THRESHOLDS = (0.2, 0.5, 0.9, 0.99)


@functools.lru_cache(None)
def golden():
    return np.load(os.path.join(GOLD, 'tantan_vectors.npz'))


def up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf), dtype=np.float32)


def _key(f):
    """float32 -> integers ordered as the floats are"""
    b = np.asarray(f, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, 0x7FFFFFFF - (b & 0x7FFFFFFF), b + 0x80000000)


def _unkey(k):
    k = np.asarray(k, np.int64)
    b = np.where(k >= 0x80000000, k - 0x80000000, (0x7FFFFFFF - k) | 0x80000000)
    return b.astype(np.uint32).view(np.float32)


LO, HI = np.float32(-1.0), np.float32(2.0)   # the search range: a posterior outside [0, 1] is found, not clipped


def recover(mask_fn, seq):
    """the float32 posterior of every residue of seq (no X in it) from mask_fn(seq, threshold) -> (masked bytes, count): the
    largest float the residue is still masked at, by bisection over the bit patterns of [-1, 2]; positions that share a
    midpoint share the call"""
    seq = np.ascontiguousarray(seq, np.uint8)
    assert not (seq == X).any()
    lo = np.full(len(seq), int(_key(LO)), np.int64)   # masked at lo ...
    hi = np.full(len(seq), int(_key(HI)), np.int64)   # ... and not at hi
    for edge, want in ((LO, True), (HI, False)):
        m, _ = mask_fn(seq, float(edge))
        assert ((m == X) == want).all(), 'a posterior outside [-1, 2)'
    while True:
        act = np.nonzero(hi - lo > 1)[0]
        if len(act) == 0:
            break
        mids = (lo[act] + hi[act]) // 2
        for mid in np.unique(mids):
            m, _ = mask_fn(seq, float(_unkey(mid)))
            sel = act[mids == mid]
            x = m[sel] == X
            lo[sel[x]] = mid
            hi[sel[~x]] = mid
    return _unkey(lo)


@functools.lru_cache(None)
def seqset(name):
    """(residues uint8, offsets uint64, posteriors float32 per residue) of set 'A' (the ladder: lengths 1..72, 100, 127, 128, 129,
    260) or 'B' (two long sequences); arrays are read-only"""
    g = golden()
    out = g[name + '_res'], g[name + '_off'].astype(np.uint64), g[name + '_post']
    for a in out:
        a.setflags(write=False)
    return out


def sequences(name):
    res, off, post = seqset(name)
    return [(res[int(off[i]):int(off[i + 1])], post[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


@functools.lru_cache(None)
def set_c():
    """X on input: (residues, offsets, masked bytes [threshold][residue], counts [threshold][sequence]) at C_THRESHOLDS"""
    g = golden()
    assert tuple(g['C_thr']) == C_THRESHOLDS
    return g['C_res'], g['C_off'].astype(np.uint64), g['C_mask'], g['C_count']


def concat(seqs):
    """[(residues, posteriors)] -> (residues, offsets, posteriors) of one DB"""
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s, _ in seqs])
    cat = lambda parts, dt: np.concatenate([np.asarray(p, dt) for p in parts]) if parts else np.zeros(0, dt)
    return cat([s for s, _ in seqs], np.uint8), off, cat([p for _, p in seqs], np.float32)


def expected(res, post, thr):
    """(masked bytes, count) the posteriors give at threshold thr: the compare of tantan.cpp:527, float against double"""
    x = post.astype(np.float64) >= float(thr)
    return np.where(x, np.uint8(X), res).astype(np.uint8), int(x.sum())


def edge_thresholds():
    return [-1.0, 0.0, float(np.float32(1e-45)), 0.5, 0.9, 1.0, float(up(1.0)), 2.0]


def pick(post, n=48):
    """n of the distinct posteriors: the four nearest below 0.9 and the four at or above it, the smallest above 0 and the largest
    below 1, the rest spread evenly by rank"""
    d = np.unique(post)
    at = int(np.searchsorted(d, np.float32(0.9)))
    take = set(range(max(0, at - 4), min(len(d), at + 4)))
    take.add(int(np.searchsorted(d, np.float32(0), side='right')))
    take.add(int(np.searchsorted(d, np.float32(1))) - 1)
    take = {i for i in take if 0 <= i < len(d)}
    rest = [i for i in range(len(d)) if i not in take]
    want = min(n - len(take), len(rest))
    if want > 0:
        take.update(rest[int(i)] for i in np.linspace(0, len(rest) - 1, want).round())
    return d[sorted(take)]
