"""Helpers of the k = 5 tests (tests/test_k5_host.py, tests/test_gpu_k5.py) and of tools/make_golden_k5.py, which writes the golden file
they read: how the crafted DB is laid out in tests/golden/k5_vectors.npz and how it is put together again."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'k5_vectors.npz')
PROFILE_GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'profile_vectors.npz')
SPAN = 12                 # spaced seed 110010000101 (Sequence.h:21)
SEED = (0, 1, 4, 9, 11)
TABLE = 20 ** 5
# QueryMatcher's hit buffer: 2 * max(10^6, number of targets) entries (QueryMatcher.cpp:43-47; c.maxDbMatches in sd_prefilter.hip)
HIT_BUFFER = 2 * 1000000

_cache = {}


def golden():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(GOLDEN))
    return _cache['g']


def family(base, mut):
    """the near-copies of `base` (ASCII bytes): mut rows are (copy, position, letter), copies without a row equal the base"""
    n = int(mut[:, 0].max()) + 1 if len(mut) else 0
    fam = np.tile(np.frombuffer(base, np.uint8), (n, 1))
    fam[mut[:, 0], mut[:, 1]] = mut[:, 2].astype(np.uint8)
    return [row.tobytes().decode() for row in fam]


def sequences(g=None):
    """the crafted DB: the small part as it is stored, then the family -> (list of ASCII strings, number of small sequences)"""
    g = g or golden()
    off = g['off'].astype(np.int64)
    blob = g['blob'].tobytes().decode()
    small = [blob[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return small + family(g['fam_base'].tobytes(), g['fam_mut'].astype(np.int64)), len(small)


def offsets_of(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return off


def profile_inputs():
    """profile_vectors.npz: (list of profile entries as bytes, list of ASCII sequences)"""
    if 'p' not in _cache:
        d = np.load(PROFILE_GOLDEN)
        poff = d['poff'].astype(np.int64)
        pdata = d['profiles'].tobytes()
        off = d['off'].astype(np.int64)
        blob = d['blob'].tobytes().decode()
        _cache['p'] = ([pdata[poff[i]:poff[i + 1]] for i in range(len(poff) - 1)], [blob[off[i]:off[i + 1]] for i in range(len(off) - 1)])
    return _cache['p']


def index_triples(kmer_offsets, entry_seq, entry_pos, n_seq=None):
    """(k-mer, sequence, position) of every index entry in index order; n_seq: only the entries of sequences below it"""
    lens = np.diff(np.asarray(kmer_offsets).astype(np.int64))
    kmer = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    t = np.stack([kmer, np.asarray(entry_seq).astype(np.int64), np.asarray(entry_pos).astype(np.int64)], axis=1)
    return t if n_seq is None else t[t[:, 1] < n_seq]


def rows_of(hits, cnt, queries):
    """(query, target, score, diagonal) rows of a prefilter result, query x of the call being queries[x]"""
    out = []
    for x, q in enumerate(queries):
        for h in hits[x, :int(cnt[x])]:
            out.append((int(q), int(h['seqId']), int(h['score']), int(h['diagonal'])))
    return np.array(out, np.int64).reshape(-1, 4)


def expected_rows(rows):
    e = rows.astype(np.int64).copy()
    e[:, 3] &= 0xFFFF
    return e
