"""Helpers of the --target-search-mode 1 tests (tests/test_target_similar_golden.py, tests/test_gpu_target_similar.py): the golden
file tools/make_golden_target_similar.py writes and a plain restatement of the sequence form of KmerGenerator::generateKmerList."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'target_similar_vectors.npz')
SPAN = 10
SEED = (0, 1, 3, 5, 8, 9)

_cache = {}


def golden():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(GOLDEN))
    return _cache['g']


def seqs_of(name):
    """the ASCII sequences of a set ('S', 'R', 'B', 'G', 'M', 'Q')"""
    g = golden()
    letters, off = g[name + '_letters'].tobytes().decode(), g[name + '_off'].astype(np.int64)
    return [letters[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def short(v):
    """the reference's `short` arithmetic"""
    return ((int(v) + 32768) & 0xFFFF) - 32768


def window_list(score3, index3, w, thr):
    """generateKmerList of one window of six residue codes over the sorted 3-mer rows (KmerGenerator.cpp:107-216 at k = 6): parents of
    row0 at or above short(thr - best1), children of row1 at or above short(thr - parent); k-mer = i0 + 8000 i1"""
    i0 = w[0] + 20 * w[1] + 400 * w[2]
    i1 = w[3] + 20 * w[4] + 400 * w[5]
    r0, r1 = score3[i0].astype(np.int64), score3[i1].astype(np.int64)
    x0, x1 = index3[i0].astype(np.int64), index3[i1].astype(np.int64)
    n0 = int((r0 >= short(thr - int(r1[0]))).sum())
    out = []
    for a in range(n0):
        c = int((r1 >= short(thr - int(r0[a]))).sum())
        out.append(x0[a] + 8000 * x1[:c])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def restated_index(host, seqs, thr):
    """(triples in index order, list length of every window, records) of the similar-k-mer index of `seqs`, restated"""
    s3, i3, _ = host.ext_matrix(3)
    s3, i3 = np.asarray(s3).reshape(8000, 8000), np.asarray(i3).reshape(8000, 8000)
    res, off = host.map_sequences(seqs)
    rec, wl = [], []
    for t in range(len(seqs)):
        r = res[int(off[t]):int(off[t + 1])].astype(np.int64)
        for p in range(len(r) - SPAN + 1):
            w = [int(r[p + o]) for o in SEED]
            if max(w) >= 20:
                wl.append(0)
                continue
            km = window_list(s3, i3, w, thr)
            wl.append(len(km))
            rec.append(np.stack([km, np.full(len(km), t, np.int64), np.full(len(km), p, np.int64)], axis=1))
    rec = np.concatenate(rec) if rec else np.zeros((0, 3), np.int64)
    order = np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))
    rec = rec[order]
    first = np.ones(len(rec), bool)
    first[1:] = (rec[1:, 0] != rec[:-1, 0]) | (rec[1:, 1] != rec[:-1, 1])
    return rec[first], np.array(wl, np.int64), len(rec)


def windows_without_x(seq):
    n = 0
    for i in range(len(seq) - SPAN + 1):
        n += all(seq[i + s] != 'X' for s in SEED)
    return n
