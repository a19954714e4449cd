"""Writes tests/golden/ungapped_paths.npz: the input of the multi-strip / grid-stride test of the exhaustive ungapped scan
(tests/test_gpu_ungapped_paths.py, test B) with the score of every pair from the numpy restatement of tests/ungapped_ref.py,
with and without composition bias.  Sequences, biases and scores only.

  * 64 queries of 513 to 1 601 residues: both sides of 1 024 and 1 536 (two, three and four strips of 512 rows), exact
    multiples of 512, odd lengths;
  * 300 targets of 0 to 1 200 residues in random order: unrelated ones of every length, short ones, empty ones, and windows
    of the queries mutated at 2 to 15 %, whose diagonals sit at the ceiling across strip boundaries;
  * PLANTED pairs of targets STEP apart (the targets one wavefront scans one after the other): the first ends on the
    query's rows up to 1 023, the second starts with the query's first rows one column later.  A scan whose first strip
    read the boundary line the previous target left behind would continue that diagonal.  `stale_cb` / `stale_nocb` hold
    what such a scan would give (lines zero at the start), so that the test can assert its input tells the two apart.

    python tools/make_golden_ungapped_paths.py        (needs a built libsdgpu.so for the matrix and the bias; no GPU;
                                                        about 10^10 cells per bias setting, spread over the CPUs)
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ungapped_ref as ur   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'ungapped_paths.npz')
Q_FIXED = [513, 514, 1023, 1024, 1025, 1535, 1536, 1537, 1599, 1601]
N_Q, N_T = 64, 300
STEP = 128      # 4 wavefronts x 32 workgroups along the targets: ugScanRange's launch for 64 multi-strip queries, 75 target groups
PLANTED = 14


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.concatenate(seqs).astype(np.uint8), off


def random_seq(rng, n):
    s = rng.integers(0, 20, n).astype(np.uint8)
    s[rng.random(n) < 0.01] = 20   # a few X
    return s


def make_inputs(rng):
    q_len = Q_FIXED + rng.integers(513, 1601, N_Q - len(Q_FIXED)).tolist()
    queries = [random_seq(rng, n) for n in q_len]
    targets = [random_seq(rng, int(n)) for n in rng.integers(0, 1201, 100)]
    targets += [random_seq(rng, int(n)) for n in rng.integers(1, 61, 52)]
    targets += [np.zeros(0, np.uint8)] * 8
    while len(targets) < N_T:   # windows of the queries, mutated, some with unrelated flanks
        q = queries[int(rng.integers(0, N_Q))]
        n = int(rng.integers(40, min(len(q), 1200) + 1))
        a = int(rng.integers(0, len(q) - n + 1))
        w = q[a:a + n].copy()
        hit = rng.random(n) < rng.choice([0.02, 0.05, 0.15])
        w[hit] = rng.integers(0, 20, int(hit.sum()))
        if n < 1100 and rng.random() < 0.5:
            w = np.concatenate([random_seq(rng, int(rng.integers(1, 1200 - n))), w])[:1200]
        targets.append(w)
    targets = [targets[i] for i in rng.permutation(N_T)]
    long_q = [q for q in queries if len(q) > 1024]
    for x, i in enumerate(rng.choice(STEP, PLANTED, replace=False)):
        q = long_q[x % len(long_q)]
        w, f = int(rng.integers(150, 400)), int(rng.integers(0, 300))
        first = np.concatenate([random_seq(rng, f), q[1024 - w:1024]])
        targets[int(i)] = first
        targets[int(i) + STEP] = np.concatenate([random_seq(rng, len(first)), q[:int(rng.integers(20, 60))]])
    return queries, targets


def stale_rows(args):
    """one query of three or four strips as a scan would score it whose FIRST strip read the boundary line of rows 1 023 that
    the wavefront's previous target (STEP before) left behind: row -1 at column j is that line's entry j - 1"""
    M, q, cb, t_res, t_off = args
    M = np.asarray(M, np.int16).reshape(21, 21)
    nt = len(t_off) - 1
    t_len = (t_off[1:] - t_off[:-1]).astype(np.int64)
    lmax = int(t_len.max())
    cbi = np.zeros(len(q), np.int16) if cb is None else cb.astype(np.int16)
    cap = 255 - ur.bias_of(M, cbi)
    prof = np.full((22, len(q)), -1000, np.int16)
    prof[:21] = M[:, q.astype(np.int64)] + cbi
    out = np.zeros(nt, np.int32)
    line = np.zeros((STEP, lmax + 1), np.int16)
    for t0 in range(0, nt, STEP):
        ids = np.arange(t0, min(nt, t0 + STEP))
        T = np.full((len(ids), lmax), 21, np.int64)
        for x, t in enumerate(ids):
            T[x, :t_len[t]] = t_res[int(t_off[t]):int(t_off[t + 1])]
        S = np.zeros((len(ids), len(q) + 1), np.int16)
        best = np.zeros(len(ids), np.int16)
        new = line[:len(ids)].copy()
        for j in range(lmax):
            live = j < t_len[ids]
            S[:, 0] = np.where(live & (j >= 1), line[:len(ids), j - 1] if j else 0, 0)
            S[:, 1:] = np.clip(S[:, :-1] + prof[T[:, j]], 0, cap)
            np.maximum(best, S.max(axis=1), out=best)
            new[live, j] = S[live, 1024]
        line[:len(ids)] = new
        out[ids] = best
    return out


def stale_matrix(M, queries, q_off, cb, t_res, t_off, plain, workers):
    out = plain.copy()
    rows = [x for x, q in enumerate(queries) if len(q) > 1024]
    args = [(M, queries[x], None if cb is None else cb[int(q_off[x]):int(q_off[x + 1])], t_res, t_off) for x in rows]
    with ProcessPoolExecutor(workers) as ex:
        for x, r in zip(rows, ex.map(stale_rows, args)):
            out[x] = r
    return out


def _rows(args):
    M, q_res, q_off, cb, t_res, t_off, a, b = args
    o = q_off[a:b + 1]
    lo, hi = int(o[0]), int(o[-1])
    return ur.restate_matrix(M, q_res[lo:hi], o - o[0], None if cb is None else cb[lo:hi], t_res, t_off)


def restate_parallel(M, q_res, q_off, cb, t_res, t_off, workers):
    n = len(q_off) - 1
    with ProcessPoolExecutor(workers) as ex:
        parts = list(ex.map(_rows, [(M, q_res, q_off, cb, t_res, t_off, a, a + 1) for a in range(n)]))
    return np.concatenate(parts)


def main():
    from spacedust_amd.api import Host
    rng = np.random.default_rng(20261017)
    host = Host()
    M = host.matrix(0)[0].reshape(21, 21)
    queries, targets = make_inputs(rng)
    q_res, q_off = pack(queries)
    t_res, t_off = pack(targets)
    cb = host.comp_bias(q_res, q_off)[0]
    workers = min(16, os.cpu_count() or 1)
    with_cb = restate_parallel(M, q_res, q_off, cb, t_res, t_off, workers)
    without = restate_parallel(M, q_res, q_off, None, t_res, t_off, workers)
    assert with_cb.max() <= 255 and without.max() <= 255
    stale_cb = stale_matrix(M, queries, q_off, cb, t_res, t_off, with_cb, workers)
    stale_nocb = stale_matrix(M, queries, q_off, None, t_res, t_off, without, workers)
    for plain, stale in ((with_cb, stale_cb), (without, stale_nocb)):
        changed = plain != stale
        print('a stale first strip changes %d pairs of %d queries' % (int(changed.sum()), int(changed.any(axis=1).sum())))
        assert (stale >= plain).all() and changed.sum() >= 3 * PLANTED and changed.any(axis=1).sum() >= PLANTED // 2
    np.savez_compressed(OUT, M=M.astype(np.int8), q_res=q_res, q_off=q_off, q_cb=cb.astype(np.int8), t_res=t_res, t_off=t_off,
                        score_cb=with_cb.astype(np.uint8), score_nocb=without.astype(np.uint8),
                        stale_cb=stale_cb.astype(np.uint8), stale_nocb=stale_nocb.astype(np.uint8))
    print('%s: %d queries (%d residues), %d targets (%d residues), %d bytes'
          % (OUT, N_Q, len(q_res), N_T, len(t_res), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
