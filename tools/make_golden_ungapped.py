"""Writes tests/golden/ungapped_vectors.npz from the LIVE reference (oracle/_ref/libsdref.so, see tests/ungapped_ref.py):
sequence pairs with the score SmithWaterman::ungapped_alignment gives them, and the prefilter lists `ungappedprefilter`
writes for a fixed sample of queries of the two example genomes.  Results only: sequences, scores, lists.

    python tools/make_golden_ungapped.py        (needs `make -C oracle _ref/libsdref.so` and a built libsdgpu.so; no GPU)
"""
import gzip
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ungapped_ref as ur   # noqa: E402
from spacedust_amd.api import Host   # noqa: E402

# both sides of every boundary of the kernel's layout: 64 target columns per fetch, 128 / 256 / 512 query rows
# per length class, 512-row strips of longer queries
LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1537]
EX_SAMPLE, EX_MAX_SEQS, EX_MIN_SCORE, EX_COV_MODE, EX_COV = 32, 300, 15, 2, 0.8


def mutate(rng, s, rate):
    s = s.copy()
    hit = rng.random(len(s)) < rate
    s[hit] = rng.integers(0, 20, int(hit.sum()))
    return s


def example_sequences():
    seqs = []
    for f in ('NC_000913.faa', 'NC_000915.faa'):
        cur = None
        for line in gzip.open(os.path.join(ROOT, 'tests', 'golden', 'examples', f + '.gz'), 'rt'):
            line = line.rstrip('\n')
            if line.startswith('>'):
                if cur is not None:
                    seqs.append(''.join(cur))
                cur = []
            else:
                cur.append(line)
        seqs.append(''.join(cur))
    return seqs


def main():
    rng = np.random.default_rng(20261016)
    host = Host()
    M = host.matrix(0)[0].reshape(21, 21)
    a2n = host.matrix(0)[2]
    assert all(a2n[ord(c)] == i for i, c in enumerate(ur.ALPHABET))
    master = rng.integers(0, 20, 65535).astype(np.uint8)
    pool, names = [], {}

    def add(name, s):
        names[name] = len(pool)
        pool.append(np.asarray(s, np.uint8))
        return names[name]

    pairs = []
    for L in LENGTHS:
        add(('A', L), master[:L])
        add(('B', L), mutate(rng, master[:L], 0.3))
        add(('C', L), rng.integers(0, 20, L))
    for a in LENGTHS:
        for b in LENGTHS:
            pairs.append((names['A', a], names['B', b]))
        pairs.append((names['A', a], names['C', a]))
        pairs.append((names['C', a], names['A', a]))
    # low complexity
    lq = [add(('LQ', L), np.array([ur.ALPHABET.index(c) for c in rng.choice(list('AAAAGGSLWC'), L)])) for L in (200, 700)]
    lt = [add(('LT', L), np.array([ur.ALPHABET.index(c) for c in rng.choice(list('AAAAAGGSSL'), L)])) for L in (300, 900)]
    pairs += [(q, t) for q in lq for t in lt]
    # X: scattered, in runs, and nothing else
    xa = master[:300].copy()
    xa[rng.random(300) < 0.1] = 20
    xb = mutate(rng, master[:300], 0.2)
    xb[100:140] = 20
    ix = [add('XA', xa), add('XB', xb), add('XX', np.full(77, 20))]
    pairs += [(a, b) for a in ix for b in ix]
    # the longest sequences: a query longer than every target and the reverse
    q_long = add('Q65535', master)
    t_long = add('T65535', mutate(rng, master, 0.4))
    t_5000 = add('T5000', mutate(rng, master[:5000], 0.25))
    pairs += [(q_long, names['B', 1025]), (q_long, t_5000), (q_long, names['C', 65]), (names['A', 513], t_long),
              (names['A', 64], t_long), (names['C', 1], t_long), (q_long, names['C', 1])]

    off = np.zeros(len(pool) + 1, np.uint64)
    np.cumsum([len(s) for s in pool], out=off[1:])
    res = np.concatenate(pool).astype(np.uint8)
    cb = host.comp_bias(res, off)[0]

    pq, pt, comp, score = [], [], [], []
    for use_cb in (1, 0):
        ref = ur.RefUngapped(bool(use_cb))
        last = None
        for q, t in sorted(pairs):
            if q != last:
                ref.set_query(pool[q])
                last = q
            pq.append(q)
            pt.append(t)
            comp.append(use_cb)
            score.append(ref.score(pool[t]))
    pq, pt, comp, score = (np.array(x, np.int32) for x in (pq, pt, comp, score))
    caps = np.array([255 - ur.bias_of(M, cb[int(off[q]):int(off[q + 1])] if c else None) for q, c in zip(pq, comp)])
    print('%d pairs, %d at the ceiling (with bias %d, without %d), ceilings %s' % (
        len(pq), int((score == caps).sum()), int(((score == caps) & (comp == 1)).sum()), int(((score == caps) & (comp == 0)).sum()),
        sorted(set(caps.tolist()))))

    # the module's lists on the example genomes (key = position in the two FASTA files, createsetdb's order)
    seqs = example_sequences()
    e_res, e_off = host.map_sequences(seqs)
    e_len = (e_off[1:] - e_off[:-1]).astype(np.int64)
    sample = np.sort(np.random.default_rng(7).choice(len(seqs), EX_SAMPLE, replace=False))
    ref = ur.RefUngapped(True)
    ex_off, ex_key, ex_score = [0], [], []
    for q in sample:
        ref.set_query(e_res[int(e_off[q]):int(e_off[q + 1])])
        sc = [ref.score(e_res[int(e_off[t]):int(e_off[t + 1])]) if ur.can_be_covered(EX_COV, EX_COV_MODE, e_len[q], e_len[t]) else 0
              for t in range(len(seqs))]
        hits = ur.list_rule(sc, range(len(seqs)), e_len[q], e_len, EX_MIN_SCORE, EX_MAX_SEQS, EX_COV_MODE, EX_COV, identity_key=q)
        ex_key += [h[0] for h in hits]
        ex_score += [h[1] for h in hits]
        ex_off.append(len(ex_key))
    print('example lists: %d queries, %d hits' % (len(sample), len(ex_key)))

    np.savez_compressed(ur.GOLDEN, M=M.astype(np.int8), res=res, off=off, cb=cb.astype(np.int8), pq=pq, pt=pt, comp=comp.astype(np.uint8),
                        score=score, ex_n=np.int64(len(seqs)), ex_query=sample.astype(np.int64), ex_off=np.array(ex_off, np.int64),
                        ex_key=np.array(ex_key, np.int64), ex_score=np.array(ex_score, np.int32),
                        ex_par=np.array([EX_MAX_SEQS, EX_MIN_SCORE, EX_COV_MODE], np.int64), ex_cov=np.float32(EX_COV))
    print('wrote', ur.GOLDEN, os.path.getsize(ur.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
