#!/usr/bin/env python3
"""Golden vectors for the alternative alignments (`align --alt-ali N`): the loop of Alignment::computeAlternativeAlignment
(M/src/alignment/Alignment.cpp:569-601) around the REAL reference matcher (oracle/_ref/libsdref.so through oracle.pyoracle.RefSW):
set_query once, then align() on the target's ASCII with X written over the masked positions, accepted by tests/altali_ref.py's
checkCriteria with the thresholds the tests use.  Dev container only:  python tools/make_golden_altali.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import altali_ref as ar  # noqa: E402
from oracle.pyoracle import Ref, RefSW  # noqa: E402

AA = 'ACDEFGHIKLMNPQRSTVWY'
DB_RESIDUES = 5000000
# sw_mode, cov_mode, cov_thr, eval_thr, seq_id_thr, aln_len_thr, seq_id_mode
PARAMS = [(2, 2, 0.5, 1e-3, 0.0, 0, 0), (1, 2, 0.5, 1e-3, 0.0, 0, 0), (2, 0, 0.0, 10.0, 0.3, 30, 0), (2, 2, 0.8, 1e-5, 0.2, 0, 1),
          (1, 1, 0.05, 1e-3, 0.25, 40, 0), (2, 2, 0.3, 1e-3, 0.0, 0, 2)]
REC = ar.REC_FIELDS


def main():
    rng = np.random.default_rng(20261017)

    def rand(n):
        return ''.join(rng.choice(list(AA), int(n)))

    def diverge(s, rate):
        s = list(s)
        for p in np.nonzero(rng.random(len(s)) < rate)[0]:
            s[p] = AA[rng.integers(20)]
        if rate > 0 and rng.random() < 0.5:
            p = int(rng.integers(3, len(s) - 3))
            if rng.random() < 0.5:
                s[p:p] = list(rand(rng.integers(1, 6)))
            else:
                del s[p:p + int(rng.integers(1, 5))]
        return ''.join(s)

    seqs, cases, cls = [], [], []

    def add(q, t, pi, n, kind, identity=False):
        seqs.append(q)
        if identity:
            ti = len(seqs) - 1
        else:
            seqs.append(t)
            ti = len(seqs) - 1
        cases.append((len(seqs) - (1 if identity else 2), ti, pi, n, 1 if identity else 0))
        cls.append(kind)

    def tandem(dom, rates, lead=None, tail=None):
        parts = [rand(rng.integers(10, 60)) if lead is None else lead]
        for i, r in enumerate(rates):
            parts.append(diverge(dom, r))
            parts.append(rand(rng.integers(10, 50)) if (tail is None or i + 1 < len(rates)) else tail)
        return ''.join(parts)

    # 2, 3 and 4 diverged copies of the query's domain, N in {1, 2, 3, 10}: rounds end by N and by a rejected result
    for copies in (2, 3, 4):
        for n in (1, 2, 3, 10):
            for rep in range(8):
                dom = rand(rng.integers(60, 200 if copies < 4 else 150))   # (targets stay below 900 residues)
                rates = [0.1] + [float(rng.uniform(0.15, 0.45)) for _ in range(copies - 1)]
                order = rng.permutation(copies)
                add(dom, tandem(dom, [rates[i] for i in order]), int((rep + copies + n) % len(PARAMS)), n, 'copies%d' % copies)
    for rep in range(10):   # one copy: the first alternative is rejected
        dom = rand(rng.integers(60, 200))
        add(dom, tandem(dom, [0.15]), rep % len(PARAMS), 3, 'single')
    for rep in range(4):    # identity seeds are skipped
        dom = rand(rng.integers(80, 200))
        add(dom + rand(20) + diverge(dom, 0.2), None, rep % 2, 3, 'identity', identity=True)
    for rep in range(6):    # the accepted interval starts at target position 0 / ends at the last residue
        dom = rand(rng.integers(60, 160))
        add(dom, tandem(dom, [0.0, 0.3], lead=''), [0, 1, 5][rep % 3], 2, 'start0')
        add(dom, tandem(dom, [0.3, 0.0], tail=''), [0, 1, 5][rep % 3], 2, 'endlast')
    for rep in range(6):    # a masked round that still saturates the byte kernel (score >= 255: rerun on the word kernel)
        dom = rand(200)
        add(dom, tandem(dom, [0.03, 0.05, 0.08]), [0, 1, 3][rep % 3], 3, 'saturate')
    for rep in range(6):    # identical copies: alternatives of one target with equal scores (the tie rule)
        dom = rand(rng.integers(60, 120))
        add(dom, tandem(dom, [0.0, 0.0, 0.0]), [0, 1][rep % 2], 10, 'tie')
    for rep in range(8):    # a query containing X
        dom = list(rand(rng.integers(80, 200)))
        t = tandem(''.join(dom), [0.1, 0.25, 0.3])
        for p in rng.choice(len(dom), 4, replace=False):
            dom[p] = 'X'
        add(''.join(dom), t, rep % len(PARAMS), 3, 'queryx')

    forced = {}
    for rep in range(4):    # a seed interval of one residue, [0, 0]: its exclusive end masks nothing, so the alternative is the full
        dom = rand(rng.integers(60, 160))   # alignment from target position 0 (an inclusive end would move its start to 1)
        add(dom, tandem(dom, [0.0, 0.3], lead=''), rep % 2, 2, 'exclusive')
        forced[len(cases) - 1] = (0, 0)

    ref = Ref(6)
    sw = RefSW(ref, 1200, DB_RESIDUES)
    assert max(len(s) for s in seqs) <= 900
    seeds, counts, recs, evs, bts = [], [], [], [], []
    seen = set()
    for ci, ((qi, ti, pi, n, ident), kind) in enumerate(zip(cases, cls)):
        p = ar.params(PARAMS[pi])
        q, t = seqs[qi], seqs[ti]
        sw.set_query(q)

        def align(num, t=t, p=p):
            masked = bytes(ord('X') if c == ar.X else a for a, c in zip(t.encode(), num))
            r = sw.align(masked, sw_mode=p['sw_mode'], eval_thr=p['eval_thr'], cov_mode=p['cov_mode'], cov_thr=p['cov_thr'])
            if r['btLen'] <= 0:
                r['identical'] = 0
            return r
        marker = np.zeros(len(t), np.uint8)   # (only positions equal to ar.X matter to align())
        if ident:
            seeds.append((0, len(t) - 1))
            alts = ar.alternatives(align, marker, 0, len(t) - 1, n, len(q), p, identity=True)
            assert alts == []
        else:
            first = align(marker)
            assert ar.accepted(first, len(q), len(t), p), (kind, pi, first)   # a seed is an accepted alignment
            if ci in forced:
                first = dict(first, tStart=forced[ci][0], tEnd=forced[ci][1])
            seeds.append((first['tStart'], first['tEnd']))
            alts = ar.alternatives(align, marker, first['tStart'], first['tEnd'], n, len(q), p)
            if ci in forced:
                assert alts and alts[0]['tStart'] == 0
            if first['tStart'] == 0:
                seen.add('start0')
            if first['tEnd'] == len(t) - 1:
                seen.add('endlast')
        counts.append(len(alts))
        for r in alts:
            recs.append([r[f] for f in REC])
            evs.append(r['evalue'])
            bts.append(r['backtrace'])
        if not ident:
            seen.add('byN' if len(alts) == n else 'byReject')
            if len(alts) == 0:
                seen.add('firstRejected')
            if any(r['score'] >= 255 for r in alts):
                seen.add('saturated')
            if len({r['score'] for r in alts}) < len(alts):
                seen.add('tie')
            seen.add('swMode%d' % p['sw_mode'])
            if 'X' in q and alts:
                seen.add('queryx')
            seen.add(kind)
        else:
            seen.add('identity')
    need = {'byN', 'byReject', 'firstRejected', 'identity', 'start0', 'endlast', 'saturated', 'tie', 'swMode1', 'swMode2', 'queryx', 'copies2',
            'copies3', 'copies4', 'exclusive'}
    assert need <= seen, need - seen
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    np.savez_compressed(ar.GOLDEN, letters=np.frombuffer(''.join(seqs).encode(), np.uint8), off=off, cases=np.array(cases, np.int64),
                        cls=np.array(cls), params=np.array(PARAMS, np.float64), db_residues=np.int64(DB_RESIDUES),
                        seeds=np.array(seeds, np.int64), counts=np.array(counts, np.int64), recs=np.array(recs, np.int64).reshape(-1, len(REC)),
                        evalues=np.array(evs, np.float64), bts=np.frombuffer('\n'.join(bts).encode(), np.uint8))
    print('%d cases, %d alternatives, %d bytes' % (len(cases), len(recs), os.path.getsize(ar.GOLDEN)), sorted(seen))


if __name__ == '__main__':
    main()
