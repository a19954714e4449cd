#!/usr/bin/env python3
"""Golden rows for the constructed traceback pairs of tests/tbgen.py: every pair through the REAL reference classes
(oracle/_ref/libsdref.so: score, coordinates, identities, backtrace, E-value) into tests/golden/tb_classes.npz, next to
the letters, the pair names and the traceback class each pair is built to end in.  Prints the band history that the
reference's record implies and whether the oracle agrees.  Dev container only:  python tools/make_golden_tb_classes.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.pyoracle import Oracle, Ref, RefSW  # noqa: E402
import tbgen  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
DB_RESIDUES = 10 ** 7
FIELDS = ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'identical', 'btLen')


def main():
    ref, orc = Ref(6), Oracle(4)
    ps = tbgen.pairs()
    sw = RefSW(ref, max(max(len(p['q']), len(p['t'])) for p in ps), DB_RESIDUES)
    rows, bts, evs, labels = [], [], [], []
    for p in ps:
        sw.set_query(p['q'])
        r = sw.align(p['t'], sw_mode=2, eval_thr=10.0, cov_mode=2, cov_thr=0.0)
        o = orc.sw_align(orc.map_sequence(p['q']), orc.map_sequence(p['t']), DB_RESIDUES, cov_thr=0.0)
        same = all(o[k] == r[k] for k in FIELDS + ('backtrace', 'evalue'))
        got = tbgen.history(r['qEnd'] - r['qStart'] + 1, r['tEnd'] - r['tStart'] + 1, tbgen.deviation(r['backtrace']))
        want = got if p['dev'] is None else tbgen.history(len(p['q']), len(p['t']), p['dev'])   # (tie pairs: whatever the reference's path needs)
        whole = p['dev'] is None or (r['qStart'], r['tStart'], r['qEnd'], r['tEnd']) == (0, 0, len(p['q']) - 1, len(p['t']) - 1)
        gaps = [(a, n) for a, n in tbgen.runs(r['backtrace']) if a != 'M']
        print('%-16s %4d x %4d score %5d gaps %-28s %s%s%s' % (p['name'], len(p['q']), len(p['t']), r['score'], gaps[:4], '>'.join(got),
                                                           '' if got == want else '   NOT ' + '>'.join(want), '' if whole else '   NOT END TO END')
              + ('' if same else '   ORACLE DIFFERS'))
        rows.append([r[k] for k in FIELDS])
        bts.append(r['backtrace'])
        evs.append(r['evalue'])
        labels.append(want[-1])
    np.savez_compressed(os.path.join(GOLD, 'tb_classes.npz'), name=np.array([p['name'] for p in ps]), kind=np.array([p['kind'] for p in ps]),
                        q=np.array([p['q'] for p in ps]), t=np.array([p['t'] for p in ps]), label=np.array(labels),
                        res=np.array(rows, np.int64), bt=np.array(bts), evalue=np.array(evs, np.float64), db_residues=np.int64(DB_RESIDUES))


if __name__ == '__main__':
    main()
