#!/usr/bin/env python3
"""Golden rows for the constructed pairs of tests/nfgen.py (forward scores 1022, 1023 and 1024 in a 32-lane and a 64-lane class):
every pair through the REAL reference classes (oracle/_ref/libsdref.so) in alignment modes 0, 1 and 2 with the default gates
into tests/golden/narrow_final.npz, in the layout of score_classes.npz (tools/make_golden_score_classes.py; scgen.Rows reads
both).  --search first repeats the search for nfgen.TUNE with the oracle and prints it.  Writes the archive with fixed time
stamps: it regenerates byte for byte.  Dev container only: python tools/make_golden_narrow_final.py"""
import os
import pprint
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle.pyoracle import Oracle, Ref, RefSW  # noqa: E402
from spacedust_amd.api import Host  # noqa: E402
import nfgen  # noqa: E402
import scgen  # noqa: E402
from make_golden_score_classes import GOLD, rows_of, save  # noqa: E402


def main():
    ref, orc, host = Ref(6), Oracle(4), Host()
    if '--search' in sys.argv:
        found = nfgen.search(orc)
        pprint.pprint(found, width=140, compact=True)
        assert found == nfgen.TUNE, 'tests/nfgen.py: TUNE differs from what the search finds'
    seqs, pairs = nfgen.build()
    num = [orc.map_sequence(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    sw_bias, _, _ = host.comp_bias(np.concatenate(num), off)
    mat, _, _ = host.matrix(0)
    mat = np.array([mat[i] for i in range(441)], np.int32)
    sw = RefSW(ref, max(len(s) for s in seqs), nfgen.DB_RESIDUES)
    out = {k: [[] for _ in scgen.MODES] for k in ('res', 'evalue')}
    out.update({k: [] for k in ('bt', 'word', 'qbias', 'bt_nocov', 'start_nocov')})
    for p in pairs:
        q, t = p['q'], p['t']
        bias = abs(int(mat.min())) + abs(min(0, int(sw_bias[int(off[q]):int(off[q + 1])].min())))
        sw.set_query(seqs[q])
        res, evs, bts, word, nocov = rows_of(sw, lambda t_: orc.sw_align(num[q], orc.map_sequence(t_), nfgen.DB_RESIDUES), [seqs[t]], bias)
        for m in scgen.MODES:
            out['res'][m] += res[m]
            out['evalue'][m] += evs[m]
        out['bt'] += bts
        out['bt_nocov'].append(nocov[0][0])
        out['start_nocov'].append(nocov[0][1])
        out['word'] += word
        out['qbias'].append(bias)
        r = res[2][0]
        print('%-10s %4d x %4d score %5d word %d qEnd+1 %4d start %5d E %.2g' % (p['name'], len(seqs[q]), len(seqs[t]), r[0], word[0], r[2] + 1,
                                                                            r[1], evs[2][0]))
        assert r[0] == p['want'] and word[0] == 1, p
    arrays = dict(name=np.array([p['name'] for p in pairs]), q=np.array([p['q'] for p in pairs], np.int32),
                  t=np.array([p['t'] for p in pairs], np.int32), qlen=np.array([len(seqs[p['q']]) for p in pairs], np.int32),
                  tlen=np.array([len(seqs[p['t']]) for p in pairs], np.int32), digest=np.array(scgen.digest(seqs)),
                  n_seqs=np.int64(len(seqs)), db_residues=np.int64(nfgen.DB_RESIDUES), res=np.array(out['res'], np.int32),
                  evalue=np.array(out['evalue'], np.float64), bt=np.array('\n'.join(out['bt'])),
                  bt_nocov=np.array('\n'.join(out['bt_nocov'])), start_nocov=np.array(out['start_nocov'], np.int32),
                  word=np.array(out['word'], np.uint8), qbias=np.array(out['qbias'], np.int32),
                  wide_row_limit=np.int64(32767 // (int(mat.max()) + max(0, int(sw_bias.max())))))
    save(os.path.join(GOLD, 'narrow_final.npz'), arrays)
    print(len(pairs), 'pairs', len(seqs), 'sequences', os.path.getsize(os.path.join(GOLD, 'narrow_final.npz')), 'bytes')


if __name__ == '__main__':
    main()
