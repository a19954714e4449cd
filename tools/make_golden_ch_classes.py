#!/usr/bin/env python3
"""Golden rows for the constructed clusterhits entries of tests/chgen.py (class_entries): every entry through the reference's
own compiled clusterhits code (oracle/_ref/libsdref_ch.so: R/src/util/ClusterHits.cpp compiled where it lies, its merge loop
re-driven over flat arrays, with the reference's logGamma table) under every parameter set of chgen.param_sets(), into
tests/golden/ch_classes.npz.  Per parameter set and entry: the cluster of every hit and its place in the printed order
(16 bits each, 0xFFFF = in no cluster), the number of clusters, their sizes and the bit patterns of pCO and pMH; the sets
follow one another in flat arrays.  A digest of the generator's output goes with them.  Writes the archive with fixed time
stamps: it regenerates byte for byte.  Dev container only:  python tools/make_golden_ch_classes.py"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.pyoracle import RefClusterHits  # noqa: E402
import chgen  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def save(path, arrays):
    with zipfile.ZipFile(path, 'w') as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED, 9)


def main():
    ref = RefClusterHits()
    cases = chgen.class_entries()
    lg = ref.lgamma_table(max(int(max(c['q'].max(initial=0), c['t'].max(initial=0), c['nq'], len(c['q']))) for c in cases) + 16)
    cof, rank, ncl, size, pco, pmh, par = [], [], [], [], [], [], []
    for ps, idx in chgen.param_sets():
        par.append([ps['d'], ps['cls'], ps['alpha'], ps['p_clu'], ps['p_mh'], len(idx)])
        for x in idx:
            c = cases[x]
            rcof, rrank, rcs, rpco, rpmh = ref.entry(c['q'], c['t'], c['s'], c['p'], c['nq'], d=ps['d'], cls=ps['cls'], alpha=ps['alpha'],
                                                     p_clu=ps['p_clu'], p_mh=ps['p_mh'], lg=lg)
            assert len(rcs) < 0xFFFF and (len(rcs) == 0 or rcs.max() < 0xFFFF)
            cof.append(np.where(rcof == 0xFFFFFFFF, 0xFFFF, rcof).astype(np.uint16))
            rank.append(np.where(rcof == 0xFFFFFFFF, 0xFFFF, rrank).astype(np.uint16))
            ncl.append(len(rcs))
            size.append(rcs.astype(np.uint32))
            pco.append(rpco.view(np.uint64))
            pmh.append(rpmh.view(np.uint64))
        print('d %2d cls %d alpha %-4g thresholds %-5g %-5g: %3d entries, %4d clusters' % (ps['d'], ps['cls'], ps['alpha'], ps['p_clu'], ps['p_mh'],
                                                                                      len(idx), sum(ncl[-len(idx):])))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    arrays = dict(name=np.array([c['name'] for c in cases]), K=np.array([len(c['q']) for c in cases], np.uint32),
                  repeats=np.array([c['repeats'] for c in cases], np.uint8), digest=np.array(chgen.digest(cases)),
                  params=np.array(par, np.float64), cluster_of=cat(cof, np.uint16), rank=cat(rank, np.uint16),
                  n_clusters=np.array(ncl, np.uint32), size=cat(size, np.uint32), pCO=cat(pco, np.uint64), pMH=cat(pmh, np.uint64))
    path = os.path.join(GOLD, 'ch_classes.npz')
    save(path, arrays)
    print(len(cases), 'entries,', len(par), 'parameter sets,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
