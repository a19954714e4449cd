"""GPU: sd_clusterhits_batch on the constructed classes of chgen.class_entries against the golden rows of the reference's
compiled code (tests/golden/ch_classes.npz; tests/test_ch_classes.py shows on the CPU which branch every case reaches): one
batched call per parameter set -- the whole set of entries with K = 0 and K = 1 entries at its start, inside and at its end,
entries that repeat a query position (the dense host path) among the device's -- and everything exact: the number of
clusters, the cluster and printed place of every hit, sizes, and the bit patterns of pCO and pMH.  Needs neither the
reference tree nor oracle/_ref.  The `sdgpu clusterhits` run with other than the workflow's flags is in tests/test_gpu_cli.py
(test_clusterhits_module_with_other_flags), on the matches DB built there."""
import numpy as np
import pytest

import ch_ref
import chgen
from spacedust_amd import api

pytestmark = pytest.mark.gpu

SETS = chgen.param_sets()


@pytest.fixture(scope='module')
def cases():
    return chgen.class_entries()


@pytest.fixture(scope='module')
def golden(cases):
    g, rows = ch_ref.load_golden()
    assert str(g['digest']) == chgen.digest(cases), 'chgen.class_entries changed: rerun tools/make_golden_ch_classes.py'
    return rows


@pytest.fixture(scope='module')
def lg(host, cases):
    return host.lgamma_table(max(int(max(c['q'].max(initial=0), c['t'].max(initial=0), c['nq'], len(c['q']))) for c in cases) + 16)


def run_batch(gpu, host, lg, cases, idx, ps):
    off = np.zeros(len(idx) + 1, np.uint64)
    off[1:] = np.cumsum([len(cases[x]['q']) for x in idx])
    cat = lambda k, dt: np.concatenate([cases[x][k] for x in idx]).astype(dt)
    out = api.clusterhits(gpu, host, off, cat('q', np.uint32), cat('t', np.uint32), cat('s', np.uint8), cat('p', np.float64),
                          np.array([cases[x]['nq'] for x in idx], np.uint32), max_gene_gap=ps['d'], cluster_size=ps['cls'], alpha=ps['alpha'],
                          p_clu_thr=ps['p_clu'], p_mh_thr=ps['p_mh'], lgamma=lg)
    return off, out


def check_batch(off, out, cases, idx, rows, si, ps):
    clusters = 0
    for p, x in enumerate(idx):
        name = cases[x]['name']
        cof, rank, sizes, pco, pmh = rows[(si, x)]
        a, b, n = int(off[p]), int(off[p + 1]), len(sizes)
        assert int(out['n_clusters'][p]) == n, (name, ps, int(out['n_clusters'][p]), n)
        assert np.array_equal(out['cluster_of'][a:b], cof), (name, ps)
        assert np.array_equal(out['size'][a:a + n], sizes), (name, ps)
        assert np.array_equal(out['rank'][a:b], rank), (name, ps)
        assert np.array_equal(out['pCO'][a:a + n].view(np.uint64), pco), (name, ps, out['pCO'][a:a + n], pco.view(np.float64))
        assert np.array_equal(out['pMH'][a:a + n].view(np.uint64), pmh), (name, ps, out['pMH'][a:a + n], pmh.view(np.float64))
        clusters += n
    return clusters


@pytest.mark.parametrize('si', range(len(SETS)), ids=['d%d-cls%d-alpha%g-clu%g-mh%g' % (ps['d'], ps['cls'], ps['alpha'], ps['p_clu'], ps['p_mh'])
                                                     for ps, _ in SETS])
def test_one_batch_per_parameter_set_equals_golden_rows(si, gpu, host, lg, cases, golden):
    ps, idx = SETS[si]
    assert len(idx) == (len(cases) if si < len(chgen.WIDE_SETS) else len(chgen.GRID_CASES))   # no case left out
    off, out = run_batch(gpu, host, lg, cases, idx, ps)
    clusters = check_batch(off, out, cases, idx, golden, si, ps)
    if si < len(chgen.WIDE_SETS):
        assert clusters > 700


def test_batches_of_one_entry(gpu, host, lg, cases, golden):
    """every entry as a batch of its own, the empty one and the single hit included, under the workflow's parameters"""
    ps, idx = SETS[0]
    for x in idx:
        if len(cases[x]['q']) == 0:   # a batch without hits returns before it touches the device, outputs as they were
            off, out = run_batch(gpu, host, lg, cases, [x], ps)
            assert int(out['n_clusters'][0]) == 0
            continue
        off, out = run_batch(gpu, host, lg, cases, [x], ps)
        check_batch(off, out, cases, [x], golden, 0, ps)
