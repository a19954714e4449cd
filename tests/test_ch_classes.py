"""CPU: the constructed clusterhits classes (chgen.class_entries) against the golden rows of the reference's compiled code
(tests/golden/ch_classes.npz, tools/make_golden_ch_classes.py).  No reference tree, no GPU:

  * the restatement of the kernel's incremental algorithm (ch_ref.cluster) with the product's emission arithmetic equals the
    golden rows on every entry with distinct query positions, under every parameter set;
  * every branch of that algorithm is taken by the case built for it, and the interleaved forms by none: they need a
    repeated query position, which neither the constructed cases with distinct positions nor chgen.many_entries have --
    the kernel states that as its invariant and has no code for them;
  * the dense host path (sd_host_clusterhits_dense, what sd_clusterhits_batch runs for an entry that repeats a query
    position) equals the golden rows on those entries and on every small entry beside them;
  * the restatement, turned wrong in the ways DESIGN lists as mutants of the kernel, misses the golden rows."""
import ctypes as C

import numpy as np
import pytest

import ch_ref
import chgen
from spacedust_amd import _lib
from spacedust_amd._lib import ptr

# the case built for every branch (ch_ref's docstring has the branches); counted under the workflow's parameters
REACHED_BY = {
    'score_append': 'stop_zero', 'score_prepend': 'stop_zero', 'merge_append': 'stop_zero', 'merge_prepend': 'init_tie',
    'stale_absorbed': 'stale_absorbed', 'stale_absorbing': 'stale_absorbing_falls', 'stale_absorbing_fell': 'stale_absorbing_falls',
    'stale_third': 'stale_third', 'takeover': 'stale_absorbed', 'stop_zero': 'stop_zero_at_once', 'stop_smin': 'stop_below_smin',
    'tied_argmax': 'tie_lattice', 'init_tie': 'init_tie',
}
NEVER = ('score_interleaved', 'merge_interleaved')


@pytest.fixture(scope='module')
def cases():
    return chgen.class_entries()


@pytest.fixture(scope='module')
def golden(cases):
    g, rows = ch_ref.load_golden()
    assert str(g['digest']) == chgen.digest(cases), 'chgen.class_entries changed: rerun tools/make_golden_ch_classes.py'
    assert list(g['name']) == [c['name'] for c in cases] and (g['K'] == [len(c['q']) for c in cases]).all()
    return rows


@pytest.fixture(scope='module')
def lg(host, cases):
    return host.lgamma_table(max(int(max(c['q'].max(initial=0), c['t'].max(initial=0), c['nq'], len(c['q']))) for c in cases) + 16)


@pytest.fixture(scope='module')
def partitions(cases, lg):
    """the restatement's partition and branch counts of every case with distinct positions, per gene gap"""
    memo = {}

    def get(x, d):
        if (x, d) not in memo:
            counts = ch_ref.new_counts()
            c = cases[x]
            memo[(x, d)] = ch_ref.cluster(c['q'], c['t'], c['s'], d, lg, counts)[0], counts
        return memo[(x, d)]
    return get


def same_rows(got, want):
    cof, rank, sizes, pco, pmh = got
    return (np.array_equal(cof, want[0]) and np.array_equal(rank, want[1]) and np.array_equal(sizes, want[2])
            and np.array_equal(np.asarray(pco, np.float64).view(np.uint64), want[3])
            and np.array_equal(np.asarray(pmh, np.float64).view(np.uint64), want[4]))


def test_case_set_is_what_the_issue_lists(cases):
    K = {c['name']: len(c['q']) for c in cases}
    assert {K['stride_%d' % k] for k in (2, 3, 255, 256, 257, 511, 512, 513)} == {2, 3, 255, 256, 257, 511, 512, 513}
    assert 1025 <= K['stride_1030'] and max(K.values()) <= 1100
    assert K['tie_lattice'] == K['tie_lattice_perm'] == 520 and K['collinear_600'] == 600
    assert sum(k <= 64 for k in K.values()) > len(K) * 2 // 3
    names = [c['name'] for c in cases]
    assert names[:2] == ['k0_first', 'k1_first'] and names[-2:] == ['k0_last', 'k1_last'] and 2 < names.index('k0_mid') < len(names) - 3
    rep = [c for c in cases if c['repeats']]
    assert len(rep) >= 10 and max(len(c['q']) for c in rep) == 60 and any(len(c['q']) <= 16 for c in rep)
    for c in rep:   # two or three hits per position somewhere; never two hits on one target position (see chgen)
        assert np.unique(c['q'], return_counts=True)[1].max() >= 2 and len(np.unique(c['t'])) == len(c['t'])
    sets = chgen.param_sets()
    assert {(ps['d'], ps['cls'], ps['p_clu']) for ps, _ in sets} >= {(d, cls, thr) for d in (1, 3, 10) for cls in (1, 2, 3, 5)
                                                                       for thr in (0.01, 1.0, 1e-10)}
    assert {ps['alpha'] for ps, _ in sets} == {1.0, 0.01}


def test_restatement_equals_golden_rows_on_distinct_positions(cases, golden, lg, partitions):
    L = _lib.load()
    n = clusters = 0
    for si, (ps, idx) in enumerate(chgen.param_sets()):
        for x in idx:
            c = cases[x]
            if c['repeats']:
                continue
            node_of, _ = partitions(x, ps['d'])
            got = ch_ref.emit(L, lg, c['q'], c['t'], c['s'], c['p'], c['nq'], node_of, ps['cls'], ps['alpha'], ps['p_clu'], ps['p_mh'])
            assert same_rows(got, golden[(si, x)]), (c['name'], ps)
            n += 1
            clusters += len(got[2])
    assert n > 900 and clusters > 3000


def test_every_branch_is_reached_by_its_case(cases, partitions, lg):
    names = [c['name'] for c in cases]
    d = chgen.DEFAULT['d']
    for branch, name in REACHED_BY.items():
        assert partitions(names.index(name), d)[1][branch] >= 1, (branch, name)
    assert set(REACHED_BY) | set(NEVER) == set(ch_ref.BRANCHES)
    for x, c in enumerate(cases):
        if not c['repeats']:
            counts = partitions(x, d)[1]
            assert all(counts[b] == 0 for b in NEVER), (c['name'], counts)
    # the numbers the cases were built for: 455 tied selections in either form of the lattice; a stale row for almost every
    # (merge, row) of the long chain
    for name in ('tie_lattice', 'tie_lattice_perm'):
        assert partitions(names.index(name), d)[1]['tied_argmax'] == 455
    chain = partitions(names.index('collinear_600'), d)[1]
    assert chain['stale_third'] + chain['stale_absorbing'] + chain['stale_absorbed'] >= 175000 and chain['merge_append'] == 599
    # a repeated position is what the interleaved forms need
    reached = ch_ref.new_counts()
    for c in cases:
        if c['repeats']:
            ch_ref.cluster(c['q'], c['t'], c['s'], d, lg, reached)
    assert reached['score_interleaved'] > 50 and reached['merge_interleaved'] > 20


def test_random_entries_never_repeat_a_query_position(lg):
    """why tests/test_gpu_clusterhits.py and the oracle tests never saw the interleaved forms: chgen.entry draws positions
    without replacement, and with distinct positions two compatible nodes never interleave"""
    counts = ch_ref.new_counts()
    for seed, n in ((2024, 1500), (77, 600)):
        for e in chgen.many_entries(seed, n):
            assert len(np.unique(e[0])) == len(e[0])
    for e in chgen.many_entries(2024, 40):
        ch_ref.cluster(e[0], e[1], e[2], 3, lg, counts)
    assert counts['score_interleaved'] == counts['merge_interleaved'] == 0 and counts['merge_prepend'] > 0 and counts['takeover'] > 0


def dense(L, lg, c, ps):
    K = len(c['q'])
    par = _lib.ChParams(ps['d'], ps['cls'], ps['alpha'], ps['p_clu'], ps['p_mh'])
    cof, rank, size = np.full(max(K, 1), 0xFFFFFFFF, np.uint32), np.zeros(max(K, 1), np.uint32), np.zeros(max(K, 1), np.uint32)
    pco, pmh, n = np.zeros(max(K, 1)), np.zeros(max(K, 1)), C.c_uint32()
    rc = L.sd_host_clusterhits_dense(K, ptr(c['q']), ptr(c['t']), ptr(c['s']), ptr(c['p']), c['nq'], C.byref(par), ptr(lg), len(lg),
                                     ptr(cof), ptr(rank), C.byref(n), ptr(pco), ptr(pmh), ptr(size))
    return rc, (cof[:K], rank[:K], size[:n.value], pco[:n.value], pmh[:n.value])


def test_dense_host_path_equals_golden_rows(cases, golden, lg):
    """the host function alone: every entry with a repeated query position (partition, printed order, P-value bits) and,
    being the reference's loop restated, every small entry with distinct positions as well"""
    L = _lib.load()
    n = 0
    for si, (ps, idx) in enumerate(chgen.param_sets()):
        for x in idx:
            c = cases[x]
            if c['repeats'] or len(c['q']) <= 64:
                rc, got = dense(L, lg, c, ps)
                assert rc == 0 and same_rows(got, golden[(si, x)]), (c['name'], ps)
                n += c['repeats']
    assert n >= 36 + 35 * 3


def test_dense_host_path_refuses_what_the_reference_reads_outside_its_table(lg):
    """four hits on two query and two target positions: a cluster of k = 4 over span 2 makes the reference read
    lookup[span - k + 1] = lookup[-1]; the host path fails instead of reading there"""
    L = _lib.load()
    c = chgen._case('outside', [0, 0, 1, 1], [0, 1, 1, 0])
    rc, _ = dense(L, lg, c, chgen.DEFAULT)
    assert rc != 0
    rc, _ = dense(L, lg, c, dict(chgen.DEFAULT, d=len(lg)))   # the gene gap's own table entry, lg[d + 2]
    assert rc != 0


@pytest.mark.parametrize('mutant', ch_ref.MUTANTS)
def test_golden_rows_catch_the_restatement_turned_wrong(mutant, cases, golden, lg):
    """each rule of the algorithm turned wrong in the restatement (the kernel's mutants of DESIGN, which the GPU file has to
    catch on the device) misses the golden rows on a small case -- or merges an emptied node, where the kernel would index
    with NIL"""
    L = _lib.load()
    small = {'argmax_block': 'box_touching', 'argmax_stride': 'tie_lattice_perm', 'keep_absorbed': 'box_nested', 'init_ge': 'init_tie',
             'no_seam': 'tpos_repeat_seam', 'box_d1': 'gaps_d3'}[mutant]
    x = [c['name'] for c in cases].index(small)
    c, ps = cases[x], chgen.DEFAULT
    try:
        node_of, _ = ch_ref.cluster(c['q'], c['t'], c['s'], ps['d'], lg, None, mutant)
    except IndexError:
        assert mutant == 'keep_absorbed'
        return
    got = ch_ref.emit(L, lg, c['q'], c['t'], c['s'], c['p'], c['nq'], node_of, ps['cls'], ps['alpha'], 1.0, 1.0)
    assert not same_rows(got, golden[(1, x)]), mutant
