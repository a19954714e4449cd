"""GPU: r2p_column_weights_kernel (csrc/hip/sd_r2p.hip) on every path, bit for bit.  sd_selftest_r2p_weights runs the weights
stage alone -- through the staging sd_r2p_batch_device uses -- on the constructed alignments of tests/r2pgen.py; the kernel's
freq and eff must equal the host's columnWeights in every bit.  Each test first asserts, from the float64 restatement's facts
(tests/r2p_ref.py; tests/test_r2p_restatement.py pins the host to it on the CPU), the input condition that reaches its path."""
import numpy as np
import pytest

import r2pgen
import r2p_ref
from spacedust_amd import api

pytestmark = pytest.mark.gpu
NT, ACT, LDSCOLS = r2pgen.NT, r2pgen.ACT, r2pgen.LDSCOLS


@pytest.fixture(scope='module')
def R():
    return r2p_ref.restated()


@pytest.fixture(scope='module')
def host_results(R):
    keys = list(R)
    return dict(zip(keys, api.r2p_weights([R[k][0] for k in keys])))


def _same_bits(what, cells, dev, host, change):
    for part, d, h in (('freq', dev[0], host[0]), ('eff', dev[1], host[1])):
        a, b = d.view(np.uint32).reshape(len(d), -1), h.view(np.uint32).reshape(len(h), -1)
        if not np.array_equal(a, b):
            cols = np.nonzero((a != b).any(axis=1))[0]
            c = int(cols[0])
            raise AssertionError('%s (%d rows x %d columns): %s differs in %d columns, first in column %d (%s): device %s, host %s'
                                 % (what, cells.shape[0], cells.shape[1], part, len(cols), c,
                                    'a change column' if c in change else 'no change column', d[c], h[c]))


def _check_case(gpu, R, host_results, name):
    keys = [k for k in R if k[0] == name]
    dev = api.r2p_weights([R[k][0] for k in keys], ctx=gpu)
    for k, d in zip(keys, dev):
        _same_bits('%s task %d' % k, R[k][0], d, host_results[k], R[k][3]['change'])


@pytest.mark.parametrize('n', r2pgen.ROW_PASS_ROWS)
def test_row_passes(gpu, R, host_results, n):
    """rows per pass of R2P_NT = 512: the change list and its drain, the active-row compaction with its running total, the
    staged residue sums and the row loops, at 1 .. 1 025 rows"""
    cells, _, _, f = R[('rows_%d' % n, 0)]
    assert cells.shape == (n, 48) and -(-n // NT) == {1: 1, 2: 1, 63: 1, 64: 1, 65: 1, 511: 1, 512: 1, 513: 2, 1024: 2, 1025: 3}[n]
    if n in (513, 1025):
        assert len(f['starts'][2]) == n > NT and any(r >= NT for r in f['ends'][40]) and (n == 513 or any(r >= 2 * NT for r in f['ends'][40]))
    if n >= NT:
        assert max(f['nActive'].values()) > (n - 1) // NT * NT   # active rows in every pass at once
    _check_case(gpu, R, host_results, 'rows_%d' % n)


def test_active_staging_boundary(gpu, R, host_results):
    """R2P_ACT = 768 active rows: staged in LDS with sixteen rows in flight and a tail at 767 / 768, the unstaged loop with
    eight in flight and a tail from 769 on"""
    f = R[('active_1537', 0)][3]
    assert tuple(f['nActive'][i] for i in range(10)) == r2pgen.ACTIVE_COUNTS and all(f['width'][i] >= 20 for i in range(10))
    assert {c % 16 for c in r2pgen.ACTIVE_COUNTS if c <= ACT} == {15, 0} and {c % 8 for c in r2pgen.ACTIVE_COUNTS if c > ACT} == {0, 1, 7}
    _check_case(gpu, R, host_results, 'active_1537')


@pytest.mark.parametrize('L', r2pgen.COLUMN_CLASS_L)
def test_column_classes(gpu, R, host_results, L):
    """windows under 20 columns (global weights), the sixteen-column unroll of the row-weight sum and its tail, LDSCOLS = 320
    (frequencies and logarithms in LDS, the shares aliasing the logarithms) and the long path above it: accumulator slices,
    global scratch, the entropy chain staged 320 columns at a time in two to four rounds with a partial last one"""
    cells, _, _, f = R[('cols_%d' % L, 0)]
    widths = set(f['width'].values())
    assert cells.shape == (40, L) and (L < 319 or len(f['change']) < L)   # (columns where nothing changes among the long ones)
    if L < 20:
        assert max(widths) < 20
    else:
        assert f['width'][0] == L and f['nActive'][0] >= 2
        assert max(-(-w // LDSCOLS) for w in widths) == -(-L // LDSCOLS)                  # the entropy rounds of the longest window
        assert L <= LDSCOLS or any(w % LDSCOLS for w in widths if w > LDSCOLS) or L == 640   # a partial last round
        assert L in (320, 512, 640) or f['width'][0] % 16 != 0   # the unroll's tail (a whole number of sixteens at 320, 512, 640)
    if L == 513:
        assert f['width'][0] > NT   # columns jmin + t and jmin + t + 512 share thread t's accumulator slice
    _check_case(gpu, R, host_results, 'cols_%d' % L)


@pytest.mark.parametrize('name', ['width_19', 'width_20', 'width_1'] + ['tie_%d' % P for P in r2pgen.TIE_PARTICIPATING])
def test_windows(gpu, R, host_results, name):
    """windows of exactly 19 (global weights) and 20 columns (shares) strictly inside the alignment, of one column, and the
    end-gap limit at its float32 tie: a tenth of the participating rows is inside the window, a tenth plus one outside"""
    f = R[(name, 0)][3]
    if name in ('width_19', 'width_20'):
        w = int(name[6:])
        assert (f['width'][10], f['jmin'][10], f['jmax'][10]) == (w, 10, 9 + w) and 0 < f['jmin'][10] and f['jmax'][10] < 47
    elif name == 'width_1':
        assert f['width'][7] == 1 and f['edge'][7] == (9, 0, 0, 9)
    else:
        P = int(name[4:])
        assert f['nActive'][2] == P and np.float32(P // 10) == np.float32(0.1) * np.float32(P)
        assert f['edge'][2] == (P // 10 + 1, P // 10, P // 10, P // 10 + 1) and (f['jmin'][2], f['jmax'][2]) == (1, 46)
    _check_case(gpu, R, host_results, name)


def test_degenerate_rows_and_columns(gpu, R, host_results):
    """an all-gap row, an all-X row, a row with one residue, X in the centre, a column with only X and gaps below the centre, a
    first column where nothing changes (eff 0, background frequencies); rows identical to the centre; eff carried over columns
    where nothing changes"""
    cells, _, eff, f = R[('degenerate', 0)]
    assert (cells[9] == 21).all() and (cells[10] == 20).all() and (cells[11] < 20).sum() == 1 and (cells[1:, 20] >= 20).all()
    assert 0 not in f['change'] and eff[0] == 0.0
    assert R[('degenerate', 1)][3]['nActive'] == {0: 50} and R[('degenerate', 2)][3]['change'] == [0, 9, 30, 61]
    _check_case(gpu, R, host_results, 'degenerate')


def test_mixed_batch_and_one_task_per_call(gpu):
    """48 alignments of shuffled shapes in one call -- the launch order (longest first) against the staging offsets, strides
    padded from L that is no multiple of 4 and row counts that are no multiple of 64 -- and the same alignments one per call"""
    tasks = r2pgen.cases()['mixed_48']
    shapes = [t.shape for t in tasks]
    assert len(tasks) == 48 and sum(L % 4 != 0 for _, L in shapes) >= 20 and sum(n % 64 != 0 for n, _ in shapes) >= 20
    assert sorted(range(48), key=lambda k: (-shapes[k][1], -shapes[k][0])) != list(range(48))
    host = api.r2p_weights(tasks)
    dev = api.r2p_weights(tasks, ctx=gpu)
    for k, t in enumerate(tasks):
        _same_bits('mixed task %d' % k, t, dev[k], host[k], r2p_ref.change_columns(t))
    for k, t in enumerate(tasks):
        _same_bits('mixed task %d alone' % k, t, api.r2p_weights([t], ctx=gpu)[0], host[k], r2p_ref.change_columns(t))


def _launches(gpu, fn):
    gpu.profile()
    try:
        out = fn()
        rep = gpu.profile_report()
    finally:
        gpu.profile(False)
    return out, int(rep['r2p_column_weights'][1]) if 'r2p_column_weights' in rep else 0


@pytest.fixture(scope='module')
def regression():
    """the first 300 regression queries with at least two edges; in the middle a centre of length 0 and a centre without edges"""
    from test_result2profile import _load, _edges
    api_, seqs, res, off, aln = _load()
    all_off, _, _, _, _ = _edges(api_, aln, range(len(seqs)))
    sel = [q for q in range(len(seqs)) if all_off[q + 1] - all_off[q] >= 2][:300]
    lonely = next(q for q in range(len(seqs)) if all_off[q + 1] == all_off[q])
    sel = sel[:150] + [None, lonely] + sel[150:]
    edge_off, et, eq, ets, bts = _edges(api_, aln, [q for q in sel if q is not None])
    edge_off = edge_off[:151] + [edge_off[150]] + edge_off[151:]   # the empty centre has no edges either
    letters = [res[int(off[q]):int(off[q + 1])] if q is not None else res[:0] for q in sel]
    qoff = np.zeros(len(sel) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(x) for x in letters])
    return (np.concatenate(letters), qoff, edge_off, et, eq, ets, bts, res, off)


def _groups(qoff, edge_off, budget):
    """the groups of r2pBatchImpl: centres are added while the estimate (edges + 1) x (L + 4) stays within the budget; returns
    (groups, groups with at least one centre of non-zero length = device calls)"""
    n = len(qoff) - 1
    groups = calls = 0
    g0 = 0
    while g0 < n:
        g1, est = g0, 0
        while g1 < n:
            add = (int(edge_off[g1 + 1]) - int(edge_off[g1]) + 1) * (int(qoff[g1 + 1]) - int(qoff[g1]) + 4)
            if g1 > g0 and est + add > budget:
                break
            est += add
            g1 += 1
        groups += 1
        calls += any(qoff[q + 1] > qoff[q] for q in range(g0, g1))
        g0 = g1
    return groups, calls


def test_groups_of_a_batch(gpu, regression, monkeypatch):
    """the group loop of sd_r2p_batch_device under SD_R2P_BUDGET: one centre per group, a handful of groups and one group give
    the bytes of the host path; one kernel launch per group that has a task"""
    args = regression
    qoff, edge_off = args[1], args[2]
    assert len(qoff) - 1 == 302 and qoff[151] == qoff[150] and edge_off[152] == edge_off[151] and qoff[152] > qoff[151]
    host = api.result2profile(*args)
    total = sum((edge_off[q + 1] - edge_off[q] + 1) * (int(qoff[q + 1]) - int(qoff[q]) + 4) for q in range(302))
    some = total // 6
    assert _groups(qoff, edge_off, 1) == (302, 301) and 3 <= _groups(qoff, edge_off, some)[0] <= 10
    assert _groups(qoff, edge_off, 1 << 30) == (1, 1)
    for budget in (1, some, None):
        if budget is None:
            monkeypatch.delenv('SD_R2P_BUDGET', raising=False)
        else:
            monkeypatch.setenv('SD_R2P_BUDGET', str(budget))
        try:
            dev, launches = _launches(gpu, lambda: api.result2profile(*args, ctx=gpu))
        finally:
            monkeypatch.delenv('SD_R2P_BUDGET', raising=False)
        assert launches == _groups(qoff, edge_off, budget if budget else 1 << 30)[1], (budget, launches)
        bad = [q for q in range(302) if dev[int(qoff[q]) * 25:int(qoff[q + 1]) * 25] != host[int(qoff[q]) * 25:int(qoff[q + 1]) * 25]]
        assert bad == [], (budget, bad[:10])


def test_global_weights_never_reach_the_device(gpu, regression):
    """--wg 1 (one weight per row everywhere) is a host computation also with a context: no launch of the kernel"""
    args = regression
    out, launches = _launches(gpu, lambda: api.result2profile(*args, ctx=gpu, wg=1))
    assert launches == 0 and out == api.result2profile(*args, wg=1)
    out, launches = _launches(gpu, lambda: api.result2profile(*args, ctx=gpu))
    assert launches == 1 and out != api.result2profile(*args, wg=1)
