"""CPU: the host's columnWeights (sd_selftest_r2p_weights without a context) against the float64 restatement of
tests/r2p_ref.py on the constructed alignments of tests/r2pgen.py, and each case's declared shape -- which row pass, staging
class, column class and window it reaches in r2p_column_weights_kernel -- asserted from the restatement's facts.
tests/test_gpu_r2p_weights.py compares the kernel with the host bit for bit on the same cases."""
import numpy as np
import pytest

import r2pgen
import r2p_ref
from spacedust_amd import api
from spacedust_amd._lib import SdError

# The largest deviation of the host from the restatement over the whole case set (float32 sums of up to about 1 500 addends,
# the approximate reciprocal with one Newton step, a float32 entropy chain of up to 961 x 20 terms), measured on an Intel
# Xeon host: |freq - ref| and |eff - ref| / max(1, ref).  The bounds are four times that: room for another CPU's rcpps bits.
MEASURED_FREQ, MEASURED_EFF = 2.54e-7, 1.62e-5
BOUND_FREQ, BOUND_EFF = 4 * MEASURED_FREQ, 4 * MEASURED_EFF


@pytest.fixture(scope='module')
def R():
    return r2p_ref.restated()


@pytest.fixture(scope='module')
def host_results(R):
    keys = list(R)
    return dict(zip(keys, api.r2p_weights([R[k][0] for k in keys])))


def test_host_agrees_with_the_restatement(R, host_results):
    worst_f = worst_e = 0.0
    for key, (hf, he) in host_results.items():
        cells, f, e, facts = R[key]
        df = float(np.abs(hf.astype(np.float64) - f).max())
        de = float((np.abs(he.astype(np.float64) - e) / np.maximum(1.0, e)).max())
        worst_f, worst_e = max(worst_f, df), max(worst_e, de)
        assert df <= BOUND_FREQ and de <= BOUND_EFF, (key, df, de)
    print('largest deviations: freq %.3g, eff %.3g (bounds %.3g, %.3g)' % (worst_f, worst_e, BOUND_FREQ, BOUND_EFF))


def test_one_window_column_is_worth_more_than_the_bound(R):
    """the bound distinguishes windows: on the case with the narrowest window of at least 20 columns, a window one column longer
    moves eff by more than the bound"""
    narrow = min((facts['width'][i], key, i) for key, (cells, _, _, facts) in R.items() for i in facts['change']
                 if facts['width'][i] >= 20 and facts['jmax'][i] < cells.shape[1] - 1)   # (a window that can grow by a column)
    width, key, i = narrow
    assert (width, key, i) == (20, ('width_20', 0), 10)
    cells, f, e, facts = R[key]
    background = api.Host().matrix(0)[1][:20]
    f2, e2, facts2 = r2p_ref.column_weights(cells, background, jmax_shift=1)
    assert facts2['width'][i] == 21
    moved = abs(e2[i] - e[i]) / max(1.0, e[i])
    print('eff at column %d: %.6f -> %.6f' % (i, e[i], e2[i]))
    assert moved > 10 * BOUND_EFF, moved


def test_a_window_always_holds_its_own_column(R):
    """`width == 0` (no column at or under the end-gap limit: jmin = L, jmax = -1, eff = 1) cannot be reached: the rows taking
    part at a change column have a residue there, so that column has no end gap among them and passes.  Every change column of
    every case has jmin <= i <= jmax; the narrowest window (one column) is the case width_1."""
    for key, (_, _, _, facts) in R.items():
        for i in facts['change']:
            assert facts['jmin'][i] <= i <= facts['jmax'][i], (key, i)
    f = R[('width_1', 0)][3]
    assert f['width'][7] == 1 and f['nActive'][7] == 10 and f['edge'][7] == (9, 0, 0, 9)


def _f(R, name, k=0):
    return R[(name, k)][3]


def test_row_pass_cases_are_what_they_say(R):
    for n in r2pgen.ROW_PASS_ROWS:
        cells, _, _, f = R[('rows_%d' % n, 0)]
        assert cells.shape == (n, 48) and f['change'] == r2p_ref.change_columns(cells)
    for n in (513, 1025):
        f = _f(R, 'rows_%d' % n)
        assert f['change'][0] == 2 and len(f['starts'][2]) == n > r2pgen.NT           # more rows start at once than a pass holds
        ends = f['ends'][40]
        assert any(r2pgen.NT <= r < 2 * r2pgen.NT for r in ends)                       # a row of the second pass ends
        assert n == 513 or (any(r >= 2 * r2pgen.NT for r in ends) and len(ends) > 100)   # and of the third
        assert R[('rows_%d' % n, 0)][2][0] == 0.0                                      # column 0 changes nothing: eff 0
    # active rows on both sides of every 512-row pass boundary in one change column
    assert any(v > 2 * r2pgen.NT for v in _f(R, 'rows_1025')['nActive'].values())


def test_active_staging_case_is_what_it_says(R):
    f = _f(R, 'active_1537')
    counts = [f['nActive'][i] for i in range(10)]
    assert tuple(counts) == r2pgen.ACTIVE_COUNTS and f['change'][:10] == list(range(10))
    assert all(f['width'][i] >= 20 for i in range(10))            # the share path, not the global weights
    # staged (<= 768): the sixteen-loop with tails of 15 and 0 rows; unstaged: the eight-loop with tails of 1, 7 and 0 rows
    assert [c % 16 for c in counts if c <= r2pgen.ACT] == [15, 0] and [c % 8 for c in counts if c > r2pgen.ACT] == [1, 7, 0, 1, 7, 0, 1, 1]
    assert any(r2pgen.ACT < v < 1537 for i, v in f['nActive'].items() if i >= 10)


def test_column_class_cases_are_what_they_say(R):
    for L in r2pgen.COLUMN_CLASS_L:
        cells, _, _, f = R[('cols_%d' % L, 0)]
        assert cells.shape == (40, L)
        widths = set(f['width'].values())
        if L < 20:
            assert max(widths) < 20            # global weights everywhere
        else:
            assert f['width'][0] == L          # the whole alignment is one window at column 0 ...
            assert L < 100 or len(widths) > 3  # ... and shorter ones follow
        rounds = set(-(-w // r2pgen.LDSCOLS) for w in widths if w >= 1)
        want = {1: {1}, 2: {1, 2}, 3: {2, 3}, 4: {3, 4}}[-(-L // r2pgen.LDSCOLS)]
        assert max(rounds) == max(want), (L, rounds)
    assert _f(R, 'cols_20')['width'][0] == 20 and _f(R, 'cols_21')['width'][0] == 21      # the share path's smallest windows
    assert _f(R, 'cols_36')['width'][0] % 16 == 4 and _f(R, 'cols_37')['width'][0] % 16 == 5
    assert _f(R, 'cols_513')['width'][0] == 513 > r2pgen.NT    # a thread's accumulator slice is used twice
    # a partial last entropy round on the long path, and an exactly full one
    assert any(w > r2pgen.LDSCOLS and w % r2pgen.LDSCOLS for w in _f(R, 'cols_961')['width'].values())
    assert _f(R, 'cols_640')['width'][0] == 2 * r2pgen.LDSCOLS
    # columns where nothing changes
    assert all(len(_f(R, 'cols_%d' % L)['change']) < L for L in r2pgen.COLUMN_CLASS_L if L >= 319)


def test_window_cases_are_what_they_say(R):
    for w in (19, 20):
        f = _f(R, 'width_%d' % w)
        assert f['change'] == [0, 10, 10 + w]
        assert (f['width'][10], f['jmin'][10], f['jmax'][10]) == (w, 10, 9 + w) and f['jmin'][10] > 0 and f['jmax'][10] < 47
        assert f['width'][0] == 48 and f['nActive'][10] == 10
    for P in r2pgen.TIE_PARTICIPATING:
        f = _f(R, 'tie_%d' % P)
        t = P // 10
        assert f['nActive'][2] == P and P % 10 == 0
        assert np.float32(t) == np.float32(0.1) * np.float32(P)      # the tie is exact in float32
        assert (f['jmin'][2], f['jmax'][2]) == (1, 46)
        assert f['edge'][2] == (t + 1, t, t, t + 1)                  # a tenth inside the window, a tenth plus one outside


def test_degenerate_cases_are_what_they_say(R):
    cells, freq, eff, f = R[('degenerate', 0)]
    assert (cells[9] == r2pgen.GAP).all() and (cells[10] == r2pgen.ANY).all() and (cells[11] < 20).sum() == 1
    assert cells[0, 0] == r2pgen.ANY and cells[0, 13] == r2pgen.ANY and cells[0, 20] < 20 and (cells[1:, 20] >= 20).all()
    assert 0 not in f['change'] and eff[0] == 0.0 and f['nActive'][20] == 1
    cells, freq, eff, f = R[('degenerate', 1)]
    assert (cells == cells[0]).all() and f['change'] == [0] and f['nActive'][0] == 50 and (eff == 1.0).all()
    cells, freq, eff, f = R[('degenerate', 2)]
    assert f['change'] == [0, 9, 30, 61] and (eff[1:9] == eff[0]).all() and eff[9] != eff[0]


def test_mixed_batch_is_what_it_says():
    tasks = r2pgen.cases()['mixed_48']
    assert len(tasks) == 48
    shapes = [t.shape for t in tasks]
    assert sum(L % 4 != 0 for _, L in shapes) >= 20 and sum(n % 64 != 0 for n, _ in shapes) >= 20
    assert sum(L > r2pgen.LDSCOLS for _, L in shapes) >= 5 and sum(n > r2pgen.NT for n, _ in shapes) >= 3
    order = sorted(range(48), key=lambda k: (-shapes[k][1], -shapes[k][0]))
    assert order != list(range(48))   # the launch order is not the staging order
    assert all(t.shape[1] ** 2 * t.shape[0] <= 2e8 for t in tasks)


def test_entry_rejects_what_it_cannot_take():
    ok = np.zeros((2, 3), np.uint8)
    for bad in (np.zeros((2, 0), np.uint8), np.zeros((0, 3), np.uint8), np.full((2, 3), 22, np.uint8)):
        with pytest.raises(SdError, match=r'\(-3\)'):
            api.r2p_weights([ok, bad])
    (f, e), = api.r2p_weights([ok])
    assert f.shape == (3, 20) and e.shape == (3,)
