"""CPU: the premise of sd_sw_set_shared_start (sd_sw.hip, sd_sw_pk.h).

A start-position task is the reversed query cut at qEnd against the reversed target cut at tEnd.  The profile of the WHOLE
reversed query holds the task's rows from row j0 = qLen - 1 - qEnd on, so the task can run as a suffix of that one profile:
its chain begins in lane j0 // RT with a zero hand-off, the rows of that lane before j0 are masked, earlier lanes are left
out of the maximum, and the row is counted from j0 (revgen.start_row restates that layout without the kernel's number formats).
Checked here on the constructed pairs of tests/revgen.py against the oracle's striped pass over the CUT reversed profile, which
is what the per-task kernels compute; and the routing restated in revgen against the library's class table."""
from types import SimpleNamespace

import numpy as np
import pytest

import nfgen
import revgen
import scgen


@pytest.fixture(scope='module')
def rv(oracle, host):
    letters, pairs = revgen.build()
    seqs = [oracle.map_sequence(s) for s in letters]
    mat = np.asarray(oracle.matrix(0)[0], np.int64)
    prof, fwd = {}, []
    for p in pairs:
        q = p['q']
        if q not in prof:
            prof[q] = mat[:, seqs[q].astype(np.int64)]        # (revgen's sequences carry no composition bias: exact ties)
        fwd.append(oracle.sw_pass(prof[q], seqs[p['t']], 32))
    return SimpleNamespace(letters=letters, pairs=pairs, seqs=seqs, prof=prof, fwd=fwd)


def _cut_and_whole(rv, x):
    p = rv.pairs[x]
    score, t_end, q_end = rv.fwd[x]
    prof = rv.prof[p['q']]
    n = prof.shape[1]
    return (np.ascontiguousarray(prof[:, q_end::-1]), np.ascontiguousarray(prof[:, ::-1]), np.ascontiguousarray(rv.seqs[p['t']][t_end::-1]),
            n - 1 - q_end, (n + 31) // 32)


def test_pairs_are_what_they_are_meant_to_be(rv):
    """the forward pass ends where the construction says, and the chains begin where the cases need them: at the first, second
    and last row of a lane, in lane 0 (j0 = 0), in one of the last lanes, mid-lane for the periodic queries; one column, odd
    and even column counts"""
    seen, cols = set(), set()
    for x, p in enumerate(rv.pairs):
        score, t_end, q_end = rv.fwd[x]
        n, rt = len(rv.letters[p['q']]), p['rt']
        assert (n + 31) // 32 == rt and 129 <= n <= 768 and score > 0
        if p['e'] is not None:
            assert q_end == p['e'], (p['name'], q_end, p['e'])
        else:
            assert t_end == 0
        j0 = n - 1 - q_end
        seen.add((rt, p['name'].split('_')[0], q_end % rt))
        cols.add(1 if t_end == 0 else 2 + (t_end + 1) % 2)
        if p['name'].startswith('late'):
            assert j0 // rt >= 24
        if p['name'] == 'tan_RT24':
            assert j0 % rt >= revgen.TAN_U                      # the second U lies inside the lane the chain begins in
        if p['name'] == 'per_RT12':
            assert 0 < j0 % rt < rt - 1
    for rt, n in revgen.CLASSES:
        assert {(rt, 'mod0', 0), (rt, 'mod1', 1), (rt, 'modlast', rt - 1), (rt, 'whole', (n - 1) % rt)} <= seen
    assert cols == {1, 2, 3}


def test_start_rows_equal_the_cut_reverse_pass(oracle, rv):
    """every pair: the start-row scheme on the whole reversed profile gives the oracle's (score, column, row) of the cut reversed
    profile with the byte kernel's lane count, and its score is the forward score"""
    for x, p in enumerate(rv.pairs):
        cut, whole, t_rev, j0, rt = _cut_and_whole(rv, x)
        want = oracle.sw_pass(cut, t_rev, 32)
        assert want[0] == rv.fwd[x][0], p['name']
        assert nfgen.forward(cut, t_rev) == want, p['name']
        got = revgen.start_row(whole, rt, j0, t_rev)
        assert got == want, (p['name'], got, want)


def test_periodic_queries_need_the_cut(oracle, rv):
    """M M against M, and the tandem U U: the reverse pass over the UNCUT reversed query ends in another row than the task's (in
    the task's coordinates), so a kernel that scanned the shared profile from its first row would report another start; for
    the tandem pair the same holds inside the lane the chain begins in -- the scheme without its row mask is wrong, and
    neither the zero hand-off nor leaving out the earlier lanes repairs that"""
    names = [p['name'] for p in rv.pairs]
    for name in ('per_RT12', 'tan_RT24'):
        x = names.index(name)
        cut, whole, t_rev, j0, rt = _cut_and_whole(rv, x)
        want = oracle.sw_pass(cut, t_rev, 32)
        uncut = oracle.sw_pass(whole, t_rev, 32)
        assert uncut[0] == want[0] and (uncut[1], uncut[2] - j0) != (want[1], want[2]), (name, uncut, want, j0)
    x = names.index('tan_RT24')
    cut, whole, t_rev, j0, rt = _cut_and_whole(rv, x)
    want = oracle.sw_pass(cut, t_rev, 32)
    assert revgen.start_row(whole, rt, j0, t_rev, mask=False) != want
    assert revgen.start_row(whole, rt, j0, t_rev, mask=True) == want


def test_routing_restated_against_the_library(host):
    """the start form's classes in the library's table (kernel 3 of sd_selftest_score_class) are revgen.start_klass's for every
    query length, paired or not; outside 129 .. 768 rows and beyond 65 535 columns they are the narrow form's"""
    W = 2340
    for tl in (1, 300, 65535, 65536):
        for n in list(range(1, 1000)) + [2600]:
            for shared in (True, False):
                got = host.score_class(3, n, tl, shared, W)
                if 129 <= n <= 768 and tl <= 65535:
                    assert got == revgen.start_klass(n, 1, tl, W, False), (n, tl, got)
                    assert got[0] == 42 + (n + 31) // 32 - 5 and got[1] == 'sw_score_pk.s_seg%d' % ((n + 31) // 32)
                else:
                    assert got == host.score_class(0, n, tl, shared, W) == scgen.klass('fwd', n, shared, W, tl=tl), (n, tl, got)
    # a task is routed by its QUERY's length: 40 rows of a query of 760 run in s_seg24, the wide and int32 tasks as before
    assert revgen.start_klass(760, 40, 50, W, False)[1] == 'sw_score_pk.s_seg24'
    assert revgen.start_klass(760, 40, 50, W, True) == scgen.klass('start', 40, False, W, word=True, tl=50)
    assert revgen.start_klass(128, 40, 50, W, False) == scgen.klass('start', 40, False, W, tl=50)
    assert revgen.start_klass(769, 769, 50, W, False)[1] == 'sw_score_pk.rt8x64s2'
    assert revgen.start_klass(300, 300, 50, W, False, packed=False)[1] == 'sw_score.rt16'
    assert revgen.start_klass(300, 300, 50, W, False, shared_queries=False)[1] == 'sw_score_pk.a_seg10'
