"""CPU: the premise of sd_sw_set_narrow_final (sd_sw.hip).

The packed score kernels evaluate one recurrence whatever their layout (tests/test_sw_fl_equivalence.py) and choose the end
cell by one rule: the largest value, then the first column, then the smallest row.  The narrow kernels hold cells in int16
and report the column maximum through a row code that is exact below 1023.  So a narrow forward result below 1023 is what
the word-structure rerun of a pair whose byte score saturates computes, and the rerun is needed at 1023 and beyond only.
Checked here on the reference's own rows: the layout-free restatement (nfgen.forward) against the forward rows of every
constructed pair of tests/scgen.py and of the boundary pairs of tests/nfgen.py, the oracle's striped pass
with the byte and the word kernel's lane counts, the start-position pass, and the routing the switch leaves."""
from types import SimpleNamespace

import numpy as np
import pytest

import nfgen
import scgen


def _load(oracle, host, letters, g):
    assert scgen.digest(letters) == str(g['digest'])
    seqs = [oracle.map_sequence(s) for s in letters]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    bias, _, _ = host.comp_bias(np.concatenate(seqs), off)
    bias = [bias[int(off[i]):int(off[i + 1])].astype(np.int64) for i in range(len(seqs))]
    return SimpleNamespace(g=g, rows=scgen.Rows(g), seqs=seqs, bias=bias, names=[str(s) for s in g['name']], pq=g['q'], pt=g['t'])


@pytest.fixture(scope='module')
def sets(oracle, host):
    """the constructed pairs of scgen and of nfgen with their golden rows, and per pair (2 348 rows the longest) the forward
    result of the restatement, computed once"""
    mat = np.asarray(oracle.matrix(0)[0], np.int64)
    out = []
    for letters, g in ((scgen.build()[0], scgen.golden()), (nfgen.build()[0], nfgen.golden())):
        s = _load(oracle, host, letters, g)
        s.prof, s.fwd = {}, {}
        for x in range(s.rows.n):
            q = int(s.pq[x])
            if q not in s.prof:
                s.prof[q] = mat[:, s.seqs[q].astype(np.int64)] + s.bias[q][None, :]
            s.fwd[x] = nfgen.forward(s.prof[q], s.seqs[int(s.pt[x])])
        out.append(s)
    return out


def _golden_forward(s, x):
    r = dict(zip(scgen.FIELDS, (int(v) for v in s.rows.res[0][x])))
    return r['score'], r['tEnd'], r['qEnd']


def test_restatement_gives_the_reference_forward_rows(sets):
    """mode 0 rows (score, tEnd, qEnd) of every pair, 2 348 rows the longest: the restatement equals them for every pair below 1023
    -- none left out -- and, being unsaturated, for every other pair as well"""
    sc, nf = sets
    assert len(sc.fwd) == sc.rows.n == 279 and len(nf.fwd) == nf.rows.n == 6
    below = word_below = 0
    for s in sets:
        for x, got in s.fwd.items():
            want = _golden_forward(s, x)
            if want[0] < nfgen.NARROW_EXACT:
                below += 1
                word_below += int(s.rows.word[x])
            assert got == want, (s.names[x], got, want)
    assert below >= 200 and word_below == 37 + 2, (below, word_below)


def test_striped_pass_is_the_same_with_32_and_16_lanes(oracle, sets):
    """every pair with the word flag: oracle.sw_pass (the restated striped kernel, unsaturated) with the byte kernel's 32 and the
    word kernel's 16 lanes gives one result, the restatement's; the start-position pass over the reversed prefixes up to the
    end cell has the forward score as its maximum with either lane count, so no cell of it leaves the narrow kernels' range
    when the forward score is below 1023"""
    n_word = 0
    for s in sets:
        for x, fwd in s.fwd.items():
            if not s.rows.word[x]:
                continue
            n_word += 1
            prof, t = s.prof[int(s.pq[x])], s.seqs[int(s.pt[x])]
            a, b = oracle.sw_pass(prof, t, 32), oracle.sw_pass(prof, t, 16)
            assert a == b == fwd, (s.names[x], a, b, fwd)
            score, t_end, q_end = fwd
            rprof, rt = np.ascontiguousarray(prof[:, q_end::-1]), np.ascontiguousarray(t[t_end::-1])
            ra, rb = oracle.sw_pass(rprof, rt, 32), oracle.sw_pass(rprof, rt, 16)
            assert ra == rb and ra[0] == score == nfgen.forward(rprof, rt)[0], (s.names[x], ra, rb, score)
    assert n_word >= 80


def test_boundary_pairs_have_their_scores(sets):
    """the pairs of nfgen: 1022, 1023 and 1024 exactly, the word flag set, in all three modes, aligned end to end in the classes
    they are meant for"""
    _, nf = sets
    letters, pairs = nfgen.build()
    assert [p['name'] for p in pairs] == nf.names
    assert sorted(len(letters[p['q']]) for p in pairs) == [300] * 3 + [450] * 3
    for x, p in enumerate(pairs):
        assert int(nf.rows.word[x]) == 1
        for mode in scgen.MODES:
            assert int(nf.rows.res[mode][x][0]) == p['want']
        n = len(letters[p['q']])
        r = dict(zip(scgen.FIELDS, (int(v) for v in nf.rows.res[2][x])))
        assert (r['qStart'], r['qEnd'], r['btLen']) == (0, n - 1, n)
        scopes = [s for _, _, s in nfgen.tasks_on(nf.rows, x, 2)]
        lanes = 'x32' if n == 300 else 'x64'
        if p['want'] >= nfgen.NARROW_EXACT:
            assert len(scopes) == 3 and scopes[0].startswith('sw_score_pk.a_seg') and all(s.startswith('sw_score_pk.w_') and s.endswith(lanes) for s in scopes[1:])
        else:
            assert len(scopes) == 2 and not any('.w_' in s for s in scopes)
            assert scopes[1] == ('sw_score_pk.a_seg10' if n == 300 else 'sw_score_pk.rt8x64')


def test_routing_with_the_switch_on(sets):
    """the class table with word := score >= 1023: the word pairs below 1023 of scgen's rows leave the wide classes -- their
    start-position tasks reach the unshared narrow scopes of every kernel family -- and the pairs at 1023 and beyond keep
    reaching the wide scopes and the int32 kernel beyond wideRowLimit; a pair without the word flag is routed as before"""
    sc, _ = sets
    rows = sc.rows
    low = [x for x in range(rows.n) if rows.word[x] and rows.res[0][x][0] < nfgen.NARROW_EXACT]
    high = [x for x in range(rows.n) if rows.word[x] and rows.res[0][x][0] >= nfgen.NARROW_EXACT]
    assert len(low) == 37 and len(high) >= 40
    for x in range(rows.n):
        if not rows.word[x]:
            for mode in scgen.MODES:
                assert nfgen.tasks_on(rows, x, mode) == [(p, c, s) for p, c, s, _ in rows.tasks(x, mode)]
    on = [tk for x in low for tk in nfgen.tasks_on(rows, x, 2)]
    assert not any('.w_' in s or s.startswith('sw_score.') for _, _, s in on)
    start = set(s.split('.', 1)[1] for p, _, s in on if p == 2)
    want = set(['rt4x32', 'a_seg12', 'rt8x64', 'rt10x64', 'rt12x64', 'rt8x64s2', 'rt8x64s3'] + ['a_seg%d' % rt for rt in range(5, 11)])
    assert start >= want, sorted(want - start)
    off = set(s for x in low for _, _, s, _ in rows.tasks(x, 2))
    assert sum(1 for s in off if '.w_' in s) >= 10           # (what these pairs launch with the switch off)
    hi = set(s for x in high for _, _, s in nfgen.tasks_on(rows, x, 2))
    assert sum(1 for s in hi if '.w_' in s) >= 10 and 'sw_score.rt32' in hi
    for x in high:
        for mode in scgen.MODES:
            assert nfgen.tasks_on(rows, x, mode) == [(p, c, s) for p, c, s, _ in rows.tasks(x, mode)]
    full = list(range(rows.n))
    for mode in scgen.MODES:
        a, b = nfgen.launches_on(rows, full, mode), rows.launches(full, mode)
        assert all(a[s] <= b[s] for s in b if '.w_' in s) and sum(a.values()) <= sum(b.values())
