"""GPU: sd_sw_set_group16 (sd_sw.hip: pairsPerWave, k_pair_leaders, launchScorePkAligned; sd_sw_pk.h: the 16-lane form of the
aligned kernel).  With the switch on the paired forward tasks of 129 .. 448 query rows (a_seg5 .. a_seg14; the row code would allow
a_seg15 and a_seg16, 481 and 512 rows below, which were measured no faster and stay on 32 lanes) run four task pairs of a query per wavefront, a lane holding twice the rows; everything a caller sees stays the same bytes, and so do the scopes and the
launches per scope.  Every case: records and pool with the switch on against the switch-off call of the same process, both
against the oracle's rows (the reference's golden rows where the fixtures hold them), and the launch counters on against off.

The constructed grid uses the smallest shapes at which the form can go wrong: query rows at the first row, the last row and the
middle of classes 5, 6, 9, 10, 15 and 16 (2 RT = 2 and 0 mod 4; 129 rows leave the last three lanes with padding rows alone), the
last row on 16 lanes and the first beyond (448 | 449), 513 rows (a class that could not take the form) and 128 (general kernel); target columns around the 16-column chunk reloads, shorter than the ramp,
odd step counts; runs of 1 .. 17 tasks per (class, query), i.e. EMPTY pairs in every slot of the eight and an odd last task."""
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

import flgen
import revgen
import scgen
from tbgen import _mutate, _rnd
from test_gpu_sw_narrow_final import _same
from test_gpu_sw_score_classes import _check
from test_gpu_sw_shared_start import _check_oracle, _merge_rows, _oracle_rows, sh  # noqa: F401  (sh: the module fixture of scgen + nfgen + revgen)

pytestmark = pytest.mark.gpu

Q_ROWS = (129, 160, 161, 288, 320, 481, 512, 513, 128, 448, 449)
T_COLS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 300)
RUNS = (1, 2, 3, 7, 8, 9, 16, 17)
MOTIF = 'WCHYFPMWCHYF'
COLD_Q, COLD_T = 'DEGKNQRS', 'FILMVWY'
GO, GE = 11, 1


def _align(gpu, on, par, qs, ts, pq, pt, narrow_final=False, shared_start=False):
    """one call with the switches as given: what sw_align returns and {scope: launches} of the score scopes"""
    gpu.set_group16(on)
    gpu.set_narrow_final(narrow_final)
    gpu.set_shared_start(shared_start)
    gpu.profile()
    try:
        out = gpu.sw_align(par, qs, ts, pq, pt)
        rep = gpu.profile_report()
    finally:
        gpu.profile(False)
        gpu.set_group16(False)
        gpu.set_narrow_final(False)
        gpu.set_shared_start(False)
    return out, Counter({k: int(v[1]) for k, v in rep.items() if k.startswith('sw_score')})


def _both(gpu, par, qs, ts, pq, pt, **kw):
    """(on, off, launches): the two calls give the same bytes and the same launch counters"""
    off, l_off = _align(gpu, False, par, qs, ts, pq, pt, **kw)
    on, l_on = _align(gpu, True, par, qs, ts, pq, pt, **kw)
    assert _same(on, off), kw
    assert l_on == l_off, (l_on, l_off)
    return on, off, l_on


def _grid(seed=20261021):
    """(seqs, pairs, ties): per query of Q_ROWS and column count of T_COLS a target that ends with the query's last residues (the
    maximum in the last used lane, at the last column) and one with a fragment from the middle of the query that ends at the
    target's end or, for the long target, at column 16, 17, 32 or 33 ...; per query one homolog of 300 columns whose byte score
    saturates.  ties: see test_ties"""
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []

    def add(s):
        seqs.append(s)
        return len(seqs) - 1

    for x, n in enumerate(Q_ROWS):
        qs = _rnd(rng, n)
        q = add(qs)
        for tl in T_COLS:
            k = min(tl, 20)
            pairs.append(dict(name='end_%d_%d' % (n, tl), q=q, t=add(_rnd(rng, tl - k) + qs[n - k:])))
            k = min(tl, 36)
            p = int(rng.integers(0, n - k + 1))
            frag = _mutate(rng, qs[p:p + k], 0.15, keep=min(4, k // 3))
            lead = tl - k if tl < 300 else (48, 49, 64, 65, 80, 81, 37, 96, 97, 112, 113)[x] - k   # (the fragment's last column + 1)
            pairs.append(dict(name='mid_%d_%d' % (n, tl), q=q, t=add(_rnd(rng, lead) + frag + _rnd(rng, tl - k - lead))))
        pairs.append(dict(name='hom_%d_300' % n, q=q, t=add(_mutate(rng, (qs + _rnd(rng, 300))[:300], 0.12))))
    # ---- ties.  No composition bias, the query's filling letters from COLD_Q and the target's from COLD_T (no letter of the one
    # scores above 0 against a letter of the other): every copy of the unit scores exactly what the unit scores against itself
    def fill(alphabet, n):
        return ''.join(alphabet[i] for i in rng.integers(0, len(alphabet), n))

    u = _rnd(rng, 8) + MOTIF + _rnd(rng, 8)
    ties = {}
    # the unit twice in a query of 320 rows, 160 rows apart (20 rows per lane of 16, 10 per lane of 32): two lanes of one group
    q = add(fill(COLD_Q, 37) + u + fill(COLD_Q, 132) + u + fill(COLD_Q, 320 - 37 - 132 - 2 * len(u)))
    ties['rows'] = dict(q=q, t=add(fill(COLD_T, 9) + u + fill(COLD_T, 5)))
    ties['rows_columns'] = dict(q=q, t=add(fill(COLD_T, 5) + u + fill(COLD_T, 132) + u + fill(COLD_T, 5)))
    # the unit once in a query of 200 rows: twice in one target, and once in four targets of a run of eight tasks, at different columns
    q = add(fill(COLD_Q, 100) + u + fill(COLD_Q, 200 - 100 - len(u)))
    ties['columns'] = dict(q=q, t=add(fill(COLD_T, 3) + u + fill(COLD_T, 21) + u + fill(COLD_T, 7)))
    for k, (lead, tl) in enumerate(((2, 100), (31, 90), (40, 80), (17, 70))):
        ties['groups_%d' % k] = dict(q=q, t=add(fill(COLD_T, lead) + u + fill(COLD_T, tl - lead - len(u))))
        ties['groups_fill_%d' % k] = dict(q=q, t=add(fill(COLD_T, tl - 5)))
    return seqs, pairs, ties


@pytest.fixture(scope='module')
def grid(gpu, host, oracle):
    letters, pairs, ties = _grid()
    seqs = [oracle.map_sequence(s) for s in letters]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    ss = gpu.seqset(np.concatenate(seqs), off, np.zeros(int(off[-1]), np.int8))
    mat, _, _ = host.matrix(0)
    wrl = 32767 // max(int(mat[i]) for i in range(441))
    db = revgen.DB_RESIDUES
    par = [gpu.sw_params(mat, db, sw_mode=m, eval_thr=revgen.EVAL_THR, cov_thr=revgen.COV_THR) for m in scgen.MODES]
    pq = np.array([p['q'] for p in pairs] + [p['q'] for p in ties.values()], np.uint32)
    pt = np.array([p['t'] for p in pairs] + [p['t'] for p in ties.values()], np.uint32)
    names = [p['name'] for p in pairs] + ['tie_' + k for k in ties]
    rows = _oracle_rows(oracle, seqs, pq, pt, wrl, False, revgen.EVAL_THR, revgen.COV_THR, db)
    return SimpleNamespace(seqs=seqs, ss=ss, mat=mat, par=par, pq=pq, pt=pt, names=names, rows=rows, n_grid=len(pairs), db=db,
                           tie={k: len(pairs) + i for i, k in enumerate(ties)}, by_q={n: [x for x, p in enumerate(pairs) if p['name'].split('_')[1] == str(n)]
                                                                                     for n in Q_ROWS})


def _call(gpu, grid, mode, idx, **kw):
    on, off, launches = _both(gpu, grid.par[mode], grid.ss, grid.ss, grid.pq[idx], grid.pt[idx], **kw)
    _check_oracle(grid.rows, grid.names, mode, idx, on[0], on[1], 'group16')
    _check_oracle(grid.rows, grid.names, mode, idx, off[0], off[1], 'switch off')
    assert launches == revgen.launches_on(grid.rows, idx, mode, kw.get('narrow_final', False), shared_start=kw.get('shared_start', False)), (mode, launches)
    return launches


@pytest.mark.parametrize('mode', scgen.MODES)
def test_grid(gpu, grid, mode):
    """every query against every target of its own, shuffled, in one call (runs of 23 tasks: twelve pairs, no EMPTY one) and the
    queries of the classes one by one"""
    assert (grid.rows.res[0][:grid.n_grid, 0] > 0).sum() > grid.n_grid - 12    # (one- and two-column targets may score nothing)
    order = [x for x in scgen.shuffled(grid.n_grid, seed=21)]
    launches = _call(gpu, grid, mode, order)
    assert set(launches) >= set('sw_score_pk.a_seg%d' % rt for rt in (5, 6, 9, 10, 14, 15, 16, 17)) | {'sw_score_pk.rt4x32'}, launches
    for n in Q_ROWS:
        _call(gpu, grid, mode, grid.by_q[n])


def test_hom_saturates_and_both_final_paths(gpu, grid):
    """the homologs saturate the byte score (rerun wide, or final from the narrow pass with sd_sw_set_narrow_final on): the 16-lane
    form's result is then the record's"""
    idx = [x for x in range(grid.n_grid) if grid.names[x].startswith('hom_')]
    assert all(grid.rows.word[x] for x in idx if grid.rows.qlen[x] > 128)
    assert any(grid.rows.res[0][x][0] < 1023 for x in idx) and any(grid.rows.res[0][x][0] >= 1023 for x in idx)
    for nf_ in (False, True):
        for mode in scgen.MODES:
            _call(gpu, grid, mode, idx + grid.by_q[320][:5], narrow_final=nf_)


@pytest.mark.parametrize('shift', range(8))
def test_runs(gpu, grid, shift):
    """runs of 1, 2, 3, 7, 8, 9, 16 and 17 tasks per (class, query), several queries of a class (129 | 160 and 481 | 512 rows) in
    one shuffled call: EMPTY pairs in every slot, an odd last task, a lone task in a wavefront of eight; every run length meets
    every query in one of the eight cases"""
    rng = np.random.default_rng(40 + shift)
    idx = []
    for k, n in enumerate((129, 160, 161, 288, 320, 448, 481, 512, 513, 449)):
        r = RUNS[(k + shift) % len(RUNS)]
        mine = grid.by_q[n]
        idx += [mine[int(i)] for i in rng.permutation(len(mine))[:r]]
    idx += grid.by_q[128][:5]
    idx = [idx[int(i)] for i in rng.permutation(len(idx))]
    for mode in ((2,) if shift else scgen.MODES):
        _call(gpu, grid, mode, idx)
    _call(gpu, grid, 2, idx, narrow_final=True, shared_start=True)


def test_ties(gpu, oracle, grid):
    """the largest value wins, then the first column, then the smallest row.  The model (flgen.model_np, no bias) shows what is
    constructed: the maximum stands in two rows of one column that belong to two lanes of a 16-lane group (and of a 32-lane
    one); in two columns as well; in two columns of one row; and four tasks of a run of eight reach the same maximum at four
    different columns, so they sit in two groups of a wavefront at least"""
    mat = np.array([grid.mat[i] for i in range(441)], np.int64).reshape(21, 21)

    def cells(x):
        q, t = grid.seqs[int(grid.pq[x])], grid.seqs[int(grid.pt[x])]
        G = flgen.model_np(mat[:, q], t, GO, GE)[0]
        mx = int(G.max())
        assert (mx, flgen.best(G)[1], flgen.best(G)[2]) == tuple(int(grid.rows.res[0][x][i]) for i in (0, 4, 2))
        return mx, [(int(c), int(r)) for c, r in zip(*np.nonzero(G == mx))]

    cold = [[int(mat[a][b]) for a in oracle.map_sequence(COLD_Q)] for b in oracle.map_sequence(COLD_T)]
    assert max(max(r) for r in cold) <= 0
    x = grid.tie['rows']
    mx, at = cells(x)
    rows = sorted(r for c, r in at if c == at[0][0])
    assert len(rows) == 2 and rows[1] == rows[0] + 160 and rows[0] // 20 != rows[1] // 20 and not grid.rows.word[x]
    x2 = grid.tie['rows_columns']
    mx2, at2 = cells(x2)
    assert mx2 == mx and sorted(r for c, r in at2 if c == at2[0][0]) == rows and sorted(set(c for c, r in at2 if r == rows[0])) == [at2[0][0], at2[0][0] + 160]
    x3 = grid.tie['columns']
    mx3, at3 = cells(x3)
    assert mx3 == mx and len(set(c for c, r in at3 if r == at3[0][1])) == 2
    groups = [grid.tie['groups_%d' % k] for k in range(4)]
    fill = [grid.tie['groups_fill_%d' % k] for k in range(4)]
    got = [cells(g) for g in groups]
    assert set(m for m, _ in got) == {mx} and len(set(a[0][0] for _, a in got)) == 4 and all(cells(f)[0] < mx for f in fill)
    for mode in scgen.MODES:
        _call(gpu, grid, mode, [x])
        _call(gpu, grid, mode, [x2, x])
        _call(gpu, grid, mode, [x3])
        _call(gpu, grid, mode, groups + fill)
        _call(gpu, grid, mode, [x, x2, x3] + fill[:1] + groups[::-1] + grid.by_q[320][:6])


@pytest.mark.parametrize('narrow_final', [False, True])
@pytest.mark.parametrize('mode', scgen.MODES)
def test_all_pairs_all_switches(gpu, sh, mode, narrow_final):  # noqa: F811
    """every pair of scgen (tie_*, tie_rows_*, edge_255 | edge_254), nfgen (narrow scores of 1022, 1023 and beyond in a_seg10 and
    a_seg15) and revgen once, shuffled, default gates, with sd_sw_set_narrow_final off and on and sd_sw_set_shared_start on as
    the streaming search runs them: on equals off, the reference's golden rows and the oracle's, the restated routing's launches"""
    rows = _merge_rows(sh.gold, sh.r_def)
    order = scgen.shuffled(rows.n, seed=14)
    for name in ('edge_255', 'edge_254', 'tie_rows_n', 'nf32_1022', 'nf32_1023', 'nf64_1023'):
        assert name in sh.names
    assert sum(1 for s in sh.names if s.startswith('tie_')) >= 5
    for shared_start in (False, True):
        on, off, launches = _both(gpu, sh.default[mode], sh.ss, sh.ss, sh.pq[order], sh.pt[order], narrow_final=narrow_final, shared_start=shared_start)
        for out, what in ((on, 'group16'), (off, 'switch off')):
            k_gold = [k for k, x in enumerate(order) if x < sh.gold.n]
            k_rev = [k for k, x in enumerate(order) if x >= sh.gold.n]
            _check(sh.gold, sh.names, mode, [order[k] for k in k_gold], out[0][k_gold], out[1], what)
            _check_oracle(sh.r_def, sh.names[sh.gold.n:], mode, [order[k] - sh.gold.n for k in k_rev], out[0][k_rev], out[1], what)
        assert launches == revgen.launches_on(rows, order, mode, narrow_final, shared_start=shared_start), (mode, launches)
        assert all('sw_score_pk.a_seg%d' % rt in launches for rt in range(5, 25))


def test_profile_queries(gpu, host, oracle, grid):
    """profile queries (sd_profileset) through the same classes: the queries of 129, 161, 320 and 512 rows as profiles against
    their own targets, and runs of one and three tasks"""
    mat = np.array([grid.mat[i] for i in range(441)], np.int32)
    rows_q = (129, 161, 320, 512)
    first = {n: int(grid.pq[grid.by_q[n][0]]) for n in rows_q}
    recs, boff = [], [0]
    for n in rows_q:
        recs.append(scgen.profile_record(grid.seqs[first[n]], mat, 7000 + n))
        boff.append(boff[-1] + len(recs[-1]))
    prof = host.map_profiles(b''.join(recs), np.array(boff, np.uint64))
    qs = gpu.profileset(prof['letters'], prof['offsets'], prof['aln'])
    po = prof['offsets']
    pairs = [(k, x) for k, n in enumerate(rows_q) for x in grid.by_q[n]]
    pq = np.array([k for k, _ in pairs], np.uint32)
    pt = np.array([grid.pt[x] for _, x in pairs], np.uint32)
    names = [grid.names[x] + ' as a profile' for _, x in pairs]
    res = np.zeros((3, len(pairs), len(scgen.FIELDS)), np.int64)
    word, bts = np.zeros(len(pairs), np.int64), []
    for i, (k, x) in enumerate(pairs):
        a, b = int(po[k]), int(po[k + 1])
        for mode in scgen.MODES:
            o = oracle.sw_align_profile(prof['letters'][a:b], prof['aln'][a:b], grid.seqs[int(pt[i])], grid.db, sw_mode=mode,
                                        eval_thr=revgen.EVAL_THR, cov_thr=revgen.COV_THR)
            res[mode][i] = [o[f] for f in scgen.FIELDS]
            word[i] = o['flags'] & 1
        bts.append(o['backtrace'])
    rows = SimpleNamespace(res=res, word=word, bt=bts, wrl=32767 // int(prof['aln'].max()), n=len(pairs),
                           qlen=np.array([int(po[k + 1] - po[k]) for k, _ in pairs]), tlen=np.array([len(grid.seqs[int(t)]) for t in pt]))
    every = scgen.shuffled(rows.n, seed=31)
    by_k = {k: [i for i, (kk, _) in enumerate(pairs) if kk == k] for k in range(len(rows_q))}
    for idx in (every, by_k[0][:1] + by_k[2][:3] + by_k[3][:9]):
        for mode in scgen.MODES:
            on, off, launches = _both(gpu, grid.par[mode], qs, grid.ss, pq[idx], pt[idx])
            _check_oracle(rows, names, mode, idx, on[0], on[1], 'profiles, group16')
            _check_oracle(rows, names, mode, idx, off[0], off[1], 'profiles, switch off')
            assert launches == revgen.launches_on(rows, idx, mode, shared_start=False), (mode, launches)


def test_streaming_search_switches_it_on(gpu, host, monkeypatch):
    """sd_search_stream turns the switch on for its alignment lanes (SD_SW_GROUP16=0 keeps it off): every returned array and the
    launches per scope are the same either way"""
    from spacedust_amd.pipeline import ClusterSearch, SetDB
    from spacedust_amd.synth import make_proteomes
    ps = make_proteomes(4, genes_per_proteome=300, n_families=50, seed=78)
    db = SetDB.from_proteomes(ps)
    outs, stats = {}, {}
    for env in ('0', None):
        if env is None:
            monkeypatch.delenv('SD_SW_GROUP16', raising=False)
        else:
            monkeypatch.setenv('SD_SW_GROUP16', env)
        cs = ClusterSearch(gpu, host, db, max_seqs=300, bin_size=2, filter_self_match=True)
        for c in cs.contexts:
            c.profile()
        outs[env] = cs.search(db, same_db=True, chunk_queries=400)
        st = Counter()
        for c in cs.contexts:
            for k, v in c.profile_report().items():
                if k.startswith('sw_score'):
                    st[k] += int(v[1])
        stats[env] = st
        del cs
    a, b = outs['0'], outs[None]
    assert a['matched_hits'] > 500
    for k_ in ('entries', 'matched_hits', 'clusters', 'cluster_hits', 'aligned', 'accepted', 'prefilter_hits'):
        assert a[k_] == b[k_], k_
    for k_ in ('entry_q', 'entry_t', 'entry_off', 'hit_q', 'hit_t', 'hit_pval'):
        assert a[k_].tobytes() == b[k_].tobytes(), k_
    for k_ in ('cluster_of', 'rank', 'n_clusters', 'size', 'pCO', 'pMH'):
        assert a['cluster_out'][k_].tobytes() == b['cluster_out'][k_].tobytes(), k_
    assert stats['0'] == stats[None] and any(s.startswith('sw_score_pk.a_seg') for s in stats[None]), stats
