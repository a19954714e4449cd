"""GPU: sd_sw_set_narrow_final (sd_sw.hip: k_pre_word, k_gate_word, k_gate_rev).  With the switch on a pair whose byte score
saturates is rerun on the wide kernels only when the narrow forward pass reports 1023 or was skipped; everything a caller sees
stays the same bytes.  On the constructed pairs of tests/scgen.py and the boundary pairs of tests/nfgen.py (forward scores
1022, 1023, 1024 in a 32-lane and a 64-lane class): records and backtrace pool against the switch-off call of the same process
and against the rows of the REAL reference, and the launch counts of the sw_score* scopes against the restated routing
(nfgen.tasks_on; tests/test_sw_narrow_final.py proves on the CPU which scopes it reaches)."""
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

import nfgen
import scgen
from test_gpu_sw_score_classes import EVAL_THR, _check, _set  # noqa: F401

pytestmark = pytest.mark.gpu
NO_DIAG = 0x8000


def _merged(a, b):
    """the golden rows of scgen's pairs and of nfgen's as one table (the layout scgen.Rows reads)"""
    g = {k: np.concatenate([a[k], b[k]], axis=1) for k in ('res', 'evalue')}
    g.update({k: np.concatenate([a[k], b[k]]) for k in ('word', 'qlen', 'tlen', 'start_nocov', 'name')})
    g.update({k: np.array(str(a[k]) + '\n' + str(b[k])) for k in ('bt', 'bt_nocov')})
    g['wide_row_limit'] = a['wide_row_limit']
    return g


@pytest.fixture(scope='module')
def nf(gpu, host, oracle):
    ga, gb = scgen.golden(), nfgen.golden()
    la, lb = scgen.build()[0], nfgen.build()[0]
    assert scgen.digest(la) == str(ga['digest']) and scgen.digest(lb) == str(gb['digest'])
    seqs = [oracle.map_sequence(s) for s in la + lb]
    mat, _, _ = host.matrix(0)
    ss, max_bias = _set(gpu, host, seqs)
    rows = scgen.Rows(_merged(ga, gb))
    assert rows.n == 279 + 6 and rows.wrl == 32767 // (max(int(mat[i]) for i in range(441)) + max_bias)
    par = [gpu.sw_params(mat, int(ga['db_residues']), sw_mode=m) for m in scgen.MODES]
    assert int(ga['db_residues']) == int(gb['db_residues'])
    names = [str(s) for s in ga['name']] + [str(s) for s in gb['name']]
    pq = np.concatenate([ga['q'], gb['q'] + len(la)]).astype(np.uint32)
    pt = np.concatenate([ga['t'], gb['t'] + len(la)]).astype(np.uint32)
    score = rows.res[0][:, 0]
    low = [x for x in range(279) if rows.word[x] and score[x] < nfgen.NARROW_EXACT]
    assert len(low) == 37
    return SimpleNamespace(g=ga, rows=rows, prow=scgen.Rows(ga, 'p_'), seqs=seqs, mat=mat, ss=ss, par=par, names=names, pq=pq, pt=pt,
                           low=low, x={n: i for i, n in enumerate(names)})


def _align(gpu, on, par, qs, ts, pq, pt, **kw):
    """one call with the switch as given: what sw_align returns and {scope: launches} of the score scopes"""
    gpu.set_narrow_final(on)
    gpu.profile()
    try:
        out = gpu.sw_align(par, qs, ts, pq, pt, **kw)
        rep = gpu.profile_report()
    finally:
        gpu.profile(False)
        gpu.set_narrow_final(False)
    assert ('stat.sw_word_pairs' in rep) == bool(on)
    if on:
        assert rep['stat.sw_word_pairs'][0] == rep['stat.sw_word_wide'][0] + rep['stat.sw_word_narrow_final'][0]
    return out, Counter({k: int(v[1]) for k, v in rep.items() if k.startswith('sw_score')}), rep


def _same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _wide(launches):
    return sorted(s for s in launches if '.w_' in s or s.startswith('sw_score.'))


@pytest.mark.parametrize('mode', scgen.MODES)
def test_all_pairs_switch_on_against_switch_off(gpu, nf, mode):
    """every pair once, shuffled, in one call: records and pool are the bytes of the switch-off call and the reference's rows, bit 0
    of the flags is the golden word flag, and the launches are the restated routing's -- wide scopes only for classes that
    hold a pair at 1023 or beyond; with the switch off they are scgen's, as before"""
    order = scgen.shuffled(nf.rows.n, seed=8)
    off, l_off, _ = _align(gpu, False, nf.par[mode], nf.ss, nf.ss, nf.pq[order], nf.pt[order])
    on, l_on, rep = _align(gpu, True, nf.par[mode], nf.ss, nf.ss, nf.pq[order], nf.pt[order])
    assert _same(on, off)
    _check(nf.rows, nf.names, mode, order, on[0], on[1], 'narrow final')
    _check(nf.rows, nf.names, mode, order, off[0], off[1], 'switch off')
    assert l_off == nf.rows.launches(order, mode), (mode, l_off)
    assert l_on == nfgen.launches_on(nf.rows, order, mode), (mode, l_on)
    high = [x for x in order if nf.rows.word[x] and nf.rows.res[0][x][0] >= nfgen.NARROW_EXACT]
    assert set(_wide(l_on)) == set(s for x in high for _, _, s in nfgen.tasks_on(nf.rows, x, mode) if '.w_' in s or s.startswith('sw_score.'))
    assert sum(l_on.values()) < sum(l_off.values())
    n_word = int(nf.rows.word.sum())
    assert rep['stat.sw_word_pairs'][0] == n_word and rep['stat.sw_word_wide'][0] == len(high) and len(high) == n_word - 37 - 2


@pytest.mark.parametrize('mode', scgen.MODES)
def test_word_pairs_below_1023_launch_no_wide_kernel(gpu, nf, mode):
    """the 37 pairs of scgen whose byte score saturates below 1023, alone in a call: no wide and no int32 scope in any mode (with the
    switch off: a dozen of them), the reference's rows all the same"""
    idx = nf.low
    on, l_on, rep = _align(gpu, True, nf.par[mode], nf.ss, nf.ss, nf.pq[idx], nf.pt[idx])
    _check(nf.rows, nf.names, mode, idx, on[0], on[1], 'below 1023')
    assert _wide(l_on) == [] and l_on == nfgen.launches_on(nf.rows, idx, mode), l_on
    assert rep['stat.sw_word_pairs'][0] == rep['stat.sw_word_narrow_final'][0] == len(idx)
    off, l_off, _ = _align(gpu, False, nf.par[mode], nf.ss, nf.ss, nf.pq[idx], nf.pt[idx])
    assert _same(on, off) and len(_wide(l_off)) >= 10 and l_off == nf.rows.launches(idx, mode)


@pytest.mark.parametrize('lanes', ['nf32', 'nf64'])
def test_boundary_scores(gpu, nf, lanes):
    """1022, 1023 and 1024: each pair alone, and the three targets of the query in one call -- two of them share the halves of a
    register, a saturating half beside an exact one.  1022 is final after the narrow pass, 1023 and 1024 are rerun wide, in the
    32-lane (nf32) and the 64-lane (nf64) kernels; the reference's rows in every case"""
    three = [nf.x['%s_%d' % (lanes, w)] for w in (1022, 1023, 1024)]
    for mode in scgen.MODES:
        for idx in [[x] for x in three] + [three, three[::-1], [three[0], three[2]], [three[2], three[0], three[0]]]:
            on, l_on, rep = _align(gpu, True, nf.par[mode], nf.ss, nf.ss, nf.pq[idx], nf.pt[idx])
            _check(nf.rows, nf.names, mode, idx, on[0], on[1], ('boundary', idx))
            assert l_on == nfgen.launches_on(nf.rows, idx, mode), (idx, mode, l_on)
            wide = _wide(l_on)
            if idx == [three[0]]:
                assert wide == []
            else:
                assert wide == ['sw_score_pk.w_' + ('rt10x32' if lanes == 'nf32' else 'rt8x64')] and l_on[wide[0]] == (2 if mode else 1)
            assert rep['stat.sw_word_narrow_final'][0] == sum(1 for x in idx if x == three[0])
        off, l_off, _ = _align(gpu, False, nf.par[mode], nf.ss, nf.ss, nf.pq[three], nf.pt[three])
        on, _, _ = _align(gpu, True, nf.par[mode], nf.ss, nf.ss, nf.pq[three], nf.pt[three])
        assert _same(on, off) and l_off == nf.rows.launches(three, mode)


def _true_diag(rows, x):
    """the diagonal (query position - target position, as 16 bits) the pair's alignment starts on, from the reference's path
    without the coverage gate; no path: no hint"""
    bt = rows.bt_nocov[x]
    if not bt:
        return NO_DIAG
    t_end = int(rows.res[0][x][scgen.FIELDS.index('tEnd')])
    t_start = t_end + 1 - sum(1 for ch in bt if ch != 'I')
    return (int(rows.start_nocov[x]) - t_start) & 0xFFFF


def test_diagonals_change_no_record(gpu, nf):
    """sd_sw_align_batch_compact_diag with the switch on: the prefilter's diagonal only decides whether a pair skips the narrow pass
    (its ungapped stretch proves 1023), never a record -- true diagonals, none (0x8000) and absurd ones against the call
    without diagonals, switch on and off"""
    order = scgen.shuffled(nf.rows.n, seed=9)
    pq, pt = nf.pq[order], nf.pt[order]
    base, l_base, _ = _align(gpu, True, nf.par[2], nf.ss, nf.ss, pq, pt, compact=True)
    off, _, _ = _align(gpu, False, nf.par[2], nf.ss, nf.ss, pq, pt, compact=True)
    reported = [k for k, x in enumerate(order) if nf.rows.res[2][x][scgen.FIELDS.index('btLen')] > 0]   # (passed every gate)
    assert _same(base, off) and [int(k) for k in base[0]] == reported and len(reported) > 50
    rng = np.random.default_rng(10)
    true = np.array([_true_diag(nf.rows, x) for x in order], np.uint16)
    for what, diag in (('true', true), ('none', np.full(len(order), NO_DIAG, np.uint16)),
                       ('absurd', rng.integers(0, 1 << 16, len(order)).astype(np.uint16)),
                       ('shifted', (true.astype(np.int64) + 3).astype(np.uint16))):
        got, l_got, rep = _align(gpu, True, nf.par[2], nf.ss, nf.ss, pq, pt, compact=True, diag=diag)
        assert _same(got, base), what
        assert rep['stat.sw_word_pairs'][0] == int(nf.rows.word.sum())
        if what == 'none':
            assert l_got == l_base
        off_d, _, _ = _align(gpu, False, nf.par[2], nf.ss, nf.ss, pq, pt, compact=True, diag=diag)
        assert _same(off_d, base), what
    # the skip-pass-1 case: an ungapped diagonal far above 1023 -- no narrow forward scope, the rerun and the start positions wide
    x = nf.x['wrl_flat']
    d = np.array([_true_diag(nf.rows, x)], np.uint16)
    assert int(d[0]) == scgen.WRL_LEN - 300
    got, l_got, rep = _align(gpu, True, nf.par[2], nf.ss, nf.ss, nf.pq[[x]], nf.pt[[x]], compact=True, diag=d)
    want = Counter(s for _, _, s in nfgen.tasks_on(nf.rows, x, 2, pre_word=True))
    assert l_got == want and all('.w_' in s for s in l_got) and sum(l_got.values()) == 2, l_got   # (the rerun and the start positions)
    assert rep['stat.sw_word_wide'][0] == 1
    plain, l_plain, _ = _align(gpu, False, nf.par[2], nf.ss, nf.ss, nf.pq[[x]], nf.pt[[x]])
    assert _same(got, _align(gpu, False, nf.par[2], nf.ss, nf.ss, nf.pq[[x]], nf.pt[[x]], compact=True)[0])
    _check(nf.rows, nf.names, 2, [x], plain[0], plain[1], 'wrl_flat')
    assert sum(l_plain.values()) == 3
    # a homolog below 1023 with its true diagonal: narrow from end to end
    x = nf.x['hom_243']
    d = np.array([_true_diag(nf.rows, x)], np.uint16)
    assert int(d[0]) != NO_DIAG and nf.rows.word[x] and nf.rows.res[0][x][0] < nfgen.NARROW_EXACT
    got, l_got, rep = _align(gpu, True, nf.par[2], nf.ss, nf.ss, nf.pq[[x]], nf.pt[[x]], compact=True, diag=d)
    assert _wide(l_got) == [] and l_got == nfgen.launches_on(nf.rows, [x], 2), l_got
    assert len(got[0]) == 1 and _same(got, _align(gpu, False, nf.par[2], nf.ss, nf.ss, nf.pq[[x]], nf.pt[[x]], compact=True)[0])
    _check(nf.rows, nf.names, 2, [x], got[1], got[2], 'hom_243')


def test_profile_twins(gpu, host, nf):
    """the eight profile queries of scgen (set_query_profile rows of the reference): switch on against switch off, identical
    records; the launches are what the restated routing derives from the p_ rows"""
    twins = [int(x) for x in nf.g['p_twin']]
    recs, boff = [], [0]
    for x in twins:
        recs.append(scgen.profile_record(nf.seqs[int(nf.pq[x])], np.array([nf.mat[i] for i in range(441)], np.int32), 1000 + x))
        boff.append(boff[-1] + len(recs[-1]))
    prof = host.map_profiles(b''.join(recs), np.array(boff, np.uint64))
    assert nf.prow.wrl == 32767 // int(prof['aln'].max())
    qs = gpu.profileset(prof['letters'], prof['offsets'], prof['aln'])
    names = [nf.names[x] + ' as a profile' for x in twins]
    idx = list(range(len(twins)))
    n_low = sum(1 for k in idx if nf.prow.word[k] and nf.prow.res[0][k][0] < nfgen.NARROW_EXACT)
    assert n_low >= 1
    for mode in scgen.MODES:
        for sub in [idx] + [[k] for k in idx]:
            pq, pt = np.array(sub, np.uint32), nf.pt[[twins[k] for k in sub]]
            off, l_off, _ = _align(gpu, False, nf.par[mode], qs, nf.ss, pq, pt)
            on, l_on, rep = _align(gpu, True, nf.par[mode], qs, nf.ss, pq, pt)
            assert _same(on, off)
            _check(nf.prow, names, mode, sub, on[0], on[1], 'profiles')
            assert l_off == nf.prow.launches(sub, mode) and l_on == nfgen.launches_on(nf.prow, sub, mode), (mode, sub, l_on)
            assert rep['stat.sw_word_narrow_final'][0] == sum(1 for k in sub if nf.prow.word[k] and nf.prow.res[0][k][0] < nfgen.NARROW_EXACT)


def test_streaming_search_switches_it_on(gpu, host, monkeypatch):
    """sd_search_stream turns the switch on for its alignment lanes (SD_SW_NARROW_FINAL=0 keeps it off): every returned array is
    the same either way, and with the default the lanes count word pairs that the narrow pass answered"""
    from spacedust_amd.pipeline import ClusterSearch, SetDB
    from spacedust_amd.synth import make_proteomes
    ps = make_proteomes(5, genes_per_proteome=400, n_families=60, seed=77)
    db = SetDB.from_proteomes(ps)
    outs, stats = {}, {}
    for env in ('0', None):
        if env is None:
            monkeypatch.delenv('SD_SW_NARROW_FINAL', raising=False)
        else:
            monkeypatch.setenv('SD_SW_NARROW_FINAL', env)
        cs = ClusterSearch(gpu, host, db, max_seqs=300, bin_size=2, filter_self_match=True)
        for c in cs.contexts:
            c.profile()
        outs[env] = cs.search(db, same_db=True, chunk_queries=500)
        st = Counter()
        for c in cs.contexts:
            for k, v in c.profile_report().items():
                if k.startswith('stat.sw_word'):
                    st[k] += int(v[0])
        stats[env] = st
        del cs
    a, b = outs['0'], outs[None]
    assert a['matched_hits'] > 1000 and a['clusters'] > 20
    for k_ in ('entries', 'matched_hits', 'clusters', 'cluster_hits', 'aligned', 'accepted', 'prefilter_hits'):
        assert a[k_] == b[k_], k_
    for k_ in ('entry_q', 'entry_t', 'entry_off', 'hit_q', 'hit_t', 'hit_pval'):
        assert a[k_].tobytes() == b[k_].tobytes(), k_
    for k_ in ('cluster_of', 'rank', 'n_clusters', 'size', 'pCO', 'pMH'):
        assert a['cluster_out'][k_].tobytes() == b['cluster_out'][k_].tobytes(), k_
    assert not stats['0']
    st = stats[None]
    print(dict(st))
    assert st['stat.sw_word_pairs'] == st['stat.sw_word_wide'] + st['stat.sw_word_narrow_final'] and st['stat.sw_word_narrow_final'] > 0
