"""GPU: sd_sw_set_shared_start (sd_sw.hip: k_gate_rev, k_pair_keys, devRunScore; sd_sw_pk.h: the start-row form of the aligned
kernel).  With the switch on the narrow start-position tasks of a query of 129 .. 768 rows run as suffixes of the query's one
profile, four tasks of a query per wavefront; everything a caller sees stays the same bytes.  On the constructed pairs of
tests/revgen.py (chains that begin at the first, second and last row of a lane, in the first and in one of the last lanes, one
column, the periodic queries that need the row mask), of tests/scgen.py and of tests/nfgen.py: records, flags and backtrace
pool against the switch-off call of the same process and against the oracle's rows (the golden rows of the reference where the
fixtures hold them), and the launch counts of the sw_score* scopes against the restated routing (revgen.tasks_on;
tests/test_sw_shared_start.py checks the scheme and that restatement on the CPU)."""
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

import nfgen
import revgen
import scgen
from test_gpu_sw_narrow_final import _merged, _same
from test_gpu_sw_score_classes import _check

pytestmark = pytest.mark.gpu
FIELDS6 = ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'btLen')


def _oracle_rows(oracle, seqs, pq, pt, wrl, comp_bias, eval_thr, cov_thr, db):
    """a scgen.Rows-like table of the oracle's records, modes 0, 1, 2"""
    n = len(pq)
    res = np.zeros((3, n, len(scgen.FIELDS)), np.int64)
    word = np.zeros(n, np.int64)
    bt = []
    for x in range(n):
        for mode in scgen.MODES:
            o = oracle.sw_align(seqs[int(pq[x])], seqs[int(pt[x])], db, sw_mode=mode, eval_thr=eval_thr, cov_thr=cov_thr, comp_bias=comp_bias)
            res[mode][x] = [o[f] for f in scgen.FIELDS]
            word[x] = o['flags'] & 1
        bt.append(o['backtrace'])
    return SimpleNamespace(res=res, word=word, bt=bt, wrl=wrl, n=n, qlen=np.array([len(seqs[int(q)]) for q in pq]),
                           tlen=np.array([len(seqs[int(t)]) for t in pt]))


def _check_oracle(rows, names, mode, idx, res, pool, what):
    for x, r in zip(idx, res):
        want = tuple(int(rows.res[mode][x][scgen.FIELDS.index(f)]) for f in FIELDS6)
        got = tuple(int(r[f]) for f in FIELDS6)
        assert got == want, (what, mode, names[x], got, want)
        assert (int(r['flags']) & 1) == int(rows.word[x]), (what, mode, names[x])
        if mode == 2 and want[5] > 0:
            bt = pool[int(r['btOffset']):int(r['btOffset']) + int(r['btLen'])].tobytes().decode()
            assert bt == rows.bt[x] and int(r['identical']) == int(rows.res[2][x][scgen.FIELDS.index('identical')]), (what, names[x])


@pytest.fixture(scope='module')
def sh(gpu, host, oracle):
    """one sequence set: scgen's and nfgen's sequences with their composition bias, revgen's with a bias of zero"""
    ga, gb = scgen.golden(), nfgen.golden()
    la, lb = scgen.build()[0], nfgen.build()[0]
    lc, rp = revgen.build()
    assert scgen.digest(la) == str(ga['digest']) and scgen.digest(lb) == str(gb['digest'])
    seqs = [oracle.map_sequence(s) for s in la + lb + lc]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    resid = np.concatenate(seqs)
    bias, _, _ = host.comp_bias(resid, off)
    first_rev = len(la) + len(lb)
    bias[int(off[first_rev]):] = 0
    ss = gpu.seqset(resid, off, bias)
    mat, _, _ = host.matrix(0)
    gold = scgen.Rows(_merged(ga, gb))
    assert gold.n == 279 + 6 and gold.wrl == 32767 // (max(int(mat[i]) for i in range(441)) + int(bias.max()))
    db = int(ga['db_residues'])
    assert db == revgen.DB_RESIDUES
    pq = np.concatenate([ga['q'], gb['q'] + len(la), np.array([p['q'] for p in rp]) + first_rev]).astype(np.uint32)
    pt = np.concatenate([ga['t'], gb['t'] + len(la), np.array([p['t'] for p in rp]) + first_rev]).astype(np.uint32)
    names = [str(s) for s in ga['name']] + [str(s) for s in gb['name']] + [p['name'] for p in rp]
    rev = list(range(gold.n, gold.n + len(rp)))
    default = [gpu.sw_params(mat, db, sw_mode=m) for m in scgen.MODES]
    opened = [gpu.sw_params(mat, db, sw_mode=m, eval_thr=revgen.EVAL_THR, cov_thr=revgen.COV_THR) for m in scgen.MODES]
    # the oracle's rows of revgen's pairs: gates open, and with the default gates (most of them stop at the coverage gate)
    r_open = _oracle_rows(oracle, seqs, pq[rev], pt[rev], gold.wrl, False, revgen.EVAL_THR, revgen.COV_THR, db)
    r_def = _oracle_rows(oracle, seqs, pq[rev], pt[rev], gold.wrl, False, 10.0, 0.8, db)
    return SimpleNamespace(seqs=seqs, ss=ss, mat=mat, gold=gold, pq=pq, pt=pt, names=names, rev=rev, default=default, opened=opened,
                           r_open=r_open, r_def=r_def, db=db, first_rev=first_rev, g=ga, prow=scgen.Rows(ga, 'p_'), rp=rp)


def _merge_rows(a, b):
    """a scgen.Rows-like table of a's pairs followed by b's (what the restated routing reads)"""
    return SimpleNamespace(res=np.concatenate([np.asarray(a.res, np.int64), np.asarray(b.res, np.int64)], axis=1), wrl=a.wrl, n=a.n + b.n,
                           word=np.concatenate([a.word, b.word]), qlen=np.concatenate([a.qlen, b.qlen]), tlen=np.concatenate([a.tlen, b.tlen]))


def _align(gpu, on, par, qs, ts, pq, pt, narrow_final=False):
    """one call with the switches as given: what sw_align returns and {scope: launches} of the score scopes"""
    gpu.set_shared_start(on)
    gpu.set_narrow_final(narrow_final)
    gpu.profile()
    try:
        out = gpu.sw_align(par, qs, ts, pq, pt)
        rep = gpu.profile_report()
    finally:
        gpu.profile(False)
        gpu.set_shared_start(False)
        gpu.set_narrow_final(False)
    return out, Counter({k: int(v[1]) for k, v in rep.items() if k.startswith('sw_score')})


def _start_scopes(launches):
    return sorted(s for s in launches if s.startswith('sw_score_pk.s_seg'))


@pytest.mark.parametrize('mode', scgen.MODES)
def test_constructed_pairs(gpu, sh, mode):
    """revgen's pairs with the gates open: all in one call, each alone (a lone task and an EMPTY pair), the late and the whole
    task of a query together (two chains that begin 24 and more lanes apart in the halves of one register), three, four and five
    tasks of one query (odd and even runs of pairs).  On equals off byte for byte and the oracle's rows; the start-position
    launches are the start form's alone, one per class"""
    rows, names = sh.r_open, [p['name'] for p in sh.rp]
    assert not rows.word.any()          # (no byte score saturates: every start-position task is a narrow one)
    assert (rows.res[1][:, 1] >= 0).all() and (rows.res[1][:, 0] > 0).all()      # (and every pair has one, the one-column pairs too)
    x = {n: i for i, n in enumerate(names)}
    subsets = [list(range(rows.n)), list(range(rows.n))[::-1]] + [[i] for i in range(rows.n)]
    for rt in (5, 12, 24):
        late, whole, m0, m1, ml = (x['%s_RT%d' % (w, rt)] for w in ('late', 'whole', 'mod0', 'mod1', 'modlast'))
        subsets += [[late, whole], [whole, late], [late, whole, m0], [m1, late, whole, m0], [late, m0, m1, ml, whole], [late, late, late]]
    subsets += [[x['tan_RT24'], x['late_RT24']], [x['per_RT12'], x['whole_RT12'], x['onecol_RT12']]]
    for idx in subsets:
        pq, pt = sh.pq[sh.rev][idx], sh.pt[sh.rev][idx]
        off, l_off = _align(gpu, False, sh.opened[mode], sh.ss, sh.ss, pq, pt)
        on, l_on = _align(gpu, True, sh.opened[mode], sh.ss, sh.ss, pq, pt)
        assert _same(on, off), (mode, [names[i] for i in idx])
        _check_oracle(rows, names, mode, idx, on[0], on[1], 'shared start')
        _check_oracle(rows, names, mode, idx, off[0], off[1], 'switch off')
        assert l_off == revgen.launches_on(rows, idx, mode, shared_start=False) and not _start_scopes(l_off), (idx, l_off)
        assert l_on == revgen.launches_on(rows, idx, mode), (idx, l_on)
        if mode == 0:
            assert l_on == l_off
        else:   # every pair of revgen is in range: what the call launches beyond its forward pass are start-form scopes, one per class
            fwd = revgen.launches_on(rows, idx, 0)
            extra = l_on - fwd
            assert sorted(extra) == _start_scopes(l_on) == sorted(set('sw_score_pk.s_seg%d' % sh.rp[i]['rt'] for i in idx)), (idx, l_on)
            assert all(v == 1 for v in extra.values())


@pytest.mark.parametrize('narrow_final', [False, True])
@pytest.mark.parametrize('mode', scgen.MODES)
def test_all_pairs_default_gates(gpu, sh, mode, narrow_final):
    """every pair of scgen, nfgen and revgen once, shuffled, in one call with the default gates: on equals off, the golden rows of
    the reference (scgen, nfgen) and the oracle's (revgen); the launches are the restated routing's -- start-form scopes for
    exactly the classes that hold a narrow start-position task of a query in range, the per-task scopes for the others.  With
    sd_sw_set_narrow_final on as well, the pair at 1022 is one of them"""
    rows = _merge_rows(sh.gold, sh.r_def)
    order = scgen.shuffled(rows.n, seed=12)
    off, l_off = _align(gpu, False, sh.default[mode], sh.ss, sh.ss, sh.pq[order], sh.pt[order], narrow_final)
    on, l_on = _align(gpu, True, sh.default[mode], sh.ss, sh.ss, sh.pq[order], sh.pt[order], narrow_final)
    assert _same(on, off)
    for out, what in ((on, 'shared start'), (off, 'switch off')):
        k_gold = [k for k, x in enumerate(order) if x < sh.gold.n]
        k_rev = [k for k, x in enumerate(order) if x >= sh.gold.n]
        _check(sh.gold, sh.names, mode, [order[k] for k in k_gold], out[0][k_gold], out[1], what)
        _check_oracle(sh.r_def, sh.names[sh.gold.n:], mode, [order[k] - sh.gold.n for k in k_rev], out[0][k_rev], out[1], what)
    assert l_off == revgen.launches_on(rows, order, mode, narrow_final, shared_start=False) and not _start_scopes(l_off), (mode, l_off)
    assert l_on == revgen.launches_on(rows, order, mode, narrow_final), (mode, l_on)
    moved = [x for x in order if revgen.in_range(rows, x, mode, narrow_final)]
    assert _start_scopes(l_on) == sorted(set('sw_score_pk.s_seg%d' % ((int(rows.qlen[x]) + 31) // 32) for x in moved))
    if mode:
        assert len(_start_scopes(l_on)) == 20 and len(moved) > 60
        if narrow_final:
            assert sh.names.index('nf32_1022') in moved and sh.names.index('nf64_1022') in moved
            assert sh.names.index('nf32_1023') not in moved


def test_all_pairs_gates_open(gpu, oracle, sh):
    """the same call with the gates open, modes 1 and 2: every pair with a score has a start-position task, most of scgen's
    end early in their queries.  On equals off and the oracle's rows for every pair"""
    n = sh.gold.n
    seqs_rows = _oracle_rows(oracle, sh.seqs, sh.pq[:n], sh.pt[:n], sh.gold.wrl, True, revgen.EVAL_THR, revgen.COV_THR, sh.db)
    rows = _merge_rows(seqs_rows, sh.r_open)
    rows.bt = seqs_rows.bt + sh.r_open.bt
    order = scgen.shuffled(rows.n, seed=13)
    for mode in (1, 2):
        off, l_off = _align(gpu, False, sh.opened[mode], sh.ss, sh.ss, sh.pq[order], sh.pt[order])
        on, l_on = _align(gpu, True, sh.opened[mode], sh.ss, sh.ss, sh.pq[order], sh.pt[order])
        assert _same(on, off)
        _check_oracle(rows, sh.names, mode, order, on[0], on[1], 'gates open')
        assert l_off == revgen.launches_on(rows, order, mode, shared_start=False), (mode, l_off)
        assert l_on == revgen.launches_on(rows, order, mode), (mode, l_on)
        assert len(_start_scopes(l_on)) == 20


def test_profile_twins(gpu, host, oracle, sh):
    """profile queries: the eight twins of scgen (golden rows, default gates) and revgen's five queries as profiles against their
    targets (the oracle's rows, gates open) -- on equals off, and the launches are the restated routing's"""
    mat = np.array([sh.mat[i] for i in range(441)], np.int32)

    def profiles(seqs, seeds):
        recs, boff = [], [0]
        for s, seed in zip(seqs, seeds):
            recs.append(scgen.profile_record(s, mat, seed))
            boff.append(boff[-1] + len(recs[-1]))
        prof = host.map_profiles(b''.join(recs), np.array(boff, np.uint64))
        return prof, gpu.profileset(prof['letters'], prof['offsets'], prof['aln']), 32767 // int(prof['aln'].max())

    twins = [int(x) for x in sh.g['p_twin']]
    prof, qs, wrl = profiles([sh.seqs[int(sh.pq[x])] for x in twins], [1000 + x for x in twins])
    assert sh.prow.wrl == wrl
    names = [sh.names[x] + ' as a profile' for x in twins]
    idx = list(range(len(twins)))
    moved_twins = set()
    for mode in scgen.MODES:
        pq, pt = np.array(idx, np.uint32), sh.pt[twins]
        off, l_off = _align(gpu, False, sh.default[mode], qs, sh.ss, pq, pt)
        on, l_on = _align(gpu, True, sh.default[mode], qs, sh.ss, pq, pt)
        assert _same(on, off)
        _check(sh.prow, names, mode, idx, on[0], on[1], 'profile twins')
        assert l_off == sh.prow.launches(idx, mode) and l_on == revgen.launches_on(sh.prow, idx, mode), (mode, l_on)
        moved_twins |= set(_start_scopes(l_on))
    assert len(moved_twins) >= 2
    # revgen's queries as profiles
    rq = sorted(set(p['q'] for p in sh.rp))
    prof, qs, wrl = profiles([sh.seqs[sh.first_rev + q] for q in rq], [5000 + q for q in rq])
    po = prof['offsets']
    pairs = [(rq.index(p['q']), p) for p in sh.rp]
    pq = np.array([k for k, _ in pairs], np.uint32)
    pt = np.array([sh.first_rev + p['t'] for _, p in pairs], np.uint32)
    rnames = [p['name'] + ' as a profile' for _, p in pairs]
    res = np.zeros((3, len(pairs), len(scgen.FIELDS)), np.int64)
    word, bts = np.zeros(len(pairs), np.int64), []
    for x, (k, p) in enumerate(pairs):
        a, b = int(po[k]), int(po[k + 1])
        for mode in scgen.MODES:
            o = oracle.sw_align_profile(prof['letters'][a:b], prof['aln'][a:b], sh.seqs[sh.first_rev + p['t']], sh.db, sw_mode=mode,
                                        eval_thr=revgen.EVAL_THR, cov_thr=revgen.COV_THR)
            res[mode][x] = [o[f] for f in scgen.FIELDS]
            word[x] = o['flags'] & 1
        bts.append(o['backtrace'])
    rows = SimpleNamespace(res=res, word=word, bt=bts, wrl=wrl, n=len(pairs), qlen=np.array([int(po[k + 1] - po[k]) for k, _ in pairs]),
                           tlen=np.array([len(sh.seqs[int(t)]) for t in pt]))
    moved = 0
    for mode in scgen.MODES:
        off, l_off = _align(gpu, False, sh.opened[mode], qs, sh.ss, pq, pt)
        on, l_on = _align(gpu, True, sh.opened[mode], qs, sh.ss, pq, pt)
        assert _same(on, off)
        _check_oracle(rows, rnames, mode, list(range(rows.n)), on[0], on[1], 'profiles of revgen')
        assert l_off == revgen.launches_on(rows, range(rows.n), mode, shared_start=False), (mode, l_off)
        assert l_on == revgen.launches_on(rows, range(rows.n), mode), (mode, l_on)
        moved += len(_start_scopes(l_on))
    assert moved == 2 * 3


def test_tasks_out_of_range_keep_their_path(gpu, host, sh, monkeypatch):
    """with the switch on nothing changes for a query set of 2^17 sequences (tasks are not paired by query there) nor for a call
    on the int32 kernel: the launches are the switch-off call's, no start-form scope among them, the records the same bytes"""
    rows, names = sh.r_open, [p['name'] for p in sh.rp]
    idx = list(range(rows.n))
    pad = 1 << 17
    seqs = [np.array([x % 20], np.uint8) for x in range(pad)] + sh.seqs[sh.first_rev:]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    big = gpu.seqset(np.concatenate(seqs), off, np.zeros(int(off[-1]), np.int8))
    pq = np.array([p['q'] for p in sh.rp], np.uint32) + np.uint32(pad)
    pt = np.array([p['t'] for p in sh.rp], np.uint32) + np.uint32(pad)
    off_, l_off = _align(gpu, False, sh.opened[2], big, big, pq, pt)
    on, l_on = _align(gpu, True, sh.opened[2], big, big, pq, pt)
    assert _same(on, off_) and l_on == l_off == revgen.launches_on(rows, idx, 2, shared=False) and not _start_scopes(l_on), l_on
    _check_oracle(rows, names, 2, idx, on[0], on[1], 'unpaired')
    monkeypatch.setenv('SD_SW_INT32', '1')
    pq, pt = sh.pq[sh.rev], sh.pt[sh.rev]
    off_, l_off = _align(gpu, False, sh.opened[2], sh.ss, sh.ss, pq, pt)
    on, l_on = _align(gpu, True, sh.opened[2], sh.ss, sh.ss, pq, pt)
    assert _same(on, off_) and l_on == l_off and all(s.startswith('sw_score.') for s in l_on), l_on
    _check_oracle(rows, names, 2, idx, on[0], on[1], 'int32')


def test_streaming_search_switches_it_on(gpu, host, monkeypatch):
    """sd_search_stream turns the switch on for its alignment lanes (SD_SW_SHARED_START=0 keeps it off): every returned array is
    the same either way, and with the default the lanes launch start-form kernels"""
    from spacedust_amd.pipeline import ClusterSearch, SetDB
    from spacedust_amd.synth import make_proteomes
    ps = make_proteomes(5, genes_per_proteome=400, n_families=60, seed=77)
    db = SetDB.from_proteomes(ps)
    outs, stats = {}, {}
    for env in ('0', None):
        if env is None:
            monkeypatch.delenv('SD_SW_SHARED_START', raising=False)
        else:
            monkeypatch.setenv('SD_SW_SHARED_START', env)
        cs = ClusterSearch(gpu, host, db, max_seqs=300, bin_size=2, filter_self_match=True)
        for c in cs.contexts:
            c.profile()
        outs[env] = cs.search(db, same_db=True, chunk_queries=500)
        st = Counter()
        for c in cs.contexts:
            for k, v in c.profile_report().items():
                if k.startswith('sw_score_pk.'):
                    st[k] += int(v[1])
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
    print(dict(stats[None]))
    assert not _start_scopes(stats['0']) and len(_start_scopes(stats[None])) >= 3
