"""GPU: the packed score kernels without the lane-structure F chain (sd_sw_pk.h) on the F-then-E pairs of tests/flgen.py --
pairs that tests/test_sw_fl_equivalence.py shows to use the removed term in the forward and in the start-position pass --
through Context.sw_align in modes 0 and 2.  Every record (score, starts, ends, backtrace length, word flag) and every
backtrace equals oracle.sw_align's, whose score passes carry the lane structure.  The profile scopes show that the calls reach
every kernel family: the general kernel of 32 lanes, the aligned kernel shared and unshared, below and beyond 12 rows per lane,
the 64-lane kernel, the strips with their boundary buffer, and the wide kernels."""
import re
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

import flgen
import scgen

pytestmark = pytest.mark.gpu
MODES = (0, 2)
FIELDS = ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'btLen')


@pytest.fixture(scope='module')
def fl(gpu, host, oracle):
    letters, pairs = flgen.fte_pairs()
    seqs = [oracle.map_sequence(s) for s in letters]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    resid = np.concatenate(seqs)
    bias, _, _ = host.comp_bias(resid, off)
    mat, _, _ = host.matrix(0)
    db = int(off[-1])
    pq, pt = np.array([p[1] for p in pairs], np.uint32), np.array([p[2] for p in pairs], np.uint32)
    exp = {m: [oracle.sw_align(seqs[q], seqs[t], db, sw_mode=m, cov_thr=0.0) for q, t in zip(pq, pt)] for m in MODES}
    # the same queries as profiles: their matrix rows plus noise (the recipe of the profile twins of tests/scgen.py)
    queries = sorted(set(int(q) for q in pq))
    recs, boff = [], [0]
    for q in queries:
        recs.append(scgen.profile_record(seqs[q], np.array([mat[i] for i in range(441)], np.int32), 500 + q))
        boff.append(boff[-1] + len(recs[-1]))
    prof = host.map_profiles(b''.join(recs), np.array(boff, np.uint64))
    po = prof['offsets']
    ppq = np.array([queries.index(int(q)) for q in pq], np.uint32)
    pexp = {m: [oracle.sw_align_profile(prof['letters'][int(po[q]):int(po[q + 1])], prof['aln'][int(po[q]):int(po[q + 1])], seqs[t], db,
                                        sw_mode=m, cov_thr=0.0) for q, t in zip(ppq, pt)] for m in MODES}
    return SimpleNamespace(names=[p[0] for p in pairs], pq=pq, pt=pt, exp=exp, ppq=ppq, pexp=pexp,
                           ss=gpu.seqset(resid, off, bias), ps=gpu.profileset(prof['letters'], prof['offsets'], prof['aln']),
                           par={m: gpu.sw_params(mat, db, sw_mode=m, cov_thr=0.0) for m in MODES})


def _align(gpu, par, qs, ts, pq, pt):
    gpu.profile()
    res, pool = gpu.sw_align(par, qs, ts, pq, pt)
    rep = gpu.profile_report()
    gpu.profile(False)
    return res, pool, Counter({k: int(v[1]) for k, v in rep.items() if k.startswith('sw_score')})


def _check(names, idx, res, pool, exp, mode, what):
    for x, r in zip(idx, res):
        o = exp[x]
        assert tuple(int(r[f]) for f in FIELDS) == tuple(o[f] for f in FIELDS), (what, mode, names[x], r, o)
        assert (int(r['flags']) & 1) == (o['flags'] & 1), (what, mode, names[x])
        if mode == 2:
            assert o['btLen'] > 0 and int(r['identical']) == o['identical'], (what, names[x])
            assert pool[int(r['btOffset']):int(r['btOffset']) + int(r['btLen'])].tobytes().decode() == o['backtrace'], (what, names[x])


def _families(scopes):
    """the kernel families among profile scope names"""
    fam = set()
    for s in scopes:
        m = re.fullmatch(r'sw_score_pk\.(w_)?(a_seg(\d+)|rt(\d+)x(32|64)(s\w)?)', s)
        assert m, s   # (no int32 kernel on these pairs)
        if m.group(1):
            fam.add('wide strips' if m.group(6) else 'wide x' + m.group(5))
        elif m.group(3):
            fam.add('aligned <= 12' if int(m.group(3)) <= 12 else 'aligned > 12')
        else:
            fam.add('strips' if m.group(6) else 'general x' + m.group(5))
    return fam


@pytest.mark.parametrize('mode', MODES)
def test_all_pairs_in_one_call(gpu, fl, mode):
    """every pair in one call: queries with one and with two targets, so shared profiles with full and with half-empty pairs"""
    idx = list(range(len(fl.pq)))
    res, pool, launches = _align(gpu, fl.par[mode], fl.ss, fl.ss, fl.pq, fl.pt)
    print(mode, dict(launches))
    _check(fl.names, idx, res, pool, fl.exp[mode], mode, 'together')
    want = {'general x32', 'aligned <= 12', 'aligned > 12', 'strips', 'wide x32', 'wide x64', 'wide strips'}
    if mode == 2:
        want.add('general x64')   # start positions of the queries beyond 384 rows
    assert _families(launches) >= want, launches


@pytest.mark.parametrize('mode', MODES)
def test_lone_and_odd_task_counts(gpu, fl, mode):
    """one call per pair (a lone task: the second half of its lane group idles on the same rows) and one call of three tasks
    per pair (an odd count: a full pair and a lone task of the same query)"""
    seen = Counter()
    for x in range(len(fl.pq)):
        for idx in ([x], [x, x, x]):
            res, pool, launches = _align(gpu, fl.par[mode], fl.ss, fl.ss, fl.pq[idx], fl.pt[idx])
            _check(fl.names, idx, res, pool, fl.exp[mode], mode, 'lone' if len(idx) == 1 else 'odd')
            seen.update(launches)
            fam = _families(launches)
            name = fl.names[x].split('/')[0]
            if name.startswith('wide'):
                assert any(f.startswith('wide') for f in fam), (name, launches)
            elif name.startswith('strips'):
                assert 'strips' in fam, (name, launches)
            elif name.startswith('a_seg'):
                assert 'aligned <= 12' in fam or 'aligned > 12' in fam, (name, launches)
                # start positions run unshared: the aligned kernel up to 384 rows, the 64-lane kernel beyond
                if mode == 2 and name == 'a_seg19':
                    assert 'general x64' in fam, launches
                elif mode == 2:
                    assert fam == {'aligned <= 12'} and sum(launches.values()) == 2, launches
            else:
                assert fam == {'general x32'}, (name, launches)
    print(mode, dict(seen))


@pytest.mark.parametrize('mode', MODES)
def test_profile_queries(gpu, fl, mode):
    """the same shapes with the queries as profiles, through the profile entry (sd_profileset_create)"""
    idx = list(range(len(fl.ppq)))
    res, pool, launches = _align(gpu, fl.par[mode], fl.ps, fl.ss, fl.ppq, fl.pt)
    print(mode, dict(launches))
    _check(fl.names, idx, res, pool, fl.pexp[mode], mode, 'profiles')
    fam = _families(launches)
    assert {'general x32', 'aligned <= 12', 'aligned > 12', 'strips'} <= fam and any(f.startswith('wide') for f in fam), launches
    for x in (0, len(idx) - 1):   # and alone
        res, pool, _ = _align(gpu, fl.par[mode], fl.ps, fl.ss, fl.ppq[[x]], fl.pt[[x]])
        _check(fl.names, [x], res, pool, fl.pexp[mode], mode, 'profile alone')
