"""GPU: every instantiation of the Smith-Waterman score kernels (sd_sw_pk.h, SCORE_CLASSES / devRunScore in sd_sw.hip) in every pass that
reaches it, on the constructed pairs of tests/scgen.py, through the device orchestration (Context.sw_align).  Every record is
compared exactly with the rows that the REAL reference produced (tests/golden/score_classes.npz, alignment modes 0, 1, 2),
and the launch counts of the sw_score* profile scopes equal what the restated class table derives from those rows: one
launch per pass and non-empty class, none anywhere else (tests/test_score_classes.py proves on the CPU that these calls
reach all 63 instantiations, each with odd and even task counts)."""
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

import scgen

pytestmark = pytest.mark.gpu
EVAL_THR = 10.0


def _set(gpu, host, seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    resid = np.concatenate(seqs)
    sw_bias, _, _ = host.comp_bias(resid, off)
    return gpu.seqset(resid, off, sw_bias), int(sw_bias.max())


@pytest.fixture(scope='module')
def sc(gpu, host, oracle):
    g = scgen.golden()
    letters, pairs = scgen.build()
    assert scgen.digest(letters) == str(g['digest'])
    seqs = [oracle.map_sequence(s) for s in letters]
    mat, _, _ = host.matrix(0)
    ss, max_bias = _set(gpu, host, seqs)
    rows = scgen.Rows(g)
    assert rows.wrl == 32767 // (max(int(mat[i]) for i in range(441)) + max_bias)
    par = [gpu.sw_params(mat, int(g['db_residues']), sw_mode=m) for m in scgen.MODES]   # (default gates: E-value 10, query coverage 0.8)
    return SimpleNamespace(g=g, rows=rows, prow=scgen.Rows(g, 'p_'), seqs=seqs, mat=mat, ss=ss, par=par, names=[str(s) for s in g['name']],
                           pq=g['q'].astype(np.uint32), pt=g['t'].astype(np.uint32))


def _align(gpu, par, qs, ts, pq, pt):
    """one call: the records, the backtrace pool and {scope: launches} of the score scopes"""
    gpu.profile()
    res, pool = gpu.sw_align(par, qs, ts, pq, pt)
    rep = gpu.profile_report()
    gpu.profile(False)
    return res, pool, Counter({k: int(v[1]) for k, v in rep.items() if k.startswith('sw_score')})


def _check(rows, names, mode, idx, res, pool, what):
    for x, r in zip(idx, res):
        w = dict(zip(scgen.FIELDS, (int(v) for v in rows.res[mode][x])))
        got = tuple(int(r[f]) for f in ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'btLen'))
        assert got == tuple(w[f] for f in ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'btLen')), (what, mode, names[x], got, w)
        assert (int(r['flags']) & 1) == int(rows.word[x]), (what, mode, names[x])
        if rows.evalue[mode][x] <= 2.0 * EVAL_THR:
            assert float(r['evalue']) == float(rows.evalue[mode][x]), (what, mode, names[x], r['evalue'], rows.evalue[mode][x])
        if mode == 2 and w['btLen'] > 0:
            bt = pool[int(r['btOffset']):int(r['btOffset']) + int(r['btLen'])].tobytes().decode()
            assert bt == rows.bt[x] and int(r['identical']) == w['identical'], (what, names[x])
        elif mode == 2:
            assert rows.bt[x] == ''


def _groups(gpu, sc, mode, odd, packed=True):
    groups = sc.rows.groups(mode, True, packed)
    for key, members in groups.items():
        idx = scgen.padded(members, odd)
        res, pool, launches = _align(gpu, sc.par[mode], sc.ss, sc.ss, sc.pq[idx], sc.pt[idx])
        print([s for _, _, s in key], [sc.names[x] for x in members], len(idx), dict(launches))
        _check(sc.rows, sc.names, mode, idx, res, pool, key)
        assert launches == Counter(s for _, _, s in key) == sc.rows.launches(idx, mode, True, packed), (key, launches)
    return groups


@pytest.mark.parametrize('count', ['odd', 'even'])
@pytest.mark.parametrize('mode', scgen.MODES)
def test_class_groups(gpu, sc, mode, count):
    """one call per group of pairs that share their class in every pass, padded to an odd count of at least three tasks or to an
    even one (a repeated pair is a second task of its query: lone tasks, padded EMPTY pairs, full wavefronts): the records
    against the reference's rows, and exactly one launch per pass and class of the group"""
    groups = _groups(gpu, sc, mode, count == 'odd')
    assert len(groups) >= (45 if mode == 0 else 80)


def test_all_pairs_shuffled_in_one_call(gpu, sc):
    """every pair once, in random order, modes 0 and 2: the sort by class, the pairing by query across classes (runs of one to six
    tasks of a query) and the three devRunScore rounds with every class populated"""
    order = scgen.shuffled(sc.rows.n)
    for mode in (0, 2):
        res, pool, launches = _align(gpu, sc.par[mode], sc.ss, sc.ss, sc.pq[order], sc.pt[order])
        _check(sc.rows, sc.names, mode, order, res, pool, 'shuffled')
        assert launches == sc.rows.launches(order, mode), (mode, launches)
    # (mode 2: every packed scope -- 20 aligned, 7 general narrow, 14 wide -- and the int32 kernel beyond wideRowLimit, rerun and start positions)
    assert len(launches) == 20 + 7 + 14 + 1 and launches['sw_score.rt32'] == 2


def test_forward_pass_without_shared_profiles(gpu, host, sc):
    """the same sequences behind 2^17 one-residue sequences: a query set of that size has no room in the pairing key, so the
    forward and the rerun pass launch the unshared instantiations (aligned up to 384 rows, rt8x64 / rt10x64 / rt12x64 beyond,
    every wide one).  The records equal the same golden rows"""
    pad = 1 << 17
    big, max_bias = _set(gpu, host, [np.array([x % 20], np.uint8) for x in range(pad)] + sc.seqs)
    assert max_bias == 3
    order = scgen.shuffled(sc.rows.n, seed=6)
    pq, pt = sc.pq[order] + np.uint32(pad), sc.pt[order] + np.uint32(pad)
    for mode in (0, 1):
        res, pool, launches = _align(gpu, sc.par[mode], big, big, pq, pt)
        _check(sc.rows, sc.names, mode, order, res, pool, 'unshared')
        assert launches == sc.rows.launches(order, mode, shared=False), (mode, launches)
        assert not any(k.startswith('sw_score_pk.a_seg') and int(k[17:]) > 12 for k in launches)
        assert all(launches['sw_score_pk.' + k] == (8 if mode else 4) for k in ('rt8x64', 'rt10x64', 'rt12x64'))   # four classes of 32 rows each: forward, and start positions


def test_int32_classes_in_the_device_orchestration(gpu, sc, monkeypatch):
    """SD_SW_INT32=1, mode 1: only the four int32 scopes appear, all four in the forward and in the start-position pass"""
    monkeypatch.setenv('SD_SW_INT32', '1')
    order = scgen.shuffled(sc.rows.n, seed=7)
    res, pool, launches = _align(gpu, sc.par[1], sc.ss, sc.ss, sc.pq[order], sc.pt[order])
    _check(sc.rows, sc.names, 1, order, res, pool, 'int32')
    assert launches == Counter({'sw_score.' + k: 3 for k in scgen.I32_NAMES}) == sc.rows.launches(order, 1, packed=False), launches
    seen = set((p, s) for x in order for p, _, s, _ in sc.rows.tasks(x, 1, packed=False))
    assert seen == set((p, 'sw_score.' + k) for p in (0, 1, 2) for k in scgen.I32_NAMES)
    for odd in (True, False):
        _groups(gpu, sc, 1, odd, packed=False)


def test_profile_queries_per_kernel_family(gpu, host, sc):
    """the profile twins (the query as a profile: its matrix rows plus noise) against the reference's rows for them
    (set_query_profile), in the scopes of their plain twins: aligned shared and unshared, the general narrow kernels, the strips,
    the wide kernels of 32 and of 64 lanes"""
    twins = [int(x) for x in sc.g['p_twin']]
    recs, boff = [], [0]
    for x in twins:
        recs.append(scgen.profile_record(sc.seqs[int(sc.pq[x])], np.array([sc.mat[i] for i in range(441)], np.int32), 1000 + x))
        boff.append(boff[-1] + len(recs[-1]))
    prof = host.map_profiles(b''.join(recs), np.array(boff, np.uint64))
    assert sc.prow.wrl == 32767 // int(prof['aln'].max())
    qs = gpu.profileset(prof['letters'], prof['offsets'], prof['aln'])
    names = [sc.names[x] + ' as a profile' for x in twins]
    for mode in scgen.MODES:
        for k, x in enumerate(twins):
            idx = [k] * 3
            res, pool, launches = _align(gpu, sc.par[mode], qs, sc.ss, np.array(idx, np.uint32), sc.pt[[x] * 3])
            _check(sc.prow, names, mode, idx, res, pool, 'profile')
            assert launches == sc.prow.launches(idx, mode) == sc.rows.launches([x], mode), (names[k], mode, launches)
        idx = list(range(len(twins)))
        res, pool, launches = _align(gpu, sc.par[mode], qs, sc.ss, np.array(idx, np.uint32), sc.pt[twins])
        _check(sc.prow, names, mode, idx, res, pool, 'profiles together')
        assert launches == sc.prow.launches(idx, mode), (mode, launches)
