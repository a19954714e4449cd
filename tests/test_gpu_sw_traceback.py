"""GPU: every traceback task class of sd_sw.hip, its boundaries and the band doubling inside and between classes, on the
constructed pairs of tests/tbgen.py.  Every record is compared exactly with the rows that the REAL reference produced
(tests/golden/tb_classes.npz) and with the oracle; the launch counts of the sw_traceback.* profile scopes say that the
pairs ran through the classes they were built for (tests/test_tb_classes.py checks the construction on the CPU)."""
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

import tbgen

pytestmark = pytest.mark.gpu
FIELDS = ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'identical', 'btLen')


@pytest.fixture(scope='module')
def tb(gpu, host, oracle):
    g = tbgen.golden()
    n = len(g['name'])
    seqs = []
    for q, t in zip(g['q'], g['t']):
        seqs += [oracle.map_sequence(str(q)), oracle.map_sequence(str(t))]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    resid = np.concatenate(seqs)
    sw_bias, _, _ = host.comp_bias(resid, off)
    mat, _, _ = host.matrix(0)
    db = int(g['db_residues'])
    want = []
    for x in range(n):
        o = oracle.sw_align(seqs[2 * x], seqs[2 * x + 1], db, cov_thr=0.0)
        row = tuple(int(v) for v in g['res'][x]) + (str(g['bt'][x]), float(g['evalue'][x]))
        assert tuple(o[k] for k in FIELDS) + (o['backtrace'], o['evalue']) == row, g['name'][x]   # (oracle == reference, as on the CPU)
        want.append(row)
    return SimpleNamespace(g=g, n=n, seqs=seqs, mat=mat, db=db, want=want, names=[str(s) for s in g['name']],
                           ss=gpu.seqset(resid, off, sw_bias), par=gpu.sw_params(mat, db, cov_thr=0.0))


def _align(gpu, tb, idx, hostpath=False):
    """one call on the pairs idx: [(score, ..., btLen, backtrace, evalue)] and the launches per traceback class"""
    idx = np.asarray(idx, np.uint32)
    gpu.profile()
    res, pool = gpu.sw_align(tb.par, tb.ss, tb.ss, 2 * idx, 2 * idx + 1, hostpath=hostpath)
    rep = gpu.profile_report()
    gpu.profile(False)
    assert all(k[13:] in tbgen.CLASSES for k in rep if k.startswith('sw_traceback')), sorted(rep)
    launches = Counter({c: int(rep['sw_traceback.' + c][1]) for c in tbgen.CLASSES if 'sw_traceback.' + c in rep})
    recs = [tuple(int(r[k]) for k in FIELDS) + (pool[int(r['btOffset']):int(r['btOffset']) + int(r['btLen'])].tobytes().decode(), float(r['evalue']))
            for r in res]
    return recs, launches


def _check(tb, idx, recs, what):
    for x, r in zip(idx, recs):
        assert r[:7] == tb.want[x][:7], (what, tb.names[x], r[:7], tb.want[x][:7])
        assert r[7] == tb.want[x][7], (what, tb.names[x], tbgen.compress_alignment(r[7]), tbgen.compress_alignment(tb.want[x][7]))
        assert r[8] == tb.want[x][8], (what, tb.names[x], r[8], tb.want[x][8])


@pytest.mark.parametrize('count', ['odd', 'even'])
@pytest.mark.parametrize('hostpath', [False, True], ids=['device', 'hostpath'])
def test_path_groups(gpu, tb, hostpath, count):
    """one call per path group (the pairs that run through the same classes in the same rounds), padded to an odd count of
    at least three tasks (the idle half of the last wavefront) or to an even one: records against the reference's rows, and
    exactly one launch per class and round of the group's history -- none in any class the group does not pass through.
    Device orchestration: 27 groups over the thirteen classes; host orchestration: 15 groups over its four."""
    groups = tbgen.groups(tb.g, hostpath)
    assert set(c for h in groups for c in h) == set(tbgen.CLASSES if not hostpath else tbgen.CLASSES[9:])
    for h, members in groups.items():
        idx = tbgen.padded(members, count == 'odd')
        recs, launches = _align(gpu, tb, idx, hostpath)
        print('>'.join(h), [tb.names[x] for x in members], len(idx), dict(launches))
        _check(tb, idx, recs, h)
        assert launches == Counter(h), (h, launches)
    if not hostpath:   # one band per round in the global class
        h = tbgen.golden_history(tb.g, tb.names.index('double_g1025'))
        assert h.count('global') == 2 and len(groups[h]) == 1


def test_all_pairs_shuffled_in_one_call(gpu, tb):
    """every pair in random order, every class with an odd count in the first round: the sort by class key, the order array and
    rounds in which tasks of several classes arrive from different predecessors.  The records equal the reference's rows, which
    is what the grouped calls return; a class is launched once in every round in which the histories put a task there."""
    order = tbgen.shuffled(tb.g)
    rounds = tbgen.round_counts(tb.g, order)
    assert all(rounds[(0, c)] >= 3 and rounds[(0, c)] % 2 == 1 for c in tbgen.CLASSES)
    for hostpath in (False, True):
        recs, launches = _align(gpu, tb, order, hostpath)
        _check(tb, order, recs, 'shuffled hostpath=%d' % hostpath)
        assert launches == Counter(c for _, c in tbgen.round_counts(tb.g, order, hostpath)), launches


def test_small_scratch_budget(gpu, tb, monkeypatch):
    """the shuffled call under a direction-scratch budget of 1 MiB: the global-band tasks need several MiB each, so no task fits
    at some point and the budget grows to what one task needs, and tasks wait deferred while others migrate between classes"""
    order = tbgen.shuffled(tb.g)
    free, launches_free = _align(gpu, tb, order)
    monkeypatch.setenv('SD_TB_BUDGET', '1048576')
    try:
        recs, launches = _align(gpu, tb, order)
    finally:
        monkeypatch.delenv('SD_TB_BUDGET')
    _check(tb, order, recs, 'budget')
    assert recs == free
    # (band 2048 x 1955 rows: 8 MB of direction bytes for one task)
    x = tb.names.index('double_g1025')
    assert (2 * 2048 + 1) * (int(tb.g['res'][x][2]) + 1) > 4 * 1048576
    print(dict(launches_free), dict(launches))
    # more rounds than the five of the free call: the LDS and global classes run in slices
    assert all(launches[c] >= launches_free[c] for c in tbgen.CLASSES)
    assert sum(launches[c] for c in tbgen.CLASSES[9:]) > sum(launches_free[c] for c in tbgen.CLASSES[9:]) + 3, (launches_free, launches)


def test_run_length_text_of_long_runs(gpu, tb):
    """sd_sw_set_cigar_pool on the doubling and boundary pairs: single runs of up to 1 025 I or D (four-digit counts, runs that
    span many 64-letter steps of k_bt_cigar) against Matcher::compressAlignment of the reference's backtrace"""
    idx = [x for x in range(tb.n) if str(tb.g['kind'][x]) in ('doubling', 'skew', 'boundary')]
    longest = [max([n for a, n in tbgen.runs(tb.want[x][7]) if a != 'M'] or [0]) for x in idx]
    assert sum(n >= 64 for n in longest) >= 10 and sum(n >= 256 for n in longest) >= 6 and sum(n >= 1024 for n in longest) >= 2
    ix = np.asarray(idx, np.uint32)
    try:
        gpu.set_cigar_pool(True)
        res, pool = gpu.sw_align(tb.par, tb.ss, tb.ss, 2 * ix, 2 * ix + 1)
        for x, r in zip(idx, res):
            assert tuple(int(r[k]) for k in FIELDS) == tb.want[x][:7], tb.names[x]
            txt = pool[int(r['btOffset']):int(r['btOffset']) + (int(r['flags']) >> 8)].tobytes().decode()
            assert txt == tbgen.compress_alignment(tb.want[x][7]), (tb.names[x], txt)
    finally:
        gpu.set_cigar_pool(False)


def test_profile_queries_double_their_band(gpu, host, oracle, tb):
    """the PROF instantiations beyond their first band: three doubling pairs with the query as a profile (its own matrix rows
    times five plus noise), one that ends in a narrow class after three bands, one in lds512 at its second band there, one
    in the global class after two rounds -- against the oracle, in the classes of their plain twins"""
    names = ('double_g4', 'double_g128', 'double_g1025')
    m = np.array([tb.mat[i] for i in range(441)], np.int32).reshape(21, 21)
    rng = np.random.default_rng(31)
    recs, boff, targets = [], [0], []
    for nm in names:
        x = tb.names.index(nm)
        s = tb.seqs[2 * x]
        rows = m[np.minimum(s.astype(np.int64), 19), :20] * 5 + rng.integers(-3, 4, (len(s), 20))
        rec = np.zeros((len(s), 25), np.uint8)
        rec[:, :20] = np.clip(rows, -128, 127).astype(np.int8).view(np.uint8)
        rec[:, 20] = s
        rec[:, 21] = np.argmax(rows, axis=1)
        recs.append(rec.tobytes())
        boff.append(boff[-1] + len(recs[-1]))
        targets.append(tb.seqs[2 * x + 1])
    prof = host.map_profiles(b''.join(recs), np.array(boff, np.uint64))
    toff = np.zeros(len(targets) + 1, np.uint64)
    toff[1:] = np.cumsum([len(t) for t in targets])
    qs = gpu.profileset(prof['letters'], prof['offsets'], prof['aln'])
    ts = gpu.seqset(np.concatenate(targets), toff, None)
    po = prof['offsets']
    for k, nm in enumerate(names):
        a, b = int(po[k]), int(po[k + 1])
        o = oracle.sw_align_profile(prof['letters'][a:b], prof['aln'][a:b], targets[k], tb.db, cov_thr=0.0)
        h = tbgen.history(o['qEnd'] - o['qStart'] + 1, o['tEnd'] - o['tStart'] + 1, tbgen.deviation(o['backtrace']))
        assert h == tbgen.golden_history(tb.g, tb.names.index(nm)), (nm, h)   # the twin's classes, round by round
        pq, pt = np.full(3, k, np.uint32), np.full(3, k, np.uint32)
        gpu.profile()
        res, pool = gpu.sw_align(tb.par, qs, ts, pq, pt)
        rep = gpu.profile_report()
        gpu.profile(False)
        for r in res:
            assert tuple(int(r[f]) for f in FIELDS) == tuple(o[f] for f in FIELDS), (nm, r, o)
            assert pool[int(r['btOffset']):int(r['btOffset']) + int(r['btLen'])].tobytes().decode() == o['backtrace'], nm
            assert float(r['evalue']) == o['evalue'], nm
        launches = Counter({c: int(rep['sw_traceback.' + c][1]) for c in tbgen.CLASSES if 'sw_traceback.' + c in rep})
        assert launches == Counter(h), (nm, launches)
