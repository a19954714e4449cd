"""Host side of `expandaln` (no GPU): the restatement tests/exp_ref.py against the reference's own rows
(tests/golden/expand_vectors.npz, tools/make_golden_expand.py), the defining condition of every constructed class on that file, the
run-list form against the expanded-column form, and what the module and the C ABI declare or refuse without a device."""
import numpy as np
import pytest

import exp_ref
import expgen
import expgold
from dbutil import sdgpu, write_db


@pytest.mark.parametrize('run_form', [True, False])
@pytest.mark.parametrize('tag', ['K', 'G'])
def test_restatement_reproduces_the_reference(tag, run_form):
    got_pairs = []
    out = exp_ref.expand(expgold.db(tag + '_ab'), expgold.db(tag + '_bc'), pairs=got_pairs, run_form=run_form)
    assert out == expgold.db(tag + '_out')
    coords, texts = expgold.pairs(tag)
    assert len(got_pairs) == len(coords) > 0
    assert np.array_equal(np.array([p[:5] for p in got_pairs], np.int32), coords)
    assert [p[5].encode() for p in got_pairs] == texts


@pytest.mark.parametrize('i', range(len(expgen.P_PARAMS)))
def test_restatement_reproduces_the_criteria(i):
    out = exp_ref.expand(expgold.db('P_ab'), expgold.db('P_bc'), expgen.P_PARAMS[i])
    assert out == expgold.db('P_out_%d' % i)


def test_generators_give_the_recorded_inputs():
    for tag, (ab, bc) in (('K', expgen.set_k()), ('P', expgen.set_p())):
        assert ab == expgold.db(tag + '_ab') and bc == expgold.db(tag + '_bc')
    assert int(expgold.golden()['dbtype']) == 5 | (2 << 16)   # DBTYPE_ALIGNMENT_RES, DBTYPE_EXTENDED_INDEX_NEED_SRC


def _class(name):
    """(AB rows, BC DB as rows, output rows) of a class of set K"""
    q = expgen.K_QUERY[name]
    bc = {k: exp_ref.rows_of(t) for k, t in expgold.db('K_bc').items()}
    return exp_ref.rows_of(expgold.db('K_ab')[q]), bc, exp_ref.rows_of(expgold.db('K_out')[q])


def _facts(name):
    ab, bc, out = _class(name)
    return [expgen.pair_facts(r, m) for r in ab if r['key'] in bc for m in bc[r['key']]], out


def test_class_start_positions():
    f, out = _facts('ab_earlier')
    assert f[0]['ab_start_b'] < f[0]['bc_start_b'] and not f[0]['skip_short'] and len(out) == 1
    f, out = _facts('bc_earlier')
    assert f[0]['ab_start_b'] > f[0]['bc_start_b'] and not f[0]['skip_short'] and len(out) == 1
    f, out = _facts('same_start')
    assert f[0]['ab_start_b'] == f[0]['bc_start_b'] and len(out) == 1
    for name in ('skip_exhausts_ab', 'skip_exhausts_bc'):
        f, out = _facts(name)
        assert f[0]['skip_short'] and f[0]['lockstep_columns'] == 0 and out == []
    assert _facts('skip_exhausts_ab')[0][0]['ab_start_b'] < _facts('skip_exhausts_ab')[0][0]['bc_start_b']
    assert _facts('skip_exhausts_bc')[0][0]['ab_start_b'] > _facts('skip_exhausts_bc')[0][0]['bc_start_b']


def test_class_dropped_columns_and_tails():
    f, out = _facts('id_di_middle')
    assert f[0]['none_in_middle'] and f[0]['none_columns'] == 6 and len(out) == 1
    f, out = _facts('only_id_di')
    assert f[0]['lockstep_columns'] == f[0]['none_columns'] == 8 and f[0]['emitted'] == 0 and out == []
    f, out = _facts('gap_after_last_m')
    assert len(f) == 2 and all(x['emitted'] > x['last_m'] > 0 for x in f) and len(out) == 2
    for x, row in zip(f, out):
        printed = exp_ref.uncompress(row['cigar'])
        assert len(printed) == x['last_m']
        # the ends count columns the printed backtrace no longer has
        assert row['q_end'] - row['q_start'] + 1 > sum(c in 'MD' for c in printed) or row['db_end'] - row['db_start'] + 1 > sum(c in 'MI' for c in printed)
    f, out = _facts('no_m')
    assert f[0]['emitted'] > 0 and f[0]['last_m'] == 0 and out == []
    f, out = _facts('one_column')
    assert f[0]['ab_columns'] == f[0]['bc_columns'] == f[0]['emitted'] == 1 and out[0]['cigar'] == '1M'


def test_class_sizes():
    f, out = _facts('long_runs')
    assert min(f[0]['ab_columns'], f[0]['bc_columns']) >= 5000 and min(f[0]['ab_runs'], f[0]['bc_runs']) >= 600 and len(out) == 1
    assert len(exp_ref.runs_of(out[0]['cigar'])) > 600
    f, out = _facts('single_3000m')
    assert f[0]['ab_runs'] == 1 and f[0]['ab_columns'] == 3000 and len(out) == 1
    assert len(_facts('cluster_1')[0]) == 1
    f, out = _facts('cluster_300')
    assert len(f) == 300 and len(out) > 250


def test_class_one_row_per_key_and_query():
    ab, bc, out = _class('two_b_first_kept')
    assert [m['key'] for m in bc[ab[0]['key']]] == [1500] and 1500 in [m['key'] for m in bc[ab[1]['key']]]
    assert [r['key'] for r in out] == [1500, 1501] and out[0]['score'] == ab[0]['score']
    ab, bc, out = _class('two_b_first_fails_e')
    assert ab[0]['eval'] > exp_ref.DEFAULTS['e'] >= ab[1]['eval']
    assert [r['key'] for r in out] == [1500, 1501] and out[0]['score'] == ab[1]['score']
    ab, bc, out = _class('two_b_nonoverlap_dropped')
    both = exp_ref.expand({0: expgold.db('K_ab')[expgen.K_QUERY['two_b_nonoverlap_dropped']].splitlines(keepends=True)[1]}, expgold.db('K_bc'))
    second = exp_ref.rows_of(both[0])
    assert len(out) == 1 and len(second) == 1 and second[0]['key'] == out[0]['key'] == 1502     # alone, the second candidate is kept
    assert second[0]['q_start'] > out[0]['q_end']                                               # and it does not overlap the first
    ab, bc, out = _class('b_absent')
    assert ab[0]['key'] not in bc and ab[1]['key'] in bc and len(out) == 1
    ab, bc, out = _class('empty_ab')
    assert ab == [] and out == [] and expgen.K_QUERY['empty_ab'] in expgold.db('K_out')


def test_class_criteria_have_rows_on_both_sides():
    base = set(expgold.db('P_out_0')[0].splitlines())
    assert len(base) == 11                                           # -e 0.001 itself drops one of the twelve
    evals = [r['eval'] for r in exp_ref.rows_of(expgold.db('P_ab')[0])]
    assert any(e <= 0.001 for e in evals) and any(0.001 < e < 0.0011 for e in evals)
    dropped_by = []
    for i in range(1, len(expgen.P_PARAMS)):
        rows = set(expgold.db('P_out_%d' % i)[0].splitlines())
        assert rows < base and rows, expgen.P_PARAMS[i]              # the criterion drops some rows and keeps others
        dropped_by.append(frozenset(base - rows))
    assert len(set(dropped_by)) == len(dropped_by)                   # and no two parameter sets drop the same rows


@pytest.fixture(scope='module')
def seqs(host):
    return expgold.mode1_seqs(host)


@pytest.mark.parametrize('mode', range(4))
def test_restatement_reproduces_mode_1(seqs, mode):
    """--expansion-mode 1 on set G with its sequences, every --seq-id-mode: score, identity and E-value come from the walk"""
    walks = []
    out = exp_ref.expand(expgold.db('G1_ab'), expgold.db('G_bc'), dict(mode=1, seq_id_mode=mode), seqs=dict(seqs, walks=walks))
    assert out == expgold.db('G1_out_%d' % mode)
    assert len(walks) > 300 and all(w is not None for w in walks)       # every recorded row is defined behaviour
    assert out != expgold.db('G_out') and sum(t.count(b'\n') for t in out.values()) == 310
    if mode:
        assert out != expgold.db('G1_out_0')


def test_mode_1_score_bound_and_bias(seqs):
    par = dict(mode=1, e=1e9)
    q6, q7, real = (int(v) for v in expgold.golden()['M_raw_queries'])
    walks = []
    out = exp_ref.expand(expgold.db('M_ab'), expgold.db('M_bc'), par, seqs=dict(seqs, walks=walks))
    assert out == expgold.db('M_out_bias1')
    raws = sorted(w[0] for w in walks)
    assert raws[:2] == [-7, -6]                                          # on either side of "raw score below -6"
    assert len(exp_ref.rows_of(out[q6])) == 1 and (q7 == q6 or out[q7] == b'')
    assert sum(t.count(b'\n') for t in out.values()) == len(walks) - 1  # only the -7 row goes
    plain = exp_ref.expand(expgold.db('M_ab'), expgold.db('M_bc'), dict(par, comp_bias_corr=0), seqs=seqs)
    assert plain == expgold.db('M_out_bias0') and plain[real] != out[real]   # the rounded bias changes scores
    bias = seqs['a_bias'][real]
    assert (bias != 0).any()


def test_walk_outside_a_sequence_is_reported(seqs):
    a, c = seqs['a'][0], seqs['c'][1]
    assert exp_ref.walk('MM', len(a) - 2, 0, a, c, None, seqs['matrix']) is not None
    assert exp_ref.walk('MM', len(a) - 1, 0, a, c, None, seqs['matrix']) is None
    assert exp_ref.walk('MDDM', 0, len(c) - 3, a, c, None, seqs['matrix']) is None
    assert exp_ref.walk('MIIM', len(a) - 3, 0, a, c, None, seqs['matrix']) is None


def _random_cigar(rng):
    return ''.join('%d%s' % (rng.integers(0, 9), 'MID'[rng.integers(0, 3)]) for _ in range(rng.integers(1, 12)))


def test_run_form_equals_column_form_on_random_pairs():
    rng = np.random.default_rng(7)
    empty = 0
    for _ in range(2000):
        ab, bc = _random_cigar(rng), _random_cigar(rng)
        sa, sb, tb, tc = (int(v) for v in rng.integers(0, 12, 4))
        a0, a1, c0, c1, bt = exp_ref.translate_columns(sa, sb, exp_ref.uncompress(ab), tb, tc, exp_ref.uncompress(bc))
        got = exp_ref.translate_runs(sa, sb, exp_ref.runs_of(ab), tb, tc, exp_ref.runs_of(bc))
        assert got == (a0, a1, c0, c1, len(bt), exp_ref.compress(bt) if bt else ''), (ab, bc, sa, sb, tb, tc)
        empty += not bt
    assert 100 < empty < 1900


def test_identity_bc_row_returns_ab():
    rng = np.random.default_rng(11)
    for _ in range(200):
        cigar = expgen.random_cigar(rng, int(rng.integers(1, 20)), 1, 30)
        bt = exp_ref.uncompress(cigar)
        sa, sb = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        b_len = sb + sum(c in 'MD' for c in bt) + int(rng.integers(0, 20))
        # B aligned with itself over all of B: one M run from position 0 that outlasts AB's columns
        a0, a1, c0, c1, n, text = exp_ref.translate_runs(sa, sb, exp_ref.runs_of(cigar), 0, 0, [('M', b_len + len(bt))])
        assert (a0, c0) == (sa, sb)
        last_m = max(i + 1 for i, c in enumerate(bt) if c == 'M')
        assert n == last_m and text == exp_ref.compress(bt[:last_m])
        assert a1 == sa + sum(c in 'MD' for c in bt) - 1 and c1 == sb + sum(c in 'MI' for c in bt) - 1


def test_header_declares_the_expansion_calls():
    from spacedust_amd import _lib
    for name in ('sd_expand_batch', 'sd_expand_backtraces', 'sd_expand_last_stats'):
        assert name in _lib.DECLARED_SYMBOLS
    assert _lib.EXPAND_DTYPE.itemsize == 48


def test_module_is_registered():
    p = sdgpu('expandaln', check=False)
    assert p.returncode != 0 and 'usage: expandaln <queryDB> <targetDB> <resultDB_AB> <resultDB_BC> <outDB>' in p.stderr
    assert 'unknown module' not in p.stderr
    assert 'expandaln' in sdgpu('--help').stdout


@pytest.fixture(scope='module')
def dbs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('expand_host')
    for name, dbtype in (('seq', 0), ('prof', 2), ('idx', 9)):
        write_db(str(tmp / name), [(0, b'ACDEFGHIKL\n')], dbtype)
    write_db(str(tmp / 'ab'), sorted(expgold.db('P_ab').items()), 5)
    write_db(str(tmp / 'bc'), sorted(expgold.db('P_bc').items()), 5)
    plain = {k: b''.join(b'\t'.join(l.split(b'\t')[:10]) + b'\n' for l in t.splitlines()) for k, t in expgold.db('P_bc').items()}
    write_db(str(tmp / 'bc_plain'), sorted(plain.items()), 5)
    return tmp


@pytest.mark.parametrize('a,c,bc,flags,words', [
    ('seq', 'seq', 'bc', ['--expand-filter-clusters', '1'], '--expand-filter-clusters 1'),
    ('seq', 'seq', 'bc', ['--compressed', '1'], '--compressed 1'),
    ('seq', 'idx', 'bc', [], 'index DB'),
    ('prof', 'prof', 'bc', [], 'Profile-profile is currently not supported'),
    ('seq', 'prof', 'bc', ['--expansion-mode', '1'], '--expansion-mode 1 with a profile database'),
    ('prof', 'seq', 'bc', ['--expansion-mode', '1'], '--expansion-mode 1 with a profile database'),
    ('seq', 'seq', 'bc', ['--expansion-mode', '1', '--gap-open', '10'], 'gap costs other than --gap-open 11 --gap-extend 1'),
    ('seq', 'seq', 'bc', ['--expansion-mode', '1', '--sub-mat', 'VTML80.out'], 'only blosum62.out'),
    ('seq', 'seq', 'bc', ['--expansion-mode', '1', '--comp-bias-corr-scale', '0.5'], '--comp-bias-corr-scale'),
    ('seq', 'seq', 'bc', ['--expansion-mode', '2'], '--expansion-mode 2'),
    ('seq', 'seq', 'bc_plain', [], 'Alignment must contain a backtrace'),
])
def test_module_refusals_that_need_no_device(dbs, a, c, bc, flags, words):
    out = str(dbs / ('refused_' + a + c + bc + ''.join(flags).replace('-', '_')))
    p = sdgpu('expandaln', dbs / a, dbs / c, dbs / 'ab', dbs / bc, out, *flags, check=False)
    assert p.returncode != 0 and words in p.stderr, p.stderr
    assert not (dbs / (out + '.index')).exists()
