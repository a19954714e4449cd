"""GPU: the expansion kernels (sd_expand_batch / sd_expand_backtraces through spacedust_amd.api.expand) and `sdgpu expandaln` against the
reference's own per-pair results and rows (tests/golden/expand_vectors.npz, tools/make_golden_expand.py)."""
import os
import subprocess

import numpy as np
import pytest

import exp_ref
import expgen
import expgold
from dbutil import SDGPU, read_db, sdgpu, write_db
from spacedust_amd import _lib, api

pytestmark = pytest.mark.gpu


def _want(tag):
    """the golden pairs of a set as EXPAND_DTYPE fields"""
    coords, texts = expgold.pairs(tag)
    n_runs = np.array([len(exp_ref.runs_of(t.decode())) for t in texts], np.int32)
    text_len = np.array([len(t) for t in texts], np.int32)
    return coords, texts, n_runs, text_len


def _check(res, coords, n_runs, text_len):
    for i, f in enumerate(('aStart', 'aEnd', 'cStart', 'cEnd', 'btLen')):
        assert np.array_equal(res[f], coords[:, i]), f
    assert np.array_equal(res['nRuns'], n_runs) and np.array_equal(res['textLen'], text_len)
    assert np.array_equal(res['flags'], np.where(coords[:, 4] == 0, _lib.EXPAND_EMPTY, 0))
    assert not res['rawScore'].any() and not res['identities'].any()


@pytest.mark.parametrize('tag', expgold.SETS)
def test_records_and_text_against_the_reference(gpu, tag):
    inp, pair_rows = expgold.batch_inputs(expgold.db(tag + '_ab'), expgold.db(tag + '_bc'))
    coords, texts, n_runs, text_len = _want(tag)
    res, pool, off = api.expand(gpu, want_text=True, **inp)
    assert len(res) == len(pair_rows) == len(coords)
    _check(res, coords, n_runs, text_len)
    kept = np.flatnonzero(coords[:, 4] > 0)
    assert len(off) == len(kept) + 1 and int(off[-1]) == int(text_len.sum()) == len(pool)
    blob = pool.tobytes()
    assert [blob[int(off[k]):int(off[k + 1])] for k in range(len(kept))] == [texts[i] for i in kept]
    st = api.expand_last_stats(gpu)
    assert st['pairs'] == len(res) and st['bytes_written'] == 48 * len(res) + len(pool) and st['runs_read'] > 0


def test_all_pairs_shuffled_into_one_call(gpu):
    """the rows of the three sets in one call, in random order, their clusters side by side: every record is its pair's"""
    rng = np.random.default_rng(3)
    sa, sb, runs, clu, bc_rows, want, origin = [], [], [], [], [], [], []
    for tag in expgold.SETS:
        inp, _ = expgold.batch_inputs(expgold.db(tag + '_ab'), expgold.db(tag + '_bc'))
        coords, texts, _, _ = _want(tag)
        base, p = len(bc_rows), 0
        for i in range(len(inp['ab_runs'])):
            c = inp['ab_cluster'][i]
            n = len(inp['bc_rows'][c]) if c >= 0 else 0
            sa.append(inp['ab_start_a'][i])
            sb.append(inp['ab_start_b'][i])
            runs.append(inp['ab_runs'][i])
            clu.append(base + c if c >= 0 else -1)
            want.append((coords[p:p + n], texts[p:p + n]))
            p += n
        bc_rows += inp['bc_rows']
    order = rng.permutation(len(runs))
    res, pool, off = api.expand(gpu, [sa[i] for i in order], [sb[i] for i in order], [runs[i] for i in order], [clu[i] for i in order], bc_rows,
                                want_text=True)
    coords = np.concatenate([want[i][0] for i in order])
    texts = [t for i in order for t in want[i][1]]
    assert len(res) == len(coords) > 600
    for i, f in enumerate(('aStart', 'aEnd', 'cStart', 'cEnd', 'btLen')):
        assert np.array_equal(res[f], coords[:, i]), f
    blob = pool.tobytes()
    assert [blob[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)] == [t for t in texts if t]
    # pass 2 for a chosen few, in another order than pass 1 met them
    pick = np.flatnonzero(coords[:, 4] > 0)[::-7].astype(np.uint64)
    _, pool2, off2 = api.expand(gpu, [sa[i] for i in order], [sb[i] for i in order], [runs[i] for i in order], [clu[i] for i in order], bc_rows,
                                want_text=pick)
    blob2 = pool2.tobytes()
    assert [blob2[int(off2[k]):int(off2[k + 1])] for k in range(len(pick))] == [texts[int(i)] for i in pick]


def test_bad_input_is_refused_by_value(gpu):
    ok = dict(ab_start_a=[0], ab_start_b=[0], ab_runs=[[(5 << 2) | 0]], ab_cluster=[0], bc_rows=[[(0, 0, [(5 << 2) | 0])]])
    assert api.expand(gpu, **ok)['btLen'][0] == 5
    for key, bad in (('ab_runs', [[(5 << 2) | 3]]), ('ab_runs', [[0 | 1]]), ('bc_rows', [[(0, 0, [(5 << 2) | 3])]]), ('bc_rows', [[(0, 0, [2])]]),
                     ('ab_cluster', [1])):
        with pytest.raises(api.SdError, match=r'\(-3\)'):          # SD_EINVAL
            api.expand(gpu, **dict(ok, **{key: bad}))
    with pytest.raises(api.SdError, match=r'\(-3\)'):          # mode 1 without the sequence sets
        api.expand(gpu, mode=1, **ok)
    with pytest.raises(api.SdError, match=r'\(-3\)'):
        api.expand(gpu, mode=2, **ok)
    # and the context goes on working
    assert api.expand(gpu, **ok)['aEnd'][0] == 4


@pytest.fixture(scope='module')
def dbs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('expand_gpu')
    write_db(str(tmp / 'seq'), [(0, b'ACDEFGHIKL\n')], 0)
    write_db(str(tmp / 'prof'), [(0, b'\0' * 24)], 2)
    for tag in expgold.SETS:
        # split data files, as the reference's multi-threaded writers leave them (set P has one query: one file)
        write_db(str(tmp / (tag + '_ab')), sorted(expgold.db(tag + '_ab').items()), 5, splits=1 if tag == 'P' else 3)
        write_db(str(tmp / (tag + '_bc')), sorted(expgold.db(tag + '_bc').items()), 5, splits=2)
    return tmp


DBTYPE = b'\x05\x00\x02\x00'   # DBTYPE_ALIGNMENT_RES | DBTYPE_EXTENDED_INDEX_NEED_SRC << 16


@pytest.mark.parametrize('threads', [1, 8])
@pytest.mark.parametrize('tag', ['K', 'G'])
def test_module_writes_the_reference_db(dbs, tag, threads):
    out = str(dbs / ('%s_out_%d' % (tag, threads)))
    # C is a profile DB, as in clustersearch.sh: mode 0 reads no sequence
    sdgpu('expandaln', dbs / 'seq', dbs / 'prof', dbs / (tag + '_ab'), dbs / (tag + '_bc'), out, '--threads', threads, '-v', '0', '--db-load-mode', '2')
    assert read_db(out) == expgold.db(tag + '_out')
    assert open(out + '.dbtype', 'rb').read() == DBTYPE == np.int32(expgold.golden()['dbtype']).tobytes()


def test_module_in_calls_of_seven_pairs(dbs):
    """SD_EXPAND_PAIRS: whole entries per device call, at most so many pairs unless one entry has more (the 300 of cluster_300 go alone)"""
    out = str(dbs / 'K_out_budget7')
    p = subprocess.run([SDGPU, 'expandaln', str(dbs / 'seq'), str(dbs / 'seq'), str(dbs / 'K_ab'), str(dbs / 'K_bc'), out, '-v', '0'],
                       env=dict(os.environ, SD_EXPAND_PAIRS='7'), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr
    assert read_db(out) == expgold.db('K_out')


@pytest.mark.parametrize('i', range(len(expgen.P_PARAMS)))
def test_module_criteria(dbs, i):
    names = dict(e='-e', c='-c', cov_mode='--cov-mode', min_seq_id='--min-seq-id', min_aln_len='--min-aln-len')
    flags = [x for k, v in expgen.P_PARAMS[i].items() for x in (names[k], repr(v))]
    out = str(dbs / ('P_out_%d' % i))
    sdgpu('expandaln', dbs / 'seq', dbs / 'seq', dbs / 'P_ab', dbs / 'P_bc', out, '-v', '0', *flags)
    assert read_db(out) == expgold.db('P_out_%d' % i)


def test_module_refuses_an_ab_row_without_backtrace(dbs):
    plain = [(k, b''.join(b'\t'.join(l.split(b'\t')[:10]) + b'\n' for l in t.splitlines())) for k, t in sorted(expgold.db('P_ab').items())]
    write_db(str(dbs / 'P_ab_plain'), plain, 5)
    out = str(dbs / 'refused_plain')
    p = sdgpu('expandaln', dbs / 'seq', dbs / 'seq', dbs / 'P_ab_plain', dbs / 'P_bc', out, check=False)
    assert p.returncode != 0 and 'Alignment must contain a backtrace' in p.stderr
    assert not os.path.exists(out + '.index')


# ---- --expansion-mode 1 ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def seqs(host, gpu):
    s = expgold.mode1_seqs(host)
    s['set_bias'] = gpu.seqset(s['residues'], s['offsets'], s['sw_bias'])
    s['set_plain'] = gpu.seqset(s['residues'], s['offsets'], None)
    return s


def _mode1_inputs(ab_db, bc_db):
    inp, pair_rows = expgold.batch_inputs(ab_db, bc_db)
    ab_query = [q for q in sorted(ab_db) for _ in exp_ref.rows_of(ab_db[q])]
    bc_target = [m['key'] for k in sorted(bc_db) for m in exp_ref.rows_of(bc_db[k])]
    pair_query = [q for q in sorted(ab_db) for r in exp_ref.rows_of(ab_db[q]) if r['key'] in bc_db for _ in exp_ref.rows_of(bc_db[r['key']])]
    return inp, pair_rows, ab_query, bc_target, pair_query


def _walks(seqs, texts, coords, pair_rows, pair_query, bias):
    out = []
    for i, (ab, bc) in enumerate(pair_rows):
        q = pair_query[i]
        out.append(exp_ref.walk(exp_ref.uncompress(texts[i].decode()), int(coords[i, 0]), int(coords[i, 2]), seqs['a'][q], seqs['c'][bc['key']],
                                seqs['a_bias'][q] if bias else None, seqs['matrix']) if coords[i, 4] else (0, 0))
    return out


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('tag,ab,bc', [('G1', 'G1_ab', 'G_bc'), ('M', 'M_ab', 'M_bc')])
def test_mode_1_records(gpu, seqs, tag, ab, bc, bias):
    """the walk's raw score and identities of every pair, next to the records of mode 0, which stay what the reference gives"""
    inp, pair_rows, ab_query, bc_target, pair_query = _mode1_inputs(expgold.db(ab), expgold.db(bc))
    coords, texts, n_runs, text_len = _want(tag)
    res = api.expand(gpu, mode=1, queries=seqs['set_bias' if bias else 'set_plain'], targets=seqs['set_plain'], ab_query=ab_query, bc_target=bc_target,
                     matrix=seqs['matrix'], **inp)
    for i, f in enumerate(('aStart', 'aEnd', 'cStart', 'cEnd', 'btLen')):
        assert np.array_equal(res[f], coords[:, i]), f
    assert np.array_equal(res['nRuns'], n_runs) and np.array_equal(res['textLen'], text_len)
    want = _walks(seqs, texts, coords, pair_rows, pair_query, bias)
    assert all(w is not None for w in want)
    assert np.array_equal(res['rawScore'], [w[0] for w in want]) and np.array_equal(res['identities'], [w[1] for w in want])
    assert np.array_equal(res['flags'], np.where(coords[:, 4] == 0, _lib.EXPAND_EMPTY, 0))
    assert res['identities'].max() > 20 and res['rawScore'].min() < 0 < res['rawScore'].max()


def test_mode_1_walks_that_leave_a_sequence_are_flagged(gpu, seqs):
    """constructed pairs whose walk would read outside A or C come back flagged, unread, and every other record of the call is exact"""
    a_len, c_len = len(seqs['a'][0]), len(seqs['c'][1])
    M = lambda n: (n << 2) | 0
    I = lambda n: (n << 2) | 1
    D = lambda n: (n << 2) | 2
    # (A start, B start, AB runs) through identity rows of C = sequence 1 at C start cs: the AC backtrace is AB's
    rows = [(a_len - 2, [M(2)], 0, True), (a_len - 1, [M(2)], 0, False), (a_len - 3, [M(1), I(2), M(1)], 0, False),
            (0, [M(1), D(2), M(1)], c_len - 3, False), (0, [M(1), D(2), M(1)], c_len - 4, True), (5, [M(30)], 7, True),
            (0, [M(3)], c_len - 2, False)]
    bc_rows = [[(0, cs, [M(100)])] for _, _, cs, _ in rows]
    res = api.expand(gpu, [r[0] for r in rows], [0] * len(rows), [r[1] for r in rows], list(range(len(rows))), bc_rows, mode=1,
                     queries=seqs['set_bias'], targets=seqs['set_plain'], ab_query=[0] * len(rows), bc_target=[1] * len(rows), matrix=seqs['matrix'])
    for i, (a0, runs, cs, inside) in enumerate(rows):
        bt = ''.join('MID'[r & 3] * (r >> 2) for r in runs)
        w = exp_ref.walk(bt, a0, cs, seqs['a'][0], seqs['c'][1], seqs['a_bias'][0], seqs['matrix'])
        assert (w is not None) == inside, i
        assert (int(res['aStart'][i]), int(res['cStart'][i]), int(res['btLen'][i])) == (a0, cs, len(bt)), i
        if inside:
            assert int(res['flags'][i]) == 0 and (int(res['rawScore'][i]), int(res['identities'][i])) == w, i
        else:
            assert int(res['flags'][i]) == _lib.EXPAND_LEAVES_SEQUENCE and int(res['rawScore'][i]) == 0 and int(res['identities'][i]) == 0, i


def test_mode_1_refuses_profile_sets(gpu, host, seqs):
    import tpref
    data, poff = tpref.g_profiles()
    prof = host.map_profiles(data[int(poff[0]):int(poff[1])], np.array([0, int(poff[1] - poff[0])], np.uint64))
    pset = gpu.profileset(prof['letters'], prof['offsets'], prof['aln'])
    ok = dict(ab_start_a=[0], ab_start_b=[0], ab_runs=[[(5 << 2) | 0]], ab_cluster=[0], bc_rows=[[(0, 0, [(5 << 2) | 0])]], ab_query=[0], bc_target=[0],
              matrix=seqs['matrix'])
    for q, t in ((pset, seqs['set_plain']), (seqs['set_plain'], pset)):
        with pytest.raises(api.SdError, match=r'\(-5\)'):      # SD_EUNSUPPORTED
            api.expand(gpu, mode=1, queries=q, targets=t, **ok)


@pytest.fixture(scope='module')
def seq_db(dbs):
    import swapgold
    return swapgold.write_set_g(dbs)[0]


@pytest.mark.parametrize('mode', range(4))
def test_module_mode_1(dbs, seq_db, mode):
    write_db(str(dbs / 'G1_ab'), sorted(expgold.db('G1_ab').items()), 5)
    out = str(dbs / ('G1_out_%d' % mode))
    sdgpu('expandaln', seq_db, seq_db, dbs / 'G1_ab', dbs / 'G_bc', out, '--expansion-mode', '1', '--seq-id-mode', mode, '--threads', '8', '-v', '0')
    assert read_db(out) == expgold.db('G1_out_%d' % mode)
    assert open(out + '.dbtype', 'rb').read() == DBTYPE


@pytest.mark.parametrize('bias', [1, 0])
def test_module_mode_1_score_bound_and_bias(dbs, seq_db, bias):
    write_db(str(dbs / 'M_ab'), sorted(expgold.db('M_ab').items()), 5)
    write_db(str(dbs / 'M_bc'), sorted(expgold.db('M_bc').items()), 5)
    out = str(dbs / ('M_out_%d' % bias))
    sdgpu('expandaln', seq_db, seq_db, dbs / 'M_ab', dbs / 'M_bc', out, '--expansion-mode', '1', '-e', '1e9', '--comp-bias-corr', bias, '-v', '0')
    assert read_db(out) == expgold.db('M_out_bias%d' % bias)


def test_module_mode_1_counts_the_walks_it_drops(dbs, seq_db):
    """a row whose translated backtrace walks off the end of A: no reference row exists; the module drops it and says how many"""
    import swapgold
    a_len = len(swapgold.sequences()[0])
    write_db(str(dbs / 'L_ab'), [(0, b'7\t50\t0.500\t1.000E-10\t%d\t%d\t%d\t0\t1\t100\t2M\n' % (a_len - 1, a_len, a_len) +
                                  b'8\t50\t0.500\t1.000E-10\t0\t1\t%d\t0\t1\t100\t2M\n' % a_len)], 5)
    write_db(str(dbs / 'L_bc'), [(7, b'1\t50\t1.00\t1.000E-10\t0\t99\t100\t0\t99\t100\t100M\n'), (8, b'2\t50\t1.00\t1.000E-10\t0\t99\t100\t0\t99\t100\t100M\n')], 5)
    out = str(dbs / 'L_out')
    p = sdgpu('expandaln', seq_db, seq_db, dbs / 'L_ab', dbs / 'L_bc', out, '--expansion-mode', '1', '-e', '1e9')
    assert '1 pairs dropped' in p.stderr
    rows = read_db(out)[0].splitlines()
    assert len(rows) == 1 and rows[0].startswith(b'2\t')
