"""swapresults on the host -- sd_host_swapresults through spacedust_amd.api and `sdgpu swapresults` on DBs -- against the reference's
own doswap arithmetic (Matcher::swapResult / compareHits / resultToBuffer, QueryMatcher::parsePrefilterHit, EvalueComputation) as
tools/make_golden_swap.py recorded it.  No GPU."""
import numpy as np
import pytest

import swapgold
from dbutil import read_db, sdgpu, write_db
from spacedust_amd import api

G = swapgold.golden


def _e_columns(d):
    """(entry key, first column, E-value) of every alignment line"""
    return [(k, int(l.split(b'\t')[0]), float(l.split(b'\t')[3])) for k, t in d.items() for l in t.splitlines()]


@pytest.mark.parametrize('tag,n_rows', [('G110', 83), ('G95', 183)])
def test_golden_file_shows_both_branches(tag, n_rows):
    g = G()
    pref, pref_swapped, aln = swapgold.db(tag + '_pref'), swapgold.db(tag + '_pref_swapped'), swapgold.db(tag + '_aln_swapped')
    final = [swapgold.db(tag + '_final_%d' % i) for i in (0, 1)]
    e_hi, e_lo = (float(x) for x in g[tag + '_E'])
    assert swapgold.rows(pref) == swapgold.rows(pref_swapped) == n_rows
    assert sorted(pref) == list(range(swapgold.N_SEQ)) and sorted(pref_swapped) == list(range(swapgold.N_PROF))
    assert sorted(aln) == list(range(swapgold.N_PROF))
    n_aln = swapgold.rows(aln)
    assert 0 < n_aln <= n_rows
    # E[0]: every aligned row survives; E[1]: at least one is removed and a query that had rows is left with an empty entry
    assert swapgold.rows(final[0]) == n_aln and 0 < swapgold.rows(final[1]) < n_aln
    for f in final:
        assert sorted(f) == list(range(swapgold.N_SEQ))
    emptied = [q for q in final[0] if final[0][q] and not final[1][q]]
    assert emptied
    assert list(g[tag + '_figures']) == [n_rows, n_aln, swapgold.rows(final[0]), swapgold.rows(final[1]), len(emptied)]
    # the two E-values of a row differ (the two DBs differ in size), and E[1] separates no row's pair: align at E[1] keeps what the
    # second swap at E[1] keeps
    aligned = {(p, s): e for p, s, e in _e_columns(aln)}
    swapped = {(p, s): e for s, p, e in _e_columns(final[0])}
    assert sorted(aligned) == sorted(swapped)
    assert all(aligned[k] != swapped[k] for k in aligned if aligned[k] > 0)
    assert not any(swapped[k] <= e_lo < aligned[k] for k in aligned)
    assert all(swapped[k] <= e_hi and aligned[k] <= e_hi for k in aligned)


def test_golden_file_constructed_set():
    pref = b''.join(swapgold.db('C_pref').values())
    assert b'\t-32768\n' in pref and b'\t32767\n' in pref
    sw = swapgold.db('C_pref_swapped')
    assert sorted(sw) == [0, 1, 2, 3, 7] and sw[3] == b''          # 3: in the DB, no hits; 2: hits, not in the DB; 4 - 6: nothing
    assert sw[1] == b'2\t60\t0\n0\t50\t-32768\n1\t50\t-5\n5\t50\t7\n' and sw[0] == b'0\t40\t-32767\n'
    bt = b''.join(swapgold.db('C_aln_bt').values())
    assert b'I' in bt and b'D' in bt
    assert all(len(l.split(b'\t')) == 10 for t in swapgold.db('C_aln_plain').values() for l in t.splitlines())


@pytest.mark.parametrize('tag', swapgold.SETS)
def test_prefilter_swap_equals_reference(tag):
    g = G()
    got, n_in, n_out = api.swapresults(swapgold.db(tag + '_pref'), int(g['seq_residues']), np.arange(swapgold.N_PROF), want_counts=True)
    assert got == swapgold.db(tag + '_pref_swapped')
    assert n_in == n_out == int(g[tag + '_figures'][0])


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('tag', swapgold.SETS)
def test_alignment_swap_equals_reference(tag, which):
    g = G()
    got, n_in, n_out = api.swapresults(swapgold.db(tag + '_aln_swapped'), int(g['prof_residues']), np.arange(swapgold.N_SEQ),
                                       eval_thr=float(g[tag + '_E'][which]), want_counts=True)
    assert got == swapgold.db(tag + '_final_%d' % which)
    assert (n_in, n_out) == (int(g[tag + '_figures'][1]), int(g[tag + '_figures'][2 + which]))


def test_constructed_set_equals_reference():
    g = G()
    keys, res = g['C_keys'], int(g['C_residues'])
    assert api.swapresults(swapgold.db('C_pref'), res, keys) == swapgold.db('C_pref_swapped')
    for name in ('C_aln_bt', 'C_aln_plain'):
        got = api.swapresults(swapgold.db(name), res, keys, eval_thr=float(g['C_E'][0]))
        assert got == swapgold.db(name + '_swapped'), name
    sw = swapgold.db('C_aln_bt_swapped')
    assert sw[5] == b'' and 5 not in keys                           # emptied by the E-value: an entry although the DB has no key 5
    assert [l.split(b'\t')[0] for l in sw[1].splitlines()] == [b'0', b'1', b'6']   # equal E-value, score and length: the key decides
    assert sw[1].splitlines()[0].endswith(b'\t10M2D30M3I40M1D5M')


def test_refused_input():
    with pytest.raises(api.SdError) as e:
        api.swapresults({0: b'9\t50\t1\n'}, 1000, [0, 1, 2])          # a row on a key behind the DB's last
    assert '(-3)' in str(e.value)
    with pytest.raises(api.SdError):
        api.swapresults({0: b'1\t50\n'}, 1000, [0, 1, 2])             # neither a prefilter nor an alignment line
    with pytest.raises(api.SdError) as e:
        api.swapresults({0: b'1\t50\t1\n'}, 1000, [0, 1, 2], gap_open=10)
    assert '(-5)' in str(e.value)
    assert api.swapresults({}, 1000, [0, 2]) == {0: b'', 2: b''}


@pytest.mark.parametrize('tag', swapgold.SETS)
def test_prefilter_swap_twice_gives_the_rows_back(tag):
    g = G()
    pref = swapgold.db(tag + '_pref')
    once = api.swapresults(pref, int(g['seq_residues']), np.arange(swapgold.N_PROF))
    twice = api.swapresults(once, int(g['prof_residues']), np.arange(swapgold.N_SEQ))
    assert sorted(twice) == sorted(pref)
    for q in pref:
        assert sorted(twice[q].splitlines()) == sorted(pref[q].splitlines()), q


@pytest.fixture(scope='module')
def dbs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('swapdbs')
    seq_db, prof_db = swapgold.write_set_g(tmp)
    return tmp, seq_db, prof_db


@pytest.mark.parametrize('tag', swapgold.SETS)
def test_module_on_dbs(dbs, tag):
    """`sdgpu swapresults` both ways: the same bytes with one thread, with eight, and when the input lies in eight data files"""
    tmp, seq_db, prof_db = dbs
    g = G()
    pref, aln = sorted(swapgold.db(tag + '_pref').items()), sorted(swapgold.db(tag + '_aln_swapped').items())
    e_lo = '%.3E' % float(g[tag + '_E'][1])
    for splits in (1, 8):
        write_db(str(tmp / ('%s_pref_%d' % (tag, splits))), pref, 7, splits=splits)
        write_db(str(tmp / ('%s_aln_%d' % (tag, splits))), aln, 5, splits=splits)
    for threads, splits in ((1, 1), (8, 1), (8, 8)):
        out = str(tmp / ('%s_ps_%d_%d' % (tag, threads, splits)))
        sdgpu('swapresults', seq_db, prof_db, tmp / ('%s_pref_%d' % (tag, splits)), out, '--threads', threads, '-v', '0')
        assert read_db(out) == swapgold.db(tag + '_pref_swapped'), (threads, splits)
        assert open(out + '.dbtype', 'rb').read() == b'\x07\x00\x00\x00'
        out = str(tmp / ('%s_fin_%d_%d' % (tag, threads, splits)))
        sdgpu('swapresults', prof_db, seq_db, tmp / ('%s_aln_%d' % (tag, splits)), out, '--threads', threads, '-v', '0', '-e', e_lo,
              '--sub-mat', 'aa:blosum62.out,nucl:nucleotide.out', '--gap-open', 'aa:11,nucl:5', '--gap-extend', 'aa:1,nucl:2',
              '--split-memory-limit', '0', '--compressed', '0', '--db-load-mode', '0')
        assert read_db(out) == swapgold.db(tag + '_final_1'), (threads, splits)
        assert open(out + '.dbtype', 'rb').read() == b'\x05\x00\x00\x00'


def test_module_refusals(dbs):
    tmp, seq_db, prof_db = dbs
    write_db(str(tmp / 'one'), [(0, b'1\t50\t1\n')], 7)
    p = sdgpu('swapresults', seq_db, prof_db, tmp / 'one', tmp / 'r1', '--gap-open', 'aa:10,nucl:5', check=False)
    assert p.returncode != 0 and 'gap costs' in p.stderr
    p = sdgpu('swapresults', seq_db, prof_db, tmp / 'one', check=False)
    assert p.returncode != 0 and 'usage: swapresults' in p.stderr
    write_db(str(tmp / 'far'), [(0, b'99\t50\t1\n')], 7)
    p = sdgpu('swapresults', seq_db, prof_db, tmp / 'far', tmp / 'r2', check=False)
    assert p.returncode != 0 and 'Invalid result record' in p.stderr


def test_help_names_the_module():
    assert 'swapresults' in sdgpu('--help').stdout
