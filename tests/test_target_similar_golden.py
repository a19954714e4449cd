"""CPU: the golden file of `--target-search-mode 1` (tools/make_golden_target_similar.py, the reference's own IndexTable, KmerGenerator
and QueryMatcher) holds the conditions that make it worth pinning; a plain restatement of the sequence form of generateKmerList gives the
same index; the library declares and exports sd_target_build_similar; and the modules refuse, without a device, what the mode does not
cover -- each by its words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tsim
from dbutil import sdgpu, write_db
from spacedust_amd import _lib
from spacedust_amd._lib import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _windows(off):
    return np.maximum(np.diff(off.astype(np.int64)) - tsim.SPAN + 1, 0)


def test_full_index_sets_are_consistent_and_ordered(host):
    g = tsim.golden()
    for name in ('S', 'R'):
        t = g[name + '_triples'].astype(np.int64)
        wl = g[name + '_window_len'].astype(np.int64)
        assert len(wl) == int(_windows(g[name + '_off']).sum())
        assert int(wl.sum()) == int(g[name + '_records']) >= len(t) > 0
        # index order: ascending k-mer; inside a list ascending (target, position), a target at most once
        key = (t[:, 0] << 40) | (t[:, 1] << 16) | t[:, 2]
        assert (np.diff(key) > 0).all()
        assert len(np.unique((t[:, 0] << 24) | t[:, 1])) == len(t)
        # the lookup is the sequence as it came: nothing masked
        assert np.array_equal(g[name + '_lookup'], host.map_sequences(tsim.seqs_of(name))[0])
    # S: a sequence shorter than the window, windows with X, and a window without X whose list is empty at the threshold
    lens = np.diff(g['S_off'].astype(np.int64)).tolist()
    assert lens == [7, 12, 25, 40] and tsim.seqs_of('S')[2].count('X') == 2
    assert int(g['S_empty_plain_windows']) >= 1 and int(g['S_thr']) > 112
    wl = g['S_window_len'].astype(np.int64)
    plain = np.array([tsim.windows_without_x(s[i:i + tsim.SPAN]) == 1 for s in tsim.seqs_of('S') for i in range(len(s) - tsim.SPAN + 1)])
    assert len(plain) == len(wl) and (wl[~plain] == 0).all() and (~plain).sum() > 0
    assert int((wl[plain] == 0).sum()) == int(g['S_empty_plain_windows']) and (wl[plain] > 0).any()


@pytest.mark.parametrize('name', ['S', 'R'])
def test_restated_generator_gives_the_reference_index(host, name):
    """the 3-mer x 3-mer product with the `short` cutoffs, the dedupe at the smallest position and the order, restated in numpy"""
    g = tsim.golden()
    t, wl, records = tsim.restated_index(host, tsim.seqs_of(name), int(g[name + '_thr']))
    assert np.array_equal(wl, g[name + '_window_len'].astype(np.int64)) and records == int(g[name + '_records'])
    assert np.array_equal(t, g[name + '_triples'].astype(np.int64))


def test_repeat_set_keeps_the_smaller_position():
    g = tsim.golden()
    t = g['R_triples'].astype(np.int64)
    wl = g['R_window_len'].astype(np.int64)
    p1, p2 = (int(x) for x in g['R_copies'])
    # the segment twice in target 0 (50 residues, 41 windows) and alone as target 1 (7 windows): equal lists
    assert len(wl) == 48 and (wl[p1:p1 + 7] == wl[p2:p2 + 7]).all() and (wl[41:] == wl[p1:p1 + 7]).all() and int(wl[p1:p1 + 7].sum()) > 0
    assert int(g['R_removed']) == int(g['R_records']) - len(t) >= int(wl[p2:p2 + 7].sum())
    # every k-mer of the second copy's windows is in the list of the window 21 positions before it: target 0 keeps none at p2 .. p2 + 6
    t0 = t[t[:, 1] == 0]
    assert not ((t0[:, 2] >= p2) & (t0[:, 2] < p2 + 7)).any() and ((t0[:, 2] >= p1) & (t0[:, 2] < p1 + 7)).any()
    # the second target holds the same k-mers at its own positions
    t1 = t[t[:, 1] == 1]
    assert len(t1) > 0 and set(t1[:, 0].tolist()) <= set(t0[:, 0].tolist())


def test_big_and_g_sets_hold_their_conditions(host):
    g = tsim.golden()
    assert int(g['B_window_len'].max()) > 65536 and int(g['B_window_len'].max()) < (1 << 23) and int(g['B_thr']) < 112
    assert int(g['B_window_len'].sum()) == int(g['B_records']) >= int(g['B_entries']) > 0
    assert host.kmer_threshold(5.7, 6) == 112 == int(g['G_thr'])
    assert len(g['G_off']) - 1 == 36 and len(g['Q_off']) - 1 == 42
    assert int(g['G_per_target'].sum()) == int(g['G_entries']) <= int(g['G_records'])
    assert 0 < int(g['G_lists']) <= int(g['G_entries']) and len(str(g['G_digest'])) == 64
    queries = tsim.seqs_of('Q')
    for i, q in enumerate(g['Q_x_of']):
        a, b = queries[36 + i], queries[int(q)]
        assert len(a) == len(b) and 1 <= a.count('X') - b.count('X') <= 3
    for name in ('rows_bias1', 'rows_bias0'):
        r = g[name].astype(np.int64)
        assert np.array_equal(g[name + '_kmers'], [tsim.windows_without_x(q) for q in queries])   # the reference's kmerListLen
        same = r[1:, 0] == r[:-1, 0]
        assert (np.diff(r[:, 0]) >= 0).all()
        assert ((r[1:, 2] < r[:-1, 2]) | ((r[1:, 2] == r[:-1, 2]) & (r[1:, 1] > r[:-1, 1])))[same].all()
        assert (r[:, 2] >= 15).all() and (r[:, 1] < 36).all() and len(r) >= 36
        pl = r[r[:, 0] < 36]   # query i is member 2 + i % 2 of family i // 2, target t member t % 2 of family t // 2
        assert (pl[:, 1] // 2 != pl[:, 0] // 2).any() and (pl[:, 1] // 2 == pl[:, 0] // 2).any()
    assert not np.array_equal(g['rows_bias1'], g['rows_bias0'])
    # mode 1 is not mode 0: a run of the regular index cannot pass for it
    m1 = g['rows_bias1'].astype(np.int64).copy()
    m1[:, 3] = m1[:, 3].astype(np.int16)
    assert not np.array_equal(m1, g['rows_mode0'].astype(np.int64))
    # set M: tantan would mask the probe, the branch does not
    assert int(g['M_masked_by_tantan']) > 0 and int(g['M_entries']) > 0


def test_symbol_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'spacedust_gpu.h')).read()
    assert re.search(r'\bint\s+sd_target_build_similar\s*\(', hdr)
    assert 'sd_target_build_similar' in _lib.DECLARED_SYMBOLS
    L = _lib.load()
    assert hasattr(L, 'sd_target_build_similar') and 'sd_target_build_similar' not in L._sd_missing


def test_null_arguments_are_einval_without_a_device():
    L = _lib.load()
    z8, z16, u16, off = np.zeros(20, np.uint8), np.zeros(16, np.int16), np.zeros(16, np.uint16), np.array([0, 20], np.uint64)
    out = C.c_void_p()
    fake = C.c_void_p(1)   # never dereferenced: the NULL checks come first
    args = [ptr(z8), ptr(off), 1, ptr(z16), ptr(u16)]
    assert L.sd_target_build_similar(None, 6, 112, *args, C.byref(out), None) == _lib.SD_EINVAL
    for drop in (0, 1, 3, 4):
        a = list(args)
        a[drop] = None
        assert L.sd_target_build_similar(fake, 6, 112, *a, C.byref(out), None) == _lib.SD_EINVAL
    assert L.sd_target_build_similar(fake, 6, 112, *args, None, None) == _lib.SD_EINVAL
    assert not out.value


@pytest.fixture(scope='module')
def dbs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('tsm')
    seqs = tsim.seqs_of('G')[:4]
    write_db(str(tmp / 'seq'), [(i, s.encode() + b'\n') for i, s in enumerate(seqs)], 0)
    write_db(str(tmp / 'prof'), [(i, bytes(25 * 30)) for i in range(2)], 2)
    return tmp


def test_module_refusals_without_a_device(dbs):
    seq, prof = dbs / 'seq', dbs / 'prof'
    p = sdgpu('prefilter', seq, seq, dbs / 'o1', '--target-search-mode', '1', '--split', '2', check=False)
    assert p.returncode != 0 and '--split 2: --target-search-mode 1 searches the target unsplit' in p.stderr
    p = sdgpu('prefilter', prof, seq, dbs / 'o2', '--target-search-mode', '1', check=False)
    assert p.returncode != 0 and '--target-search-mode 1 with a profile query database is not implemented' in p.stderr
    p = sdgpu('prefilter', seq, seq, dbs / 'o3', '--target-search-mode', '2', check=False)
    assert p.returncode != 0 and '--target-search-mode 2: 0 (regular k-mer index) or 1 (similar k-mer index)' in p.stderr
    p = sdgpu('createindex', seq, dbs / 'tmp', '--target-search-mode', '1', check=False)
    assert p.returncode != 0 and 'createindex --target-search-mode 1 is not implemented' in p.stderr
    assert not os.path.exists(str(seq) + '.idx')


@pytest.mark.parametrize('workflow', ['search', 'clustersearch'])
def test_workflow_refusals_without_a_device(dbs, workflow):
    seq = dbs / 'seq'
    base = [workflow, seq, seq, dbs / ('w_' + workflow), dbs / ('wt_' + workflow), '--target-search-mode', '1']
    p = sdgpu(*base, '--num-iterations', '2', check=False)
    assert p.returncode != 0 and '--target-search-mode 1 with --num-iterations > 1 is not implemented' in p.stderr
    p = sdgpu(*base, '--prefilter-mode', '1', check=False)
    assert p.returncode != 0 and '--target-search-mode 1 with --prefilter-mode 1' in p.stderr
    p = sdgpu(*base, '--world-size', '2', check=False)
    assert p.returncode != 0 and '--target-search-mode 1 runs on one rank' in p.stderr
    if workflow == 'clustersearch':
        p = sdgpu(*base, '--profile-cluster-search', '1', '--exhaustive-search', '0', check=False)
        assert p.returncode != 0 and '--target-search-mode 1 with --profile-cluster-search 1' in p.stderr
    assert not os.path.exists(str(dbs / ('wt_' + workflow)))


def test_mode_0_is_still_accepted_by_the_parser(dbs):
    """with or without a device: the flag's default value is no reason to refuse"""
    seq = dbs / 'seq'
    p = sdgpu('prefilter', seq, seq, dbs / 'o0', '--target-search-mode', '0', check=False)
    assert 'target-search-mode' not in p.stderr
    assert p.returncode == 0 or 'GPU' in p.stderr or 'device' in p.stderr
