"""CPU: the golden file of the profile-target prefilter (tools/make_golden_target_profile.py, the reference's own IndexTable and
QueryMatcher) holds the conditions that make it worth pinning, and the library declares, exports and guards sd_target_build_profile."""
import ctypes as C
import os
import re

import numpy as np

import tpref
from spacedust_amd import _lib
from spacedust_amd._lib import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _windows(poff_bytes):
    L = np.diff(poff_bytes.astype(np.int64)) // 25
    return np.maximum(L - tpref.SPAN + 1, 0)


def test_full_index_sets_are_consistent_and_ordered():
    g = tpref.golden()
    for name in ('S', 'R'):
        t = g[name + '_triples'].astype(np.int64)
        wl = g[name + '_window_len'].astype(np.int64)
        assert len(wl) == int(_windows(g[name + '_poff']).sum())
        assert int(wl.sum()) == int(g[name + '_records']) >= len(t) > 0
        assert len(g[name + '_lookup']) == int(g[name + '_poff'][-1]) // 25
        # index order: ascending k-mer; inside a list ascending (target, position), a target at most once
        key = (t[:, 0] << 40) | (t[:, 1] << 16) | t[:, 2]
        assert (np.diff(key) > 0).all()
        assert len(np.unique((t[:, 0] << 24) | t[:, 1])) == len(t)
        # the lookup is the consensus column of the profile records
        rec = g[name + '_profiles'].reshape(-1, 25)
        assert (g[name + '_lookup'] == rec[:, 21]).all()
    # S keeps windows whose query letters hold an X (they contribute nothing) beside windows that do
    assert (g['S_window_len'] == 0).any() and (g['S_window_len'] > 0).any()
    assert len(g['S_poff']) - 1 == 3 and sorted((np.diff(g['S_poff'].astype(np.int64)) // 25).tolist()) == [12, 25, 40]


def test_repeat_set_keeps_the_smaller_position():
    g = tpref.golden()
    t = g['R_triples'].astype(np.int64)
    wl = g['R_window_len'].astype(np.int64)
    # the 16-position segment twice: windows p and p + 16 (p < 7) give the same list, so the raw lists hold those k-mers twice
    assert (wl[:7] == wl[16:23]).all() and int(wl[:7].sum()) > 0
    assert len(wl) == 23 and int(g['R_records']) - len(t) >= int(wl[16:23].sum()) > 0
    # one target: every k-mer of the index once.  Every k-mer of a window 16 .. 22 is in the list of the window 16 positions before
    # it, so the duplicated k-mers carry the smaller position: no entry is left at 16 .. 22, and the first windows keep theirs
    assert len(np.unique(t[:, 0])) == len(t)
    assert not (t[:, 2] >= 16).any()
    cnt = np.bincount(t[:, 2], minlength=23)
    assert (cnt <= wl).all() and int(cnt[:7].sum()) > 0


def test_big_and_g_sets_hold_their_conditions():
    g = tpref.golden()
    assert len(g['B_profiles']) == 12 * 25 and int(g['B_window_len'].max()) > 65536 and int(g['B_window_len'].max()) < (1 << 23)
    assert int(g['B_window_len'].sum()) == int(g['B_records']) >= int(g['B_entries']) > 0
    _, poff = tpref.g_profiles()
    assert len(poff) - 1 == 18 and int(poff[-1]) // 25 == 5084
    for thr, rows_min in ((110, 60), (95, 140)):
        tag = 'G%d' % thr
        assert int(g[tag + '_per_target'].sum()) == int(g[tag + '_entries']) <= int(g[tag + '_records'])
        assert 0 < int(g[tag + '_lists']) <= int(g[tag + '_entries'])
        assert len(str(g[tag + '_digest'])) == 64
        rows = g['rows_%d_bias1' % thr]
        plain = rows[rows[:, 0] < 144]
        assert len(plain) >= rows_min
        assert (plain[:, 1] != plain[:, 0] // 4).any()   # a row on a target outside the query's own family
        fig = g['rows_%d_bias1_figures' % thr]
        assert fig[0] == len(rows) and fig[1] == len(plain)
    assert int(g['G95_entries']) > int(g['G110_entries'])
    # composition bias changes the diagonal scores: the two row sets at 110 differ
    assert not np.array_equal(g['rows_110_bias1'], g['rows_110_bias0'])
    # queries: the 144 sequences and eight copies with 1 - 3 letters replaced by X, which look up fewer k-mers
    letters, off = tpref.queries()
    assert len(off) - 1 == 152
    for i, q in enumerate(g['Q_x_of']):
        a, b = letters[int(off[144 + i]):int(off[145 + i])], letters[int(off[q]):int(off[q + 1])]
        assert len(a) == len(b) and 1 <= a.count(b'X') - b.count(b'X') <= 3
        for name in ('rows_110_bias1', 'rows_95_bias1', 'rows_110_bias0'):
            km = g[name + '_kmers']
            assert km[144 + i] == tpref.windows_without_x(a) < km[q] == tpref.windows_without_x(b)
    # rows: per query descending score, then ascending target (no identity id: hit_t::compareHitsByScoreAndId over the whole list)
    for name in ('rows_110_bias1', 'rows_95_bias1', 'rows_110_bias0'):
        r = g[name].astype(np.int64)
        same = r[1:, 0] == r[:-1, 0]
        assert (np.diff(r[:, 0]) >= 0).all()
        assert ((r[1:, 2] < r[:-1, 2]) | ((r[1:, 2] == r[:-1, 2]) & (r[1:, 1] > r[:-1, 1])))[same].all()
        assert (r[:, 2] >= 15).all() and (r[:, 1] < 18).all()


def test_symbol_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'spacedust_gpu.h')).read()
    assert re.search(r'\bint\s+sd_target_build_profile\s*\(', hdr)
    assert 'sd_target_build_profile' in _lib.DECLARED_SYMBOLS
    L = _lib.load()
    assert hasattr(L, 'sd_target_build_profile') and 'sd_target_build_profile' not in L._sd_missing


def test_null_arguments_are_einval_without_a_device():
    L = _lib.load()
    z8, z16, off = np.zeros(20, np.uint8), np.zeros(400, np.int16), np.array([0, 20], np.uint64)
    i8 = np.zeros(400, np.uint8)
    out = C.c_void_p()
    fake = C.c_void_p(1)   # never dereferenced: the NULL checks come first
    args = [ptr(z8), ptr(z8), ptr(z16), ptr(i8), ptr(off)]
    assert L.sd_target_build_profile(None, 6, 110, *args, 1, C.byref(out), None) == _lib.SD_EINVAL
    for drop in range(5):
        a = list(args)
        a[drop] = None
        assert L.sd_target_build_profile(fake, 6, 110, *a, 1, C.byref(out), None) == _lib.SD_EINVAL
    assert L.sd_target_build_profile(fake, 6, 110, *args, 1, None, None) == _lib.SD_EINVAL
    assert not out.value
