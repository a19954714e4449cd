"""GPU: the kmermatcher's device stages one by one.  The records that km_select_kernel and km_emit_kernel leave (sd_selftest_kmermatch_records:
the function sd_kmermatch_batch itself starts with) against the records the reference's own object code emitted
(tests/golden/kmermatch_vectors.npz, kmermatch_edges.npz) and, on a grid of lengths around the wavefront's 64-window chunks and 64 lane
blocks that nothing records, against the restatement tests/kmm_ref.py; the widths of the two chained sorts through the hits, with the longest
sequence on either side of a power of two and keys up to 2^32 - 1.  Every comparison is equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmm_ref
import kmmgold
from spacedust_amd import _lib, api
from spacedust_amd._lib import ptr

pytestmark = pytest.mark.gpu


def as_rows(rep, mem, score, diag):
    return np.stack([rep.astype(np.int64), mem.astype(np.int64), score.astype(np.int64), diag.astype(np.int64)], axis=1).reshape(-1, 4)


@functools.lru_cache(None)
def selection(tag):
    """(considered, threshold, excess) int64 [n, 3] of every sequence of a recorded run, from kmm_ref.selection_info"""
    res, off = kmmgold.sequences(tag.split('_')[0])
    off = off.astype(np.int64)
    par, lmap = kmmgold.par(tag), kmmgold.letter_map(tag)
    return np.array([kmm_ref.selection_info(par, res[off[i]:off[i + 1]], lmap)[1:4] for i in range(len(off) - 1)], np.int64).reshape(-1, 3)


def assert_records_are_the_recorded_ones(got, tag):
    res, off = kmmgold.sequences(tag.split('_')[0])
    keys = kmmgold.keys(tag)
    want_key, want_pos, want_off = kmmgold.records(tag)
    rec_off = got['rec_off'].astype(np.int64)
    count = np.diff(rec_off)
    # the reference read the sequences in key order: its emission order is the device's, sequence by sequence in that order
    order = np.argsort(keys, kind='stable')
    assert np.array_equal(np.concatenate([[0], np.cumsum(count[order])]), want_off.astype(np.int64))
    pick = np.concatenate([np.arange(rec_off[i], rec_off[i + 1]) for i in order])
    assert len(pick) == len(want_key) == len(got['key'])
    assert np.array_equal(got['key'][pick], want_key) and np.array_equal(got['pos'][pick].astype(np.int64), want_pos.astype(np.int64))
    assert np.array_equal(got['id'], np.repeat(keys, count)) and np.array_equal(got['len'], np.repeat(np.diff(off.astype(np.int64)), count))
    want = selection(tag)
    assert np.array_equal(got['considered'], want[:, 0]) and np.array_equal(got['threshold'], want[:, 1])
    assert np.array_equal(got['excess'], want[:, 2])


@pytest.mark.parametrize('tag', kmmgold.SMALL_RUNS)
def test_records_equal_the_reference(gpu, tag):
    res, off = kmmgold.sequences(tag.split('_')[0])
    got = api.kmermatch_records(gpu, kmmgold.api_par(kmmgold.par(tag)), res, off, kmmgold.keys(tag))
    assert len(got['key']) > len(kmmgold.keys(tag)) or tag == 'S_r3'   # (S_r3: --kmer-per-seq 1, identity records alone)
    assert_records_are_the_recorded_ones(got, tag)


# ---- a lane grid that nothing records -------------------------------------------------------------------------------------------------
def grid_lengths(k):
    return sorted({0, 1, k - 1, k, 63, 64, 65, k + 62, k + 63, k + 64, 127, 128, 129, 4 * 64 + k - 1})


def letter_map_of(alph_size):
    if alph_size == 5:   # hand-made: twenty letters onto four codes, X the fifth
        return np.array([i % 4 for i in range(20)] + [4], np.uint8)
    return api.reduced_alphabet(alph_size)[0]


# (k, alphabet, --kmer-per-seq, --kmer-per-seq-scale, --hash-shift): few different windows at k 1 and 2 and on four codes, so that score
# bins hold many equal windows; more than a chunk of windows considered at (2, 13) and (18, 13); 18 the largest k whose powers of 12 fit
# 64 bits, the index itself wraps as the reference's does
GRID = [(1, 21, 20, 0.0, 67), (2, 13, 70, 0.0, 67), (10, 13, 20, 0.3, 67), (18, 13, 100, 0.0, -3), (24, 5, 20, 0.5, 67)]


@pytest.mark.parametrize('k,alph_size,kmer_per_seq,scale,hash_shift', GRID)
def test_records_equal_the_restatement_on_the_lane_grid(gpu, k, alph_size, kmer_per_seq, scale, hash_shift):
    rng = np.random.default_rng(1000 * k + alph_size)
    seqs = []
    for length in grid_lengths(k):
        seqs.append(rng.integers(0, 20, length).astype(np.uint8))                  # no X
        s = rng.integers(0, 20, length).astype(np.uint8)
        s[rng.random(length) < 0.03] = 20                                           # X here and there
        seqs.append(s)
        s = rng.integers(0, 20, length).astype(np.uint8)
        s[np.array([x for x in (0, 63, 64, 64 + k - 1, length - 1) if 0 <= x < length], np.int64)] = 20   # X at the ends and on the chunk edge
        seqs.append(s)
        seqs.append(np.tile(rng.integers(0, 20, 3).astype(np.uint8), length // 3 + 1)[:length])   # a period-3 repeat
    res = np.concatenate(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    keys = (5 + 13 * rng.permutation(len(seqs))).astype(np.uint32)
    par = kmm_ref.params(k=k, alph_size=alph_size, kmer_per_seq=kmer_per_seq, kmer_per_seq_scale=scale, hash_shift=hash_shift)
    lmap = letter_map_of(alph_size)
    want_key, want_id, want_len, want_pos, want_off = kmm_ref.records(par, res, off, keys, lmap)
    info = np.array([kmm_ref.selection_info(par, s, lmap) for s in seqs], np.int64)
    # the grid is what it is meant to be: sequences without a window, with all windows taken, with a choice, and with an excess
    assert (info[:, 0] == 0).any() and ((info[:, 0] > 0) & (info[:, 1] == info[:, 0])).any() and (info[:, 1] < info[:, 0]).any()
    assert (info[:, 3] > 0).any() and len(want_key) > 3 * len(seqs)
    got = api.kmermatch_records(gpu, kmmgold.api_par(par), res, off, keys, letter_map=lmap)
    assert np.array_equal(got['rec_off'].astype(np.int64), want_off)
    assert np.array_equal(got['key'], want_key) and np.array_equal(got['pos'].astype(np.int64), want_pos)
    assert np.array_equal(got['id'], want_id) and np.array_equal(got['len'].astype(np.int64), want_len)
    assert np.array_equal(got['considered'], info[:, 1]) and np.array_equal(got['threshold'], info[:, 2])
    assert np.array_equal(got['excess'], info[:, 3])


# ---- capacity ---------------------------------------------------------------------------------------------------------------------------
def test_records_capacity(gpu):
    L = _lib.load()
    tag = 'E_r1'
    res, off = kmmgold.sequences('E')
    keys, lmap, par = kmmgold.keys(tag), kmmgold.letter_map(tag), kmmgold.api_par(kmmgold.par(tag))
    n, r = len(keys), len(kmmgold.records(tag)[0])
    per_seq = [np.full(n, 77, np.uint32) for _ in range(3)] + [np.full(n + 1, 77, np.uint64)]
    per_rec = [np.full(r, 77, np.uint64)] + [np.full(r, 77, np.uint32) for _ in range(3)]
    stats = np.zeros(1, np.uint64)
    call = lambda cap: L.sd_selftest_kmermatch_records(gpu.h, C.byref(par), n, ptr(res), ptr(off), ptr(keys), ptr(lmap), cap,
                                                       *[ptr(a) for a in per_seq + per_rec], ptr(stats))
    assert call(r - 1) == _lib.SD_ENOMEM and int(stats[0]) == r and 'room for %d' % (r - 1) in L.sd_last_error(gpu.h).decode()
    assert all((a == 77).all() for a in per_seq + per_rec)
    stats[:] = 0
    assert call(r) == 0 and int(stats[0]) == r
    got = dict(zip(('considered', 'threshold', 'excess', 'rec_off', 'key', 'id', 'len', 'pos'), per_seq + per_rec))
    assert_records_are_the_recorded_ones(got, tag)


# ---- the widths of the chained sorts, through the hits ---------------------------------------------------------------------------------
SPECIAL_KEYS = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]


def width_set(longest, seed):
    """families of related sequences, the longest of `longest` residues; members shorter than half of it (the first sort's seqLen field
    uses its top bit), members that begin later or earlier than their root (diagonals of both signs) and members that do both (both signs
    inside one pair, for the second sort's biased field)"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: rng.integers(0, 20, n).astype(np.uint8)
    seqs = []
    for f in range(14):
        n = longest if f < 2 else int(rng.integers(longest // 2 + 10, longest + 1))
        root = rnd(n)
        mid = n // 2
        seqs += [root, root[7:].copy(), np.concatenate([rnd(6), root[:n - 9]]), root[n // 4:n // 4 + int(0.4 * n)].copy(),
                 np.concatenate([root[5:mid], rnd(9), root[mid:n - 8]]), root[:n - 1 - f].copy()]
    keys = np.array(SPECIAL_KEYS + rng.choice(np.arange(2, 2 ** 32 - 2, 4099), len(seqs) - len(SPECIAL_KEYS), replace=False).tolist(), np.uint64)
    keys = rng.permutation(keys).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return np.concatenate(seqs), off, keys


@pytest.mark.parametrize('longest', [127, 128, 255, 256, 257, 511])
def test_hits_equal_the_restatement_around_a_sort_width(gpu, longest):
    res, off, keys = width_set(longest, longest)
    lens = np.diff(off.astype(np.int64))
    assert int(lens.max()) == longest and int(lens.min()) < longest // 2 and len(set(keys.tolist())) == len(keys)
    assert set(SPECIAL_KEYS) <= set(keys.tolist())
    p = kmm_ref.params(k=10, kmer_per_seq=60)
    want, want_stats, _ = kmm_ref.kmermatch(p, res, off, keys, api.reduced_alphabet(13)[0])
    # an empty or one-sided result cannot pass
    assert len(want) > 50 and (want[:, 3] < 0).any() and (want[:, 3] > 0).any()
    rep, mem, score, diag, stats = api.kmermatch(gpu, kmmgold.api_par(p), res, off, keys)
    assert np.array_equal(as_rows(rep, mem, score, diag), want) and stats == want_stats


@pytest.mark.parametrize('cov_mode', [3, 4, 5])
def test_only_extendable_under_the_range_coverage_modes(gpu, cov_mode):
    """--cov-mode 3, 4 and 5 with --include-only-extendable 1 on set G (without it the recorded runs G_r6 .. G_r8 hold them against the
    reference in test_gpu_kmermatch.py): the coverage rule is then not asked at all"""
    res, off = kmmgold.sequences('G')
    keys = kmmgold.keys('G_r0')
    p = kmm_ref.params(k=10, cov_mode=cov_mode, c=0.8, include_only_extendable=True)
    want, want_stats, _ = kmm_ref.kmermatch(p, res, off, keys, kmmgold.letter_map('G_r0'))
    assert len(want) > 0
    rep, mem, score, diag, stats = api.kmermatch(gpu, kmmgold.api_par(p), res, off, keys)
    assert np.array_equal(as_rows(rep, mem, score, diag), want) and stats == want_stats
