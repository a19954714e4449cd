"""CPU: the restatement tests/clusthash_ref.py and the host stages of `clusthash` (sd_host_clusthash_min_identical,
sd_host_clusthash_format, the byte -> reduced code table) against what tools/make_golden_clusthash.py recorded from the reference's own
object code (tests/golden/clusthash_vectors.npz)."""
import ctypes as C
import functools

import numpy as np
import pytest

import chgold
import clusthash_ref as ref
from dbutil import sdgpu
from spacedust_amd import _lib, api

T_THRESHOLDS = (0.99, 0.9, 0.5, 1.0, 0.0)


@functools.lru_cache(None)
def restated(tag):
    name = tag.split('_')[0]
    let, off = chgold.sequences(name)
    return ref.clusthash(let, off, chgold.byte_map(tag), chgold.par(tag)[1])


@pytest.mark.parametrize('tag', chgold.ALL_RUNS)
def test_restatement_equals_the_reference(tag):
    name = tag.split('_')[0]
    found_by, identical, h, stats = restated(tag)
    assert np.array_equal(h, chgold.hashes(tag))
    assert ref.entries(chgold.keys(name), chgold.sequences(name)[1], found_by, identical) == chgold.entries(tag)
    assert stats['unique_hashes'] == chgold.unique(tag)


def test_hash_is_the_loop():
    let, off = chgold.sequences('S')
    off = off.astype(np.int64)
    m = chgold.byte_map('S_r0')
    h = chgold.hashes('S_r0')
    for s in range(0, len(h), 7):
        assert ref.hash_one(m[let[off[s]:off[s + 1]]]) == int(h[s])


def test_byte_tables_equal_the_reference():
    aa2num = np.asarray(api.Host().matrix(0)[2], np.uint8)
    seen = set()
    for tag in chgold.ALL_RUNS:
        size = chgold.par(tag)[0]
        lmap, reduced = api.reduced_alphabet(size)
        # (byte 255 is the reference's "no letter" mark and no byte of a sequence DB)
        assert reduced == size and np.array_equal(lmap[aa2num][:255], chgold.byte_map(tag)[:255])
        seen.add(size)
    assert seen == {3, 13}


def test_min_identical_equals_the_float_comparison():
    for thr in T_THRESHOLDS + (0.995, 1.5, -0.5, 1e-9):
        for length in range(1, 301):
            got = api.clusthash_min_identical(thr, length)
            passes = [ref.reaches(d, length, thr) for d in range(length + 1)]
            # monotone in d: the integer states the comparison for every d
            assert passes == [d >= got for d in range(length + 1)], (thr, length, got)
        assert api.clusthash_min_identical(thr, 0) == 1   # 0 / 0 is not >= anything
    assert api.clusthash_min_identical(float('nan'), 10) == 11
    for length in (100, 101, 200, 1000, 65535, 1 << 24, (1 << 24) + 1, (1 << 30) - 1):
        for thr in T_THRESHOLDS:
            got = api.clusthash_min_identical(thr, length)
            assert (got == 0 or not ref.reaches(got - 1, length, thr)) and (got == length + 1 or ref.reaches(got, length, thr))


@pytest.mark.parametrize('tag', chgold.ALL_RUNS)
def test_format_equals_the_reference(tag):
    name = tag.split('_')[0]
    found_by, identical, _, _ = restated(tag)
    assert api.clusthash_format(chgold.keys(name), chgold.sequences(name)[1], found_by, identical) == chgold.entries(tag)


def test_format_of_short_and_empty_sequences():
    # L = 0: "L - 1" is unsigned int arithmetic; L = 1: the only identities are 0 and 1
    off = np.array([0, 0, 1, 2, 2], np.uint64)
    found_by = np.array([ref.NONE, ref.NONE, 1, ref.NONE], np.uint32)
    identical = np.array([0, 0, 1, 0], np.uint32)
    keys = np.array([4, 9, 11, 4000000000], np.uint32)
    got = api.clusthash_format(keys, off, found_by, identical)
    assert got == ref.entries(keys, off, found_by, identical)
    assert got[4] == b'4\t255\t1.00\t0\t0\t4294967295\t0\t0\t4294967295\t0\n'
    assert got[9] == b'9\t255\t1.00\t0\t0\t0\t1\t0\t0\t1\n11\t255\t1.000\t0\t0\t0\t1\t0\t0\t1\n'
    assert got[4000000000] == b'4000000000\t255\t1.00\t0\t0\t4294967295\t0\t0\t4294967295\t0\n'
    # recorded: the two empty sequences of S and a sequence of one residue with its twin
    want = chgold.entries('S_r0')
    i = chgold.class_seq('S', 'length_0')
    assert want[int(chgold.keys('S')[i])].endswith(b'\t4294967295\t0\t0\t4294967295\t0\n')
    # a found-by that is no sequence
    bad = np.array([7], np.uint32)
    rc = _lib.load().sd_host_clusthash_format(1, _lib.ptr(keys), _lib.ptr(off), _lib.ptr(bad), _lib.ptr(identical), None, 0, None,
                                              C.byref(C.c_uint64()))
    assert rc == _lib.SD_EINVAL


def test_symbols_are_exported():
    L = _lib.load()
    for name in ('sd_clusthash_batch', 'sd_host_clusthash_min_identical', 'sd_host_clusthash_format'):
        assert name in _lib.DECLARED_SYMBOLS and hasattr(L, name)


def test_help_lists_the_module():
    assert 'clusthash' in sdgpu('--help').stdout
