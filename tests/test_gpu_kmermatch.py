"""GPU: sd_kmermatch_batch against the hits the reference's own object code recorded (tests/golden/kmermatch_vectors.npz) and against the
restatement tests/kmm_ref.py at the device sort's tile boundary, `sdgpu kmermatcher` against the recorded prefilter DBs, and the chain
kmermatcher -> rescorediagonal -> clust."""
import functools

import numpy as np
import pytest

import kmm_ref
import kmmgold
from dbutil import read_db, sdgpu
from spacedust_amd import _lib, api
from spacedust_amd._lib import ptr

pytestmark = pytest.mark.gpu


def printed(diag):
    """a diagonal as the prefilter DB prints it: through a short"""
    return ((np.asarray(diag, np.int64) + 32768) & 0xFFFF) - 32768


@functools.lru_cache(None)
def restated(tag):
    res, off = kmmgold.sequences(tag.split('_')[0])
    hits, stats, _ = kmm_ref.kmermatch(kmmgold.par(tag), res, off, kmmgold.keys(tag), kmmgold.letter_map(tag))
    return hits, stats


def as_rows(rep, mem, score, diag):
    return np.stack([rep.astype(np.int64), mem.astype(np.int64), score.astype(np.int64), diag.astype(np.int64)], axis=1).reshape(-1, 4)


@pytest.mark.parametrize('tag', kmmgold.SMALL_RUNS)
def test_hits_equal_the_reference(gpu, tag):
    res, off = kmmgold.sequences(tag.split('_')[0])
    rep, mem, score, diag, stats = api.kmermatch(gpu, kmmgold.api_par(kmmgold.par(tag)), res, off, kmmgold.keys(tag))
    want = kmmgold.hits_of(kmmgold.entries(tag))
    got = as_rows(rep, mem, score, printed(diag))
    assert (len(want) > 0) == (tag != 'S_r3') and np.array_equal(got, want)   # (S_r3: --kmer-per-seq 1, identity records alone)
    assert stats == restated(tag)[1]


def tile_set(n_records, seed):
    """related sequences whose records after selection number n_records: 204 of (mostly) 20 records each and short ones with the rest"""
    rng = np.random.default_rng(seed)
    seqs = []
    for f in range(34):
        root = rng.integers(0, 20, int(rng.integers(60, 200))).astype(np.uint8)
        for m in range(6):
            s = root.copy()
            hit = rng.random(len(s)) < 0.06
            s[hit] = rng.integers(0, 20, int(hit.sum()))
            seqs.append(s[:max(40, int(len(s) * rng.uniform(0.8, 1.0)))])
    flat = lambda: (np.concatenate(seqs), np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64))
    # (a sequence gives fewer than 20 records where the last-bin rule drops windows: counted, not assumed)
    rest = n_records - int(kmm_ref.records(kmm_ref.params(k=10), *flat(), np.arange(len(seqs)), api.reduced_alphabet(13)[0])[4][-1])
    while rest > 20:
        seqs.append(rng.integers(0, 20, 20).astype(np.uint8))   # 11 windows, all taken, and the identity record
        rest -= 12
    assert 1 <= rest <= 20
    seqs.append(rng.integers(0, 20, 10 + rest - 2).astype(np.uint8))   # rest - 1 windows, all taken
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), off, rng.permutation(len(seqs)).astype(np.uint32)


@pytest.mark.parametrize('n_records', [4095, 4096, 4097])
def test_hits_equal_the_restatement_at_the_sort_tile(gpu, n_records):
    res, off, keys = tile_set(n_records, n_records)
    p = kmm_ref.params(k=10)
    want, want_stats, _ = kmm_ref.kmermatch(p, res, off, keys, api.reduced_alphabet(13)[0])
    rep, mem, score, diag, stats = api.kmermatch(gpu, kmmgold.api_par(p), res, off, keys, cap=len(want) + 5)   # (room to spare: one call)
    assert stats['records'] == n_records and len(want) > 100
    assert np.array_equal(as_rows(rep, mem, score, diag), want) and stats == want_stats


def test_count_only_and_too_small_a_capacity(gpu):
    L = _lib.load()
    tag = 'A_r0'
    res, off = kmmgold.sequences('A')
    keys, lmap, par = kmmgold.keys(tag), kmmgold.letter_map(tag), kmmgold.api_par(kmmgold.par(tag))
    want, want_stats = restated(tag)
    stats = np.zeros(4, np.uint64)
    import ctypes as C
    rc = L.sd_kmermatch_batch(gpu.h, C.byref(par), len(keys), ptr(res), ptr(off), ptr(keys), ptr(lmap), 0, None, None, None, None, ptr(stats))
    assert rc == _lib.SD_ENOMEM and stats.tolist() == [want_stats[k] for k in ('records', 'grouped', 'hits', 'largest_group')]
    h = len(want)
    out = [np.full(h, 77, np.uint32) for _ in range(3)] + [np.full(h, 77, np.int32)]
    stats[:] = 0
    rc = L.sd_kmermatch_batch(gpu.h, C.byref(par), len(keys), ptr(res), ptr(off), ptr(keys), ptr(lmap), h - 1, *[ptr(a) for a in out], ptr(stats))
    assert rc == _lib.SD_ENOMEM and 'room for %d' % (h - 1) in L.sd_last_error(gpu.h).decode() and int(stats[2]) == h
    assert all((a == 77).all() for a in out)
    rc = L.sd_kmermatch_batch(gpu.h, C.byref(par), len(keys), ptr(res), ptr(off), ptr(keys), ptr(lmap), h, *[ptr(a) for a in out], ptr(stats))
    assert rc == 0 and np.array_equal(as_rows(*out), want)
    # no sequence, and sequences without a shared k-mer: no hit, SD_OK in the count-only form too
    rc = L.sd_kmermatch_batch(gpu.h, C.byref(par), 0, None, ptr(np.zeros(1, np.uint64)), None, ptr(lmap), 0, None, None, None, None, ptr(stats))
    assert rc == 0 and stats.tolist() == [0, 0, 0, 0]
    two = np.random.default_rng(5).integers(0, 20, 40).astype(np.uint8)
    rc = L.sd_kmermatch_batch(gpu.h, C.byref(par), 2, ptr(two), ptr(np.array([0, 25, 40], np.uint64)), ptr(np.array([4, 9], np.uint32)), ptr(lmap), 0,
                              None, None, None, None, ptr(stats))
    assert rc == 0 and stats.tolist() == [2 + 16 + 6, 0, 0, 1]
    bad = two.copy()
    bad[7] = 21
    rc = L.sd_kmermatch_batch(gpu.h, C.byref(par), 2, ptr(bad), ptr(np.array([0, 25, 40], np.uint64)), ptr(np.array([4, 9], np.uint32)), ptr(lmap), 0,
                              None, None, None, None, ptr(stats))
    assert rc == _lib.SD_EINVAL and 'residue 7 has code 21' in L.sd_last_error(gpu.h).decode()


def test_sets_in_one_call_give_the_same_entries(gpu):
    """S, G, H, A and W (their runs at the defaults with k 10) concatenated in shuffled order with the keys moved apart: the 32 767-residue
    sequence of W beside the hub of H in one sort"""
    res, lens, keys, want, base = [], [], [], {}, 0
    for name, tag in (('S', 'S_r0'), ('G', 'G_r0'), ('H', 'H_r0'), ('A', 'A_r0'), ('W', 'W_r1')):
        r, o = kmmgold.sequences(name)
        k = kmmgold.keys(tag).astype(np.int64)
        res.append(r)
        lens.append(np.diff(o.astype(np.int64)))
        keys.append(k + base)
        for key, text in kmmgold.entries(tag).items():
            rows = [line.split(b'\t') for line in text.splitlines()]
            want[key + base] = b''.join(b'%d\t%s\t%s\n' % (int(c[0]) + base, c[1], c[2]) for c in rows)
        base += int(k.max()) + 1000
    res, lens, keys = np.concatenate(res), np.concatenate(lens), np.concatenate(keys)
    off = np.concatenate([[0], np.cumsum(lens)])
    perm = np.random.default_rng(3).permutation(len(keys))
    res2 = np.concatenate([res[off[i]:off[i + 1]] for i in perm])
    off2 = np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.uint64)
    keys2 = keys[perm].astype(np.uint32)
    rep, mem, score, diag, stats = api.kmermatch(gpu, kmmgold.api_par(kmmgold.par('S_r0')), res2, off2, keys2)
    assert api.kmermatch_format(keys2, rep, mem, score, diag) == want
    assert stats['largest_group'] == 5000


@pytest.mark.parametrize('tag', ['C1_r0', 'G_r0', 'G_r1', 'G_r4', 'W_r0'])
def test_module_equals_the_reference(tmp_path, tag):
    p = kmmgold.par(tag)
    seq = kmmgold.write_seq_db(tmp_path, tag.split('_')[0], tag)
    out = str(tmp_path / 'pref')
    flags = ['-k', 0 if tag == 'C1_r0' else p['k'], '--alph-size', p['alph_size'], '--cov-mode', p['cov_mode'], '-c', p['c'],
             '--kmer-per-seq-scale', p['kmer_per_seq_scale'], '--include-only-extendable', int(p['include_only_extendable'])]
    sdgpu('kmermatcher', seq, out, *flags, '--threads', '4', '-v', '0')
    assert read_db(out) == kmmgold.entries(tag)
    assert open(out + '.dbtype', 'rb').read() == b'\x07\x00\x00\x00'
    index_keys = [int(line.split()[0]) for line in open(out + '.index')]
    assert index_keys == sorted(index_keys)


def test_kmermatcher_rescorediagonal_clust(tmp_path):
    """the head of linclust on the 5 898 example proteins: all three run, and every sequence lands in exactly one cluster"""
    seq = kmmgold.write_seq_db(tmp_path, 'C1', 'C1_r0')
    common = ['--threads', '8', '-v', '0']
    sdgpu('kmermatcher', seq, tmp_path / 'pref', *common)
    sdgpu('rescorediagonal', seq, seq, tmp_path / 'pref', tmp_path / 'resc', '--rescore-mode', '0', '-c', '0.8', '--cov-mode', '0', '--min-seq-id', '0.5',
          *common)
    sdgpu('clust', seq, tmp_path / 'resc', tmp_path / 'clu', *common)
    clu = read_db(str(tmp_path / 'clu'))
    members = sorted(int(l) for text in clu.values() for l in text.splitlines())
    assert members == list(range(5898))
    assert all(int(text.split(b'\n')[0]) == rep for rep, text in clu.items())
    assert sum(text.count(b'\n') > 1 for text in clu.values()) >= 10   # clusters of more than one member
