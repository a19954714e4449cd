"""GPU: sd_clusthash_batch against the hashes and entries the reference's own object code recorded (tests/golden/clusthash_vectors.npz)
and against the restatement tests/clusthash_ref.py around the single-wavefront bound of the group pass, and `sdgpu clusthash` against the
recorded DBs."""
import functools
import re

import numpy as np
import pytest

import chgold
import clusthash_ref as ref
from dbutil import read_db, sdgpu, write_db
from spacedust_amd import _lib, api

pytestmark = pytest.mark.gpu

WAVE_BOUND = 64   # CH_WAVE_BOUND of csrc/hip/sd_clusthash.hip
AA = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', np.uint8)


@functools.lru_cache(None)
def aa2num():
    return np.asarray(api.Host().matrix(0)[2], np.uint8)


@functools.lru_cache(None)
def byte_map(alph):
    return api.reduced_alphabet(alph)[0][aa2num()]


@functools.lru_cache(None)
def restated(tag):
    name = tag.split('_')[0]
    let, off = chgold.sequences(name)
    return ref.clusthash(let, off, chgold.byte_map(tag), chgold.par(tag)[1])


def run(gpu, letters, off, alph=3, thr=0.99):
    letters = np.ascontiguousarray(letters, np.uint8)
    return api.clusthash(gpu, aa2num()[letters], off, letters, alph_size=alph, min_seq_id=thr)


def check_against_restatement(gpu, letters, off, alph=3, thr=0.99):
    found_by, identical, h, stats = run(gpu, letters, off, alph, thr)
    want = ref.clusthash(letters, off, byte_map(alph), thr)
    assert np.array_equal(h, want[2]) and np.array_equal(found_by, want[0]) and np.array_equal(identical, want[1])
    assert stats == want[3]
    return found_by, stats


@pytest.mark.parametrize('tag', chgold.SMALL_RUNS)
def test_equals_the_reference(gpu, tag):
    name = tag.split('_')[0]
    let, off = chgold.sequences(name)
    alph, thr = chgold.par(tag)
    found_by, identical, h, stats = run(gpu, let, off, alph, thr)
    assert np.array_equal(h, chgold.hashes(tag))
    assert ref.entries(chgold.keys(name), off, found_by, identical) == chgold.entries(tag)
    assert api.clusthash_format(chgold.keys(name), off, found_by, identical) == chgold.entries(tag)
    want = restated(tag)
    assert stats == want[3] and stats['unique_hashes'] == chgold.unique(tag)
    assert np.array_equal(found_by, want[0]) and np.array_equal(identical, want[1])


def test_sets_in_one_call_give_the_same_entries(gpu):
    """S, T, G, O, N, H and A at the defaults one behind the other, keys moved apart: every group of every set in one sort and one pass"""
    lets, lens, keys, want, hashes, base = [], [], [], {}, [], 0
    for name in ('S', 'T', 'G', 'O', 'N', 'H', 'A'):
        tag = name + '_r0'
        assert chgold.par(tag) == (3, 0.99)
        let, off = chgold.sequences(name)
        k = chgold.keys(name).astype(np.int64)
        lets.append(let)
        lens.append(np.diff(off.astype(np.int64)))
        keys.append(k + base)
        hashes.append(chgold.hashes(tag))
        for key, text in chgold.entries(tag).items():
            rows = [line.split(b'\t', 1) for line in text.splitlines()]
            want[key + base] = b''.join(b'%d\t%s\n' % (int(c[0]) + base, c[1]) for c in rows)
        base += int(k.max()) + 1000
    let, keys = np.concatenate(lets), np.concatenate(keys).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.uint64)
    found_by, identical, h, stats = run(gpu, let, off)
    assert np.array_equal(h, np.concatenate(hashes))
    assert api.clusthash_format(keys, off, found_by, identical) == want
    assert stats['largest_group'] == 5050


def group(rng, cl_peers, size, length):
    """`size` sequences of one hash and length: a root, and copies with 0 .. 3 letters swapped inside their class of the alphabet of 3"""
    root = AA[rng.integers(0, 20, length)]
    out = [root]
    for _ in range(size - 1):
        s = root.copy()
        for p in rng.permutation(length)[:int(rng.integers(0, 4))]:
            peers = cl_peers[int(root[p])]
            s[p] = peers[int(rng.integers(0, len(peers)))]
        out.append(s)
    return out


@functools.lru_cache(None)
def peers():
    m = byte_map(3)
    return {int(c): [int(d) for d in AA if d != c and m[d] == m[c]] for c in AA}


def flat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.uint8), off


@pytest.mark.parametrize('size', [WAVE_BOUND - 1, WAVE_BOUND, WAVE_BOUND + 1, 2 * WAVE_BOUND + 1, 8 * WAVE_BOUND + 3])
def test_group_sizes_around_the_wavefront_bound(gpu, size):
    """three groups of the size, of lengths on both sides of a 4-byte word and of the 1 024-byte chunk, interleaved with single sequences;
    150 residues at 0.99 ask for 149 equal bytes, so copies are marked in chains"""
    rng = np.random.default_rng(size)
    seqs = []
    for length in (150, 151, 1100):
        seqs += group(rng, peers(), size, length)
    seqs += [AA[rng.integers(0, 20, int(rng.integers(1, 40)))] for _ in range(50)]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    found_by, stats = check_against_restatement(gpu, *flat(seqs))
    assert stats['largest_group'] == size and stats['groups'] >= 3
    # the roots mark their near copies; the copies two and three letters away stay, each a representative with a turn of its own
    assert int((found_by != ref.NONE).sum()) >= size and int((found_by == ref.NONE).sum()) > 53


@pytest.mark.parametrize('n', [0, 1, 2])
def test_few_sequences(gpu, n):
    if n == 0:
        found_by, identical, h, stats = run(gpu, np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        assert len(found_by) == 0 and len(h) == 0 and stats == dict(unique_hashes=0, groups=0, pairs=0, largest_group=0)
        return
    seq = AA[np.random.default_rng(1).integers(0, 20, 90)]
    found_by, stats = check_against_restatement(gpu, *flat([seq] * n))
    assert found_by.tolist() == [ref.NONE, 0][:n] and stats['largest_group'] == n


def test_every_sequence_identical_and_every_sequence_distinct(gpu):
    rng = np.random.default_rng(2)
    seq = AA[rng.integers(0, 20, 333)]
    found_by, stats = check_against_restatement(gpu, *flat([seq] * 300))
    assert found_by.tolist() == [ref.NONE] + [0] * 299 and stats['pairs'] == 299
    found_by, stats = check_against_restatement(gpu, *flat([AA[rng.integers(0, 20, 100 + i % 7)] for i in range(300)]))
    assert (found_by == ref.NONE).all() and stats['unique_hashes'] == 300 and stats['groups'] == 0


def test_refused_parameters(gpu):
    let = AA[np.random.default_rng(3).integers(0, 20, 50)]
    off = np.array([0, 50], np.uint64)
    for alph in (21, 5):   # (the reference refuses 21 itself: no reduced alphabet)
        with pytest.raises(Exception, match='alphabet size %d' % alph):
            api.clusthash(gpu, aa2num()[let], off, let, alph_size=alph, letter_map=np.zeros(21, np.uint8))


@pytest.mark.parametrize('tag', ['A_r0', 'A_r1', 'A_r2', 'A_r3', 'C1_r0'])
def test_module_equals_the_reference(tmp_path, tag):
    name = tag.split('_')[0]
    alph, thr = chgold.par(tag)
    seq = chgold.write_seq_db(tmp_path, name)
    out = str(tmp_path / 'res')
    p = sdgpu('clusthash', seq, out, '--alph-size', alph, '--min-seq-id', thr, '--max-seq-len', 10, '--threads', '4')
    assert read_db(out) == chgold.entries(tag)
    assert int(re.search(r'Found (\d+) unique hashes', p.stdout + p.stderr).group(1)) == chgold.unique(tag)
    assert open(out + '.dbtype', 'rb').read() == b'\x05\x00\x00\x00'
    index_keys = [int(line.split()[0]) for line in open(out + '.index')]
    assert index_keys == sorted(index_keys) == chgold.keys(name).tolist()


def test_module_defaults_are_alphabet_3_and_099(tmp_path):
    seq = chgold.write_seq_db(tmp_path, 'G')
    sdgpu('clusthash', seq, tmp_path / 'res', '-v', '0')
    assert read_db(str(tmp_path / 'res')) == chgold.entries('G_r0')


@pytest.mark.parametrize('dbtype,flags,named', [(1, [], 'nucleotide'), (2, [], 'profile'), (0, ['--alph-size', '5'], '--alph-size 5'),
                                                (0, ['--compressed', '1'], '--compressed 1')])
def test_module_refuses_by_name(tmp_path, dbtype, flags, named):
    seq = str(tmp_path / 'seq')
    write_db(seq, [(0, b'MKVLAAGIVGLLLAQ\n')], dbtype)
    p = sdgpu('clusthash', seq, tmp_path / 'out', *flags, check=False)
    assert p.returncode != 0 and named in p.stderr + p.stdout


def test_module_takes_ids_in_data_order(tmp_path):
    """a DB whose data does not lie in key order: ids follow the data offsets (the reference opens the DB with LINEAR_ACCESS), so the copy
    that lies first marks the other, whatever their keys"""
    rng = np.random.default_rng(4)
    a, b = AA[rng.integers(0, 20, 140)], AA[rng.integers(0, 20, 90)]
    in_data_order = [(9, a), (4, b), (2, a.copy()), (7, b.copy()), (1, a.copy())]
    seq = str(tmp_path / 'seq')
    write_db(seq, [(k, s.tobytes() + b'\n') for k, s in in_data_order], 0)
    sdgpu('clusthash', seq, tmp_path / 'res', '-v', '0')
    let, off = flat([s for _, s in in_data_order])
    keys = np.array([k for k, _ in in_data_order], np.uint32)
    found_by, identical, _, _ = ref.clusthash(let, off, byte_map(3), 0.99)
    got = read_db(str(tmp_path / 'res'))
    assert got == ref.entries(keys, off, found_by, identical)
    assert [l.split(b'\t')[0] for l in got[9].splitlines()] == [b'9', b'2', b'1'] and got[1].count(b'\n') == 1
    assert [l.split(b'\t')[0] for l in got[4].splitlines()] == [b'4', b'7']
