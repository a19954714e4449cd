"""Helpers of the profile-target tests (tests/test_target_profile_golden.py, tests/test_gpu_target_profile.py): the golden file
tools/make_golden_target_profile.py writes, and the digest of an index both sides compute."""
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'target_profile_vectors.npz')
PROFILE_GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'profile_vectors.npz')
SPAN = 10            # spaced seed 1101010011
SEED = (0, 1, 3, 5, 8, 9)

_cache = {}


def golden():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(GOLDEN))
    return _cache['g']


def g_profiles():
    """the 18 profiles of profile_vectors.npz: (bytes, byte offsets)"""
    if 'p' not in _cache:
        d = np.load(PROFILE_GOLDEN)
        _cache['p'] = (d['profiles'].tobytes(), d['poff'].astype(np.uint64))
    return _cache['p']


def digest(list_kmer, list_start, entry_seq, entry_pos):
    """SHA-256 over the non-empty lists' k-mers (u32) || their starts (u64) || entry_seq (u32) || entry_pos (u16), index order, little endian
    (the generator's digest())"""
    h = hashlib.sha256()
    for a, t in ((list_kmer, '<u4'), (list_start, '<u8'), (entry_seq, '<u4'), (entry_pos, '<u2')):
        h.update(np.ascontiguousarray(a, t).tobytes())
    return h.hexdigest()


def digest_of_download(d):
    """the same digest from Target.download()"""
    starts = d['starts']
    lens = np.diff(starts.astype(np.int64))
    ne = np.nonzero(lens > 0)[0]
    return digest(ne, starts[ne], d['entry_seq'], d['entry_pos'])


def triples_of_download(d):
    """(k-mer, target, position) of every entry, index order"""
    lens = np.diff(d['starts'].astype(np.int64))
    kmer = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    return np.stack([kmer, d['entry_seq'].astype(np.int64), d['entry_pos'].astype(np.int64)], axis=1)


def queries():
    """the golden queries as (letters ASCII bytes, offsets)"""
    g = golden()
    return g['Q_letters'].tobytes(), g['Q_off'].astype(np.uint64)


def windows_without_x(seq):
    """windows of an ASCII sequence whose seed positions hold no X"""
    n = 0
    for i in range(len(seq) - SPAN + 1):
        n += all(seq[i + s] != ord('X') for s in SEED)
    return n
