"""Helpers of the swapresults tests (tests/test_swapresults.py, tests/test_gpu_target_profile_search.py): the golden file
tools/make_golden_swap.py writes -- DBs as (keys, offsets, text) triples -- and the two DBs of set G on disk."""
import os

import numpy as np

import tpref
from dbutil import write_db

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'swap_vectors.npz')
SETS = ('G110', 'G95')
N_PROF, N_SEQ = 18, 152

_cache = {}


def golden():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(GOLDEN))
    return _cache['g']


def db(name):
    """the DB `name` of the golden file: dict key -> bytes"""
    g = golden()
    keys, off, text = g[name + '_keys'], g[name + '_off'].astype(np.int64), g[name + '_text'].tobytes()
    return {int(k): text[off[i]:off[i + 1]] for i, k in enumerate(keys)}


def rows(d):
    return sum(t.count(b'\n') for t in d.values())


def sequences():
    letters, off = tpref.queries()
    return [letters[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def write_set_g(tmp):
    """the 152 sequences and the 18 profiles as DBs under tmp: (sequence DB path, profile DB path)"""
    data, poff = tpref.g_profiles()
    seq_db, prof_db = os.path.join(str(tmp), 'seq'), os.path.join(str(tmp), 'prof')
    write_db(seq_db, [(i, s + b'\n') for i, s in enumerate(sequences())], 0)
    write_db(prof_db, [(i, data[int(poff[i]):int(poff[i + 1])]) for i in range(len(poff) - 1)], 2)
    return seq_db, prof_db
