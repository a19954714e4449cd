"""tests/golden/clusthash_vectors.npz (tools/make_golden_clusthash.py: byte tables, hashes, entries and the "unique hashes" count from the
reference's own object code) as the clusthash tests read it."""
import functools
import gzip
import os

import numpy as np

from dbutil import GOLD, write_db

SETS = ['S', 'T', 'G', 'O', 'N', 'H', 'A', 'C1']


@functools.lru_cache(None)
def golden():
    return np.load(os.path.join(GOLD, 'clusthash_vectors.npz'))


def runs(name):
    return ['%s_r%d' % (name, r) for r in range(int(golden()[name + '_runs']))]


ALL_RUNS = [r for s in SETS for r in runs(s)]
SMALL_RUNS = [r for r in ALL_RUNS if not r.startswith('C1')]


@functools.lru_cache(None)
def sequences(name):
    """(letters uint8: the DB's own bytes, offsets uint64); ids are positions"""
    g = golden()
    if name != 'C1':
        return g[name + '_let'], g[name + '_off']
    seqs = []
    for f in ('NC_000913.faa', 'NC_000915.faa'):
        cur = None
        for line in gzip.open(os.path.join(GOLD, 'examples', f + '.gz'), 'rt'):
            if line.startswith('>'):
                if cur is not None:
                    seqs.append(cur)
                cur = ''
            else:
                cur += line.strip()
        seqs.append(cur)
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(''.join(seqs).encode(), np.uint8), off


@functools.lru_cache(None)
def residues(name):
    """the 21-letter codes of the set, as the product maps the bytes"""
    from spacedust_amd.api import Host
    return np.asarray(Host().matrix(0)[2], np.uint8)[sequences(name)[0]]


def keys(name):
    return golden()[name + '_keys']


def par(tag):
    """(alphabet size, threshold)"""
    p = golden()[tag + '_par']
    return int(p[0]), float(p[1])


def byte_map(tag):
    return golden()[tag + '_map']


def hashes(tag):
    return golden()[tag + '_hash']


def unique(tag):
    return int(golden()[tag + '_unique'])


def entries(tag):
    g = golden()
    k, off, text = g[tag + '_db_keys'], g[tag + '_db_off'].astype(np.int64), g[tag + '_db_text'].tobytes()
    return {int(x): text[off[i]:off[i + 1]] for i, x in enumerate(k)}


def class_seq(name, cls):
    g = golden()
    return int(g[name + '_class_seq'][list(g[name + '_class_names']).index(cls)])


def write_seq_db(tmp, name):
    """the sequences of a set as a sequence DB -> path"""
    let, off = sequences(name)
    off = off.astype(np.int64)
    k = keys(name)
    path = os.path.join(str(tmp), name + '_seq')
    write_db(path, [(int(k[i]), let[off[i]:off[i + 1]].tobytes() + b'\n') for i in range(len(k))], 0)
    return path
