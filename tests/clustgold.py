"""tests/golden/clust_vectors.npz (tools/make_golden_clust.py: the reference's own graphs and clusterings) as the clust tests read it."""
import functools
import os

import numpy as np

from dbutil import GOLD, entries_by_first_column, flat_lines_from_gz, write_db

SETS = ['K_aln', 'K1_aln', 'R_aln', 'R_pref', 'C1_aln']
RUNS = {'m0': (0, 1000), 'm1': (1, 1000), 'm1c1': (1, 1), 'm2': (2, 1000)}   # run -> (--cluster-mode, --max-iterations)


@functools.lru_cache(None)
def golden():
    return np.load(os.path.join(GOLD, 'clust_vectors.npz'))


def unpack(name):
    g = golden()
    keys, off, text = g[name + '_keys'], g[name + '_off'].astype(np.int64), g[name + '_text'].tobytes()
    return {int(k): text[off[i]:off[i + 1]] for i, k in enumerate(keys)}


@functools.lru_cache(None)
def inputs(name):
    """(keys ascending, index lengths, result DB as dict key -> bytes, dbtype)"""
    g = golden()
    s = name.split('_')[0]
    keys, lens = g[s + '_keys'], g[s + '_lens']
    if s == 'C1':
        db = dict(entries_by_first_column(flat_lines_from_gz('config1_aln.tsv.gz'), len(keys)))
    else:
        db = unpack(name)
    return keys, lens, db, int(g[name + '_dbtype'])


@functools.lru_cache(None)
def local(name):
    """(keys by local id, entries by local id)"""
    from spacedust_amd import api
    keys, lens, db, _ = inputs(name)
    order = api.clust_order(lens)
    local_keys = keys[order]
    return local_keys, [db[int(k)] for k in local_keys]


def graph(name, t):
    g = golden()
    tag = '%s_t%d' % (name, t)
    return g[tag + '_off'], g[tag + '_elem'], g[tag + '_score']


def input_rows(name, t):
    """the input part of every golden row: (row_off, elem, score)"""
    off, elem, score = graph(name, t)
    _, entries = local(name)
    n_in = np.array([max(1, e.count(b'\n')) for e in entries], np.int64)
    row_off = np.zeros(len(n_in) + 1, np.uint64)
    row_off[1:] = np.cumsum(n_in)
    take = np.concatenate([np.arange(int(off[i]), int(off[i]) + int(n_in[i])) for i in range(len(n_in))]) if len(n_in) else np.zeros(0, np.int64)
    return row_off, elem[take], score[take]


def pairs(name, t, run):
    return golden()['%s_t%d_%s_pairs' % (name, t, run)]


def cluster_db(name, t, run):
    return unpack('%s_t%d_%s_db' % (name, t, run))


def write_inputs(tmp, name):
    """the sequence DB (entries of the recorded index lengths) and the result DB of a set as DB files -> (seq path, result path)"""
    keys, lens, db, dbtype = inputs(name)
    seq, res = os.path.join(str(tmp), name + '_seq'), os.path.join(str(tmp), name + '_res')
    write_db(seq, [(int(k), b'A' * (int(l) - 2) + b'\n') for k, l in zip(keys, lens)], 0)
    write_db(res, [(int(k), db[int(k)]) for k in keys], dbtype)
    return seq, res
