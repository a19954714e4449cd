"""tests/golden/clusterdb_vectors.npz (tools/make_golden_clusterdb.py: the reference's result2profile on a cluster DB, profile2consensus,
the per-pair realignments of its Matcher and the rows of `align -a`) as the clusterdb tests read it, and the files a DB consists of."""
import functools
import os
import struct

import numpy as np

from dbutil import GOLD, write_db

RUNS = ['K_r0', 'K_r1']   # the cluster DB as `cluster` writes it; one entry mixing 11-column and one-column rows


@functools.lru_cache(None)
def golden():
    return np.load(os.path.join(GOLD, 'clusterdb_vectors.npz'))


def _db(name):
    g = golden()
    k, off, text = g[name + '_keys'], g[name + '_off'].astype(np.int64), g[name + '_text'].tobytes()
    return [(int(x), text[off[i]:off[i + 1]]) for i, x in enumerate(k)]


@functools.lru_cache(None)
def sequences():
    """[(key, letters)] of <T> in id order"""
    g = golden()
    let, off = g['K_let'].tobytes(), g['K_off'].astype(np.int64)
    return [(int(k), let[off[i]:off[i + 1]]) for i, k in enumerate(g['K_keys'])]


def q_keys():
    return [int(k) for k in golden()['K_q_keys']]


def class_key(name):
    g = golden()
    return int(g['K_class_key'][list(g['K_class_names']).index(name)])


def classes():
    return [str(n) for n in golden()['K_class_names']]


def cluster_db(run):
    return _db(run + '_clu')


def profile_db(run):
    return _db(run + '_profile')


def consensus_db(run):
    return _db(run + '_consensus')


def aln_db():
    return _db('K_r0_aln')


@functools.lru_cache(None)
def pairs(run):
    """{(centre key, member key): (qStart, tStart, backtrace str)}: every row's realignment as result2profile computes it"""
    g = golden()
    off, bt = g[run + '_pair_bt_off'].astype(np.int64), g[run + '_pair_bt'].tobytes()
    return {(int(q), int(t)): (int(g[run + '_pair_qstart'][i]), int(g[run + '_pair_tstart'][i]), bt[off[i]:off[i + 1]].decode())
            for i, (q, t) in enumerate(zip(g[run + '_pair_q'], g[run + '_pair_t']))}


def db_files(entries, dbtype):
    """the three files of a DB whose entries were written in this order: (data, index, dbtype) bytes"""
    data, index, at = b'', [], 0
    for key, payload in entries:
        data += payload + b'\0'
        index.append((key, at, len(payload) + 1))
        at += len(payload) + 1
    return data, ''.join('%d\t%d\t%d\n' % e for e in sorted(index)).encode(), struct.pack('<i', dbtype)


def read_files(path):
    return tuple(open(path + s, 'rb').read() for s in ('', '.index', '.dbtype'))


def write_inputs(tmp, run='K_r0'):
    """<T>, db_clu (the representatives' sequences, as createsubdb copies them) and the cluster DB of a run -> their paths"""
    tmp = str(tmp)
    t, q, r = os.path.join(tmp, 't'), os.path.join(tmp, 'db_clu'), os.path.join(tmp, run + '_clu')
    seqs = sequences()
    by = dict(seqs)
    write_db(t, [(k, s + b'\n') for k, s in seqs], 0)
    write_db(q, [(k, by[k] + b'\n') for k in q_keys()], 0)
    write_db(r, cluster_db(run), 6)
    return t, q, r
