"""tests/golden/kmermatch_vectors.npz and kmermatch_edges.npz (tools/make_golden_kmermatch.py: letter maps, records and entries from the
reference's own object code) as the kmermatcher tests read them: one table of arrays.  The second file holds set E and further runs of
sets of the first (<S>_more_runs of them, numbered on from <S>_runs)."""
import functools
import gzip
import os

import numpy as np

from dbutil import GOLD, write_db

SETS = ['S', 'G', 'H', 'A', 'W', 'C1', 'E']
LETTERS = 'ACDEFGHIKLMNPQRSTVWYX'


class _Files:
    def __init__(self, *names):
        self.files = [np.load(os.path.join(GOLD, n)) for n in names]

    def __contains__(self, key):
        return any(key in f.files for f in self.files)

    def __getitem__(self, key):
        for f in self.files:
            if key in f.files:
                return f[key]
        raise KeyError(key)


@functools.lru_cache(None)
def golden():
    return _Files('kmermatch_vectors.npz', 'kmermatch_edges.npz')


def runs(name):
    g = golden()
    n = int(g[name + '_runs']) + (int(g[name + '_more_runs']) if name + '_more_runs' in g else 0)
    return ['%s_r%d' % (name, r) for r in range(n)]


ALL_RUNS = [r for s in SETS for r in runs(s)]
SMALL_RUNS = [r for r in ALL_RUNS if not r.startswith('C1')]


@functools.lru_cache(None)
def sequences(name):
    """(residues as 21-letter codes, offsets uint64)"""
    g = golden()
    if name != 'C1':
        return g[name + '_res'], g[name + '_off']
    from spacedust_amd.api import Host
    aa2num = Host().matrix(0)[2]
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
    return aa2num[np.frombuffer(''.join(seqs).encode(), np.uint8)].astype(np.uint8), off


def par(tag):
    p = golden()[tag + '_par']
    return dict(k=int(p[0]), alph_size=int(p[1]), kmer_per_seq=int(p[2]), kmer_per_seq_scale=float(p[3]), hash_shift=int(p[4]),
                cov_mode=int(p[5]), c=float(p[6]), include_only_extendable=bool(p[7]))


def api_par(p):
    from spacedust_amd import api
    return api.kmermatch_params(**p)


def keys(tag):
    return golden()[tag + '_keys']


def letter_map(tag):
    return golden()[tag + '_map']


def entries(tag):
    g = golden()
    k, off, text = g[tag + '_db_keys'], g[tag + '_db_off'].astype(np.int64), g[tag + '_db_text'].tobytes()
    return {int(x): text[off[i]:off[i + 1]] for i, x in enumerate(k)}


def hits_of(db):
    """the hit lines of a prefilter DB -> int64 [h, 4] (rep, member, score, diagonal as printed), sorted by (rep, member)"""
    out = []
    for rep in sorted(db):
        for line in db[rep].splitlines()[1:]:
            m, s, d = line.split(b'\t')
            out.append((rep, int(m), int(s), int(d)))
    return np.array(out, np.int64).reshape(-1, 4)


def records(tag):
    g = golden()
    return g[tag + '_rec_key'], g[tag + '_rec_pos'], g[tag + '_rec_off']


def write_seq_db(tmp, name, tag):
    """the sequences of a set with the keys of a run, as a sequence DB -> path"""
    res, off = sequences(name)
    off = off.astype(np.int64)
    lut = np.frombuffer(LETTERS.encode(), np.uint8)
    k = keys(tag)
    path = os.path.join(str(tmp), tag + '_seq')
    write_db(path, [(int(k[i]), lut[res[off[i]:off[i + 1]]].tobytes() + b'\n') for i in np.argsort(k, kind='stable')], 0)
    return path
