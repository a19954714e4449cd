#!/usr/bin/env python3
"""Writes tests/golden/clust_vectors.npz from the LIVE reference: what the `clust` module (M/src/clustering) makes of a result DB of a set
against itself.  Inputs and results only.

Clustering.cpp cannot be linked (DBReader / DBWriter files), so DRIVER below compiles ClusteringAlgorithms.cpp and AlignmentSymmetry.cpp
where they lie, links oracle/_ref/libsdref.so for Util / Debug, and defines the six DBReader<unsigned int> accessors those two files leave
undefined (getData, getDataByDBKey, getDbKey, getId, getSize, remapData) over tables in memory -- reader plumbing only: the local order is
DBReader::open(SORT_BY_LENGTH)'s (index length descending, then id), the algorithm is the reference's own object code.  It calls
ClusteringAlgorithms::readInClusterData (made reachable with `#define private public`) and dumps the symmetric graph, then
ClusteringAlgorithms::execute on a fresh object and dumps the sorted pairs.  The printed cluster DB is Clustering::writeData
(Clustering.cpp:237-266) applied to those pairs by write_data() below (DBWriter cannot be linked either).  Nothing compiled is kept.

    python tools/make_golden_clust.py [reference root]          (needs `make -C oracle _ref/libsdref.so`; no GPU)
    python tools/make_golden_clust.py --time <edges>            (the driver's readInClusterData / execute seconds on a random graph)
    python tools/make_golden_clust.py --time-graph <file.npz>   (the same on the lists of tools/bench_clust.py --dump-graph)

Per set <S>: <S>_keys / <S>_lens (sequence DB: keys ascending, index lengths), <S>_<db>_{keys,off,text} (the result DB, except C1 whose rows
are tests/golden/config1_aln.tsv.gz), <S>_<db>_dbtype, and per similarity type t (1 alignment score, 2 sequence identity)
<S>_<db>_t<t>_{off,elem,score} (the symmetric graph over local ids) and, per run r in m0 (set cover), m1 (connected component,
--max-iterations 1000), m1c1 (--max-iterations 1), m2 (greedy): <S>_<db>_t<t>_<r>_pairs [n, 2] and <S>_<db>_t<t>_<r>_db_{keys,off,text}.
Sets:
  K    constructed: one named class per entry (K_class_names / K_class_keys), see set_k()
  K1   n = 1
  R    300 sequences, 3 000 one-way edges, seeded: as an alignment DB (aln) and as a prefilter DB with negative scores (pref)
  C1   the 5 898 proteins of the two example proteomes with the rows of config1_aln.tsv.gz (an empty entry where the file has no row)
The tie of equal set sizes (class tie_*) is built twice with the two tied nodes in either local order; main() asserts that the
reference's set cover picks a different representative in the two copies, i.e. that the bucket order decides the result there.
"""
import gzip
import io
import os
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLD = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLD, 'clust_vectors.npz')
ALN, CLU, PREF = 5, 6, 7   # Parameters::DBTYPE_*

DRIVER = r'''
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <queue>
#include <set>
#include <sstream>
#include <fstream>
#include <iostream>
#include <iomanip>
#include <memory>
#include <limits>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <atomic>
#include <stdexcept>
#include <utility>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>
#include <omp.h>
#define private public
#include "DBReader.h"
#include "ClusteringAlgorithms.h"
#undef private
// a reader over tables in memory: keys / data by the reader's id, id by key
struct Table {
    std::vector<unsigned int> keyOfId;
    std::vector<char *> dataOfId;
    std::map<unsigned int, size_t> idOfKey;
};
static std::map<const void *, Table> g_tables;
template <> char *DBReader<unsigned int>::getData(size_t id, int) { return g_tables[this].dataOfId[id]; }
template <> size_t DBReader<unsigned int>::getId(unsigned int key) {
    const Table &t = g_tables[this];
    std::map<unsigned int, size_t>::const_iterator it = t.idOfKey.find(key);
    return it == t.idOfKey.end() ? UINT_MAX : it->second;
}
template <> char *DBReader<unsigned int>::getDataByDBKey(unsigned int key, int thr) { return getData(getId(key), thr); }
template <> unsigned int DBReader<unsigned int>::getDbKey(size_t id) { return g_tables[this].keyOfId[id]; }
template <> size_t DBReader<unsigned int>::getSize() const { return size; }
template <> void DBReader<unsigned int>::remapData() {}
#include "ClusteringAlgorithms.cpp"
#include "AlignmentSymmetry.cpp"

static DBReader<unsigned int> *makeReader(size_t n, int dbtype, const std::vector<unsigned int> &entryLen) {
    // (no constructor of the class is linked: the object is zeroed storage with the members the inline accessors read)
    DBReader<unsigned int> *r = (DBReader<unsigned int> *) calloc(1, sizeof(DBReader<unsigned int>));
    r->size = n;
    r->dbtype = dbtype;
    r->index = (DBReader<unsigned int>::Index *) calloc(n + 1, sizeof(DBReader<unsigned int>::Index));
    for (size_t i = 0; i < n; i++) r->index[i].length = entryLen[i];
    return r;
}
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// job: i32 dbtype, scoretype, maxIterations, mode (1 set cover, 3 connected component, 4 greedy), threads; u32 n; u32 keys[n] ascending;
//      u32 indexLength[n]; per key u64 length + entry text
// result: u64 n; u64 hasGraph; [u64 off[n + 1]; u32 elem[]; u16 score[]]; u32 pairs[n][2]; f64 seconds of readInClusterData, of execute
int main(int argc, char **argv) {
    if (argc != 3) return 1;
    Debug::setDebugLevel(1);
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 1;
    int hdr[5];
    unsigned int n;
    if (fread(hdr, 4, 5, in) != 5 || fread(&n, 4, 1, in) != 1) return 2;
    const int dbtype = hdr[0], scoretype = hdr[1], maxIterations = hdr[2], mode = hdr[3], threads = hdr[4];
    omp_set_num_threads(threads);
    std::vector<unsigned int> keys(n), lens(n);
    if (n && (fread(keys.data(), 4, n, in) != n || fread(lens.data(), 4, n, in) != n)) return 2;
    std::vector<std::string> text(n);
    std::vector<unsigned int> entryLen(n);
    for (unsigned int i = 0; i < n; i++) {
        uint64_t len;
        if (fread(&len, 8, 1, in) != 1) return 2;
        text[i].resize(len);
        if (len && fread(&text[i][0], 1, len, in) != len) return 2;
        entryLen[i] = (unsigned int) len + 1;
    }
    fclose(in);
    // DBReader::open(SORT_BY_LENGTH), DBReader.cpp:325-342
    std::vector<unsigned int> local2id(n);
    for (unsigned int i = 0; i < n; i++) local2id[i] = i;
    std::stable_sort(local2id.begin(), local2id.end(), [&](unsigned int a, unsigned int b) { return lens[a] > lens[b]; });
    DBReader<unsigned int> *seqDbr = makeReader(n, 0, lens), *alnDbr = makeReader(n, dbtype, entryLen);
    Table &st = g_tables[seqDbr], &at = g_tables[alnDbr];
    st.keyOfId.resize(n);
    for (unsigned int i = 0; i < n; i++) {
        st.keyOfId[i] = keys[local2id[i]];
        st.idOfKey[keys[local2id[i]]] = i;
        at.keyOfId.push_back(keys[i]);
        at.dataOfId.push_back(&text[i][0]);
        at.idOfKey[keys[i]] = i;
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 1;
    const uint64_t n64 = n, hasGraph = mode != 4;
    fwrite(&n64, 8, 1, out);
    fwrite(&hasGraph, 8, 1, out);
    double tRead = 0.0;
    if (hasGraph) {
        ClusteringAlgorithms algo(seqDbr, alnDbr, threads, scoretype, maxIterations, NULL, NULL, NULL, NULL, 0, false);
        size_t elementCount = 0;
        for (size_t i = 0; i < n; i++) elementCount += (*alnDbr->getData(i, 0) == '\0') ? 1 : Util::countLines(alnDbr->getData(i, 0), alnDbr->getEntryLen(i));
        unsigned int *elements = new unsigned int[elementCount];
        unsigned int **elementLookupTable = new unsigned int *[n];
        unsigned short **scoreLookupTable = new unsigned short *[n];
        unsigned short *score = NULL;
        size_t *elementOffsets = new size_t[n + 1];
        elementOffsets[n] = 0;
        const double t0 = now();
        algo.readInClusterData(elementLookupTable, elements, scoreLookupTable, score, elementOffsets, elementCount);
        tRead = now() - t0;
        std::vector<uint64_t> off(elementOffsets, elementOffsets + n + 1);
        fwrite(off.data(), 8, n + 1, out);
        fwrite(elements, 4, off[n], out);
        fwrite(score, 2, off[n], out);
    }
    ClusteringAlgorithms algo(seqDbr, alnDbr, threads, scoretype, maxIterations, NULL, NULL, NULL, NULL, 0, false);
    const double t0 = now();
    std::pair<unsigned int, unsigned int> *ret = algo.execute(mode);
    const double tExec = now() - t0;
    for (unsigned int i = 0; i < n; i++) {
        fwrite(&ret[i].first, 4, 1, out);
        fwrite(&ret[i].second, 4, 1, out);
    }
    fwrite(&tRead, 8, 1, out);
    fwrite(&tExec, 8, 1, out);
    fclose(out);
    return 0;
}
'''


def build_driver(ref_root, tmp):
    m = os.path.join(ref_root, 'lib', 'mmseqs')
    src, exe = os.path.join(tmp, 'driver.cpp'), os.path.join(tmp, 'driver')
    open(src, 'w').write(DRIVER)
    inc = [os.path.join(m, *p) for p in (('src', 'commons'), ('src', 'alignment'), ('src', 'prefiltering'), ('src', 'clustering'), ('lib',),
                                          ('lib', 'simd'), ('lib', 'alp'), ('lib', 'tantan'), ('lib', 'fmt'), ('lib', 'simde'), ('lib', 'zstd', 'lib'))]
    refdir = os.path.join(ROOT, 'oracle', '_ref')
    subprocess.check_call(['g++', '-std=c++14', '-O3', '-mavx2', '-mfma', '-mcx16', '-DAVX2=1', '-DOPENMP=1', '-fopenmp', '-w',
                           '-ffunction-sections', '-fdata-sections'] + ['-I' + d for d in inc] +
                          [src, '-L' + refdir, '-lsdref', '-Wl,-rpath,' + refdir, '-Wl,--gc-sections', '-Wl,--allow-shlib-undefined', '-o', exe])
    return exe


def run_driver(exe, tmp, keys, lens, db, dbtype, scoretype, mode, max_iterations=1000, threads=4):
    """db: dict key -> bytes.  mode: the reference's execute() argument (1, 3, 4).  Returns dict(off, elem, score (mode 1 / 3), pairs, t_read, t_exec)."""
    job, res = os.path.join(tmp, 'job.bin'), os.path.join(tmp, 'res.bin')
    n = len(keys)
    with open(job, 'wb') as f:
        f.write(struct.pack('<5iI', dbtype, scoretype, max_iterations, mode, threads, n))
        f.write(np.asarray(keys, np.uint32).tobytes() + np.asarray(lens, np.uint32).tobytes())
        for k in keys:
            t = db[int(k)]
            f.write(struct.pack('<Q', len(t)) + t)
    subprocess.check_call([exe, job, res], stdout=subprocess.DEVNULL)
    raw = open(res, 'rb').read()
    n_out, has_graph = struct.unpack_from('<QQ', raw, 0)
    assert n_out == n
    at, out = 16, {}
    if has_graph:
        out['off'] = np.frombuffer(raw, np.uint64, n + 1, at).copy()
        at += 8 * (n + 1)
        total = int(out['off'][-1])
        out['elem'] = np.frombuffer(raw, np.uint32, total, at).copy()
        at += 4 * total
        out['score'] = np.frombuffer(raw, np.uint16, total, at).copy()
        at += 2 * total
    out['pairs'] = np.frombuffer(raw, np.uint32, 2 * n, at).reshape(n, 2).copy()
    at += 8 * n
    out['t_read'], out['t_exec'] = struct.unpack_from('<dd', raw, at)
    assert at + 16 == len(raw)
    return out


def write_data(pairs):
    """Clustering::writeData (Clustering.cpp:237-266) on the sorted pairs -> dict representative key -> entry text"""
    db, prev, cur_text = {}, None, b''
    for rep, mem in pairs.tolist():
        if prev != rep:
            if prev is not None:
                db[prev] = cur_text
            cur_text = b'%d\n' % rep
        if mem != rep:
            cur_text += b'%d\n' % mem
        prev = rep
    if prev is not None:
        db[prev] = cur_text
    return db


def save(path, arrays):
    """an .npz with fixed time stamps: it regenerates byte for byte"""
    with zipfile.ZipFile(path, 'w') as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED, 9)


def pack(out, name, db):
    keys = sorted(db)
    off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        off[1:] = np.cumsum([len(db[k]) for k in keys])
    out[name + '_keys'] = np.array(keys, np.uint32)
    out[name + '_off'] = off
    out[name + '_text'] = np.frombuffer(b''.join(db[k] for k in keys), np.uint8)


def aln_line(t, score=100, seq_id='0.500'):
    return b'%d\t%d\t%s\t1.000E-10\t0\t9\t10\t0\t9\t10\n' % (t, score, seq_id.encode())


def set_k():
    """-> (keys, lens, db, classes): classes maps a name to the key of the entry that is the class"""
    rng = np.random.default_rng(20)
    keys, lens, db, classes = [], [], {}, {}

    def node(length=None):
        k = 7 + 3 * len(keys)
        keys.append(k)
        lens.append(int(length if length is not None else rng.integers(40, 400)))
        db[k] = b''
        return k

    def row(k, *entries):
        db[k] = b''.join(aln_line(*e) if isinstance(e, tuple) else aln_line(e) for e in entries)

    a = node()
    classes['empty'] = a
    a = node()
    row(a, a)
    classes['self_only'] = a
    a, b = node(), node()
    row(a, (b, 77, '0.770'))
    row(b, b)
    classes['not_listing_itself'] = a
    a, b = node(), node()
    row(a, a, (b, 123, '0.456'))
    row(b, b)
    classes['one_way'] = a
    a, b = node(), node()
    row(a, a, (b, 300, '0.900'))
    row(b, b, (a, 200, '0.500'))
    classes['two_way_different_scores'] = a
    a, b = node(), node()
    row(a, a, (b, 50, '0.310'), (b, 60, '0.320'))
    row(b, b)
    classes['target_twice'] = a
    a, b, c = node(), node(), node()
    row(a, a, b, c)
    row(b, b, a, c)
    row(c, c, b, a)
    classes['already_symmetric'] = a
    a, b, c, d = node(), node(), node(), node()
    row(a, a, (b, 32767, '0.100'), (c, 32768, '0.200'), (d, 40000, '0.300'))
    for x in (b, c, d):
        row(x, x)
    classes['short_cast'] = a
    a, b, c, d = node(), node(), node(), node()
    row(a, a, (b, 10, '0.290'), (c, 11, '0.570'), (d, 12, '1.000'))
    for x in (b, c, d):
        row(x, x)
    classes['seq_id_rounding'] = a
    # equal lengths: the local order falls back to the key order
    same = [node(250) for _ in range(4)]
    row(same[3], same[3], same[0])
    row(same[1], same[1], same[2])
    classes['equal_lengths'] = same[0]
    # equal set sizes: a path a - b - c - d, b and c both of size 3; whoever leaves the bucket first takes the other.  Twice, with b and c
    # in either local order (lengths).  The four are the shortest sequences of the set, so they are the last of their bucket and leave
    # it before any other set's decreaseClustersize has swapped that bucket's head
    for tag, (lb, lc) in (('tie_bc', (31, 30)), ('tie_cb', (28, 29))):
        a, b, c, d = node(100), node(lb), node(lc), node(90)
        row(a, a, b)
        row(b, b, a, c)
        row(c, c, b, d)
        row(d, d, c)
        classes[tag] = b
    # a chain deeper than --max-iterations 1
    chain = [node() for _ in range(6)]
    for x, y in zip(chain, chain[1:]):
        row(x, x, y)
    row(chain[-1], chain[-1])
    classes['chain'] = chain[0]
    # a hub of 5 000 entries, every other row short
    hub = node(500)
    spokes = [node() for _ in range(4999)]
    db[hub] = aln_line(hub) + b''.join(aln_line(s, int(rng.integers(20, 900)), '0.%03d' % rng.integers(0, 1000)) for s in spokes)
    for s in spokes:
        row(s, s)
    classes['hub'] = hub
    return keys, lens, db, classes


def set_r(as_prefilter):
    rng = np.random.default_rng(31)
    n = 300
    keys = [2 * i + 1 for i in range(n)]
    lens = rng.integers(30, 120, n).tolist()
    rows = {k: [] for k in keys}
    for _ in range(3000):
        s, t = (int(x) for x in rng.integers(0, n, 2))
        score = int(rng.integers(-300, 300)) if as_prefilter else int(rng.integers(10, 2000))
        sid = '%.3f' % (rng.integers(0, 1001) / 1000.0)
        rows[keys[s]].append(b'%d\t%d\t%d\n' % (keys[t], score, int(rng.integers(-50, 50))) if as_prefilter else aln_line(keys[t], score, sid))
    return keys, lens, {k: b''.join(v) for k, v in rows.items()}


def set_c1():
    seqs = []
    for f in ('NC_000913.faa.gz', 'NC_000915.faa.gz'):
        for line in gzip.open(os.path.join(GOLD, 'examples', f), 'rt'):
            if line.startswith('>'):
                seqs.append('')
            else:
                seqs[-1] += line.strip()
    keys = list(range(len(seqs)))
    lens = [len(s) + 2 for s in seqs]
    rows = {k: [] for k in keys}
    for l in gzip.open(os.path.join(GOLD, 'config1_aln.tsv.gz'), 'rb'):
        k, rest = l.split(b'\t', 1)
        rows[int(k)].append(rest)
    return keys, lens, {k: b''.join(v) for k, v in rows.items()}


RUNS = (('m0', 1, 1000), ('m1', 3, 1000), ('m1c1', 3, 1), ('m2', 4, 1000))


def record(out, exe, tmp, name, keys, lens, db, dbtype, store_db=True):
    out[name + '_dbtype'] = np.int32(dbtype)
    if store_db:
        pack(out, name, db)
    res = {}
    for t in (1, 2):
        for run, mode, cap in RUNS:
            r = run_driver(exe, tmp, keys, lens, db, dbtype, t, mode, cap)
            tag = '%s_t%d' % (name, t)
            if run == 'm0':
                out[tag + '_off'], out[tag + '_elem'], out[tag + '_score'] = r['off'], r['elem'], r['score']
            elif 'off' in r:
                assert np.array_equal(out[tag + '_off'], r['off']) and np.array_equal(out[tag + '_elem'], r['elem'])
            out['%s_%s_pairs' % (tag, run)] = r['pairs']
            pack(out, '%s_%s_db' % (tag, run), write_data(r['pairs']))
            res[(t, run)] = r
    n_in = sum(max(1, t.count(b'\n')) for t in db.values())
    print('set %s: %d sequences, %d entries in, %d added; clusters m0 / m1 / m1c1 / m2 at similarity type 2: %s'
          % (name, len(keys), n_in, int(out[name + '_t2_off'][-1]) - n_in,
             ' / '.join(str(len(set(res[(2, run)]['pairs'][:, 0].tolist()))) for run, _, _ in RUNS)))
    return res


def time_run(exe, tmp, n_edges):
    rng = np.random.default_rng(1)
    n = max(2, n_edges // 40)
    keys = list(range(n))
    lens = rng.integers(30, 1000, n).tolist()
    src = np.sort(rng.integers(0, n, n_edges))
    dst = rng.integers(0, n, n_edges)
    cut = np.searchsorted(src, np.arange(n + 1))
    db = {k: b''.join(aln_line(int(t)) for t in dst[cut[k]:cut[k + 1]]) for k in keys}
    r = run_driver(exe, tmp, keys, lens, db, ALN, 2, 1, threads=16)
    print('%d sequences, %d entries, 16 threads: readInClusterData %.3f s, execute(set cover; reads the data again) %.3f s'
          % (n, n_edges, r['t_read'], r['t_exec']))


def time_graph(exe, tmp, path):
    """the reference's seconds on the lists tools/bench_clust.py --dump-graph wrote (rows of local ids with the identity column as score)"""
    g = np.load(path)
    keys, lens, order = g['keys'], g['lens'], g['order']
    off, elem, score = g['off'].astype(np.int64), g['elem'], g['score']
    local_keys = keys[order]
    tkeys = local_keys[elem].tolist()
    sc = score.tolist()
    db = {}
    for i, k in enumerate(local_keys.tolist()):
        db[k] = b''.join(b'%d\t100\t%d.%03d\t1.000E-10\t0\t9\t10\t0\t9\t10\n' % (tkeys[e], sc[e] // 1000, sc[e] % 1000) for e in range(off[i], off[i + 1]))
    for run, mode in (('set cover', 1), ('connected component', 3), ('greedy', 4)):
        r = run_driver(exe, tmp, keys.tolist(), lens.tolist(), db, ALN, 2, mode, threads=16)
        print('%d sequences, %d entries, 16 threads, %s: readInClusterData %.3f s; execute (reads the data again, then the algorithm) %.3f s'
              % (len(keys), len(elem), run, r['t_read'], r['t_exec']), flush=True)


def reference_root():
    """$REF, else the default oracle/Makefile builds the checkers from"""
    if os.environ.get('REF'):
        return os.environ['REF']
    for line in open(os.path.join(ROOT, 'oracle', 'Makefile')):
        if line.startswith('REF ?='):
            return line.split('=', 1)[1].strip()
    raise SystemExit('no reference root: set REF')


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    with tempfile.TemporaryDirectory() as tmp:
        if '--time-graph' in sys.argv:
            exe = build_driver(reference_root(), tmp)
            return time_graph(exe, tmp, args[0])
        if '--time' in sys.argv:
            exe = build_driver(reference_root(), tmp)
            return time_run(exe, tmp, int(args[0]))
        exe = build_driver(args[0] if args else reference_root(), tmp)
        out = {}
        keys, lens, db, classes = set_k()
        out['K_keys'], out['K_lens'] = np.array(keys, np.uint32), np.array(lens, np.uint32)
        out['K_class_names'] = np.array(sorted(classes))
        out['K_class_keys'] = np.array([classes[c] for c in sorted(classes)], np.uint32)
        res = record(out, exe, tmp, 'K_aln', keys, lens, db, ALN)
        # the tie decides: in the two copies of the path the set cover's representative of the tied pair is the other node of the pair
        rep_of = {int(m): int(r) for r, m in res[(2, 'm0')]['pairs'].tolist()}
        b1, b2 = classes['tie_bc'], classes['tie_cb']
        assert rep_of[b1] in (b1, b1 + 3) and rep_of[b2] in (b2, b2 + 3) and (rep_of[b1] == b1) != (rep_of[b2] == b2), (rep_of[b1], rep_of[b2])
        print('tie of equal set sizes: representatives %d (b = %d) and %d (b = %d)' % (rep_of[b1], b1, rep_of[b2], b2))
        out['K1_keys'], out['K1_lens'] = np.array([5], np.uint32), np.array([33], np.uint32)
        record(out, exe, tmp, 'K1_aln', [5], [33], {5: aln_line(5)}, ALN)
        for name, dbtype in (('aln', ALN), ('pref', PREF)):
            keys, lens, db = set_r(dbtype == PREF)
            out['R_keys'], out['R_lens'] = np.array(keys, np.uint32), np.array(lens, np.uint32)
            record(out, exe, tmp, 'R_' + name, keys, lens, db, dbtype)
        keys, lens, db = set_c1()
        out['C1_keys'], out['C1_lens'] = np.array(keys, np.uint32), np.array(lens, np.uint32)
        record(out, exe, tmp, 'C1_aln', keys, lens, db, ALN, store_db=False)
    save(OUT, out)
    size = os.path.getsize(OUT)
    print('wrote %s (%d bytes)' % (OUT, size))
    assert size < 1024 * 1024


if __name__ == '__main__':
    main()
