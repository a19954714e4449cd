#!/usr/bin/env python3
"""Writes tests/golden/clusthash_vectors.npz from the LIVE reference: what `clusthash` (M/src/util/clusthash.cpp) makes of an amino-acid
sequence DB.  Inputs, parameters and recorded outputs only.

The module cannot be linked as it stands (Parameters.cpp needs generated headers; DBReader / DBWriter are files), so DRIVER below includes
clusthash.cpp and ReducedMatrix.cpp where they lie, links oracle/_ref/libsdref.so for Sequence, SubstitutionMatrix, BaseMatrix, Util and
Debug, and runs clusthash() itself.  Function by function:

  the reference's own object code
    clusthash()                                       the whole function: SubstitutionMatrix and ReducedMatrix, Sequence::mapSequence,
                                                      Util::hash, SORT_PARALLEL, the hash runs, the greedy loop with
                                                      DistanceCalculator::computeInverseHammingDistance and Util::fastSeqIdToBuffer, the text;
                                                      its "Found N unique hashes" line is read from its output
    the hash per sequence                             Sequence::mapSequence + Util::hash again, called by the driver over a ReducedMatrix built
                                                      with clusthash()'s own arguments (the function does not hand its hashes out); the byte ->
                                                      code table is that matrix's aa2num
  reader / writer plumbing defined in the driver (no algorithm)
    DBReader<unsigned int>  constructor, open, close, readMmapedDataInMemory, getData, getDbKey, getSize   over tables in memory, ids in
                                                      input order
    DBWriter                constructor, open, close, writeData into a map key -> text
    Parameters              zeroed storage; parseParameters sets the members the function reads (alphabetSize, seqIdThr, threads,
                                                      maxSeqLen, scoringMatrixFile, the DB names) and nothing else

    python tools/make_golden_clusthash.py [reference root]      (needs `make -C oracle _ref/libsdref.so`; no GPU)
    python tools/make_golden_clusthash.py --time <file.npz> <threads>   (the driver's seconds for clusthash() on the `letters` / `off` of the file)

Per set <S>: <S>_let (the DB's bytes), <S>_off, <S>_keys, <S>_runs, and per run <S>_r<i>_{par (alphabet, threshold), map (256), hash,
unique, db_keys, db_off, db_text}.  C1 records no sequences: they are tests/golden/examples.  <S>_class_names / <S>_class_seq name the
sequences built for a class.  main() asserts the class properties on the recorded output, that tests/clusthash_ref.py equals every recorded
hash and entry, and what the three misreadings clusthash_ref.py names do to set G.
"""
import gzip
import io
import os
import re
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import clusthash_ref as ref  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLD, 'clusthash_vectors.npz')
AA = b'ACDEFGHIKLMNPQRSTVWY'

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
#include <sys/stat.h>
#include <sys/mman.h>
#include <fcntl.h>
#include <omp.h>
#define private public
#define protected public
#include "DBReader.h"
#include "DBWriter.h"
#include "Parameters.h"
#undef private
#undef protected
struct Table {
    std::vector<unsigned int> keyOfId;
    std::vector<char *> dataOfId;
    std::vector<unsigned int> lenOfId;
};
static Table g_table;
static std::map<unsigned int, std::string> g_written;
static int g_alph, g_threads;
static float g_thr;
static std::string g_matrix;
template <> DBReader<unsigned int>::DBReader(const char *, const char *, int threads_, int mode) {
    memset((void *) &threads, 0, (char *) &magicBytes - (char *) &threads);
    new (&dataFileNames) std::vector<std::string>();
    threads = threads_;
    dataMode = mode;
    indexFileName = (char *) "memory";
    dataFileName = (char *) "memory";
    size = g_table.keyOfId.size();
    dbtype = Parameters::DBTYPE_AMINO_ACIDS;
    index = (Index *) calloc(size + 1, sizeof(Index));
    for (size_t i = 0; i < size; i++) index[i].length = g_table.lenOfId[i] + 2;
    closed = 0;
}
template <> DBReader<unsigned int>::~DBReader() { free(index); }
template <> bool DBReader<unsigned int>::open(int) { return true; }
template <> void DBReader<unsigned int>::close() {}
template <> void DBReader<unsigned int>::readMmapedDataInMemory() {}
template <> char *DBReader<unsigned int>::getData(size_t id, int) { return g_table.dataOfId[id]; }
template <> unsigned int DBReader<unsigned int>::getDbKey(size_t id) { return g_table.keyOfId[id]; }
template <> size_t DBReader<unsigned int>::getSize() const { return size; }
DBWriter::DBWriter(const char *, const char *, unsigned int threads_, size_t mode_, int dbtype_) : threads(threads_), mode(mode_), dbtype(dbtype_) {}
DBWriter::~DBWriter() {}
void DBWriter::open(size_t) {}
void DBWriter::close(bool, bool) {}
void DBWriter::writeData(const char *data, size_t dataSize, unsigned int key, unsigned int, bool, bool) {
#pragma omp critical
    g_written[key] = std::string(data, dataSize);
}
Parameters *Parameters::instance = NULL;
void initParameterSingleton(void) { abort(); }
void Parameters::parseParameters(int, const char **, const Command &, bool, int, int) {
    alphabetSize = MultiParam<NuclAA<int>>(NuclAA<int>(g_alph, 5));
    seqIdThr = g_thr;
    threads = g_threads;
    compressed = 0;
    maxSeqLen = 65535;
    preloadMode = Parameters::PRELOAD_MODE_MMAP;
}
#include "clusthash.cpp"
#include "ReducedMatrix.cpp"
// what the nucleotide branch names: it must link, it is never read
const char *Orf::iupacReverseComplementTable = NULL;

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// job: i32 alphabet, threads; f32 threshold; u32 n; u32 keys[n]; u64 off[n + 1]; letters
// result: u8 aa2num[256] of the reduced matrix; u64 hash[n]; u64 nEntries; per entry u32 key, u64 len, text; f64 seconds of clusthash()
int main(int argc, char **argv) {
    if (argc != 4) return 1;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 1;
    int hdr[2];
    float thr;
    unsigned int n;
    if (fread(hdr, 4, 2, in) != 2 || fread(&thr, 4, 1, in) != 1 || fread(&n, 4, 1, in) != 1) return 2;
    std::vector<unsigned int> keys(n);
    std::vector<uint64_t> off(n + 1);
    if (n && fread(keys.data(), 4, n, in) != n) return 2;
    if (fread(off.data(), 8, n + 1, in) != n + 1) return 2;
    std::vector<char> letters(off[n] + 1);
    if (off[n] && fread(letters.data(), 1, off[n], in) != off[n]) return 2;
    fclose(in);
    g_alph = hdr[0];
    g_threads = hdr[1];
    g_thr = thr;
    g_matrix = argv[3];
    omp_set_num_threads(g_threads);
    std::vector<std::string> text(n);
    for (unsigned int i = 0; i < n; i++) {
        text[i].assign(letters.data() + off[i], off[i + 1] - off[i]);
        text[i] += "\n";
        g_table.keyOfId.push_back(keys[i]);
        g_table.dataOfId.push_back(&text[i][0]);
        g_table.lenOfId.push_back((unsigned int) (off[i + 1] - off[i]));
    }
    Parameters *par = (Parameters *) calloc(1, sizeof(Parameters));
    new (&par->db1) std::string("in");
    new (&par->db1Index) std::string("in.index");
    new (&par->db2) std::string("out");
    new (&par->db2Index) std::string("out.index");
    new (&par->scoringMatrixFile) MultiParam<NuclAA<std::string>>(NuclAA<std::string>(g_matrix, "nucleotide.out"));
    Parameters::instance = par;
    Debug::setDebugLevel(3);
    const double t0 = now();
    const Command *none = NULL;
    if (clusthash(0, NULL, *none) != EXIT_SUCCESS) return 3;
    const double t1 = now();
    fflush(stdout);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 1;
    {
        SubstitutionMatrix sMat(g_matrix.c_str(), 2.0, -0.2);
        ReducedMatrix red(sMat.probMatrix, sMat.subMatrixPseudoCounts, sMat.aa2num, sMat.num2aa, sMat.alphabetSize, g_alph, 2.0);
        for (int c = 0; c < 256; c++) fputc(red.aa2num[c], out);
        Sequence seq(65535, Parameters::DBTYPE_AMINO_ACIDS, &red, 0, false, false);
        for (unsigned int i = 0; i < n; i++) {
            seq.mapSequence(i, 0, g_table.dataOfId[i], g_table.lenOfId[i]);
            uint64_t h = Util::hash(seq.numSequence, seq.L);
            fwrite(&h, 8, 1, out);
        }
    }
    uint64_t nEntries = g_written.size();
    fwrite(&nEntries, 8, 1, out);
    for (std::map<unsigned int, std::string>::const_iterator it = g_written.begin(); it != g_written.end(); ++it) {
        uint32_t key = it->first;
        uint64_t len = it->second.size();
        fwrite(&key, 4, 1, out);
        fwrite(&len, 8, 1, out);
        fwrite(it->second.data(), 1, len, out);
    }
    const double t = t1 - t0;
    fwrite(&t, 8, 1, out);
    fclose(out);
    return 0;
}
'''


def build_driver(ref_root, tmp):
    m = os.path.join(ref_root, 'lib', 'mmseqs')
    src, exe = os.path.join(tmp, 'driver.cpp'), os.path.join(tmp, 'driver')
    open(src, 'w').write(DRIVER)
    inc = [os.path.join(m, *p) for p in (('src', 'commons'), ('src', 'alignment'), ('src', 'prefiltering'), ('src', 'clustering'), ('src', 'linclust'),
                                          ('src', 'util'), ('lib',), ('lib', 'simd'), ('lib', 'alp'), ('lib', 'tantan'), ('lib', 'fmt'), ('lib', 'simde'),
                                          ('lib', 'zstd', 'lib'), ('lib', 'xxhash'), ('lib', 'omptl'), ('lib', 'ips4o'), ('lib', 'kerasify'))]
    inc = [d for d in inc if os.path.isdir(d)]
    refdir = os.path.join(ROOT, 'oracle', '_ref')
    subprocess.check_call(['g++', '-std=c++14', '-O3', '-mavx2', '-mfma', '-mcx16', '-DAVX2=1', '-DOPENMP=1', '-fopenmp', '-w', '-fvisibility=hidden',
                           '-ffunction-sections', '-fdata-sections'] + ['-I' + d for d in inc] +
                          [src, '-L' + refdir, '-lsdref', '-Wl,-rpath,' + refdir, '-Wl,--gc-sections', '-Wl,--allow-shlib-undefined', '-o', exe])
    return exe


def run_driver(exe, tmp, matrix, alph, thr, letters, offsets, keys, threads=4):
    """-> dict(map 256, hash, db, unique, seconds); the sequences in the order given = id order"""
    keys = np.asarray(keys, np.uint32)
    off = np.asarray(offsets, np.uint64)
    job, res = os.path.join(tmp, 'job.bin'), os.path.join(tmp, 'res.bin')
    with open(job, 'wb') as f:
        f.write(struct.pack('<2ifI', alph, threads, thr, len(keys)))
        f.write(keys.tobytes() + off.tobytes() + np.asarray(letters, np.uint8).tobytes())
    said = subprocess.run([exe, job, res, matrix], stdout=subprocess.PIPE, check=True).stdout.decode(errors='replace')
    raw = open(res, 'rb').read()
    n = len(keys)
    out = dict(map=np.frombuffer(raw, np.uint8, 256, 0).copy(), hash=np.frombuffer(raw, '<u8', n, 256).copy())
    at = 256 + 8 * n
    n_ent, = struct.unpack_from('<Q', raw, at)
    at += 8
    db = {}
    for _ in range(n_ent):
        key, ln = struct.unpack_from('<IQ', raw, at)
        at += 12
        db[key] = raw[at:at + ln]
        at += ln
    out['db'] = db
    out['seconds'], = struct.unpack_from('<d', raw, at)
    assert at + 8 == len(raw)
    out['unique'] = int(re.search(r'Found (\d+) unique hashes', said).group(1))
    return out


def save(path, arrays):
    """an .npz with fixed time stamps: it regenerates byte for byte"""
    with zipfile.ZipFile(path, 'w') as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED, 9)


def pack_db(out, name, db):
    keys = sorted(db)
    off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        off[1:] = np.cumsum([len(db[k]) for k in keys])
    out[name + '_keys'] = np.array(keys, np.uint32)
    out[name + '_off'] = off
    out[name + '_text'] = np.frombuffer(b''.join(db[k] for k in keys), np.uint8)


# ---- the sets ----------------------------------------------------------------------------------------------------------------------
def rnd(rng, length):
    return np.frombuffer(AA, np.uint8)[rng.integers(0, 20, length)].copy()


def flat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs).astype(np.uint8) if len(seqs) and int(off[-1]) else np.zeros(0, np.uint8)), off


class Classes:
    """letters that share a reduced code with a letter: substitutions that keep the hash"""

    def __init__(self, map256):
        self.map = np.asarray(map256, np.uint8)
        self.peers = {}
        for c in AA:
            self.peers[c] = [d for d in AA if d != c and self.map[d] == self.map[c]]

    def swap(self, seq, positions, rng=None):
        """a copy with another letter of the same class at every position"""
        s = seq.copy()
        for p in positions:
            peers = self.peers[int(seq[p])]
            assert peers, 'letter %c is alone in its class' % seq[p]
            s[p] = peers[0] if rng is None else peers[int(rng.integers(0, len(peers)))]
        return s


S_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)


def twin_positions(length):
    """single substitutions: the first and the last byte, and the byte on each side of the first and the last 4-, 16-, 64- and 256-byte edge"""
    pos = {0, length - 1}
    for e in (4, 16, 64, 256):
        if length > e:
            last = (length - 1) // e * e
            pos |= {e - 1, e, last - 1, last}
    return sorted(p for p in pos if 0 <= p < length)


def set_s(cl):
    """hash and comparison lengths.  Runs: r0 the defaults (alphabet 3, 0.99); r1 0.5, which accepts the comb twins"""
    rng = np.random.default_rng(31)
    seqs, classes, filler = [], {}, [0]

    def add(s):
        seqs.append(rnd(rng, filler[0] % 16 + 1))   # a filler in front of every sequence: every start alignment mod 16 occurs
        filler[0] += 1
        seqs.append(s)

    for length in S_LENGTHS:
        base = rnd(rng, length)
        classes['length_%d' % length] = len(seqs) + 1
        add(base)
        if length == 0:
            add(base.copy())
            continue
        for p in twin_positions(length):
            add(cl.swap(base, [p]))
        if length >= 8:   # every 4-byte edge at once: the bytes before the edges, and the bytes behind them
            add(cl.swap(base, range(3, length, 4)))
            add(cl.swap(base, range(4, length, 4)))
    return seqs, [(3, 0.99), (3, 0.5)], classes


T_LENGTHS = (100, 101, 200, 1000)
T_THRESHOLDS = (0.99, 0.9, 0.5, 1.0, 0.0)


def set_t(cl):
    """the threshold boundary: per length a base and, per threshold, copies with minIdentical - 1, minIdentical and L equal bytes.  One
    run per threshold over the whole set; the base has the smallest id of its group"""
    rng = np.random.default_rng(37)
    seqs, classes = [], {}
    for length in T_LENGTHS:
        base = rnd(rng, length)
        classes['base_%d' % length] = len(seqs)
        seqs.append(base)
        for thr in T_THRESHOLDS:
            need = ref.min_identical(thr, length)
            for name, eq in (('below', need - 1), ('at', need), ('all', length)):
                if 0 <= eq <= length:
                    classes['%s_%d_%g' % (name, length, thr)] = len(seqs)
                    seqs.append(cl.swap(base, rng.permutation(length)[:length - eq], rng))
    return seqs, [(3, thr) for thr in T_THRESHOLDS], classes


def set_g(cl, map256):
    """greedy classes; all at 200 residues unless said.  Runs: r0 the defaults; r1 threshold 0.0 (everything of one hash and length is
    marked by the first, identity "0.000" included)"""
    rng = np.random.default_rng(41)
    seqs, classes = [], {}

    def add(name, *ss):
        classes[name] = len(seqs)
        seqs.extend(np.asarray(s, np.uint8) for s in ss)

    a = rnd(rng, 200)
    add('chain', a, cl.swap(a, [10, 20]), cl.swap(a, [10, 20, 30, 40]))   # A~B, B~C, A !~ C: B is found between the unfound A and C
    a = rnd(rng, 200)
    add('chain_closed', a, cl.swap(a, [10, 20]), cl.swap(a, [20, 30]))     # A~B, B~C and C~A: A marks both
    a = rnd(rng, 200)
    add('late_pair', cl.swap(a, [1, 2, 3, 4, 5, 6]), a, cl.swap(a, [100]))  # the first is far from both, the second marks the third
    zero = bytes([c for c in AA if map256[c] == 0])[:1]
    assert zero
    a = rnd(rng, 150)
    add('equal_hash_unequal_length', a, np.concatenate([np.frombuffer(zero * 3, np.uint8), a]))
    a = rnd(rng, 120)
    add('lower_case', a, np.frombuffer(a.tobytes().lower(), np.uint8))
    a = rnd(rng, 130)
    a[[5, 50, 90]] = np.frombuffer(b'BZX', np.uint8)
    b = a.copy()
    b[5] = ord('D') if map256[ord('B')] == map256[ord('D')] else b[5]
    add('bzx', a, b, a.copy())
    return seqs, [(3, 0.99), (3, 0.0)], classes


def set_one():
    return [rnd(np.random.default_rng(43), 77)], [(3, 0.99)], {}


def set_nopair():
    rng = np.random.default_rng(47)
    return [rnd(rng, 80), rnd(rng, 81), rnd(rng, 82)], [(3, 0.99)], {}


def set_h(cl):
    """a hub: one sequence of 50 residues 5 000 times, and 50 copies that miss the threshold by one, shuffled"""
    rng = np.random.default_rng(53)
    hub = rnd(rng, 50)
    seqs = [hub.copy() for _ in range(5000)] + [cl.swap(hub, [p]) for p in range(50)]
    order = rng.permutation(len(seqs))
    return [seqs[i] for i in order], [(3, 0.99)], {}


def example_proteins():
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
    return [np.frombuffer(s.encode(), np.uint8) for s in seqs]


def set_a(cl):
    """200 of the example proteins (the first 200 of up to 400 residues) with 1 .. 8 substituted copies each, shuffled.  Copies carry 0 .. 5
    substitutions, most of them inside the reduced class of alphabet 3.  Runs: alphabets 3, 13 x thresholds 0.99, 0.9 (the reference refuses
    --alph-size 21: "Reduced alphabet has to be smaller than the original one")"""
    rng = np.random.default_rng(59)
    roots = [s for s in example_proteins() if 30 <= len(s) <= 400 and set(s.tobytes()) <= set(AA + b'*')][:200]   # (they end in '*')
    assert len(roots) == 200
    seqs = []
    for root in roots:
        seqs.append(root.copy())
        for _ in range(int(rng.integers(1, 9))):
            k = int(rng.integers(0, 6))
            pos = rng.permutation(np.flatnonzero(root != ord('*')))[:k]
            if rng.random() < 0.8:
                seqs.append(cl.swap(root, pos, rng))
            else:
                s = root.copy()
                s[pos] = rnd(rng, k)
                seqs.append(s)
    order = rng.permutation(len(seqs))
    return [seqs[i] for i in order], [(a, t) for a in (3, 13) for t in (0.99, 0.9)], {}


def host_map256(alph):
    """the product's own byte -> reduced code table: sd_host_matrix's aa2num through sd_host_reduced_alphabet"""
    from spacedust_amd import api
    aa2num = np.asarray(api.Host().matrix(0)[2], np.uint8)
    return api.reduced_alphabet(alph)[0][aa2num]


def lines(db, key):
    return [l.split(b'\t') for l in db[key].splitlines()]


def members(db, key):
    return [int(l[0]) for l in lines(db, key)]


def check_classes(rec):
    key = lambda name, c, i=0: int(rec[name]['keys'][rec[name]['classes'][c] + i])
    # S: every start alignment mod 16, and every pair of alignments mod 4 among the compared pairs
    s = rec['S']
    off = s['off'].astype(np.int64)
    starts = {int(off[i]) % 16 for i in range(1, len(off) - 1, 2)}
    assert starts == set(range(16)), starts
    fb = s['runs'][1]['found_by']
    assert {(int(off[i]) % 4, int(off[fb[i]]) % 4) for i in range(len(fb)) if fb[i] != ref.NONE} == {(x, y) for x in range(4) for y in range(4)}
    db0, db1 = s['runs'][0]['db'], s['runs'][1]['db']
    assert len(members(db0, key('S', 'length_1025'))) > 10 and len(members(db0, key('S', 'length_63'))) == 1   # one of 63 differs: below 0.99
    assert len(members(db1, key('S', 'length_1025'))) == len(twin_positions(1025)) + 3   # the combs too at 0.5
    assert members(db0, key('S', 'length_0')) == [key('S', 'length_0')]                 # empty sequences: 0 / 0 reaches nothing
    # T: the boundary pairs fall on both sides
    t = rec['T']
    for r, thr in enumerate(T_THRESHOLDS):
        db = t['runs'][r]['db']
        for length in T_LENGTHS:
            got = members(db, key('T', 'base_%d' % length))
            at, below = 'at_%d_%g' % (length, thr), 'below_%d_%g' % (length, thr)
            if at in t['classes']:
                assert key('T', at) in got, (thr, length)
            if below in t['classes']:
                assert key('T', below) not in got, (thr, length)
    assert any(l[2] == b'1.000' for l in lines(t['runs'][0]['db'], key('T', 'base_100'))[1:])   # the C string, not "1.00"
    # G
    g = rec['G']
    db = g['runs'][0]['db']
    k = lambda c, i=0: key('G', c, i)
    assert members(db, k('chain')) == [k('chain'), k('chain', 1)] and members(db, k('chain', 1)) == [k('chain', 1)]
    assert members(db, k('chain', 2)) == [k('chain', 2)]
    assert members(db, k('chain_closed')) == [k('chain_closed'), k('chain_closed', 1), k('chain_closed', 2)]
    assert members(db, k('late_pair')) == [k('late_pair')] and members(db, k('late_pair', 1)) == [k('late_pair', 1), k('late_pair', 2)]
    h = g['runs'][0]['hash']
    i = g['classes']['equal_hash_unequal_length']
    assert h[i] == h[i + 1] and len(members(db, k('equal_hash_unequal_length'))) == 1
    i = g['classes']['lower_case']
    assert h[i] == h[i + 1] and len(members(db, k('lower_case'))) == 1
    assert members(db, k('bzx')) == [k('bzx'), k('bzx', 1), k('bzx', 2)] or members(db, k('bzx')) == [k('bzx'), k('bzx', 2)]
    zero = lines(g['runs'][1]['db'], k('lower_case'))
    assert len(zero) == 2 and zero[1][2] == b'0.000'
    assert rec['H']['runs'][0]['unique'] == 1 and max(t.count(b'\n') for t in rec['H']['runs'][0]['db'].values()) == 5000
    assert sum(t.count(b'\n') == 1 for t in rec['H']['runs'][0]['db'].values()) == 4999 + 50
    assert all(t.count(b'\n') == 1 for t in rec['N']['runs'][0]['db'].values()) and len(rec['O']['runs'][0]['db']) == 1


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--time':
        return time_driver(sys.argv[2], int(sys.argv[3]))
    ref_root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    matrix = os.path.join(ref_root, 'lib', 'mmseqs', 'data', 'blosum62.out')
    map3 = host_map256(3)
    cl = Classes(map3)
    out, rec = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        for name, maker in (('S', lambda: set_s(cl)), ('T', lambda: set_t(cl)), ('G', lambda: set_g(cl, map3)), ('O', set_one), ('N', set_nopair),
                            ('H', lambda: set_h(cl)), ('A', lambda: set_a(cl)), ('C1', lambda: (example_proteins(), [(3, 0.99)], {}))):
            seqs, runs, classes = maker()
            letters, off = flat(seqs)
            keys = (5 + 3 * np.arange(len(seqs))).astype(np.uint32)
            if name != 'C1':
                out[name + '_let'], out[name + '_off'] = letters, off
            out[name + '_keys'] = keys
            out[name + '_class_names'] = np.array(sorted(classes), dtype='U40') if classes else np.zeros(0, 'U40')
            out[name + '_class_seq'] = np.array([classes[c] for c in sorted(classes)], np.int64)
            out[name + '_runs'] = np.int64(len(runs))
            rec[name] = dict(keys=keys, off=off, letters=letters, classes=classes, runs=[])
            for r, (alph, thr) in enumerate(runs):
                got = run_driver(exe, tmp, matrix, alph, thr, letters, off, keys)
                tag = '%s_r%d' % (name, r)
                assert np.array_equal(got['map'][:255], host_map256(alph)[:255]), (tag, 'sd_host_reduced_alphabet differs from the reduced matrix')
                fb, ident, h, stats = ref.clusthash(letters, off, got['map'], thr)
                assert np.array_equal(h, got['hash']), tag
                assert ref.entries(keys, off, fb, ident) == got['db'], tag
                assert stats['unique_hashes'] == got['unique'], tag
                out[tag + '_par'] = np.array([alph, thr], np.float64)
                out[tag + '_map'], out[tag + '_hash'], out[tag + '_unique'] = got['map'], got['hash'], np.int64(got['unique'])
                pack_db(out, tag + '_db', got['db'])
                rec[name]['runs'].append(dict(db=got['db'], hash=got['hash'], unique=got['unique'], found_by=fb, map=got['map'], thr=thr, stats=stats))
                print('%s: %d sequences, alphabet %d, threshold %g: %d unique hashes, %d groups, %d pairs, largest group %d, %d found' %
                      (tag, len(keys), alph, thr, got['unique'], stats['groups'], stats['pairs'], stats['largest_group'], int((fb != ref.NONE).sum())))
        check_classes(rec)
        # the misreadings on G: bytes against codes changes entries; the two about j < i change the comparisons made and no entry
        # (clusthash_ref.py says why)
        g = rec['G']
        for r, run in enumerate(g['runs']):
            for drop in ('j_gt_i', 'skip_reps', 'codes'):
                fb, ident, _, stats = ref.clusthash(g['letters'], g['off'], run['map'], run['thr'], drop=drop)
                same = ref.entries(g['keys'], g['off'], fb, ident) == run['db']
                print('G_r%d with %s: entries %s, %d pairs (literal: %d)' % (r, drop, 'equal' if same else 'differ', stats['pairs'], run['stats']['pairs']))
                assert same == (drop != 'codes'), (r, drop)
                if drop == 'j_gt_i' and r == 0:   # (at threshold 0 the first of a group marks all: nobody looks back)
                    assert stats['pairs'] < run['stats']['pairs']
    save(OUT, out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


def time_driver(npz, threads):
    z = np.load(npz)
    ref_root = '/root/reference'
    matrix = os.path.join(ref_root, 'lib', 'mmseqs', 'data', 'blosum62.out')
    n = len(z['off']) - 1
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        ts = [run_driver(exe, tmp, matrix, 3, 0.99, z['letters'], z['off'], np.arange(n, dtype=np.uint32), threads=threads)['seconds'] for _ in range(3)]
    print('reference driver, %d threads, %d sequences: clusthash() %s s (3 runs)' % (threads, n, [round(t, 3) for t in ts]))


if __name__ == '__main__':
    main()
