#!/usr/bin/env python3
"""Writes tests/golden/kmermatch_vectors.npz from the LIVE reference: what `kmermatcher` (M/src/linclust/kmermatcher.cpp) makes of an
amino-acid sequence DB that fits one split.  Inputs, parameters and recorded outputs only.

The module itself cannot be linked (Parameters.cpp needs generated headers; DBReader / DBWriter are files), so DRIVER below includes
kmermatcher.cpp and ReducedMatrix.cpp where they lie, links oracle/_ref/libsdref.so for Sequence, Indexer, SubstitutionMatrix, BaseMatrix,
Util and Debug, and is linked with section GC so that what kmermatcher.cpp's unused functions need stays out.  Function by function:

  the reference's own object code
    SubstitutionMatrix, ReducedMatrix                 the letter map is read from the constructed matrix's aa2num
    fillKmerPositionArray<0, T>                       with Sequence::mapSequence, Indexer::int2index, XXH64 (xxhash.h), Util::hash: the
                                                      records, in emission order (one thread)
    doComputation<T>                                  fill again (all threads), SORT_PARALLEL with KmerPosition<T>'s comparators,
                                                      assignGroup<0, T>, the second sort
    writeKmerMatcherResult<0, T>                      with QueryMatcher::prefilterHitToBuffer
    computeKmerCount                                  the size of the record array
  reader / writer plumbing defined in the driver (no algorithm)
    DBReader<unsigned int>::getData / getDbKey / getSize / remapData / unmapData   over tables in memory, ids in key order (NOSORT)
    DBWriter::writeData                               into a map key -> text
    Parameters                                        zeroed storage with the members the three functions read set by hand (no constructor
                                                      of the class is linked)
  restated in the driver (weaker evidence; DESIGN 4.17 names them)
    kmermatcher()'s choice of T                       `getMaxSeqLen() < SHRT_MAX` as `longest sequence < 32767`
    kmermatcherInner's array size                     max(1025, computeKmerCount + 1): one split
    the "add missing entries" step                    kmermatcher.cpp:779-790 in the driver's own words: every key that wrote no entry
                                                      gets the line "key 0 0", tab separated (from the written map, not from the reference's flag array)
  restated in Python (weaker evidence)
    setLinearFilterDefault / setKmerLengthAndAlphabet   kmm_ref.params / kmm_ref.auto_k: the runs record the k and alphabet they used

    python tools/make_golden_kmermatch.py [reference root]          (needs `make -C oracle _ref/libsdref.so`; no GPU)
    python tools/make_golden_kmermatch.py --edges [reference root]  (writes tests/golden/kmermatch_edges.npz alone: set E and further
                                                                     runs of G, see main_edges(); reads kmermatch_vectors.npz)
    python tools/make_golden_kmermatch.py --time <file.npz> <threads>   (the driver's seconds on the sequences of tools/bench_kmermatcher.py --dump)

Per set <S>: <S>_res (21-letter codes), <S>_off, and per run <S>_r<i>_{keys, par, map, rec_key, rec_pos, rec_off, db_keys, db_off, db_text}
(par: k, alphabet, kmer-per-seq, scale, hash-shift, cov-mode, c, include-only-extendable; C1 records no sequences -- they are
tests/golden/examples -- and no records).  <S>_class_names / <S>_class_seq name the sequences built for a class.  Sets: see set_s() ... below.
main() asserts every class property with tests/kmm_ref.py before recording, that kmm_ref equals every recorded stage, and that leaving out
each of the three quirks kmm_ref.py names changes a recorded entry of S or G.
kmermatch_edges.npz has the same layout for set E (set_e(): the edges of the device's lane logic) and for the runs r6 .. r8 of G, whose
sequences stay in the first file; <S>_more_runs counts the runs a set of the first file gains there.  tests/kmmgold.py reads both as one.
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
import kmm_ref  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLD, 'kmermatch_vectors.npz')
OUT_EDGES = os.path.join(GOLD, 'kmermatch_edges.npz')
LETTERS = 'ACDEFGHIKLMNPQRSTVWYX'

DRIVER = r'''
#define XXH_INLINE_ALL
#include "xxhash.h"
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
};
static Table g_table;
static std::map<unsigned int, std::string> g_written;
template <> char *DBReader<unsigned int>::getData(size_t id, int) { return g_table.dataOfId[id]; }
template <> unsigned int DBReader<unsigned int>::getDbKey(size_t id) { return g_table.keyOfId[id]; }
template <> size_t DBReader<unsigned int>::getSize() const { return size; }
template <> void DBReader<unsigned int>::remapData() {}
template <> void DBReader<unsigned int>::unmapData() {}
void DBWriter::writeData(const char *data, size_t dataSize, unsigned int key, unsigned int, bool, bool) { g_written[key] = std::string(data, dataSize); }
#include "kmermatcher.cpp"
#include "ReducedMatrix.cpp"
// what doComputation names in branches a run without --weights and with one split never takes: they must link, they must not run
SequenceWeights::SequenceWeights(const char *) { abort(); }
SequenceWeights::~SequenceWeights() {}
float SequenceWeights::getWeightById(unsigned int) { abort(); }
FILE *FileUtil::openFileOrDie(const char *, const char *, bool) { abort(); }

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <typename T>
static void run(FILE *out, DBReader<unsigned int> &rd, Parameters &par, BaseMatrix *subMat, int threads, bool wantRecords) {
    const size_t n = rd.getSize();
    float scale = par.kmersPerSequenceScale.values.aminoacid();
    const size_t totalKmers = computeKmerCount(rd, par.kmerSize, par.kmersPerSequence, scale);
    const size_t perSplit = std::max(static_cast<size_t>(1024 + 1), totalKmers + 1);
    uint64_t nRec = 0;
    if (wantRecords) {
        omp_set_num_threads(1);
        KmerPosition<T> *arr = initKmerPositionMemory<T>(perSplit);
        std::pair<size_t, size_t> ret = fillKmerPositionArray<Parameters::DBTYPE_AMINO_ACIDS, T>(arr, perSplit, rd, par, subMat, true, 0, (size_t) -1, NULL);
        nRec = ret.first;
        fwrite(&nRec, 8, 1, out);
        for (size_t i = 0; i < nRec; i++) {
            uint64_t kmer = arr[i].kmer;
            uint32_t id = arr[i].id;
            int32_t len = arr[i].seqLen, pos = arr[i].pos;
            fwrite(&kmer, 8, 1, out);
            fwrite(&id, 4, 1, out);
            fwrite(&len, 4, 1, out);
            fwrite(&pos, 4, 1, out);
        }
        delete[] arr;
    } else {
        fwrite(&nRec, 8, 1, out);
    }
    omp_set_num_threads(threads);
    const double t0 = now();
    KmerPosition<T> *pairs = doComputation<T>(perSplit, 0, (size_t) -1, std::string(""), rd, par, subMat);
    const double t1 = now();
    // which keys wrote an entry of their own is tracked by the reference's function in a byte per key up to the largest key
    unsigned int largestKey = 0;
    for (size_t i = 0; i < n; i++) largestKey = std::max(largestKey, g_table.keyOfId[i]);
    std::vector<char> isRep(static_cast<size_t>(largestKey) + 1, 0);
    DBWriter *dbw = (DBWriter *) calloc(1, sizeof(DBWriter));
    writeKmerMatcherResult<Parameters::DBTYPE_AMINO_ACIDS>(*dbw, pairs, perSplit, isRep, 1);
    // the module's last step in this driver's own words: a sequence without an entry of its own gets the single line "key 0 0"
    for (size_t i = 0; i < n; i++) {
        const unsigned int key = g_table.keyOfId[i];
        if (g_written.find(key) == g_written.end()) g_written[key] = std::to_string(key) + "\t0\t0\n";
    }
    const double t2 = now();
    uint64_t nEntries = g_written.size();
    fwrite(&nEntries, 8, 1, out);
    for (std::map<unsigned int, std::string>::const_iterator it = g_written.begin(); it != g_written.end(); ++it) {
        uint32_t key = it->first;
        uint64_t len = it->second.size();
        fwrite(&key, 4, 1, out);
        fwrite(&len, 8, 1, out);
        fwrite(it->second.data(), 1, len, out);
    }
    const double tCompute = t1 - t0, tWrite = t2 - t1;
    fwrite(&tCompute, 8, 1, out);
    fwrite(&tWrite, 8, 1, out);
    delete[] pairs;
}

// job: i32 k, alphabet, kmersPerSequence, hashShift, covMode, includeOnlyExtendable, threads, wantRecords; f32 scale, covThr; u32 n;
//      u32 keys[n] ascending; u64 off[n + 1]; letters
// result: u8 map[21]; u64 nRec; nRec x (u64 kmer, u32 id, i32 seqLen, i32 pos); u64 nEntries; per entry u32 key, u64 len, text;
//         f64 seconds of doComputation, of writeKmerMatcherResult + missing entries
int main(int argc, char **argv) {
    if (argc != 4) return 1;
    Debug::setDebugLevel(1);
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 1;
    int hdr[8];
    float fl[2];
    unsigned int n;
    if (fread(hdr, 4, 8, in) != 8 || fread(fl, 4, 2, in) != 2 || fread(&n, 4, 1, in) != 1) return 2;
    std::vector<unsigned int> keys(n);
    std::vector<uint64_t> off(n + 1);
    if (n && fread(keys.data(), 4, n, in) != n) return 2;
    if (fread(off.data(), 8, n + 1, in) != n + 1) return 2;
    std::vector<char> letters(off[n] + 1);
    if (off[n] && fread(letters.data(), 1, off[n], in) != off[n]) return 2;
    fclose(in);
    std::vector<std::string> text(n);
    size_t maxLen = 0;
    for (unsigned int i = 0; i < n; i++) {
        text[i].assign(letters.data() + off[i], off[i + 1] - off[i]);
        text[i] += "\n";
        maxLen = std::max(maxLen, (size_t) (off[i + 1] - off[i]));
    }
    DBReader<unsigned int> *rd = (DBReader<unsigned int> *) calloc(1, sizeof(DBReader<unsigned int>));
    rd->size = n;
    rd->dbtype = Parameters::DBTYPE_AMINO_ACIDS;
    rd->index = (DBReader<unsigned int>::Index *) calloc(n + 1, sizeof(DBReader<unsigned int>::Index));
    for (unsigned int i = 0; i < n; i++) {
        rd->index[i].length = (unsigned int) (off[i + 1] - off[i]) + 2;
        g_table.keyOfId.push_back(keys[i]);
        g_table.dataOfId.push_back(&text[i][0]);
    }
    Parameters *par = (Parameters *) calloc(1, sizeof(Parameters));
    new (&par->spacedKmerPattern) std::string("");
    new (&par->kmersPerSequenceScale) MultiParam<NuclAA<float>>(NuclAA<float>(fl[0], 0.2));
    par->kmerSize = hdr[0];
    par->kmersPerSequence = hdr[2];
    par->hashShift = hdr[3];
    par->covMode = hdr[4];
    par->covThr = fl[1];
    par->includeOnlyExtendable = hdr[5] != 0;
    par->maskMode = 0;
    par->spacedKmer = false;
    par->adjustKmerLength = false;
    par->ignoreMultiKmer = false;
    par->pickNbest = 1;
    par->maxSeqLen = 65535;
    par->weightThr = 0.9;
    BaseMatrix *subMat;
    if (hdr[1] == 21) {
        subMat = new SubstitutionMatrix(argv[3], 2.0, 0.0);
    } else {
        SubstitutionMatrix sMat(argv[3], 8.0, -0.2f);
        subMat = new ReducedMatrix(sMat.probMatrix, sMat.subMatrixPseudoCounts, sMat.aa2num, sMat.num2aa, sMat.alphabetSize, hdr[1], 2.0);
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 1;
    const char *order = "ACDEFGHIKLMNPQRSTVWYX";
    for (int a = 0; a < 21; a++) fputc(subMat->aa2num[(int) order[a]], out);
    if (maxLen < SHRT_MAX) run<short>(out, *rd, *par, subMat, hdr[6], hdr[7] != 0);
    else run<int>(out, *rd, *par, subMat, hdr[6], hdr[7] != 0);
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


def run_driver(exe, tmp, matrix, par, residues, offsets, keys, threads=4, want_records=True):
    """-> dict(map, rec_key, rec_id, rec_len, rec_pos, db, t_compute, t_write); the driver reads the sequences in key order"""
    keys = np.asarray(keys, np.uint32)
    order = np.argsort(keys, kind='stable')
    offsets = np.asarray(offsets, np.int64)
    lut = np.frombuffer(LETTERS.encode(), np.uint8)
    parts = [lut[residues[offsets[i]:offsets[i + 1]]] for i in order]
    off = np.zeros(len(keys) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    job, res = os.path.join(tmp, 'job.bin'), os.path.join(tmp, 'res.bin')
    with open(job, 'wb') as f:
        f.write(struct.pack('<8i2fI', par['k'], par['alph_size'], par['kmer_per_seq'], par['hash_shift'], par['cov_mode'],
                            int(par['include_only_extendable']), threads, int(want_records), par['kmer_per_seq_scale'], par['c'], len(keys)))
        f.write(keys[order].tobytes() + off.tobytes() + (np.concatenate(parts).tobytes() if parts else b''))
    subprocess.check_call([exe, job, res, matrix], stdout=subprocess.DEVNULL)
    raw = open(res, 'rb').read()
    out = dict(map=np.frombuffer(raw, np.uint8, 21, 0).copy())
    at = 21
    n_rec, = struct.unpack_from('<Q', raw, at)
    at += 8
    rec = np.frombuffer(raw, np.dtype([('key', '<u8'), ('id', '<u4'), ('len', '<i4'), ('pos', '<i4')]), n_rec, at)
    at += 20 * n_rec
    out.update(rec_key=rec['key'].copy(), rec_id=rec['id'].copy(), rec_len=rec['len'].copy(), rec_pos=rec['pos'].copy())
    n_ent, = struct.unpack_from('<Q', raw, at)
    at += 8
    db = {}
    for _ in range(n_ent):
        key, ln = struct.unpack_from('<IQ', raw, at)
        at += 12
        db[key] = raw[at:at + ln]
        at += ln
    out['db'] = db
    out['t_compute'], out['t_write'] = struct.unpack_from('<dd', raw, at)
    assert at + 16 == len(raw)
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


def par_array(par):
    return np.array([par['k'], par['alph_size'], par['kmer_per_seq'], par['kmer_per_seq_scale'], par['hash_shift'], par['cov_mode'], par['c'],
                     int(par['include_only_extendable'])], np.float64)


# ---- the sets ----------------------------------------------------------------------------------------------------------------------
def rnd(rng, length):
    return rng.integers(0, 20, length).astype(np.uint8)


def mutate(rng, seq, rate):
    s = seq.copy()
    hit = rng.random(len(s)) < rate
    s[hit] = rng.integers(0, 20, int(hit.sum()))
    return s


def flat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs).astype(np.uint8) if seqs else np.zeros(0, np.uint8)), off


selection_info = kmm_ref.selection_info


def set_s(lmap):
    """selection: (seqs, keys, runs, classes).  Runs: r0 defaults at k 10; r1 --kmer-per-seq 2000 (the last-bin cases on 3 000 residues);
    r2 --kmer-per-seq-scale 0.013; r3 --kmer-per-seq 1"""
    rng = np.random.default_rng(7)
    runs = [kmm_ref.params(k=10), kmm_ref.params(k=10, kmer_per_seq=2000), kmm_ref.params(k=10, kmer_per_seq_scale=0.013),
            kmm_ref.params(k=10, kmer_per_seq=1)]
    seqs, classes = [], {}

    def add(name, s):
        classes[name] = len(seqs)
        seqs.append(np.asarray(s, np.uint8))

    add('shorter_than_k', rnd(rng, 5))
    add('length_k', rnd(rng, 10))
    add('all_taken', rnd(rng, 25))
    s = rnd(rng, 90)
    s[[3, 40, 41, 77]] = 20
    add('windows_with_x', s)
    add('all_x', np.full(30, 20, np.uint8))
    found = {}
    while len(found) < 2:   # the threshold of r0 on a multiple of 512, and one past it
        s = rnd(rng, 300)
        _, cons, thr, _, _ = selection_info(runs[0], s, lmap)
        if thr % 512 in (0, 1) and (thr % 512) not in found:
            found[thr % 512] = s
    add('threshold_multiple_of_512', found[0])
    add('threshold_one_past_512', found[1])
    quirk = e0 = None
    while quirk is None or e0 is None:   # r1: 2 991 windows, 1 999 considered: the last bin often holds several
        s = rnd(rng, 3000)
        _, cons, thr, e, c = selection_info(runs[1], s, lmap)
        if quirk is None and c >= 3 and 0 < e < c and e != c - e:
            quirk = s
        elif e0 is None and e == 0 and c >= 2:
            e0 = s
    add('last_bin_quirk', quirk)
    add('last_bin_whole', e0)
    base = len(seqs)
    for i in range(12):   # relatives, so that the set has hits
        root = rnd(rng, int(rng.integers(60, 260)))
        seqs.append(root)
        seqs.append(mutate(rng, root, 0.08)[:int(len(root) * 0.9)])
    seqs.append(mutate(rng, quirk, 0.02))
    seqs.append(mutate(rng, e0, 0.02))
    classes['relatives_from'] = base
    keys = np.arange(len(seqs), dtype=np.uint32)
    return seqs, [keys] * len(runs), runs, classes


def set_g(lmap):
    """grouping: keys 3 + 7 i.  Runs: r0 defaults at k 10; r1 the two keys of equal_lengths swapped; r2 / r3 --cov-mode 1 / 2; r4
    --include-only-extendable 1; r5 -c 0.5"""
    rng = np.random.default_rng(11)
    seqs, classes = [], {}

    def add(name, *ss):
        classes[name] = len(seqs)
        seqs.extend(np.asarray(s, np.uint8) for s in ss)

    a = rnd(rng, 120)
    add('identical', a, a.copy())
    a = rnd(rng, 110)
    groups = {}
    for letter in range(20):
        groups.setdefault(int(lmap[letter]), []).append(letter)
    swap = np.arange(21)
    for g in groups.values():
        if len(g) > 1:
            for x, y in zip(g, g[1:] + g[:1]):
                swap[x] = y
    b = swap[a].astype(np.uint8)
    assert (b != a).any() and (lmap[a] == lmap[b]).all()
    add('identical_under_13', a, b)
    a = rnd(rng, 150)
    add('equal_lengths', a, mutate(rng, a, 0.05))
    unit = rnd(rng, 40)
    add('repeat_alone', np.concatenate([rnd(rng, 20), unit, unit, rnd(rng, 20)]))
    unit = rnd(rng, 40)
    rep = np.concatenate([rnd(rng, 25), unit, unit, rnd(rng, 25)])
    add('repeat_shared', rep, np.concatenate([rnd(rng, 10), unit, unit, rnd(rng, 25)]))
    a = rnd(rng, 140)
    add('one_diagonal', a, mutate(rng, a, 0.03)[:130])
    a = rnd(rng, 150)
    add('longer_has_larger_key', a[:130].copy(), a)
    a = rnd(rng, 200)
    add('negative_diagonal', np.concatenate([a, rnd(rng, 30)]), np.concatenate([rnd(rng, 10), a]))
    a = rnd(rng, 100)
    add('coverage', a, a[:80].copy(), a[:79].copy(), a[20:].copy(), a[21:].copy())
    tie = None
    while tie is None:   # two diagonals with equally many shared k-mers: found where the reference's `>=` and a `>` disagree
        a = rnd(rng, 160)
        b = np.concatenate([a[:75], rnd(rng, 6), a[75:]])[:155]
        res, off = flat([a, b])
        keys = np.array([0, 1], np.uint32)
        h1 = kmm_ref.kmermatch(kmm_ref.params(k=10), res, off, keys, lmap)[0]
        h2 = kmm_ref.kmermatch(kmm_ref.params(k=10), res, off, keys, lmap, drop='tie')[0]
        if len(h1) and not np.array_equal(h1, h2):
            tie = (a, b)
    add('diagonal_tie', *tie)
    keys = (3 + 7 * np.arange(len(seqs))).astype(np.uint32)
    swapped = keys.copy()
    i = classes['equal_lengths']
    swapped[[i, i + 1]] = swapped[[i + 1, i]]
    runs = [kmm_ref.params(k=10), kmm_ref.params(k=10), kmm_ref.params(k=10, cov_mode=1), kmm_ref.params(k=10, cov_mode=2),
            kmm_ref.params(k=10, include_only_extendable=True), kmm_ref.params(k=10, c=0.5)]
    return seqs, [keys, swapped, keys, keys, keys, keys], runs, classes


def set_h():
    """a hub: one 12-mer shared by 5 000 sequences of 20 residues (all of their 11 windows are taken)"""
    rng = np.random.default_rng(13)
    hub = rnd(rng, 12)
    seqs = [np.concatenate([hub, rnd(rng, 8)]) for _ in range(5000)]
    return seqs, [np.arange(5000, dtype=np.uint32)], [kmm_ref.params(k=10)], {'hub': 0}


def set_a():
    """300 related sequences: 30 families of 10.  Runs: alphabet 13 / 21 x k 10 / 14; -k 0 at --min-seq-id 0.5, 0.9, 1.0; --hash-shift 5, 1000"""
    rng = np.random.default_rng(17)
    seqs = []
    for f in range(30):
        root = rnd(rng, int(rng.integers(80, 300)))
        for m in range(10):
            s = mutate(rng, root, rng.uniform(0.02, 0.2))
            seqs.append(s[:int(len(s) * rng.uniform(0.75, 1.0))])
    total = sum(len(s) for s in seqs)
    runs = [kmm_ref.params(k=k, alph_size=a) for a in (13, 21) for k in (10, 14)]
    runs += [kmm_ref.params(k=0, min_seq_id=m, residues=total) for m in (0.5, 0.9, 1.0)]
    runs += [kmm_ref.params(k=10, hash_shift=h) for h in (5, 1000)]
    order = rng.permutation(300).astype(np.uint32)
    return seqs, [order] * len(runs), runs, {}


def set_w():
    """T = int: one sequence of 32 767 residues among 24 short ones, half of them pieces of it.  Runs: r0 --kmer-per-seq-scale 0.05 -c 0;
    r1 the defaults at k 10 (what the one-call test of all sets uses)"""
    rng = np.random.default_rng(19)
    long_seq = rnd(rng, 32767)
    seqs = [long_seq]
    for i in range(12):
        at = int(rng.integers(0, 32767 - 400))
        if i == 0:
            at = 32767 - 300
        seqs.append(mutate(rng, long_seq[at:at + 300], 0.02))
        seqs.append(rnd(rng, int(rng.integers(50, 300))))
    keys = np.arange(len(seqs), dtype=np.uint32)
    return seqs, [keys, keys], [kmm_ref.params(k=10, kmer_per_seq_scale=0.05, c=0.0), kmm_ref.params(k=10)], {'long': 0}


E_LENGTHS = (9, 10, 11, 63, 64, 65, 73, 74, 127, 128, 129, 137, 138, 201)   # k - 1, k, k + 1; 64, 65, 128 and 129 windows at k 10
E_PERIODS = (1, 2, 3, 5, 7)


def set_e(lmap):
    """the edges of the device's lane logic (kmermatch_edges.npz): 64-window chunks, 64 lane blocks of the identity hash, X on chunk edges,
    repeats (nothing is masked), thresholds at both ends of the score range.  Keys shuffled and not dense.  Runs: r0 defaults at k 10;
    r1 / r2 --kmer-per-seq 150 / 300; r3 --kmer-per-seq-scale 1.0; r4 --kmer-per-seq 2; r5 k 14 on 21 letters; r6 --hash-shift -3"""
    rng = np.random.default_rng(29)
    runs = [kmm_ref.params(k=10), kmm_ref.params(k=10, kmer_per_seq=150), kmm_ref.params(k=10, kmer_per_seq=300),
            kmm_ref.params(k=10, kmer_per_seq_scale=1.0), kmm_ref.params(k=10, kmer_per_seq=2), kmm_ref.params(k=14, alph_size=21),
            kmm_ref.params(k=10, hash_shift=-3)]
    seqs, classes = [], {}

    def add(name, s):
        classes[name] = len(seqs)
        seqs.append(np.asarray(s, np.uint8))

    for length in E_LENGTHS:
        add('length_%d' % length, rnd(rng, length))
    for name, at in (('x_at_63', [63]), ('x_at_64', [64]), ('x_at_73', [73]), ('ends_in_x', [199]),
                     # every window that starts before 64 or from 128 on holds an X: windows 64 .. 127 alone are free
                     ('free_in_second_chunk_only', list(range(3, 64, 10)) + list(range(137, 200, 10)))):
        s = rnd(rng, 200)
        s[at] = 20
        add(name, s)
    # letters of seven different classes of the 13-letter alphabet, so that the period stays what it is after reduction
    unit = np.array([LETTERS.index(c) for c in 'ACDEFGH'], np.uint8)
    assert len(set(lmap[unit].tolist())) == 7
    for p in E_PERIODS:
        add('period_%d' % p, np.tile(unit[:p], 400 // p + 1)[:400])
    s = rnd(rng, 300)
    s[90:210] = LETTERS.index('K')
    add('homopolymer_inside', s)
    top = bottom = coarse0 = None
    while top is None or bottom is None:
        s = rnd(rng, 300)
        if top is None and selection_info(runs[3], s, lmap)[2] == 65536:
            top = s
        elif bottom is None and selection_info(runs[4], s, lmap)[2] == 1:
            bottom = s
    while coarse0 is None:
        s = rnd(rng, 3000)
        if selection_info(runs[0], s, lmap)[2] < 512:
            coarse0 = s
    add('threshold_65536', top)
    add('threshold_1', bottom)
    add('threshold_in_coarse_bin_0', coarse0)
    base = len(seqs)
    for c in ('length_201', 'length_138', 'x_at_64', 'free_in_second_chunk_only', 'homopolymer_inside', 'threshold_65536', 'threshold_1'):
        seqs.append(mutate(rng, seqs[classes[c]], 0.04))
    for p in E_PERIODS:   # a repeat with a few residues changed, and a shorter stretch of the same repeat
        seqs.append(mutate(rng, seqs[classes['period_%d' % p]], 0.02))
    seqs.append(seqs[classes['period_3']][:330].copy())
    seqs.append(seqs[classes['period_7']][5:370].copy())
    seqs.append(mutate(rng, coarse0, 0.02)[:2800])
    classes['relatives_from'] = base
    keys = (11 + 37 * rng.permutation(len(seqs))).astype(np.uint32)
    return seqs, [keys] * len(runs), runs, classes


def check_classes_e(recorded, lmap13):
    """the class properties of set E, from the restatement alone"""
    par, res, off, keys, lmap, db, seqs, cl = recorded['E_r0']
    info = lambda run, c: selection_info(recorded['E_r%d' % run][0], seqs[cl[c]], lmap13)
    for length in E_LENGTHS:
        assert info(0, 'length_%d' % length)[0] == max(length - 9, 0)
    assert [info(0, 'length_%d' % n)[0] for n in (73, 74, 137, 138)] == [64, 65, 128, 129]
    assert [info(0, c)[0] for c in ('x_at_63', 'x_at_64', 'x_at_73', 'ends_in_x')] == [181, 181, 181, 190]
    rec = kmm_ref.records(recorded['E_r1'][0], *flat([seqs[cl['free_in_second_chunk_only']]]), np.array([0], np.uint32), lmap13)
    assert info(1, 'free_in_second_chunk_only')[:2] == (64, 64) and rec[3][1:].tolist() == list(range(64, 128))
    # repeats: p different windows, each some 391 / p times -- whole score bins of equal windows
    w, cons, thr, e, c = info(1, 'period_3')
    assert (w, cons) == (391, 149) and e > 64 and c > 64

    def from_last_bin(run, c):
        """positions of the windows taken from the last bin"""
        p = recorded['E_r%d' % run][0]
        rec = kmm_ref.records(p, *flat([seqs[cl[c]]]), np.array([0], np.uint32), lmap13)
        score = (kmm_ref.xxh64_word(rec[0][1:], p['hash_shift']) & np.uint64(0xFFFF)).astype(np.int64)
        return rec[3][1:][score == info(run, c)[2] - 1], len(score)

    # (kmerConsidered ends this selection, after 75 windows of the last bin in four 64-window chunks)
    taken, selected = from_last_bin(1, 'period_3')
    assert selected == cons and 64 < len(taken) < e and len(set((taken // 64).tolist())) >= 3
    # the excess ends these two, in the second chunk or later: fewer than kmerConsidered windows are taken, and the count of last-bin
    # windows seen has to be carried from chunk to chunk
    for run, c in ((2, 'period_1'), (1, 'period_2')):
        w, cons, thr, e, c_last = info(run, c)
        taken, selected = from_last_bin(run, c)
        assert 0 < e < c_last and len(taken) == e and selected < cons and int(taken.max()) >= 64, (run, c)
    assert info(2, 'period_1')[3] > 64   # (more than a chunk of them)
    w, cons, thr, e, c = info(0, 'period_1')
    assert (w, cons, c) == (391, 19, 391) and e == 372 and e > cons
    for p in E_PERIODS:
        assert info(2, 'period_%d' % p)[4] >= 391 // p
    assert info(3, 'threshold_65536')[1:3] == (291, 65536) and info(4, 'threshold_1')[1:3] == (1, 1)
    assert info(0, 'threshold_in_coarse_bin_0')[2] < 512 and info(0, 'threshold_in_coarse_bin_0')[0] == 2991
    assert sum(t.count(b'\n') > 1 for t in db.values()) >= 8   # the relatives give hits and groups
    assert len(set(np.diff(np.sort(keys)).tolist())) == 1 and int(np.diff(np.sort(keys))[0]) == 37 and (np.diff(keys.astype(np.int64)) < 0).any()
    assert recorded['E_r5'][0]['alph_size'] == 21 and recorded['E_r6'][0]['hash_shift'] == -3
    rec = kmm_ref.records(recorded['E_r5'][0], *flat([seqs[cl['length_201']]]), np.array([0], np.uint32), recorded['E_r5'][4])
    assert (rec[0][1:] >> np.uint64(32)).any()   # 20^13 and more: the k-mer index of 14 letters uses the key's high word


def check_coverage_modes(recorded):
    """G under --cov-mode 3, 4 and 5 at -c 0.8: the members of the `coverage` representative (100 residues; pieces of 80, 79, 80, 79).
    A representative is the longest sequence of its run (the first sort's seqLen-descending field), so target / query = min / max <= 1
    for every pair: modes 3 and 5 must coincide, here and everywhere.  Mode 4 asks query / target <= 1: only members as long as the
    representative remain, none of `coverage` and the second of `identical`."""
    par, res, off, keys, lmap, db, seqs, cl = recorded['G_r6']
    lines = lambda d, k: [tuple(int(x) for x in l.split(b'\t')) for l in d[k].splitlines()]
    k = [int(keys[cl['coverage'] + j]) for j in range(5)]
    cov = lambda tag: [l[0] for l in lines(recorded[tag][5], k[0])][1:]
    assert [recorded['G_r%d' % r][0]['cov_mode'] for r in (6, 7, 8)] == [3, 4, 5]
    assert cov('G_r6') == [k[1], k[3]] and cov('G_r7') == [] and cov('G_r8') == [k[1], k[3]]
    i = cl['identical']
    assert [l[0] for l in lines(recorded['G_r7'][5], int(keys[i]))] == [int(keys[i]), int(keys[i + 1])]


def set_c1():
    from spacedust_amd.api import Host
    host = Host()
    aa2num = host.matrix(0)[2]
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
    seqs = [aa2num[np.frombuffer(s.encode(), np.uint8)].astype(np.uint8) for s in seqs]
    total = sum(len(s) for s in seqs)
    return seqs, [np.arange(len(seqs), dtype=np.uint32)], [kmm_ref.params(k=0, residues=total)], {}


def blosum_prob():
    from spacedust_amd import _lib
    import ctypes as C
    # the joint probabilities kmm_ref.reduced_alphabet takes: rebuilt from the matrix text as SubstitutionMatrix::readProbMatrix does
    buf = C.create_string_buffer(1 << 16)
    L = _lib.load()
    L.sd_host_matrix_text.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    L.sd_host_matrix_text(0, buf, 1 << 16)
    return kmm_ref.matrix_prob(buf.value.decode())


def record_run(out, recorded, exe, tmp, matrix, prob, name, r, par, keys, res, off, seqs, classes):
    """one run of the driver into out / recorded, after the restatement has been held against every stage of it"""
    got = run_driver(exe, tmp, matrix, par, res, off, keys, want_records=name != 'C1')
    tag = '%s_r%d' % (name, r)
    out[tag + '_keys'], out[tag + '_par'], out[tag + '_map'] = keys, par_array(par), got['map']
    lmap = kmm_ref.reduced_alphabet(prob, par['alph_size'])
    assert np.array_equal(lmap, got['map']), (tag, lmap, got['map'])
    hits, stats, rec = kmm_ref.kmermatch(par, res, off, keys, lmap)
    if name != 'C1':
        # emission order: the driver reads in key order; per sequence (key, pos) as emitted
        order = np.argsort(keys, kind='stable')
        want_key = np.concatenate([rec[0][rec[4][i]:rec[4][i + 1]] for i in order])
        want_pos = np.concatenate([rec[3][rec[4][i]:rec[4][i + 1]] for i in order])
        want_id = np.concatenate([rec[1][rec[4][i]:rec[4][i + 1]] for i in order])
        assert np.array_equal(got['rec_id'], want_id), tag
        assert np.array_equal(got['rec_key'], want_key) and np.array_equal(got['rec_pos'], want_pos), tag
        out[tag + '_rec_key'], out[tag + '_rec_pos'] = got['rec_key'], got['rec_pos'].astype(np.int32)
        cnt = np.diff(rec[4])[order]
        out[tag + '_rec_off'] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    assert kmm_ref.entries(keys, hits) == got['db'], tag
    pack_db(out, tag + '_db', got['db'])
    recorded[tag] = (par, res, off, keys, lmap, got['db'], seqs, classes)
    print('%s: %d sequences, %d records, %d grouped, %d hits, largest group %d' % (tag, len(keys), stats['records'], stats['grouped'],
                                                                                 stats['hits'], stats['largest_group']))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--time':
        return time_driver(sys.argv[2], int(sys.argv[3]))
    edges = len(sys.argv) > 1 and sys.argv[1] == '--edges'
    args = sys.argv[2:] if edges else sys.argv[1:]
    ref_root = args[0] if args else '/root/reference'
    matrix = os.path.join(ref_root, 'lib', 'mmseqs', 'data', 'blosum62.out')
    prob = blosum_prob()
    lmap13 = kmm_ref.reduced_alphabet(prob, 13)
    if edges:
        return main_edges(ref_root, matrix, prob, lmap13)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        recorded = {}
        for name, maker in (('S', lambda: set_s(lmap13)), ('G', lambda: set_g(lmap13)), ('H', set_h), ('A', set_a), ('W', set_w), ('C1', set_c1)):
            seqs, keys_of_run, runs, classes = maker()
            res, off = flat(seqs)
            if name != 'C1':
                out[name + '_res'], out[name + '_off'] = res, off
            out[name + '_class_names'] = np.array(sorted(classes), dtype='U40') if classes else np.zeros(0, 'U40')
            out[name + '_class_seq'] = np.array([classes[c] for c in sorted(classes)], np.int64)
            out[name + '_runs'] = np.int64(len(runs))
            for r, (par, keys) in enumerate(zip(runs, keys_of_run)):
                record_run(out, recorded, exe, tmp, matrix, prob, name, r, par, keys, res, off, seqs, classes)
        check_classes(recorded, lmap13)
        # each quirk left out changes a recorded entry of S or G
        for drop in ('last_bin', 'tie', 'len_desc'):
            changed = []
            for tag, (par, res, off, keys, lmap, db, _, _) in recorded.items():
                if tag[0] in 'SG':
                    hits = kmm_ref.kmermatch(par, res, off, keys, lmap, drop=drop)[0]
                    if kmm_ref.entries(keys, hits) != db:
                        changed.append(tag)
            assert changed, 'leaving out %s changes no recorded entry of S or G' % drop
            print('without %s: %s differ' % (drop, ', '.join(changed)))
    save(OUT, out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


def main_edges(ref_root, matrix, prob, lmap13):
    """kmermatch_edges.npz: set E, and set G again under --cov-mode 3, 4 and 5 as its runs r6 .. r8 (G's sequences and keys are those of
    kmermatch_vectors.npz, which this mode reads and does not write: <S>_more_runs counts the runs a set gains here)"""
    old = np.load(OUT)
    out, recorded = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        seqs, keys_of_run, runs, classes = set_e(lmap13)
        res, off = flat(seqs)
        out['E_res'], out['E_off'] = res, off
        out['E_class_names'] = np.array(sorted(classes), dtype='U40')
        out['E_class_seq'] = np.array([classes[c] for c in sorted(classes)], np.int64)
        out['E_runs'] = np.int64(len(runs))
        for r, (par, keys) in enumerate(zip(runs, keys_of_run)):
            record_run(out, recorded, exe, tmp, matrix, prob, 'E', r, par, keys, res, off, seqs, classes)
        check_classes_e(recorded, lmap13)
        seqs, keys_of_run, runs, classes = set_g(lmap13)
        res, off = flat(seqs)
        assert np.array_equal(res, old['G_res']) and np.array_equal(off, old['G_off']) and np.array_equal(keys_of_run[0], old['G_r0_keys'])
        first = int(old['G_runs'])
        out['G_more_runs'] = np.int64(3)
        for r, mode in enumerate((3, 4, 5)):
            record_run(out, recorded, exe, tmp, matrix, prob, 'G', first + r, kmm_ref.params(k=10, cov_mode=mode, c=0.8), keys_of_run[0], res, off,
                       seqs, classes)
        check_coverage_modes(recorded)
    save(OUT_EDGES, out)
    print('wrote %s (%d bytes)' % (OUT_EDGES, os.path.getsize(OUT_EDGES)))


def check_classes(recorded, lmap13):
    """the named class properties, on the CPU, before anything is recorded"""
    par, res, off, keys, lmap, db, seqs, cl = recorded['S_r0']
    info = lambda run, c: selection_info(recorded['S_r%d' % run][0], seqs[cl[c]], lmap13)
    assert info(0, 'shorter_than_k')[0] == 0 and info(0, 'length_k')[:2] == (1, 1)
    w, cons, thr, e, c = info(0, 'all_taken')
    assert w == 16 and cons == 16 and e == 0
    assert 0 < info(0, 'windows_with_x')[0] < 81 and info(0, 'all_x')[0] == 0
    assert info(0, 'threshold_multiple_of_512')[2] % 512 == 0 and info(0, 'threshold_one_past_512')[2] % 512 == 1
    w, cons, thr, e, c = info(1, 'last_bin_quirk')
    assert c >= 3 and 0 < e < c and e != c - e
    w, cons, thr, e, c = info(1, 'last_bin_whole')
    assert e == 0 and c >= 2
    want = np.float32(19) + np.float32(0.013) * np.float32(len(seqs[cl['windows_with_x']]))
    assert want != int(want)
    assert all(info(3, c)[1] == 0 for c in cl if c != 'relatives_from')   # --kmer-per-seq 1: kmerConsidered 0
    assert any(t.count(b'\n') > 1 for t in db.values())
    par, res, off, keys, lmap, db, seqs, cl = recorded['G_r0']
    key_of = lambda c, i=0: int(keys[cl[c] + i])
    lines = lambda d, k: [tuple(int(x) for x in l.split(b'\t')) for l in d[k].splitlines()]
    for c in ('identical', 'identical_under_13'):
        assert [l[0] for l in lines(db, key_of(c))] == [key_of(c), key_of(c, 1)] and lines(db, key_of(c, 1)) == [(key_of(c, 1), 0, 0)]
    assert len(lines(db, key_of('equal_lengths'))) == 2 and len(lines(db, key_of('equal_lengths', 1))) == 1
    db1, keys1 = recorded['G_r1'][5], recorded['G_r1'][3]
    i = cl['equal_lengths']
    assert len(lines(db1, int(keys1[i + 1]))) == 2 and len(lines(db1, int(keys1[i]))) == 1   # the smaller key leads, whichever sequence has it
    assert lines(db, key_of('repeat_alone')) == [(key_of('repeat_alone'), 0, 0)]
    hits, stats, rec = kmm_ref.kmermatch(par, *flat([seqs[cl['repeat_alone']]]), np.array([5], np.uint32), lmap)
    assert stats['largest_group'] >= 2 and stats['grouped'] >= 2 and stats['hits'] == 0   # repeated inside, shared with nobody
    rs = lines(db, key_of('repeat_shared'))
    assert len(rs) == 2 and rs[1][0] == key_of('repeat_shared', 1)
    od = lines(db, key_of('one_diagonal'))
    assert len(od) == 2 and od[1][1] >= 3 and od[1][2] == 0
    assert len(lines(db, key_of('longer_has_larger_key', 1))) == 2 and len(lines(db, key_of('longer_has_larger_key'))) == 1
    nd = lines(db, key_of('negative_diagonal'))
    assert len(nd) == 2 and nd[1][2] == -10
    cov = lambda d: [l[0] for l in lines(d, key_of('coverage'))][1:]
    k = [key_of('coverage', j) for j in range(5)]
    assert cov(db) == [k[1], k[3]] and cov(recorded['G_r2'][5]) == k[1:] and cov(recorded['G_r3'][5]) == [k[1], k[3]]
    assert cov(recorded['G_r5'][5]) == k[1:]
    ext = recorded['G_r4'][5]
    assert len(lines(ext, key_of('coverage'))) == 1   # pieces that end inside the representative: diagonal in [0, repLen - memberLen]
    assert len(lines(ext, key_of('negative_diagonal'))) == 2
    hub = recorded['H_r0'][5]
    assert max(t.count(b'\n') for t in hub.values()) == 5000
    par, res, off, keys, lmap, db, seqs, cl = recorded['W_r0']
    assert len(seqs[0]) == 32767 and db[0].count(b'\n') >= 6


def time_driver(npz, threads):
    z = np.load(npz)
    ref_root = '/root/reference'
    matrix = os.path.join(ref_root, 'lib', 'mmseqs', 'data', 'blosum62.out')
    par = kmm_ref.params(k=0, residues=int(z['off'][-1]))
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        ts = []
        for _ in range(3):
            got = run_driver(exe, tmp, matrix, par, z['res'], z['off'], np.arange(len(z['off']) - 1, dtype=np.uint32), threads=threads, want_records=False)
            ts.append((got['t_compute'], got['t_write']))
        print('reference driver, %d threads, k %d: doComputation %s s, write %s s (3 runs)' % (threads, par['k'], [round(t[0], 3) for t in ts],
                                                                                            [round(t[1], 3) for t in ts]))


if __name__ == '__main__':
    main()
