#!/usr/bin/env python3
"""Writes tests/golden/target_profile_vectors.npz from the LIVE reference: the k-mer index of a *profile* target DB
(IndexBuilder::fillDatabase's profile branch, M/src/prefiltering/IndexBuilder.cpp:61-62,94-128,200-219, with the reference's own
IndexTable::addSimilarKmerCount / addSimilarSequence / sortDBSeqLists, IndexTable.h:97-130,302-345) and the rows
QueryMatcher::matchQuery gives for amino-acid queries against it with takeOnlyBestKmer (Prefiltering.cpp:176-179,
QueryMatcher.cpp:225-257).  Results and inputs only.

fillDatabase itself cannot be linked (DBReader -> Parameters.cpp -> generated headers), so DRIVER below (ours) restates its profile
branch over the reference's classes; it is compiled into a temporary directory against the reference's headers and linked to
oracle/_ref/libsdref.so, and nothing compiled is kept.

    python tools/make_golden_target_profile.py [reference root]          (needs `make -C oracle _ref/libsdref.so`; no GPU)
    python tools/make_golden_target_profile.py --time-build REPS THR     (wall time of the driver's build of set G x REPS; writes nothing)

Sets (tests/test_target_profile_golden.py checks the conditions, tests/test_gpu_target_profile.py the device against them):
  S  three short profiles cut from profile_vectors.npz: every (k-mer, target, position) triple and the consensus lookup
  R  one profile that repeats a 16-position segment: equal k-mers at two positions of one target, full triples
  B  one profile of 12 positions at a threshold where a window's list passes 65 536 k-mers: counts, list lengths, digest
  G  the 18 profiles of profile_vectors.npz at thresholds 110 and 95: counts and digest; prefilter rows of 152 sequence queries
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLD, 'target_profile_vectors.npz')
AA = 'ACDEFGHIKLMNPQRSTVWY'

DRIVER = r'''
#include "SubstitutionMatrix.h"
#include "Sequence.h"
#include "IndexTable.h"
#include "SequenceLookup.h"
#include "KmerGenerator.h"
#include "QueryMatcher.h"
#include "Indexer.h"
#include "Util.h"
#include "Debug.h"
#include "Parameters.h"
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
// argv: blosum62 path, VTML80 path, job file, result file.
// job:    i32 kmerThr, compBias, wantRows, pad; u64 nProf; u64 byteOff[nProf + 1]; profile bytes; u64 nSeq; u64 off[nSeq + 1]; letters
// result: u64 nEntries, nRecords, nWindows, nLists, nRows; f64 buildSeconds; u32 windowLen[nWindows] (every window, (target, position)
//         order, 0 where the query letters hold an X); u8 lookup[positions]; (u32 kmer, u64 start)[nLists] of the non-empty lists;
//         u32 entrySeq[nEntries]; u16 entryPos[nEntries]; (i32 query, target, score, diagonal16)[nRows]; u32 kmerListLen[nSeq]
template <typename T> static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) exit(2);
    return v;
}
template <typename T> static void wr(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(3);
}
int main(int argc, char **argv) {
    if (argc != 5) return 1;
    Debug::setDebugLevel(1);
    FILE *in = fopen(argv[3], "rb");
    if (!in) return 1;
    std::vector<int> head = rd<int>(in, 4);
    const int kmerThr = head[0], compBias = head[1], wantRows = head[2], kmerSize = 6;
    const size_t nProf = rd<uint64_t>(in, 1)[0];
    std::vector<uint64_t> pOff = rd<uint64_t>(in, nProf + 1);
    std::vector<char> pData = rd<char>(in, pOff[nProf]);
    const size_t nSeq = rd<uint64_t>(in, 1)[0];
    std::vector<uint64_t> sOff = rd<uint64_t>(in, nSeq + 1);
    std::vector<char> sData = rd<char>(in, sOff[nSeq]);
    fclose(in);
    SubstitutionMatrix ungapped2(argv[1], 2.0f, -0.2f);   // Prefiltering.cpp:69,991
    SubstitutionMatrix seed8(argv[2], 8.0f, -0.2f);       // Prefiltering.cpp:68,991
    const int alphabetSize = seed8.alphabetSize - 1;      // Prefiltering.cpp:530-533
    size_t maxLen = 0, positions = 0;
    std::vector<size_t> posOff(nProf + 1, 0);
    for (size_t i = 0; i < nProf; i++) {
        const size_t L = (pOff[i + 1] - pOff[i]) / Sequence::PROFILE_READIN_SIZE;
        maxLen = std::max(maxLen, L);
        posOff[i + 1] = posOff[i] + L;
    }
    positions = posOff[nProf];
    for (size_t i = 0; i < nSeq; i++) maxLen = std::max<size_t>(maxLen, sOff[i + 1] - sOff[i]);
    maxLen += 2;
    const auto t0 = std::chrono::steady_clock::now();
    // ---- the profile branch of fillDatabase (isTargetSimiliarKmerSearch, no masking: Prefiltering.cpp:172-174)
    IndexTable table(alphabetSize, kmerSize, false);
    SequenceLookup lookup(nProf, positions);
    Sequence s(maxLen, Parameters::DBTYPE_HMM_PROFILE, &seed8, kmerSize, true, false, true, "");
    std::vector<unsigned int> windowLen;
    size_t nRecords = 0, tableSize = 0;
    {
        KmerGenerator generator(kmerSize, alphabetSize, (short) kmerThr);
        generator.setDivideStrategy(s.profile_matrix);
        for (size_t id = 0; id < nProf; id++) {
            s.resetCurrPos();
            s.mapSequence(id, (unsigned int) id, pData.data() + pOff[id], (unsigned int) (posOff[id + 1] - posOff[id]));
            table.addSimilarKmerCount(&s, &generator);
            lookup.addSequence(s.numConsensusSequence, s.L, id, posOff[id]);
            if (Util::overlappingKmers(s.L, s.getEffectiveKmerSize()) > 0) tableSize += 1;
            // the lengths of the lists addSimilarKmerCount has just walked (a second walk of our own: it keeps no record of them)
            s.resetCurrPos();
            while (s.hasNextKmer()) {
                const unsigned char *kmer = s.nextKmer();
                if (s.kmerContainsX()) {
                    windowLen.push_back(0);
                    continue;
                }
                const size_t n = generator.generateKmerList(kmer).second;
                windowLen.push_back((unsigned int) n);
                nRecords += n;
            }
        }
    }
    table.initMemory(tableSize);
    table.init();
    {
        Indexer idxer(alphabetSize, kmerSize);
        // addSimilarSequence doubles its buffer once per window and writes past it when one list is longer than the buffer
        size_t bufferSize = std::max<size_t>((size_t) 1 << 24, 2 * nRecords / std::max<size_t>(nProf, 1));
        IndexEntryLocalTmp *buffer = (IndexEntryLocalTmp *) malloc(bufferSize * sizeof(IndexEntryLocalTmp));
        KmerGenerator generator(kmerSize, alphabetSize, (short) kmerThr);
        generator.setDivideStrategy(s.profile_matrix);
        for (size_t id = 0; id < nProf; id++) {
            s.resetCurrPos();
            s.mapSequence(id, (unsigned int) id, pData.data() + pOff[id], (unsigned int) (posOff[id + 1] - posOff[id]));
            table.addSimilarSequence(&s, &generator, &buffer, bufferSize, &idxer);
        }
        free(buffer);
    }
    table.revertPointer();
    table.sortDBSeqLists();
    const double buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const size_t ts = table.getTableSize();
    const size_t *offsets = table.getOffsets();
    const size_t nEntries = offsets[ts];
    std::vector<unsigned int> listKmer, entrySeq(nEntries);
    std::vector<uint64_t> listStart;
    std::vector<unsigned short> entryPos(nEntries);
    for (size_t k = 0; k < ts; k++)
        if (offsets[k + 1] > offsets[k]) {
            listKmer.push_back((unsigned int) k);
            listStart.push_back(offsets[k]);
        }
    const IndexEntryLocal *e = table.getEntries();
    for (size_t i = 0; i < nEntries; i++) {
        entrySeq[i] = e[i].seqId;
        entryPos[i] = e[i].position_j;
    }
    // ---- amino-acid queries, takeOnlyBestKmer (Prefiltering.cpp:176-179,797-799)
    std::vector<int> rows;
    std::vector<unsigned int> kmerListLen(nSeq, 0);
    if (wantRows) {
        QueryMatcher matcher(&table, &lookup, &seed8, &ungapped2, (short) kmerThr, kmerSize, nProf, (unsigned int) maxLen, 300, compBias != 0,
                             1.0f, true, 15, true, false);
        matcher.setSubstitutionMatrix(NULL, NULL);
        Sequence q(maxLen, Parameters::DBTYPE_AMINO_ACIDS, &seed8, kmerSize, true, compBias != 0);
        for (size_t i = 0; i < nSeq; i++) {
            q.mapSequence(i, (unsigned int) i, sData.data() + sOff[i], (unsigned int) (sOff[i + 1] - sOff[i]));
            std::pair<hit_t *, size_t> r = matcher.matchQuery(&q, UINT_MAX, false);
            for (size_t x = 0; x < r.second; x++) {
                rows.push_back((int) i);
                rows.push_back((int) r.first[x].seqId);
                rows.push_back(r.first[x].prefScore);
                rows.push_back((int) r.first[x].diagonal);
            }
            kmerListLen[i] = (unsigned int) (matcher.getStatistics()->kmersPerPos * (double) q.L + 0.5);
        }
    }
    FILE *out = fopen(argv[4], "wb");
    if (!out) return 1;
    const uint64_t h[5] = {nEntries, nRecords, windowLen.size(), listKmer.size(), rows.size() / 4};
    fwrite(h, sizeof(uint64_t), 5, out);
    fwrite(&buildSeconds, sizeof(double), 1, out);
    wr(out, windowLen);
    fwrite(lookup.getData(), 1, positions, out);
    wr(out, listKmer);
    wr(out, listStart);
    wr(out, entrySeq);
    wr(out, entryPos);
    wr(out, rows);
    wr(out, kmerListLen);
    fclose(out);
    return 0;
}
'''


def build_driver(ref_root, tmp):
    """compiles DRIVER against the reference's headers into tmp, linked to oracle/_ref/libsdref.so; returns the program's path"""
    m = os.path.join(ref_root, 'lib', 'mmseqs')
    src, exe = os.path.join(tmp, 'driver.cpp'), os.path.join(tmp, 'driver')
    open(src, 'w').write(DRIVER)
    inc = [os.path.join(m, *p) for p in (('src', 'commons'), ('src', 'alignment'), ('src', 'prefiltering'), ('lib',), ('lib', 'simd'),
                                          ('lib', 'alp'), ('lib', 'tantan'), ('lib', 'fmt'), ('lib', 'simde'), ('lib', 'zstd', 'lib'))]
    refdir = os.path.join(ROOT, 'oracle', '_ref')
    # (the library leaves ProfileStates unresolved: referenced, never reached on this path)
    subprocess.check_call(['g++', '-std=c++14', '-O3', '-mavx2', '-mfma', '-mcx16', '-DAVX2=1', '-DOPENMP=1', '-fopenmp', '-w'] +
                          ['-I' + d for d in inc] + [src, '-L' + refdir, '-lsdref', '-Wl,-rpath,' + refdir, '-Wl,--allow-shlib-undefined',
                                                     '-o', exe])
    return exe


def run_driver(exe, tmp, profiles, seqs, thr, comp_bias=True, want_rows=False):
    """profiles: list of bytes (25 per position); seqs: list of ASCII strings.  Returns the driver's result as a dict."""
    from oracle.pyoracle import matrix_spec
    poff = np.zeros(len(profiles) + 1, np.uint64)
    poff[1:] = np.cumsum([len(p) for p in profiles])
    soff = np.zeros(len(seqs) + 1, np.uint64)
    soff[1:] = np.cumsum([len(s) for s in seqs])
    job, res = os.path.join(tmp, 'job.bin'), os.path.join(tmp, 'res.bin')
    with open(job, 'wb') as f:
        f.write(struct.pack('<4i', thr, 1 if comp_bias else 0, 1 if want_rows else 0, 0))
        f.write(struct.pack('<Q', len(profiles)) + poff.tobytes() + b''.join(profiles))
        f.write(struct.pack('<Q', len(seqs)) + soff.tobytes() + ''.join(seqs).encode())
    t0 = time.time()
    subprocess.check_call([exe, matrix_spec(0), matrix_spec(1), job, res])
    wall = time.time() - t0
    raw = open(res, 'rb').read()
    n_entries, n_records, n_windows, n_lists, n_rows = struct.unpack_from('<5Q', raw, 0)
    build_seconds, = struct.unpack_from('<d', raw, 40)
    at = [48]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, at[0]).copy()
        at[0] += a.nbytes
        return a
    positions = int(poff[-1]) // 25
    out = dict(n_entries=n_entries, n_records=n_records, build_seconds=build_seconds, wall=wall)
    out['window_len'] = take(np.uint32, n_windows)
    out['lookup'] = take(np.uint8, positions)
    out['list_kmer'] = take(np.uint32, n_lists)
    out['list_start'] = take(np.uint64, n_lists)
    out['entry_seq'] = take(np.uint32, n_entries)
    out['entry_pos'] = take(np.uint16, n_entries)
    out['rows'] = take(np.int32, n_rows * 4).reshape(n_rows, 4)
    out['kmer_list_len'] = take(np.uint32, len(seqs))
    assert at[0] == len(raw)
    return out


def digest(list_kmer, list_start, entry_seq, entry_pos):
    """SHA-256 over the non-empty lists' k-mers (u32) || their starts (u64) || entry_seq (u32) || entry_pos (u16), index order, little endian"""
    h = hashlib.sha256()
    for a, t in ((list_kmer, '<u4'), (list_start, '<u8'), (entry_seq, '<u4'), (entry_pos, '<u2')):
        h.update(np.ascontiguousarray(a, t).tobytes())
    return h.hexdigest()


def triples(r):
    """(k-mer, target, position) of every entry, index order"""
    lens = np.diff(np.append(r['list_start'], np.uint64(r['n_entries']))).astype(np.int64)
    return np.stack([np.repeat(r['list_kmer'], lens).astype(np.int64), r['entry_seq'].astype(np.int64), r['entry_pos'].astype(np.int64)], axis=1)


def cut(profile_bytes, a, b):
    return bytes(profile_bytes[25 * a:25 * b])


def no_x(rec_bytes):
    """the query letters of a profile record without X (the consensus letter takes an X's place)"""
    rec = np.frombuffer(rec_bytes, np.uint8).reshape(-1, 25).copy()
    x = rec[:, 20] >= 20
    rec[x, 20] = rec[x, 21]
    return rec.tobytes()


def with_x(seq, rng, n):
    s = list(seq)
    for p in rng.choice(np.arange(5, len(s) - 5), n, replace=False):
        s[int(p)] = 'X'
    return ''.join(s)


def load_inputs():
    d = np.load(os.path.join(GOLD, 'profile_vectors.npz'))
    poff = d['poff'].astype(np.int64)
    pdata = d['profiles'].tobytes()
    profiles = [pdata[poff[i]:poff[i + 1]] for i in range(len(poff) - 1)]
    off = d['off'].astype(np.int64)
    blob = d['blob'].tobytes().decode()
    seqs = [blob[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return profiles, seqs


def main():
    args = sys.argv[1:]
    profiles, seqs = load_inputs()
    if args and args[0] == '--time-build':
        reps, thr = int(args[1]), int(args[2])
        with tempfile.TemporaryDirectory() as tmp:
            exe = build_driver('/root/reference' if len(args) < 4 else args[3], tmp)
            r = run_driver(exe, tmp, profiles * reps, [], thr)
        print('reference driver (one thread): %d profiles, %d positions, threshold %d: %d records, %d entries, build %.2f s'
              % (len(profiles) * reps, len(r['lookup']), thr, r['n_records'], r['n_entries'], r['build_seconds']))
        return
    ref_root = args[0] if args else '/root/reference'
    rng = np.random.default_rng(20261020)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)

        def full(name, profs, thr):
            r = run_driver(exe, tmp, profs, [], thr)
            t = triples(r)
            poff = np.zeros(len(profs) + 1, np.uint64)
            poff[1:] = np.cumsum([len(p) for p in profs])
            out[name + '_profiles'] = np.frombuffer(b''.join(profs), np.uint8)
            out[name + '_poff'] = poff
            out[name + '_thr'] = np.int32(thr)
            out[name + '_triples'] = t.astype(np.uint32)
            out[name + '_lookup'] = r['lookup']
            out[name + '_records'] = np.int64(r['n_records'])
            out[name + '_window_len'] = r['window_len']
            print('set %s: threshold %d, %d records, %d entries, longest window list %d' % (name, thr, r['n_records'], r['n_entries'], r['window_len'].max()))
            return r, t

        # ---- S: three short profiles (12, 25 and 40 positions), X windows included
        s_profs = [cut(profiles[0], 0, 12), cut(profiles[1], 5, 30), cut(profiles[2], 10, 50)]
        r, t = full('S', s_profs, 112)
        assert 1000 < r['n_entries'] < 40000

        # ---- R: a 16-position segment twice (windows p and p + 16 give the same list for p < 7), no X in the query letters
        seg = no_x(cut(profiles[3], 20, 36))
        r, t = full('R', [seg + seg], 108)
        assert r['n_records'] > r['n_entries'], 'no k-mer of the raw lists occurs at two positions'
        assert (r['window_len'][:7] == r['window_len'][16:23]).all() and r['window_len'][0] > 0
        assert int(r['n_records'] - r['n_entries']) >= int(r['window_len'][:7].min())

        # ---- B: 12 positions, a threshold where a window's list passes 65 536 k-mers (the second scratch tier of the device kernel)
        b_prof = no_x(cut(profiles[4], 30, 42))
        thr_b = None
        for thr in range(80, -40, -5):
            r = run_driver(exe, tmp, [b_prof], [], thr)
            if r['window_len'].max() > 65536:
                thr_b = thr
                break
        assert thr_b is not None and r['window_len'].max() < (1 << 23)
        out['B_profiles'] = np.frombuffer(b_prof, np.uint8)
        out['B_thr'] = np.int32(thr_b)
        out['B_entries'] = np.int64(r['n_entries'])
        out['B_records'] = np.int64(r['n_records'])
        out['B_window_len'] = r['window_len']
        out['B_digest'] = np.array(digest(r['list_kmer'], r['list_start'], r['entry_seq'], r['entry_pos']))
        print('set B: threshold %d, window lists %s, %d entries' % (thr_b, r['window_len'].tolist(), r['n_entries']))

        # ---- G: the 18 profiles; queries: the 144 sequences + eight of them with 1 - 3 letters replaced by X
        x_of = np.array([1, 6, 13, 22, 30, 41, 50, 66], np.int32)
        queries = list(seqs) + [with_x(seqs[int(q)], rng, 1 + i % 3) for i, q in enumerate(x_of)]
        out['Q_letters'] = np.frombuffer(''.join(queries).encode(), np.uint8)
        qoff = np.zeros(len(queries) + 1, np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        out['Q_off'] = qoff
        out['Q_x_of'] = x_of
        for thr, bias in ((110, True), (95, True), (110, False)):
            r = run_driver(exe, tmp, profiles, queries, thr, comp_bias=bias, want_rows=True)
            tag = 'G%d' % thr
            if bias:
                out[tag + '_entries'] = np.int64(r['n_entries'])
                out[tag + '_records'] = np.int64(r['n_records'])
                out[tag + '_per_target'] = np.bincount(r['entry_seq'], minlength=len(profiles)).astype(np.int64)
                out[tag + '_lists'] = np.int64(len(r['list_kmer']))
                out[tag + '_longest_list'] = np.int64(np.diff(np.append(r['list_start'], np.uint64(r['n_entries']))).max())
                out[tag + '_digest'] = np.array(digest(r['list_kmer'], r['list_start'], r['entry_seq'], r['entry_pos']))
                out[tag + '_ref_build_seconds'] = np.float64(r['build_seconds'])
            rows = r['rows']
            name = 'rows_%d_bias%d' % (thr, 1 if bias else 0)
            out[name] = rows
            out[name + '_kmers'] = r['kmer_list_len']
            plain = rows[rows[:, 0] < len(seqs)]
            n_q = len(np.unique(plain[:, 0]))
            # family of a query: sequence 4 b + j descends from base b, profile b is built from base b
            other = int((plain[:, 1] != plain[:, 0] // 4).sum())
            print('G threshold %d bias %d: %d records, %d entries, longest list %d; %d rows (%d of the 144 plain queries, %d queries with a row, '
                  '%d rows outside the query\'s family), build %.2f s'
                  % (thr, bias, r['n_records'], r['n_entries'], np.diff(np.append(r['list_start'], np.uint64(r['n_entries']))).max(),
                     len(rows), len(plain), n_q, other, r['build_seconds']))
            assert len(plain) >= (60 if thr == 110 else 140), 'too few rows to pin'
            assert other >= 1, 'no row on a target outside the query\'s own family'
            # a window with an X contributes nothing: the X copies look up fewer k-mers than their originals
            for i, q in enumerate(x_of):
                assert r['kmer_list_len'][len(seqs) + i] < r['kmer_list_len'][int(q)]
            out[name + '_figures'] = np.array([len(rows), len(plain), n_q, other], np.int64)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print('wrote %s (%d bytes)' % (OUT, size))
    assert size < (1 << 20)


if __name__ == '__main__':
    main()
