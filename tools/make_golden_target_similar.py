#!/usr/bin/env python3
"""Writes tests/golden/target_similar_vectors.npz from the LIVE reference: the k-mer index of a *sequence* target DB under
--target-search-mode 1 (the sequence-similar branch of IndexBuilder::fillDatabase, M/src/prefiltering/IndexBuilder.cpp:61-62,94-128,
200-219: setDivideStrategy(&three, &two), no masking, the unmasked numSequence as the lookup) with the reference's own
IndexTable::addSimilarKmerCount / addSimilarSequence / sortDBSeqLists (IndexTable.h:97-130,302-345), and the rows
QueryMatcher::matchQuery gives for amino-acid queries against it with takeOnlyBestKmer (Prefiltering.cpp:176-179,
QueryMatcher.cpp:225-257).  Results and inputs only.

fillDatabase itself cannot be linked (DBReader -> Parameters.cpp -> generated headers), so DRIVER below (ours) restates that branch
over the reference's classes; it is compiled into a temporary directory against the reference's headers and linked to
oracle/_ref/libsdref.so, and nothing compiled is kept.  The driver runs the Masker's constructor and never its maskSequence, as the
branch does; that masking changes nothing is asserted here against the reference's own masker (set M below).

    python tools/make_golden_target_similar.py [reference root]          (needs `make -C oracle _ref/libsdref.so`; no GPU)

Sets (tests/test_target_similar_golden.py checks the conditions, tests/test_gpu_target_similar.py the device against them):
  S  four short sequences (one shorter than the spaced window, one with X): every (k-mer, target, position) triple, the lookup
  R  one 16-residue segment twice inside one target and once in a second target: full triples
  B  one 14-residue sequence at a low threshold where a window's list passes 65 536 k-mers and none reaches 2^23: counts, digest
  G  36 family proteins of profile_vectors.npz (members 0 and 1 of every family) at threshold 112; queries: members 2 and 3 and six
     of them with letters replaced by X: counts and digest; rows with and without composition bias; the reference's mode-0 rows
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLD, 'target_similar_vectors.npz')

DRIVER = r'''
#include "SubstitutionMatrix.h"
#include "ExtendedSubstitutionMatrix.h"
#include "Sequence.h"
#include "IndexTable.h"
#include "SequenceLookup.h"
#include "KmerGenerator.h"
#include "QueryMatcher.h"
#include "Indexer.h"
#include "Masker.h"
#include "Util.h"
#include "Debug.h"
#include "Parameters.h"
#include <cstdio>
#include <cstring>
#include <vector>
// argv: blosum62 path, VTML80 path, job file, result file.
// job:    i32 kmerThr, compBias, wantRows, pad; u64 nT; u64 tOff[nT + 1]; target letters; u64 nQ; u64 qOff[nQ + 1]; query letters
// result: u64 nEntries, nRecords, nWindows, nLists, nRows; u32 windowLen[nWindows] (every window, (target, position) order, 0 where
//         the letters hold an X); u8 lookup[residues]; (u32 kmer, u64 start)[nLists] of the non-empty lists; u32 entrySeq[nEntries];
//         u16 entryPos[nEntries]; (i32 query, target, score, diagonal16)[nRows]; u32 kmerListLen[nQ]
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
    const size_t nT = rd<uint64_t>(in, 1)[0];
    std::vector<uint64_t> tOff = rd<uint64_t>(in, nT + 1);
    std::vector<char> tData = rd<char>(in, tOff[nT]);
    const size_t nQ = rd<uint64_t>(in, 1)[0];
    std::vector<uint64_t> qOff = rd<uint64_t>(in, nQ + 1);
    std::vector<char> qData = rd<char>(in, qOff[nQ]);
    fclose(in);
    SubstitutionMatrix ungapped2(argv[1], 2.0f, -0.2f);   // Prefiltering.cpp:69,991
    SubstitutionMatrix seed8(argv[2], 8.0f, -0.2f);       // Prefiltering.cpp:68,991
    const int alphabetSize = seed8.alphabetSize - 1;      // Prefiltering.cpp:530-533
    seed8.alphabetSize = alphabetSize;                    // the extended matrices leave X out (Prefiltering.cpp:209-214)
    ScoreMatrix two = ExtendedSubstitutionMatrix::calcScoreMatrix(seed8, 2);
    ScoreMatrix three = ExtendedSubstitutionMatrix::calcScoreMatrix(seed8, 3);
    seed8.alphabetSize = alphabetSize + 1;
    size_t maxLen = 0;
    for (size_t i = 0; i < nT; i++) maxLen = std::max<size_t>(maxLen, tOff[i + 1] - tOff[i]);
    for (size_t i = 0; i < nQ; i++) maxLen = std::max<size_t>(maxLen, qOff[i + 1] - qOff[i]);
    maxLen += 2;
    const size_t residues = tOff[nT];
    // ---- the sequence branch of isTargetSimiliarKmerSearch: the Masker is constructed (needMasking) and maskSequence never called
    IndexTable table(alphabetSize, kmerSize, false);
    SequenceLookup lookup(nT, residues);
    Sequence s(maxLen, Parameters::DBTYPE_AMINO_ACIDS, &seed8, kmerSize, true, false, true, "");
    Masker masker(seed8);
    std::vector<unsigned int> windowLen;
    size_t nRecords = 0, tableSize = 0;
    {
        KmerGenerator generator(kmerSize, alphabetSize, (short) kmerThr);
        generator.setDivideStrategy(&three, &two);
        for (size_t id = 0; id < nT; id++) {
            s.resetCurrPos();
            s.mapSequence(id, (unsigned int) id, tData.data() + tOff[id], (unsigned int) (tOff[id + 1] - tOff[id]));
            table.addSimilarKmerCount(&s, &generator);
            lookup.addSequence(s.numSequence, s.L, id, tOff[id]);
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
        size_t bufferSize = std::max<size_t>((size_t) 1 << 24, 2 * nRecords / std::max<size_t>(nT, 1));
        IndexEntryLocalTmp *buffer = (IndexEntryLocalTmp *) malloc(bufferSize * sizeof(IndexEntryLocalTmp));
        KmerGenerator generator(kmerSize, alphabetSize, (short) kmerThr);
        generator.setDivideStrategy(&three, &two);
        for (size_t id = 0; id < nT; id++) {
            s.resetCurrPos();
            s.mapSequence(id, (unsigned int) id, tData.data() + tOff[id], (unsigned int) (tOff[id + 1] - tOff[id]));
            table.addSimilarSequence(&s, &generator, &buffer, bufferSize, &idxer);
        }
        free(buffer);
    }
    table.revertPointer();
    table.sortDBSeqLists();
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
    std::vector<unsigned int> kmerListLen(nQ, 0);
    if (wantRows) {
        QueryMatcher matcher(&table, &lookup, &seed8, &ungapped2, (short) kmerThr, kmerSize, nT, (unsigned int) maxLen, 300, compBias != 0,
                             1.0f, true, 15, true, false);
        matcher.setSubstitutionMatrix(&three, &two);
        Sequence q(maxLen, Parameters::DBTYPE_AMINO_ACIDS, &seed8, kmerSize, true, compBias != 0);
        for (size_t i = 0; i < nQ; i++) {
            q.mapSequence(i, (unsigned int) i, qData.data() + qOff[i], (unsigned int) (qOff[i + 1] - qOff[i]));
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
    wr(out, windowLen);
    fwrite(lookup.getData(), 1, residues, out);
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


def run_driver(exe, tmp, targets, queries, thr, comp_bias=True, want_rows=False):
    """targets, queries: lists of ASCII strings.  Returns the driver's result as a dict."""
    from oracle.pyoracle import matrix_spec
    toff = np.zeros(len(targets) + 1, np.uint64)
    toff[1:] = np.cumsum([len(t) for t in targets])
    qoff = np.zeros(len(queries) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(q) for q in queries])
    job, res = os.path.join(tmp, 'job.bin'), os.path.join(tmp, 'res.bin')
    with open(job, 'wb') as f:
        f.write(struct.pack('<4i', thr, 1 if comp_bias else 0, 1 if want_rows else 0, 0))
        f.write(struct.pack('<Q', len(targets)) + toff.tobytes() + ''.join(targets).encode())
        f.write(struct.pack('<Q', len(queries)) + qoff.tobytes() + ''.join(queries).encode())
    subprocess.check_call([exe, matrix_spec(0), matrix_spec(1), job, res])
    raw = open(res, 'rb').read()
    n_entries, n_records, n_windows, n_lists, n_rows = struct.unpack_from('<5Q', raw, 0)
    at = [40]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, at[0]).copy()
        at[0] += a.nbytes
        return a
    out = dict(n_entries=n_entries, n_records=n_records)
    out['window_len'] = take(np.uint32, n_windows)
    out['lookup'] = take(np.uint8, int(toff[-1]))
    out['list_kmer'] = take(np.uint32, n_lists)
    out['list_start'] = take(np.uint64, n_lists)
    out['entry_seq'] = take(np.uint32, n_entries)
    out['entry_pos'] = take(np.uint16, n_entries)
    out['rows'] = take(np.int32, n_rows * 4).reshape(n_rows, 4)
    out['kmer_list_len'] = take(np.uint32, len(queries))
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


def with_x(seq, rng, n):
    s = list(seq)
    for p in rng.choice(np.arange(5, len(s) - 5), n, replace=False):
        s[int(p)] = 'X'
    return ''.join(s)


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(''.join(seqs).encode(), np.uint8), off


def load_family_sequences():
    """the 144 sequences of profile_vectors.npz: sequence 4 b + j is member j of family b"""
    d = np.load(os.path.join(GOLD, 'profile_vectors.npz'))
    off = d['off'].astype(np.int64)
    blob = d['blob'].tobytes().decode()
    return [blob[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def main():
    args = sys.argv[1:]
    ref_root = args[0] if args else '/root/reference'
    from oracle.pyoracle import Ref
    from spacedust_amd import api
    host = api.Host(1)
    assert host.kmer_threshold(5.7, 6) == 112, 'k = 6 at -s 5.7 is no longer 112'
    seqs = load_family_sequences()
    rng = np.random.default_rng(20261020)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)

        def full(name, targets, thr):
            r = run_driver(exe, tmp, targets, [], thr)
            t = triples(r)
            out[name + '_letters'], out[name + '_off'] = pack(targets)
            out[name + '_thr'] = np.int32(thr)
            out[name + '_triples'] = t.astype(np.uint32)
            out[name + '_lookup'] = r['lookup']
            out[name + '_records'] = np.int64(r['n_records'])
            out[name + '_window_len'] = r['window_len']
            print('set %s: threshold %d, %d windows, %d records, %d entries, longest window list %d'
                  % (name, thr, len(r['window_len']), r['n_records'], r['n_entries'], r['window_len'].max()))
            return r, t

        # ---- S: 7 residues (shorter than the window: no window), 12, 25 with two X, 40; threshold 120: some lists are empty
        a, b, c = seqs[0], seqs[5], seqs[9]
        s3 = list(b[10:35])
        s3[4] = s3[17] = 'X'
        s_set = [a[3:10], a[20:32], ''.join(s3), c[50:90]]
        x_win = np.array([any(s3[i + o] == 'X' for o in (0, 1, 3, 5, 8, 9)) for i in range(16)])
        # the lowest threshold (steps of 4 from the default) at which a window without X has an empty list (addIdentity is false)
        for thr_s in range(112, 200, 4):
            wl = run_driver(exe, tmp, s_set, [], thr_s)['window_len']
            empty_plain = int((wl[3:19][~x_win] == 0).sum() + (wl[:3] == 0).sum() + (wl[19:] == 0).sum())
            if empty_plain >= 1:
                break
        assert empty_plain >= 1, 'no window without X has an empty list'
        r, t = full('S', s_set, thr_s)
        wl = r['window_len']
        assert len(wl) == 0 + 3 + 16 + 31 and 200 < r['n_entries'] < 60000
        assert x_win.any() and (wl[3:19][x_win] == 0).all()
        out['S_empty_plain_windows'] = np.int64(empty_plain)

        # ---- R: target 0 = head + segment + middle + segment + tail, target 1 = segment alone.  The windows inside the two copies give the
        # same lists, so target 0 meets those k-mers at two positions and keeps the smaller
        seg = seqs[12][40:56]
        t0 = seqs[16][5:12] + seg + seqs[16][30:35] + seg + seqs[16][60:66]
        r, t = full('R', [t0, seg], 112)
        wl = r['window_len']
        p1, p2 = 7, 7 + 16 + 5
        assert len(t0) == 50 and (wl[p1:p1 + 7] == wl[p2:p2 + 7]).all() and int(wl[p1:p1 + 7].sum()) > 0
        assert (wl[41:48] == wl[p1:p1 + 7]).all()
        removed = int(r['n_records'] - r['n_entries'])
        assert removed >= int(wl[p2:p2 + 7].sum()), 'the dedupe removes fewer records than the second copy holds'
        out['R_removed'] = np.int64(removed)
        out['R_copies'] = np.array([p1, p2], np.int32)
        print('set R: the dedupe removes %d records (second copy: %d)' % (removed, int(wl[p2:p2 + 7].sum())))

        # ---- B: 14 residues at a low threshold: a window list beyond 65 536 k-mers, none at 2^23
        b_seq = seqs[20][30:44]
        thr_b = None
        for thr in range(100, 20, -4):
            r = run_driver(exe, tmp, [b_seq], [], thr)
            if r['window_len'].max() > 65536:
                thr_b = thr
                break
        assert thr_b is not None and r['window_len'].max() < (1 << 23) - 1
        out['B_letters'], out['B_off'] = pack([b_seq])
        out['B_thr'] = np.int32(thr_b)
        out['B_entries'] = np.int64(r['n_entries'])
        out['B_records'] = np.int64(r['n_records'])
        out['B_window_len'] = r['window_len']
        out['B_digest'] = np.array(digest(r['list_kmer'], r['list_start'], r['entry_seq'], r['entry_pos']))
        print('set B: threshold %d, window lists %s, %d entries' % (thr_b, r['window_len'].tolist(), r['n_entries']))

        # ---- G: members 0 and 1 of the 18 families as targets; members 2 and 3 as queries, six of them again with 1 - 3 X
        targets = [seqs[4 * f + j] for f in range(18) for j in (0, 1)]
        plain = [seqs[4 * f + j] for f in range(18) for j in (2, 3)]
        x_of = np.array([1, 6, 13, 22, 27, 34], np.int32)
        queries = plain + [with_x(plain[int(q)], rng, 1 + i % 3) for i, q in enumerate(x_of)]
        out['G_letters'], out['G_off'] = pack(targets)
        out['Q_letters'], out['Q_off'] = pack(queries)
        out['Q_x_of'] = x_of
        thr = 112
        out['G_thr'] = np.int32(thr)
        for bias in (True, False):
            r = run_driver(exe, tmp, targets, queries, thr, comp_bias=bias, want_rows=True)
            if bias:
                out['G_entries'] = np.int64(r['n_entries'])
                out['G_records'] = np.int64(r['n_records'])
                out['G_per_target'] = np.bincount(r['entry_seq'], minlength=len(targets)).astype(np.int64)
                out['G_lists'] = np.int64(len(r['list_kmer']))
                out['G_digest'] = np.array(digest(r['list_kmer'], r['list_start'], r['entry_seq'], r['entry_pos']))
                assert (r['lookup'] == host.map_sequences(targets)[0]).all()
            rows = r['rows']
            name = 'rows_bias%d' % (1 if bias else 0)
            out[name] = rows
            out[name + '_kmers'] = r['kmer_list_len']
            pl = rows[rows[:, 0] < len(plain)]
            other = int((pl[:, 1] // 2 != pl[:, 0] // 2).sum())
            print('G bias %d: %d records, %d entries (%.0f records per residue); %d rows, %d outside the query\'s family'
                  % (bias, r['n_records'], r['n_entries'], r['n_records'] / float(len(r['lookup'])), len(rows), other))
            assert len(pl) >= 36 and other >= 1
            for i, q in enumerate(x_of):
                assert r['kmer_list_len'][len(plain) + i] < r['kmer_list_len'][int(q)]
        assert not np.array_equal(out['rows_bias1'], out['rows_bias0'])

        # ---- the mode-0 rows of the same input: the reference's regular index (masked, self-score threshold) and similar-k-mer queries
        ref = Ref(6)
        blob = ''.join(targets).encode()
        idx = ref.index(blob, out['G_off'], kmer_thr=thr, mask=True, mask_prob=0.9, threads=1)
        pf = idx.prefilter(max(len(q) for q in queries) + 2, max_hits=300, min_diag=15, comp_bias=True)
        m0 = []
        for i, q in enumerate(queries):
            ids, sc, dg, _ = pf.query(q)
            m0 += [(i, int(t), int(s), int(np.int16(d))) for t, s, d in zip(ids, sc, dg)]
        m0 = np.array(m0, np.int32).reshape(-1, 4)
        out['rows_mode0'] = m0
        m1 = out['rows_bias1'].copy()
        m1[:, 3] = m1[:, 3].astype(np.int16)
        assert not np.array_equal(m0, m1), 'mode 1 and mode 0 give the same rows: the set cannot tell them apart'
        print('mode 0: %d rows; mode 1: %d rows' % (len(m0), len(m1)))

        # ---- M: masking plays no part.  The reference's masker does change these targets (so --mask 1 would matter if it ran) ...
        masked = sum(int(ref.mask(host.map_sequences([t])[0], 0.9)[1]) for t in targets)
        low = 'ACDEFGHIKL' + 'SSSSSSSSSSSSSSSSSSSS' + 'MNPQRSTVWY'
        lm, n_low = ref.mask(host.map_sequences([low])[0], 0.9)
        assert n_low > 0, 'the low-complexity probe is not masked by the reference'
        # ... and the driver, which constructs the Masker and never calls it, keeps the probe's letters in the lookup and indexes its windows
        r = run_driver(exe, tmp, [low], [], 112)
        assert (r['lookup'] == host.map_sequences([low])[0]).all() and (r['lookup'] != lm).any()
        assert int((r['window_len'][10:20] > 0).sum()) > 0
        out['M_letters'], out['M_off'] = pack([low])
        out['M_masked_by_tantan'] = np.int64(n_low)
        out['M_entries'] = np.int64(r['n_entries'])
        out['M_digest'] = np.array(digest(r['list_kmer'], r['list_start'], r['entry_seq'], r['entry_pos']))
        print('set M: tantan would mask %d residues of the probe (%d of set G); the branch masks none' % (n_low, masked))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print('wrote %s (%d bytes)' % (OUT, size))
    assert size < (1 << 20)


if __name__ == '__main__':
    main()
