#!/usr/bin/env python3
"""Writes tests/golden/expand_vectors.npz from the LIVE reference: what `expandaln --expansion-mode 0` (M/src/util/expandaln.cpp:86-464
with returnAlnRes = true) makes of an A -> B and a B -> C alignment DB.  Results and inputs only.

expandaln itself cannot be linked (DBReader / DBWriter / Parameters), so DRIVER below (ours) restates its loop over entries in memory and
calls the reference's own BacktraceTranslator::translateResult, Matcher::parseAlignmentRecord / readAlignmentResults' row parser,
Matcher::resultToBuffer, Util::canBeCovered / hasCoverage, SmithWaterman::computeCov, IntervalArray and DBReader::setExtendedDbtype.  It
is compiled into a temporary directory against the reference's headers, together with the reference's Matcher.cpp where it lies, and
linked to oracle/_ref/libsdref.so; nothing compiled is kept.

    python tools/make_golden_expand.py [reference root]          (needs `make -C oracle _ref/libsdref.so`; no GPU)

Per set the file holds the two input DBs, the entries the reference writes, and for every translated pair (in the order expandaln
meets them) translateResult's coordinates and printed backtrace:
  K   tests/expgen.py set_k: one query per named pair class, at the module's defaults
  P   tests/expgen.py set_p: rows on either side of every criterion's threshold, one output per parameter set of expgen.P_PARAMS
  G   set G of tests/golden/swap_vectors.npz: its G95_final_1 entries (152 sequence queries against 18 profiles) as A -> B, and as B -> C
      a clustering of the 152 sequences made by hand from G95_aln_swapped -- the reference matcher's profile -> sequence alignments with
      backtrace: every sequence is the member of the first profile that lists it -- expanded at the module's defaults
dbtype: the output DB's type (DBTYPE_ALIGNMENT_RES with DBTYPE_EXTENDED_INDEX_NEED_SRC).
--expansion-mode 1 (rescoreResultByBacktrace, compiled from expandaln.cpp where it lies), sequences on both sides (A = C = the 152):
  G1  set G without the A -> B rows that have a pair whose walk leaves a sequence (the generator walks every pair itself and fails
      if one is left: every recorded row is defined behaviour), one output per --seq-id-mode 0 .. 3
  M   constructed rows "1M2I1M" through an identity B -> C row, placed where the walk's raw score is exactly -6 (kept) and -7 (dropped),
      and a real row of set G, at -e 1e9, with and without composition bias (the bias changes the scores)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLD = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLD, 'expand_vectors.npz')

DRIVER = r'''
// rescoreResultByBacktrace is a free function of expandaln.cpp: the file is compiled where it lies; its DB-bound entry points are not
// referenced and go with their sections at link time
#include "expandaln.cpp"
#include "SubstitutionMatrix.h"
#include "Matcher.h"
#include "BacktraceTranslator.h"
#include "IntervalArray.h"
#include "DBReader.h"
#include "Parameters.h"
#include "Util.h"
#include "Debug.h"
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <stack>
#include <string>
#include <vector>
// argv: blosum62 path, job file, result file.
// job:    f64 evalThr; f32 covThr; i32 covMode; f32 seqIdThr; i32 alnLenThr; i32 expansionMode; i32 seqIdMode; i32 compBiasCorr; f32
//         compBiasScale; then the A -> B DB, the B -> C DB and (mode 1: the letters of) the A and the C sequence DB, each u32 nEntries
//         and per entry u32 key, u64 length, text
// result: i32 dbtype; u32 nEntries, per entry u32 key, u64 length, text; u32 nPairs, per pair i32 qStart, qEnd, dbStart, dbEnd, u32 columns of
//         the printed backtrace, u64 length + its compressed text ("" when there is none)
struct Entry {
    unsigned int key;
    std::string text;
};
static bool readDb(FILE *in, std::vector<Entry> &db) {
    unsigned int n;
    if (fread(&n, 4, 1, in) != 1) return false;
    db.resize(n);
    for (Entry &e : db) {
        uint64_t len;
        if (fread(&e.key, 4, 1, in) != 1 || fread(&len, 8, 1, in) != 1) return false;
        e.text.resize(len);
        if (len && fread(&e.text[0], 1, len, in) != len) return false;
    }
    return true;
}
int main(int argc, char **argv) {
    if (argc != 4) return 1;
    Debug::setDebugLevel(1);
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 1;
    double evalThr;
    float covThr, seqIdThr, compBiasScale;
    int covMode, alnLenThr, expansionMode, seqIdMode, compBiasCorr;
    if (fread(&evalThr, 8, 1, in) != 1 || fread(&covThr, 4, 1, in) != 1 || fread(&covMode, 4, 1, in) != 1 || fread(&seqIdThr, 4, 1, in) != 1 ||
        fread(&alnLenThr, 4, 1, in) != 1 || fread(&expansionMode, 4, 1, in) != 1 || fread(&seqIdMode, 4, 1, in) != 1 ||
        fread(&compBiasCorr, 4, 1, in) != 1 || fread(&compBiasScale, 4, 1, in) != 1)
        return 2;
    std::vector<Entry> ab, bcDb, aDb, cDb;
    if (!readDb(in, ab) || !readDb(in, bcDb) || !readDb(in, aDb) || !readDb(in, cDb)) return 2;
    fclose(in);
    const bool rescore = expansionMode == Parameters::EXPAND_RESCORE_BACKTRACE;
    SubstitutionMatrix subMat(argv[1], 2.0, 0.0);
    std::map<unsigned int, const Entry *> aOfKey, cOfKey;
    size_t cResidues = 0, maxLen = 0;
    for (const Entry &e : aDb) { aOfKey[e.key] = &e; maxLen = std::max(maxLen, e.text.size()); }
    for (const Entry &e : cDb) { cOfKey[e.key] = &e; cResidues += e.text.size(); maxLen = std::max(maxLen, e.text.size()); }
    EvalueComputation evaluer(cResidues, &subMat, 11, 1);          // cReader->getAminoAcidDBSize()
    Sequence aSeq(maxLen + 1, Parameters::DBTYPE_AMINO_ACIDS, &subMat, 0, false, compBiasCorr != 0);
    Sequence cSeq(maxLen + 1, Parameters::DBTYPE_AMINO_ACIDS, &subMat, 0, false, false);
    std::vector<float> compositionBias(maxLen + 2, 0.0f);
    std::map<unsigned int, const Entry *> bcOfKey;
    for (const Entry &e : bcDb) bcOfKey[e.key] = &e;
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 1;
    int dbType = DBReader<unsigned int>::setExtendedDbtype(Parameters::DBTYPE_ALIGNMENT_RES, Parameters::DBTYPE_EXTENDED_INDEX_NEED_SRC);
    fwrite(&dbType, 4, 1, out);
    const unsigned int nEntries = (unsigned int) ab.size();
    fwrite(&nEntries, 4, 1, out);
    BacktraceTranslator translator;
    std::vector<char> buffer(1024 + 32768 * 4 + (1 << 20));
    std::vector<Matcher::result_t> resultsBc, resultsAc;
    Matcher::result_t resultAc;
    std::map<unsigned int, IntervalArray *> interval;
    std::stack<IntervalArray *> intervalBuffer;
    std::string pairDump;
    unsigned int nPairs = 0;
    for (Entry &e : ab) {
        if (rescore) {
            const Entry *a = aOfKey.at(e.key);
            aSeq.mapSequence(0, e.key, a->text.c_str(), a->text.size());
            std::fill(compositionBias.begin(), compositionBias.end(), 0.0f);
            if (compBiasCorr != 0)
                SubstitutionMatrix::calcLocalAaBiasCorrection(&subMat, aSeq.numSequence, aSeq.L, compositionBias.data(), compBiasScale);
        }
        e.text.push_back('\0');
        char *data = &e.text[0];
        while (*data != '\0') {
            Matcher::result_t resultAb = Matcher::parseAlignmentRecord(data, false);
            data = Util::skipLine(data);
            if (resultAb.backtrace.empty()) return 5;   // "Alignment must contain a backtrace"
            std::map<unsigned int, const Entry *>::const_iterator bcIt = bcOfKey.find(resultAb.dbKey);
            if (bcIt == bcOfKey.end()) continue;        // "Missing alignments for sequence"
            std::string bcText = bcIt->second->text;
            bcText.push_back('\0');
            Matcher::readAlignmentResults(resultsBc, &bcText[0], false);
            for (size_t k = 0; k < resultsBc.size(); ++k) {
                Matcher::result_t &resultBc = resultsBc[k];
                if (resultBc.backtrace.size() == 0) return 5;
                translator.translateResult(resultAb, resultBc, resultAc);
                {
                    const int v[4] = {resultAc.qStartPos, resultAc.qEndPos, resultAc.dbStartPos, resultAc.dbEndPos};
                    const unsigned int cols = (unsigned int) resultAc.backtrace.size();
                    const std::string cig = cols ? Matcher::compressAlignment(resultAc.backtrace) : std::string();
                    const uint64_t len = cig.size();
                    pairDump.append((const char *) v, 16);
                    pairDump.append((const char *) &cols, 4);
                    pairDump.append((const char *) &len, 8);
                    pairDump.append(cig);
                    nPairs++;
                }
                if (resultAc.backtrace.size() == 0) continue;
                if (Util::canBeCovered(covThr, covMode, resultAc.qLen, resultAc.dbLen) == false) continue;
                unsigned int cSeqKey = resultBc.dbKey;
                std::map<unsigned int, IntervalArray *>::iterator it = interval.find(cSeqKey);
                if (it != interval.end()) {
                    if (it->second->doesOverlap(resultAc.qStartPos, resultAc.qEndPos)) continue;
                } else {
                    if (rescore) {
                        const Entry *c = cOfKey.at(cSeqKey);
                        cSeq.mapSequence(0, cSeqKey, c->text.c_str(), c->text.size());
                        rescoreResultByBacktrace(resultAc, aSeq, cSeq, subMat, compositionBias.data(), 11, 1);
                        if (resultAc.score < -6) continue;
                        resultAc.eval = evaluer.computeEvalue(resultAc.score, aSeq.L);
                        resultAc.score = static_cast<int>(evaluer.computeBitScore(resultAc.score) + 0.5);
                        resultAc.seqId = Util::computeSeqId(seqIdMode, resultAc.seqId, aSeq.L, cSeq.L, resultAc.backtrace.size());
                    } else {
                    resultAc.eval = resultAb.eval;
                    resultAc.score = resultAb.score;
                    resultAc.seqId = resultAb.seqId;
                    }
                    float queryCov = SmithWaterman::computeCov(resultAc.qStartPos, resultAc.qEndPos, resultAc.qLen);
                    float targetCov = SmithWaterman::computeCov(resultAc.dbStartPos, resultAc.dbEndPos, resultAc.dbLen);
                    bool hasCov = Util::hasCoverage(covThr, covMode, queryCov, targetCov);
                    bool hasSeqId = resultAc.seqId >= (seqIdThr - std::numeric_limits<float>::epsilon());
                    bool hasEvalue = (resultAc.eval <= evalThr);
                    bool hasAlnLen = (static_cast<int>(resultAc.alnLength) >= alnLenThr);
                    if (hasCov && hasSeqId && hasEvalue && hasAlnLen) {
                        resultsAc.emplace_back(resultAc);
                        IntervalArray *tmp;
                        if (intervalBuffer.size() == 0) {
                            tmp = new IntervalArray();
                        } else {
                            tmp = intervalBuffer.top();
                            intervalBuffer.pop();
                        }
                        tmp->insert(resultAc.qStartPos, resultAc.qEndPos);
                        interval.insert(std::make_pair(cSeqKey, tmp));
                    }
                }
            }
            resultsBc.clear();
        }
        for (std::map<unsigned int, IntervalArray *>::iterator it = interval.begin(); it != interval.end(); ++it) {
            it->second->reset();
            intervalBuffer.push(it->second);
        }
        interval.clear();
        std::string text;
        for (size_t j = 0; j < resultsAc.size(); ++j) {
            size_t len = Matcher::resultToBuffer(buffer.data(), resultsAc[j], true, true);
            text.append(buffer.data(), len);
        }
        resultsAc.clear();
        const uint64_t len = text.size();
        fwrite(&e.key, 4, 1, out);
        fwrite(&len, 8, 1, out);
        fwrite(text.data(), 1, len, out);
    }
    fwrite(&nPairs, 4, 1, out);
    fwrite(pairDump.data(), 1, pairDump.size(), out);
    fclose(out);
    return 0;
}
'''


def build_driver(ref_root, tmp):
    """compiles DRIVER and the reference's Matcher.cpp into tmp, linked to oracle/_ref/libsdref.so; returns the program's path"""
    m = os.path.join(ref_root, 'lib', 'mmseqs')
    src, exe = os.path.join(tmp, 'driver.cpp'), os.path.join(tmp, 'driver')
    open(src, 'w').write(DRIVER)
    inc = [os.path.join(m, *p) for p in (('src', 'commons'), ('src', 'alignment'), ('src', 'prefiltering'), ('lib',), ('lib', 'simd'),
                                          ('lib', 'alp'), ('lib', 'tantan'), ('lib', 'fmt'), ('lib', 'simde'), ('lib', 'zstd', 'lib'), ('src', 'util'))]
    refdir = os.path.join(ROOT, 'oracle', '_ref')
    # (sections: what Matcher.cpp and DBReader.h name but the driver never reaches is dropped at link time)
    subprocess.check_call(['g++', '-std=c++14', '-O3', '-mavx2', '-mfma', '-mcx16', '-DAVX2=1', '-DOPENMP=1', '-fopenmp', '-w',
                           '-ffunction-sections', '-fdata-sections'] + ['-I' + d for d in inc] +
                          [src, os.path.join(m, 'src', 'alignment', 'Matcher.cpp'), '-L' + refdir, '-lsdref', '-Wl,-rpath,' + refdir,
                           '-Wl,--gc-sections', '-Wl,--allow-shlib-undefined', '-o', exe])
    return exe


def db_bytes(db):
    return struct.pack('<I', len(db)) + b''.join(struct.pack('<IQ', k, len(t)) + t for k, t in sorted(db.items()))


def run_driver(exe, tmp, ab, bc, params, a_seqs=None, c_seqs=None):
    """ab / bc: dict key -> bytes.  Returns (dbtype, dict key -> bytes, pair coordinates int32 [n, 5], list of pair texts)."""
    import exp_ref
    p = dict(exp_ref.DEFAULTS)
    p.update(params)
    job, res = os.path.join(tmp, 'job.bin'), os.path.join(tmp, 'res.bin')
    with open(job, 'wb') as f:
        f.write(struct.pack('<dfifiiiif', p['e'], p['c'], p['cov_mode'], p['min_seq_id'], p['min_aln_len'], p['mode'], p['seq_id_mode'],
                            p['comp_bias_corr'], 1.0) + db_bytes(ab) + db_bytes(bc) + db_bytes(a_seqs or {}) + db_bytes(c_seqs or {}))
    from oracle.pyoracle import matrix_spec
    subprocess.check_call([exe, matrix_spec(0), job, res])
    raw = open(res, 'rb').read()
    dbtype, n = struct.unpack_from('<iI', raw, 0)
    at, out = 8, {}
    for _ in range(n):
        k, ln = struct.unpack_from('<IQ', raw, at)
        out[k] = raw[at + 12:at + 12 + ln]
        at += 12 + ln
    n_pairs, = struct.unpack_from('<I', raw, at)
    at += 4
    coords, texts = np.zeros((n_pairs, 5), np.int32), []
    for i in range(n_pairs):
        coords[i] = struct.unpack_from('<iiiiI', raw, at)
        ln, = struct.unpack_from('<Q', raw, at + 20)
        texts.append(raw[at + 28:at + 28 + ln])
        at += 28 + ln
    assert at == len(raw)
    return dbtype, out, coords, texts


def pack(out, name, db):
    """dict key -> bytes as three arrays: keys, offsets, text"""
    keys = sorted(db)
    off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        off[1:] = np.cumsum([len(db[k]) for k in keys])
    out[name + '_keys'] = np.array(keys, np.uint32)
    out[name + '_off'] = off
    out[name + '_text'] = np.frombuffer(b''.join(db[k] for k in keys), np.uint8)


def pack_pairs(out, name, coords, texts):
    out[name + '_pairs'] = coords
    off = np.zeros(len(texts) + 1, np.uint64)
    if texts:
        off[1:] = np.cumsum([len(t) for t in texts])
    out[name + '_pair_off'] = off
    out[name + '_pair_text'] = np.frombuffer(b''.join(texts), np.uint8)


def unpack(g, name):
    keys, off, text = g[name + '_keys'], g[name + '_off'].astype(np.int64), g[name + '_text'].tobytes()
    return {int(k): text[off[i]:off[i + 1]] for i, k in enumerate(keys)}


def set_g():
    """A -> B: G95_final_1 of swap_vectors.npz.  B -> C: every sequence under the first profile (by key) of G95_aln_swapped that lists it."""
    s = np.load(os.path.join(GOLD, 'swap_vectors.npz'))
    ab = unpack(s, 'G95_final_1')
    listed = unpack(s, 'G95_aln_swapped')
    member_of, bc = {}, {}
    for p in sorted(listed):
        rows = []
        for l in listed[p].splitlines(keepends=True):
            seq = int(l.split(b'\t')[0])
            if seq not in member_of:
                member_of[seq] = p
                rows.append(l)
        if rows:
            bc[p] = b''.join(rows)
    return ab, bc


def mode1_sets(out, exe, tmp, ab, bc):
    import exp_ref
    import expgold
    from spacedust_amd.api import Host
    seqs = expgold.mode1_seqs(Host())
    letters = {i: s.encode() for i, s in enumerate(seqs['letters'])}
    bc_rows = {k: exp_ref.rows_of(t) for k, t in bc.items()}

    def inside(q, line):
        r = exp_ref.parse_row(line.decode().rstrip('\n'))
        for m in bc_rows.get(r['key'], []):
            a0, _, c0, _, n, text = exp_ref.translate_runs(r['q_start'], r['db_start'], exp_ref.runs_of(r['cigar']), m['q_start'], m['db_start'],
                                                        exp_ref.runs_of(m['cigar']))
            if n and exp_ref.walk(exp_ref.uncompress(text), a0, c0, seqs['a'][q], seqs['c'][m['key']], None, seqs['matrix']) is None:
                return False
        return True
    ab1 = {q: b''.join(l for l in t.splitlines(keepends=True) if inside(q, l)) for q, t in ab.items()}
    dropped = sum(t.count(b'\n') for t in ab.values()) - sum(t.count(b'\n') for t in ab1.values())
    pack(out, 'G1_ab', ab1)
    for mode in range(4):
        par = dict(mode=1, seq_id_mode=mode)
        walks = []
        exp_ref.expand(ab1, bc, par, seqs=dict(seqs, walks=walks))
        assert walks and all(w is not None for w in walks), 'a recorded walk leaves a sequence'
        _, res, coords, texts = run_driver(exe, tmp, ab1, bc, par, letters, letters)
        pack(out, 'G1_out_%d' % mode, res)
        print('set G1, --seq-id-mode %d: %d rows kept of %d pairs (%d A -> B rows left out: a walk leaves a sequence)'
              % (mode, sum(t.count(b'\n') for t in res.values()), len(coords), dropped))
    pack_pairs(out, 'G1', coords, texts)
    # M: "1M2I1M" from A position a0 against C position c0: raw = s(a0, c0) + bias(a0) - 11 - 1 + s(a0 + 3, c0 + 1) + bias(a0 + 3)
    found = {}
    for q in range(4):
        for c in range(4, 8):
            for a0 in range(0, len(seqs['a'][q]) - 4):
                for c0 in range(0, len(seqs['c'][c]) - 2):
                    w = exp_ref.walk('MIIM', a0, c0, seqs['a'][q], seqs['c'][c], seqs['a_bias'][q], seqs['matrix'])
                    if w[0] == (-6 if c < 6 else -7) and w[0] not in found:   # (two C keys: a query keeps one row per key)
                        found[w[0]] = (q, c, a0, c0)
    assert sorted(found) == [-7, -6]
    m_ab, m_bc = {}, {}
    for i, raw in enumerate((-6, -7)):
        q, c, a0, c0 = found[raw]
        a_len, c_len = len(seqs['a'][q]), len(seqs['c'][c])
        m_ab[q] = m_ab.get(q, b'') + b'%d\t10\t0.500\t1.000E-01\t%d\t%d\t%d\t%d\t%d\t%d\t1M2I1M\n' % (500 + i, a0, a0 + 3, a_len, 20, 21, 100)
        m_bc[500 + i] = b'%d\t10\t1.00\t1.000E-01\t%d\t%d\t%d\t%d\t%d\t%d\t4M\n' % (c, 20, 23, 100, c0, c0 + 3, c_len)
    real_q = next(q for q in sorted(ab1) if ab1[q] and q not in m_ab)
    m_ab[real_q] = ab1[real_q]
    for k in set(exp_ref.parse_row(l)['key'] for l in ab1[real_q].decode().splitlines()):
        m_bc[k] = bc[k]
    pack(out, 'M_ab', m_ab)
    pack(out, 'M_bc', m_bc)
    out['M_raw_queries'] = np.array([found[-6][0], found[-7][0], real_q], np.int64)
    for bias in (1, 0):
        par = dict(mode=1, e=1e9, comp_bias_corr=bias)
        _, res, coords, texts = run_driver(exe, tmp, m_ab, m_bc, par, letters, letters)
        pack(out, 'M_out_bias%d' % bias, res)
        print('set M, --comp-bias-corr %d: %d rows kept of %d pairs' % (bias, sum(t.count(b'\n') for t in res.values()), len(coords)))
    pack_pairs(out, 'M', coords, texts)


def main():
    import expgen
    ref_root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        ab, bc = expgen.set_k()
        dbtype, res, coords, texts = run_driver(exe, tmp, ab, bc, {})
        out['dbtype'] = np.int32(dbtype)
        pack(out, 'K_ab', ab)
        pack(out, 'K_bc', bc)
        pack(out, 'K_out', res)
        pack_pairs(out, 'K', coords, texts)
        print('set K: %d queries, %d pairs, %d rows kept' % (len(ab), len(coords), sum(t.count(b'\n') for t in res.values())))
        ab, bc = expgen.set_p()
        pack(out, 'P_ab', ab)
        pack(out, 'P_bc', bc)
        for i, par in enumerate(expgen.P_PARAMS):
            _, res, coords, texts = run_driver(exe, tmp, ab, bc, par)
            pack(out, 'P_out_%d' % i, res)
            print('set P, %s: %d rows kept of %d pairs' % (par, sum(t.count(b'\n') for t in res.values()), len(coords)))
        pack_pairs(out, 'P', coords, texts)
        ab, bc = set_g()
        _, res, coords, texts = run_driver(exe, tmp, ab, bc, {})
        pack(out, 'G_ab', ab)
        pack(out, 'G_bc', bc)
        pack(out, 'G_out', res)
        pack_pairs(out, 'G', coords, texts)
        print('set G: %d queries, %d clusters with %d members, %d pairs, %d rows kept'
              % (len(ab), len(bc), sum(t.count(b'\n') for t in bc.values()), len(coords), sum(t.count(b'\n') for t in res.values())))
        mode1_sets(out, exe, tmp, ab, bc)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print('wrote %s (%d bytes)' % (OUT, size))
    assert size < 200 * 1024


if __name__ == '__main__':
    main()
