#!/usr/bin/env python3
"""Writes tests/golden/swap_vectors.npz from the LIVE reference: what `swapresults` (doswap(par, false), M/src/util/swapresults.cpp:18-348)
makes of the prefilter rows of sequence queries against a profile target DB, the alignments of the swapped prefilter result with the
profile as the Smith-Waterman query, and the second swap of those -- the chain of M/data/workflow/searchtargetprofile.sh.  Results
and inputs only.

doswap itself cannot be linked (DBReader / DBWriter / Parameters), so DRIVER below (ours) restates its control flow over entries in
memory and calls the reference's own Matcher::parseAlignmentRecord, Matcher::result_t::swapResult, Matcher::compareHits,
Matcher::resultToBuffer, QueryMatcher::parsePrefilterHit / prefilterHitToBuffer and EvalueComputation.  It is compiled into a temporary
directory against the reference's headers, together with the reference's Matcher.cpp where it lies, and linked to oracle/_ref/libsdref.so;
nothing compiled is kept.

    python tools/make_golden_swap.py [reference root]          (needs `make -C oracle _ref/libsdref.so`; no GPU)

Inputs: the 18 profiles of set G and the 152 sequence queries of tests/golden/target_profile_vectors.npz with its prefilter rows at
threshold 110 (83 rows) and 95 (183 rows), both with composition bias.  Per row set (tests/test_swapresults.py checks the conditions,
tests/test_gpu_target_profile_search.py the modules and `search` against the texts):
  pref / pref_swapped   the prefilter DB as `prefilter` writes it and its swap, per profile key
  aln_swapped           the reference matcher with the profile as the query (oracle.pyoracle.RefSW: backtrace mode, E-value over the
                        residues of the 152 sequences, no coverage gate) at -e E[0], lines as Matcher::resultToBuffer prints them
  final_0 / final_1     the second swap at -e E[0] and at -e E[1]
  E                     E[0]: every aligned row survives the second swap.  E[1]: the recomputed E-value (over the profile DB's residues,
                        with the sequence's length) removes rows `align` had kept and leaves a query with an empty entry; E[1] lies in
                        no row's interval [swapped E-value, aligned E-value), so `search -e E[1]` -- whose align step runs at E[1] too --
                        ends at final_1 as well.
A constructed set C for the swap alone: diagonals -32768 and 32767, equal scores on one target, a target key without hits, a key gap
in the target DB, rows on a key the DB does not hold, run-length backtraces with I and D runs, rows without a backtrace column, an
entry emptied by the E-value on a key the DB does not hold.
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLD, 'swap_vectors.npz')

DRIVER = r'''
#include "SubstitutionMatrix.h"
#include "EvalueComputation.h"
#include "Matcher.h"
#include "QueryMatcher.h"
#include "Util.h"
#include "Debug.h"
#include "itoa.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
// argv: blosum62 path, job file, result file.
// job:    u64 residues of the first DB; f64 evalThr; u32 nKeys; u32 keys[nKeys] of the second DB; u32 nEntries; per entry u32 key,
//         u64 length, text
// result: u32 nEntries; per entry u32 key, u64 length, text -- the entries doswap(par, false) writes, by key
struct Entry {
    unsigned int key;
    std::string text;
};
int main(int argc, char **argv) {
    if (argc != 4) return 1;
    Debug::setDebugLevel(1);
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 1;
    uint64_t aaResSize;
    double evalThr;
    unsigned int nKeys, nEntries;
    if (fread(&aaResSize, 8, 1, in) != 1 || fread(&evalThr, 8, 1, in) != 1 || fread(&nKeys, 4, 1, in) != 1) return 2;
    std::vector<unsigned int> keys(nKeys);
    if (nKeys && fread(keys.data(), 4, nKeys, in) != nKeys) return 2;
    if (fread(&nEntries, 4, 1, in) != 1) return 2;
    std::vector<Entry> entries(nEntries);
    for (Entry &e : entries) {
        uint64_t len;
        if (fread(&e.key, 4, 1, in) != 1 || fread(&len, 8, 1, in) != 1) return 2;
        e.text.resize(len);
        if (len && fread(&e.text[0], 1, len, in) != len) return 2;
    }
    fclose(in);
    SubstitutionMatrix subMat(argv[1], 2.0, 0.0);
    EvalueComputation evaluer(aaResSize, &subMat, 11, 1);
    const unsigned int maxTargetId = *std::max_element(keys.begin(), keys.end());
    std::vector<char> targetElementExists(maxTargetId + 1, 0);
    for (unsigned int k : keys) targetElementExists[k] = 1;
    // the lines with the entry's key in front, gathered per target key (doswap: sizes, exclusive scan, copy)
    std::vector<std::string> perTarget(maxTargetId + 1);
    bool isAlignmentResult = false, hasBacktrace = false, formKnown = false;
    for (Entry &e : entries) {
        char *data = &e.text[0];
        if (!formKnown && *data != '\0') {
            const char *entry[255];
            const size_t columns = Util::getWordsOfLine(data, entry, 255);
            isAlignmentResult = columns >= Matcher::ALN_RES_WITHOUT_BT_COL_CNT;
            hasBacktrace = columns >= Matcher::ALN_RES_WITH_BT_COL_CNT;
            formKnown = true;
        }
        char queryKeyStr[64];
        *Itoa::u32toa_sse2((uint32_t) e.key, queryKeyStr) = '\0';
        while (*data != '\0') {
            char dbKeyBuffer[256];
            Util::parseKey(data, dbKeyBuffer);
            const unsigned int dbKey = (unsigned int) strtoul(dbKeyBuffer, NULL, 10);
            char *nextLine = Util::skipLine(data);
            if (dbKey > maxTargetId) return 4;
            perTarget[dbKey].append(queryKeyStr);
            perTarget[dbKey].append(data + strlen(dbKeyBuffer), nextLine - data - strlen(dbKeyBuffer));
            data = nextLine;
        }
    }
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 1;
    std::vector<Entry> written;
    std::vector<Matcher::result_t> curRes;
    std::vector<char> buffer(1024 + 32768 * 4);
    for (unsigned int i = 0; i <= maxTargetId; i++) {
        char *data = &perTarget[i][0];
        size_t dataSize = perTarget[i].size();
        bool evalBreak = false;
        curRes.clear();
        while (dataSize > 0) {
            if (isAlignmentResult) {
                Matcher::result_t res = Matcher::parseAlignmentRecord(data, true);
                Matcher::result_t::swapResult(res, evaluer, hasBacktrace);
                if (res.eval > evalThr) evalBreak = true;
                else curRes.emplace_back(res);
            } else {
                hit_t hit = QueryMatcher::parsePrefilterHit(data);
                hit.diagonal = static_cast<unsigned short>(static_cast<short>(hit.diagonal) * -1);
                curRes.emplace_back(hit.seqId, hit.prefScore, 0, 0, 0, -static_cast<float>(hit.prefScore), hit.diagonal, 0, 0, 0, 0, 0, 0, "");
            }
            char *nextLine = Util::skipLine(data);
            dataSize -= nextLine - data;
            data = nextLine;
        }
        if (!curRes.empty()) {
            std::sort(curRes.begin(), curRes.end(), Matcher::compareHits);
            Entry e;
            e.key = i;
            for (const Matcher::result_t &res : curRes) {
                size_t len;
                if (isAlignmentResult) {
                    len = Matcher::resultToBuffer(buffer.data(), res, hasBacktrace, false);
                } else {
                    hit_t hit;
                    hit.seqId = res.dbKey;
                    hit.prefScore = res.score;
                    hit.diagonal = res.alnLength;
                    len = QueryMatcher::prefilterHitToBuffer(buffer.data(), hit);
                }
                e.text.append(buffer.data(), len);
            }
            written.push_back(e);
        } else if (evalBreak || targetElementExists[i] == 1) {
            Entry e;
            e.key = i;
            written.push_back(e);
        }
    }
    const unsigned int n = (unsigned int) written.size();
    fwrite(&n, 4, 1, out);
    for (const Entry &e : written) {
        const uint64_t len = e.text.size();
        fwrite(&e.key, 4, 1, out);
        fwrite(&len, 8, 1, out);
        fwrite(e.text.data(), 1, len, out);
    }
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
                                          ('lib', 'alp'), ('lib', 'tantan'), ('lib', 'fmt'), ('lib', 'simde'), ('lib', 'zstd', 'lib'))]
    refdir = os.path.join(ROOT, 'oracle', '_ref')
    # (sections: Matcher's constructor, which wants the nucleotide aligner, is not reached and is dropped at link time)
    subprocess.check_call(['g++', '-std=c++14', '-O3', '-mavx2', '-mfma', '-mcx16', '-DAVX2=1', '-DOPENMP=1', '-fopenmp', '-w',
                           '-ffunction-sections', '-fdata-sections'] + ['-I' + d for d in inc] +
                          [src, os.path.join(m, 'src', 'alignment', 'Matcher.cpp'), '-L' + refdir, '-lsdref', '-Wl,-rpath,' + refdir,
                           '-Wl,--gc-sections', '-Wl,--allow-shlib-undefined', '-o', exe])
    return exe


def run_driver(exe, tmp, entries, first_db_residues, second_db_keys, eval_thr):
    """entries: list of (key, bytes).  Returns dict key -> bytes of the entries the reference's swap writes."""
    from oracle.pyoracle import matrix_spec
    job, res = os.path.join(tmp, 'job.bin'), os.path.join(tmp, 'res.bin')
    with open(job, 'wb') as f:
        f.write(struct.pack('<Qd', first_db_residues, eval_thr))
        keys = np.ascontiguousarray(second_db_keys, np.uint32)
        f.write(struct.pack('<I', len(keys)) + keys.tobytes() + struct.pack('<I', len(entries)))
        for k, t in entries:
            f.write(struct.pack('<IQ', k, len(t)) + t)
    subprocess.check_call([exe, matrix_spec(0), job, res])
    raw = open(res, 'rb').read()
    n, = struct.unpack_from('<I', raw, 0)
    at, out = 4, {}
    for _ in range(n):
        k, ln = struct.unpack_from('<IQ', raw, at)
        out[k] = raw[at + 12:at + 12 + ln]
        at += 12 + ln
    assert at == len(raw)
    return out


def seqid_text(seqid):
    """Util::fastSeqIdToBuffer as Matcher::resultToBuffer leaves it (tools/make_golden_alndb.py pins this against the binary's DB)"""
    if seqid == np.float32(1.0):
        return '1.00'
    return '0.' + ('0' if seqid < np.float32(0.10) else '') + ('0' if seqid < np.float32(0.01) else '') + str(int(np.float32(seqid * np.float32(1000))))


def compress(bt):
    cig, st, c = [], 'M', 0
    for ch in bt:
        if ch != st:
            cig.append('%d%s' % (c, st))
            st, c = ch, 1
        else:
            c += 1
    cig.append('%d%s' % (c, st))
    return ''.join(cig)


def pack(out, name, db):
    """dict key -> bytes as three arrays: keys, offsets, text"""
    keys = sorted(db)
    off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        off[1:] = np.cumsum([len(db[k]) for k in keys])
    out[name + '_keys'] = np.array(keys, np.uint32)
    out[name + '_off'] = off
    out[name + '_text'] = np.frombuffer(b''.join(db[k] for k in keys), np.uint8)


def evalues(db):
    """(entry key, first column, E-value text as a float) of every alignment line"""
    rows = []
    for k, t in db.items():
        for l in t.decode().splitlines():
            c = l.split('\t')
            rows.append((k, int(c[0]), float(c[3])))
    return rows


def main():
    from oracle.pyoracle import Ref, RefSW
    ref_root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    g = np.load(os.path.join(GOLD, 'target_profile_vectors.npz'))
    pv = np.load(os.path.join(GOLD, 'profile_vectors.npz'))
    poff = pv['poff'].astype(np.int64)
    pdata = pv['profiles'].tobytes()
    profiles = [pdata[poff[i]:poff[i + 1]] for i in range(len(poff) - 1)]
    qoff = g['Q_off'].astype(np.int64)
    letters = g['Q_letters'].tobytes().decode()
    queries = [letters[qoff[i]:qoff[i + 1]] for i in range(len(qoff) - 1)]
    n_prof, n_q = len(profiles), len(queries)
    assert (n_prof, n_q) == (18, 152)
    seq_residues = int(qoff[-1])                                                   # DBReader::getAminoAcidDBSize of the sequence DB
    prof_residues = sum(len(p) + 1 for p in profiles) // 25 - n_prof               # ... of the profile DB (DBReader.cpp:589-597)
    prof_len = [len(p) // 25 for p in profiles]
    out = dict(seq_residues=np.int64(seq_residues), prof_residues=np.int64(prof_residues))
    ref = Ref(6)
    sw = RefSW(ref, max(max(prof_len), max(len(q) for q in queries)) + 10, seq_residues)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        for thr, n_rows in ((110, 83), (95, 183)):
            tag = 'G%d' % thr
            rows = g['rows_%d_bias1' % thr].astype(np.int64)
            assert len(rows) == n_rows
            pref = {q: b'' for q in range(n_q)}
            for q, t, s, d in rows:
                pref[int(q)] += b'%d\t%d\t%d\n' % (t, s, int(np.int16(np.uint16(d & 0xFFFF))))
            pref_swapped = run_driver(exe, tmp, sorted(pref.items()), seq_residues, range(n_prof), 0.001)
            assert sorted(pref_swapped) == list(range(n_prof)) and sum(t.count(b'\n') for t in pref_swapped.values()) == n_rows

            def align(e_align):
                """`align <profileDB> <sequenceDB> pref_swapped` -a 1 -e e_align -c 0: Matcher::getSWResult, Alignment::checkCriteria,
                compareHits order, resultToBuffer"""
                aln = {}
                for p in sorted(pref_swapped):
                    sw.set_query_profile(profiles[p])
                    mine = []
                    for l in pref_swapped[p].decode().splitlines():
                        s = int(l.split('\t')[0])
                        r = sw.align(queries[s], sw_mode=2, eval_thr=e_align, cov_mode=0, cov_thr=0.0)
                        if r['tStart'] < 0 or r['qStart'] < 0 or r['btLen'] == 0 or not r['evalue'] <= e_align:
                            continue
                        bits = int(sw.bitscore(r['score']) + 0.5)
                        seqid = np.float32(r['identical']) / np.float32(r['btLen'])
                        text = '%d\t%d\t%s\t%.3E\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n' % (s, bits, seqid_text(seqid), r['evalue'], r['qStart'], r['qEnd'],
                                                                               prof_len[p], r['tStart'], r['tEnd'], len(queries[s]),
                                                                               compress(r['backtrace']))
                        mine.append(((r['evalue'], -bits, len(queries[s]), s), text, r['evalue']))
                    mine.sort(key=lambda x: x[0])
                    aln[p] = ''.join(t for _, t, _ in mine).encode()
                return aln

            # every prefilter row aligned and kept, swapped without a threshold: the two E-values of every row
            all_aln = align(1e300)
            both = {}
            for k, s, e in evalues(all_aln):
                both[(k, s)] = [e, None]
            for s, k, e in evalues(run_driver(exe, tmp, sorted(all_aln.items()), prof_residues, range(n_q), 1e300)):
                both[(k, s)][1] = e
            assert all(b is not None for _, b in both.values())
            ratio = sorted(a / b for a, b in both.values() if b > 0)
            print('%s: %d rows aligned; aligned E-value / swapped E-value between %.2f and %.2f' % (tag, len(both), ratio[0], ratio[-1]))
            assert ratio[0] != 1.0 or ratio[-1] != 1.0, 'the two E-values do not differ'
            e_hi = 0.001
            kept_hi = {ks: ab for ks, ab in both.items() if ab[0] <= e_hi * 0.99}
            assert all(not (e_hi * 0.99 < ab[0] < e_hi * 1.01) for ab in both.values()), 'an aligned E-value too close to E[0]'
            assert all(b <= e_hi * 0.99 for _, b in kept_hi.values()), 'E[0] removes a row in the second swap'
            # E[1]: the largest threshold between two neighbouring E-values that lies in no row's [swapped, aligned) interval, removes a
            # kept row in the second swap and empties a query's entry by it
            marks = sorted(set(v for ab in kept_hi.values() for v in ab if v > 0))
            e_lo = None
            for lo, hi in reversed(list(zip(marks[:-1], marks[1:]))):
                if hi / lo < 1.1:
                    continue
                e = float('%.3E' % ((lo * hi) ** 0.5))
                if not lo * 1.02 < e < hi / 1.02:
                    continue
                if any(b <= e < a for a, b in kept_hi.values()):
                    continue
                removed = [ks for ks, ab in kept_hi.items() if ab[1] > e]
                left = set(s for (_, s), ab in kept_hi.items() if ab[1] <= e)
                emptied = set(s for _, s in removed) - left
                if removed and emptied:
                    e_lo = e
                    break
            assert e_lo is not None, 'no threshold shows the second branch'
            aln_swapped = align(e_hi)
            final = [run_driver(exe, tmp, sorted(aln_swapped.items()), prof_residues, range(n_q), e) for e in (e_hi, e_lo)]
            n_aln = sum(t.count(b'\n') for t in aln_swapped.values())
            n_fin = [sum(t.count(b'\n') for t in f.values()) for f in final]
            assert n_aln == len(kept_hi) == n_fin[0] and n_fin[1] == n_aln - len(removed) and n_fin[1] > 0
            assert all(sorted(f) == list(range(n_q)) for f in final)
            assert all(final[1][s] == b'' and final[0][s] != b'' for s in emptied)
            print('%s: %d prefilter rows, %d aligned at -e %g; second swap keeps %d at -e %g and %d at -e %g (%d queries emptied)'
                  % (tag, n_rows, n_aln, e_hi, n_fin[0], e_hi, n_fin[1], e_lo, len(emptied)))
            pack(out, tag + '_pref', pref)
            pack(out, tag + '_pref_swapped', pref_swapped)
            pack(out, tag + '_aln_swapped', aln_swapped)
            pack(out, tag + '_final_0', final[0])
            pack(out, tag + '_final_1', final[1])
            out[tag + '_E'] = np.array([e_hi, e_lo])
            out[tag + '_figures'] = np.array([n_rows, n_aln, n_fin[0], n_fin[1], len(emptied)], np.int64)

        # ---- C: constructed inputs for the swap alone.  The second DB holds keys 0, 1, 3 and 7: 3 has no hits, 2 and 4 - 6 do not exist
        c_keys = [0, 1, 3, 7]
        c_pref = {0: b'1\t50\t-32768\n0\t40\t32767\n', 1: b'1\t50\t5\n7\t20\t-3\n', 2: b'1\t60\t0\n', 4: b'', 5: b'7\t20\t100\n2\t33\t-1\n1\t50\t-7\n'}
        c_residues = 40000
        pack(out, 'C_pref', c_pref)
        pack(out, 'C_pref_swapped', run_driver(exe, tmp, sorted(c_pref.items()), c_residues, c_keys, 0.001))

        def aln_line(t, bits, seqid, e, qs, qe, ql, ts, te, tl, bt=None):
            return ('%d\t%d\t%s\t%.3E\t%d\t%d\t%d\t%d\t%d\t%d' % (t, bits, seqid, e, qs, qe, ql, ts, te, tl) + ('' if bt is None else '\t' + bt) + '\n').encode()
        # equal bit scores and lengths on target 1 (the key decides), a weak row alone on key 5 (dropped: an empty entry on a key the DB
        # does not hold) and one on key 7 next to a strong one
        c_bt = {0: aln_line(1, 120, '0.345', 1e-30, 3, 90, 100, 5, 95, 110, '10M2I30M3D40M1I5M') + aln_line(0, 300, '1.00', 1e-90, 0, 99, 100, 0, 99, 100, '100M'),
                1: aln_line(1, 120, '0.099', 2e-30, 0, 80, 100, 2, 82, 110, '0M3D40M12I25M') + aln_line(7, 25, '0.250', 1.0, 10, 40, 100, 7, 37, 400, '31M'),
                2: b'',
                6: aln_line(5, 24, '0.009', 0.5, 1, 30, 100, 4, 33, 400, '12M1D17M') + aln_line(7, 200, '0.610', 1e-55, 0, 99, 100, 0, 59, 60, '30M40I30M') +
                   aln_line(1, 120, '0.500', 3e-30, 5, 85, 100, 9, 89, 110, '81M')}
        c_plain = {k: b''.join(b'\t'.join(l.split(b'\t')[:10]) + b'\n' for l in t.splitlines()) for k, t in c_bt.items()}
        out['C_E'] = np.array([1e-3])
        out['C_keys'] = np.array(c_keys, np.uint32)
        out['C_residues'] = np.int64(c_residues)
        for name, db in (('C_aln_bt', c_bt), ('C_aln_plain', c_plain)):
            sw_db = run_driver(exe, tmp, sorted(db.items()), c_residues, c_keys, 1e-3)
            assert sorted(sw_db) == [0, 1, 3, 5, 7] and sw_db[3] == b'' and sw_db[5] == b'' and sw_db[7].count(b'\n') == 1 and sw_db[1].count(b'\n') == 3
            pack(out, name, db)
            pack(out, name + '_swapped', sw_db)
        print('set C: pref_swapped keys %s; alignment swaps keys %s' % (sorted(run_driver(exe, tmp, sorted(c_pref.items()), c_residues, c_keys, 0.001)),
                                                                     [0, 1, 3, 5, 7]))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print('wrote %s (%d bytes)' % (OUT, size))
    assert size < 100 * 1024


if __name__ == '__main__':
    main()
