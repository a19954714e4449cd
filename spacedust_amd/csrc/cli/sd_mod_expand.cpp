// expandaln <queryDB A> <targetDB C> <resultDB A->B> <resultDB B->C> <outDB> (M/src/util/expandaln.cpp:86-464 with returnAlnRes = true):
// every alignment of a query A with a B is carried over to the C's that B is aligned with -- in `clustersearch --profile-cluster-search 1`
// B is a cluster's representative profile and the C's are the members of its cluster (R/data/clustersearch.sh:69-80).  The translation
// of a pair of backtraces runs on the device (sd_expand_batch / sd_expand_backtraces, on run lists); the row logic -- which pairs
// there are, Util::canBeCovered, one kept row per C key and query, the criteria, the text -- is the host side here.
#include "sd_cli.h"

#include <omp.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <limits>
#include <unordered_set>

namespace sdcli {

namespace {

// Util::fast_atoi<int> (M/src/commons/Util.h:107-121): an optional '-', digits, no range check
inline int32_t exAtoi(const char *p, const char *e) {
    bool neg = false;
    if (p < e && *p == '-') {
        neg = true;
        p++;
    }
    uint32_t v = 0;
    for (; p < e && *p >= '0' && *p <= '9'; p++) v = v * 10u + (uint32_t) (*p - '0');
    return (int32_t) (neg ? 0u - v : v);
}

// SmithWaterman::computeCov (StripedSmithWaterman.cpp:1671-1673)
inline float exCov(unsigned start, unsigned end, unsigned len) {
    return (std::min(len, std::max(start, end)) - std::min(start, end) + 1) / (float) len;
}
// Util::hasCoverage (Util.cpp:496-511): mode 0 both, 1 target, 2 query
inline bool exHasCov(float thr, int mode, float qCov, float tCov) {
    switch (mode) {
        case 0: return qCov >= thr && tCov >= thr;
        case 1: return tCov >= thr;
        case 2: return qCov >= thr;
        default: return true;
    }
}
// Util::fastSeqIdToBuffer as Matcher::resultToBuffer leaves it (Util.cpp:222-251, Matcher.cpp:286-287): truncated to three digits, and
// "1.00" for an identity of one (the separator lands on the last zero)
inline char *exSeqIdText(float seqId, char *p) {
    if (seqId == 1.0f) {
        memcpy(p, "1.00", 4);
        return p + 4;
    }
    *p++ = '0';
    *p++ = '.';
    if (seqId < 0.10) *p++ = '0';
    if (seqId < 0.01) *p++ = '0';
    return p + snprintf(p, 16, "%d", (int) (seqId * 1000));
}

// One alignment row of a result DB (Matcher::parseAlignmentRecord, Matcher.cpp:203-277).  Returns 0, or 1 for a line with fewer than
// ten columns, 2 for one without a backtrace column, 3 for a backtrace that is not run-length M / I / D text.
struct ExRow {
    uint32_t dbKey;
    int32_t score, qStart, qEnd, qLen, dbStart, dbEnd, dbLen;
    float seqId;
    double eval;
};
int exParseRow(const char *ls, const char *le, ExRow &r, std::vector<uint32_t> &runs) {
    const char *col[12];
    uint32_t n = 0;
    col[n++] = ls;
    for (const char *c = ls; c < le && n < 12; c++)
        if (*c == '\t') col[n++] = c + 1;
    if (n < 10) return 1;
    if (n < 11) return 2;
    r.dbKey = (uint32_t) exAtoi(col[0], le);
    r.score = exAtoi(col[1], le);
    r.seqId = (float) strtod(col[2], nullptr);
    r.eval = strtod(col[3], nullptr);
    r.qStart = exAtoi(col[4], le);
    r.qEnd = exAtoi(col[5], le);
    r.qLen = exAtoi(col[6], le);
    r.dbStart = exAtoi(col[7], le);
    r.dbEnd = exAtoi(col[8], le);
    r.dbLen = exAtoi(col[9], le);
    // Matcher::uncompressAlignment (:187-201): a count of 0 is one column
    const char *e = n == 12 ? col[11] - 1 : le;
    uint64_t count = 0;
    bool any = false;
    for (const char *c = col[10]; c < e; c++) {
        if (*c >= '0' && *c <= '9') {
            count = count * 10 + (uint64_t) (*c - '0');
            if (count >= (1u << 30)) return 3;
        } else {
            const uint32_t st = *c == 'M' ? 0u : *c == 'I' ? 1u : *c == 'D' ? 2u : 3u;
            if (st == 3u) return 3;
            const uint32_t len = count == 0 ? 1u : (uint32_t) count;
            // (neighbouring runs of one state stay two runs: the translation sees columns, not run boundaries)
            runs.push_back((len << 2) | st);
            count = 0;
            any = true;
        }
    }
    return any ? 0 : 2;
}

template <typename F>
inline bool exForLines(const char *p, F fn) {
    while (*p != '\0') {
        const char *le = p;
        while (*le != '\0' && *le != '\n') le++;
        if (le > p && !fn(p, le)) return false;
        p = *le == '\n' ? le + 1 : le;
    }
    return true;
}

const char *exRowError(int rc) {
    return rc == 1 ? "Invalid alignment result record" : rc == 2 ? "Alignment must contain a backtrace" : "Invalid alignment state";
}

// the rows of a range of entries as flat arrays; entry e holds the rows rowOff[e] .. rowOff[e + 1]
struct ExRows {
    std::vector<uint64_t> rowOff, runOff;
    std::vector<ExRow> rows;
    std::vector<uint32_t> runs;
    int parse(const sddb::Reader &rd, size_t first, size_t last) {
        const size_t n = last - first;
        std::vector<std::vector<ExRow> > pr(n);
        std::vector<std::vector<uint32_t> > pu(n);
        std::vector<std::vector<uint32_t> > pn(n);   // runs per row
        int bad = 0;
#pragma omp parallel for schedule(dynamic, 16)
        for (size_t i = 0; i < n; i++) {
            exForLines(rd.data(first + i), [&](const char *ls, const char *le) {
                ExRow r;
                const size_t before = pu[i].size();
                const int rc = exParseRow(ls, le, r, pu[i]);
                if (rc != 0) {
#pragma omp atomic write
                    bad = rc;
                    return false;
                }
                pr[i].push_back(r);
                pn[i].push_back((uint32_t) (pu[i].size() - before));
                return true;
            });
        }
        if (bad) return bad;
        rowOff.assign(n + 1, 0);
        std::vector<uint64_t> runBase(n + 1, 0);
        for (size_t i = 0; i < n; i++) {
            rowOff[i + 1] = rowOff[i] + pr[i].size();
            runBase[i + 1] = runBase[i] + pu[i].size();
        }
        rows.resize(rowOff[n]);
        runs.resize(runBase[n]);
        runOff.assign(rowOff[n] + 1, 0);
#pragma omp parallel for schedule(dynamic, 16)
        for (size_t i = 0; i < n; i++) {
            uint64_t at = runBase[i];
            for (size_t x = 0; x < pr[i].size(); x++) {
                rows[rowOff[i] + x] = pr[i][x];
                runOff[rowOff[i] + x] = at;
                at += pn[i][x];
            }
            if (!pu[i].empty()) memcpy(&runs[runBase[i]], pu[i].data(), pu[i].size() * sizeof(uint32_t));
        }
        runOff[rowOff[n]] = runBase[n];
        return 0;
    }
};

double exNow() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

int expandalnModule(const Args &a) {
    if (a.pos.size() != 5) return fail("usage: expandaln <queryDB> <targetDB> <resultDB_AB> <resultDB_BC> <outDB> [options]");
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    if (a.integer("--expand-filter-clusters", 0) != 0)
        return fail("--expand-filter-clusters 1 (the MSA filter of every cluster before it is expanded) is not implemented");
    const int mode = (int) a.integer("--expansion-mode", 0);
    const int aType = sddb::baseType(sddb::readDbType(a.pos[0])), cType = sddb::baseType(sddb::readDbType(a.pos[1]));
    if (cType == sddb::DBTYPE_INDEX_DB) return fail("an index DB as <targetDB> is not implemented: pass the sequence DB and its alignment DB");
    if (aType == sddb::DBTYPE_HMM_PROFILE && cType == sddb::DBTYPE_HMM_PROFILE) return fail("Profile-profile is currently not supported");
    if (mode != 0 && mode != 1) return fail("--expansion-mode " + std::to_string(mode) + ": 0 and 1 are implemented");
    const bool compBias = a.integer("--comp-bias-corr", 1) != 0;
    const int seqIdMode = (int) a.integer("--seq-id-mode", 0);
    if (mode == 1) {
        if (aType == sddb::DBTYPE_HMM_PROFILE || cType == sddb::DBTYPE_HMM_PROFILE)
            return fail("--expansion-mode 1 with a profile database is not implemented");
        if (int rc = checkCommon(a)) return rc;   // another --sub-mat
        const int gapOpen = atoi(a.multi("--gap-open", "aa", "11").c_str()), gapExtend = atoi(a.multi("--gap-extend", "aa", "1").c_str());
        if (gapOpen != 11 || gapExtend != 1)
            return fail("gap costs other than --gap-open 11 --gap-extend 1 need other E-value parameters than the built-in preset");
        if (compBias && a.real("--comp-bias-corr-scale", 1.0) != 1.0) return fail("--comp-bias-corr-scale other than 1 is not implemented");
    }
    const double evalThr = a.real("-e", 0.001);
    const float covThr = (float) a.real("-c", 0.0), seqIdThr = (float) a.real("--min-seq-id", 0.0);
    const int covMode = (int) a.integer("--cov-mode", 0), alnLenThr = (int) a.integer("--min-aln-len", 0);
    // pairs per device call (whole AB entries; an entry with more pairs goes alone)
    uint64_t pairBudget = 4000000;
    if (const char *e = getenv("SD_EXPAND_PAIRS")) pairBudget = std::max<uint64_t>(1, strtoull(e, nullptr, 10));

    Lap lap("expandaln");
    double tParse = 0, tDevice = 0, tSelect = 0, tPrint = 0, t0 = exNow();
    std::string err;
    sddb::Reader ab, bc;
    if (!ab.open(a.pos[2], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    if (!bc.open(a.pos[3], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::NOSORT, &err)) return fail(err);
    ExRows B;
    if (int rc = B.parse(bc, 0, bc.size())) return fail(std::string(exRowError(rc)) + " (" + a.pos[3] + ")");
    if (bc.size() >= UINT32_MAX || B.rows.size() >= UINT32_MAX) return fail("more than 2^32 - 1 entries or rows in " + a.pos[3]);
    std::vector<int32_t> bcStartB(B.rows.size()), bcStartC(B.rows.size());
    for (size_t i = 0; i < B.rows.size(); i++) {
        bcStartB[i] = B.rows[i].qStart;
        bcStartC[i] = B.rows[i].dbStart;
    }
    tParse += exNow() - t0;
    lap.mark("open + parse BC");

    CtxH ctx;
    int rc = ctx.open(deviceOf(a));
    if (rc != SD_OK) return failNoDevice(rc);
    // mode 1: both sequence DBs on the device, the queries with their rounded composition bias (expandaln.cpp:246-255)
    HostH host;
    SeqDb aDb, cDb;
    SeqSetH aSet, cSet;
    std::vector<uint32_t> bcTarget;
    if (mode == 1) {
        if (host.open(threadsOf(a)) != SD_OK) return fail("sd_host_create failed");
        if (!aDb.load(a.pos[0], host.h, &err) || !cDb.load(a.pos[1], host.h, &err)) return fail(err);
        std::vector<int8_t> bias;
        if (compBias) {
            bias.resize(aDb.totalResidues() + 1);
            sd_host_sw_comp_bias(host.h, 0, aDb.residues.data(), aDb.offsets.data(), aDb.n, bias.data());
        }
        rc = sd_seqset_create(ctx.c, aDb.residues.data(), aDb.offsets.data(), aDb.n, compBias ? bias.data() : nullptr, &aSet.s);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create(queries)");
        rc = sd_seqset_create(ctx.c, cDb.residues.data(), cDb.offsets.data(), cDb.n, nullptr, &cSet.s);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create(targets)");
        bcTarget.resize(B.rows.size());
        for (size_t i = 0; i < B.rows.size(); i++) {
            const size_t id = cDb.rd.idOfKey(B.rows[i].dbKey);
            if (id == SIZE_MAX) return fail("Invalid database read for key " + std::to_string(B.rows[i].dbKey) + " (" + a.pos[1] + ")");
            bcTarget[i] = (uint32_t) id;
        }
    }
    const uint64_t cResidues = mode == 1 ? cDb.totalResidues() : 0;   // cReader->getAminoAcidDBSize() (:169)
    const bool timing = getenv("SD_DEBUG_TIMING") != nullptr;
    if (timing) sd_profile_enable(ctx.c, 1);
    sddb::Writer out;
    if (!out.open(a.pos[4], sddb::withExtended(sddb::DBTYPE_ALIGNMENT_RES, sddb::EXT_INDEX_NEED_SRC), &err)) return fail(err);

    // a failure from here on leaves no half-written DB behind
    struct RemoveOut {
        std::string db;
        bool on = true;
        ~RemoveOut() { if (on) sddb::removeDb(db); }
    } removeOut{a.pos[4]};
    sd_expand_params par;
    memset(&par, 0, sizeof(par));
    par.mode = mode;
    par.gapOpen = 11;
    par.gapExtend = 1;
    if (mode == 1) sd_host_matrix(host.h, 0, par.matrix, nullptr, nullptr);
    uint64_t leftSequence = 0;
    std::vector<uint32_t> abQuery;
    std::vector<double> evalOf;
    std::vector<int32_t> bitsOf;
    std::vector<float> seqIdOf;
    const size_t nEntries = ab.size();
    const bool warn = a.integer("-v", 3) >= 2;
    uint64_t pairsTotal = 0, keptTotal = 0, missing = 0, runsRead = 0, bytesWritten = 0, calls = 0;
    std::vector<sd_expand_result> rec;
    std::vector<uint32_t> cluster;
    std::vector<int32_t> abStartA, abStartB;
    std::vector<uint64_t> kept, keptOff, poolOff;
    std::vector<char> pool;
    std::vector<std::string> text;
    // the pairs of an entry need its rows parsed: entries are taken a block at a time and cut into calls by their pair counts
    const size_t BLOCK = 4096;
    for (size_t e0 = 0; e0 < nEntries; e0 += BLOCK) {
        const size_t e1 = std::min(nEntries, e0 + BLOCK), nE = e1 - e0;
        t0 = exNow();
        ExRows A;
        if (int prc = A.parse(ab, e0, e1)) return fail(std::string(exRowError(prc)) + " (" + a.pos[2] + ")");
        const size_t nRows = A.rows.size();
        cluster.assign(nRows, UINT32_MAX);
        std::vector<uint64_t> rowPairs(nRows, 0);
        for (size_t i = 0; i < nRows; i++) {
            const size_t id = bc.idOfKey(A.rows[i].dbKey);
            if (id == SIZE_MAX) {   // expandaln.cpp:270-274
                if (warn) fprintf(stderr, "Missing alignments for sequence %u\n", A.rows[i].dbKey);
                missing++;
                continue;
            }
            cluster[i] = (uint32_t) id;
            rowPairs[i] = B.rowOff[id + 1] - B.rowOff[id];
        }
        tParse += exNow() - t0;
        size_t c0 = 0;   // first entry (inside the block) of the next call
        while (c0 < nE) {
            size_t c1 = c0;
            uint64_t pairs = 0;
            while (c1 < nE) {
                uint64_t ep = 0;
                for (uint64_t r = A.rowOff[c1]; r < A.rowOff[c1 + 1]; r++) ep += rowPairs[r];
                if (c1 > c0 && pairs + ep > pairBudget) break;
                pairs += ep;
                c1++;
            }
            // the rows of entries c0 .. c1 as a call of their own: run offsets relative to the first row
            t0 = exNow();
            const uint64_t r0 = A.rowOff[c0], r1 = A.rowOff[c1], nR = r1 - r0;
            std::vector<uint64_t> runOff(nR + 1);
            for (uint64_t r = 0; r <= nR; r++) runOff[r] = A.runOff[r0 + r] - A.runOff[r0];
            abStartA.resize(nR);
            abStartB.resize(nR);
            for (uint64_t r = 0; r < nR; r++) {
                abStartA[r] = A.rows[r0 + r].qStart;
                abStartB[r] = A.rows[r0 + r].dbStart;
            }
            rec.resize(pairs);
            if (mode == 1) {
                abQuery.resize(nR);
                for (size_t e = c0; e < c1; e++) {
                    const size_t id = aDb.rd.idOfKey(ab.key(e0 + e));
                    if (id == SIZE_MAX) return fail("Invalid database read for key " + std::to_string(ab.key(e0 + e)) + " (" + a.pos[0] + ")");
                    for (uint64_t r = A.rowOff[e]; r < A.rowOff[e + 1]; r++) abQuery[r - r0] = (uint32_t) id;
                }
                evalOf.assign(pairs, 0.0);
                bitsOf.assign(pairs, 0);
                seqIdOf.assign(pairs, 0.0f);
            }
            uint64_t got = 0;
            if (nR) {
                rc = sd_expand_batch(ctx.c, &par, (uint32_t) nR, abStartA.data(), abStartB.data(), runOff.data(), A.runs.data() + A.runOff[r0],
                                     cluster.data() + r0, (uint32_t) bc.size(), B.rowOff.data(), bcStartB.data(), bcStartC.data(), B.runOff.data(),
                                     B.runs.data(), aSet.s, cSet.s, mode == 1 ? abQuery.data() : nullptr, mode == 1 ? bcTarget.data() : nullptr, pairs,
                                     rec.data(), &got);
                if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_expand_batch");
                if (got != pairs) return fail("sd_expand_batch returned another pair count than the rows give");
            }
            tDevice += exNow() - t0;
            t0 = exNow();
            // the selection of expandaln.cpp:318-377 per entry, in row order; the pairs of an entry are contiguous
            const size_t nC = c1 - c0;
            std::vector<uint64_t> firstPair(nC + 1, 0);
            for (size_t e = 0; e < nC; e++) {
                uint64_t ep = 0;
                for (uint64_t r = A.rowOff[c0 + e]; r < A.rowOff[c0 + e + 1]; r++) ep += rowPairs[r];
                firstPair[e + 1] = firstPair[e] + ep;
            }
            std::vector<std::vector<uint64_t> > keptOf(nC);
            uint64_t left = 0;
#pragma omp parallel reduction(+ : left)
            {
                std::unordered_set<uint32_t> seen;
#pragma omp for schedule(dynamic, 16)
                for (size_t e = 0; e < nC; e++) {
                    seen.clear();
                    for (uint64_t p = firstPair[e]; p < firstPair[e + 1]; p++) {
                        const sd_expand_result &x = rec[p];
                        if (x.btLen == 0) continue;
                        const ExRow &rab = A.rows[r0 + x.abRow], &rbc = B.rows[x.bcRow];
                        if (!sd_host_can_be_covered(covThr, covMode, (float) rab.qLen, (float) rbc.dbLen)) continue;
                        // a C key that has a kept row in this query takes no other, overlapping or not (:329-334)
                        if (seen.count(rbc.dbKey)) continue;
                        const float qCov = exCov((unsigned) x.aStart, (unsigned) x.aEnd, (unsigned) rab.qLen);
                        const float tCov = exCov((unsigned) x.cStart, (unsigned) x.cEnd, (unsigned) rbc.dbLen);
                        const bool hasCov = exHasCov(covThr, covMode, qCov, tCov);
                        float seqId = rab.seqId;
                        double eval = rab.eval;
                        if (mode == 1) {
                            // a walk that leaves a sequence has no reference row (the reference reads stale memory): dropped and counted
                            if (x.flags & SD_EXPAND_LEAVES_SEQUENCE) {
                                left++;
                                continue;
                            }
                            if (x.rawScore < -6) continue;   // "alignment too bad" (:346-348)
                            const int aLen = aDb.lens[abQuery[x.abRow]], cLen = cDb.lens[bcTarget[x.bcRow]];
                            eval = sd_host_evalue(cResidues, (double) x.rawScore, (double) aLen);
                            bitsOf[p] = static_cast<int>(sd_host_bitscore((double) x.rawScore) + 0.5);
                            switch (seqIdMode) {   // Util::computeSeqId (Util.cpp:532-542)
                                case 0: seqId = static_cast<float>(x.identities) / static_cast<float>(x.btLen); break;
                                case 1: seqId = static_cast<float>(x.identities) / static_cast<float>(std::min(aLen, cLen)); break;
                                case 2: seqId = static_cast<float>(x.identities) / static_cast<float>(std::max(aLen, cLen)); break;
                                default: seqId = 0.0f; break;
                            }
                            evalOf[p] = eval;
                            seqIdOf[p] = seqId;
                        }
                        const bool hasSeqId = seqId >= (seqIdThr - std::numeric_limits<float>::epsilon());
                        const bool hasEvalue = eval <= evalThr;
                        // BC's alignment length (translateResult carries it over, BacktraceTranslator.h:145)
                        const int alnLen = std::max(std::abs(rbc.qEnd - (rbc.qStart == -1 ? 0 : rbc.qStart)), std::abs(rbc.dbEnd - (rbc.dbStart == -1 ? 0 : rbc.dbStart))) + 1;
                        if (hasCov && hasSeqId && hasEvalue && alnLen >= alnLenThr) {
                            keptOf[e].push_back(p);
                            seen.insert(rbc.dbKey);
                        }
                    }
                }
            }
            leftSequence += left;
            keptOff.assign(nC + 1, 0);
            for (size_t e = 0; e < nC; e++) keptOff[e + 1] = keptOff[e] + keptOf[e].size();
            kept.resize(keptOff[nC]);
            for (size_t e = 0; e < nC; e++)
                if (!keptOf[e].empty()) memcpy(&kept[keptOff[e]], keptOf[e].data(), keptOf[e].size() * sizeof(uint64_t));
            tSelect += exNow() - t0;
            t0 = exNow();
            uint64_t poolBytes = 0;
            for (const uint64_t p : kept) poolBytes += (uint64_t) rec[p].textLen;
            pool.resize(poolBytes + 1);
            poolOff.assign(kept.size() + 1, 0);
            rc = sd_expand_backtraces(ctx.c, kept.size(), kept.data(), pool.data(), pool.size(), poolOff.data());
            if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_expand_backtraces");
            tDevice += exNow() - t0;
            if (timing && nR) {
                uint64_t p = 0, r = 0, w = 0;
                sd_expand_last_stats(ctx.c, &p, &r, &w);
                runsRead += r;
                bytesWritten += w;
                calls++;
            }
            t0 = exNow();
            if (text.size() < nC) text.resize(nC);
#pragma omp parallel for schedule(dynamic, 16)
            for (size_t e = 0; e < nC; e++) {
                std::string &s = text[e];
                s.clear();
                char head[256], ev[32];
                double evBack;
                for (uint64_t k = keptOff[e]; k < keptOff[e + 1]; k++) {
                    const sd_expand_result &x = rec[kept[k]];
                    const ExRow &rab = A.rows[r0 + x.abRow], &rbc = B.rows[x.bcRow];
                    // Matcher::resultToBuffer (Matcher.cpp:280-327): score, identity and E-value are AB's (expandaln.cpp:353-355)
                    char *p = head + snprintf(head, 32, "%u\t%d\t", rbc.dbKey, mode == 1 ? bitsOf[kept[k]] : rab.score);
                    p = exSeqIdText(mode == 1 ? seqIdOf[kept[k]] : rab.seqId, p);
                    if (mode == 1) snprintf(ev, sizeof(ev), "%.3E", evalOf[kept[k]]);
                    else sd_host_quantise_3e(rab.eval, ev, &evBack);
                    p += snprintf(p, 160, "\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t", ev, x.aStart, x.aEnd, rab.qLen, x.cStart, x.cEnd, rbc.dbLen);
                    s.append(head, (size_t) (p - head));
                    s.append(pool.data() + poolOff[k], (size_t) (poolOff[k + 1] - poolOff[k]));
                    s.push_back('\n');
                }
            }
            for (size_t e = 0; e < nC; e++)
                if (!out.write(ab.key(e0 + c0 + e), text[e].data(), text[e].size())) return fail("cannot write " + a.pos[4]);
            tPrint += exNow() - t0;
            pairsTotal += pairs;
            keptTotal += kept.size();
            c0 = c1;
        }
    }
    if (!out.close(&err)) return fail(err);
    removeOut.on = false;
    if (leftSequence && a.integer("-v", 3) >= 2)
        fprintf(stderr, "expandaln: %llu pairs dropped: the walk along their backtrace leaves a sequence (the reference reads outside it there)\n",
                (unsigned long long) leftSequence);
    lap.mark("expand");
    if (timing) {
        // the device share: host -> device copies of the run lists, the two kernels, the records and the text back
        double ms1 = 0, ms2 = 0;
        uint64_t n1 = 0, n2 = 0;
        sd_synchronize(ctx.c);
        sd_profile_get(ctx.c, "expand_records", &ms1, &n1);
        sd_profile_get(ctx.c, "expand_text", &ms2, &n2);
        fprintf(stderr, "[expandaln] parse %.3f s, device %.3f s, select %.3f s, print %.3f s\n", tParse, tDevice, tSelect, tPrint);
        fprintf(stderr, "[expandaln] %llu calls, %llu pairs, %llu kept; kernels: expand_records %.3f ms, expand_text %.3f ms; %llu runs read, %llu bytes written\n",
                (unsigned long long) calls, (unsigned long long) pairsTotal, (unsigned long long) keptTotal, ms1, ms2, (unsigned long long) runsRead,
                (unsigned long long) bytesWritten);
    }
    info(a, "%zu entries, %llu pairs translated, %llu rows kept (%llu rows on a B without alignments)\n", nEntries, (unsigned long long) pairsTotal,
         (unsigned long long) keptTotal, (unsigned long long) missing);
    return 0;
}

}  // namespace sdcli
