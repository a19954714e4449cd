// prefilter <queryDB> <targetDB> <resultDB>          (M/src/prefiltering/Main.cpp:13, Prefiltering.cpp:570-951), its --split plan and target
// split, and ungappedprefilter <queryDB> <targetDB> <resultDB>.  DB in, C ABI of libsdgpu.so (HIP kernels) in the middle, DB out.  No
// compute here, no CPU fallback: without a GPU sd_ctx_create fails and the module exits non-zero.
#include "sd_pref_core.h"
#include "../host/sd_target_build.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace sdcli {

// ---------------------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------------------
// --split / --split-mode / --split-memory-limit (Prefiltering::setupSplit, Prefiltering.cpp:273-377).  The reference decides by host
// RAM; here the memory that matters is the device's: sd_target_footprint against --split-memory-limit or 0.9 x the free device memory.
namespace {

// ByteParser::parse (M/src/commons/ByteParser.cpp): digits with an optional B / K / M / G / T suffix, powers of 1024
bool parseBytes(const std::string &t, uint64_t &out) {
    if (t.empty()) return false;
    size_t i = 0;
    while (i < t.size() && t[i] >= '0' && t[i] <= '9') i++;
    if (i == 0 || t.size() - i > 1) return false;
    uint64_t v = strtoull(t.substr(0, i).c_str(), nullptr, 10), mul = 1ull << 20;   // no suffix: megabytes, as ByteParser reads it
    if (i < t.size()) {
        switch (t[i]) {
            case 'b': case 'B': mul = 1; break;
            case 'k': case 'K': mul = 1ull << 10; break;
            case 'm': case 'M': mul = 1ull << 20; break;
            case 'g': case 'G': mul = 1ull << 30; break;
            case 't': case 'T': mul = 1ull << 40; break;
            default: return false;
        }
    }
    out = v * mul;
    return true;
}

std::string formatBytes(uint64_t b) {   // ByteParser::format: the largest unit that leaves a value >= 1
    static const char unit[] = {'B', 'K', 'M', 'G', 'T'};
    int u = 0;
    uint64_t v = b;
    while (u < 4 && v >= 1024) {
        v /= 1024;
        u++;
    }
    return v ? std::to_string(v) + unit[u] : "0";
}

}  // namespace

int resolveSplit(const Args &a, const sddb::Reader &target, uint64_t residues, uint64_t nQueries, sd_ctx *ctx, bool residentTarget, SplitPlan &p) {
    const long long split = a.integer("--split", 0), mode = a.integer("--split-mode", 2);
    if (split < 0) return fail("--split " + std::to_string(split) + ": a number of splits, or 0 to choose it from the device memory");
    if (mode < 0 || mode > 2) return fail("Invalid split mode: " + std::to_string(mode));
    const uint64_t nSeq = target.size();
    const int kArg = (int) a.integer("-k", 0);
    // DBReader::index is in key order: the plan sums the length column in that order (DBReader.cpp:1243-1250)
    std::vector<uint64_t> lengths(nSeq);
    {
        std::vector<std::pair<uint32_t, uint32_t> > byKey(nSeq);
        for (uint64_t i = 0; i < nSeq; i++) byKey[i] = std::make_pair(target.key(i), (uint32_t) i);
        std::sort(byKey.begin(), byKey.end());
        for (uint64_t i = 0; i < nSeq; i++) lengths[i] = target.entryLength(byKey[i].second);
    }
    const uint64_t maxSeqs = (uint64_t) std::max<long long>(0, a.integer("--max-seqs", 300));
    auto planFor = [&](uint32_t n) -> int {
        p.from.assign(n, 0);
        p.size.assign(n, 0);
        return sd_host_split_plan(lengths.data(), nSeq, n, maxSeqs, kArg, residues, p.from.data(), p.size.data(), &p.listLen, &p.k);
    };
    // the largest per-split footprint of an n-way target split (residues of a split: its length column minus the "\n\0" per entry)
    std::vector<uint64_t> cum(nSeq + 1, 0);
    for (uint64_t i = 0; i < nSeq; i++) cum[i + 1] = cum[i] + (lengths[i] >= 2 ? lengths[i] - 2 : 0);
    auto footprintFor = [&](uint32_t n, uint64_t &bytes) -> int {
        if (int rc = planFor(n)) return rc;
        bytes = 0;
        for (uint32_t s = 0; s < n; s++)
            if (p.size[s]) bytes = std::max(bytes, sd_target_footprint(p.k, p.size[s], cum[p.from[s] + p.size[s]] - cum[p.from[s]]));
        return 0;
    };
    p.n = 1;
    p.target = false;
    // a k = 5 target is searched unsplit: sd_target_footprint does not model its index (it returns 0), so --split 0 has nothing to decide
    // with (it means 1) and a split the user asks for is refused
    if (kArg == 5) {
        if (split > 1) return fail("--split " + std::to_string(split) + ": a k=5 target index is searched unsplit (--split 0 or 1)");
        if (planFor(1)) return fail("sd_host_split_plan failed");
        return 0;
    }
    const bool detect = split == 0 || mode == 2;
    uint64_t limit = 0, whole = 0, perSplit = 0;
    bool fits = true;
    if (detect && !residentTarget) {
        const std::string lim = a.str("--split-memory-limit", "0");
        if (lim != "0" && !lim.empty()) {
            if (!parseBytes(lim, limit)) return fail("--split-memory-limit " + lim + ": a number with an optional B/K/M/G/T suffix");
        } else {
            sd_ctx *own = nullptr;
            if (!ctx) {
                const int rc = sd_ctx_create(deviceOf(a), &own);
                if (rc != SD_OK) return failNoDevice(rc);
            }
            uint64_t freeB = 0, totalB = 0;
            const int rc = sd_device_memory(ctx ? ctx : own, &freeB, &totalB);
            if (own) sd_ctx_destroy(own);
            if (rc != SD_OK) return fail("sd_device_memory failed (" + std::to_string(rc) + ")");
            limit = (uint64_t) (0.9 * (double) freeB);   // the reference's factor (Prefiltering.cpp:281,308)
        }
        if (footprintFor(1, whole)) return fail("sd_host_split_plan failed");
        fits = whole <= limit;
    }
    if (split > 1 && (uint64_t) split > (mode == 1 || (mode == 2 && fits) ? nQueries : nSeq))   // Prefiltering.cpp:346-349
        return fail("split was set to " + std::to_string(split) + " but the db to split has only " +
                    std::to_string(mode == 1 || (mode == 2 && fits) ? nQueries : nSeq) + " sequences. Please run with default paramerters");
    if (mode == 1 && !fits)   // :282-286
        return fail("--split-mode was set to query-split (1) but memory limit requires target-split. Please use a device with more memory or run "
                    "with default --split-mode setting.");
    if (split == 0) {
        if (!fits) {
            // the smallest N whose largest split fits.  No split is smaller than one sequence, so a limit below that footprint ends the
            // search before it starts; otherwise the loop ends at N = nSeq at the latest (in practice near whole / limit)
            const int kMin = kArg ? kArg : 6;
            uint32_t n = 0;
            if (sd_target_footprint(kMin, 1, 1) <= limit)
                for (uint32_t c = 2; c <= nSeq; c++) {
                    uint64_t b = 0;
                    if (footprintFor(c, b)) return fail("sd_host_split_plan failed");
                    if (b <= limit) {
                        n = c;
                        perSplit = b;
                        break;
                    }
                }
            if (n == 0) return fail("Cannot fit databases into " + formatBytes(limit) + ". Please use a device with more memory.");
            p.n = (int) n;
            p.target = true;
        }
    } else {
        p.n = (int) split;
        p.target = split > 1 && (mode == 0 || (mode == 2 && !fits));
        if (p.target && detect && !residentTarget && footprintFor((uint32_t) split, perSplit)) return fail("sd_host_split_plan failed");
    }
    // the automatic k-mer size follows the number of splits in either mode (:351-354); the list length shrinks in a target split only
    if (planFor((uint32_t) p.n)) return fail("split was set to " + std::to_string(p.n) + ": more splits than the target DB has bytes");
    if (!p.target) {
        const int k = p.k;
        planFor(1);
        p.k = k;
    }
    if (p.n > 1) info(a, "%s split mode. Searching through %d splits\n", p.target ? "Target" : "Query", p.n);
    if (detect && !residentTarget)
        info(a, "Estimated device memory of the target index: %s per split (limit %s)\n",
             formatBytes(p.target ? perSplit : whole).c_str(), formatBytes(limit).c_str());
    return 0;
}

int prefilterSetupFromArgs(const Args &a, sd_host *host, const SeqDb &tdb, bool profileQueries, PrefSetup &s, int kOverride) {
    // parameters the way Prefiltering's constructor derives them (Prefiltering.cpp:180-215,1005-1065)
    s.k = kOverride ? kOverride : (int) a.integer("-k", 0);
    if (s.k == 0) s.k = sd_host_auto_kmer_size(tdb.totalResidues());
    if (s.k < 5 || s.k > 7) return fail("-k " + std::to_string(s.k) + ": k-mer sizes 5, 6 and 7 are implemented");
    const float sens = (float) a.real("-s", 4.0);
    const long long kScore = strtoll(a.multi("--k-score", profileQueries ? "prof" : "seq", "2147483647").c_str(), nullptr, 10);
    s.kmerThr = kScore != INT_MAX ? (int) kScore
                                  : (profileQueries ? sd_host_profile_kmer_threshold(sens, s.k) : sd_host_kmer_threshold(sens, s.k));
    s.indexThr = profileQueries ? 0 : s.kmerThr;   // profile searches index every k-mer (Prefiltering.cpp:525-527)
    s.mask = a.integer("--mask", 1) != 0;
    s.maskProb = a.real("--mask-prob", 0.9);
    s.includeIdentity = a.flag("--add-self-matches", false);
    s.compBias = a.integer("--comp-bias-corr", 1) != 0;
    sd_prefilter_params &par = s.par;
    memset(&par, 0, sizeof(par));
    par.kmerSize = s.k;
    par.kmerThr = s.kmerThr;
    par.maxHitsPerQuery = (int32_t) std::min<long long>(a.integer("--max-seqs", 300), tdb.n);   // Prefiltering.cpp:184
    par.minDiagScore = (int32_t) a.integer("--min-ungapped-score", 15);
    par.binSize = a.has("--bin-size") ? (uint32_t) a.integer("--bin-size", 0)
                                      : sd_host_bin_size(tdb.n, (uint64_t) a.integer("--l2-cache-size", 0));
    par.covMode = (int32_t) a.integer("--cov-mode", 0);
    par.covThr = (float) a.real("-c", 0.0);
    // the writer's coverage pre-filter only exists for these modes (Prefiltering.cpp:856-858)
    if (!(par.covMode == 0 || par.covMode == 2 || par.covMode == 5)) par.covThr = 0.0f;
    sd_host_matrix(host, 2, par.ungappedMatrix, nullptr, nullptr);
    if (par.maxHitsPerQuery < 1) par.maxHitsPerQuery = 1;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// `prefilter --split N --split-mode 0` (Prefiltering::runSplits / runSplit / mergeTargetSplits, Prefiltering.cpp:662-951, 379-479): per
// non-empty split its own index is built on the device, every query chunk is searched against it with the per-split list length, and
// the index is destroyed before the next one is built.  A query's entry is the concatenation of its per-split lists, sorted by
// hit_t::compareHitsByScoreAndId and not cut.  The per-split rows wait in host memory (12 bytes per hit) where the reference keeps them in
// one temporary DB per split.
namespace {

struct SplitRow {
    uint32_t key;
    int32_t score;
    int16_t diagonal;
};

int prefilterTargetSplit(const Args &a, sd_host *host, sd_ctx *ctx, const SeqDb &qdb, const SeqDb &tdb, bool sameDb, const PrefSetup &PS,
                         const SplitPlan &plan, Lap &lap) {
    const int k = PS.k;
    info(a, "Index table k-mer threshold: %d at k-mer size %d\n", PS.kmerThr, k);
    if (sddb::fileExists(a.pos[1] + ".idx.index")) info(a, "Index file not used: a target split builds the index of every split on the device\n");
    const uint32_t chunk = (uint32_t) std::max<long long>(1, a.integer("--chunk-queries", 16384));
    const int nSplits = plan.n;
    std::vector<std::vector<SplitRow> > rows((size_t) nSplits);             // per split: the rows of all queries, query after query
    std::vector<std::vector<uint32_t> > rowCount((size_t) nSplits);         // per split: rows of every query
    std::vector<uint8_t> failed(qdb.n, 0);
    QueryChunk qc;
    qc.printEach = true;
    std::vector<uint64_t> tOff;
    for (int sp = 0; sp < nSplits; sp++) {
        info(a, "Process prefiltering step %d of %d\n", sp + 1, nSplits);
        const uint64_t dbFrom = plan.from[sp], dbSize = plan.size[sp];
        if (dbSize == 0) continue;   // Prefiltering.cpp:736-738
        info(a, "Target db start %llu to %llu\n", (unsigned long long) (dbFrom + 1), (unsigned long long) (dbFrom + dbSize));
        // the split's sequences as a target of their own: ids relative to dbFrom
        const uint64_t t0 = tdb.offsets[dbFrom];
        tOff.resize(dbSize + 1);
        for (uint64_t i = 0; i <= dbSize; i++) tOff[i] = tdb.offsets[dbFrom + i] - t0;
        TargetH target;   // never resident: destroyed at the end of this split
        uint64_t st[2] = {0, 0};
        if (int rcB = buildTarget(host, ctx, PS, tdb.residues.data() + t0, tOff.data(), (uint32_t) dbSize, &target.t, st,
                                  "sdgpu prefilter: the index of split " + std::to_string(sp + 1) + " of " + std::to_string(nSplits) +
                                      " did not fit the device memory; raise --split or let --split 0 choose"))
            return rcB;
        info(a, "Index statistics\nEntries:          %llu\n", (unsigned long long) st[0]);
        lap.mark("split: index build");
        sd_prefilter_params par = PS.par;
        par.maxHitsPerQuery = (int32_t) std::min<uint64_t>(plan.listLen, dbSize);   // (a list holds no more rows than the split has sequences)
        // QueryMatcher is constructed with the split's dbSize (Prefiltering.cpp:797-799)
        if (!a.has("--bin-size")) par.binSize = sd_host_bin_size(dbSize, (uint64_t) a.integer("--l2-cache-size", 0));
        rowCount[sp].assign(qdb.n, 0);
        for (uint32_t c0 = 0; c0 < qdb.n; c0 += chunk) {
            const uint32_t c1 = std::min(qdb.n, c0 + chunk), nq = c1 - c0;
            const int rc = qc.run(ctx, host, target.t, par, PS, QuerySpan{&qdb, c0, &qdb, c0, nq}, tdb, sameDb, dbFrom, dbSize, failed.data() + c0,
                                  nullptr);
            const std::vector<uint32_t> &counts = qc.counts;
            if (rc != SD_OK) return failCtx(ctx, rc, "sd_prefilter_batch");
            for (uint32_t i = 0; i < nq; i++) {
                const sd_hit *row = qc.hits.data() + (size_t) i * par.maxHitsPerQuery;
                // the split's ids become ids of the whole DB, then keys (Prefiltering.cpp:848-850)
                for (uint32_t x = 0; x < counts[i]; x++)
                    rows[sp].push_back(SplitRow{tdb.keys[dbFrom + row[x].seqId], row[x].score, (int16_t) row[x].diagonal});
                rowCount[sp][c0 + i] = counts[i];
            }
        }
        lap.mark("split: query passes");
    }
    // mergeTargetSplits: per query the lists of the splits one after the other, sorted, nothing cut
    std::string err, text;
    sddb::Writer out;
    if (!out.open(a.pos[2], sddb::DBTYPE_PREFILTER_RES, &err)) return fail(err);
    std::vector<size_t> cursor((size_t) nSplits, 0);
    std::vector<SplitRow> merged;
    uint64_t totalHits = 0;
    for (uint32_t q = 0; q < qdb.n; q++) {
        merged.clear();
        for (int sp = 0; sp < nSplits; sp++) {
            if (rowCount[sp].empty()) continue;
            merged.insert(merged.end(), rows[sp].begin() + cursor[sp], rows[sp].begin() + cursor[sp] + rowCount[sp][q]);
            cursor[sp] += rowCount[sp][q];
        }
        if (failed[q]) merged.clear();   // a query one split could not compute is written empty, as in the one-index run
        std::stable_sort(merged.begin(), merged.end(), [](const SplitRow &x, const SplitRow &y) {   // hit_t::compareHitsByScoreAndId
            if (abs(x.score) != abs(y.score)) return abs(x.score) > abs(y.score);
            return x.key < y.key;
        });
        text.clear();
        for (const SplitRow &r : merged) appendPrefRow(text, r.key, r.score, r.diagonal);
        totalHits += merged.size();
        if (!out.write(qdb.keys[q], text.data(), text.size())) return fail("cannot write " + a.pos[2]);
    }
    if (!out.close(&err)) return fail(err);
    lap.mark("merge + write");
    info(a, "%llu prefilter hits written for %u queries\n", (unsigned long long) totalHits, qdb.n);
    if (qc.notComputed) return failNotComputed(qc.notComputed, "written as empty entries; every other entry is complete");
    return 0;
}

}  // namespace

int prefilterModule(const Args &a) {
    if (a.pos.size() != 3) return fail("usage: prefilter <queryDB> <targetDB> <resultDB> [options]");
    if (int rc = checkCommon(a)) return rc;
    const std::string ssm = a.multi("--seed-sub-mat", "aa", "VTML80.out");
    if (ssm != "VTML80.out") return fail("--seed-sub-mat " + ssm + ": only VTML80.out is built into this path");
    if (a.integer("--spaced-kmer-mode", 1) != 1 || a.has("--spaced-kmer-pattern"))
        return fail("only the default spaced k-mer patterns are supported (--spaced-kmer-mode 1)");
    if (a.integer("--exact-kmer-matching", 0) != 0) return fail("--exact-kmer-matching 1 is not supported");
    if (!a.flag("--diag-score", true)) return fail("--diag-score 0 is not supported");
    const long long tsm = a.integer("--target-search-mode", 0);
    if (tsm != 0 && tsm != 1) return fail("--target-search-mode " + std::to_string(tsm) + ": 0 (regular k-mer index) or 1 (similar k-mer index)");
    if (a.integer("--mask-lower-case", 0) != 0 || a.integer("--mask-n-repeat", 0) != 0)
        return fail("--mask-lower-case / --mask-n-repeat are not supported");
    if (a.multi("--alph-size", "aa", "21") != "21") return fail("--alph-size aa:21 only");
    if (a.real("--comp-bias-corr-scale", 1.0) != 1.0) return fail("--comp-bias-corr-scale 1 only");
    if (a.has("--taxon-list") && !a.str("--taxon-list", "").empty()) return fail("--taxon-list is not supported");
    const int threads = threadsOf(a);

    Lap lap("prefilter");
    HostH host;
    if (host.open(threads) != SD_OK) return fail("sd_host_create failed");
    std::string err;
    DbPair db;
    if (!db.open(a.pos[0], a.pos[1], host.h, true, false, &err)) return fail(err);
    const bool sameDb = db.sameDb;
    const SeqDb *const qdb = db.qdb, *const tdb = db.tdb.get();
    // A profile target DB (clusterdb's <target>_clu_rep_profile): its index holds the similar k-mers of every profile window and the
    // sequence queries look up their own k-mers only (Prefiltering.cpp:172-179, IndexBuilder.cpp:61-62).  Profile queries against it
    // are an error in the reference (Prefiltering.cpp:144-148).
    const bool profileTarget = tdb->profile;
    if (profileTarget && qdb->profile) return fail("Query-profiles cannot be searched against a target-profile database!");
    // --target-search-mode 1 on a sequence target: the similar k-mers of every target window go into the index (at the sequence
    // threshold, nothing masked) and the queries look up their own k-mers only (IndexBuilder.cpp:62,100; Prefiltering.cpp:176-179,525-527).
    // A profile target is that kind of index already (isProfile || targetSearchMode): the flag changes nothing there.
    const bool similarTarget = tsm == 1 && !profileTarget;
    if (similarTarget && qdb->profile)
        return fail("--target-search-mode 1 with a profile query database is not implemented (the reference allows it; the exact-lookup path "
                    "here reads query sequences)");
    // searched unsplit, as a profile target is: hundreds of index records per residue, which sd_target_footprint does not model
    if (similarTarget && a.integer("--split", 0) > 1)
        return fail("--split " + std::to_string(a.integer("--split", 0)) + ": --target-search-mode 1 searches the target unsplit (--split 0 or 1)");
    // what -k itself rules out is said before a device is asked for (an automatic size, -k 0, is judged where it is resolved, below)
    if (const int kArg = (int) a.integer("-k", 0)) {
        if (kArg < 5 || kArg > 7) return fail("-k " + std::to_string(kArg) + ": k-mer sizes 5, 6 and 7 are implemented");
        if (profileTarget && kArg == 7) return fail("-k 7: the index of a profile target is built at k=5 and k=6 only");
        if (similarTarget && kArg != 6)
            return fail("-k " + std::to_string(kArg) + ": the similar-k-mer index of --target-search-mode 1 is built at k=6 only");
        if (kArg == 5 && !profileTarget && a.integer("--split", 0) > 1)
            return fail("--split " + std::to_string(a.integer("--split", 0)) + ": a k=5 target index is searched unsplit (--split 0 or 1)");
    }
    lap.mark("load DBs");
    info(a, "Query database size: %u type: %s\nTarget database size: %u type: %s\n", qdb->n, qdb->profile ? "Profile" : "Aminoacid", tdb->n,
         profileTarget ? "Profile" : "Aminoacid");

    CtxH ctx;
    int rc = ctx.open(deviceOf(a));
    if (rc != SD_OK) return failNoDevice(rc);
    lap.mark("context");

    // --split: one index for the whole target (today's path, below) or one per target split (prefilterTargetSplit)
    SplitPlan plan;
    if (profileTarget) {
        // searched unsplit: sd_target_footprint models one index record per residue and does not describe the similar-k-mer index, so
        // --split 0 has nothing to decide with (it means 1 here) and a split the user asks for is refused
        if (a.integer("--split", 0) > 1)
            return fail("--split " + std::to_string(a.integer("--split", 0)) + ": a profile target database is searched unsplit (--split 0 or 1)");
        plan.k = (int) a.integer("-k", 0);
    } else if (similarTarget) {
        plan.k = (int) a.integer("-k", 0);   // unsplit (refused above): --split 0 means 1
    } else if (int rcP = resolveSplit(a, tdb->rd, tdb->totalResidues(), qdb->n, ctx.c, !residentTargetOf(a.pos[1], deviceOf(a)).empty(), plan)) {
        // (a workflow that holds this DB's index on this device has nothing left to decide)
        return rcP;
    }
    PrefSetup PS;
    // a profile on either side makes it a profile search: the profile threshold, -s / --k-score prof: (Prefiltering.cpp:196-202)
    if (int rcS = prefilterSetupFromArgs(a, host.h, *tdb, qdb->profile || profileTarget, PS, plan.k)) return rcS;
    if (profileTarget) {
        if (PS.k != 5 && PS.k != 6) return fail("-k " + std::to_string(PS.k) + ": the index of a profile target is built at k=5 and k=6 only");
        PS.indexThr = PS.kmerThr;   // the similar k-mers are generated at the threshold itself
        PS.mask = false;            // --mask is ignored: nothing of a profile is masked (Prefiltering.cpp:172-174)
    }
    if (similarTarget) {
        if (PS.k != 6) return fail("-k " + std::to_string(PS.k) + ": the similar-k-mer index of --target-search-mode 1 is built at k=6 only");
        PS.indexThr = PS.kmerThr;   // the sequence threshold itself (Prefiltering.cpp:525-527)
        PS.mask = false;            // --mask / --mask-prob are ignored: maskSequence is not called on this branch (IndexBuilder.cpp:120-131)
    }
    if (plan.target) return prefilterTargetSplit(a, host.h, ctx.c, *qdb, *tdb, sameDb, PS, plan, lap);
    const int k = PS.k, kmerThr = PS.kmerThr, indexThr = PS.indexThr;   // (profile searches index every k-mer: indexThr 0)
    const bool mask = PS.mask;
    const double maskProb = PS.maskProb;

    // target side: TARGET.idx when a createindex file with matching parameters lies next to the DB (PrefilteringIndexReader
    // layout, sd_mod_index.cpp), else built from the sequences (buildTarget); resident in HBM afterwards
    LoadedIndex loaded;
    std::string why;
    uint64_t nEntries = 0, maskedRes = 0;
    TargetH target;
    // a workflow's resident target of exactly this index (same DB, k, threshold, masking, device) is taken as it is
    // (the two kinds of target are different indexes: "p" in the masking field marks the similar-k-mer index of a profile DB)
    char tkey[96];
    if (profileTarget) snprintf(tkey, sizeof(tkey), "|%d|%d|p|%.6f|%d", k, indexThr, 0.0, deviceOf(a));
    else if (similarTarget) snprintf(tkey, sizeof(tkey), "|%d|%d|s|%.6f|%d", k, indexThr, 0.0, deviceOf(a));   // "s": similar k-mers of sequences
    else snprintf(tkey, sizeof(tkey), "|%d|%d|%d|%.6f|%d", k, indexThr, mask ? 1 : 0, maskProb, deviceOf(a));
    const std::string targetKey = a.pos[1] + tkey;
    if (resident().enabled && resident().targets.count(targetKey)) {
        const Resident::TargetEntry &te = resident().targets[targetKey];
        target.t = te.t;
        target.own = false;
        nEntries = te.nEntries;
        maskedRes = te.masked;
        info(a, "Target index resident from the previous module of this workflow\n");
    }
    // (createindex does not index profile DBs and writes no similar-k-mer index: no TARGET.idx to look for)
    const int got = target.t || profileTarget || similarTarget ? 1 : loadTargetIndex(a.pos[1], k, indexThr, mask ? 1 : 0, tdb->n, tdb->totalResidues(), loaded, &why);
    if (got < 0) return fail(why);
    if (got != 0 && !profileTarget && !similarTarget && sddb::fileExists(a.pos[1] + ".idx.index")) info(a, "Index file not used: %s\n", why.c_str());
    if (target.t) {
        // resident
    } else if (profileTarget) {
        uint64_t st[2] = {0, 0};
        rc = sdBuildProfileTarget(ctx.c, k, kmerThr, tdb->residues.data(), tdb->consensus.data(), tdb->sortedScore.data(), tdb->sortedIndex.data(),
                                  tdb->offsets.data(), tdb->n, &target.t, st);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_target_build_profile");
        nEntries = st[0];
    } else if (similarTarget) {
        uint64_t st[2] = {0, 0};
        rc = sdBuildSimilarTarget(host.h, ctx.c, k, kmerThr, tdb->residues.data(), tdb->offsets.data(), tdb->n, &target.t, st);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_target_build_similar");
        nEntries = st[0];
        info(a, "Target search mode 1: similar k-mers of every target window indexed, queries look up their own k-mers\n");
    } else if (got == 0) {
        nEntries = loaded.nEntries;
        info(a, "Use index %s.idx\n", a.pos[1].c_str());
        rc = sdUploadTarget(host.h, ctx.c, k, loaded.offsets.data(), loaded.blockBase.empty() ? nullptr : loaded.blockBase.data(), loaded.entrySeq.data(),
                            loaded.entryPos.data(), nEntries, loaded.masked.data(), tdb->offsets.data(), tdb->n, &target.t);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_target_create");
    } else {
        uint64_t st[2] = {0, 0};
        if (int rcB = buildTarget(host.h, ctx.c, PS, tdb->residues.data(), tdb->offsets.data(), tdb->n, &target.t, st,
                                  "sdgpu prefilter: the target index did not fit the device memory; --split 0 chooses a number of target splits "
                                  "that does, --split N --split-mode 0 sets it"))
            return rcB;
        nEntries = st[0];
        maskedRes = st[1];
    }
    info(a, "Index table k-mer threshold: %d at k-mer size %d\nIndex statistics\nEntries:          %llu\n", kmerThr, k,
         (unsigned long long) nEntries);
    if (resident().enabled && target.own) {   // stays for the next module of the workflow
        // one resident index per (DB, device): an index of the same DB with other parameters -- the sequence-threshold index of
        // iteration 0 once the profile iterations (threshold 0, a larger index) begin -- would only hold HBM until the workflow ends
        const std::string old = residentTargetOf(a.pos[1], deviceOf(a), true);
        if (!old.empty()) info(a, "Resident target index %s replaced\n", old.c_str());
        Resident::TargetEntry te;
        te.t = target.t;
        te.nEntries = nEntries;
        te.masked = maskedRes;
        resident().targets[targetKey] = te;
        target.own = false;
    }

    lap.mark("target index");
    const sd_prefilter_params par = PS.par;

    sddb::Writer out;
    if (!out.open(a.pos[2], sddb::DBTYPE_PREFILTER_RES, &err)) return fail(err);

    const uint32_t chunk = (uint32_t) std::max<long long>(1, a.integer("--chunk-queries", 16384));
    QueryChunk qc;
    qc.printEach = true;
    std::string text;
    uint64_t totalHits = 0;
    for (uint32_t c0 = 0; c0 < qdb->n; c0 += chunk) {
        const uint32_t c1 = std::min(qdb->n, c0 + chunk), nq = c1 - c0;
        rc = qc.run(ctx.c, host.h, target.t, par, PS, QuerySpan{qdb, c0, qdb, c0, nq}, *tdb, sameDb, 0, tdb->n, nullptr, nullptr);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_prefilter_batch");
        lap.mark("chunk: bias + device");
        for (uint32_t i = 0; i < nq; i++) {
            text.clear();
            const sd_hit *row = qc.hits.data() + (size_t) i * par.maxHitsPerQuery;
            for (uint32_t x = 0; x < qc.counts[i]; x++) appendPrefRow(text, tdb->keys[row[x].seqId], row[x].score, row[x].diagonal);
            totalHits += qc.counts[i];
            if (!out.write(qdb->keys[c0 + i], text.data(), text.size())) return fail("cannot write " + a.pos[2]);
        }
    }
    lap.mark("chunks: text + write");
    if (!out.close(&err)) return fail(err);
    lap.mark("close");
    info(a, "%llu prefilter hits written for %u queries\n", (unsigned long long) totalHits, qdb->n);
    if (qc.notComputed) return failNotComputed(qc.notComputed, "written as empty entries; every other entry is complete");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// ungappedprefilter <queryDB> <targetDB> <resultDB> (M/src/prefiltering/ungappedprefilter.cpp:479-562 with the parameters of
// Parameters.cpp:459-476): every query against every target with the byte-saturated ungapped scan, no k-mer index.  What
// blastp.sh calls instead of `prefilter` under --prefilter-mode 1.
int ungappedPrefilterModeCheck(const Args &a) {
    const long long mode = a.integer("--prefilter-mode", 0);
    if (mode == 2) return fail("--prefilter-mode 2 (ungapped and gapped) is not implemented");
    if (mode == 3) return fail("--prefilter-mode 3 (exhaustive) is not implemented");
    if (mode < 0 || mode > 3) return fail("--prefilter-mode " + std::to_string(mode) + ": 0 (k-mer) and 1 (ungapped) are implemented");
    return 0;
}

int ungappedprefilterModule(const Args &a) {
    if (a.pos.size() != 3) return fail("usage: ungappedprefilter <queryDB> <targetDB> <resultDB> [options]");
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    const std::string sm = a.multi("--sub-mat", "aa", "blosum62.out");
    if (sm != "blosum62.out") return fail("--sub-mat " + sm + ": only blosum62.out is built into this path");
    if (a.has("--taxon-list") && !a.str("--taxon-list", "").empty()) return fail("--taxon-list is not supported");
    if (a.integer("--gpu-server", 0) != 0) return fail("--gpu-server 1 is not supported (the module holds the GPU itself)");
    if (a.real("--comp-bias-corr-scale", 1.0) != 1.0) return fail("--comp-bias-corr-scale 1 only");
    if (int rc = ungappedPrefilterModeCheck(a)) return rc;
    // (--gpu 0 and --gpu 1 both run this path; -e and --db-load-mode are parsed and have no effect, as in the reference's mode 0)
    const bool compBias = a.integer("--comp-bias-corr", 1) != 0;
    const int threads = threadsOf(a);

    Lap lap("ungappedprefilter");
    HostH host;
    if (host.open(threads) != SD_OK) return fail("sd_host_create failed");
    std::string err;
    DbPair db;
    if (!db.open(a.pos[0], a.pos[1], host.h, true, true, &err)) return fail(err);
    const bool sameDb = db.sameDb;
    const SeqDb *const qdb = db.qdb, *const tdb = db.tdb.get();
    if (qdb->profile) return fail("profile query databases are not implemented in the ungapped prefilter");
    lap.mark("load DBs");
    info(a, "Query database size: %u type: Aminoacid\nTarget database size: %u type: Aminoacid\n", qdb->n, tdb->n);

    sd_ungapped_params par;
    memset(&par, 0, sizeof(par));
    sd_host_matrix(host.h, 0, par.matrix, nullptr, nullptr);
    par.minScore = (int32_t) a.integer("--min-ungapped-score", 15);
    par.maxHitsPerQuery = (int32_t) std::max<long long>(1, std::min<long long>(a.integer("--max-seqs", 300), tdb->n));
    par.covMode = (int32_t) a.integer("--cov-mode", 0);
    par.covThr = (float) a.real("-c", 0.0);

    CtxH ctx;
    int rc = ctx.open(deviceOf(a));
    if (rc != SD_OK) return failNoDevice(rc);
    SeqSetH ts;
    rc = sd_seqset_create(ctx.c, tdb->residues.data(), tdb->offsets.data(), tdb->n, nullptr, &ts.s);
    if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create (targets)");
    lap.mark("targets resident");

    sddb::Writer out;
    if (!out.open(a.pos[2], sddb::DBTYPE_PREFILTER_RES, &err)) return fail(err);
    const uint32_t chunk = (uint32_t) std::max<long long>(1, a.integer("--chunk-queries", 16384));
    std::vector<sd_hit> hits;
    std::vector<uint32_t> counts, ident;
    std::vector<int8_t> swBias;
    std::vector<uint64_t> off;
    std::string text;
    uint64_t totalHits = 0, cells = 0;
    for (uint32_t c0 = 0; c0 < qdb->n; c0 += chunk) {
        const uint32_t c1 = std::min(qdb->n, c0 + chunk), nq = c1 - c0;
        const uint64_t r0 = qdb->offsets[c0], r1 = qdb->offsets[c1];
        off.resize((size_t) nq + 1);
        for (uint32_t i = 0; i <= nq; i++) off[i] = qdb->offsets[c0 + i] - r0;
        // the identity pair exists for equal DB paths only: --add-self-matches is not a parameter of this module
        ident.assign(nq, UINT32_MAX);
        if (sameDb)
            for (uint32_t i = 0; i < nq; i++) ident[i] = c0 + i;
        if (compBias) {
            swBias.assign(r1 - r0 + 1, 0);
            sd_host_sw_comp_bias(host.h, 0, qdb->residues.data() + r0, off.data(), nq, swBias.data());
        }
        SeqSetH qs;
        rc = sd_seqset_create(ctx.c, qdb->residues.data() + r0, off.data(), nq, compBias ? swBias.data() : nullptr, &qs.s);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create (queries)");
        hits.resize((size_t) nq * par.maxHitsPerQuery);
        counts.assign(nq, 0);
        rc = sd_ungapped_prefilter_batch(ctx.c, &par, qs.s, ts.s, tdb->keys.data(), ident.data(), hits.data(), counts.data());
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_ungapped_prefilter_batch");
        uint64_t c = 0;
        sd_ungapped_last_cells(ctx.c, &c);
        cells += c;
        lap.mark("chunk: bias + device");
        // the prefilter row with diagonal 0 (ungappedprefilter.cpp:447-451)
        for (uint32_t i = 0; i < nq; i++) {
            text.clear();
            const sd_hit *row = hits.data() + (size_t) i * par.maxHitsPerQuery;
            for (uint32_t x = 0; x < counts[i]; x++) appendPrefRow(text, tdb->keys[row[x].seqId], row[x].score, 0);
            totalHits += counts[i];
            if (!out.write(qdb->keys[c0 + i], text.data(), text.size())) return fail("cannot write " + a.pos[2]);
        }
    }
    if (!out.close(&err)) return fail(err);
    lap.mark("chunks: text + write");
    info(a, "%llu ungapped prefilter hits written for %u queries (%llu cells)\n", (unsigned long long) totalHits, qdb->n,
         (unsigned long long) cells);
    return 0;
}

}  // namespace sdcli
