// The three hot modules behind the reference's command lines and DB files:
//   prefilter   <queryDB> <targetDB> <resultDB>             (M/src/prefiltering/Main.cpp:13, Prefiltering.cpp:570-951)
//   align       <queryDB> <targetDB> <prefDB> <alnDB>        (M/src/alignment/Main.cpp:12, Alignment.cpp:244-542)
//   clusterhits <querySetDB> <targetSetDB> <matches> <out>   (R/src/util/ClusterHits.cpp:215-511)
// DB in, C ABI of libsdgpu.so (HIP kernels) in the middle, DB out.  No compute here, no CPU fallback: without a GPU
// sd_ctx_create fails and the module exits non-zero.
#include "sd_cli.h"
#include "sd_align_core.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

namespace sdcli {

namespace {

struct HostH {
    sd_host *h = nullptr;
    bool own = true;   // false: the resident host object of a workflow (sd_cli.h)
    ~HostH() { if (h && own) sd_host_destroy(h); }
    int open(int threads) {
        if (resident().enabled) {
            h = resident().host(threads);
            own = false;
            return h ? SD_OK : SD_ENOMEM;
        }
        return sd_host_create(threads, &h);
    }
};
struct CtxH {
    sd_ctx *c = nullptr;
    bool own = true;   // false: the resident context of a workflow (sd_cli.h)
    ~CtxH() { if (c && own) sd_ctx_destroy(c); }
    // the module's context: the workflow's resident one when that is on, else its own
    int open(int device) {
        if (resident().enabled) {
            int rc = SD_OK;
            c = resident().ctx(device, &rc);
            own = false;
            return rc;
        }
        return sd_ctx_create(device, &c);
    }
};
struct SeqSetH {
    sd_seqset *s = nullptr;
    ~SeqSetH() { if (s && own) sd_seqset_destroy(s); }
    void reset() { if (s && own) sd_seqset_destroy(s); s = nullptr; }
    bool own = true;
};
struct TargetH {
    sd_target *t = nullptr;
    bool own = true;
    ~TargetH() { if (t && own) sd_target_destroy(t); }
};
struct IndexH {
    sd_host_index *ix = nullptr;
    ~IndexH() { if (ix) sd_host_index_destroy(ix); }
};

// what the modules refuse (the reference has these paths; this build does not)
int checkCommon(const Args &a) {
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    const std::string sm = a.multi("--sub-mat", "aa", "blosum62.out");
    if (sm != "blosum62.out") return fail("--sub-mat " + sm + ": only blosum62.out is built into this path");
    if (a.integer("--gpu", 0) != 0) return fail("--gpu 1 selects the reference's CUDA ungapped prefilter (a different algorithm); run without it");
    return 0;
}

int deviceOf(const Args &a) {
    if (a.has("--device")) return (int) a.integer("--device", 0);
    const char *lr = getenv("LOCAL_RANK");
    return lr ? atoi(lr) : 0;
}

}  // namespace

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
                if (rc != SD_OK) return fail("no usable HIP device (sd_ctx_create returned " + std::to_string(rc) + "); this path has no CPU fallback");
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
    if (s.k != 6 && s.k != 7) return fail("-k " + std::to_string(s.k) + ": k-mer sizes 6 and 7 are implemented");
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

// One chunk [c0, c1) of queries against one target that holds the ids [dbFrom, dbFrom + dbSize) of the target DB (the whole DB, or
// one split of it): identity ids, composition bias, the device call.  hits: row i at i * par.maxHitsPerQuery, ids relative to dbFrom.
struct QueryChunk {
    std::vector<sd_hit> hits;
    std::vector<uint32_t> counts, ident;
    std::vector<int8_t> diagBias;
    std::vector<int16_t> kmerBias;
    std::vector<uint64_t> off;
    int run(sd_ctx *ctx, sd_host *host, const sd_target *target, const sd_prefilter_params &par, const PrefSetup &PS, const SeqDb &qdb,
            const SeqDb &tdb, bool sameDb, uint32_t c0, uint32_t c1, uint64_t dbFrom, uint64_t dbSize) {
        const uint32_t nq = c1 - c0;
        const uint64_t r0 = qdb.offsets[c0], r1 = qdb.offsets[c1];
        off.resize((size_t) nq + 1);
        for (uint32_t i = 0; i <= nq; i++) off[i] = qdb.offsets[c0 + i] - r0;
        ident.resize(nq);
        for (uint32_t i = 0; i < nq; i++) {
            uint64_t id = UINT32_MAX;
            if (sameDb) id = c0 + i;
            else if (PS.includeIdentity) {
                const size_t t = tdb.rd.idOfKey(qdb.keys[c0 + i]);
                if (t != SIZE_MAX) id = t;
            }
            // only the split that holds the query's own target gets the id, relative to dbFrom (Prefiltering.cpp:824-837)
            ident[i] = id != UINT32_MAX && id >= dbFrom && id < dbFrom + dbSize ? (uint32_t) (id - dbFrom) : UINT32_MAX;
        }
        hits.resize((size_t) nq * par.maxHitsPerQuery);
        counts.assign(nq, 0);
        if (qdb.profile)
            return sd_prefilter_profile_batch(ctx, target, &par, nq, qdb.residues.data() + r0, off.data(), qdb.sortedScore.data() + r0 * 20,
                                              qdb.sortedIndex.data() + r0 * 20, qdb.alnProfile.data() + r0 * 21, ident.data(), hits.data(),
                                              counts.data(), nullptr);
        diagBias.assign(r1 - r0 + 1, 0);
        kmerBias.assign(r1 - r0 + 1, 0);
        if (PS.compBias) sd_host_comp_bias(host, qdb.residues.data() + r0, off.data(), nq, PS.k, nullptr, diagBias.data(), kmerBias.data());
        return sd_prefilter_batch(ctx, target, &par, nq, qdb.residues.data() + r0, off.data(), kmerBias.data(), diagBias.data(), ident.data(),
                                  hits.data(), counts.data(), nullptr);
    }
};

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
    const int16_t *s2, *s3;
    const uint16_t *i2, *i3;
    uint32_t sz2, sz3;
    sd_host_ext_matrix(host, 2, &s2, &i2, &sz2);
    sd_host_ext_matrix(host, 3, &s3, &i3, &sz3);
    double ratios[21 * 21];
    int8_t self[21];
    sd_host_index_tables(host, ratios, self);
    const uint32_t chunk = (uint32_t) std::max<long long>(1, a.integer("--chunk-queries", 16384));
    const int nSplits = plan.n;
    std::vector<std::vector<SplitRow> > rows((size_t) nSplits);             // per split: the rows of all queries, query after query
    std::vector<std::vector<uint32_t> > rowCount((size_t) nSplits);         // per split: rows of every query
    std::vector<uint8_t> failed(qdb.n, 0);
    QueryChunk qc;
    std::vector<uint64_t> tOff;
    uint64_t notComputed = 0;
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
        uint64_t st[4] = {0, 0, 0, 0};
        int rc = sd_target_build(ctx, k, PS.indexThr, PS.mask ? 1 : 0, PS.maskProb, tdb.residues.data() + t0, tOff.data(), (uint32_t) dbSize, ratios, self,
                                 s2, i2, s3, i3, &target.t, st);
        if (rc != SD_OK) {
            if (rc == SD_ENOMEM || strstr(sd_last_error(ctx), "out of memory"))
                fprintf(stderr, "sdgpu prefilter: the index of split %d of %d did not fit the device memory; raise --split or let --split 0 choose\n",
                        sp + 1, nSplits);
            return failCtx(ctx, rc, "sd_target_build");
        }
        info(a, "Index statistics\nEntries:          %llu\n", (unsigned long long) st[0]);
        lap.mark("split: index build");
        sd_prefilter_params par = PS.par;
        par.maxHitsPerQuery = (int32_t) std::min<uint64_t>(plan.listLen, dbSize);   // (a list holds no more rows than the split has sequences)
        // QueryMatcher is constructed with the split's dbSize (Prefiltering.cpp:797-799)
        if (!a.has("--bin-size")) par.binSize = sd_host_bin_size(dbSize, (uint64_t) a.integer("--l2-cache-size", 0));
        rowCount[sp].assign(qdb.n, 0);
        for (uint32_t c0 = 0; c0 < qdb.n; c0 += chunk) {
            const uint32_t c1 = std::min(qdb.n, c0 + chunk), nq = c1 - c0;
            rc = qc.run(ctx, host, target.t, par, PS, qdb, tdb, sameDb, c0, c1, dbFrom, dbSize);
            std::vector<uint32_t> &counts = qc.counts;
            if (rc != SD_OK) return failCtx(ctx, rc, "sd_prefilter_batch");
            for (uint32_t i = 0; i < nq; i++) {
                if (counts[i] == UINT32_MAX) {   // per-query error slot of sd_prefilter_batch: not computed
                    if (!failed[c0 + i]) {
                        if (notComputed < 5) fprintf(stderr, "sdgpu prefilter: query %u was not computed: %s\n", qdb.keys[c0 + i], sd_last_error(ctx));
                        notComputed++;
                    }
                    failed[c0 + i] = 1;
                    counts[i] = 0;
                }
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
    char line[64];
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
        for (const SplitRow &r : merged) {
            const int len = snprintf(line, sizeof(line), "%u\t%d\t%d\n", r.key, r.score, (int) r.diagonal);
            text.append(line, (size_t) len);
        }
        totalHits += merged.size();
        if (!out.write(qdb.keys[q], text.data(), text.size())) return fail("cannot write " + a.pos[2]);
    }
    if (!out.close(&err)) return fail(err);
    lap.mark("merge + write");
    info(a, "%llu prefilter hits written for %u queries\n", (unsigned long long) totalHits, qdb.n);
    if (notComputed)
        return fail(std::to_string(notComputed) + " queries need the reference's double-overflow route (or have >= 2^32 index hits) and were "
                    "written as empty entries; every other entry is complete");
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
    if (a.integer("--target-search-mode", 0) != 0) return fail("--target-search-mode 1 is not supported");
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
    const bool sameDb = a.pos[0] == a.pos[1];
    std::shared_ptr<SeqDb> tdb = loadTargetDb(a.pos[1], host.h, &err);
    std::unique_ptr<SeqDb> qdbOwn;
    if (!tdb) return fail(err);
    if (tdb->profile) return fail("profile target databases are not supported on this path");
    SeqDb *qdb = tdb.get();
    if (!sameDb) {
        qdbOwn.reset(new SeqDb());
        if (!qdbOwn->load(a.pos[0], host.h, &err)) return fail(err);
        qdb = qdbOwn.get();
    }
    lap.mark("load DBs");
    info(a, "Query database size: %u type: %s\nTarget database size: %u type: Aminoacid\n", qdb->n,
         qdb->profile ? "Profile" : "Aminoacid", tdb->n);

    CtxH ctx;
    int rc = ctx.open(deviceOf(a));
    if (rc != SD_OK) return fail("no usable HIP device (sd_ctx_create returned " + std::to_string(rc) + "); this path has no CPU fallback");
    lap.mark("context");

    // --split: one index for the whole target (today's path, below) or one per target split (prefilterTargetSplit)
    SplitPlan plan;
    {
        bool residentTarget = false;
        if (resident().enabled) {   // a workflow that holds this DB's index on this device has nothing left to decide
            char dsuf[24];
            snprintf(dsuf, sizeof(dsuf), "|%d", deviceOf(a));
            const std::string pfx = a.pos[1] + "|", suf = dsuf;
            for (const auto &kv : resident().targets)
                if (kv.first.compare(0, pfx.size(), pfx) == 0 && kv.first.size() >= suf.size() &&
                    kv.first.compare(kv.first.size() - suf.size(), suf.size(), suf) == 0)
                    residentTarget = true;
        }
        if (int rcP = resolveSplit(a, tdb->rd, tdb->totalResidues(), qdb->n, ctx.c, residentTarget, plan)) return rcP;
    }
    PrefSetup PS;
    if (int rcS = prefilterSetupFromArgs(a, host.h, *tdb, qdb->profile, PS, plan.k)) return rcS;
    if (plan.target) return prefilterTargetSplit(a, host.h, ctx.c, *qdb, *tdb, sameDb, PS, plan, lap);
    const int k = PS.k, kmerThr = PS.kmerThr;
    const bool mask = PS.mask;
    const double maskProb = PS.maskProb;

    // target side: TARGET.idx when a createindex file with matching parameters lies next to the DB (PrefilteringIndexReader
    // layout, sd_mod_index.cpp), else IndexBuilder::fillDatabase on the device (sd_target_build: mask + lists); resident in HBM afterwards.
    // Profile searches index every k-mer (Prefiltering.cpp:525-527)
    const int indexThr = qdb->profile ? 0 : kmerThr;
    IndexH index;
    LoadedIndex loaded;
    std::string why;
    uint64_t nEntries = 0, maskedRes = 0;
    const uint32_t *kOff = nullptr, *eSeq = nullptr;
    const uint16_t *ePos = nullptr;
    const uint8_t *masked = nullptr;
    const uint64_t *kBase = nullptr;
    const int16_t *s2, *s3;
    const uint16_t *i2, *i3;
    uint32_t sz2, sz3;
    sd_host_ext_matrix(host.h, 2, &s2, &i2, &sz2);
    sd_host_ext_matrix(host.h, 3, &s3, &i3, &sz3);
    TargetH target;
    // a workflow's resident target of exactly this index (same DB, k, threshold, masking, device) is taken as it is
    char tkey[96];
    snprintf(tkey, sizeof(tkey), "|%d|%d|%d|%.6f|%d", k, indexThr, mask ? 1 : 0, maskProb, deviceOf(a));
    const std::string targetKey = a.pos[1] + tkey;
    if (resident().enabled && resident().targets.count(targetKey)) {
        const Resident::TargetEntry &te = resident().targets[targetKey];
        target.t = te.t;
        target.own = false;
        nEntries = te.nEntries;
        maskedRes = te.masked;
        info(a, "Target index resident from the previous module of this workflow\n");
    }
    const int got = target.t ? 1 : loadTargetIndex(a.pos[1], k, indexThr, mask ? 1 : 0, tdb->n, tdb->totalResidues(), loaded, &why);
    if (got < 0) return fail(why);
    if (got == 0) {
        kOff = loaded.offsets.data();
        kBase = loaded.blockBase.empty() ? nullptr : loaded.blockBase.data();
        eSeq = loaded.entrySeq.data();
        ePos = loaded.entryPos.data();
        masked = loaded.masked.data();
        nEntries = loaded.nEntries;
        info(a, "Use index %s.idx\n", a.pos[1].c_str());
    } else {
        if (sddb::fileExists(a.pos[1] + ".idx.index")) info(a, "Index file not used: %s\n", why.c_str());
    }
    if (target.t) {
        // resident
    } else if (got != 0 && !getenv("SD_INDEX_HOST")) {
        // IndexBuilder::fillDatabase on the device (sd_target_build): mask, k-mer lists, list starts
        double ratios[21 * 21];
        int8_t self[21];
        sd_host_index_tables(host.h, ratios, self);
        uint64_t st[4] = {0, 0, 0, 0};
        rc = sd_target_build(ctx.c, k, indexThr, mask ? 1 : 0, maskProb, tdb->residues.data(), tdb->offsets.data(), tdb->n, ratios, self, s2, i2,
                             s3, i3, &target.t, st);
        if (rc != SD_OK) {
            if (rc == SD_ENOMEM || strstr(sd_last_error(ctx.c), "out of memory"))
                fprintf(stderr, "sdgpu prefilter: the target index did not fit the device memory; --split 0 chooses a number of target splits "
                                "that does, --split N --split-mode 0 sets it\n");
            return failCtx(ctx.c, rc, "sd_target_build");
        }
        nEntries = st[0];
        maskedRes = st[1];
    } else if (got != 0) {
        rc = sd_host_index_build(host.h, tdb->residues.data(), tdb->offsets.data(), tdb->n, k, indexThr, mask ? 1 : 0, maskProb, &index.ix);
        if (rc != SD_OK) return fail("sd_host_index_build failed (" + std::to_string(rc) + ")");
        uint64_t tableSize = 0;
        sd_host_index_info(index.ix, &tableSize, &nEntries, &maskedRes);
        sd_host_index_arrays(index.ix, &kOff, &eSeq, &ePos, &masked);
        sd_host_index_block_base(index.ix, &kBase, nullptr);
    }
    info(a, "Index table k-mer threshold: %d at k-mer size %d\nIndex statistics\nEntries:          %llu\n", kmerThr, k,
         (unsigned long long) nEntries);
    if (!target.t) {
        rc = sd_target_create_wide(ctx.c, k, kOff, kBase, eSeq, ePos, nEntries, masked, tdb->offsets.data(), tdb->n, s2, i2, s3, i3, &target.t);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_target_create");
    }
    if (resident().enabled && target.own) {   // stays for the next module of the workflow
        // one resident index per (DB, device): an index of the same DB with other parameters -- the sequence-threshold index of
        // iteration 0 once the profile iterations (threshold 0, a larger index) begin -- would only hold HBM until the workflow ends
        char dsuf[24];
        snprintf(dsuf, sizeof(dsuf), "|%d", deviceOf(a));
        const std::string pfx = a.pos[1] + "|", suf = dsuf;
        for (auto it = resident().targets.begin(); it != resident().targets.end();) {
            const std::string &key = it->first;
            if (key.compare(0, pfx.size(), pfx) == 0 && key.size() >= suf.size() && key.compare(key.size() - suf.size(), suf.size(), suf) == 0) {
                info(a, "Resident target index %s replaced\n", key.c_str());
                sd_target_destroy(it->second.t);
                it = resident().targets.erase(it);
            } else {
                ++it;
            }
        }
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
    std::string text;
    uint64_t totalHits = 0, notComputed = 0;
    for (uint32_t c0 = 0; c0 < qdb->n; c0 += chunk) {
        const uint32_t c1 = std::min(qdb->n, c0 + chunk), nq = c1 - c0;
        rc = qc.run(ctx.c, host.h, target.t, par, PS, *qdb, *tdb, sameDb, c0, c1, 0, tdb->n);
        std::vector<uint32_t> &counts = qc.counts;
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_prefilter_batch");
        lap.mark("chunk: bias + device");
        // QueryMatcher::prefilterHitToBuffer (QueryMatcher.h:118-130): targetKey \t score \t (int16) diagonal
        char line[64];
        for (uint32_t i = 0; i < nq; i++) {
            text.clear();
            if (counts[i] == UINT32_MAX) {   // per-query error slot of sd_prefilter_batch: not computed
                if (notComputed < 5) fprintf(stderr, "sdgpu prefilter: query %u was not computed: %s\n", qdb->keys[c0 + i], sd_last_error(ctx.c));
                notComputed++;
                counts[i] = 0;
            }
            const sd_hit *row = qc.hits.data() + (size_t) i * par.maxHitsPerQuery;
            for (uint32_t x = 0; x < counts[i]; x++) {
                const int len = snprintf(line, sizeof(line), "%u\t%d\t%d\n", tdb->keys[row[x].seqId], row[x].score,
                                         (int) (int16_t) row[x].diagonal);
                text.append(line, (size_t) len);
            }
            totalHits += counts[i];
            if (!out.write(qdb->keys[c0 + i], text.data(), text.size())) return fail("cannot write " + a.pos[2]);
        }
    }
    lap.mark("chunks: text + write");
    if (!out.close(&err)) return fail(err);
    lap.mark("close");
    info(a, "%llu prefilter hits written for %u queries\n", (unsigned long long) totalHits, qdb->n);
    if (notComputed)
        return fail(std::to_string(notComputed) + " queries need the reference's double-overflow route (or have >= 2^32 index hits) and were "
                    "written as empty entries; every other entry is complete");
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
    const bool sameDb = a.pos[0] == a.pos[1];
    std::shared_ptr<SeqDb> tdb = loadTargetDb(a.pos[1], host.h, &err);
    std::unique_ptr<SeqDb> qdbOwn;
    if (!tdb) return fail(err);
    if (tdb->profile) return fail("profile target databases are not supported on this path");
    SeqDb *qdb = tdb.get();
    if (!sameDb) {
        qdbOwn.reset(new SeqDb());
        if (!qdbOwn->load(a.pos[0], host.h, &err)) return fail(err);
        qdb = qdbOwn.get();
    }
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
    if (rc != SD_OK) return fail("no usable HIP device (sd_ctx_create returned " + std::to_string(rc) + "); this path has no CPU fallback");
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
        // QueryMatcher::prefilterHitToBuffer with diagonal 0 (ungappedprefilter.cpp:447-451)
        char line[64];
        for (uint32_t i = 0; i < nq; i++) {
            text.clear();
            const sd_hit *row = hits.data() + (size_t) i * par.maxHitsPerQuery;
            for (uint32_t x = 0; x < counts[i]; x++) {
                const int len = snprintf(line, sizeof(line), "%u\t%d\t0\n", tdb->keys[row[x].seqId], row[x].score);
                text.append(line, (size_t) len);
            }
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

// ---------------------------------------------------------------------------------------------------------------
namespace {

int alignPairs(sd_ctx *ctx, const sd_sw_params &par, sd_seqset *qs, sd_seqset *ts, const SeqDb &qdb, const SeqDb &tdb,
               const std::vector<uint32_t> &qIdOfLocal, const std::vector<uint32_t> &pq, const std::vector<uint32_t> &pt,
               const std::vector<uint8_t> &ident, bool compact, std::vector<uint32_t> &outIdx, std::vector<sd_sw_result> &res,
               BtPool &pool) {
    const uint32_t n = (uint32_t) pq.size();
    res.resize(std::max<uint32_t>(n, 1));
    outIdx.resize(std::max<uint32_t>(n, 1));
    // a first guess that a second call rarely has to correct (a too small pool costs the whole batch again): a backtrace has at
    // most qLen + tLen columns and, for the full-length homologs that dominate, about min(qLen, tLen) of them
    uint64_t cap = 1u << 20;
    if (par.swMode == 2) {
        uint64_t est = 0;
        for (uint32_t i = 0; i < n; i++) est += (uint64_t) std::min(qdb.lens[qIdOfLocal[pq[i]]], tdb.lens[pt[i]]) + 16;
        cap += est + est / 4;
    }
    bool exact = false;
    for (;;) {
        pool.reserve(cap);
        uint64_t used = 0;
        int rc;
        uint32_t nOut = n;
        if (compact)
            rc = sd_sw_align_batch_compact(ctx, &par, qs, ts, n, pq.data(), pt.data(), ident.data(), outIdx.data(), res.data(),
                                           &nOut, pool.p.get(), pool.cap, &used);
        else
            rc = sd_sw_align_batch(ctx, &par, qs, ts, n, pq.data(), pt.data(), ident.data(), res.data(), pool.p.get(), pool.cap, &used);
        if (rc == SD_ENOMEM && !exact) {   // pool too small: the exact bound is sum(qLen + tLen)
            uint64_t need = 64;
            for (uint32_t i = 0; i < n; i++) need += (uint64_t) qdb.lens[qIdOfLocal[pq[i]]] + (uint64_t) tdb.lens[pt[i]];
            cap = need;
            exact = true;
            continue;
        }
        if (rc != SD_OK) return rc;
        if (compact) {
            res.resize(nOut);
            outIdx.resize(nOut);
        } else {
            for (uint32_t i = 0; i < n; i++) outIdx[i] = i;
        }
        return SD_OK;
    }
}

struct SeqSetGuard {
    sd_seqset *s = nullptr;
    ~SeqSetGuard() { if (s) sd_seqset_destroy(s); }
};

// --alt-ali (Alignment::computeAlternativeAlignment, Alignment.cpp:399-401,433-435,569-601): the records the chunk's queries have
// accepted so far are the seeds; sd_sw_align_alt_batch returns up to altAli further alignments per seed, with the pass's own
// parameters (under --realign the realigner's: score-biased matrix, the coverage threshold, no E-value gate, Alignment.cpp:434).
// The alternatives join their query's list and the list is ordered by Matcher::compareHits again (:403-405, :437-439): the sort
// is stable over (seeds in their order, then alternatives in (seed, round) order), which fixes the order of the ties the
// reference's unstable sort leaves open.
int altAlignChunk(sd_ctx *ctx, const AlignSetup &s, const SeqDb &qdb, const SeqDb &tdb, const std::vector<uint32_t> &localQ, sd_seqset *qs,
                  sd_seqset *ts, AlignChunk &c) {
    const uint32_t nq = (uint32_t) localQ.size();
    const std::vector<sd_sw_result> &recs = *c.outRecs;
    const std::vector<uint32_t> &order = *c.outOrder, &counts = *c.outCounts, &recT = *c.outT;
    const std::vector<uint8_t> &recIdent = *c.outIdent;
    uint64_t nSeeds = 0;
    for (uint32_t q = 0; q < nq; q++) nSeeds += counts[q];
    if (nSeeds == 0) return SD_OK;
    c.seedQ.resize(nSeeds); c.seedT.resize(nSeeds); c.seedB.resize(nSeeds); c.seedE.resize(nSeeds); c.seedIdent.resize(nSeeds);
    c.seedIdx.resize(nSeeds);
    uint64_t w = 0, poolNeed = 64;
    for (uint32_t q = 0; q < nq; q++)
        for (uint32_t x = 0; x < counts[q]; x++, w++) {
            const uint32_t i = order[w];
            c.seedIdx[w] = i;
            c.seedQ[w] = q;
            c.seedT[w] = recT[i];
            c.seedIdent[w] = recIdent[i];
            // an identity pair is skipped (its record may carry no positions in a mode without them)
            c.seedB[w] = recIdent[i] ? 0 : recs[i].tStart;
            c.seedE[w] = recIdent[i] ? 0 : recs[i].tEnd;
            poolNeed += (uint64_t) qdb.lens[localQ[q]] + (uint64_t) tdb.lens[recT[i]];
        }
    const sd_sw_params &par = s.realign ? s.rpar : s.par;
    const uint32_t N = (uint32_t) s.altAli;
    c.altRes.resize(nSeeds * N);
    c.altCount.assign(nSeeds, 0);
    // a first guess of two rounds' backtraces per seed; the exact bound is N rounds (a too small pool costs the call again)
    uint64_t cap = par.swMode == 2 ? std::min<uint64_t>(2, N) * poolNeed : 64, used = 0;
    for (bool exact = false;;) {
        c.pool3.reserve(cap);
        const int rc = sd_sw_align_alt_batch(ctx, &par, qs, ts, (uint32_t) nSeeds, c.seedQ.data(), c.seedT.data(), c.seedB.data(), c.seedE.data(),
                                             c.seedIdent.data(), N, s.crit.seqIdThr, s.crit.alnLenThr, s.crit.seqIdMode, c.altRes.data(),
                                             c.altCount.data(), c.pool3.p.get(), c.pool3.cap, &used);
        if (rc == SD_ENOMEM && !exact) {
            cap = (uint64_t) N * poolNeed;
            exact = true;
            continue;
        }
        if (rc != SD_OK) return rc;
        break;
    }
    // the combined records: seeds (their backtraces move behind the alternatives' in pool3), then every seed's alternatives
    uint64_t nAlt = 0, seedBt = 0;
    for (uint64_t x = 0; x < nSeeds; x++) {
        nAlt += c.altCount[x];
        if (recs[c.seedIdx[x]].btLen > 0) seedBt += (uint64_t) recs[c.seedIdx[x]].btLen;
    }
    if (c.pool3.cap < used + seedBt) {
        BtPool grown;
        grown.reserve(used + seedBt);
        memcpy(grown.p.get(), c.pool3.p.get(), used);
        std::swap(grown, c.pool3);
    }
    c.fin.resize(nSeeds + nAlt);
    c.finT.resize(nSeeds + nAlt);
    c.finIdent.assign(nSeeds + nAlt, 0);
    c.finOrder.resize(nSeeds + nAlt);
    c.finCounts.assign(std::max<uint32_t>(nq, 1), 0);
    const char *seedPool = c.outPool->data();
    uint64_t o = 0, x0 = 0;
    struct Key {
        double eval;
        int bits, dbLen;
        uint32_t dbKey, idx;
    };
    std::vector<Key> keys;
    for (uint32_t q = 0; q < nq; q++) {
        keys.clear();
        auto add = [&](const sd_sw_result &r, uint32_t t, uint8_t ident) {
            c.fin[o] = r;
            c.finT[o] = t;
            c.finIdent[o] = ident;
            Key k;
            k.eval = r.evalue;
            k.bits = static_cast<int>(sd_host_bitscore((double) (uint32_t) r.score) + 0.5);
            k.dbLen = tdb.lens[t];
            k.dbKey = tdb.keys[t];
            k.idx = (uint32_t) o++;
            keys.push_back(k);
        };
        for (uint32_t x = 0; x < counts[q]; x++) {
            sd_sw_result r = recs[c.seedIdx[x0 + x]];
            if (r.btLen > 0 && seedPool) {
                memcpy(c.pool3.p.get() + used, seedPool + r.btOffset, (size_t) r.btLen);
                r.btOffset = used;
                used += (uint64_t) r.btLen;
            }
            add(r, c.seedT[x0 + x], c.seedIdent[x0 + x]);
        }
        for (uint32_t x = 0; x < counts[q]; x++)
            for (uint32_t r = 0; r < c.altCount[x0 + x]; r++) add(c.altRes[(x0 + x) * N + r], c.seedT[x0 + x], 0);
        std::stable_sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) {   // Matcher::compareHits
            if (a.eval != b.eval) return a.eval < b.eval;
            if (a.bits != b.bits) return a.bits > b.bits;
            if (a.dbLen != b.dbLen) return a.dbLen < b.dbLen;
            return a.dbKey < b.dbKey;
        });
        const uint64_t base = o - keys.size();
        for (size_t x = 0; x < keys.size(); x++) c.finOrder[base + x] = keys[x].idx;
        c.finCounts[q] = (uint32_t) keys.size();
        x0 += counts[q];
    }
    c.outRecs = &c.fin;
    c.outOrder = &c.finOrder;
    c.outCounts = &c.finCounts;
    c.outT = &c.finT;
    c.outIdent = &c.finIdent;
    c.outPool = &c.pool3;
    return SD_OK;
}

}  // namespace

int alignSetupFromArgs(const Args &a, sd_host *host, uint64_t targetResidues, AlignSetup &s) {
    if (a.flag("--wrapped-scoring", false)) return fail("--wrapped-scoring is a nucleotide mode");
    s.altAli = (int) std::min<long long>(a.integer("--alt-ali", 0), 4096);
    if (s.altAli < 0) return fail("--alt-ali must not be negative");
    if (a.integer("--alignment-output-mode", 0) != 0) return fail("--alignment-output-mode 0 only");
    if (a.real("--score-bias", 0.0) != 0.0) return fail("--score-bias 0 only");
    if (a.real("--corr-score-weight", 0.0) != 0.0) return fail("--corr-score-weight 0 only");
    if (a.multi("--gap-open", "aa", "11") != "11" || a.multi("--gap-extend", "aa", "1") != "1")
        return fail("gap costs other than --gap-open 11 --gap-extend 1 need other E-value parameters than the built-in preset");
    if (a.real("--comp-bias-corr-scale", 1.0) != 1.0) return fail("--comp-bias-corr-scale 1 only");
    s.compBias = a.integer("--comp-bias-corr", 1) != 0;
    int alignmentMode = (int) a.integer("--alignment-mode", 0);
    if (alignmentMode == 4) return fail("Use rescorediagonal for ungapped alignment mode.");
    bool addBacktrace = a.flag("-a", false);
    s.realign = a.flag("--realign", false);
    s.realignScoreBias = (float) a.real("--realign-score-bias", -0.2);
    if (s.realign && !(s.realignScoreBias == -0.2f || s.realignScoreBias == 0.0f))
        return fail("--realign-score-bias: -0.2 (default) and 0 are built in");
    float covThr = (float) a.real("-c", 0.0);
    s.canCovThr = covThr;
    s.covMode = (int) a.integer("--cov-mode", 0);
    const float seqIdThr = (float) a.real("--min-seq-id", 0.0);
    // Alignment::Alignment (Alignment.cpp:31-57)
    if (addBacktrace) alignmentMode = 3;
    int realignSwMode = 0;
    auto initSWMode = [](int mode, float cov, float sid) {   // Alignment::initSWMode (:170-192)
        switch (mode) {
            case 0: return (cov > 0.0f && sid == 0.0f) ? 1 : ((cov > 0.0f && sid > 0.0f) ? 2 : 0);
            case 2: return 1;
            case 3: return 2;
            default: return 0;
        }
    };
    float realignCov = 0.0f;
    if (s.realign) {
        realignSwMode = initSWMode(std::max(alignmentMode, 2), 0.0f, 0.0f);
        alignmentMode = 1;
        realignCov = covThr;
        covThr = 0.0f;
        addBacktrace = true;
    }
    if (s.altAli > 0) alignmentMode = std::max(alignmentMode, 2);   // start positions for the masks (Alignment.cpp:79-89)
    s.swMode = initSWMode(alignmentMode, (float) a.real("-c", 0.0), seqIdThr);
    memset(&s.par, 0, sizeof(s.par));
    s.par.gapOpen = 11;
    s.par.gapExtend = 1;
    sd_host_matrix(host, 0, s.par.matrix, nullptr, nullptr);
    s.par.covMode = s.covMode;
    s.par.covThr = covThr;
    s.par.evalThr = a.real("-e", 0.001);
    s.par.swMode = s.swMode;
    s.par.dbResidues = targetResidues;
    s.rpar = s.par;   // the realigner (Alignment.cpp:296-303,419): score-biased matrix, E-value gate off
    if (s.realign) {
        sd_host_matrix(host, s.realignScoreBias == 0.0f ? 0 : 2, s.rpar.matrix, nullptr, nullptr);
        s.rpar.covThr = realignCov;
        s.rpar.evalThr = FLT_MAX;
        s.rpar.swMode = realignSwMode;
    }
    memset(&s.crit, 0, sizeof(s.crit));
    s.crit.evalThr = s.par.evalThr;
    s.crit.seqIdThr = seqIdThr;
    s.crit.alnLenThr = (int32_t) a.integer("--min-aln-len", 0);
    s.crit.covMode = s.covMode;
    s.crit.covThr = s.realign ? realignCov : covThr;
    s.crit.seqIdMode = (int32_t) a.integer("--seq-id-mode", 0);
    s.crit.swMode = s.swMode;
    s.crit.addBacktrace = addBacktrace ? 1 : 0;
    s.crit.realign = s.realign ? 1 : 0;
    s.crit.realignSwMode = realignSwMode;
    s.crit.realignMaxSeqs = (int32_t) std::min<long long>(a.integer("--realign-max-seqs", INT_MAX), INT_MAX);
    s.crit.maxAccept = (uint32_t) std::min<long long>(a.integer("--max-accept", INT_MAX), INT_MAX);
    s.crit.maxRejected = (uint32_t) std::min<long long>(a.integer("--max-rejected", INT_MAX), INT_MAX);
    s.stopRules = s.crit.maxAccept != (uint32_t) INT_MAX || s.crit.maxRejected != (uint32_t) INT_MAX;
    s.includeIdentity = a.flag("--add-self-matches", false);
    return 0;
}

int alignChunkCore(sd_ctx *ctx, sd_host *host, const AlignSetup &s, const SeqDb &qdb, const SeqDb &tdb, sd_seqset *tset, AlignChunk &c, Lap *lap,
                   const char **what) {
    static const char *none = "";
    const char *dummyWhat;
    if (!what) what = &dummyWhat;
    *what = none;
    int rc = SD_OK;
    const std::vector<uint32_t> &localQ = c.localQ, &pq = c.pq, &pt = c.pt;
    const std::vector<uint8_t> &ident = c.ident;
    const uint32_t nq = (uint32_t) localQ.size();
    // queries of the chunk as one sequence set on the device
    c.qoff.assign((size_t) nq + 1, 0);
    c.qlen.resize(nq);
    for (uint32_t i = 0; i < nq; i++) {
        c.qlen[i] = qdb.lens[localQ[i]];
        c.qoff[i + 1] = c.qoff[i] + (uint64_t) c.qlen[i];
    }
    c.qres.resize(c.qoff[nq] + 1);
    for (uint32_t i = 0; i < nq; i++) memcpy(c.qres.data() + c.qoff[i], qdb.residues.data() + qdb.offsets[localQ[i]], (size_t) c.qlen[i]);
    SeqSetGuard qset;
    if (nq) {
        if (qdb.profile) {
            c.qaln.resize((c.qoff[nq] + 1) * 21);
            for (uint32_t i = 0; i < nq; i++)
                memcpy(c.qaln.data() + c.qoff[i] * 21, qdb.alnProfile.data() + qdb.offsets[localQ[i]] * 21, (size_t) c.qlen[i] * 21);
            rc = sd_profileset_create(ctx, c.qres.data(), c.qoff.data(), nq, c.qaln.data(), &qset.s);
        } else {
            c.qbias.assign(c.qoff[nq] + 1, 0);
            if (s.compBias) sd_host_comp_bias(host, c.qres.data(), c.qoff.data(), nq, 6, c.qbias.data(), nullptr, nullptr);
            rc = sd_seqset_create(ctx, c.qres.data(), c.qoff.data(), nq, c.qbias.data(), &qset.s);
        }
        if (rc != SD_OK) {
            *what = "sd_seqset_create(queries)";
            return rc;
        }
    }
    if (lap) lap->mark("chunk: query set");
    // the pairs that are aligned (pre-rejected ones are not)
    c.apq.clear();
    c.apt.clear();
    c.aid.clear();
    c.aIdx.clear();
    c.apq.reserve(pq.size());
    for (size_t i = 0; i < pq.size(); i++)
        if (ident[i] != 2) {
            c.apq.push_back(pq[i]);
            c.apt.push_back(pt[i]);
            c.aid.push_back(ident[i]);
            c.aIdx.push_back((uint32_t) i);
        }
    c.aligned = c.apq.size();
    const bool compact = s.swMode == 2 && !s.stopRules;
    if (!c.apq.empty()) {
        rc = alignPairs(ctx, s.par, qset.s, tset, qdb, tdb, localQ, c.apq, c.apt, c.aid, compact, c.idxOut, c.res, c.pool);
        if (rc != SD_OK) {
            *what = "sd_sw_align_batch";
            return rc;
        }
    } else {
        c.res.clear();
        c.idxOut.clear();
    }
    if (lap) lap->mark("chunk: alignPairs");
    // record list handed to the criteria: compact -> only the reportable records; otherwise every pair in prefilter
    // order, pre-rejected ones as records that fail every criterion (E-value NaN)
    c.recQ.clear();
    c.recT.clear();
    c.recIdent.clear();
    std::vector<sd_sw_result> *recs = &c.res;
    if (compact) {
        c.recQ.resize(c.res.size());
        c.recT.resize(c.res.size());
        c.recIdent.resize(c.res.size());
        for (size_t x = 0; x < c.res.size(); x++) {
            c.recQ[x] = c.apq[c.idxOut[x]];
            c.recT[x] = c.apt[c.idxOut[x]];
            c.recIdent[x] = c.aid[c.idxOut[x]];
        }
    } else {
        c.full.resize(pq.size());
        sd_sw_result dummy;
        memset(&dummy, 0, sizeof(dummy));
        dummy.qStart = dummy.tStart = dummy.qEnd = dummy.tEnd = -1;
        dummy.evalue = NAN;
        for (size_t i = 0; i < pq.size(); i++) c.full[i] = dummy;
        for (size_t x = 0; x < c.aIdx.size(); x++) c.full[c.aIdx[x]] = c.res[x];
        c.recQ = pq;
        c.recT = pt;
        c.recIdent.resize(pq.size());
        for (size_t i = 0; i < pq.size(); i++) c.recIdent[i] = ident[i] == 1 ? 1 : 0;
        recs = &c.full;
    }
    c.order.resize(std::max<size_t>(recs->size(), 1));
    c.counts.assign(std::max<uint32_t>(nq, 1), 0);
    rc = sd_host_accept_sort(&s.crit, nq, (uint32_t) recs->size(), c.recQ.data(), c.recT.data(), recs->data(), c.recIdent.data(),
                             c.qlen.data(), tdb.lens.data(), tdb.keys.data(), c.order.data(), c.counts.data());
    if (rc != SD_OK) {
        *what = "sd_host_accept_sort";
        return rc;
    }
    uint64_t nAcc = 0;
    for (uint32_t i = 0; i < nq; i++) nAcc += c.counts[i];
    c.accepted = nAcc;
    c.outRecs = recs;
    c.outOrder = &c.order;
    c.outCounts = &c.counts;
    c.outT = &c.recT;
    c.outIdent = &c.recIdent;
    c.outPool = &c.pool;
    SeqSetGuard qset2;
    sd_seqset *rq = qset.s;   // the query set of the pass the output records come from
    if (s.realign && nAcc > 0) {
        // second pass over the accepted records, in their order (Alignment.cpp:408-440)
        c.pq2.resize(nAcc);
        c.pt2.resize(nAcc);
        c.ident2.resize(nAcc);
        uint64_t w = 0;
        for (uint32_t q = 0; q < nq; q++)
            for (uint32_t x = 0; x < c.counts[q]; x++, w++) {
                const uint32_t i = c.order[w];
                c.pq2[w] = q;
                c.pt2[w] = c.recT[i];
                c.ident2[w] = c.recIdent[i];
            }
        // the realigner's query profile: composition bias against the score-biased matrix (a profile query carries its
        // scores itself and is reused)
        if (!qdb.profile && s.compBias && s.realignScoreBias != 0.0f) {
            c.qbias2.assign(c.qoff[nq] + 1, 0);
            sd_host_sw_comp_bias(host, 2, c.qres.data(), c.qoff.data(), nq, c.qbias2.data());
            rc = sd_seqset_create(ctx, c.qres.data(), c.qoff.data(), nq, c.qbias2.data(), &qset2.s);
            if (rc != SD_OK) {
                *what = "sd_seqset_create(realign queries)";
                return rc;
            }
            rq = qset2.s;
        }
        rc = alignPairs(ctx, s.rpar, rq, tset, qdb, tdb, localQ, c.pq2, c.pt2, c.ident2, false, c.idx2, c.res2, c.pool2);
        if (rc != SD_OK) {
            *what = "sd_sw_align_batch(realign)";
            return rc;
        }
        c.merged.resize(nAcc);
        c.order2.resize(nAcc);
        c.counts2.assign(nq, 0);
        rc = sd_host_realign_select(&s.crit, nq, c.counts.data(), c.order.data(), c.recT.data(), recs->data(), c.res2.data(),
                                    c.ident2.data(), c.qlen.data(), tdb.lens.data(), tdb.keys.data(), c.merged.data(),
                                    c.order2.data(), c.counts2.data());
        if (rc != SD_OK) {
            *what = "sd_host_realign_select";
            return rc;
        }
        c.outRecs = &c.merged;
        c.outOrder = &c.order2;
        c.outCounts = &c.counts2;
        c.accT = c.pt2;
        c.outT = &c.accT;
        c.outIdent = &c.ident2;
        c.outPool = &c.pool2;
    } else if (s.realign) {
        c.counts2.assign(std::max<uint32_t>(nq, 1), 0);
        c.outCounts = &c.counts2;
    }
    if (lap) lap->mark("chunk: accept / sort (+ realign)");
    if (s.altAli > 0) {
        rc = altAlignChunk(ctx, s, qdb, tdb, localQ, s.realign ? rq : qset.s, tset, c);
        if (rc != SD_OK) {
            *what = "sd_sw_align_alt_batch";
            return rc;
        }
        if (lap) lap->mark("chunk: alternative alignments");
    }
    return SD_OK;
}

int alignModule(const Args &a) {
    if (a.pos.size() != 4) return fail("usage: align <queryDB> <targetDB> <prefilterDB> <alignmentDB> [options]");
    if (int rc = checkCommon(a)) return rc;
    const int threads = threadsOf(a);
    Lap lap("align");
    HostH host;
    if (host.open(threads) != SD_OK) return fail("sd_host_create failed");
    std::string err;
    const bool sameDb = a.pos[0] == a.pos[1];
    std::shared_ptr<SeqDb> tdb = loadTargetDb(a.pos[1], host.h, &err);
    std::unique_ptr<SeqDb> qdbOwn;
    if (!tdb) return fail(err);
    if (tdb->profile) return fail("profile target databases are not supported on this path");
    SeqDb *qdb = tdb.get();
    if (!sameDb) {
        qdbOwn.reset(new SeqDb());
        if (!qdbOwn->load(a.pos[0], host.h, &err)) return fail(err);
        qdb = qdbOwn.get();
    }
    AlignSetup S;
    if (int rcS = alignSetupFromArgs(a, host.h, tdb->totalResidues(), S)) return rcS;
    const int swMode = S.swMode, covMode = S.covMode;
    const float canCovThr = S.canCovThr;
    const bool includeIdentity = S.includeIdentity;
    lap.mark("load DBs");
    sddb::Reader pref;
    if (!pref.open(a.pos[2], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    info(a, "%s\nQuery database size: %u type: %s\nTarget database size: %u type: Aminoacid\n",
         swMode == 0 ? "Compute score only" : (swMode == 1 ? "Compute score and coverage" : "Compute score, coverage and sequence identity"),
         qdb->n, qdb->profile ? "Profile" : "Aminoacid", tdb->n);

    CtxH ctx;
    int rc = ctx.open(deviceOf(a));
    if (rc != SD_OK) return fail("no usable HIP device (sd_ctx_create returned " + std::to_string(rc) + "); this path has no CPU fallback");

    SeqSetH tset;
    const std::string tsetKey = a.pos[1] + "|" + std::to_string(deviceOf(a));
    if (resident().enabled && resident().seqSets.count(tsetKey)) {
        tset.s = resident().seqSets[tsetKey];   // the target sequences are on the device already
        tset.own = false;
    } else {
        rc = sd_seqset_create(ctx.c, tdb->residues.data(), tdb->offsets.data(), tdb->n, nullptr, &tset.s);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create(targets)");
        if (resident().enabled) {
            resident().seqSets[tsetKey] = tset.s;
            tset.own = false;
        }
    }

    lap.mark("context + target sequences on the device");
    sddb::Writer out;
    int outType = sddb::withExtended(sddb::DBTYPE_ALIGNMENT_RES, sddb::extendedType(pref.dbtype()));
    if (!out.open(a.pos[3], outType, &err)) return fail(err);
    sd_alntext *text = nullptr;
    sd_alntext_create(&text);
    std::unique_ptr<sd_alntext, void (*)(sd_alntext *)> textGuard(text, sd_alntext_destroy);

    const uint64_t maxPairs = 4000000;
    const size_t nEntries = pref.size();
    uint64_t alignmentsNum = 0, passedNum = 0;
    AlignChunk C;
    std::vector<uint32_t> &localQ = C.localQ, &pq = C.pq, &pt = C.pt;
    std::vector<uint8_t> &ident = C.ident;
    // lines per prefilter entry (one pass over the DB on all threads): the chunks are cut from these, and a chunk's lines are then
    // parsed in parallel into their places
    std::vector<uint32_t> lineCount(nEntries, 0);
#pragma omp parallel for schedule(dynamic, 256)
    for (size_t e = 0; e < nEntries; e++) {
        uint32_t c = 0;
        for (const char *d = pref.data(e); *d != '\0';) {
            const char *nl = strchr(d, '\n');
            c++;
            if (!nl) break;
            d = nl + 1;
        }
        lineCount[e] = c;
    }
    lap.mark("count prefilter lines");
    std::vector<uint64_t> pairOff;
    for (size_t e0 = 0; e0 < nEntries;) {
        // chunk of entries bounded by pairs
        localQ.clear();
        size_t e1 = e0;
        std::vector<uint32_t> entryLocal;   // local query index of entry (UINT32_MAX: empty entry)
        pairOff.assign(1, 0);
        while (e1 < nEntries && (pairOff.back() < maxPairs || e1 == e0) && localQ.size() < 20000) {
            if (lineCount[e1] == 0) {
                entryLocal.push_back(UINT32_MAX);
                pairOff.push_back(pairOff.back());
                e1++;
                continue;
            }
            const uint32_t qKey = pref.key(e1);
            const size_t qId = qdb->rd.idOfKey(qKey);
            if (qId == SIZE_MAX)
                return fail("Query sequence " + std::to_string(qKey) + " is required in the prefiltering, but is not contained in the query sequence database.");
            entryLocal.push_back((uint32_t) localQ.size());
            localQ.push_back((uint32_t) qId);
            pairOff.push_back(pairOff.back() + lineCount[e1]);
            e1++;
        }
        pq.resize(pairOff.back());
        pt.resize(pairOff.back());
        ident.resize(pairOff.back());
        uint32_t missingKey = UINT32_MAX;
        bool missing = false;
#pragma omp parallel for schedule(dynamic, 64)
        for (size_t e = e0; e < e1; e++) {
            const uint32_t lq = entryLocal[e - e0];
            if (lq == UINT32_MAX) continue;
            const uint32_t qKey = pref.key(e);
            const float qL = (float) qdb->lens[localQ[lq]];
            uint64_t w = pairOff[e - e0];
            for (const char *d = pref.data(e); *d != '\0';) {
                const uint32_t tKey = (uint32_t) strtoul(d, nullptr, 10);
                while (*d != '\n' && *d != '\0') d++;
                if (*d == '\n') d++;
                const size_t tId = tdb->rd.idOfKey(tKey);
                if (tId == SIZE_MAX) {
#pragma omp critical(sd_align_missing)
                    {
                        missing = true;
                        missingKey = tKey;
                    }
                    break;
                }
                // Util::canBeCovered pre-check (Alignment.cpp:370-373): a rejected pair, never aligned
                const bool can = sd_host_can_be_covered(canCovThr, covMode, qL, (float) tdb->lens[tId]) != 0;
                pq[w] = lq;
                pt[w] = (uint32_t) tId;
                // 2 marks the pre-rejected pair: kept only so that --max-rejected counts it
                ident[w] = !can ? 2 : ((qKey == tKey && (includeIdentity || sameDb)) ? 1 : 0);
                w++;
            }
        }
        if (missing)
            return fail("Sequence " + std::to_string(missingKey) + " is required in the prefiltering, but is not contained in the target sequence database!");
        lap.mark("chunk: parse prefilter entries");
        const uint32_t nq = (uint32_t) localQ.size();
        const char *what = "";
        rc = alignChunkCore(ctx.c, host.h, S, *qdb, *tdb, tset.s, C, &lap, &what);
        if (rc != SD_OK) return failCtx(ctx.c, rc, what);
        alignmentsNum += C.aligned;
        passedNum += C.accepted;
        rc = sd_alntext_format(text, &S.crit, nq, C.outCounts->data(), C.outOrder->data(), C.outT->data(), C.outRecs->data(), C.outIdent->data(),
                               C.outPool->data(), C.qlen.data(), tdb->lens.data(), tdb->keys.data());
        if (rc != SD_OK) return fail("sd_alntext_format failed (" + std::to_string(rc) + ")");
        lap.mark("chunk: format");
        const char *txt;
        const uint64_t *eoff;
        sd_alntext_get(text, &txt, &eoff);
        for (size_t e = e0; e < e1; e++) {
            const uint32_t lq = entryLocal[e - e0];
            if (lq == UINT32_MAX) {
                if (!out.write(pref.key(e), "", 0)) return fail("cannot write " + a.pos[3]);
            } else if (!out.write(pref.key(e), txt + eoff[lq], (size_t) (eoff[lq + 1] - eoff[lq]))) {
                return fail("cannot write " + a.pos[3]);
            }
        }
        lap.mark("chunk: write");
        e0 = e1;
    }
    if (!out.close(&err)) return fail(err);
    lap.mark("close");
    info(a, "%llu alignments calculated\n%llu sequence pairs passed the thresholds\n", (unsigned long long) alignmentsNum,
         (unsigned long long) passedNum);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// rescorediagonal <queryDB> <targetDB> <prefilterDB> <resultDB> (M/src/alignment/rescorediagonal.cpp:45-434 with the parameters of
// Parameters.cpp:506-523): the best ungapped local alignment on every prefilter hit's own diagonal -- what blastp.sh calls instead of
// `align` under --alignment-mode 4.  The per-hit arithmetic runs on the device (sd_rescore_diagonal_batch); the row logic of
// doRescorediagonal (:194-363) is the host side here.
namespace {

// SmithWaterman::computeCov (StripedSmithWaterman.cpp:1671-1673)
inline float rescoreCov(unsigned start, unsigned end, unsigned len) {
    return (std::min(len, std::max(start, end)) - std::min(start, end) + 1) / (float) len;
}
// Util::hasCoverage (Util.cpp:496-511)
inline bool rescoreHasCov(float thr, int mode, float qCov, float tCov) {
    switch (mode) {
        case 0: return qCov >= thr && tCov >= thr;
        case 1: return qCov >= thr;
        case 2: return tCov >= thr;
        default: return true;
    }
}
// Util::computeSeqId (Util.cpp:532-542)
inline float rescoreSeqId(int mode, int ids, int qLen, int tLen, int alnLen) {
    switch (mode) {
        case 1: return static_cast<float>(ids) / static_cast<float>(std::min(qLen, tLen));
        case 2: return static_cast<float>(ids) / static_cast<float>(std::max(qLen, tLen));
        case 0: return static_cast<float>(ids) / static_cast<float>(alnLen);
    }
    return 0.0f;
}

// the DB's bytes of every sequence, laid out like SeqDb::residues
void gatherLetters(const SeqDb &db, std::vector<char> &out) {
    out.resize(db.totalResidues() + 1);
#pragma omp parallel for schedule(static)
    for (uint32_t i = 0; i < db.n; i++) memcpy(out.data() + db.offsets[i], db.rd.data(i), (size_t) db.lens[i]);
}

}  // namespace

int rescorediagonalModule(const Args &a) {
    if (a.pos.size() != 4) return fail("usage: rescorediagonal <queryDB> <targetDB> <prefilterDB> <resultDB> [options]");
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    const std::string sm = a.multi("--sub-mat", "aa", "blosum62.out");
    if (sm != "blosum62.out") return fail("--sub-mat " + sm + ": only blosum62.out is built into this path");
    const int mode = (int) a.integer("--rescore-mode", 0);
    if (mode == 3) return fail("--rescore-mode 3 (global alignment) is not implemented");
    if (mode == 4) return fail("--rescore-mode 4 (window quality alignment) is not implemented");
    if (mode < 0 || mode > 4) return fail("--rescore-mode " + std::to_string(mode) + ": 0 (Hamming), 1 (substitution) and 2 (alignment) are implemented");
    if (a.flag("--filter-hits", false)) return fail("--filter-hits 1 is not implemented (its score-per-column thresholds are a table of the reference)");
    if (a.flag("--wrapped-scoring", false)) return fail("--wrapped-scoring 1 is a nucleotide mode and is not implemented");
    const double evalThr = a.real("-e", 0.001);
    const float covThr = (float) a.real("-c", 0.0), seqIdThr = (float) a.real("--min-seq-id", 0.0);
    const int covMode = (int) a.integer("--cov-mode", 0), alnLenThr = (int) a.integer("--min-aln-len", 0);
    const int seqIdMode = (int) a.integer("--seq-id-mode", 0);
    const bool addBacktrace = a.flag("-a", false), includeIdentity = a.flag("--add-self-matches", false);
    const bool sortResults = a.integer("--sort-results", 0) > 0;
    const int threads = threadsOf(a);

    Lap lap("rescorediagonal");
    HostH host;
    if (host.open(threads) != SD_OK) return fail("sd_host_create failed");
    std::string err;
    {   // (SeqDb::load names amino acid and profile DBs only; say what this module was given)
        const int qt = sddb::baseType(sddb::readDbType(a.pos[0])), tt = sddb::baseType(sddb::readDbType(a.pos[1]));
        if (qt == sddb::DBTYPE_NUCLEOTIDES || tt == sddb::DBTYPE_NUCLEOTIDES) return fail("nucleotide databases are not implemented in rescorediagonal");
        if (qt == sddb::DBTYPE_HMM_PROFILE || tt == sddb::DBTYPE_HMM_PROFILE) return fail("profile databases are not implemented in rescorediagonal");
    }
    const bool sameDb = a.pos[0] == a.pos[1];
    std::shared_ptr<SeqDb> tdb = loadTargetDb(a.pos[1], host.h, &err);
    std::unique_ptr<SeqDb> qdbOwn;
    if (!tdb) return fail(err);
    SeqDb *qdb = tdb.get();
    if (!sameDb) {
        qdbOwn.reset(new SeqDb());
        if (!qdbOwn->load(a.pos[0], host.h, &err)) return fail(err);
        qdb = qdbOwn.get();
    }
    sddb::Reader pref;
    if (!pref.open(a.pos[2], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    if (sddb::baseType(pref.dbtype()) == 14)   // Parameters::DBTYPE_PREFILTER_REV_RES
        return fail("reverse (bi-directional) prefilter results are a nucleotide mode and are not implemented");
    lap.mark("load DBs");
    info(a, "Rescore mode %d\nQuery database size: %u type: Aminoacid\nTarget database size: %u type: Aminoacid\n", mode, qdb->n, tdb->n);

    CtxH ctx;
    int rc = ctx.open(deviceOf(a));
    if (rc != SD_OK) return fail("no usable HIP device (sd_ctx_create returned " + std::to_string(rc) + "); this path has no CPU fallback");
    // both sides as sets that carry the DB's letters; the target set of a workflow is the resident one
    SeqSetH tset, qsetOwn;
    std::vector<char> letters;
    const std::string tsetKey = a.pos[1] + "|" + std::to_string(deviceOf(a));
    if (resident().enabled && resident().seqSets.count(tsetKey)) {
        tset.s = resident().seqSets[tsetKey];
        tset.own = false;
    } else {
        rc = sd_seqset_create(ctx.c, tdb->residues.data(), tdb->offsets.data(), tdb->n, nullptr, &tset.s);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create(targets)");
        if (resident().enabled) {
            resident().seqSets[tsetKey] = tset.s;
            tset.own = false;
        }
    }
    // a resident set that carries its letters already (an earlier rescorediagonal of the workflow) is taken as it is
    const std::string lettersKey = tsetKey + "|letters";
    if (tset.own || !resident().seqSets.count(lettersKey)) {
        gatherLetters(*tdb, letters);
        rc = sd_seqset_set_letters(tset.s, letters.data());
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_set_letters(targets)");
        if (!tset.own) resident().seqSets[lettersKey] = nullptr;   // a mark only: Resident::clear and the stale-DB sweep skip null entries
    }
    sd_seqset *qset = tset.s;
    if (!sameDb) {
        rc = sd_seqset_create(ctx.c, qdb->residues.data(), qdb->offsets.data(), qdb->n, nullptr, &qsetOwn.s);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create(queries)");
        gatherLetters(*qdb, letters);
        rc = sd_seqset_set_letters(qsetOwn.s, letters.data());
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_set_letters(queries)");
        qset = qsetOwn.s;
    }
    letters.clear();
    letters.shrink_to_fit();
    lap.mark("context + sequences on the device");

    sd_rescore_params par;
    memset(&par, 0, sizeof(par));
    sd_host_matrix(host.h, 0, par.matrix, nullptr, par.aa2num);
    par.mode = mode;
    sd_aln_criteria crit;
    memset(&crit, 0, sizeof(crit));
    crit.evalThr = evalThr;
    crit.seqIdMode = seqIdMode;
    crit.swMode = 2;
    crit.addBacktrace = addBacktrace ? 1 : 0;
    const uint64_t dbResidues = tdb->totalResidues();   // tdbr->getAminoAcidDBSize() (rescorediagonal.cpp:107)

    sddb::Writer out;
    // rescorediagonal.cpp:396-401: an alignment DB in mode 2, else the input's type
    if (!out.open(a.pos[3], mode == 2 ? (int) sddb::DBTYPE_ALIGNMENT_RES : pref.dbtype(), &err)) return fail(err);
    sd_alntext *text = nullptr;
    sd_alntext_create(&text);
    std::unique_ptr<sd_alntext, void (*)(sd_alntext *)> textGuard(text, sd_alntext_destroy);
    const std::string mPool(65536, 'M');   // the backtrace of an ungapped alignment: alnLen matches

    const size_t nEntries = pref.size();
    const uint64_t maxHits = 4000000;
    uint64_t rescored = 0, passed = 0;
    std::vector<uint32_t> hq, ht, entryQ, order, counts, recT;
    std::vector<uint16_t> hd;
    std::vector<uint64_t> hitOff;
    std::vector<sd_rescore_result> res;
    std::vector<sd_sw_result> rec;
    std::vector<int32_t> qlen;
    std::vector<std::string> shortText;
    struct Short {
        int score;
        uint32_t key;
        int diagonal;
    };
    for (size_t e0 = 0; e0 < nEntries;) {
        // a chunk of entries bounded by hits; the pairs that cannot be covered never reach the device (rescorediagonal.cpp:211-213)
        size_t e1 = e0;
        hq.clear();
        ht.clear();
        hd.clear();
        entryQ.clear();
        hitOff.assign(1, 0);
        while (e1 < nEntries && (hq.size() < maxHits || e1 == e0)) {
            const char *d = pref.data(e1);
            uint32_t qId = UINT32_MAX;
            if (*d != '\0') {
                const size_t id = qdb->rd.idOfKey(pref.key(e1));
                if (id == SIZE_MAX)
                    return fail("Query sequence " + std::to_string(pref.key(e1)) + " is required in the prefiltering, but is not contained in the query sequence database.");
                qId = (uint32_t) id;
            }
            while (*d != '\0') {
                char *end;
                const uint32_t tKey = (uint32_t) strtoul(d, &end, 10);
                (void) strtol(end, &end, 10);
                const long diag = strtol(end, &end, 10);
                while (*d != '\n' && *d != '\0') d++;
                if (*d == '\n') d++;
                const size_t tId = tdb->rd.idOfKey(tKey);
                if (tId == SIZE_MAX)
                    return fail("Sequence " + std::to_string(tKey) + " is required in the prefiltering, but is not contained in the target sequence database!");
                if (!sd_host_can_be_covered(covThr, covMode, (float) qdb->lens[qId], (float) tdb->lens[tId])) continue;
                hq.push_back(qId);
                ht.push_back((uint32_t) tId);
                hd.push_back((uint16_t) (short) diag);   // QueryMatcher::parsePrefilterHit: a short, kept as an unsigned short
            }
            entryQ.push_back(qId);
            hitOff.push_back(hq.size());
            e1++;
        }
        const uint32_t nHits = (uint32_t) hq.size(), nE = (uint32_t) (e1 - e0);
        res.resize(std::max<uint32_t>(nHits, 1));
        rc = sd_rescore_diagonal_batch(ctx.c, &par, qset, tset.s, nHits, hq.data(), ht.data(), hd.data(), res.data());
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_rescore_diagonal_batch");
        rescored += nHits;
        lap.mark("chunk: parse + device");
        // the row logic per entry (rescorediagonal.cpp:239-341), the accepted rows of an entry in input order or sorted
        rec.resize(std::max<uint32_t>(nHits, 1));
        recT = ht;
        order.assign(std::max<uint32_t>(nHits, 1), 0);
        counts.assign(std::max<uint32_t>(nE, 1), 0);
        qlen.assign(std::max<uint32_t>(nE, 1), 0);
        shortText.assign(nE, std::string());
#pragma omp parallel
        {
            std::vector<uint32_t> acc;
            std::vector<Short> shorts;
#pragma omp for schedule(dynamic, 64)
            for (uint32_t e = 0; e < nE; e++) {
                acc.clear();
                shorts.clear();
                const uint32_t qId = entryQ[e];
                const int qLen = qId == UINT32_MAX ? 0 : qdb->lens[qId];
                qlen[e] = qLen;
                for (uint64_t x = hitOff[e]; x < hitOff[e + 1]; x++) {
                    const sd_rescore_result &r = res[x];
                    const uint32_t tId = ht[x];
                    const int tLen = tdb->lens[tId];
                    const bool isIdentity = qId == tId && (includeIdentity || sameDb);
                    double seqId = 0, evalue = 0.0;
                    int bitScore = 0, alnLen = 0, idCnt = 0;
                    float targetCov = static_cast<float>(r.diagonalLen) / static_cast<float>(tLen);
                    float queryCov = static_cast<float>(r.diagonalLen) / static_cast<float>(qLen);
                    sd_sw_result &o = rec[x];
                    memset(&o, 0, sizeof(o));
                    if (mode == 0) {
                        seqId = rescoreSeqId(seqIdMode, r.score, qLen, tLen, r.diagonalLen);
                        alnLen = r.diagonalLen;
                    } else {
                        evalue = sd_host_evalue(dbResidues, (double) r.score, (double) qLen);
                        bitScore = static_cast<int>(sd_host_bitscore((double) r.score) + 0.5);
                        if (mode == 2) {
                            alnLen = (r.endPos - r.startPos) + 1;
                            int qS, qE, tS, tE;
                            if (r.diagonal >= 0) {
                                qS = r.startPos + r.distToDiagonal;
                                qE = r.endPos + r.distToDiagonal;
                                tS = r.startPos;
                                tE = r.endPos;
                            } else {
                                qS = r.startPos;
                                qE = r.endPos;
                                tS = r.startPos + r.distToDiagonal;
                                tE = r.endPos + r.distToDiagonal;
                            }
                            if (evalue <= evalThr || isIdentity) {   // the identity count is used only here (:284-292)
                                idCnt = r.idCnt;
                                seqId = rescoreSeqId(seqIdMode, idCnt, qLen, tLen, alnLen);
                            }
                            queryCov = rescoreCov((unsigned) qS, (unsigned) qE, (unsigned) qLen);
                            targetCov = rescoreCov((unsigned) tS, (unsigned) tE, (unsigned) tLen);
                            o.score = r.score;
                            o.qStart = qS;
                            o.qEnd = qE;
                            o.tStart = tS;
                            o.tEnd = tE;
                            o.identical = idCnt;
                            o.btLen = alnLen;
                            o.evalue = evalue;
                        }
                    }
                    const bool hasCov = rescoreHasCov(covThr, covMode, queryCov, targetCov);
                    const bool hasSeqId = seqId >= (seqIdThr - std::numeric_limits<float>::epsilon());
                    const bool hasEvalue = evalue <= evalThr;
                    const bool hasAlnLen = alnLen >= alnLenThr;
                    if (!(isIdentity || (hasAlnLen && hasCov && hasSeqId && hasEvalue))) continue;
                    if (mode == 2) acc.push_back((uint32_t) x);
                    else shorts.push_back({mode == 1 ? bitScore : (int) (100 * seqId), tdb->keys[tId], r.diagonal});
                }
                if (mode == 2) {
                    if (sortResults && acc.size() > 1)   // Matcher::compareHits (Matcher.h:157-168)
                        std::sort(acc.begin(), acc.end(), [&](uint32_t x, uint32_t y) {
                            const sd_sw_result &p = rec[x], &q = rec[y];
                            if (p.evalue != q.evalue) return p.evalue < q.evalue;
                            const int bp = static_cast<int>(sd_host_bitscore((double) p.score) + 0.5), bq = static_cast<int>(sd_host_bitscore((double) q.score) + 0.5);
                            if (bp != bq) return bp > bq;
                            if (tdb->lens[ht[x]] != tdb->lens[ht[y]]) return tdb->lens[ht[x]] < tdb->lens[ht[y]];
                            return tdb->keys[ht[x]] < tdb->keys[ht[y]];
                        });
                    counts[e] = (uint32_t) acc.size();
                    for (size_t i = 0; i < acc.size(); i++) order[hitOff[e] + i] = acc[i];   // compacted below
                } else {
                    if (sortResults && shorts.size() > 1)   // hit_t::compareHitsByScoreAndId (QueryMatcher.h:38-48)
                        std::sort(shorts.begin(), shorts.end(), [](const Short &p, const Short &q) {
                            if (abs(p.score) != abs(q.score)) return abs(p.score) > abs(q.score);
                            return p.key < q.key;
                        });
                    char line[64];
                    for (const Short &h : shorts) {   // QueryMatcher::prefilterHitToBuffer: the diagonal as a short
                        const int len = snprintf(line, sizeof(line), "%u\t%d\t%d\n", h.key, h.score, (int) (short) (unsigned short) h.diagonal);
                        shortText[e].append(line, (size_t) len);
                    }
                    counts[e] = (uint32_t) shorts.size();
                }
            }
        }
        for (uint32_t e = 0; e < nE; e++) passed += counts[e];
        if (mode == 2) {
            uint64_t w = 0;
            for (uint32_t e = 0; e < nE; e++)
                for (uint32_t i = 0; i < counts[e]; i++) order[w++] = order[hitOff[e] + i];
            rc = sd_alntext_format(text, &crit, nE, counts.data(), order.data(), recT.data(), rec.data(), nullptr, mPool.data(), qlen.data(),
                                   tdb->lens.data(), tdb->keys.data());
            if (rc != SD_OK) return fail("sd_alntext_format failed (" + std::to_string(rc) + ")");
            const char *txt;
            const uint64_t *eoff;
            sd_alntext_get(text, &txt, &eoff);
            for (uint32_t e = 0; e < nE; e++)
                if (!out.write(pref.key(e0 + e), txt + eoff[e], (size_t) (eoff[e + 1] - eoff[e]))) return fail("cannot write " + a.pos[3]);
        } else {
            for (uint32_t e = 0; e < nE; e++)
                if (!out.write(pref.key(e0 + e), shortText[e].data(), shortText[e].size())) return fail("cannot write " + a.pos[3]);
        }
        lap.mark("chunk: rows + write");
        e0 = e1;
    }
    if (!out.close(&err)) return fail(err);
    info(a, "%llu hits rescored\n%llu sequence pairs passed the thresholds\n", (unsigned long long) rescored, (unsigned long long) passed);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
int clusterhitsModule(const Args &a) {
    if (a.pos.size() != 4) return fail("usage: clusterhits <querySetDB> <targetSetDB> <matchesDB> <clustersDB> [options]");
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    if (a.flag("--cluster-use-weight", false)) return fail("--cluster-use-weight 1 is not supported");
    std::string err;
    Lap lap("clusterhits");
    const std::shared_ptr<const SetInfo> qsP = loadSetInfo(a.pos[0], false, &err);
    if (!qsP) return fail(err);
    const bool sameDb = a.pos[0] == a.pos[1];
    const std::shared_ptr<const SetInfo> tsP = sameDb ? qsP : loadSetInfo(a.pos[1], false, &err);
    if (!tsP) return fail(err);
    const SetInfo &qs = *qsP, &ts = *tsP;
    lap.mark("set info");
    sddb::Reader res, hdr;
    if (!res.open(a.pos[2], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    if (!hdr.open(a.pos[2] + "_h", sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    if (hdr.size() != res.size()) return fail("matches and matches_h differ in size");
    const bool dbOut = a.flag("--db-output", false);

    sd_ch_params par;
    par.maxGeneGap = (uint32_t) a.integer("--max-gene-gap", 3);
    par.clusterSize = (uint32_t) a.integer("--cluster-size", 2);
    par.alpha = a.real("--alpha", 1.0);
    par.pCluThr = (float) a.real("--cluster-pval", 0.01);
    par.pMHThr = (float) a.real("--multihit-pval", 0.01);

    // entries -> flat arrays (R/src/util/ClusterHits.cpp:300-353)
    std::vector<uint64_t> hitOff(1, 0);
    std::vector<uint32_t> qPos, tPos, Nq, entryQSet, entryTSet;
    std::vector<uint8_t> strands;
    std::vector<double> pval;
    std::vector<std::pair<const char *, uint32_t> > lines;   // hit line (with its '\n')
    uint32_t maxOrf = 0;
    for (uint32_t s : qs.setSize) maxOrf = std::max(maxOrf, s);
    for (uint32_t s : ts.setSize) maxOrf = std::max(maxOrf, s);
    uint32_t maxPos = 0;
    // the matches parsed on all threads, each into lists of its own, then laid out back to back in entry order
    struct ParsedMatch {
        std::vector<std::pair<const char *, uint32_t> > lines;
        std::vector<uint32_t> qPos, tPos;
        std::vector<uint8_t> strands;
        std::vector<double> pval;
        unsigned long qSet = 0, tSet = 0, nq = 0;
        uint32_t maxPos = 0;
        std::string error;
    };
    std::vector<ParsedMatch> parsed;
    const size_t parseBlock = 8192;
    for (size_t b0 = 0; b0 < res.size(); b0 += parseBlock) {
        const size_t b1 = std::min(res.size(), b0 + parseBlock);
        parsed.resize(b1 - b0);
#pragma omp parallel for schedule(dynamic, 8)
        for (size_t i = b0; i < b1; i++) {
            ParsedMatch &pm = parsed[i - b0];
            pm.lines.clear();
            pm.qPos.clear();
            pm.tPos.clear();
            pm.strands.clear();
            pm.pval.clear();
            pm.error.clear();
            pm.maxPos = 0;
            const char *h = hdr.data(i);
            char *end;
            pm.qSet = strtoul(h, &end, 10);
            pm.tSet = strtoul(end, &end, 10);
            pm.nq = strtoul(end, &end, 10);
            // six tab separated columns are required (ClusterHits.cpp:303-307)
            int cols = 0;
            for (const char *c = h; *c && *c != '\n'; c++) cols += (*c == '\t');
            if (cols < 5) {
                pm.error = "Invalid header record";
                continue;
            }
            const char *d = res.data(i);
            while (*d != '\0') {
                const char *ls = d;
                char *e2;
                const unsigned long qid = strtoul(d, &e2, 10);
                const unsigned long tid = strtoul(e2, &e2, 10);
                const double p = strtod(e2, nullptr);
                while (*d != '\n' && *d != '\0') d++;
                if (*d == '\n') d++;
                if (qid >= qs.nameOfKey.size() || qs.nameOfKey[qid].empty()) {
                    pm.error = "Invalid query lookup record";
                    break;
                }
                if (tid >= ts.nameOfKey.size() || ts.nameOfKey[tid].empty()) {
                    pm.error = "Invalid target lookup record";
                    break;
                }
                pm.lines.push_back(std::make_pair(ls, (uint32_t) (d - ls)));
                pm.qPos.push_back(qs.posOfKey[qid]);
                pm.tPos.push_back(ts.posOfKey[tid]);
                pm.maxPos = std::max(pm.maxPos, std::max(qs.posOfKey[qid], ts.posOfKey[tid]));
                pm.strands.push_back((uint8_t) (qs.strandOfKey[qid] | (ts.strandOfKey[tid] << 1)));
                pm.pval.push_back(p);
            }
        }
        for (size_t i = b0; i < b1; i++) {
            const ParsedMatch &pm = parsed[i - b0];
            if (!pm.error.empty()) return fail(pm.error);
            const size_t K = pm.lines.size();
            if (K <= 1) continue;   // a single hit is no cluster (ClusterHits.cpp:359-361)
            lines.insert(lines.end(), pm.lines.begin(), pm.lines.end());
            qPos.insert(qPos.end(), pm.qPos.begin(), pm.qPos.end());
            tPos.insert(tPos.end(), pm.tPos.begin(), pm.tPos.end());
            strands.insert(strands.end(), pm.strands.begin(), pm.strands.end());
            pval.insert(pval.end(), pm.pval.begin(), pm.pval.end());
            maxPos = std::max(maxPos, pm.maxPos);
            hitOff.push_back(lines.size());
            Nq.push_back((uint32_t) pm.nq);
            entryQSet.push_back((uint32_t) pm.qSet);
            entryTSet.push_back((uint32_t) pm.tSet);
        }
    }
    parsed.clear();
    parsed.shrink_to_fit();
    lap.mark("parse matches");
    const uint32_t nPairs = (uint32_t) Nq.size();
    const uint64_t total = hitOff.back();
    std::vector<uint32_t> clusterOf(std::max<uint64_t>(total, 1), UINT32_MAX), rank(std::max<uint64_t>(total, 1), 0),
        nClusters(std::max<uint32_t>(nPairs, 1), 0), cSize(std::max<uint64_t>(total, 1), 0);
    std::vector<double> pCO(std::max<uint64_t>(total, 1), 0.0), pMH(std::max<uint64_t>(total, 1), 0.0);
    if (nPairs > 0) {
        CtxH ctx;
        int rc = sd_ctx_create(deviceOf(a), &ctx.c);
        if (rc != SD_OK) return fail("no usable HIP device (sd_ctx_create returned " + std::to_string(rc) + "); this path has no CPU fallback");
        const uint32_t lgN = std::max(maxOrf, maxPos) + 8;
        std::vector<double> lg(lgN);
        sd_host_lgamma_table(lg.data(), lgN);
        rc = sd_clusterhits_batch(ctx.c, &par, nPairs, hitOff.data(), qPos.data(), tPos.data(), strands.data(), pval.data(), Nq.data(),
                                  lg.data(), lgN, clusterOf.data(), rank.data(), nClusters.data(), pCO.data(), pMH.data(), cSize.data());
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_clusterhits_batch");
    }
    lap.mark("device");
    sddb::Writer out, outH;
    if (!out.open(a.pos[3], dbOut ? res.dbtype() : (int) sddb::DBTYPE_OMIT_FILE, &err)) return fail(err);
    if (!outH.open(a.pos[3] + "_h", sddb::DBTYPE_GENERIC_DB, &err)) return fail(err);
    uint32_t key = 0;
    // the clusters of a block of set pairs formatted on all threads (members in their rank order), written in order
    struct PairText {
        std::string body, head;
        std::vector<uint32_t> bodyEnd, headEnd;   // per cluster
    };
    std::vector<PairText> texts;
    const uint32_t writeBlock = 4096;
    for (uint32_t e0 = 0; e0 < nPairs; e0 += writeBlock) {
        const uint32_t e1 = std::min(nPairs, e0 + writeBlock);
        texts.resize(e1 - e0);
#pragma omp parallel
        {
            std::vector<uint32_t> member, start;
            char co[32], mh[32];
#pragma omp for schedule(dynamic, 8)
            for (uint32_t e = e0; e < e1; e++) {
                PairText &pt = texts[e - e0];
                pt.body.clear();
                pt.head.clear();
                pt.bodyEnd.clear();
                pt.headEnd.clear();
                const uint64_t off = hitOff[e], end = hitOff[e + 1];
                const uint32_t nC = nClusters[e];
                start.assign((size_t) nC + 1, 0);
                for (uint32_t c = 0; c < nC; c++) start[c + 1] = start[c] + cSize[off + c];
                member.assign(start[nC], 0);
                for (uint64_t h = off; h < end; h++)
                    if (clusterOf[h] < nC) member[start[clusterOf[h]] + rank[h]] = (uint32_t) (h - off);
                for (uint32_t c = 0; c < nC; c++) {
                    for (uint32_t x = start[c]; x < start[c + 1]; x++) pt.body.append(lines[off + member[x]].first, lines[off + member[x]].second);
                    snprintf(co, sizeof(co), "%.3E", pCO[off + c]);
                    snprintf(mh, sizeof(mh), "%.3E", pMH[off + c]);
                    pt.head += std::to_string(entryQSet[e]) + "\t" + std::to_string(entryTSet[e]) + "\t" + co + "\t" + mh + "\t" +
                               std::to_string(cSize[off + c]) + "\n";
                    pt.bodyEnd.push_back((uint32_t) pt.body.size());
                    pt.headEnd.push_back((uint32_t) pt.head.size());
                }
            }
        }
        for (uint32_t e = e0; e < e1; e++) {
            const PairText &pt = texts[e - e0];
            uint32_t b0 = 0, h0 = 0;
            for (size_t c = 0; c < pt.bodyEnd.size(); c++) {
                if (!out.write(key, pt.body.data() + b0, pt.bodyEnd[c] - b0) || !outH.write(key, pt.head.data() + h0, pt.headEnd[c] - h0))
                    return fail("cannot write " + a.pos[3]);
                b0 = pt.bodyEnd[c];
                h0 = pt.headEnd[c];
                key++;
            }
        }
    }
    lap.mark("write clusters");
    if (!out.close(&err) || !outH.close(&err)) return fail(err);
    if (!dbOut) ::remove((a.pos[3] + ".index").c_str());
    lap.mark("close");
    info(a, "%u clusters from %u set pairs\n", key, nPairs);
    return 0;
}

}  // namespace sdcli
