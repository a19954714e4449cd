// What the modules around the prefilter share (sd_pref_core.cpp): the query / target DB pair, a device target built from sequences, one
// chunk of queries against a target with its "not computed" slots, the text of a prefilter row and a workflow's resident target objects.
// prefilter, its target split and ungappedprefilter (sd_mod_prefilter.cpp), align and rescorediagonal, result2profile and the search
// workflows (sd_mod_workflow.cpp) and the in-memory iterative search (sd_mod_iter.cpp) are the callers.
#ifndef SD_PREF_CORE_H
#define SD_PREF_CORE_H

#include "sd_cli.h"

#include <memory>
#include <string>
#include <vector>

namespace sdcli {

// what Prefiltering's constructor derives from the command line (Prefiltering.cpp:180-215,1005-1065)
struct PrefSetup {
    int k = 6, kmerThr = 0, indexThr = 0;
    bool mask = true, includeIdentity = false, compBias = true;
    double maskProb = 0.9;
    sd_prefilter_params par;
};
// kOverride != 0: the k-mer size a split plan has chosen (the automatic size follows the number of splits)
int prefilterSetupFromArgs(const Args &a, sd_host *host, const SeqDb &tdb, bool profileQueries, PrefSetup &s, int kOverride = 0);

// --split / --split-mode / --split-memory-limit resolved (Prefiltering::setupSplit, Prefiltering.cpp:273-377) against the device's memory
struct SplitPlan {
    int n = 1;                        // number of splits
    bool target = false;              // a target split with n > 1: one index per split, built, searched and destroyed in turn
    int k = 0;                        // k-mer size: -k, or the automatic size of residues / n
    uint64_t listLen = 0;             // result list length of one split (of the whole run when !target)
    std::vector<uint64_t> from, size; // the target ids of every split (sd_host_split_plan)
};
// target: the target DB's reader (any access mode); residues: its residue count; ctx (nullable): a context of the device whose
// free memory decides when no --split-memory-limit is given (one is created for the question otherwise); residentTarget: the
// workflow already holds this target's index on the device, so nothing is left to decide.  Prints the reference's split-mode line.
int resolveSplit(const Args &a, const sddb::Reader &target, uint64_t residues, uint64_t nQueries, sd_ctx *ctx, bool residentTarget, SplitPlan &p);

// The query and the target DB of a module or workflow.  Equal paths are one load and qdb == tdb.  useResidentCache: the target goes
// through loadTargetDb (a module: a workflow's cache keeps it between modules); otherwise it is loaded for this call alone.
struct DbPair {
    std::shared_ptr<SeqDb> tdb;
    SeqDb *qdb = nullptr;
    bool sameDb = false;
    bool open(const std::string &queryPath, const std::string &targetPath, sd_host *host, bool useResidentCache, bool rejectProfileTarget,
              std::string *err);

private:
    std::unique_ptr<SeqDb> qdbOwn;
};

// A device target from n sequences with the index parameters of PS (sdBuildTarget, csrc/host/sd_target_build.h); st: {entries, masked
// residues}.  A failure is reported as `what` (the caller's name for the sd_target_build call) -- after oomHint when the device memory
// ran out and the caller has one -- and the exit code returned; 0 otherwise.
int buildTarget(sd_host *host, sd_ctx *ctx, const PrefSetup &PS, const uint8_t *residues, const uint64_t *offsets, uint32_t n, sd_target **out,
                uint64_t st[2], const std::string &oomHint = std::string(), const char *what = "sd_target_build");

// the queries of one chunk: n sequences or profiles of `seqs` from local id `base` on, which are the queries g0 .. g0 + n of `ids`, the
// query DB (the in-memory iterations search with the previous iteration's profiles of the chunk; everywhere else seqs == ids, base == g0)
struct QuerySpan {
    const SeqDb *seqs;
    uint32_t base;
    const SeqDb *ids;
    uint32_t g0, n;
};

// One chunk of queries against one target that holds the ids [dbFrom, dbFrom + dbSize) of the target DB (the whole DB, or one split of
// it): offsets rebased to the chunk, identity ids, composition bias, sd_prefilter_batch or sd_prefilter_profile_batch, and the
// per-query "not computed" slot (UINT32_MAX) of those calls.  The scratch is kept between chunks.
struct QueryChunk {
    std::vector<sd_hit> hits;        // row i at i * par.maxHitsPerQuery, ids relative to dbFrom
    std::vector<uint32_t> counts;    // a query that was not computed has 0 rows
    std::vector<uint64_t> off;       // the chunk's residue offsets, from 0 (n + 1)
    uint64_t notComputed = 0;        // queries counted so far
    std::string firstError;          // sd_last_error of the first of them
    bool printEach = false;          // the prefilter module's line per query (the first five)
    // failed (nullable): a flag per query of the chunk, set for a query that was not computed; one that is set already is not counted
    // again (the target split meets a query once per split, the iterations once per iteration).  stats (nullable): five sums the call adds
    // to -- similar k-mers, index hits, diagonals, diagonal length (the device call's statistics) and query residues.
    int run(sd_ctx *ctx, sd_host *host, const sd_target *target, const sd_prefilter_params &par, const PrefSetup &PS, const QuerySpan &q,
            const SeqDb &tdb, bool sameDb, uint64_t dbFrom, uint64_t dbSize, uint8_t *failed, uint64_t *stats);

private:
    std::vector<uint32_t> ident;
    std::vector<int8_t> diagBias;
    std::vector<int16_t> kmerBias;
    std::vector<uint64_t> perQuery;
};
// the run's last word when n > 0 queries were not computed: fail(...) with the caller's account of what became of them
int failNotComputed(uint64_t n, const char *whatBecameOfThem);

// QueryMatcher::prefilterHitToBuffer (QueryMatcher.h:118-130): targetKey \t score \t diagonal \n
void appendPrefRow(std::string &text, uint32_t key, int score, int diagonal);

// A workflow's resident target index of `db` on `device` ("db|k|threshold|mask|prob|device" in resident().targets, with "p" in the
// mask field for the similar-k-mer index of a profile DB; one per DB and device).  erase: it is destroyed and forgotten.  Returns its key, or an empty string when there is none.
std::string residentTargetOf(const std::string &db, int device, bool erase = false);
// the target sequences of `db` on the device: a workflow's resident set ("db|device" in resident().seqSets; created and registered on
// first use), else the module's own
int residentSeqSet(sd_ctx *ctx, const std::string &db, int device, const SeqDb &tdb, SeqSetH &out);

}  // namespace sdcli
#endif
