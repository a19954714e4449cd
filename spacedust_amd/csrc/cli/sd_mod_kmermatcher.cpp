// kmermatcher <sequenceDB> <prefDB>  (M/src/linclust/kmermatcher.cpp:847-874, 660-801): the first stage of linclust -- sequences that
// share one of their selected k-mers are grouped under the longest of them; the prefilter DB holds, per representative, its members
// with the number of shared k-mers and the best diagonal.  Records, sorts and the two segmented passes run on the GPU
// (sd_kmermatch_batch); the reduced alphabet, the -k 0 rule and the text are host stages (sd_host_reduced_alphabet,
// sd_host_kmermatch_auto_k, sd_host_kmermatch_format).  Amino-acid sequence DBs that fit the device in one split.
#include "sd_cli.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace sdcli {

namespace {
int envIntOr(const char *name, int def) {
    const char *v = getenv(name);
    return v ? atoi(v) : def;
}
}  // namespace

int kmermatcherModule(const Args &a) {
    if (a.pos.size() != 2) return fail("usage: kmermatcher <sequenceDB> <prefDB> [options]");
    if (int rc = checkCommon(a)) return rc;
    // what the reference has and this build does not, each by name
    if (a.integer("--mask", 0) != 0) return fail("--mask 1 (tantan masking before the k-mers are drawn) is not implemented");
    if (a.integer("--spaced-kmer-mode", 0) != 0) return fail("--spaced-kmer-mode 1 is not implemented (kmermatcher's default is 0)");
    if (!a.str("--spaced-kmer-pattern", "").empty()) return fail("--spaced-kmer-pattern is not implemented");
    if (a.flag("--ignore-multi-kmer", false)) return fail("--ignore-multi-kmer 1 is not implemented");
    if (!a.str("--weights", "").empty()) return fail("--weights (representatives by a weight file) is not implemented");
    if (a.flag("--adjust-kmer-len", false)) return fail("--adjust-kmer-len is not implemented (it applies to nucleotide DBs)");
    if (envIntOr("WORLD_SIZE", 1) > 1 || a.integer("--world-size", 1) > 1) return fail("kmermatcher runs on one rank");
    Lap lap("kmermatcher");
    std::string err;
    {
        sddb::Reader probe;
        if (!probe.open(a.pos[0], sddb::Reader::USE_INDEX, sddb::Reader::NOSORT, &err)) return fail(err);
        const int bt = sddb::baseType(probe.dbtype());
        if (bt == sddb::DBTYPE_NUCLEOTIDES) return fail("nucleotide DBs are not implemented (" + a.pos[0] + ")");
        if (bt == sddb::DBTYPE_HMM_PROFILE) return fail("profile DBs are not implemented (" + a.pos[0] + ")");
    }
    HostH host;
    if (host.open(threadsOf(a)) != SD_OK) return fail("sd_host_create failed");
    SeqDb db;
    if (!db.load(a.pos[0], host.h, &err)) return fail(err);
    if (db.profile) return fail("profile DBs are not implemented (" + a.pos[0] + ")");
    lap.mark("open");
    // setLinearFilterDefault + setKmerLengthAndAlphabet
    sd_kmermatch_params par;
    memset(&par, 0, sizeof(par));
    par.kmerSize = (int) a.integer("-k", 0);
    par.alphabetSize = atoi(a.multi("--alph-size", "aa", "13").c_str());
    if (par.kmerSize == 0) {
        if (sd_host_kmermatch_auto_k((float) a.real("--min-seq-id", 0.0), db.totalResidues(), &par.kmerSize, &par.alphabetSize) != SD_OK)
            return fail("sd_host_kmermatch_auto_k failed");
    }
    if (par.alphabetSize != 13 && par.alphabetSize != 21) return fail("--alph-size " + std::to_string(par.alphabetSize) + ": 13 and 21 are implemented");
    par.kmersPerSequence = (int) a.integer("--kmer-per-seq", 0);
    if (par.kmersPerSequence == 0) par.kmersPerSequence = 20;
    if (par.kmersPerSequence < 1) return fail("--kmer-per-seq must be at least 1");
    par.kmersPerSequenceScale = (float) atof(a.multi("--kmer-per-seq-scale", "aa", "0.0").c_str());
    par.hashShift = (int) a.integer("--hash-shift", 67);
    par.covMode = (int) a.integer("--cov-mode", 0);
    par.covThr = (float) a.real("-c", 0.8);
    par.includeOnlyExtendable = a.flag("--include-only-extendable", false) ? 1 : 0;
    uint8_t letterMap[21];
    int reduced = 0;
    if (sd_host_reduced_alphabet(0, par.alphabetSize, letterMap, &reduced) != SD_OK || reduced != par.alphabetSize)
        return fail("sd_host_reduced_alphabet failed");
    info(a, "kmermatcher: k %d, alphabet %d, %d k-mers per sequence (+ %g x length), %u sequences\n", par.kmerSize, par.alphabetSize,
         par.kmersPerSequence, (double) par.kmersPerSequenceScale, db.n);
    lap.mark("letter map");
    CtxH ctx;
    int rc = ctx.open(deviceOf(a));
    if (rc != SD_OK) return failNoDevice(rc, "sd_ctx_create", "kmermatcher builds and groups its records on the GPU (there is no CPU fallback)");
    lap.mark("context");
    const bool timing = getenv("SD_DEBUG_TIMING") != nullptr;
    if (timing) sd_profile_enable(ctx.c, 1);
    uint64_t stats[4] = {0, 0, 0, 0};
    // one call: a hit is a grouped record's run, so the record bound of the input (1 + kmerConsidered per sequence) is room enough
    uint64_t cap = 0;
    for (uint32_t i = 0; i < db.n; i++) {
        const uint64_t windows = db.lens[i] >= par.kmerSize ? (uint64_t) (db.lens[i] - par.kmerSize + 1) : 0;
        cap += 1 + std::min(sd_host_kmermatch_considered(par.kmersPerSequence, par.kmersPerSequenceScale, (uint32_t) db.lens[i]), windows);
    }
    std::unique_ptr<uint32_t[]> rep(new uint32_t[cap ? cap : 1]), member(new uint32_t[cap ? cap : 1]), score(new uint32_t[cap ? cap : 1]);
    std::unique_ptr<int32_t[]> diag(new int32_t[cap ? cap : 1]);
    rc = sd_kmermatch_batch(ctx.c, &par, db.n, db.residues.data(), db.offsets.data(), db.keys.data(), letterMap, cap, rep.get(), member.get(),
                            score.get(), diag.get(), stats);
    if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_kmermatch_batch");
    const uint64_t nHits = stats[2];
    if (timing) {
        static const char *const stage[] = {"km_prepare", "km_alloc", "km_copy_in", "km_records", "km_sort1", "km_group", "km_sort2", "km_hits", "km_copy_out"};
        fprintf(stderr, "[kmermatcher] device:");
        for (const char *s : stage) {
            double ms = 0;
            uint64_t calls = 0;
            sd_profile_get(ctx.c, (std::string("host:") + s).c_str(), &ms, &calls);
            fprintf(stderr, " %s %.3f ms", s + 3, ms);
        }
        fprintf(stderr, "; %llu records, %llu grouped, %llu hits, largest group %llu\n", (unsigned long long) stats[0], (unsigned long long) stats[1],
                (unsigned long long) stats[2], (unsigned long long) stats[3]);
    }
    lap.mark("device");
    uint64_t textBytes = 0;
    rc = sd_host_kmermatch_format(db.n, db.keys.data(), nHits, rep.get(), member.get(), score.get(), diag.get(), nullptr, nullptr, 0, nullptr,
                                  &textBytes);
    if (rc != SD_OK) return fail("sd_host_kmermatch_format failed (" + std::to_string(rc) + ")");
    std::vector<uint32_t> entryKey(db.n ? db.n : 1);
    std::vector<uint64_t> entryOff((size_t) db.n + 1);
    std::vector<char> text(textBytes + 1);
    rc = sd_host_kmermatch_format(db.n, db.keys.data(), nHits, rep.get(), member.get(), score.get(), diag.get(), entryKey.data(), entryOff.data(),
                                  textBytes, text.data(), &textBytes);
    if (rc != SD_OK) return fail("sd_host_kmermatch_format failed (" + std::to_string(rc) + ")");
    sddb::Writer out;
    if (!out.open(a.pos[1], sddb::DBTYPE_PREFILTER_RES, &err)) return fail(err);
    for (uint64_t e = 0; e < db.n; e++)
        if (!out.write(entryKey[e], text.data() + entryOff[e], (size_t) (entryOff[e + 1] - entryOff[e]))) return fail("cannot write " + a.pos[1]);
    if (!out.close(&err)) return fail(err);
    lap.mark("text and write");
    info(a, "Size of the sequence database: %u\nk-mer records: %llu, grouped: %llu, hits: %llu\n", db.n, (unsigned long long) stats[0],
         (unsigned long long) stats[1], (unsigned long long) stats[2]);
    return 0;
}

}  // namespace sdcli
