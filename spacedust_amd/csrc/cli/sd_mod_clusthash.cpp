// clusthash <sequenceDB> <resultDB>  (M/src/util/clusthash.cpp): sequences of equal hash over a reduced alphabet and of equal length are
// compared byte for byte; the alignment DB holds, per sequence, its self row and the sequences it marked at --min-seq-id.  Hash, sort and
// the greedy pass over the groups run on the GPU (sd_clusthash_batch); the reduced alphabet, the threshold per length and the text are
// host stages (sd_host_reduced_alphabet, sd_host_clusthash_min_identical, sd_host_clusthash_format).  Amino-acid sequence DBs that fit
// the device at once.  --sub-mat (blosum62), --alph-size (default 3), --min-seq-id (default 0.99), --threads, -v and --device are used;
// --max-seq-len is accepted and has no effect, as in the reference (Sequence::mapSequence(const char *, unsigned) does not cut).
#include "sd_cli.h"

#include <cstdlib>
#include <cstring>

namespace sdcli {

int clusthashModule(const Args &a) {
    if (a.pos.size() != 2) return fail("usage: clusthash <sequenceDB> <resultDB> [options]");
    if (int rc = checkCommon(a)) return rc;
    Lap lap("clusthash");
    std::string err;
    {
        sddb::Reader probe;
        if (!probe.open(a.pos[0], sddb::Reader::USE_INDEX, sddb::Reader::NOSORT, &err)) return fail(err);
        const int bt = sddb::baseType(probe.dbtype());
        if (bt == sddb::DBTYPE_NUCLEOTIDES) return fail("nucleotide DBs are not implemented (" + a.pos[0] + ")");
        if (bt == sddb::DBTYPE_HMM_PROFILE) return fail("profile DBs are not implemented (" + a.pos[0] + ")");
    }
    sd_clusthash_params par;
    memset(&par, 0, sizeof(par));
    par.alphabetSize = atoi(a.multi("--alph-size", "aa", "3").c_str());
    par.seqIdThr = (float) a.real("--min-seq-id", 0.99);
    // (the reference refuses 21 itself: its ReducedMatrix wants an alphabet smaller than the full one)
    if (par.alphabetSize != 3 && par.alphabetSize != 13)
        return fail("--alph-size " + std::to_string(par.alphabetSize) + ": 3 and 13 are implemented");
    HostH host;
    if (host.open(threadsOf(a)) != SD_OK) return fail("sd_host_create failed");
    SeqDb db;
    if (!db.load(a.pos[0], host.h, &err)) return fail(err);
    if (db.profile) return fail("profile DBs are not implemented (" + a.pos[0] + ")");
    // the DB's own bytes, laid out like the residues: the comparison is case sensitive
    std::vector<uint8_t> letters(db.totalResidues() ? db.totalResidues() : 1);
#pragma omp parallel for schedule(static)
    for (uint32_t i = 0; i < db.n; i++) memcpy(letters.data() + db.offsets[i], db.rd.data(i), (size_t) db.lens[i]);
    lap.mark("open");
    uint8_t letterMap[21];
    int reduced = 0;
    if (sd_host_reduced_alphabet(0, par.alphabetSize, letterMap, &reduced) != SD_OK || reduced != par.alphabetSize)
        return fail("sd_host_reduced_alphabet failed");
    lap.mark("letter map");
    CtxH ctx;
    int rc = ctx.open(deviceOf(a));
    if (rc != SD_OK) return failNoDevice(rc, "sd_ctx_create", "clusthash hashes, sorts and compares on the GPU (there is no CPU fallback)");
    lap.mark("context");
    const bool timing = getenv("SD_DEBUG_TIMING") != nullptr;
    if (timing) sd_profile_enable(ctx.c, 1);
    info(a, "Hashing sequences...\n");
    uint64_t stats[4] = {0, 0, 0, 0};
    std::vector<uint32_t> foundBy(db.n ? db.n : 1), identical(db.n ? db.n : 1);
    rc = sd_clusthash_batch(ctx.c, &par, db.n, db.residues.data(), db.offsets.data(), letters.data(), letterMap, foundBy.data(), identical.data(),
                            nullptr, stats);
    if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_clusthash_batch");
    info(a, "Found %llu unique hashes\n", (unsigned long long) stats[0]);
    if (timing) {
        static const char *const stage[] = {"ch_prepare", "ch_alloc", "ch_copy_in", "ch_hash", "ch_sort", "ch_groups", "ch_pass", "ch_copy_out"};
        fprintf(stderr, "[clusthash] device:");
        for (const char *s : stage) {
            double ms = 0;
            uint64_t calls = 0;
            sd_profile_get(ctx.c, (std::string("host:") + s).c_str(), &ms, &calls);
            fprintf(stderr, " %s %.3f ms", s + 3, ms);
        }
        fprintf(stderr, "; %llu groups, %llu pairs compared, largest group %llu\n", (unsigned long long) stats[1], (unsigned long long) stats[2],
                (unsigned long long) stats[3]);
    }
    lap.mark("device");
    uint64_t textBytes = 0;
    rc = sd_host_clusthash_format(db.n, db.keys.data(), db.offsets.data(), foundBy.data(), identical.data(), nullptr, 0, nullptr, &textBytes);
    if (rc != SD_OK) return fail("sd_host_clusthash_format failed (" + std::to_string(rc) + ")");
    std::vector<uint64_t> entryOff((size_t) db.n + 1);
    std::vector<char> text(textBytes + 1);
    rc = sd_host_clusthash_format(db.n, db.keys.data(), db.offsets.data(), foundBy.data(), identical.data(), entryOff.data(), textBytes, text.data(),
                                  &textBytes);
    if (rc != SD_OK) return fail("sd_host_clusthash_format failed (" + std::to_string(rc) + ")");
    sddb::Writer out;
    if (!out.open(a.pos[1], sddb::DBTYPE_ALIGNMENT_RES, &err)) return fail(err);
    for (uint64_t e = 0; e < db.n; e++)
        if (!out.write(db.keys[e], text.data() + entryOff[e], (size_t) (entryOff[e + 1] - entryOff[e]))) return fail("cannot write " + a.pos[1]);
    if (!out.close(&err)) return fail(err);
    lap.mark("text and write");
    return 0;
}

}  // namespace sdcli
