// clust <sequenceDB> <resultDB> <clusterDB>  (M/src/clustering/Main.cpp, Clustering.cpp:11-266): a result DB of a set against itself -> a
// cluster DB.  The lines are parsed and the algorithms run on the host (sd_host_clust_*); the symmetric graph the set cover and the
// connected component read is built on the GPU (sd_clust_symmetrize).  Parameter set `clust` (Parameters.cpp:490-500): --cluster-mode,
// --max-iterations, --similarity-type, --threads, -v are used; --set-mode 1, --weights and --compressed 1 are refused by name.
#include "sd_cli.h"

#include <cstdlib>
#include <cstring>

namespace sdcli {

int clustModule(const Args &a) {
    if (a.pos.size() != 3) return fail("usage: clust <sequenceDB> <resultDB> <clusterDB> [options]");
    if (int rc = checkCommon(a)) return rc;
    if (a.flag("--set-mode", false)) return fail("--set-mode 1 (clustering by set) is not implemented");
    if (!a.str("--weights", "").empty()) return fail("--weights (cluster priorization by a weight file) is not implemented");
    const int mode = (int) a.integer("--cluster-mode", 0);
    if (mode < 0 || mode > 3) return fail("Wrong clustering mode!");
    const int maxIterations = (int) a.integer("--max-iterations", 1000);
    if (maxIterations < 1) return fail("--max-iterations must be at least 1");
    const int similarityType = (int) a.integer("--similarity-type", 2);
    if (similarityType != 1 && similarityType != 2) return fail("--similarity-type is 1 (alignment score) or 2 (sequence identity)");
    Lap lap("clust");
    std::string err;
    sddb::Reader seq, res;
    if (!seq.open(a.pos[0], sddb::Reader::USE_INDEX, sddb::Reader::NOSORT, &err)) return fail(err);
    if (!res.open(a.pos[1], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::NOSORT, &err)) return fail(err);
    if (seq.size() != res.size()) return fail("Sequence db size != result db size");
    if (sddb::isCompressed(res.dbtype())) return fail("a compressed result DB is not supported");
    const uint64_t n = seq.size();
    if (n > (uint64_t) UINT32_MAX - 1) return fail("more than 2^32 - 2 sequences");
    // local ids: DBReader::SORT_BY_LENGTH
    std::vector<uint64_t> indexLength(n);
    for (uint64_t i = 0; i < n; i++) indexLength[i] = seq.entryLength(i);
    std::vector<uint32_t> localToId(n), localKeys(n);
    if (sd_host_clust_order(n, indexLength.data(), localToId.data()) != SD_OK) return fail("sd_host_clust_order failed");
    std::vector<const char *> entries(n);
    for (uint64_t i = 0; i < n; i++) {
        localKeys[i] = seq.key(localToId[i]);
        const size_t id = res.idOfKey(localKeys[i]);
        if (id == SIZE_MAX) return fail("sequence " + std::to_string(localKeys[i]) + " has no entry in " + a.pos[1]);
        entries[i] = res.entryLength(id) ? res.data(id) : "";
    }
    lap.mark("open DBs");
    std::vector<uint64_t> rowOff(n + 1);
    uint32_t badKey = 0;
    int rc = sd_host_clust_parse(n, localKeys.data(), entries.data(), res.dbtype(), similarityType, rowOff.data(), 0, nullptr, nullptr, &badKey);
    if (rc == SD_EUNSUPPORTED) return fail("Alignment format is not supported!");
    if (rc != SD_OK) return fail("sd_host_clust_parse failed (" + std::to_string(rc) + ")");
    const uint64_t nEdges = rowOff[n];
    std::vector<uint32_t> elem(nEdges ? nEdges : 1);
    std::vector<uint16_t> score(nEdges ? nEdges : 1);
    rc = sd_host_clust_parse(n, localKeys.data(), entries.data(), res.dbtype(), similarityType, rowOff.data(), nEdges, elem.data(), score.data(), &badKey);
    if (rc == SD_EINVAL)
        return fail("Element " + std::to_string(badKey) + " contained in some alignment list, but not contained in the sequence database!");
    if (rc != SD_OK) return fail("sd_host_clust_parse failed (" + std::to_string(rc) + ")");
    lap.mark("parse");
    std::vector<uint32_t> assigned(n ? n : 1);
    if (mode >= 2) {
        info(a, "Clustering mode: Greedy Low Mem\n");
        if (sd_host_clust_greedy(n, rowOff.data(), elem.data(), assigned.data()) != SD_OK) return fail("sd_host_clust_greedy failed");
    } else {
        CtxH ctx;
        rc = ctx.open(deviceOf(a));
        if (rc != SD_OK) return failNoDevice(rc, "sd_ctx_create", "--cluster-mode 0 and 1 build their graph on the GPU (there is no CPU fallback)");
        lap.mark("context");
        const bool timing = getenv("SD_DEBUG_TIMING") != nullptr;
        if (timing) sd_profile_enable(ctx.c, 1);
        uint64_t stats[3] = {0, 0, 0};
        // (an input entry adds at most one: room for twice the entries, one call)
        const uint64_t cap = 2 * nEdges;
        std::vector<uint64_t> symOff(n + 1, 0);
        std::unique_ptr<uint32_t[]> symElemBuf(new uint32_t[cap ? cap : 1]);
        std::unique_ptr<uint16_t[]> symScoreBuf(new uint16_t[cap ? cap : 1]);
        uint32_t *const symElem = symElemBuf.get();
        uint16_t *const symScore = symScoreBuf.get();
        rc = sd_clust_symmetrize(ctx.c, n, rowOff.data(), elem.data(), score.data(), cap, symOff.data(), symElem, symScore, stats);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_clust_symmetrize");
        if (timing) {
            double msIn = 0, msKernels = 0, msOut = 0;
            uint64_t calls = 0;
            sd_profile_get(ctx.c, "host:clust_copy_in", &msIn, &calls);
            sd_profile_get(ctx.c, "host:clust_kernels", &msKernels, &calls);
            sd_profile_get(ctx.c, "host:clust_copy_out", &msOut, &calls);
            fprintf(stderr, "[clust] device: copy in %.3f ms, kernels %.3f ms, copy out %.3f ms; %llu entries in, %llu added, largest row %llu\n", msIn, msKernels,
                    msOut, (unsigned long long) stats[0], (unsigned long long) stats[1], (unsigned long long) stats[2]);
        }
        info(a, "Found %llu new connections.\n", (unsigned long long) stats[1]);
        lap.mark("symmetric graph");
        if (mode == 0) {
            info(a, "Clustering mode: Set Cover\n");
            rc = sd_host_clust_setcover(n, symOff.data(), symElem, symScore, assigned.data());
        } else {
            info(a, "Clustering mode: Connected Component\n");
            rc = sd_host_clust_connected(n, symOff.data(), symElem, maxIterations, assigned.data());
        }
        if (rc != SD_OK) return fail("the clustering algorithm failed (" + std::to_string(rc) + ")");
    }
    lap.mark("algorithm");
    std::vector<uint32_t> repKey(n ? n : 1), memberKey(n ? n : 1), entryKey(n ? n : 1);
    std::vector<uint64_t> entryOff(n + 1);
    std::vector<char> text(22 * n + 1);
    uint64_t nEntries = 0;
    if (sd_host_clust_format(n, localKeys.data(), assigned.data(), repKey.data(), memberKey.data(), &nEntries, entryKey.data(), entryOff.data(),
                             text.data()) != SD_OK)
        return fail("sd_host_clust_format failed");
    for (uint64_t i = 0; i < n; i++)
        if (assigned[i] == UINT32_MAX)
            fprintf(stderr, "there must be an error: %u\t%llu\tis not assigned to a cluster\n", localKeys[i], (unsigned long long) i);
    sddb::Writer out;
    if (!out.open(a.pos[2], sddb::DBTYPE_CLUSTER_RES, &err)) return fail(err);
    for (uint64_t e = 0; e < nEntries; e++)
        if (!out.write(entryKey[e], text.data() + entryOff[e], (size_t) (entryOff[e + 1] - entryOff[e]))) return fail("cannot write " + a.pos[2]);
    if (!out.close(&err)) return fail(err);
    lap.mark("write");
    info(a, "Size of the sequence database: %llu\nNumber of clusters: %llu\n", (unsigned long long) n, (unsigned long long) nEntries);
    return 0;
}

}  // namespace sdcli
