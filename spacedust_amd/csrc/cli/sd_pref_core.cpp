#include "sd_pref_core.h"

#include "../host/sd_target_build.h"

#include <cstdio>
#include <cstring>

namespace sdcli {

bool DbPair::open(const std::string &queryPath, const std::string &targetPath, sd_host *host, bool useResidentCache, bool rejectProfileTarget,
                  std::string *err) {
    sameDb = queryPath == targetPath;
    if (useResidentCache) {
        tdb = loadTargetDb(targetPath, host, err);
        if (!tdb) return false;
    } else {
        tdb.reset(new SeqDb());
        if (!tdb->load(targetPath, host, err)) return false;
    }
    if (rejectProfileTarget && tdb->profile) {
        *err = "profile target databases are not supported on this path";
        return false;
    }
    qdb = tdb.get();
    if (!sameDb) {
        qdbOwn.reset(new SeqDb());
        if (!qdbOwn->load(queryPath, host, err)) return false;
        qdb = qdbOwn.get();
    }
    return true;
}

int buildTarget(sd_host *host, sd_ctx *ctx, const PrefSetup &PS, const uint8_t *residues, const uint64_t *offsets, uint32_t n, sd_target **out,
                uint64_t st[2], const std::string &oomHint, const char *what) {
    const char *call = "";
    const int rc = sdBuildTarget(host, ctx, PS.k, PS.indexThr, PS.mask ? 1 : 0, PS.maskProb, residues, offsets, n, out, st, &call);
    if (rc == SD_OK) return 0;
    if (!strcmp(call, "sd_host_index_build")) return fail("sd_host_index_build failed (" + std::to_string(rc) + ")");
    if (!oomHint.empty() && (rc == SD_ENOMEM || strstr(sd_last_error(ctx), "out of memory"))) fprintf(stderr, "%s\n", oomHint.c_str());
    return failCtx(ctx, rc, !strcmp(call, "sd_target_build") ? what : call);
}

int QueryChunk::run(sd_ctx *ctx, sd_host *host, const sd_target *target, const sd_prefilter_params &par, const PrefSetup &PS, const QuerySpan &q,
                    const SeqDb &tdb, bool sameDb, uint64_t dbFrom, uint64_t dbSize, uint8_t *failed, uint64_t *stats) {
    const SeqDb &qd = *q.seqs;
    const uint32_t nq = q.n;
    const uint64_t r0 = qd.offsets[q.base], r1 = qd.offsets[q.base + nq];
    off.resize((size_t) nq + 1);
    for (uint32_t i = 0; i <= nq; i++) off[i] = qd.offsets[q.base + i] - r0;
    ident.resize(nq);
    for (uint32_t i = 0; i < nq; i++) {
        uint64_t id = UINT32_MAX;
        if (sameDb) id = q.g0 + i;
        else if (PS.includeIdentity) {
            const size_t t = tdb.rd.idOfKey(q.ids->keys[q.g0 + i]);
            if (t != SIZE_MAX) id = t;
        }
        // only the split that holds the query's own target gets the id, relative to dbFrom (Prefiltering.cpp:824-837)
        ident[i] = id != UINT32_MAX && id >= dbFrom && id < dbFrom + dbSize ? (uint32_t) (id - dbFrom) : UINT32_MAX;
    }
    hits.resize((size_t) nq * par.maxHitsPerQuery);
    counts.assign(nq, 0);
    if (stats) perQuery.resize((size_t) nq * 4);
    uint64_t *const pq = stats ? perQuery.data() : nullptr;
    int rc;
    if (qd.profile) {
        rc = sd_prefilter_profile_batch(ctx, target, &par, nq, qd.residues.data() + r0, off.data(), qd.sortedScore.data() + r0 * 20,
                                        qd.sortedIndex.data() + r0 * 20, qd.alnProfile.data() + r0 * 21, ident.data(), hits.data(), counts.data(),
                                        pq);
    } else {
        diagBias.assign(r1 - r0 + 1, 0);
        kmerBias.assign(r1 - r0 + 1, 0);
        if (PS.compBias) sd_host_comp_bias(host, qd.residues.data() + r0, off.data(), nq, PS.k, nullptr, diagBias.data(), kmerBias.data());
        rc = sd_prefilter_batch(ctx, target, &par, nq, qd.residues.data() + r0, off.data(), kmerBias.data(), diagBias.data(), ident.data(),
                                hits.data(), counts.data(), pq);
    }
    if (rc != SD_OK) return rc;
    for (uint32_t i = 0; i < nq; i++) {
        if (counts[i] != UINT32_MAX) continue;   // per-query error slot of the device call: not computed (reported, never silent)
        counts[i] = 0;
        if (failed && failed[i]) continue;
        if (failed) failed[i] = 1;
        if (!notComputed) firstError = sd_last_error(ctx);
        if (printEach && notComputed < 5)
            fprintf(stderr, "sdgpu prefilter: query %u was not computed: %s\n", q.ids->keys[q.g0 + i], sd_last_error(ctx));
        notComputed++;
    }
    if (stats) {
        for (uint32_t i = 0; i < nq; i++)
            for (int k = 0; k < 4; k++) stats[k] += perQuery[(size_t) i * 4 + k];
        stats[4] += r1 - r0;
    }
    return SD_OK;
}

int failNotComputed(uint64_t n, const char *whatBecameOfThem) {
    return fail(std::to_string(n) + " queries need the reference's double-overflow route (or have >= 2^32 index hits) and were " + whatBecameOfThem);
}

void appendPrefRow(std::string &text, uint32_t key, int score, int diagonal) {
    char line[64];
    // hit_t::diagonal is an unsigned short that the reference prints as a short: the low 16 bits of the value, signed
    const int len = snprintf(line, sizeof(line), "%u\t%d\t%d\n", key, score, (int) (int16_t) (uint16_t) diagonal);
    text.append(line, (size_t) len);
}

std::string residentTargetOf(const std::string &db, int device, bool erase) {
    if (!resident().enabled) return std::string();
    const std::string pfx = db + "|", suf = "|" + std::to_string(device);
    for (auto it = resident().targets.begin(); it != resident().targets.end(); ++it) {
        const std::string key = it->first;
        if (key.compare(0, pfx.size(), pfx) != 0 || key.size() < suf.size() || key.compare(key.size() - suf.size(), suf.size(), suf) != 0) continue;
        if (erase) {
            sd_target_destroy(it->second.t);
            resident().targets.erase(it);
        }
        return key;
    }
    return std::string();
}

int residentSeqSet(sd_ctx *ctx, const std::string &db, int device, const SeqDb &tdb, SeqSetH &out) {
    const std::string key = db + "|" + std::to_string(device);
    if (resident().enabled && resident().seqSets.count(key)) {
        out.s = resident().seqSets[key];   // the target sequences are on the device already
        out.own = false;
        resident().seqSetLog.push_back("reused " + db);
        return SD_OK;
    }
    const int rc = sd_seqset_create(ctx, tdb.residues.data(), tdb.offsets.data(), tdb.n, nullptr, &out.s);
    if (rc == SD_OK && resident().enabled) {
        resident().seqSets[key] = out.s;
        out.own = false;
        resident().seqSetLog.push_back("uploaded " + db);
    }
    return rc;
}

}  // namespace sdcli
