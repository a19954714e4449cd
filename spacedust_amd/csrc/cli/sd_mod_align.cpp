// align <queryDB> <targetDB> <prefDB> <alnDB>        (M/src/alignment/Main.cpp:12, Alignment.cpp:244-542): DB in, C ABI of libsdgpu.so
// (HIP kernels) in the middle, DB out.  No compute here, no CPU fallback.
#include "sd_align_core.h"
#include "sd_pref_core.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

namespace sdcli {

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
    DbPair db;
    if (!db.open(a.pos[0], a.pos[1], host.h, true, true, &err)) return fail(err);
    const bool sameDb = db.sameDb;
    const SeqDb *const qdb = db.qdb, *const tdb = db.tdb.get();
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
    if (rc != SD_OK) return failNoDevice(rc);

    SeqSetH tset;
    rc = residentSeqSet(ctx.c, a.pos[1], deviceOf(a), *tdb, tset);
    if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create(targets)");

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

}  // namespace sdcli
