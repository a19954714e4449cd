// sd_r2p_realign: result2profile's own alignment of the rows that carry none (M/src/util/result2profile.cpp:224-233), as one batch
// through the library's Smith-Waterman passes.  No arithmetic of its own: the matrix and the composition bias are the host stages'
// (matrix 2: blosum62 at bit factor 2 with score bias -0.2), the alignment is sd_sw_align_batch.  DESIGN.md 4.19
#ifndef SD_HOST_STAGES_ONLY   // the CPU checker links the host stages without the device library
#include "sd_host.h"
#include "spacedust_gpu.h"

#include <cfloat>
#include <cstring>
#include <vector>

extern "C" int sd_r2p_realign(sd_ctx *ctx, sd_host *h, uint32_t nQ, const uint8_t *qLetters, const uint64_t *qOff, const uint64_t *edgeOff,
                              const uint32_t *edgeT, const uint8_t *edgeRealign, int32_t compBiasCorr, const sd_seqset *targets,
                              const uint8_t *tResidues, const uint64_t *tOff, uint32_t nT, int32_t *edgeQStart, int32_t *edgeTStart,
                              char *btPool, uint64_t btCap, uint64_t *btOff, uint64_t *btNeed, uint64_t *badEdge) {
    if (badEdge) *badEdge = UINT64_MAX;
    if (btNeed) *btNeed = 0;
    if (!ctx || !h || !qOff || !edgeOff || !tOff || !btOff || !btPool) return SD_EINVAL;
    if (nQ == 0) return SD_OK;
    if (!qLetters || !edgeT || !edgeQStart || !edgeTStart || (!targets && !tResidues)) return SD_EINVAL;
    const uint64_t nE = edgeOff[nQ];
    // the marked pairs, in edge order; every index is checked before anything reaches the device
    std::vector<uint32_t> pq, pt;
    std::vector<uint64_t> edgeOfPair;
    uint64_t kept = 0, bound = 64;
    for (uint32_t q = 0; q < nQ; q++) {
        if (edgeOff[q + 1] < edgeOff[q] || qOff[q + 1] < qOff[q]) return SD_EINVAL;
        for (uint64_t e = edgeOff[q]; e < edgeOff[q + 1]; e++) {
            if (btOff[e + 1] < btOff[e] || edgeT[e] >= nT) return SD_EINVAL;
            if (edgeRealign && !edgeRealign[e]) {
                kept += btOff[e + 1] - btOff[e];
                continue;
            }
            if (btOff[e + 1] != btOff[e]) return SD_EINVAL;
            pq.push_back(q);
            pt.push_back(edgeT[e]);
            edgeOfPair.push_back(e);
            bound += (qOff[q + 1] - qOff[q]) + (tOff[edgeT[e] + 1] - tOff[edgeT[e]]);
        }
    }
    if (btOff[nE] > btCap) return SD_EINVAL;
    if (btNeed) *btNeed = kept + bound;
    if (pq.empty()) return SD_OK;
    if (pq.size() > UINT32_MAX) return SD_EINVAL;

    sd_sw_params par;
    memset(&par, 0, sizeof(par));
    par.gapOpen = 11;
    par.gapExtend = 1;
    sd_host_matrix(h, 2, par.matrix, nullptr, nullptr);
    par.covMode = 0;
    par.covThr = 0.0f;
    par.evalThr = FLT_MAX;
    par.swMode = 2;
    par.dbResidues = tOff[nT];

    struct SetGuard {
        sd_seqset *s = nullptr;
        ~SetGuard() { if (s) sd_seqset_destroy(s); }
    } qset, tset;
    const uint64_t qTotal = qOff[nQ] - qOff[0];
    std::vector<uint8_t> qres(qTotal + 1, 0);
    std::vector<uint64_t> qo((size_t) nQ + 1);
    memcpy(qres.data(), qLetters + qOff[0], qTotal);
    for (uint32_t q = 0; q <= nQ; q++) qo[q] = qOff[q] - qOff[0];
    std::vector<int8_t> qbias(qTotal + 1, 0);
    if (compBiasCorr) {
        const int rcB = sd_host_sw_comp_bias(h, 2, qres.data(), qo.data(), nQ, qbias.data());
        if (rcB != SD_OK) return rcB;
    }
    int rc = sd_seqset_create(ctx, qres.data(), qo.data(), nQ, qbias.data(), &qset.s);
    if (rc != SD_OK) return rc;
    if (!targets) {
        rc = sd_seqset_create(ctx, tResidues, tOff, nT, nullptr, &tset.s);
        if (rc != SD_OK) return rc;
        targets = tset.s;
    }
    const uint32_t nP = (uint32_t) pq.size();
    std::vector<sd_sw_result> res(nP);
    // the batch writes behind the backtraces the pool holds (btOff[nE] == kept bytes); too small: SD_ENOMEM from the call, with its
    // message, and *btNeed says what suffices
    const uint64_t held = btOff[nE];
    uint64_t used = 0;
    rc = sd_sw_align_batch(ctx, &par, qset.s, targets, nP, pq.data(), pt.data(), nullptr, res.data(), btPool + held, btCap - held, &used);
    if (rc != SD_OK) return rc;
    uint64_t total = kept;
    for (uint32_t x = 0; x < nP; x++) {
        // run-length text instead of letters (sd_sw_set_cigar_pool on this context): not what the MSA reads
        if (((uint32_t) res[x].flags >> 8) != 0) return SD_EUNSUPPORTED;
        if (res[x].score <= 0 || res[x].qStart < 0 || res[x].tStart < 0 || res[x].btLen <= 0) {
            if (badEdge) *badEdge = edgeOfPair[x];
            return SD_EINVAL;
        }
        if (res[x].btOffset + (uint64_t) res[x].btLen > used) return SD_EINVAL;
        total += (uint64_t) res[x].btLen;
    }
    if (total > held + used) return SD_EINVAL;   // (backtraces of one call do not overlap: the merged pool is no larger than what is there)
    // every edge's backtrace in edge order, assembled beside the pool (its exact size) and copied back
    std::vector<char> merged(total);
    std::vector<uint64_t> oldOff(btOff, btOff + nE + 1);
    uint64_t w = 0, x = 0;
    for (uint64_t e = 0; e < nE; e++) {
        btOff[e] = w;
        if (x < nP && edgeOfPair[x] == e) {
            memcpy(merged.data() + w, btPool + held + res[x].btOffset, (size_t) res[x].btLen);
            w += (uint64_t) res[x].btLen;
            edgeQStart[e] = res[x].qStart;
            edgeTStart[e] = res[x].tStart;
            x++;
        } else {
            memcpy(merged.data() + w, btPool + oldOff[e], (size_t) (oldOff[e + 1] - oldOff[e]));
            w += oldOff[e + 1] - oldOff[e];
        }
    }
    memcpy(btPool, merged.data(), (size_t) w);
    btOff[nE] = w;
    return SD_OK;
}
#endif
