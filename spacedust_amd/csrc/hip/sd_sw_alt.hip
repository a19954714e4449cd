// Alternative alignments (`align --alt-ali N`): Alignment::computeAlternativeAlignment (M/src/alignment/Alignment.cpp:569-601)
// for a batch of seeds.  The Smith-Waterman work of a round is the existing batch path (sd_sw_align_batch / _compact) on a
// scratch target set; this file holds what happens between two rounds, all of it on the device:
//   k_alt_lengths    lengths of the scratch set's sequences for the seeds still alive (a dead seed's copy is empty)
//   k_alt_mask_copy  one copy of the target per live seed with every interval so far overwritten by X
//   k_alt_accept     Alignment::checkCriteria on the round's records: count, next interval, liveness
//   k_alt_compact    the live seeds, compacted, as the next round's work list of k_alt_mask_copy
// The host reads one number per round, the count of live seeds, to know when a group of seeds is finished.
//
// Scratch layout: slot g of a group owns sequences 2g and 2g + 1 of the scratch set: the masked copy (tLen
// residues) and a filler of (4 - tLen % 4) % 4 residues that no pair refers to.  Every copy therefore starts on a dword, the
// mask kernel writes whole dwords and two slots never share one.  The pair list of a group is fixed, (seedQ[g], 2g): a dead
// seed's pair meets an empty target and the batch path makes no task for it (k_make_fwd).
#include "sd_common.h"

#include <cfloat>
#include <cstdlib>

namespace {

#include "sd_scan_sort.h"

constexpr uint32_t X_CODE4 = 0x14141414u;   // four residues X (code 20; Sequence.cpp:307-324)

struct AltCrit {   // Alignment::checkCriteria's arguments and what Matcher::getSWResult derives its inputs with
    double evalThr;
    float seqIdThr, covThr;
    int alnLenThr, covMode, seqIdMode, swMode;
};

__global__ void __launch_bounds__(256)
k_alt_init(uint32_t G, uint32_t stride, const int32_t *__restrict__ tStart, const int32_t *__restrict__ tEnd, int2 *__restrict__ ivl,
           uint32_t *__restrict__ nIvl, uint8_t *__restrict__ live, uint32_t *__restrict__ liveList, uint32_t *__restrict__ cnt) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    ivl[(size_t) g * stride] = make_int2(tStart[g], tEnd[g]);
    nIvl[g] = 1;
    live[g] = 1;
    liveList[g] = g;
    cnt[g] = 0;
}

__global__ void __launch_bounds__(256)
k_alt_lengths(uint32_t G, const uint32_t *__restrict__ seedT, const uint64_t *__restrict__ tOff, const uint8_t *__restrict__ live,
              uint32_t *__restrict__ len /* 2G + 1 */) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > G) return;
    if (g == G) {
        len[2 * (size_t) G] = 0;
        return;
    }
    const uint32_t t = seedT[g];
    const uint32_t L = live[g] ? (uint32_t) (tOff[t + 1] - tOff[t]) : 0u;
    len[2 * (size_t) g] = L;
    len[2 * (size_t) g + 1] = (4u - (L & 3u)) & 3u;
}

// ones in the low n bytes, n = 0 .. 4
__device__ __forceinline__ uint32_t lowBytes(int n) { return n >= 4 ? 0xFFFFFFFFu : ((1u << (8 * n)) - 1u); }

// One wavefront per live seed, a lane per destination dword.  The source starts at any byte: a lane reads the two aligned dwords
// around its four residues and v_alignbyte_b32 joins them (the source set ends in 64 bytes of padding, and its buffer starts
// aligned, so both reads stay inside it).  The masks are byte selects: per interval the bytes [s - p, e - p) of the dword at target
// position p, clamped to [0, 4], become a bit mask and v_bfi_b32 picks X under it -- no branch depends on a residue or a byte.
// The interval count is the same for the whole wavefront (one seed), so its loop is uniform.  The bytes behind the last residue
// of a copy land in the slot's filler sequence.
__global__ void __launch_bounds__(256)
k_alt_mask_copy(const uint32_t *__restrict__ nLivePtr, const uint32_t *__restrict__ liveList, const uint32_t *__restrict__ seedT,
                const uint64_t *__restrict__ tOff, const uint8_t *__restrict__ tRes, const uint64_t *__restrict__ sOff, uint32_t stride,
                const int2 *__restrict__ ivl, const uint32_t *__restrict__ nIvl, uint8_t *__restrict__ scratch) {
    const uint32_t nLive = *nLivePtr;
    const int lane = threadIdx.x & 63;
    for (uint32_t x = blockIdx.x * 4 + (threadIdx.x >> 6); x < nLive; x += gridDim.x * 4) {
        const uint32_t g = liveList[x];
        const uint32_t t = seedT[g];
        const uint64_t so = tOff[t];
        const int L = (int) (tOff[t + 1] - so);
        const int nd = (L + 3) >> 2;
        const int k = (int) nIvl[g];
        const int2 *iv = ivl + (size_t) g * stride;
        uint32_t *dst = (uint32_t *) (scratch + sOff[2 * (size_t) g]);   // a multiple of 4 by construction
        for (int w = lane; w < nd; w += 64) {
            const int p = 4 * w;
            const uint64_t a = (uint64_t) (uintptr_t) tRes + so + (uint64_t) p;
            const uint32_t *al = (const uint32_t *) (uintptr_t) (a & ~(uint64_t) 3);
            const uint32_t lo = al[0], hi = al[1];
            uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t) a & 3u);
            uint32_t m = 0;
            for (int j = 0; j < k; j++) {
                const int2 se = iv[j];
                const int b0 = min(max(se.x - p, 0), 4), b1 = min(max(se.y - p, 0), 4);
                m |= lowBytes(b1) & ~lowBytes(b0);
            }
            dst[w] = (X_CODE4 & m) | (v & ~m);
        }
    }
}

__device__ __forceinline__ float altCov(uint32_t startPos, uint32_t endPos, uint32_t len) {   // Util::computeCov
    return (float) (min(len, max(startPos, endPos)) - min(startPos, endPos) + 1u) / (float) len;
}

// Alignment::checkCriteria (Alignment.cpp:548-567) on a record of the batch path, with the fields Matcher::getSWResult derives
// (Matcher.cpp:88-126): the rule sd_sw_align_batch_best_by_group evaluates (bbAccepted, sd_sw.hip), extended by the alignment mode
// without a backtrace and by --seq-id-mode.  The record's E-value is the device's (relative error ~1e-15): a result within 1e-9 of
// the threshold passes here and the host, which has the exact value, ends the seed there.
__device__ bool altAccepted(const sd_sw_result &r, const AltCrit &c, uint32_t qL, uint32_t tL) {
    if (r.tEnd < 0 || r.qStart < 0 || r.tStart < 0) return false;   // stopped at the E-value or the coverage gate
    const uint32_t qS = (uint32_t) r.qStart, qE = (uint32_t) r.qEnd, tS = (uint32_t) r.tStart, tE = (uint32_t) r.tEnd;
    const float qcov = altCov(qS, qE, qL), dbcov = altCov(tS, tE, tL);
    uint32_t alnLength = (uint32_t) max(abs(r.qEnd - r.qStart), abs(r.tEnd - r.tStart)) + 1u;   // Matcher::computeAlnLength
    float seqId;
    if (c.swMode == 2) {
        if (r.btLen <= 0) return false;
        alnLength = (uint32_t) r.btLen;
        const uint32_t den = c.seqIdMode == 1 ? min(qL, tL) : (c.seqIdMode == 2 ? max(qL, tL) : alnLength);   // Util::computeSeqId
        seqId = (float) r.identical / (float) den;
    } else {   // Matcher::estimateSeqIdByScorePerCol: the score enters as uint16_t
        const uint32_t qAln = max(qE - qS, 1u), tAln = max(tE - tS, 1u);
        float e = (float) (((uint16_t) r.score / (float) max(qAln, tAln)) * 0.1656 + 0.1141);
        e = fminf(e, 1.0f);
        seqId = fmaxf(0.0f, e);
    }
    bool cov = true;
    if (c.covMode == 0) cov = qcov >= c.covThr && dbcov >= c.covThr;
    else if (c.covMode == 2) cov = qcov >= c.covThr;
    else if (c.covMode == 1) cov = dbcov >= c.covThr;
    return r.evalue <= c.evalThr * (1.0 + 1e-9) && seqId >= c.seqIdThr && cov && alnLength >= (uint32_t) c.alnLenThr;
}

__global__ void __launch_bounds__(256)
k_alt_accept(uint32_t G, uint32_t stride, AltCrit crit, const sd_sw_result *__restrict__ res, const uint32_t *__restrict__ seedQ,
             const uint32_t *__restrict__ seedT, const uint64_t *__restrict__ qOff, const uint64_t *__restrict__ tOff,
             int2 *__restrict__ ivl, uint32_t *__restrict__ nIvl, uint8_t *__restrict__ live, uint32_t *__restrict__ cnt) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > G) return;
    if (g == G) {   // the scan's last input
        live[G] = 0;
        return;
    }
    if (!live[g]) return;
    const uint32_t q = seedQ[g], t = seedT[g];
    const sd_sw_result r = res[g];
    if (altAccepted(r, crit, (uint32_t) (qOff[q + 1] - qOff[q]), (uint32_t) (tOff[t + 1] - tOff[t]))) {
        cnt[g] += 1;
        const uint32_t k = nIvl[g];
        if (k < stride) {   // (the last round's interval masks nothing any more)
            ivl[(size_t) g * stride + k] = make_int2(r.tStart, r.tEnd);
            nIvl[g] = k + 1;
        }
    } else {
        live[g] = 0;
    }
}

__global__ void __launch_bounds__(256)
k_alt_compact(uint32_t G, const uint8_t *__restrict__ live, const uint64_t *__restrict__ pos, uint32_t *__restrict__ liveList,
              uint32_t *__restrict__ nLive) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > G) return;
    if (g == G) {
        *nLive = (uint32_t) pos[G];
        return;
    }
    if (live[g]) liveList[pos[g]] = g;
}

// A target set that exists on the device only: what the batch path needs of targets that are never identity pairs (see
// alignBatchImpl, sd_sw.hip).  No host copies, no bias, no profile; the buffers stay the caller's.
void sdDeviceSeqView(sd_seqset &v, sd_ctx *ctx, uint32_t n, uint8_t *dRes, uint64_t *dOff) {
    v.ctx = ctx;
    v.n = n;
    v.dRes = dRes;
    v.dOff = dOff;
}

struct RoundRecords {   // what a round's batch call brought back: records of the slots idx[], their backtraces from poolBase on
    std::vector<uint32_t> idx;
    std::vector<sd_sw_result> rec;
    uint64_t poolBase = 0;
};

}  // namespace

extern "C" {

int sd_sw_alt_last_stats(sd_ctx *ctx, uint64_t *groups, uint64_t *seedRounds, uint64_t *bytesCopied) {
    if (!ctx) return SD_EINVAL;
    if (groups) *groups = ctx->altGroups;
    if (seedRounds) *seedRounds = ctx->altSeedRounds;
    if (bytesCopied) *bytesCopied = ctx->altBytes;
    return SD_OK;
}

int sd_sw_align_alt_batch(sd_ctx *ctx, const sd_sw_params *par, const sd_seqset *queries, const sd_seqset *targets, uint32_t nSeeds,
                          const uint32_t *seedQ, const uint32_t *seedT, const int32_t *tStart, const int32_t *tEnd,
                          const uint8_t *isIdentity, uint32_t maxAlt, float seqIdThr, int32_t alnLenThr, int32_t seqIdMode,
                          sd_sw_result *out, uint32_t *outCount, char *btPool, uint64_t btCap, uint64_t *btUsed) {
    if (!ctx || !par || !queries || !targets || !outCount || (nSeeds && (!seedQ || !seedT || !tStart || !tEnd || !out))) return SD_EINVAL;
    if (btUsed) *btUsed = 0;
    ctx->altGroups = ctx->altSeedRounds = ctx->altBytes = 0;
    if (maxAlt == 0 || maxAlt > 4096) return sdFail(ctx, SD_EINVAL, "sd_sw_align_alt_batch: maxAlt must be 1 .. 4096");
    if (par->swMode != 1 && par->swMode != 2)
        return sdFail(ctx, SD_EINVAL, "sd_sw_align_alt_batch: swMode 1 or 2 (the masks need start positions, Alignment.cpp:88)");
    if (targets->dProf) return sdFail(ctx, SD_EUNSUPPORTED, "profile targets are not implemented (profile queries are)");
    if (par->swMode == 2 && !btPool) return sdFail(ctx, SD_EINVAL, "swMode 2 needs a backtrace pool");
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    // the seeds that take part, in order (identity seeds are skipped, Alignment.cpp:574-577)
    std::vector<uint32_t> sIdx, sQ, sT;
    std::vector<int32_t> sB, sE;
    sIdx.reserve(nSeeds);
    for (uint32_t s = 0; s < nSeeds; s++) {
        outCount[s] = 0;
        if (seedQ[s] >= queries->n || seedT[s] >= targets->n) return sdFail(ctx, SD_EINVAL, "seed %u out of range", s);
        const int64_t tL = (int64_t) (targets->hOff[seedT[s] + 1] - targets->hOff[seedT[s]]);
        if (tStart[s] < 0 || tEnd[s] < tStart[s] || tEnd[s] >= tL)
            return sdFail(ctx, SD_EINVAL, "seed %u: target positions [%d, %d] outside a target of %lld residues", s, tStart[s], tEnd[s], (long long) tL);
        if (isIdentity && isIdentity[s]) continue;
        sIdx.push_back(s);
    }
    const size_t nS = sIdx.size();
    sQ.resize(nS); sT.resize(nS); sB.resize(nS); sE.resize(nS);
    for (size_t x = 0; x < nS; x++) {
        sQ[x] = seedQ[sIdx[x]]; sT[x] = seedT[sIdx[x]]; sB[x] = tStart[sIdx[x]]; sE[x] = tEnd[sIdx[x]];
    }
    sd_sw_params p = *par;
    p.evalThr = (double) (float) par->evalThr;   // computeAlternativeAlignment(..., float evalThr, ...)
    AltCrit crit;
    crit.evalThr = p.evalThr; crit.seqIdThr = seqIdThr; crit.covThr = p.covThr; crit.alnLenThr = alnLenThr; crit.covMode = p.covMode;
    crit.seqIdMode = seqIdMode; crit.swMode = p.swMode;
    // the last round's interval is never used: maxAlt intervals per seed (the seed's own and maxAlt - 1 alternatives)
    const uint32_t stride = maxAlt;
    uint64_t budget = 256ull << 20;
    if (const char *e = getenv("SD_ALT_BUDGET")) budget = std::max<uint64_t>(4096, strtoull(e, nullptr, 10));   // tests: force several groups
    const uint64_t perSeedState = (uint64_t) stride * sizeof(int2) + 64;   // intervals, offsets, flags, counters
    const bool compact = p.swMode == 2;
    uint64_t poolUsed = 0;
    std::vector<uint32_t> pairT, hCnt, have;
    std::vector<RoundRecords> rounds;
    std::vector<uint32_t> tmpIdx;
    std::vector<sd_sw_result> tmpRec;
    for (size_t g0 = 0; g0 < nS;) {
        // a group: as many seeds as the budget holds copies (rounded up to dwords) and per-seed state for; at least one
        size_t g1 = g0;
        uint64_t bytes = 0;
        while (g1 < nS && g1 - g0 < (1u << 30)) {
            const uint64_t tL = targets->hOff[sT[g1] + 1] - targets->hOff[sT[g1]];
            const uint64_t need = ((tL + 3) & ~3ull) + perSeedState;
            if (g1 > g0 && bytes + need > budget) break;
            bytes += need;
            g1++;
        }
        const uint32_t G = (uint32_t) (g1 - g0);
        const uint64_t scratchBytes = bytes - (uint64_t) G * perSeedState;
        ctx->altGroups++;
        const unsigned grid = (G + 1 + 255) / 256;
        uint32_t *dSeedQ = nullptr, *dSeedT = nullptr, *dNIvl = nullptr, *dLiveList = nullptr, *dCnt = nullptr, *dLen = nullptr, *dNLive = nullptr;
        int32_t *dB = nullptr, *dE = nullptr;
        int2 *dIvl = nullptr;
        uint8_t *dLive = nullptr, *dScratch = nullptr;
        uint64_t *dSOff = nullptr, *dPos = nullptr;
        SD_HIP(ctx, wsGet(ctx, "alt.seedq", G, &dSeedQ));
        SD_HIP(ctx, wsGet(ctx, "alt.seedt", G, &dSeedT));
        SD_HIP(ctx, wsGet(ctx, "alt.tstart", G, &dB));
        SD_HIP(ctx, wsGet(ctx, "alt.tend", G, &dE));
        SD_HIP(ctx, wsGet(ctx, "alt.ivl", (size_t) G * stride, &dIvl));
        SD_HIP(ctx, wsGet(ctx, "alt.nivl", G, &dNIvl));
        SD_HIP(ctx, wsGet(ctx, "alt.live", (size_t) G + 1, &dLive));
        SD_HIP(ctx, wsGet(ctx, "alt.livelist", G, &dLiveList));
        SD_HIP(ctx, wsGet(ctx, "alt.count", G, &dCnt));
        SD_HIP(ctx, wsGet(ctx, "alt.len", 2 * (size_t) G + 1, &dLen));
        SD_HIP(ctx, wsGet(ctx, "alt.soff", 2 * (size_t) G + 1, &dSOff));
        SD_HIP(ctx, wsGet(ctx, "alt.pos", (size_t) G + 1, &dPos));
        SD_HIP(ctx, wsGet(ctx, "alt.nlive", 4, &dNLive));
        SD_HIP(ctx, wsGet(ctx, "alt.scratch", scratchBytes + 64, &dScratch));
        SD_HIP(ctx, hipMemcpyAsync(dSeedQ, sQ.data() + g0, (size_t) G * 4, hipMemcpyHostToDevice, ctx->stream));
        SD_HIP(ctx, hipMemcpyAsync(dSeedT, sT.data() + g0, (size_t) G * 4, hipMemcpyHostToDevice, ctx->stream));
        SD_HIP(ctx, hipMemcpyAsync(dB, sB.data() + g0, (size_t) G * 4, hipMemcpyHostToDevice, ctx->stream));
        SD_HIP(ctx, hipMemcpyAsync(dE, sE.data() + g0, (size_t) G * 4, hipMemcpyHostToDevice, ctx->stream));
        SD_HIP(ctx, hipMemcpyAsync(dNLive, &G, 4, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_alt_init, dim3(grid), dim3(256), 0, ctx->stream, G, stride, (const int32_t *) dB, (const int32_t *) dE, dIvl, dNIvl,
                           dLive, dLiveList, dCnt);
        if (pairT.size() < G) {
            pairT.resize(G);
            for (uint32_t g = 0; g < G; g++) pairT[g] = 2 * g;
        }
        sd_seqset scratch;
        sdDeviceSeqView(scratch, ctx, 2 * G, dScratch, dSOff);
        rounds.clear();
        uint32_t nLive = G;
        for (uint32_t round = 0; round < maxAlt && nLive > 0; round++) {
            uint64_t copied = 0;
            {
                ProfScope ps(ctx, "alt_mask_copy");
                hipLaunchKernelGGL(k_alt_lengths, dim3(grid), dim3(256), 0, ctx->stream, G, (const uint32_t *) dSeedT,
                                   (const uint64_t *) targets->dOff, (const uint8_t *) dLive, dLen);
                const int rcS = sdCtxExclusiveScan(ctx, "alt.scantmp", (const uint32_t *) dLen, dSOff, 2 * (size_t) G + 1);
                if (rcS != SD_OK) return rcS;
                const unsigned cgrid = std::min<unsigned>((nLive + 3) / 4, 2048u);
                hipLaunchKernelGGL(k_alt_mask_copy, dim3(cgrid), dim3(256), 0, ctx->stream, (const uint32_t *) dNLive, (const uint32_t *) dLiveList,
                                   (const uint32_t *) dSeedT, (const uint64_t *) targets->dOff, (const uint8_t *) targets->dRes,
                                   (const uint64_t *) dSOff, stride, (const int2 *) dIvl, (const uint32_t *) dNIvl, dScratch);
                SD_HIP(ctx, hipGetLastError());
            }
            // the round's alignments: the batch path on the scratch set
            rounds.emplace_back();
            RoundRecords &R = rounds.back();
            R.poolBase = poolUsed;
            uint64_t used = 0;
            int rc;
            if (compact) {
                tmpIdx.resize(G);
                tmpRec.resize(G);
                uint32_t nOut = 0;
                rc = sd_sw_align_batch_compact(ctx, &p, queries, &scratch, G, sQ.data() + g0, pairT.data(), nullptr, tmpIdx.data(), tmpRec.data(), &nOut,
                                               btPool + poolUsed, btCap - poolUsed, &used);
                if (rc != SD_OK) return rc;
                R.idx.assign(tmpIdx.begin(), tmpIdx.begin() + nOut);
                R.rec.assign(tmpRec.begin(), tmpRec.begin() + nOut);
            } else {
                R.rec.resize(G);
                rc = sd_sw_align_batch(ctx, &p, queries, &scratch, G, sQ.data() + g0, pairT.data(), nullptr, R.rec.data(),
                                       btPool ? btPool + poolUsed : nullptr, btPool ? btCap - poolUsed : 0, &used);
                if (rc != SD_OK) return rc;
            }
            poolUsed += used;
            ctx->altSeedRounds += nLive;
            // criteria, intervals and the live list of the next round, from the records the batch path left on the device
            const sd_sw_result *dRes = ctx->alignDevRes;   // the per-pair records of the call that just returned
            if (!dRes || ctx->alignDevResN != (size_t) G) return sdFail(ctx, SD_EINVAL, "sd_sw_align_alt_batch: the batch path left no records for %u pairs", G);
            {
                ProfScope ps(ctx, "alt_accept_compact");
                hipLaunchKernelGGL(k_alt_accept, dim3(grid), dim3(256), 0, ctx->stream, G, stride, crit, dRes,
                                   (const uint32_t *) dSeedQ, (const uint32_t *) dSeedT, (const uint64_t *) queries->dOff,
                                   (const uint64_t *) targets->dOff, dIvl, dNIvl, dLive, dCnt);
                const int rcS = sdCtxExclusiveScan(ctx, "alt.scantmp", (const uint8_t *) dLive, dPos, (size_t) G + 1);
                if (rcS != SD_OK) return rcS;
                hipLaunchKernelGGL(k_alt_compact, dim3(grid), dim3(256), 0, ctx->stream, G, (const uint8_t *) dLive, (const uint64_t *) dPos,
                                   dLiveList, dNLive);
                SD_HIP(ctx, hipGetLastError());
            }
            SD_HIP(ctx, sdD2H(ctx, &nLive, dNLive, sizeof(uint32_t)));
            SD_HIP(ctx, sdD2H(ctx, &copied, dSOff + 2 * (size_t) G, sizeof(uint64_t)));   // (statistics: the size of this round's scratch set)
            SD_HIP(ctx, sdStreamSync(ctx));
            ctx->altBytes += copied;
        }
        // the group's output: per seed the records of the rounds it was accepted in
        hCnt.resize(G);
        SD_HIP(ctx, sdD2H(ctx, hCnt.data(), dCnt, (size_t) G * sizeof(uint32_t)));
        SD_HIP(ctx, sdStreamSync(ctx));
        // a seed's count ends at the first round without a record that came back and passes with the exact E-value (alignBatchImpl
        // clears the start positions of a record it puts above the threshold, and the compact call returns reportable pairs only):
        // whatever the device rule counted beyond that round is dropped, so every counted slot of `out` is written
        have.assign(G, 0);
        for (size_t r = 0; r < rounds.size(); r++) {
            const RoundRecords &R = rounds[r];
            for (size_t x = 0; x < R.rec.size(); x++) {
                const uint32_t g = compact ? R.idx[x] : (uint32_t) x;
                if (hCnt[g] <= r || have[g] != r) continue;
                sd_sw_result rec = R.rec[x];
                if (rec.qStart < 0 || rec.evalue > p.evalThr) continue;
                rec.btOffset += R.poolBase;
                out[(size_t) sIdx[g0 + g] * maxAlt + r] = rec;
                have[g] = (uint32_t) r + 1;
            }
        }
        for (uint32_t g = 0; g < G; g++) outCount[sIdx[g0 + g]] = std::min(hCnt[g], have[g]);
        g0 = g1;
    }
    if (btUsed) *btUsed = poolUsed;
    return SD_OK;
}

}  // extern "C"
