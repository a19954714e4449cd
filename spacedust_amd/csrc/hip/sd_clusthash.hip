// sd_clusthash_batch: clusthash (the amino-acid branch of M/src/util/clusthash.cpp:64-181) on the device; DESIGN.md 4.18.
//
//   ch_hash_kernel      one wavefront per sequence: Util::hash of the reduced codes (sdSeqHash31, shared with the kmermatcher's identity
//                       record) and the length
//   sort                sortByField (sd_field_sort.h: fs_key_kernel + sdRadixSortPairs per link, stable, over a permutation), least
//                       significant field first: length (the bits the data needs), hash low, hash high; then gatherFields
//                       (fs_gather_kernel per field).  The input is in id order and the passes are stable, so the result is sorted by
//                       (hash, length, id).  Only sequences of equal length ever interact in the reference's loop, so every (hash, length)
//                       run is a group of its own.
//   ch_start_kernel + max scan, ch_groupflag_kernel + sum scan, ch_grouplist_kernel
//                       the runs of more than one sequence, as two lists: up to CH_WAVE_BOUND members, and more
//   ch_group_kernel     the greedy pass (clusthash.cpp:129-177) of one group by one workgroup: one wavefront for the first list, CH_WAVES
//                       wavefronts that split the j for the second.  i is walked serially; a j is compared by all 64 lanes, 4 bytes per
//                       lane and step, 4 steps per chunk; the found flags are the foundBy array itself, behind a workgroup barrier after
//                       every i that compared anything.
// No workgroup waits for another; every store is a plain vector store (the pair counter is one vector atomic per wavefront and group).
#include "sd_batch_check.h"

#include <omp.h>

#include <memory>

namespace {

#include "sd_scan_sort.h"
#include "sd_field_sort.h"
#include "sd_seqhash.h"

constexpr int CH_BLOCK = 256;
// Largest group one wavefront takes alone.  A wavefront reads the found flags of 64 j at a time, so up to 64 members a step of i is one
// such read and further wavefronts would have nothing to take; above it the 64-member pieces go round the CH_WAVES wavefronts of a
// workgroup.  Measurement: DESIGN.md 4.18 (tuning builds: -DCH_WAVE_BOUND=...)
#ifndef CH_WAVE_BOUND
#define CH_WAVE_BOUND 64
#endif
constexpr int CH_WAVES = 8;
constexpr int CH_PAD = 16;   // bytes in front of and behind the letters on the device: the aligned words around a sequence's ends exist
constexpr uint32_t CH_NONE = UINT32_MAX;
constexpr uint32_t CH_STOPPED = UINT32_MAX;
constexpr unsigned CH_MAX_GRID = 1u << 20;

struct ChMap {
    uint8_t map[24];   // 21-letter code -> reduced code
};

__global__ void __launch_bounds__(64)
ch_hash_kernel(ChMap m, const uint8_t *__restrict__ residues, const uint64_t *__restrict__ offsets, uint32_t nSeq, uint32_t *__restrict__ hHi,
               uint32_t *__restrict__ hLo, uint32_t *__restrict__ len) {
    __shared__ uint8_t map[24];
    const int lane = threadIdx.x;
    if (lane < 21) map[lane] = m.map[lane];
    __syncthreads();
    for (uint32_t s = blockIdx.x; s < nSeq; s += gridDim.x) {
        const uint64_t off = offsets[s];
        const uint32_t L = (uint32_t) (offsets[s + 1] - off);
        const uint64_t h = sdSeqHash31(map, residues + off, L, lane);
        if (lane == 0) {
            hHi[s] = (uint32_t) (h >> 32);
            hLo[s] = (uint32_t) h;
            len[s] = L;
        }
    }
}

// hashFlag has n + 1 entries (the last one 0: the scan's total)
__global__ void __launch_bounds__(CH_BLOCK)
ch_start_kernel(const uint32_t *__restrict__ sHi, const uint32_t *__restrict__ sLo, const uint32_t *__restrict__ sLen, uint32_t n,
                uint32_t *__restrict__ startOrZero, uint32_t *__restrict__ hashFlag) {
    const uint64_t i = (uint64_t) blockIdx.x * CH_BLOCK + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        hashFlag[i] = 0;
        return;
    }
    const bool hashStart = i == 0 || sHi[i] != sHi[i - 1] || sLo[i] != sLo[i - 1];
    const bool groupStart = hashStart || sLen[i] != sLen[i - 1];
    startOrZero[i] = groupStart ? (uint32_t) i : 0u;
    hashFlag[i] = hashStart ? 1u : 0u;
}

// flag has n + 1 entries: at the last member of a group of more than one, 1 (up to CH_WAVE_BOUND members) or 1 << 32 (more)
__global__ void __launch_bounds__(CH_BLOCK)
ch_groupflag_kernel(const uint32_t *__restrict__ sHi, const uint32_t *__restrict__ sLo, const uint32_t *__restrict__ sLen,
                    const uint32_t *__restrict__ runStart, uint32_t n, uint64_t *__restrict__ flag, uint32_t *__restrict__ largest) {
    const uint64_t i = (uint64_t) blockIdx.x * CH_BLOCK + threadIdx.x;
    if (i > n) return;
    uint64_t f = 0;
    if (i < n) {
        const bool runEnd = i + 1 == n || sHi[i + 1] != sHi[i] || sLo[i + 1] != sLo[i] || sLen[i + 1] != sLen[i];
        const uint32_t size = (uint32_t) i - runStart[i] + 1;
        if (runEnd && size > 1) {
            f = size <= (uint32_t) CH_WAVE_BOUND ? 1ull : (1ull << 32);
            atomicMax(largest, size);   // (most runs are single sequences: only longer ones go to the one shared word)
        }
    }
    flag[i] = f;
}

__global__ void __launch_bounds__(CH_BLOCK)
ch_grouplist_kernel(const uint64_t *__restrict__ flag, const uint64_t *__restrict__ at, const uint32_t *__restrict__ runStart, uint32_t n,
                    uint32_t nSmall, uint32_t nLarge, uint32_t *__restrict__ smallStart, uint32_t *__restrict__ smallSize,
                    uint32_t *__restrict__ largeStart, uint32_t *__restrict__ largeSize) {
    const uint64_t i = (uint64_t) blockIdx.x * CH_BLOCK + threadIdx.x;
    if (i >= n || flag[i] == 0) return;
    const uint32_t start = runStart[i], size = (uint32_t) i - start + 1;
    if (flag[i] == 1) {
        const uint32_t k = (uint32_t) at[i];
        if (k < nSmall) {
            smallStart[k] = start;
            smallSize[k] = size;
        }
    } else {
        const uint32_t k = (uint32_t) (at[i] >> 32);
        if (k < nLarge) {
            largeStart[k] = start;
            largeSize[k] = size;
        }
    }
}

// Equal bytes of a[0, L) and b[0, L) by one wavefront, or CH_STOPPED once more than maxMis bytes differ (decided per chunk, by all lanes
// alike).  base: the first letter of the DB on the device (16-byte aligned, CH_PAD bytes before and behind it).  Lane l of step u takes
// the aligned 4-byte word 64 u + l of a, and the same bytes of b out of two aligned words (v_alignbyte); the bytes of the first and the
// last word that lie outside the sequence are masked.
__device__ __forceinline__ uint32_t chCompare(const uint8_t *__restrict__ base, uint64_t aOff, uint64_t bOff, uint32_t L, uint32_t maxMis,
                                              int lane) {
    const uint32_t head = (uint32_t) (aOff & 3);
    const uint32_t *aAl = (const uint32_t *) (base + (aOff - head));
    const int64_t bb = (int64_t) bOff - (int64_t) head;   // (>= -3: inside the pad)
    const uint32_t sh = (uint32_t) (bb & 3);
    const uint32_t *bAl = (const uint32_t *) (base + (bb - (int64_t) sh));
    const uint64_t span = (uint64_t) head + L;            // bytes from a's first aligned word to its end
    const uint32_t nWords = (uint32_t) ((span + 3) / 4);
    uint32_t mis = 0;
    for (uint32_t w0 = 0; w0 < nWords; w0 += 256) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t w = w0 + (uint32_t) u * 64 + (uint32_t) lane;
            const uint32_t wc = w < nWords ? w : nWords - 1;   // (loads stay inside the sequence's words; the result is dropped)
            const uint32_t a = aAl[wc], lo = bAl[wc], hi = bAl[wc + 1];
            uint32_t x = a ^ __builtin_amdgcn_alignbyte(hi, lo, sh);
            uint32_t outside = wc == 0 ? (1u << (8 * head)) - 1u : 0u;
            const uint64_t left = span - 4ull * wc;            // bytes of the sequence from this word on: 1 .. 3 in a partial last word
            if (left < 4) outside |= 0xFFFFFFFFu << (8 * (uint32_t) left);
            x &= ~outside;
            if (w >= nWords) x = 0;
            // bit 7 of every byte of x that is not zero
            const uint32_t nz = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
            mis += (uint32_t) __popc(nz);
        }
        if (w0 + 256 < nWords) {
            uint32_t sum = mis;
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            if (sum > maxMis) return CH_STOPPED;
        }
    }
    for (int o = 32; o > 0; o >>= 1) mis += __shfl_xor(mis, o, 64);
    return L - mis;
}

// One workgroup of WAVES wavefronts per group: members ids[start .. start + n) in id order, all of one hash and length.
template <int WAVES>
__global__ void __launch_bounds__(64 * WAVES)
ch_group_kernel(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ sId,
                const uint32_t *__restrict__ minIdentical, const uint32_t *__restrict__ gStart, const uint32_t *__restrict__ gSize,
                uint32_t nGroups, uint32_t *foundBy, uint32_t *identical, unsigned long long *pairs) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    for (uint32_t g = blockIdx.x; g < nGroups; g += gridDim.x) {
        const uint32_t *ids = sId + gStart[g];
        const uint32_t n = gSize[g];
        const uint32_t first = ids[0];
        const uint32_t L = (uint32_t) (offsets[first + 1] - offsets[first]);
        const uint32_t need = minIdentical[first];   // (one value per length)
        const bool canReach = need <= L;
        const uint32_t maxMis = canReach ? L - need : 0;
        if (!canReach) {
            // no count of equal bytes reaches the threshold at this length: every member stays open and compares itself with every other
            // one, n (n - 1) pairs, and nothing is loaded or marked -- counted, not walked
            if (threadIdx.x == 0) atomicAdd(pairs, (unsigned long long) n * (n - 1));
            continue;
        }
        unsigned long long compared = 0;
        uint32_t iBase = 0;
        // Here no member of the group has been written since the last barrier.  Every wavefront derives i for itself from plain loads of
        // foundBy while others may already be storing (after a window of found members there is no barrier).  They agree because a store
        // only closes a flag that was open and never the first open one of the window (j != i), and a flag never reopens: whenever a
        // wavefront reads the window, its first open flag is the same, so all take the same path to the same barriers.  This rests on the
        // workgroup's wavefronts sharing one CU and its vector L1 (no -mtgsplit build) and on 4-byte stores being indivisible; a change
        // that lets a flag reopen, or a threadgroup-split build, would make the barrier counts differ and hang the workgroup.
        while (iBase < n) {
            const uint32_t ii = iBase + (uint32_t) lane;
            const uint32_t idI = ii < n ? ids[ii] : 0;
            const bool open = ii < n && foundBy[idI] == CH_NONE;
            const unsigned long long openMask = __ballot(open);
            if (openMask == 0) {   // found already: they get nothing more, and nothing was written
                iBase += 64;
                continue;
            }
            const int il = __ffsll((long long) openMask) - 1;
            const uint32_t i = iBase + (uint32_t) il;
            const uint32_t qId = (uint32_t) __shfl((int) idI, il, 64);
            const uint64_t qOff = offsets[qId];
            for (uint32_t jBase = wave * 64; jBase < n; jBase += 64 * WAVES) {
                const uint32_t jj = jBase + (uint32_t) lane;
                const uint32_t idJ = jj < n ? ids[jj] : 0;
                const bool cand = jj < n && jj != i && foundBy[idJ] == CH_NONE;
                const uint64_t offJ = cand ? offsets[idJ] : 0;
                unsigned long long mask = __ballot(cand);
                compared += (unsigned long long) __popcll(mask);
                while (mask) {
                    const int jl = __ffsll((long long) mask) - 1;
                    mask &= mask - 1;
                    const uint32_t tId = (uint32_t) __shfl((int) idJ, jl, 64);
                    const uint64_t tOff = ((uint64_t) (uint32_t) __shfl((int) (uint32_t) (offJ >> 32), jl, 64) << 32) |
                                          (uint64_t) (uint32_t) __shfl((int) (uint32_t) offJ, jl, 64);
                    const uint32_t eq = chCompare(base, qOff, tOff, L, maxMis, lane);
                    if (eq != CH_STOPPED && eq >= need && lane == 0) {
                        foundBy[tId] = qId;
                        identical[tId] = eq;
                    }
                }
            }
            __syncthreads();
            iBase = i + 1;
        }
        if (lane == 0 && compared) atomicAdd(pairs, compared);
    }
}

}  // namespace

extern "C" {

int sd_clusthash_batch(sd_ctx *ctx, const sd_clusthash_params *par, uint64_t nSeq, const uint8_t *residues, const uint64_t *offsets,
                       const uint8_t *letters, const uint8_t *letterMap, uint32_t *foundBy, uint32_t *identical, uint64_t *hash,
                       uint64_t *stats) {
    const char *who = "sd_clusthash_batch";
    if (!ctx || !par || !offsets || !letterMap) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (nSeq && (!residues || !letters || !foundBy || !identical)) return SD_EINVAL;
    // (21 is no reduced alphabet: the reference's ReducedMatrix refuses it, "Reduced alphabet has to be smaller than the original one")
    if (par->alphabetSize != 3 && par->alphabetSize != 13)
        return sdFail(ctx, SD_EUNSUPPORTED, "%s: alphabet size %d (3 and 13 are implemented)", who, par->alphabetSize);
    if (nSeq > RS_MAX_ELEMENTS)
        return sdFail(ctx, SD_EUNSUPPORTED, "%s: %llu sequences in one call (the device sort counts in 32 bits: at most %llu)", who,
                      (unsigned long long) nSeq, (unsigned long long) RS_MAX_ELEMENTS);
    std::unique_ptr<HostScope> phase(new HostScope(ctx, "ch_prepare"));
    SdSeqBatch batch;
    const int rcCheck = sdCheckSeqBatch(ctx, who, par->alphabetSize, nSeq, residues, offsets, letterMap, &batch);
    if (rcCheck != SD_OK) return rcCheck;
    ChMap cm;
    memcpy(cm.map, batch.map, sizeof(cm.map));
    const uint64_t maxLen = batch.maxLen, total = batch.total;
    // per sequence: the equal bytes the threshold asks for at its length (sd_host_clusthash_min_identical: the float comparison is the
    // host's, the device compares integers)
    std::vector<uint32_t> need(nSeq ? nSeq : 1);
    {
        uint32_t lastL = UINT32_MAX, lastNeed = 0;   // (neighbours often share a length)
        for (uint64_t s = 0; s < nSeq; s++) {
            const uint32_t L = (uint32_t) (offsets[s + 1] - offsets[s]);
            if (L != lastL) {
                lastL = L;
                lastNeed = sd_host_clusthash_min_identical(par->seqIdThr, L);
            }
            need[s] = lastNeed;
        }
    }
    if (nSeq == 0) return SD_OK;
    // everything is resident at once
    {
        const uint64_t bytes = nSeq * SD_CLUSTHASH_BYTES_PER_SEQ + 2 * total + 2 * CH_PAD + sdRadixSortCountsBytes() + 4096;
        uint64_t avail = 0;   // (what this context's clusthash workspace already holds counts as available)
        SD_HIP(ctx, wsAvailableBytes(ctx, "ch.", &avail));
        if (bytes > avail)
            return sdFail(ctx, SD_ENOMEM, "%s: %llu bytes needed for %llu sequences of %llu residues, %llu free on the device", who,
                          (unsigned long long) bytes, (unsigned long long) nSeq, (unsigned long long) total, (unsigned long long) avail);
    }
    const uint32_t n32 = (uint32_t) nSeq;
    hipStream_t st = ctx->stream;
    phase.reset(new HostScope(ctx, "ch_alloc"));
    uint8_t *dRes = nullptr, *dLet = nullptr;
    uint64_t *dOff = nullptr, *dScanTmp = nullptr, *dFlag = nullptr, *dAt = nullptr, *dHashAt = nullptr;
    unsigned long long *dPairs = nullptr;
    uint32_t *dNeed, *hHi, *hLo, *hLen, *sHi, *sLo, *sLen, *dStart, *dRunStart, *dHashFlag, *dLargest, *dFoundBy, *dIdentical, *dSmallStart,
        *dSmallSize, *dLargeStart, *dLargeSize;
    FieldSortBufs sb;
    const size_t listCap = (size_t) nSeq / 2 + 1;
    SD_HIP(ctx, wsGet(ctx, "ch.res", (size_t) total, &dRes));
    SD_HIP(ctx, wsGet(ctx, "ch.let", (size_t) total + 2 * CH_PAD, &dLet));
    SD_HIP(ctx, wsGet(ctx, "ch.off", (size_t) nSeq + 1, &dOff));
    SD_HIP(ctx, wsGet(ctx, "ch.need", (size_t) nSeq, &dNeed));
    SD_HIP(ctx, wsGet(ctx, "ch.hhi", (size_t) nSeq, &hHi));
    SD_HIP(ctx, wsGet(ctx, "ch.hlo", (size_t) nSeq, &hLo));
    SD_HIP(ctx, wsGet(ctx, "ch.hlen", (size_t) nSeq, &hLen));
    SD_HIP(ctx, wsGet(ctx, "ch.shi", (size_t) nSeq, &sHi));
    SD_HIP(ctx, wsGet(ctx, "ch.slo", (size_t) nSeq, &sLo));
    SD_HIP(ctx, wsGet(ctx, "ch.slen", (size_t) nSeq, &sLen));
    SD_HIP(ctx, fieldSortBufsGet(ctx, "ch.", (size_t) nSeq, &sb));
    SD_HIP(ctx, wsGet(ctx, "ch.start", (size_t) nSeq, &dStart));
    SD_HIP(ctx, wsGet(ctx, "ch.runstart", (size_t) nSeq, &dRunStart));
    SD_HIP(ctx, wsGet(ctx, "ch.hashflag", (size_t) nSeq + 1, &dHashFlag));
    SD_HIP(ctx, wsGet(ctx, "ch.hashat", (size_t) nSeq + 1, &dHashAt));
    SD_HIP(ctx, wsGet(ctx, "ch.flag", (size_t) nSeq + 1, &dFlag));
    SD_HIP(ctx, wsGet(ctx, "ch.at", (size_t) nSeq + 1, &dAt));
    SD_HIP(ctx, wsGet(ctx, "ch.scantmp", sdScanTmpBytes(nSeq + 1) / sizeof(uint64_t), &dScanTmp));
    SD_HIP(ctx, wsGet(ctx, "ch.largest", (size_t) 1, &dLargest));
    SD_HIP(ctx, wsGet(ctx, "ch.pairs", (size_t) 1, &dPairs));
    SD_HIP(ctx, wsGet(ctx, "ch.foundby", (size_t) nSeq, &dFoundBy));
    SD_HIP(ctx, wsGet(ctx, "ch.identical", (size_t) nSeq, &dIdentical));
    SD_HIP(ctx, wsGet(ctx, "ch.smallstart", listCap, &dSmallStart));
    SD_HIP(ctx, wsGet(ctx, "ch.smallsize", listCap, &dSmallSize));
    SD_HIP(ctx, wsGet(ctx, "ch.largestart", listCap, &dLargeStart));
    SD_HIP(ctx, wsGet(ctx, "ch.largesize", listCap, &dLargeSize));
    phase.reset();
    {
        HostScope hs(ctx, "ch_copy_in");
        SD_HIP(ctx, hipMemcpyAsync(dRes, residues, (size_t) total, hipMemcpyHostToDevice, st));
        SD_HIP(ctx, hipMemsetAsync(dLet, 0, (size_t) total + 2 * CH_PAD, st));
        SD_HIP(ctx, hipMemcpyAsync(dLet + CH_PAD, letters, (size_t) total, hipMemcpyHostToDevice, st));
        SD_HIP(ctx, hipMemcpyAsync(dOff, offsets, ((size_t) nSeq + 1) * 8, hipMemcpyHostToDevice, st));
        SD_HIP(ctx, hipMemcpyAsync(dNeed, need.data(), (size_t) nSeq * 4, hipMemcpyHostToDevice, st));
        SD_HIP(ctx, hipMemsetAsync(dFoundBy, 0xFF, (size_t) nSeq * 4, st));
        SD_HIP(ctx, hipMemsetAsync(dIdentical, 0, (size_t) nSeq * 4, st));
        SD_HIP(ctx, hipMemsetAsync(dLargest, 0, 4, st));
        SD_HIP(ctx, hipMemsetAsync(dPairs, 0, 8, st));
        SD_HIP(ctx, sdStreamSync(ctx));   // (need is a local vector)
    }
    {
        HostScope hs(ctx, "ch_hash");
        hipLaunchKernelGGL(ch_hash_kernel, dim3(std::min<uint32_t>(n32, CH_MAX_GRID)), dim3(64), 0, st, cm, (const uint8_t *) dRes, (const uint64_t *) dOff,
                           n32, hHi, hLo, hLen);
        SD_HIP(ctx, hipGetLastError());
        if (ctx->profiling) SD_HIP(ctx, sdStreamSync(ctx));
    }
    {
        HostScope hs(ctx, "ch_sort");
        // (hash, length, id), least significant field first; the input is in id order and every pass is stable.  The hash takes all 64 bits
        SD_HIP(ctx, sortByField(st, sb, hLen, nullptr, n32, FS_PLAIN, 0, bitsFor(maxLen)));
        SD_HIP(ctx, sortByField(st, sb, hLo, sb.permA, n32, FS_PLAIN, 0, 32));
        SD_HIP(ctx, sortByField(st, sb, hHi, sb.permA, n32, FS_PLAIN, 0, 32));
        const uint32_t *src[3] = {hHi, hLo, hLen};
        uint32_t *dst[3] = {sHi, sLo, sLen};
        SD_HIP(ctx, gatherFields(st, sb.permA, n32, 3, src, dst));
        if (ctx->profiling) SD_HIP(ctx, sdStreamSync(ctx));
    }
    const uint32_t *sId = sb.permA;   // the sorted ids: the sort's buffers are not touched again
    uint64_t uniqueHashes = 0, packed = 0;
    uint32_t largest = 0;
    {
        HostScope hs(ctx, "ch_groups");
        hipLaunchKernelGGL(ch_start_kernel, dim3(gridFor(nSeq + 1, CH_BLOCK)), dim3(CH_BLOCK), 0, st, (const uint32_t *) sHi, (const uint32_t *) sLo,
                           (const uint32_t *) sLen, n32, dStart, dHashFlag);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, (sdScanLaunch<uint32_t, ScanMax32, true, uint32_t>(st, dStart, dRunStart, nSeq, (uint32_t *) dScanTmp)));
        SD_HIP(ctx, (sdScanLaunch<uint32_t, ScanSum64, false, uint64_t>(st, dHashFlag, dHashAt, nSeq + 1, dScanTmp)));
        hipLaunchKernelGGL(ch_groupflag_kernel, dim3(gridFor(nSeq + 1, CH_BLOCK)), dim3(CH_BLOCK), 0, st, (const uint32_t *) sHi, (const uint32_t *) sLo,
                           (const uint32_t *) sLen, (const uint32_t *) dRunStart, n32, dFlag, dLargest);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, (sdScanLaunch<uint64_t, ScanSum64, false, uint64_t>(st, dFlag, dAt, nSeq + 1, dScanTmp)));
        SD_HIP(ctx, sdD2H(ctx, &uniqueHashes, dHashAt + nSeq, 8));
        SD_HIP(ctx, sdD2H(ctx, &packed, dAt + nSeq, 8));
        SD_HIP(ctx, sdD2H(ctx, &largest, dLargest, 4));
        SD_HIP(ctx, sdStreamSync(ctx));
    }
    const uint32_t nSmall = (uint32_t) packed, nLarge = (uint32_t) (packed >> 32);
    if ((uint64_t) nSmall > listCap || (uint64_t) nLarge > listCap)
        return sdFail(ctx, SD_EHIP, "%s: %u + %u groups counted among %llu sequences", who, nSmall, nLarge, (unsigned long long) nSeq);
    unsigned long long pairs = 0;
    {
        HostScope hs(ctx, "ch_pass");
        if (nSmall + nLarge > 0) {
            hipLaunchKernelGGL(ch_grouplist_kernel, dim3(gridFor(nSeq, CH_BLOCK)), dim3(CH_BLOCK), 0, st, (const uint64_t *) dFlag, (const uint64_t *) dAt,
                               (const uint32_t *) dRunStart, n32, nSmall, nLarge, dSmallStart, dSmallSize, dLargeStart, dLargeSize);
            SD_HIP(ctx, hipGetLastError());
        }
        const uint8_t *base = dLet + CH_PAD;
        if (nLarge > 0)   // first: the long ones
            hipLaunchKernelGGL(ch_group_kernel<CH_WAVES>, dim3(std::min<uint32_t>(nLarge, CH_MAX_GRID)), dim3(64 * CH_WAVES), 0, st, base,
                               (const uint64_t *) dOff, sId, (const uint32_t *) dNeed, (const uint32_t *) dLargeStart, (const uint32_t *) dLargeSize, nLarge,
                               dFoundBy, dIdentical, dPairs);
        if (nSmall > 0)
            hipLaunchKernelGGL(ch_group_kernel<1>, dim3(std::min<uint32_t>(nSmall, CH_MAX_GRID)), dim3(64), 0, st, base, (const uint64_t *) dOff, sId,
                               (const uint32_t *) dNeed, (const uint32_t *) dSmallStart, (const uint32_t *) dSmallSize, nSmall, dFoundBy, dIdentical,
                               dPairs);
        SD_HIP(ctx, hipGetLastError());
        if (ctx->profiling) SD_HIP(ctx, sdStreamSync(ctx));
    }
    {
        HostScope hs(ctx, "ch_copy_out");
        std::vector<uint32_t> hi, lo;
        SD_HIP(ctx, hipMemcpyAsync(foundBy, dFoundBy, (size_t) nSeq * 4, hipMemcpyDeviceToHost, st));
        SD_HIP(ctx, hipMemcpyAsync(identical, dIdentical, (size_t) nSeq * 4, hipMemcpyDeviceToHost, st));
        SD_HIP(ctx, hipMemcpyAsync(&pairs, dPairs, 8, hipMemcpyDeviceToHost, st));
        if (hash) {
            hi.resize((size_t) nSeq);
            lo.resize((size_t) nSeq);
            SD_HIP(ctx, hipMemcpyAsync(hi.data(), hHi, (size_t) nSeq * 4, hipMemcpyDeviceToHost, st));
            SD_HIP(ctx, hipMemcpyAsync(lo.data(), hLo, (size_t) nSeq * 4, hipMemcpyDeviceToHost, st));
        }
        SD_HIP(ctx, sdStreamSync(ctx));
        if (hash) sdJoinHiLo(hi.data(), lo.data(), nSeq, hash);
    }
    if (stats) {
        stats[0] = uniqueHashes;
        stats[1] = (uint64_t) nSmall + nLarge;
        stats[2] = pairs;
        stats[3] = largest > 1 ? largest : 1;
    }
    return SD_OK;
}

}  // extern "C"
