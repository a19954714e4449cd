// sd_kmermatch_batch: linclust's kmermatcher (M/src/linclust/kmermatcher.cpp) for amino-acid sequences that fit one split, on the device.
//
// Records (fillKmerPositionArray's amino-acid branch, kmermatcher.cpp:104-333), one wavefront per sequence:
//   km_select_kernel   k-mer index and 16-bit XXH64 score of every window without X; the selection threshold of the sequence from a
//                      128-bin histogram of score >> 9 and, in a second pass over the windows, a 512-bin histogram of the one coarse
//                      bin the walk stops in (the reference's 64 K-bin array never exists: 2.6 KB of LDS instead of 128 KB, at the
//                      price of hashing every window three times -- DESIGN 4.17); writes threshold, excess and record count
//   sdScanLaunch       record offsets
//   km_emit_kernel     the identity record and the selected windows in position order (ballot ranks), last-bin rule included
// Grouping (doComputation, assignGroup, writeKmerMatcherResult; kmermatcher.cpp:426-625, 876-991):
//   first sort         sortByField (sd_field_sort.h: fs_key_kernel + sdRadixSortPairs per link, stable, over a permutation): pos, id,
//                      maxLen - seqLen, key low, key high; then gatherFields (fs_gather_kernel per field)
//   km_start_kernel + max scan   first record of every run of equal keys = the representative
//   km_groupflag_kernel + scan + km_groupwrite_kernel   (rep, member, diagonal) of every record that assignGroup keeps
//   second sort        diagonal (biased), member, rep
//   km_hitflag_kernel + scan + km_hit_kernel   one hit per (rep, member) run with member != rep
// No kernel waits for another workgroup; every store is a plain vector store.
// The records part is one function, kmRecordsStage, which sd_selftest_kmermatch_records calls too and copies out for tests/.
//
// The reference's element type T (short below a longest sequence of 32 767, int otherwise) only sets the width of seqLen, pos and the
// diagonal: with short every length is below 32 767, so every position and every diagonal fits and nothing is truncated; the fields are
// 32-bit here in both cases.
#include "sd_batch_check.h"

#include <omp.h>

#include <memory>

namespace {

#include "sd_scan_sort.h"
#include "sd_field_sort.h"
#include "sd_seqhash.h"

constexpr int KM_BLOCK = 256;
constexpr int KM_MAXK = 24;
constexpr int KM_CHUNK = 64;   // windows per step of a wavefront

struct KmPar {
    uint64_t pw[KM_MAXK];   // (alphabetSize - 1)^j: Indexer(alphabetSize - 1, k)
    uint64_t seed;          // --hash-shift
    int32_t k;
    uint32_t xCode;         // reduced code of X (alphabetSize - 1)
    uint8_t map[24];        // 21-letter code -> reduced code
};

// XXH64 of one 8-byte little-endian word, from the published specification (input shorter than 32 bytes: no stripe loop)
__host__ __device__ __forceinline__ uint64_t kmRotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__host__ __device__ __forceinline__ uint64_t kmXxh64Word(uint64_t v, uint64_t seed) {
    const uint64_t P1 = 11400714785074694791ULL, P2 = 14029467366897019727ULL, P3 = 1609587929392839161ULL, P4 = 9650029242287828579ULL,
                   P5 = 2870177450012600261ULL;
    uint64_t h = seed + P5 + 8;
    h ^= kmRotl(v * P2, 31) * P1;
    h = kmRotl(h, 27) * P1 + P4;
    h ^= h >> 33;
    h *= P2;
    h ^= h >> 29;
    h *= P3;
    h ^= h >> 32;
    return h;
}

// Stages the reduced codes of positions [base, base + 64 + k - 1) and gives lane `lane` the window at base + lane: true when the window
// lies inside the sequence and holds no X.  One wavefront per workgroup: the barriers are the wavefront's own.
__device__ __forceinline__ bool kmWindow(const KmPar &p, const uint8_t *__restrict__ res, uint32_t L, uint32_t base, int lane,
                                         const uint8_t *map, uint8_t *codes, uint64_t *idx, uint32_t *score) {
    __syncthreads();
    for (int x = lane; x < KM_CHUNK + p.k - 1; x += 64) {
        const uint32_t at = base + (uint32_t) x;
        codes[x] = at < L ? map[res[at]] : (uint8_t) p.xCode;
    }
    __syncthreads();
    bool ok = (uint64_t) base + (uint32_t) lane + (uint32_t) p.k <= (uint64_t) L;
    uint64_t v = 0;
    for (int j = 0; j < p.k; j++) {
        const uint32_t c = codes[lane + j];
        ok = ok && c != p.xCode;
        v += (uint64_t) c * p.pw[j];
    }
    *idx = v;
    *score = (uint32_t) (kmXxh64Word(v, p.seed) & 0xFFFFu);
    return ok;
}

__global__ void __launch_bounds__(64)
km_select_kernel(KmPar p, const uint8_t *__restrict__ residues, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ consHost,
                 uint32_t nSeq, uint32_t *__restrict__ outCount, uint32_t *__restrict__ outThr, uint32_t *__restrict__ outExcess,
                 uint32_t *__restrict__ outCons) {
    __shared__ uint32_t coarse[128];
    __shared__ uint32_t fine[512];
    __shared__ uint8_t codes[KM_CHUNK + KM_MAXK];
    __shared__ uint8_t map[24];
    const uint32_t s = blockIdx.x;
    const int lane = threadIdx.x;
    if (s >= nSeq) return;
    const uint64_t off = offsets[s];
    const uint32_t L = (uint32_t) (offsets[s + 1] - off);
    const uint8_t *res = residues + off;
    for (int x = lane; x < 128; x += 64) coarse[x] = 0;
    for (int x = lane; x < 512; x += 64) fine[x] = 0;
    if (lane < 21) map[lane] = p.map[lane];
    const uint32_t cons0 = consHost[s];
    const uint32_t nW = L >= (uint32_t) p.k ? L - (uint32_t) p.k + 1 : 0;
    uint32_t considered = 0, threshold = 0, excess = 0, selected = 0;
    if (cons0 > 0 && nW > 0) {
        uint32_t cnt = 0;
        for (uint32_t base = 0; base < nW; base += KM_CHUNK) {
            uint64_t idx;
            uint32_t score;
            const bool ok = kmWindow(p, res, L, base, lane, map, codes, &idx, &score);
            if (ok) atomicAdd(&coarse[score >> 9], 1u);
            cnt += (uint32_t) __popcll(__ballot(ok));
        }
        __syncthreads();
        considered = cons0 < cnt ? cons0 : cnt;
        if (considered > 0) {
            // kmermatcher.cpp:208-220: the coarse walk, one bin back, then the fine walk (every lane walks the same bins)
            uint32_t inBins = 0, h = 0;
            for (; h < 128 && inBins < considered; h++) inBins += coarse[h];
            h -= h > 0 ? 1 : 0;
            inBins -= coarse[h];
            for (uint32_t base = 0; base < nW; base += KM_CHUNK) {
                uint64_t idx;
                uint32_t score;
                const bool ok = kmWindow(p, res, L, base, lane, map, codes, &idx, &score);
                if (ok && (score >> 9) == h) atomicAdd(&fine[score & 511u], 1u);
            }
            __syncthreads();
            // (the walk ends inside coarse bin h: through its last fine bin the count has reached kmerConsidered; 65 536 is a possible end)
            for (threshold = h * 512; threshold < h * 512 + 512 && inBins < considered; threshold++) inBins += fine[threshold - h * 512];
            const uint32_t c = fine[threshold - 1 - h * 512];
            excess = inBins - considered;
            // lines 288-296: with an excess the first `excess` windows of the last bin are taken and the rest of it is not
            const uint32_t fromLast = excess > 0 ? excess : c;
            selected = (inBins - c) + fromLast;
            if (selected > considered) selected = considered;
        }
    }
    if (lane == 0) {
        outCount[s] = 1 + selected;
        outThr[s] = threshold;
        outExcess[s] = excess;
        outCons[s] = considered;
    }
}

__global__ void __launch_bounds__(64)
km_emit_kernel(KmPar p, const uint8_t *__restrict__ residues, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ keys,
               uint32_t nSeq, const uint64_t *__restrict__ recOff, const uint32_t *__restrict__ thr, const uint32_t *__restrict__ exc,
               const uint32_t *__restrict__ cons, uint32_t *__restrict__ rKeyHi, uint32_t *__restrict__ rKeyLo, uint32_t *__restrict__ rId,
               uint32_t *__restrict__ rLen, uint32_t *__restrict__ rPos) {
    __shared__ uint8_t codes[KM_CHUNK + KM_MAXK];
    __shared__ uint8_t map[24];
    const uint32_t s = blockIdx.x;
    const int lane = threadIdx.x;
    if (s >= nSeq) return;
    const uint64_t off = offsets[s];
    const uint32_t L = (uint32_t) (offsets[s + 1] - off);
    const uint8_t *res = residues + off;
    if (lane < 21) map[lane] = p.map[lane];
    __syncthreads();
    const uint64_t at0 = recOff[s];
    const uint32_t nRec = (uint32_t) (recOff[s + 1] - at0);   // 1 + selected windows: no lane writes beyond it
    const uint32_t key = keys[s];
    // the identity record: XXH64(Util::hash(reduced codes, L)); Util::hash is sdSeqHash31 (sd_seqhash.h, shared with sd_clusthash.hip)
    {
        const uint64_t h = sdSeqHash31(map, res, L, lane);
        if (lane == 0) {
            const uint64_t k64 = kmXxh64Word(h, p.seed);
            rKeyHi[at0] = (uint32_t) (k64 >> 32);
            rKeyLo[at0] = (uint32_t) k64;
            rId[at0] = key;
            rLen[at0] = L;
            rPos[at0] = 0;
        }
    }
    const uint32_t considered = cons[s];
    if (considered == 0 || nRec <= 1) return;
    const uint32_t t0 = thr[s], excess = exc[s];
    const uint32_t nW = L - (uint32_t) p.k + 1;   // (considered > 0: the sequence has windows)
    uint32_t lastSeen = 0, selected = 0;
    const uint64_t below = ((uint64_t) 1 << lane) - 1;
    for (uint32_t base = 0; base < nW && selected < considered; base += KM_CHUNK) {
        uint64_t idx;
        uint32_t score;
        const bool ok = kmWindow(p, res, L, base, lane, map, codes, &idx, &score);
        const bool isLast = ok && score + 1 == t0;
        const uint64_t lastMask = __ballot(isLast);
        const uint32_t lastRank = lastSeen + (uint32_t) __popcll(lastMask & below);
        bool take = ok && (score + 1 < t0 || (isLast && (excess == 0 || lastRank < excess)));
        const uint64_t takeMask = __ballot(take);
        const uint32_t rank = selected + (uint32_t) __popcll(takeMask & below);
        take = take && rank < considered && 1 + rank < nRec;
        if (take) {
            const uint64_t at = at0 + 1 + rank;
            rKeyHi[at] = (uint32_t) (idx >> 32);
            rKeyLo[at] = (uint32_t) idx;
            rId[at] = key;
            rLen[at] = L;
            rPos[at] = base + (uint32_t) lane;
        }
        lastSeen += (uint32_t) __popcll(lastMask);
        selected += (uint32_t) __popcll(takeMask);
    }
}

// ---- assignGroup --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(KM_BLOCK)
km_start_kernel(const uint32_t *__restrict__ keyHi, const uint32_t *__restrict__ keyLo, uint32_t n, uint32_t *__restrict__ startOrZero) {
    const uint64_t i = (uint64_t) blockIdx.x * KM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const bool start = i == 0 || keyHi[i] != keyHi[i - 1] || keyLo[i] != keyLo[i - 1];
    startOrZero[i] = start ? (uint32_t) i : 0u;
}

// Util::canBeCovered (M/src/commons/Util.cpp:477-494), as sd::canBeCovered states it on the host
__device__ __forceinline__ bool kmCanBeCovered(float covThr, int covMode, float queryLength, float targetLength) {
    switch (covMode) {
        case 0: return ((queryLength / targetLength >= covThr) && (targetLength / queryLength >= covThr));
        case 2: return ((targetLength / queryLength) >= covThr);
        case 1: return ((queryLength / targetLength) >= covThr);
        case 3: return ((targetLength / queryLength) >= covThr) && (targetLength / queryLength) <= 1.0f;
        case 4: return ((queryLength / targetLength) >= covThr) && (queryLength / targetLength) <= 1.0f;
        case 5: return (fminf(targetLength, queryLength) / fmaxf(targetLength, queryLength)) >= covThr;
        default: return true;
    }
}

// flag has n + 1 entries (the last one 0: the scan's total)
__global__ void __launch_bounds__(KM_BLOCK)
km_groupflag_kernel(const uint32_t *__restrict__ keyHi, const uint32_t *__restrict__ keyLo, const uint32_t *__restrict__ len,
                    const uint32_t *__restrict__ pos, const uint32_t *__restrict__ runStart, uint32_t n, int onlyExtendable, int covMode,
                    float covThr, uint32_t *__restrict__ flag, uint32_t *__restrict__ largest) {
    const uint64_t i = (uint64_t) blockIdx.x * KM_BLOCK + threadIdx.x;
    if (i > n) return;
    uint32_t f = 0;
    if (i < n) {
        const uint32_t s = runStart[i];
        const bool single = (uint64_t) s + 1 >= n || keyHi[s + 1] != keyHi[s] || keyLo[s + 1] != keyLo[s];
        if (!single) {
            const int repLen = (int) len[s], memLen = (int) len[i];
            const int diagonal = (int) pos[s] - (int) pos[i];
            const bool extendable = diagonal < 0 || diagonal > repLen - memLen;
            const bool covered = kmCanBeCovered(covThr, covMode, (float) repLen, (float) memLen);
            f = ((!onlyExtendable && covered) || (extendable && onlyExtendable)) ? 1u : 0u;
        }
        const bool runEnd = i + 1 == n || keyHi[i + 1] != keyHi[i] || keyLo[i + 1] != keyLo[i];
        // (most runs are single records: only longer ones go to the one shared word; the host starts the statistic at 1)
        if (runEnd && (uint32_t) i > s) atomicMax(largest, (uint32_t) i - s + 1);
    }
    flag[i] = f;
}

__global__ void __launch_bounds__(KM_BLOCK)
km_groupwrite_kernel(const uint32_t *__restrict__ id, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ runStart,
                     const uint32_t *__restrict__ flag, const uint64_t *__restrict__ at, uint32_t n, uint32_t *__restrict__ gRep,
                     uint32_t *__restrict__ gId, uint32_t *__restrict__ gDiag) {
    const uint64_t i = (uint64_t) blockIdx.x * KM_BLOCK + threadIdx.x;
    if (i >= n || flag[i] == 0) return;
    const uint32_t s = runStart[i];
    const uint64_t w = at[i];
    gRep[w] = id[s];
    gId[w] = id[i];
    gDiag[w] = (uint32_t) ((int) pos[s] - (int) pos[i]);
}

// ---- writeKmerMatcherResult --------------------------------------------------------------------------------------------------------
// flag has w + 1 entries
__global__ void __launch_bounds__(KM_BLOCK)
km_hitflag_kernel(const uint32_t *__restrict__ hRep, const uint32_t *__restrict__ hId, uint32_t w, uint32_t *__restrict__ flag) {
    const uint64_t j = (uint64_t) blockIdx.x * KM_BLOCK + threadIdx.x;
    if (j > w) return;
    uint32_t f = 0;
    if (j < w) {
        const bool pairStart = j == 0 || hRep[j] != hRep[j - 1] || hId[j] != hId[j - 1];
        f = (pairStart && hId[j] != hRep[j]) ? 1u : 0u;
    }
    flag[j] = f;
}

// One thread per hit walks what the reference's inner loop walks (kmermatcher.cpp:947-965): the records from the first of the (rep,
// member) run on while the MEMBER id stays the same -- the loop does not look at the representative, so a run continues into the next
// representative's records when those start with the same member, and past the last grouped record into what assignGroup left behind
// there: the first sort's records w .. n - 1, whose id and pos fields it never overwrote.  Score = records walked; diagonal = the last
// value, in that order, whose run of equal values is at least as long as every run before it (`>=`).
__global__ void __launch_bounds__(KM_BLOCK)
km_hit_kernel(const uint32_t *__restrict__ hRep, const uint32_t *__restrict__ hId, const uint32_t *__restrict__ hDiag,
              const uint32_t *__restrict__ sId, const uint32_t *__restrict__ sPos, uint32_t w, uint32_t n, const uint32_t *__restrict__ flag,
              const uint64_t *__restrict__ at, uint32_t *__restrict__ outRep, uint32_t *__restrict__ outMember, uint32_t *__restrict__ outScore,
              int32_t *__restrict__ outDiag) {
    const uint64_t j = (uint64_t) blockIdx.x * KM_BLOCK + threadIdx.x;
    if (j >= w || flag[j] == 0) return;
    const uint32_t member = hId[j];
    int diagonal = (int) hDiag[j], prev = diagonal;
    uint32_t best = 0, run = 0, score = 0;
    for (uint64_t x = j; x < n; x++) {
        const uint32_t idHere = x < w ? hId[x] : sId[x];
        if (idHere != member) break;
        const int d = x < w ? (int) hDiag[x] : (int) sPos[x];
        run = d == prev ? run + 1 : 1;
        if (run >= best) {
            diagonal = d;
            best = run;
        }
        prev = d;
        score++;
    }
    const uint64_t o = at[j];
    outRep[o] = hRep[j];
    outMember[o] = member;
    outScore[o] = score;
    outDiag[o] = diagonal;
}

// What the records stage leaves on the device: the per-sequence selection, the record offsets, the emitted records (r*) and the
// workspace of everything behind it.  sd_kmermatch_batch goes on from here; sd_selftest_kmermatch_records copies it out.
struct KmStage {
    bool empty;   // no sequence: nothing was launched and no pointer is set
    uint64_t bound, nRec, maxLen;
    uint32_t maxKey;
    uint64_t *dRecOff, *dScanTmp, *dAt;
    uint32_t *dThr, *dExc, *dConsOut, *dLargest, *dRunStart, *dFlag;
    uint32_t *rKeyHi, *rKeyLo, *rId, *rLen, *rPos, *sKeyHi, *sKeyLo, *sId, *sLen, *sPos;
    FieldSortBufs sb;
};

// Validation, workspace, upload, km_select_kernel, the scan of the record counts and km_emit_kernel (queued on the context's stream when
// this returns).  `who` names the entry point in messages.
int kmRecordsStage(sd_ctx *ctx, const char *who, const sd_kmermatch_params *par, uint64_t nSeq, const uint8_t *residues,
                   const uint64_t *offsets, const uint32_t *keys, const uint8_t *letterMap, KmStage *stage) {
    memset(stage, 0, sizeof(*stage));
    if (nSeq && (!residues || !keys)) return SD_EINVAL;
    if (nSeq > (uint64_t) INT32_MAX) return sdFail(ctx, SD_EUNSUPPORTED, "%s: %llu sequences in one call", who, (unsigned long long) nSeq);
    if (par->alphabetSize < 2 || par->alphabetSize > 21) return sdFail(ctx, SD_EINVAL, "%s: alphabet size %d", who, par->alphabetSize);
    if (par->kmerSize < 1 || par->kmerSize > KM_MAXK) return sdFail(ctx, SD_EINVAL, "%s: k-mer size %d (1 .. %d)", who, par->kmerSize, KM_MAXK);
    if (par->kmersPerSequence < 1) return sdFail(ctx, SD_EINVAL, "%s: --kmer-per-seq %d", who, par->kmersPerSequence);
    if (par->covMode < 0 || par->covMode > 5) return sdFail(ctx, SD_EINVAL, "%s: coverage mode %d", who, par->covMode);
    KmPar kp;
    memset(&kp, 0, sizeof(kp));
    kp.k = par->kmerSize;
    kp.xCode = (uint32_t) par->alphabetSize - 1;
    kp.seed = (uint64_t) (int64_t) par->hashShift;
    {
        uint64_t pw = 1;
        for (int j = 0; j < kp.k; j++) {
            kp.pw[j] = pw;
            if (j + 1 < kp.k && pw > UINT64_MAX / (uint64_t) (par->alphabetSize - 1))
                return sdFail(ctx, SD_EUNSUPPORTED, "%s: %d^%d does not fit the 64-bit k-mer index", who, par->alphabetSize - 1, kp.k);
            pw *= (uint64_t) (par->alphabetSize - 1);
        }
    }
    // Timed as km_prepare; the first-use allocations behind it as km_alloc
    std::unique_ptr<HostScope> phase(new HostScope(ctx, "km_prepare"));
    SdSeqBatch batch;
    const int rcCheck = sdCheckSeqBatch(ctx, who, par->alphabetSize, nSeq, residues, offsets, letterMap, &batch);
    if (rcCheck != SD_OK) return rcCheck;
    memcpy(kp.map, batch.map, sizeof(kp.map));
    const uint64_t maxLen = batch.maxLen, total = batch.total;
    // per sequence: kmerConsidered before the window count caps it (kmermatcher.cpp:204-206: sd_host_kmermatch_considered, the product
    // rounded to float before the sum, whatever this file's compiler would contract), and the record bound
    std::vector<uint32_t> cons(nSeq ? nSeq : 1);
    uint64_t bound = 0;
    uint32_t maxKey = 0;
    for (uint64_t s = 0; s < nSeq; s++) {
        const uint64_t L = offsets[s + 1] - offsets[s];
        const uint64_t considered = sd_host_kmermatch_considered(par->kmersPerSequence, par->kmersPerSequenceScale, (uint32_t) L);
        const uint64_t windows = L >= (uint64_t) kp.k ? L - (uint64_t) kp.k + 1 : 0;
        cons[s] = (uint32_t) std::min(considered, windows);
        bound += 1 + cons[s];
        maxKey = std::max(maxKey, keys[s]);
    }
    if (nSeq == 0) {
        stage->empty = true;
        return SD_OK;
    }
    if (bound > RS_MAX_ELEMENTS)
        return sdFail(ctx, SD_ENOMEM, "%s: up to %llu records in one call (the device sort counts in 32 bits: at most %llu); %llu bytes needed",
                      who, (unsigned long long) bound, (unsigned long long) RS_MAX_ELEMENTS, (unsigned long long) (bound * SD_KMERMATCH_BYTES_PER_RECORD + total));
    // everything is resident at once (the reference would split by hash range here, with scores saturated to a byte: another output)
    {
        const uint64_t need = bound * SD_KMERMATCH_BYTES_PER_RECORD + total + nSeq * 40;
        uint64_t avail = 0;   // (what this context's kmermatcher workspace already holds counts as available)
        SD_HIP(ctx, wsAvailableBytes(ctx, "km.", &avail));
        if (need > avail)
            return sdFail(ctx, SD_ENOMEM, "%s: %llu bytes needed for up to %llu records, %llu free on the device (splitting by hash range is not implemented)",
                          who, (unsigned long long) need, (unsigned long long) bound, (unsigned long long) avail);
    }
    const uint32_t n32 = (uint32_t) nSeq;
    hipStream_t st = ctx->stream;
    phase.reset(new HostScope(ctx, "km_alloc"));
    uint8_t *dRes = nullptr;
    uint64_t *dOff = nullptr, *dRecOff = nullptr, *dScanTmp = nullptr, *dAt = nullptr;
    uint32_t *dKeys = nullptr, *dCons = nullptr, *dCount = nullptr, *dThr = nullptr, *dExc = nullptr, *dConsOut = nullptr, *dLargest = nullptr;
    SD_HIP(ctx, wsGet(ctx, "km.res", (size_t) total, &dRes));
    SD_HIP(ctx, wsGet(ctx, "km.off", (size_t) nSeq + 1, &dOff));
    SD_HIP(ctx, wsGet(ctx, "km.recoff", (size_t) nSeq + 1, &dRecOff));
    SD_HIP(ctx, wsGet(ctx, "km.keys", (size_t) nSeq, &dKeys));
    SD_HIP(ctx, wsGet(ctx, "km.cons", (size_t) nSeq, &dCons));
    SD_HIP(ctx, wsGet(ctx, "km.count", (size_t) nSeq + 1, &dCount));
    SD_HIP(ctx, wsGet(ctx, "km.thr", (size_t) nSeq, &dThr));
    SD_HIP(ctx, wsGet(ctx, "km.exc", (size_t) nSeq, &dExc));
    SD_HIP(ctx, wsGet(ctx, "km.consout", (size_t) nSeq, &dConsOut));
    SD_HIP(ctx, wsGet(ctx, "km.largest", (size_t) 1, &dLargest));
    SD_HIP(ctx, wsGet(ctx, "km.scantmp", sdScanTmpBytes(std::max(bound, nSeq) + 1) / sizeof(uint64_t), &dScanTmp));
    // per record: the five fields as emitted (r*), the same sorted (s*), the sort's three (key, permutation) pairs, run start, flag, place
    uint32_t *rKeyHi, *rKeyLo, *rId, *rLen, *rPos, *sKeyHi, *sKeyLo, *sId, *sLen, *sPos, *dRunStart, *dFlag;
    FieldSortBufs sb;
    SD_HIP(ctx, wsGet(ctx, "km.rkeyhi", (size_t) bound, &rKeyHi));
    SD_HIP(ctx, wsGet(ctx, "km.rkeylo", (size_t) bound, &rKeyLo));
    SD_HIP(ctx, wsGet(ctx, "km.rid", (size_t) bound, &rId));
    SD_HIP(ctx, wsGet(ctx, "km.rlen", (size_t) bound, &rLen));
    SD_HIP(ctx, wsGet(ctx, "km.rpos", (size_t) bound, &rPos));
    SD_HIP(ctx, wsGet(ctx, "km.skeyhi", (size_t) bound, &sKeyHi));
    SD_HIP(ctx, wsGet(ctx, "km.skeylo", (size_t) bound, &sKeyLo));
    SD_HIP(ctx, wsGet(ctx, "km.sid", (size_t) bound, &sId));
    SD_HIP(ctx, wsGet(ctx, "km.slen", (size_t) bound, &sLen));
    SD_HIP(ctx, wsGet(ctx, "km.spos", (size_t) bound, &sPos));
    SD_HIP(ctx, fieldSortBufsGet(ctx, "km.", (size_t) bound, &sb));
    SD_HIP(ctx, wsGet(ctx, "km.runstart", (size_t) bound, &dRunStart));
    SD_HIP(ctx, wsGet(ctx, "km.flag", (size_t) bound + 1, &dFlag));
    SD_HIP(ctx, wsGet(ctx, "km.at", (size_t) bound + 1, &dAt));
    phase.reset();
    {
        HostScope hs(ctx, "km_copy_in");
        SD_HIP(ctx, hipMemcpyAsync(dRes, residues, (size_t) total, hipMemcpyHostToDevice, st));
        SD_HIP(ctx, hipMemcpyAsync(dOff, offsets, ((size_t) nSeq + 1) * 8, hipMemcpyHostToDevice, st));
        SD_HIP(ctx, hipMemcpyAsync(dKeys, keys, (size_t) nSeq * 4, hipMemcpyHostToDevice, st));
        SD_HIP(ctx, hipMemcpyAsync(dCons, cons.data(), (size_t) nSeq * 4, hipMemcpyHostToDevice, st));
        SD_HIP(ctx, hipMemsetAsync(dCount, 0, ((size_t) nSeq + 1) * 4, st));
        SD_HIP(ctx, hipMemsetAsync(dLargest, 0, 4, st));
        SD_HIP(ctx, sdStreamSync(ctx));   // (cons is a local vector)
    }
    uint64_t nRec = 0;
    {
        HostScope hs(ctx, "km_records");
        hipLaunchKernelGGL(km_select_kernel, dim3(n32), dim3(64), 0, st, kp, (const uint8_t *) dRes, (const uint64_t *) dOff, (const uint32_t *) dCons,
                           n32, dCount, dThr, dExc, dConsOut);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, (sdScanLaunch<uint32_t, ScanSum64, false, uint64_t>(st, dCount, dRecOff, nSeq + 1, dScanTmp)));
        SD_HIP(ctx, sdD2H(ctx, &nRec, dRecOff + nSeq, 8));
        SD_HIP(ctx, sdStreamSync(ctx));
        if (nRec > bound) return sdFail(ctx, SD_EHIP, "%s: %llu records counted, at most %llu expected", who, (unsigned long long) nRec, (unsigned long long) bound);
        hipLaunchKernelGGL(km_emit_kernel, dim3(n32), dim3(64), 0, st, kp, (const uint8_t *) dRes, (const uint64_t *) dOff, (const uint32_t *) dKeys, n32,
                           (const uint64_t *) dRecOff, (const uint32_t *) dThr, (const uint32_t *) dExc, (const uint32_t *) dConsOut, rKeyHi, rKeyLo, rId,
                           rLen, rPos);
        SD_HIP(ctx, hipGetLastError());
        if (ctx->profiling) SD_HIP(ctx, sdStreamSync(ctx));
    }
    stage->bound = bound;
    stage->nRec = nRec;
    stage->maxLen = maxLen;
    stage->maxKey = maxKey;
    stage->dRecOff = dRecOff;
    stage->dScanTmp = dScanTmp;
    stage->dAt = dAt;
    stage->dThr = dThr;
    stage->dExc = dExc;
    stage->dConsOut = dConsOut;
    stage->dLargest = dLargest;
    stage->dRunStart = dRunStart;
    stage->dFlag = dFlag;
    stage->rKeyHi = rKeyHi;
    stage->rKeyLo = rKeyLo;
    stage->rId = rId;
    stage->rLen = rLen;
    stage->rPos = rPos;
    stage->sKeyHi = sKeyHi;
    stage->sKeyLo = sKeyLo;
    stage->sId = sId;
    stage->sLen = sLen;
    stage->sPos = sPos;
    stage->sb = sb;
    return SD_OK;
}

}  // namespace

extern "C" {

int sd_kmermatch_batch(sd_ctx *ctx, const sd_kmermatch_params *par, uint64_t nSeq, const uint8_t *residues, const uint64_t *offsets,
                       const uint32_t *keys, const uint8_t *letterMap, uint64_t outCap, uint32_t *outRep, uint32_t *outMember,
                       uint32_t *outScore, int32_t *outDiag, uint64_t *stats) {
    if (!ctx || !par || !offsets || !letterMap) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    KmStage stage;
    const int rcStage = kmRecordsStage(ctx, "sd_kmermatch_batch", par, nSeq, residues, offsets, keys, letterMap, &stage);
    if (rcStage != SD_OK || stage.empty) return rcStage;
    hipStream_t st = ctx->stream;
    const uint64_t nRec = stage.nRec, maxLen = stage.maxLen;
    const uint32_t maxKey = stage.maxKey;
    uint64_t *dScanTmp = stage.dScanTmp, *dAt = stage.dAt;
    uint32_t *dLargest = stage.dLargest, *dRunStart = stage.dRunStart, *dFlag = stage.dFlag;
    uint32_t *rKeyHi = stage.rKeyHi, *rKeyLo = stage.rKeyLo, *rId = stage.rId, *rLen = stage.rLen, *rPos = stage.rPos;
    uint32_t *sKeyHi = stage.sKeyHi, *sKeyLo = stage.sKeyLo, *sId = stage.sId, *sLen = stage.sLen, *sPos = stage.sPos;
    const FieldSortBufs &sb = stage.sb;
    const uint32_t r32 = (uint32_t) nRec;
    if (stats) stats[0] = nRec;
    const int idBits = bitsFor(maxKey), lenBits = bitsFor(maxLen);
    {
        HostScope hs(ctx, "km_sort1");
        // compareRepSequenceAndIdAndPos, least significant field first.  The identity records are 64-bit hashes: the key takes all its bits
        SD_HIP(ctx, sortByField(st, sb, rPos, nullptr, r32, FS_PLAIN, 0, lenBits));
        SD_HIP(ctx, sortByField(st, sb, rId, sb.permA, r32, FS_PLAIN, 0, idBits));
        SD_HIP(ctx, sortByField(st, sb, rLen, sb.permA, r32, FS_FROM_TOP, (uint32_t) maxLen, lenBits));
        SD_HIP(ctx, sortByField(st, sb, rKeyLo, sb.permA, r32, FS_PLAIN, 0, 32));
        SD_HIP(ctx, sortByField(st, sb, rKeyHi, sb.permA, r32, FS_PLAIN, 0, 32));
        const uint32_t *src[5] = {rKeyHi, rKeyLo, rId, rLen, rPos};
        uint32_t *dst[5] = {sKeyHi, sKeyLo, sId, sLen, sPos};
        SD_HIP(ctx, gatherFields(st, sb.permA, r32, 5, src, dst));
        if (ctx->profiling) SD_HIP(ctx, sdStreamSync(ctx));
    }
    uint64_t nGroup = 0;
    uint32_t largest = 0;
    // the grouped records reuse the emitted fields' arrays, which the first sort has finished with
    uint32_t *gRep = rKeyHi, *gId = rKeyLo, *gDiag = rId, *hRep = rLen, *hId = rPos, *hDiag = sKeyHi;
    {
        HostScope hs(ctx, "km_group");
        hipLaunchKernelGGL(km_start_kernel, dim3(gridFor(nRec, KM_BLOCK)), dim3(KM_BLOCK), 0, st, (const uint32_t *) sKeyHi, (const uint32_t *) sKeyLo, r32, dFlag);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, (sdScanLaunch<uint32_t, ScanMax32, true, uint32_t>(st, dFlag, dRunStart, nRec, (uint32_t *) dScanTmp)));
        hipLaunchKernelGGL(km_groupflag_kernel, dim3(gridFor(nRec + 1, KM_BLOCK)), dim3(KM_BLOCK), 0, st, (const uint32_t *) sKeyHi, (const uint32_t *) sKeyLo,
                           (const uint32_t *) sLen, (const uint32_t *) sPos, (const uint32_t *) dRunStart, r32, par->includeOnlyExtendable ? 1 : 0,
                           par->covMode, par->covThr, dFlag, dLargest);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, (sdScanLaunch<uint32_t, ScanSum64, false, uint64_t>(st, dFlag, dAt, nRec + 1, dScanTmp)));
        hipLaunchKernelGGL(km_groupwrite_kernel, dim3(gridFor(nRec, KM_BLOCK)), dim3(KM_BLOCK), 0, st, (const uint32_t *) sId, (const uint32_t *) sPos,
                           (const uint32_t *) dRunStart, (const uint32_t *) dFlag, (const uint64_t *) dAt, r32, gRep, gId, gDiag);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, sdD2H(ctx, &nGroup, dAt + nRec, 8));
        SD_HIP(ctx, sdD2H(ctx, &largest, dLargest, 4));
        SD_HIP(ctx, sdStreamSync(ctx));
    }
    const uint32_t w32 = (uint32_t) nGroup;
    if (stats) {
        stats[1] = nGroup;
        stats[3] = largest > 1 ? largest : (nRec ? 1 : 0);
    }
    uint64_t nHits = 0;
    if (nGroup > 0) {
        {
            HostScope hs(ctx, "km_sort2");
            // compareRepSequenceAndIdAndDiag; the diagonal is signed: biased by the longest sequence it sorts as an unsigned value
            SD_HIP(ctx, sortByField(st, sb, gDiag, nullptr, w32, FS_BIASED, (uint32_t) maxLen, bitsFor(2 * maxLen)));
            SD_HIP(ctx, sortByField(st, sb, gId, sb.permA, w32, FS_PLAIN, 0, idBits));
            SD_HIP(ctx, sortByField(st, sb, gRep, sb.permA, w32, FS_PLAIN, 0, idBits));
            const uint32_t *src[3] = {gRep, gId, gDiag};
            uint32_t *dst[3] = {hRep, hId, hDiag};
            SD_HIP(ctx, gatherFields(st, sb.permA, w32, 3, src, dst));
            if (ctx->profiling) SD_HIP(ctx, sdStreamSync(ctx));
        }
        HostScope hs(ctx, "km_hits");
        hipLaunchKernelGGL(km_hitflag_kernel, dim3(gridFor(nGroup + 1, KM_BLOCK)), dim3(KM_BLOCK), 0, st, (const uint32_t *) hRep, (const uint32_t *) hId, w32, dFlag);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, (sdScanLaunch<uint32_t, ScanSum64, false, uint64_t>(st, dFlag, dAt, nGroup + 1, dScanTmp)));
        SD_HIP(ctx, sdD2H(ctx, &nHits, dAt + nGroup, 8));
        SD_HIP(ctx, sdStreamSync(ctx));
    }
    if (stats) stats[2] = nHits;
    if (nHits > outCap)
        return sdFail(ctx, SD_ENOMEM, "sd_kmermatch_batch: %llu hits, room for %llu", (unsigned long long) nHits, (unsigned long long) outCap);
    if (nHits == 0) return SD_OK;
    if (!outRep || !outMember || !outScore || !outDiag) return SD_EINVAL;
    // (the sort's buffers are free again: nHits <= nGroup <= bound)
    uint32_t *dOutRep = sb.keyIn, *dOutMember = sb.permIn, *dOutScore = sb.keyA;
    int32_t *dOutDiag = (int32_t *) sb.keyB;
    {
        HostScope hs(ctx, "km_hits");
        hipLaunchKernelGGL(km_hit_kernel, dim3(gridFor(nGroup, KM_BLOCK)), dim3(KM_BLOCK), 0, st, (const uint32_t *) hRep, (const uint32_t *) hId,
                           (const uint32_t *) hDiag, (const uint32_t *) sId, (const uint32_t *) sPos, w32, r32, (const uint32_t *) dFlag,
                           (const uint64_t *) dAt, dOutRep, dOutMember, dOutScore, dOutDiag);
        SD_HIP(ctx, hipGetLastError());
        if (ctx->profiling) SD_HIP(ctx, sdStreamSync(ctx));
    }
    {
        HostScope hs(ctx, "km_copy_out");
        SD_HIP(ctx, hipMemcpyAsync(outRep, dOutRep, (size_t) nHits * 4, hipMemcpyDeviceToHost, st));
        SD_HIP(ctx, hipMemcpyAsync(outMember, dOutMember, (size_t) nHits * 4, hipMemcpyDeviceToHost, st));
        SD_HIP(ctx, hipMemcpyAsync(outScore, dOutScore, (size_t) nHits * 4, hipMemcpyDeviceToHost, st));
        SD_HIP(ctx, hipMemcpyAsync(outDiag, dOutDiag, (size_t) nHits * 4, hipMemcpyDeviceToHost, st));
        SD_HIP(ctx, sdStreamSync(ctx));
    }
    return SD_OK;
}

int sd_selftest_kmermatch_records(sd_ctx *ctx, const sd_kmermatch_params *par, uint64_t nSeq, const uint8_t *residues, const uint64_t *offsets,
                                  const uint32_t *keys, const uint8_t *letterMap, uint64_t recCap, uint32_t *seqConsidered,
                                  uint32_t *seqThreshold, uint32_t *seqExcess, uint64_t *recOff, uint64_t *recKey, uint32_t *recId,
                                  uint32_t *recLen, uint32_t *recPos, uint64_t *stats) {
    if (!ctx || !par || !offsets || !letterMap) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    if (stats) stats[0] = 0;
    KmStage stage;
    const int rcStage = kmRecordsStage(ctx, "sd_selftest_kmermatch_records", par, nSeq, residues, offsets, keys, letterMap, &stage);
    if (rcStage != SD_OK) return rcStage;
    if (stage.empty) {
        if (recOff) recOff[0] = 0;
        return SD_OK;
    }
    const uint64_t nRec = stage.nRec;
    if (stats) stats[0] = nRec;
    if (nRec > recCap)
        return sdFail(ctx, SD_ENOMEM, "sd_selftest_kmermatch_records: %llu records, room for %llu", (unsigned long long) nRec, (unsigned long long) recCap);
    if (!seqConsidered || !seqThreshold || !seqExcess || !recOff || !recKey || !recId || !recLen || !recPos) return SD_EINVAL;
    hipStream_t st = ctx->stream;
    std::vector<uint32_t> hi((size_t) nRec), lo((size_t) nRec);
    SD_HIP(ctx, hipMemcpyAsync(seqConsidered, stage.dConsOut, (size_t) nSeq * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipMemcpyAsync(seqThreshold, stage.dThr, (size_t) nSeq * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipMemcpyAsync(seqExcess, stage.dExc, (size_t) nSeq * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipMemcpyAsync(recOff, stage.dRecOff, ((size_t) nSeq + 1) * 8, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipMemcpyAsync(hi.data(), stage.rKeyHi, (size_t) nRec * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipMemcpyAsync(lo.data(), stage.rKeyLo, (size_t) nRec * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipMemcpyAsync(recId, stage.rId, (size_t) nRec * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipMemcpyAsync(recLen, stage.rLen, (size_t) nRec * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipMemcpyAsync(recPos, stage.rPos, (size_t) nRec * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, sdStreamSync(ctx));
    sdJoinHiLo(hi.data(), lo.data(), nRec, recKey);
    return SD_OK;
}

int sd_selftest_field_sort(sd_ctx *ctx, uint32_t n, int nFields, const uint32_t *fields, const int32_t *modes, const uint32_t *args,
                           const int32_t *bits, uint32_t *outPerm, uint32_t *outFields) {
    if (!ctx || nFields < 1 || nFields > 5 || !modes || !args || !bits || (n && (!fields || !outPerm || !outFields))) return SD_EINVAL;
    for (int f = 0; f < nFields; f++)
        if (modes[f] < FS_PLAIN || modes[f] > FS_BIASED || bits[f] < 1 || bits[f] > 32) return SD_EINVAL;
    if (n > RS_MAX_ELEMENTS) return SD_EUNSUPPORTED;
    (void) hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t all = (size_t) nFields * n;
    uint32_t *dIn = nullptr, *dOut = nullptr;
    FieldSortBufs sb;
    SD_HIP(ctx, wsGet(ctx, "fs.in", all, &dIn));
    SD_HIP(ctx, wsGet(ctx, "fs.out", all, &dOut));
    SD_HIP(ctx, fieldSortBufsGet(ctx, "fs.", n, &sb));
    if (n) SD_HIP(ctx, hipMemcpyAsync(dIn, fields, all * 4, hipMemcpyHostToDevice, st));
    const uint32_t *src[5];
    uint32_t *dst[5];
    for (int f = 0; f < nFields; f++) {
        src[f] = dIn + (size_t) f * n;
        dst[f] = dOut + (size_t) f * n;
        SD_HIP(ctx, sortByField(st, sb, src[f], f ? sb.permA : nullptr, n, modes[f], args[f], bits[f]));
    }
    SD_HIP(ctx, gatherFields(st, sb.permA, n, nFields, src, dst));
    if (n == 0) return SD_OK;   // (the shared functions launch nothing then)
    SD_HIP(ctx, hipMemcpyAsync(outPerm, sb.permA, (size_t) n * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipMemcpyAsync(outFields, dOut, all * 4, hipMemcpyDeviceToHost, st));
    SD_HIP(ctx, hipStreamSynchronize(st));
    return SD_OK;
}

}  // extern "C"
