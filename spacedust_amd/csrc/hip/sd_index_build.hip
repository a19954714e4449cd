// Target index construction on the device.  Three builders, one per kind of target index:
//   sd_target_build          the plain sequence index (k = 6 or 7): every target tantan-masked, its own k-mers at or above kmerThr
//   sd_target_build_profile  a profile target DB (k = 5 or 6): the similar k-mers of every profile window, nothing masked
//   sd_target_build_similar  a sequence target under --target-search-mode 1 (k = 6): the similar k-mers of every sequence window
//
// What IndexBuilder::fillDatabase does on the host for the first (M/src/prefiltering/IndexBuilder.cpp:55-239; sd_index.cpp is the
// host restatement this file is tested against, entry for entry):
//   1. every target is tantan-masked to X (M/src/commons/Masker.cpp:15-55, M/lib/tantan/tantan.cpp:308-460),
//   2. per target, the spaced k-mers without X whose self score reaches kmerThr are collected, each distinct k-mer once per
//      target at its smallest position (IndexTable.h:131-166,376-392),
//   3. the lists are ordered by (target, position) (IndexTable.h:182-189).
// The other two differ in step 2 only (the comments at their generators say how).
//
// What the builders share (IndexBuild): a builder uploads what is its own and supplies a record generator that runs in three
// modes -- 0: histogram of its records over IB_COARSE_BINS k-mer ranges, 1: records of a k-mer range [lo, hi) per slot (what one
// wavefront writes in order), 2: the records themselves.  The frame cuts the k-mer space into passes along the histogram
// (ibPassCap) and per pass counts, scans, emits, sorts and dedupes (ibPasses), then turns the per-k-mer counts into list starts
// (ibListStarts).
//
// On the MI355X:
//   ib_mask_kernel     one lane per target sequence, 64 sequences of similar length per wavefront (the host deals them out by
//                      length).  The 50 repeat-offset states of tantan's HMM live in 100 VGPRs, the window of the last 50
//                      residues in 53 more, the 21 x 21 likelihood ratios in LDS; forward pass, backward pass, mask bytes.
//                      Double precision with the operation order and the fused multiply-adds of the host build (4 partial
//                      sums over the offsets combined as (s0 + s2) + (s1 + s3), see sd_tantan.cpp); that the float posterior
//                      compared with --mask-prob then has the reference's bits is checked residue by residue in
//                      tests/test_gpu_tantan.py (through sd_selftest_mask).  The forward posteriors (one float per residue)
//                      and the rescaling factors are kept between the passes in a scratch buffer laid out [position][lane].
//   ib_records_kernel<K, MODE>  the plain builder's generator.  Per k-mer range [lo, hi) that fits the sort buffers: (k-mer - lo,
//                      target << 16 | position) records of the masked sequences in (target, position) order -- a wavefront walks
//                      its 16 sequences 64 positions at a time, ballots keep the order.  ib_profile_records_kernel<MODE> and
//                      ib_similar_records_kernel<MODE> are the generators of the other two builders: a wavefront per window.
//   sdRadixSortPairs   stable radix sort of a pass's records by k-mer (sd_scan_sort.h: this library's own, as are the scans),
//   ib_keep_count / ib_place  adjacent records of one (k-mer, target) collapse to the first (= smallest position), the survivors
//                      are appended to the entry array (8 B each, the layout the prefilter kernels read) and counted per k-mer,
//   ib_offsets         after a 64-bit exclusive scan of the counts (sdScanLaunch): 32-bit starts, relative to one 64-bit base
//                      per 65 536 k-mers when the index has 2^32 entries or more (the wide form of sd_target_create_wide).
// Algorithmic bytes: 1 B read + 1 B written per residue for the mask (+ 8 B of scratch traffic), 8 B written per entry; the
// sort moves 12 B x 2 x 4 passes per record.
#include "sd_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

#pragma clang fp contract(off)   // every fused multiply-add below is written out: the host build's contractions, no others

namespace {

// the radix sort of the (k-mer, record) pairs and the scans of the counts: this library's own kernels
#include "sd_scan_sort.h"

constexpr int TT_OFF = 50;       // maxCycleLength (Masker.cpp:20-32)
constexpr int TT_SCALE = 16;     // rescaling period (tantan.cpp)
constexpr int TT_RAMP = 52;      // positions walked one at a time (the first 50 reach back to the sequence start only)
constexpr int IB_X = 20;         // residue code of X
constexpr int IB_ALPH = 21;

struct TantanPar {
    double b2b, f2b, f2f0;
    double b2f[TT_OFF];
};
__constant__ TantanPar c_tt;
__constant__ uint8_t c_ibSeed[8];
__constant__ int c_ibSelf[IB_ALPH];
__constant__ uint32_t c_ibPow[8];

struct MaskLane {
    double fg[TT_OFF];
    uint32_t W[TT_OFF + 3];   // residues (as byte offsets into a row of likelihood ratios) around the current block
    const char *lr;           // LDS
    __device__ __forceinline__ double ratio(uint32_t row, uint32_t w) const { return *(const double *) (lr + row + w); }
};

// forward step over all 50 offsets; the offsets' residues are W[SH + i]
template <int SH>
__device__ __forceinline__ double fwdFull(MaskLane &m, uint32_t row, double b) {
    const double f2f0 = c_tt.f2f0;
    double s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 48; i++) {
        const double f = m.fg[i];
        s[i & 3] += f;
        m.fg[i] = fma(c_tt.b2f[i], b, f * f2f0) * m.ratio(row, m.W[SH + i]);
    }
    double sum = (s[0] + s[2]) + (s[1] + s[3]);
#pragma unroll
    for (int i = 48; i < TT_OFF; i++) {
        const double f = m.fg[i];
        sum += f;
        m.fg[i] = fma(c_tt.b2f[i], b, f * f2f0) * m.ratio(row, m.W[SH + i]);
    }
    return sum;
}
// ... over the first maxOffset (wave-uniform, <= 50) offsets, residues W[i]
__device__ __forceinline__ double fwdPart(MaskLane &m, uint32_t row, double b, int maxOffset) {
    const double f2f0 = c_tt.f2f0;
    const int full = maxOffset & ~3;
    double s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 48; i++) {
        if (i < full) {
            const double f = m.fg[i];
            s[i & 3] += f;
            m.fg[i] = fma(c_tt.b2f[i], b, f * f2f0) * m.ratio(row, m.W[i]);
        }
    }
    double sum = (s[0] + s[2]) + (s[1] + s[3]);
#pragma unroll
    for (int i = 0; i < TT_OFF; i++) {
        if (i >= full && i < maxOffset) {
            const double f = m.fg[i];
            sum += f;
            m.fg[i] = fma(c_tt.b2f[i], b, f * f2f0) * m.ratio(row, m.W[i]);
        }
    }
    return sum;
}
template <int SH>
__device__ __forceinline__ double bwdFull(MaskLane &m, uint32_t row, double toBg) {
    const double f2f0 = c_tt.f2f0;
    double s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 48; i++) {
        const double f = m.fg[i] * m.ratio(row, m.W[SH + i]);
        s[i & 3] = fma(c_tt.b2f[i], f, s[i & 3]);
        m.fg[i] = fma(f, f2f0, toBg);
    }
    double sum = (s[0] + s[2]) + (s[1] + s[3]);
#pragma unroll
    for (int i = 48; i < TT_OFF; i++) {
        const double f = m.fg[i] * m.ratio(row, m.W[SH + i]);
        sum = fma(c_tt.b2f[i], f, sum);
        m.fg[i] = fma(f, f2f0, toBg);
    }
    return sum;
}
__device__ __forceinline__ double bwdPart(MaskLane &m, uint32_t row, double toBg, int maxOffset) {
    const double f2f0 = c_tt.f2f0;
    const int full = maxOffset & ~3;
    double s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 48; i++) {
        if (i < full) {
            const double f = m.fg[i] * m.ratio(row, m.W[i]);
            s[i & 3] = fma(c_tt.b2f[i], f, s[i & 3]);
            m.fg[i] = fma(f, f2f0, toBg);
        }
    }
    double sum = (s[0] + s[2]) + (s[1] + s[3]);
#pragma unroll
    for (int i = 0; i < TT_OFF; i++) {
        if (i >= full && i < maxOffset) {
            const double f = m.fg[i] * m.ratio(row, m.W[i]);
            sum = fma(c_tt.b2f[i], f, sum);
            m.fg[i] = fma(f, f2f0, toBg);
        }
    }
    return sum;
}

// One lane = one sequence; the lanes of a wavefront walk their sequences in step from residue 0 (position `pos` is
// wave-uniform; a lane whose sequence is shorter keeps computing on clamped residues, its stores are off and what it needs
// from the end of its own sequence -- z after the forward pass, the initial state of the backward pass -- is taken / set at
// the position where its sequence ends).
// probT / scaleT: per wavefront rows x 64 floats and rows / 16 x 64 doubles (rows = its longest sequence rounded up to 16),
// starting at row waveRow[w].
__global__ void __launch_bounds__(64)
ib_mask_kernel(const uint8_t *__restrict__ res, const uint64_t *__restrict__ seqOff, const uint32_t *__restrict__ order, uint32_t nSeq,
               const double *__restrict__ lrTable, const uint64_t *__restrict__ waveRow, float *__restrict__ probT,
               double *__restrict__ scaleT, double minMaskProb, uint8_t *__restrict__ masked, unsigned long long *__restrict__ nMasked,
               uint32_t waveBase /* first wavefront of this launch: the scratch holds the rows of [waveBase, waveBase + gridDim.x) */) {
    __shared__ double lr[IB_ALPH * IB_ALPH];
    for (int i = threadIdx.x; i < IB_ALPH * IB_ALPH; i += 64) lr[i] = lrTable[i];
    __syncthreads();
    const uint32_t wave = waveBase + blockIdx.x, lane = threadIdx.x;
    const uint32_t slot = wave * 64 + lane;
    const bool have = slot < nSeq;
    const uint32_t seq = have ? order[slot] : 0;
    const uint64_t base = have ? seqOff[seq] : 0;
    const int L = have ? (int) (seqOff[seq + 1] - base) : 0;
    int maxLen = L;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) maxLen = max(maxLen, __shfl_xor(maxLen, o, 64));
    if (maxLen == 0) return;
    const uint8_t *s = res + base;
    uint8_t *out = masked + base;
    const uint64_t row0 = waveRow[wave] - waveRow[waveBase];
    float *prob = probT + row0 * 64 + lane;
    double *scale = scaleT + row0 / TT_SCALE * 64 + lane;
    const double b2b = c_tt.b2b, f2b = c_tt.f2b;
    auto at = [&](int i) -> uint32_t {   // residue i as a byte offset into a row of lr (clamped: lanes outside their sequence)
        i = i >= L ? L - 1 : i;
        i = i < 0 ? 0 : i;
        return L > 0 ? (uint32_t) s[i] * 8u : 0u;
    };
    MaskLane m;
    m.lr = (const char *) lr;
#pragma unroll
    for (int i = 0; i < TT_OFF; i++) m.fg[i] = 0.0;
#pragma unroll
    for (int j = 0; j < TT_OFF + 3; j++) m.W[j] = 0;
    double bg = 1.0, z = 1.0;

    auto endOfStep = [&](int pos, double fromFg, double b) {
        double nb = fma(b, b2b, fromFg * f2b);
        if ((pos & (TT_SCALE - 1)) == TT_SCALE - 1) {
            const double sc = 1.0 / nb;
            if (pos < L) scale[(size_t) (pos / TT_SCALE) * 64] = sc;
            nb *= sc;
#pragma unroll
            for (int j = 0; j < TT_OFF; j++) m.fg[j] *= sc;
        }
        bg = nb;
        if (pos < L) prob[(size_t) pos * 64] = (float) nb;
        if (__ballot(pos == L - 1)) {   // some sequence ends here: its normalisation constant
            double all = 0.0;
#pragma unroll
            for (int j = 0; j < TT_OFF; j++) all += m.fg[j];
            const double zc = fma(nb, b2b, all * f2b);
            z = pos == L - 1 ? zc : z;
        }
    };

    // ---------------- forward: the first positions one at a time (W[i] = residue pos - 1 - i) ...
    const int rampEnd = min(TT_RAMP, maxLen);
    for (int pos = 0; pos < rampEnd; pos++) {
        const uint32_t cur = at(pos);
        const double b = bg;
        const double fromFg = fwdPart(m, cur * IB_ALPH, b, min(pos, TT_OFF));
        endOfStep(pos, fromFg, b);
#pragma unroll
        for (int j = TT_OFF + 2; j >= 1; j--) m.W[j] = m.W[j - 1];
        m.W[0] = cur;
    }
    // ... then blocks of four: W[j] = residue P0 + 2 - j, position P0 + u reads its offsets at W[3 - u + i]
    if (maxLen > TT_RAMP) {
#pragma unroll
        for (int j = TT_OFF + 2; j >= 3; j--) m.W[j] = m.W[j - 3];
        for (int P0 = TT_RAMP; P0 < maxLen; P0 += 4) {
            const uint32_t r0 = at(P0), r1 = at(P0 + 1), r2 = at(P0 + 2), r3 = at(P0 + 3);
            m.W[2] = r0; m.W[1] = r1; m.W[0] = r2;
            {
                const double b = bg;
                endOfStep(P0, fwdFull<3>(m, r0 * IB_ALPH, b), b);
            }
            if (P0 + 1 < maxLen) {
                const double b = bg;
                endOfStep(P0 + 1, fwdFull<2>(m, r1 * IB_ALPH, b), b);
            }
            if (P0 + 2 < maxLen) {
                const double b = bg;
                endOfStep(P0 + 2, fwdFull<1>(m, r2 * IB_ALPH, b), b);
            }
            if (P0 + 3 < maxLen) {
                const double b = bg;
                endOfStep(P0 + 3, fwdFull<0>(m, r3 * IB_ALPH, b), b);
            }
#pragma unroll
            for (int j = TT_OFF + 2; j >= 4; j--) m.W[j] = m.W[j - 4];
            m.W[3] = r3;
        }
    }

    // ---------------- backward, from the wavefront's last position down; a lane joins at its own last residue
    const double f2bInit = f2b;
    unsigned long long nX = 0;
    auto backStep = [&](int pos, uint32_t cur, auto &&offsets) {
        if (__ballot(pos == L - 1)) {
            const bool start = pos == L - 1;
            bg = start ? b2b : bg;
#pragma unroll
            for (int j = 0; j < TT_OFF; j++) m.fg[j] = start ? f2bInit : m.fg[j];
        }
        const bool live = pos < L;
        const float fwd = live ? prob[(size_t) pos * 64] : 0.f;
        const double nonRepeat = (double) fwd * bg / z;
        const float p = 1 - (float) nonRepeat;
        if (live) {
            const bool x = (double) p >= minMaskProb;   // float against double, tantan.cpp:527
            out[pos] = x ? (uint8_t) IB_X : (uint8_t) (cur >> 3);
            nX += x ? 1 : 0;
        }
        if ((pos & (TT_SCALE - 1)) == TT_SCALE - 1) {
            const double sc = live ? scale[(size_t) (pos / TT_SCALE) * 64] : 1.0;
            bg *= sc;
#pragma unroll
            for (int j = 0; j < TT_OFF; j++) m.fg[j] *= sc;
        }
        const double toBg = f2b * bg;
        const double toFg = offsets(cur * IB_ALPH, toBg);
        bg = fma(b2b, bg, toFg);
    };
    int pos = maxLen - 1;
    if (maxLen > TT_RAMP) {
        int P0 = (maxLen - 1) & ~3;
#pragma unroll
        for (int j = 0; j < TT_OFF + 3; j++) m.W[j] = at(P0 + 2 - j);
        for (; P0 >= TT_RAMP; P0 -= 4) {
            const uint32_t r3 = at(P0 + 3);
            if (P0 + 3 < maxLen) backStep(P0 + 3, r3, [&](uint32_t row, double toBg) { return bwdFull<0>(m, row, toBg); });
            if (P0 + 2 < maxLen) backStep(P0 + 2, m.W[0], [&](uint32_t row, double toBg) { return bwdFull<1>(m, row, toBg); });
            if (P0 + 1 < maxLen) backStep(P0 + 1, m.W[1], [&](uint32_t row, double toBg) { return bwdFull<2>(m, row, toBg); });
            backStep(P0, m.W[2], [&](uint32_t row, double toBg) { return bwdFull<3>(m, row, toBg); });
#pragma unroll
            for (int j = 0; j < TT_OFF - 1; j++) m.W[j] = m.W[j + 4];   // W'[j] = residue P0 - 2 - j
            m.W[TT_OFF - 1] = at(P0 - 51);
            m.W[TT_OFF] = at(P0 - 52);
            m.W[TT_OFF + 1] = at(P0 - 53);
            m.W[TT_OFF + 2] = at(P0 - 54);
        }
        pos = TT_RAMP - 1;   // W[i] = residue TT_RAMP - 2 - i = pos - 1 - i
    } else {
#pragma unroll
        for (int j = 0; j < TT_OFF + 3; j++) m.W[j] = at(pos - 1 - j);
    }
    for (; pos >= 0; pos--) {
        const uint32_t cur = at(pos);
        const int maxOffset = min(pos, TT_OFF);
        backStep(pos, cur, [&](uint32_t row, double toBg) { return bwdPart(m, row, toBg, maxOffset); });
#pragma unroll
        for (int j = 0; j < TT_OFF + 2; j++) m.W[j] = m.W[j + 1];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) nX += __shfl_xor(nX, o, 64);
    if (lane == 0 && nX) atomicAdd(nMasked, nX);
}

// ---------------------------------------------------------------------------------------------
// k-mer records
// ---------------------------------------------------------------------------------------------
constexpr int IB_SEQ_PER_WAVE = 16;
constexpr uint32_t IB_COARSE_BINS = 4096;

// k-mer index at position i of a masked sequence, 0xFFFFFFFF if it holds an X, runs off the end or scores below the threshold
template <int K>
__device__ __forceinline__ uint32_t kmerAt(const uint8_t *__restrict__ s, int L, int i, int span, int thr) {
    if (i + span > L) return 0xFFFFFFFFu;
    uint32_t idx = 0;
    int score = 0;
    bool x = false;
#pragma unroll
    for (int p = 0; p < K; p++) {
        const uint32_t a = s[i + c_ibSeed[p]];
        x |= a >= (uint32_t) IB_X;
        score += c_ibSelf[a < (uint32_t) IB_ALPH ? a : IB_X];
        idx += a * c_ibPow[p];
    }
    if (x || (thr > 0 && score < thr)) return 0xFFFFFFFFu;
    return idx;
}

// MODE 0: histogram of the valid k-mers over IB_COARSE_BINS equal ranges of the k-mer space (the host cuts the ranges of the
//         passes from it);  MODE 1: records of [lo, hi) per wavefront;  MODE 2: the records themselves at waveBase[w] + ...
template <int K, int MODE>
__global__ void __launch_bounds__(256)
ib_records_kernel(const uint8_t *__restrict__ masked, const uint64_t *__restrict__ seqOff, uint32_t nSeq, int span, int thr,
                  uint32_t binWidth, unsigned long long *__restrict__ coarse, uint32_t lo, uint32_t hi,
                  uint32_t *__restrict__ waveCount, const uint64_t *__restrict__ waveBase, uint32_t *__restrict__ keys,
                  uint64_t *__restrict__ vals) {
    __shared__ uint32_t hist[MODE == 0 ? IB_COARSE_BINS : 1];
    if (MODE == 0) {
        for (uint32_t i = threadIdx.x; i < IB_COARSE_BINS; i += 256) hist[i] = 0;
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t s0 = (uint64_t) wave * IB_SEQ_PER_WAVE;
    uint64_t written = MODE == 2 && s0 < nSeq ? waveBase[wave] : 0;
    uint32_t count = 0;
    for (uint64_t q = s0; q < s0 + IB_SEQ_PER_WAVE && q < nSeq; q++) {
        const uint64_t b = seqOff[q];
        const int L = (int) (seqOff[q + 1] - b);
        const uint8_t *s = masked + b;
        for (int i0 = 0; i0 + span <= L; i0 += 64) {
            const uint32_t km = kmerAt<K>(s, L, i0 + (int) lane, span, thr);
            if (MODE == 0) {
                if (km != 0xFFFFFFFFu) atomicAdd(&hist[km / binWidth], 1u);
            } else {
                const bool in = km != 0xFFFFFFFFu && km >= lo && km < hi;
                const unsigned long long b64 = __ballot(in);
                if (MODE == 2 && in) {
                    const uint64_t at = written + __popcll(b64 & ((1ull << lane) - 1));
                    keys[at] = km - lo;
                    vals[at] = (q << 16) | (uint64_t) (i0 + (int) lane);
                }
                written += __popcll(b64);
                count += __popcll(b64);
            }
        }
    }
    if (MODE == 0) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < IB_COARSE_BINS; i += 256)
            if (hist[i]) atomicAdd(&coarse[i], (unsigned long long) hist[i]);
    }
    if (MODE == 1 && lane == 0 && s0 < nSeq) waveCount[wave] = count;
}

// ---- records of a *profile* target (sd_target_build_profile): every window of a profile contributes its whole similar-k-mer list
// (IndexTable::addSimilarKmerCount / addSimilarSequence, IndexTable.h:97-130,302-345), which is KmerGenerator::generateKmerList over the
// window's per-position rows of 20 (score, amino acid) pairs (setDivideStrategy(profile_matrix), KmerGenerator.cpp:30-39,143-165).  A
// wavefront per window runs the k - 1 array products stage by stage exactly like profile_kmers_kernel (sd_prefilter.hip) does for a
// profile *query*: the partial list lives in a per-wavefront scratch buffer, lanes take parents, each appends its run of children after
// an exclusive scan of the run lengths; cutoffs are the reference's `short` expressions.  What differs is the last product: its
// k-mers become index records (k-mer - lo, target << 16 | position) of the pass's k-mer range [lo, hi), compacted across the lanes.
// A window's k-mers are distinct (one amino acid per seed position each), and the windows write at bases scanned in (target, position)
// order, so the records of a pass leave in ascending (target, position) order: the stable sort by k-mer keeps it, and the first
// record of a (k-mer, target) run is the one at the smallest position -- IndexEntryLocalTmp::comapreByIdAndPos (IndexTable.h:52).
//   MODE 0: the list length of every window (winCount), its scratch tier (big), the histogram over IB_COARSE_BINS k-mer ranges
//   MODE 1: the records of [lo, hi) per window (winCount);  MODE 2: the records themselves at recBase[window] + ...
// Two tiers of scratch as in profile_kmers_kernel: PROFILE_PARTIAL_CAP entries per list on the wide grid, PROFILE_PARTIAL_CAP_BIG for
// the windows MODE 0 flags.  errWin[0]: the first window whose list passes 2^23 k-mers (KmerGenerator.h:45); errWin[1]: the number of
// windows flagged for the big tier.
constexpr uint32_t IP_GRID = 1024, IP_GRID_BIG = 16;
constexpr uint32_t IP_LIST_MAX = 1u << 23;
// spaced seeds of the windowed builders, row k - 5 (M/src/commons/Sequence.h:21,23; SdKmerShape, sd_common.h)
__constant__ uint8_t c_ipSeed[2][8] = {{0, 1, 4, 9, 11, 0, 0, 0},    // k = 5: 110010000101
                                       {0, 1, 3, 5, 8, 9, 0, 0}};    // k = 6: 1101010011

template <int K, int MODE>
__global__ void __launch_bounds__(64)
ib_profile_records_kernel(uint64_t nWin, const uint64_t *__restrict__ winBase /* first window of every target, nSeq + 1 */, uint32_t nSeq,
                          const uint8_t *__restrict__ letters, const uint64_t *__restrict__ posOff, const int16_t *__restrict__ sortedScore,
                          const uint8_t *__restrict__ sortedIndex, int kmerThr, uint2 *__restrict__ scratch, uint32_t cap,
                          uint8_t *__restrict__ big, int bigTier, uint32_t binWidth, unsigned long long *__restrict__ coarse,
                          unsigned long long *__restrict__ errWin, uint32_t lo, uint32_t hi, uint32_t *__restrict__ winCount,
                          const uint64_t *__restrict__ recBase, uint32_t *__restrict__ keys, uint64_t *__restrict__ vals) {
    static_assert(K == 5 || K == 6, "c_ipSeed");
    __shared__ int16_t rowS[K][20];
    __shared__ uint8_t rowI[K][20];
    __shared__ uint32_t hist[MODE == 0 ? IB_COARSE_BINS : 1];
    const int lane = threadIdx.x;
    if (MODE == 0)
        for (uint32_t i = lane; i < IB_COARSE_BINS; i += 64) hist[i] = 0;
    uint32_t histHeld = 0;   // records in hist (MODE 0): flushed before a 32-bit bin could wrap
    auto flush = [&]() {
        __syncthreads();
        for (uint32_t i = lane; i < IB_COARSE_BINS; i += 64) {
            if (hist[i]) atomicAdd(&coarse[i], (unsigned long long) hist[i]);
            hist[i] = 0;
        }
        __syncthreads();
        histHeld = 0;
    };
    uint2 *listA = scratch + (size_t) blockIdx.x * 2 * cap;
    uint2 *listB = listA + cap;
    const int thr = kmerThr > 0 ? kmerThr : 0;   // no composition bias: the generator's threshold is kmerThr as it is (IndexBuilder.cpp:96)
    for (uint64_t p = blockIdx.x; p < nWin; p += gridDim.x) {
        if ((big[p] != 0) != (bigTier != 0)) continue;   // block-uniform
        uint32_t tl = 0, th = nSeq;   // last target with winBase[target] <= p
        while (th - tl > 1) {
            const uint32_t mid = (tl + th) >> 1;
            if (winBase[mid] <= p) tl = mid;
            else th = mid;
        }
        const uint32_t q = tl;
        const int i = (int) (p - winBase[tl]);
        const uint64_t r0 = posOff[q] + (uint64_t) i;
        bool hasX = false;
        for (int x = 0; x < K; x++) hasX |= letters[r0 + c_ipSeed[K - 5][x]] >= 20;   // kmerContainsX on the query letters (Sequence.h:397-403)
        __syncthreads();   // the previous window's rows are no longer read
        for (int x = lane; x < K * 20; x += 64) {
            const int sIdx = x / 20, e = x % 20;
            rowS[sIdx][e] = sortedScore[(r0 + c_ipSeed[K - 5][sIdx]) * 20 + e];
            rowI[sIdx][e] = sortedIndex[(r0 + c_ipSeed[K - 5][sIdx]) * 20 + e];
        }
        __syncthreads();
        uint32_t totalOut = 0;   // MODE 0: the list length; MODE 1 / 2: its records in [lo, hi)
        if (!hasX) {
            int rest[K];
            rest[K - 1] = 0;
            for (int x = K - 1; x >= 1; x--) rest[x - 1] = (int) (short) ((int) rowS[x][0] + rest[x]);
            const int cutoff1 = (int) (short) (thr - rest[0]);
            uint32_t nA = 0;
            while (nA < 20 && (int) rowS[0][nA] >= cutoff1) nA++;
            if ((uint32_t) lane < nA) listA[lane] = make_uint2((uint32_t) (int) rowS[0][lane], (uint32_t) rowI[0][lane]);
            uint32_t mult = 1;
            const uint64_t base = MODE == 2 ? recBase[p] : 0;
            const uint64_t val = ((uint64_t) q << 16) | (uint64_t) i;
            bool overflow = false;
            for (int st = 0; st + 1 < K && !overflow; st++) {
                mult *= 20u;
                const bool last = st + 2 == K;
                const int16_t *rs = rowS[st + 1];
                const uint8_t *ri = rowI[st + 1];
                const int restNext = rest[st + 1];
                uint32_t nB = 0;
                __threadfence_block();
                for (uint32_t c0 = 0; c0 < nA; c0 += 64) {
                    const uint32_t e = c0 + lane;
                    int si = 0;
                    uint32_t ki = 0, c = 0;
                    if (e < nA) {
                        // agent-scope loads: the entry was written by another lane of this wavefront a stage ago and the
                        // vector L1 may still hold the line from the buffer's previous use
                        const uint32_t px = __hip_atomic_load(&listA[e].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ki = __hip_atomic_load(&listA[e].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        si = (int) (short) px;
                        const int cutoff2 = (int) (short) (thr - si - restNext);
                        while (c < 20 && (int) rs[c] >= cutoff2) c++;
                    }
                    if (!last) {
                        uint32_t incl = c;
#pragma unroll
                        for (int off = 1; off < 64; off <<= 1) {
                            const uint32_t o = __shfl_up(incl, off, 64);
                            if (lane >= off) incl += o;
                        }
                        const uint32_t excl = incl - c;
                        const uint32_t chunkTotal = __shfl(incl, 63, 64);
                        if (nB + chunkTotal > cap) {
                            overflow = true;
                            break;
                        }
                        for (uint32_t j = 0; j < c; j++)
                            listB[nB + excl + j] = make_uint2((uint32_t) (int) (short) (si + (int) rs[j]), ki + (uint32_t) ri[j] * mult);
                        nB += chunkTotal;
                    } else if (MODE == 0) {
                        for (uint32_t j = 0; j < c; j++) atomicAdd(&hist[(ki + (uint32_t) ri[j] * mult) / binWidth], 1u);
                        uint32_t sum = c;
#pragma unroll
                        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
                        nB += sum;
                    } else {
                        uint32_t m = 0;   // this lane's children in [lo, hi)
                        for (uint32_t j = 0; j < c; j++) {
                            const uint32_t kmer = ki + (uint32_t) ri[j] * mult;
                            m += (kmer >= lo && kmer < hi) ? 1u : 0u;
                        }
                        uint32_t incl = m;
#pragma unroll
                        for (int off = 1; off < 64; off <<= 1) {
                            const uint32_t o = __shfl_up(incl, off, 64);
                            if (lane >= off) incl += o;
                        }
                        if (MODE == 2 && m) {
                            uint64_t w = base + nB + (incl - m);
                            for (uint32_t j = 0; j < c; j++) {
                                const uint32_t kmer = ki + (uint32_t) ri[j] * mult;
                                if (kmer >= lo && kmer < hi) {
                                    keys[w] = kmer - lo;
                                    vals[w] = val;
                                    w++;
                                }
                            }
                        }
                        nB += __shfl(incl, 63, 64);
                    }
                }
                if (last) {
                    totalOut = nB;
                } else {
                    uint2 *t = listA;
                    listA = listB;
                    listB = t;
                    nA = nB;
                }
            }
            if (MODE == 0) {
                // (a partial list is never longer than the final one: an overflow of the big tier is a list beyond IP_LIST_MAX as well)
                if (overflow && !bigTier) {
                    if (lane == 0) {   // redone by the narrow grid; nothing of this window is in the histogram yet
                        big[p] = 1;
                        atomicAdd(&errWin[1], 1ull);
                    }
                } else if (overflow || totalOut > IP_LIST_MAX) {
                    if (lane == 0) atomicMin(errWin, (unsigned long long) p);
                }
                if (overflow) totalOut = 0;
            }
        }
        if (MODE != 2 && lane == 0) winCount[p] = totalOut;   // (0 for a window that moves to the big tier: its launch follows and writes it)
        if (MODE == 0) {
            histHeld += totalOut;
            if (histHeld >= (1u << 31) - IP_LIST_MAX) flush();
        }
    }
    if (MODE == 0) flush();
}

// ---- records of a *sequence* target under --target-search-mode 1 (sd_target_build_similar): the sequence branch of the same reference
// code (setDivideStrategy(&three, &two), IndexBuilder.cpp:100): a window without X contributes KmerGenerator::generateKmerList of its own
// k-mer, which at k = 6 is ONE array product of two sorted 3-mer rows -- parents a of row0 with s0[a] >= short(thr - best1), children b
// of row1 with s1[b] >= short(thr - s0[a]), k-mer i0[a] + 8000 i1[b] -- exactly what count_kmers_kernel / emit_kmers_kernel enumerate for
// a query, without a bias term.  A wavefront per window: 64 parents at a time take their run lengths from ext3Cum (one read each), the
// runs are scanned and then flattened over the lanes (slot t belongs to the lane o with excl[o] <= t < incl[o], found in LDS), so all
// 64 lanes produce k-mers however unequal the runs are -- they span 1 to 8 000 between the best and the last parent -- and the records
// of the pass's range [lo, hi) are compacted with a ballot into one contiguous, ascending store.  No partial list exists, so there is
// no scratch and no tier.  A window's k-mers are distinct (a pair (a, b) gives one (i0, i1)) and the windows write at bases scanned in
// (target, position) order: the order argument of the profile generator above holds word for word.
//   MODE 0: the list length of every window (winCount) and the histogram over IB_COARSE_BINS k-mer ranges; errWin: the first window
//           whose list reaches IP_LIST_MAX (calculateArrayProduct stops there, KmerGenerator.cpp:204-213)
//   MODE 1: the records of [lo, hi) per window (winCount);  MODE 2: the records themselves at recBase[window] + ...
constexpr uint32_t IS_GRID = 4096;
template <int MODE>
__global__ void __launch_bounds__(64)
ib_similar_records_kernel(uint64_t nWin, const uint64_t *__restrict__ winBase /* first window of every target, nSeq + 1 */, uint32_t nSeq,
                          const uint8_t *__restrict__ res, const uint64_t *__restrict__ seqOff, const int16_t *__restrict__ ext3Score,
                          const uint16_t *__restrict__ ext3Index, const uint16_t *__restrict__ ext3Cum /* nullable */, int ext3Lo, int kmerThr,
                          uint32_t binWidth, unsigned long long *__restrict__ coarse, unsigned long long *__restrict__ errWin, uint32_t lo,
                          uint32_t hi, uint32_t *__restrict__ winCount, const uint64_t *__restrict__ recBase, uint32_t *__restrict__ keys,
                          uint64_t *__restrict__ vals) {
    __shared__ uint32_t hist[MODE == 0 ? IB_COARSE_BINS : 1];
    __shared__ uint32_t sIncl[64], sK0[64];
    const int lane = threadIdx.x;
    if (MODE == 0)
        for (uint32_t i = lane; i < IB_COARSE_BINS; i += 64) hist[i] = 0;
    uint32_t histHeld = 0;   // records in hist (MODE 0): flushed before a 32-bit bin could wrap
    auto flush = [&]() {
        __syncthreads();
        for (uint32_t i = lane; i < IB_COARSE_BINS; i += 64) {
            if (hist[i]) atomicAdd(&coarse[i], (unsigned long long) hist[i]);
            hist[i] = 0;
        }
        __syncthreads();
        histHeld = 0;
    };
    if (MODE == 0) __syncthreads();
    for (uint64_t p = blockIdx.x; p < nWin; p += gridDim.x) {
        uint32_t tl = 0, th = nSeq;   // last target with winBase[target] <= p
        while (th - tl > 1) {
            const uint32_t mid = (tl + th) >> 1;
            if (winBase[mid] <= p) tl = mid;
            else th = mid;
        }
        const uint32_t q = tl;
        const int i = (int) (p - winBase[tl]);
        const uint8_t *s = res + seqOff[q] + (uint64_t) i;
        uint32_t w[6];
        bool hasX = false;
#pragma unroll
        for (int x = 0; x < 6; x++) {
            w[x] = s[c_ipSeed[6 - 5][x]];
            hasX |= w[x] >= 20u;   // kmerContainsX (Sequence.h:397-403)
        }
        uint32_t totalOut = 0;   // MODE 0: the list length; MODE 1 / 2: its records in [lo, hi)
        if (!hasX) {
            const uint32_t idx0 = w[0] + 20u * w[1] + 400u * w[2], idx1 = w[3] + 20u * w[4] + 400u * w[5];
            const int16_t *row0 = ext3Score + (size_t) idx0 * 8000, *row1 = ext3Score + (size_t) idx1 * 8000;
            const uint16_t *ix0 = ext3Index + (size_t) idx0 * 8000, *ix1 = ext3Index + (size_t) idx1 * 8000;
            const uint16_t *cum0 = ext3Cum ? ext3Cum + (size_t) idx0 * EXT3_CUM_SPAN : nullptr;
            const uint16_t *cum1 = ext3Cum ? ext3Cum + (size_t) idx1 * EXT3_CUM_SPAN : nullptr;
            const int thr = (int) (short) kmerThr;   // KmerGenerator::threshold is a short; no composition bias (IndexBuilder.cpp:96)
            const int cutoff1 = (int) (short) (thr - (int) row1[0]);
            const int n0 = cum0 ? countGETab(cum0, ext3Lo, cutoff1) : countGE(row0, 8000, cutoff1);
            bool tooLong = false;
            if (MODE == 0) {   // the length first: a list the reference would cut is refused before anything of it is counted
                uint32_t total = 0;
                for (int a = lane; a < n0; a += 64) {
                    const int cutoff2 = (int) (short) (thr - (int) row0[a]);
                    total += (uint32_t) (cum1 ? countGETab(cum1, ext3Lo, cutoff2) : countGE(row1, 8000, cutoff2));
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off, 64);
                totalOut = total;
                tooLong = total >= IP_LIST_MAX;
                if (tooLong && lane == 0) atomicMin(errWin, (unsigned long long) p);
            }
            const uint64_t base = MODE == 2 ? recBase[p] : 0;
            const uint64_t val = ((uint64_t) q << 16) | (uint64_t) i;
            uint32_t written = 0;
            for (int a0 = 0; a0 < n0 && !tooLong; a0 += 64) {
                const int a = a0 + lane;
                uint32_t c = 0;
                if (a < n0) {
                    const int cutoff2 = (int) (short) (thr - (int) row0[a]);
                    c = (uint32_t) (cum1 ? countGETab(cum1, ext3Lo, cutoff2) : countGE(row1, 8000, cutoff2));
                }
                uint32_t incl = c;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t o = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += o;
                }
                const uint32_t chunkTotal = __shfl(incl, 63, 64);
                __builtin_amdgcn_wave_barrier();   // the previous chunk's readers are done
                sIncl[lane] = incl;
                sK0[lane] = a < n0 ? (uint32_t) ix0[a] : 0u;
                __builtin_amdgcn_wave_barrier();
                for (uint32_t t0 = 0; t0 < chunkTotal; t0 += 64) {
                    const uint32_t t = t0 + (uint32_t) lane;
                    uint32_t km = 0;
                    bool in = false;
                    if (t < chunkTotal) {
                        int l = 0, h = 63;   // smallest o with incl[o] > t
#pragma unroll
                        for (int st = 0; st < 6; st++) {
                            const int mid = (l + h) >> 1;
                            if (sIncl[mid] > t) h = mid;
                            else l = mid + 1;
                        }
                        const uint32_t before = l ? sIncl[l - 1] : 0u;
                        km = sK0[l] + 8000u * (uint32_t) ix1[t - before];
                        in = MODE == 0 || (km >= lo && km < hi);
                    }
                    if (MODE == 0) {
                        if (in) atomicAdd(&hist[km / binWidth], 1u);
                    } else {
                        const unsigned long long b64 = __ballot(in);
                        if (MODE == 2 && in) {
                            const uint64_t at = base + written + __popcll(b64 & ((1ull << lane) - 1));
                            keys[at] = km - lo;
                            vals[at] = val;
                        }
                        written += (uint32_t) __popcll(b64);
                    }
                }
            }
            if (MODE != 0) totalOut = written;
            if (tooLong) totalOut = 0;
        }
        if (MODE != 2 && lane == 0) winCount[p] = totalOut;
        if (MODE == 0) {
            histHeld += totalOut;
            if (histHeld >= (1u << 31) - IP_LIST_MAX) flush();
        }
    }
    if (MODE == 0) flush();
}

// ---- survivors of the sorted records: the first of every (k-mer, target) run
constexpr int IK_TILE = 2048, IK_NT = 256;
__device__ __forceinline__ bool ikKept(const uint32_t *__restrict__ keys, const uint64_t *__restrict__ vals, uint64_t i) {
    return i == 0 || keys[i] != keys[i - 1] || (vals[i] >> 16) != (vals[i - 1] >> 16);
}
__global__ void __launch_bounds__(IK_NT) ib_keep_count(const uint32_t *__restrict__ keys, const uint64_t *__restrict__ vals, uint64_t n,
                                                       uint32_t *__restrict__ tileCount) {
    __shared__ uint32_t part[IK_NT / 64];
    const uint64_t base = (uint64_t) blockIdx.x * IK_TILE;
    uint32_t c = 0;
    for (int x = threadIdx.x; x < IK_TILE; x += IK_NT)
        if (base + x < n) c += ikKept(keys, vals, base + x) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tileCount[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
// appends the survivors to the entry array (in order) and counts them per k-mer
__global__ void __launch_bounds__(IK_NT) ib_place(const uint32_t *__restrict__ keys, const uint64_t *__restrict__ vals, uint64_t n,
                                                  const uint64_t *__restrict__ tileBase, uint64_t entryBase, uint32_t lo,
                                                  uint2 *__restrict__ entries, uint32_t *__restrict__ counts) {
    __shared__ uint32_t wsum[IK_NT / 64];
    const uint64_t base = (uint64_t) blockIdx.x * IK_TILE;
    constexpr int PER = IK_TILE / IK_NT;
    uint32_t mine = 0;
    bool kept[PER];
#pragma unroll
    for (int x = 0; x < PER; x++) {
        const uint64_t i = base + (uint64_t) threadIdx.x * PER + x;
        kept[x] = i < n && ikKept(keys, vals, i);
        mine += kept[x] ? 1u : 0u;
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if ((int) (threadIdx.x & 63) >= o) incl += up;
    }
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint64_t at = entryBase + tileBase[blockIdx.x] + incl - mine;
    for (int w = 0; w < (int) (threadIdx.x >> 6); w++) at += wsum[w];
#pragma unroll
    for (int x = 0; x < PER; x++) {
        if (!kept[x]) continue;
        const uint64_t i = base + (uint64_t) threadIdx.x * PER + x;
        const uint64_t v = vals[i];
        entries[at++] = make_uint2((uint32_t) (v >> 16), (uint32_t) (v & 0xFFFFu));
        atomicAdd(&counts[lo + keys[i]], 1u);
    }
}

// list starts as the prefilter kernels read them: 32-bit, relative to base[i >> 16] in the wide form
__global__ void __launch_bounds__(256) ib_offsets(const uint64_t *__restrict__ start, uint64_t n, int wide, uint32_t *__restrict__ offsets,
                                                  uint64_t *__restrict__ blockBase) {
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = wide ? start[i & ~0xFFFFull] : 0;
    if (wide && (i & 0xFFFFu) == 0) blockBase[i >> 16] = b;
    offsets[i] = (uint32_t) (start[i] - b);
}

double firstRepeatOffsetProb(double probMult, int maxRepeatOffset) {
    if (probMult < 1 || probMult > 1) return (1 - probMult) / (1 - std::pow(probMult, maxRepeatOffset));
    return 1.0 / maxRepeatOffset;
}

// The environment knobs of a build, read once per call (not once per process: the tests flip them between builds).
//   knob                   what it is for                                           default                   clamp
//   SD_INDEX_PASS          records per sort pass (tests: many small passes)         2^30                      >= 1; ibPassCap raises it to
//                                                                                                             the fullest histogram range
//   SD_INDEX_WIDE          set to anything: list starts in the wide form (tests)    wide from 2^32 entries    --
//   SD_INDEX_MASK_BUDGET   bytes of tantan's scratch between its two passes (tests) an eighth of the device   <= half of the free memory,
//                                                                                                             >= one row per wavefront
//   SD_INDEX_PROFILE_GRID  wavefronts of the profile generator's wide tier, 1 MiB   IP_GRID (1 024)           64 .. 16 384
//                          of list scratch each (tools/bench_target_profile.py)
struct IndexKnobs {
    uint64_t passCap = 1ull << 30;
    bool wide = false;
    bool haveMaskBudget = false;
    uint64_t maskBudget = 0;
    uint64_t profileGrid = IP_GRID;
    IndexKnobs() {
        if (const char *s = getenv("SD_INDEX_PASS")) passCap = std::max<uint64_t>(1, strtoull(s, nullptr, 10));
        wide = getenv("SD_INDEX_WIDE") != nullptr;
        if (const char *s = getenv("SD_INDEX_MASK_BUDGET")) {
            haveMaskBudget = true;
            maskBudget = strtoull(s, nullptr, 10);
        }
        if (const char *s = getenv("SD_INDEX_PROFILE_GRID")) profileGrid = std::min<uint64_t>(std::max<uint64_t>(64, strtoull(s, nullptr, 10)), 16384);
    }
};

// sd_target_build_peak: the free device memory is read where a phase holds the most
struct PeakNote {
    sd_target *t = nullptr;
    size_t freeAtStart = 0;
    void begin(sd_target *target) {
        t = target;
        size_t totalDev = 0;
        (void) hipMemGetInfo(&freeAtStart, &totalDev);
    }
    void operator()() const {
        size_t f = 0, tot = 0;
        if (hipMemGetInfo(&f, &tot) == hipSuccess && f < freeAtStart) t->buildPeak = std::max<uint64_t>(t->buildPeak, freeAtStart - f);
    }
};

// The masking phase of sd_target_build: the residues go to the device and, tantan-masked (ib_mask_kernel) or as they are, into
// t->dMasked.  The sequences are dealt to the wavefronts by length; the forward posteriors and rescaling factors between the kernel's
// two passes take 64 lanes x (4 + 8 / 16) bytes per row of a wavefront, four to five times the residue bytes of the whole DB -- so the
// wavefronts run in slices against a scratch budget (IndexKnobs; never less than the longest wavefront needs).
int ibMaskPhase(sd_ctx *ctx, sd_target *t, const IndexKnobs &knobs, const uint8_t *residues, const uint64_t *seqOffsets, uint32_t nSeq, int mask,
                double maskProb, const double *maskRatios, const PeakNote &notePeak, uint64_t &nMaskedResidues) {
    const uint64_t total = seqOffsets[nSeq];
    nMaskedResidues = 0;
    DevBuf<uint8_t> dRes;
    SD_HIP(ctx, dRes.alloc(total + 64));
    SD_HIP(ctx, hipMemcpy(dRes.p, residues, total, hipMemcpyDefault));
    if (!mask || nSeq == 0) {
        SD_HIP(ctx, hipMemcpyAsync(t->dMasked, dRes.p, total, hipMemcpyDeviceToDevice, ctx->stream));
        SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return SD_OK;
    }
    TantanPar par;
    const double repeatProb = 0.005, repeatEndProb = 0.05, decay = 0.9;
    par.b2b = 1 - repeatProb;
    par.f2b = repeatEndProb;
    par.f2f0 = 1 - repeatEndProb;
    double p = repeatProb * firstRepeatOffsetProb(decay, TT_OFF);
    for (int i = 0; i < TT_OFF; i++) {
        par.b2f[i] = p;
        p *= decay;
    }
    SD_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_tt), &par, sizeof(par)));
    // sequences dealt to the wavefronts by length (counting sort, stable)
    auto len = [&](uint32_t i) { return seqOffsets[i + 1] - seqOffsets[i]; };
    uint64_t longest = 0;
    for (uint32_t i = 0; i < nSeq; i++) longest = std::max(longest, len(i));
    std::vector<uint32_t> order(nSeq);
    {
        std::vector<uint32_t> cnt((size_t) longest + 2, 0);
        for (uint32_t i = 0; i < nSeq; i++) cnt[(size_t) len(i) + 1]++;
        for (size_t l = 1; l < cnt.size(); l++) cnt[l] += cnt[l - 1];
        for (uint32_t i = 0; i < nSeq; i++) order[cnt[(size_t) len(i)]++] = i;
    }
    // rows of the scratch per wavefront: its longest (= last) sequence rounded up to the rescaling period
    const uint32_t nWaves = (nSeq + 63) / 64;
    std::vector<uint64_t> waveRow((size_t) nWaves + 1, 0);
    for (uint32_t w = 0; w < nWaves; w++) {
        const uint64_t last = len(order[std::min<uint64_t>((uint64_t) w * 64 + 63, nSeq - 1)]);
        waveRow[w + 1] = waveRow[w] + ((last + TT_SCALE - 1) / TT_SCALE) * TT_SCALE;
    }
    // slices of wavefronts whose rows fit the budget (a wavefront beyond it runs alone)
    size_t freeB = 0, totalB = 0;
    (void) hipMemGetInfo(&freeB, &totalB);
    const uint64_t budget = std::min<uint64_t>(knobs.haveMaskBudget ? knobs.maskBudget : (uint64_t) totalB / 8, (uint64_t) freeB / 2);
    const uint64_t budgetRows = std::max<uint64_t>(budget / (64 * (sizeof(float) + sizeof(double) / TT_SCALE + 1)), 1);
    std::vector<uint32_t> sliceEnd;
    uint64_t sliceRows = 0;   // the largest slice
    for (uint32_t w0 = 0; w0 < nWaves;) {
        uint32_t w1 = w0 + 1;
        while (w1 < nWaves && waveRow[w1 + 1] - waveRow[w0] <= budgetRows) w1++;
        sliceRows = std::max(sliceRows, waveRow[w1] - waveRow[w0]);
        sliceEnd.push_back(w1);
        w0 = w1;
    }
    DevBuf<uint32_t> dOrder;
    DevBuf<uint64_t> dWaveRow;
    DevBuf<float> dProb;
    DevBuf<double> dScale, dLr;
    DevBuf<unsigned long long> dN;
    SD_HIP(ctx, dOrder.alloc(nSeq));
    SD_HIP(ctx, dWaveRow.alloc(nWaves + 1));
    SD_HIP(ctx, dProb.alloc(std::max<uint64_t>(sliceRows * 64, 1)));   // (no row at all when every sequence is empty)
    SD_HIP(ctx, dScale.alloc(sliceRows / TT_SCALE * 64 + 64));
    SD_HIP(ctx, dLr.alloc(IB_ALPH * IB_ALPH));
    SD_HIP(ctx, dN.alloc(1));
    notePeak();
    SD_HIP(ctx, hipMemcpy(dOrder.p, order.data(), (size_t) nSeq * sizeof(uint32_t), hipMemcpyHostToDevice));
    SD_HIP(ctx, hipMemcpy(dWaveRow.p, waveRow.data(), ((size_t) nWaves + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    SD_HIP(ctx, hipMemcpy(dLr.p, maskRatios, IB_ALPH * IB_ALPH * sizeof(double), hipMemcpyHostToDevice));
    SD_HIP(ctx, hipMemsetAsync(dN.p, 0, sizeof(unsigned long long), ctx->stream));
    uint32_t w0 = 0;
    for (uint32_t w1 : sliceEnd) {   // one after the other on the stream: they share the scratch
        ProfScope ps(ctx, "index_mask");
        hipLaunchKernelGGL(ib_mask_kernel, dim3(w1 - w0), dim3(64), 0, ctx->stream, (const uint8_t *) dRes.p, (const uint64_t *) t->dSeqOff,
                           (const uint32_t *) dOrder.p, nSeq, (const double *) dLr.p, (const uint64_t *) dWaveRow.p, dProb.p, dScale.p, maskProb,
                           t->dMasked, dN.p, w0);
        w0 = w1;
    }
    SD_HIP(ctx, hipGetLastError());
    SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long h = 0;
    SD_HIP(ctx, hipMemcpy(&h, dN.p, sizeof(h), hipMemcpyDeviceToHost));
    nMaskedResidues = h;
    return SD_OK;
}

// records per pass: bounded by the sort's 32-bit item count and by SD_INDEX_PASS
int ibPassCap(sd_ctx *ctx, const IndexKnobs &knobs, const std::vector<unsigned long long> &coarse, uint64_t &cap, uint64_t &nRecords) {
    uint64_t biggestBin = 0;
    nRecords = 0;
    for (unsigned long long c : coarse) {
        nRecords += c;
        biggestBin = std::max<uint64_t>(biggestBin, c);
    }
    cap = std::max(knobs.passCap, biggestBin);
    if (cap >= (1ull << 31))
        return sdFail(ctx, SD_EUNSUPPORTED, "one of the %u k-mer ranges holds %llu index records (limit 2^31 per sort)", IB_COARSE_BINS,
                      (unsigned long long) biggestBin);
    return SD_OK;
}

// exclusive 64-bit scan of n 32-bit counts and of one element more, which the caller keeps at zero: out[n] is the total
hipError_t ibScan(sd_ctx *ctx, const uint32_t *in, uint64_t n, uint64_t *out, uint64_t *tmp) {
    return sdScanLaunch<uint32_t, ScanSum64, false, uint64_t>(ctx->stream, in, out, n + 1, tmp);
}

// The passes the builders share: the k-mer space is cut into ranges of at most `cap` records along the coarse histogram; per range
// countFn(lo, hi, slotCount) counts the records of [lo, hi) per slot (a slot: what one wavefront of the generator writes in order -- 16
// sequences in sd_target_build, one window in the other two), emitFn(lo, hi, slotBase, keys, vals) writes them at the scanned bases, in
// ascending (target, position) order over the whole pass; they are sorted by k-mer (stable), the first record of every (k-mer, target)
// run is appended to t->dEntries and counted in t->dOffsets.  The scratch is bounded by cap, not by nRecords.
template <typename CountFn, typename EmitFn>
int ibPasses(sd_ctx *ctx, sd_target *t, const char *who, const std::vector<unsigned long long> &coarse, uint32_t binWidth, uint64_t nRecords,
             uint64_t cap, uint32_t nSlots, CountFn countFn, EmitFn emitFn, const PeakNote &notePeak, uint64_t &nEntries, uint64_t &nPasses) {
    const uint64_t bufN = std::min<uint64_t>(cap, nRecords);   // (>= 1: the caller has records)
    const uint64_t maxTiles = (bufN + IK_TILE - 1) / IK_TILE;
    DevBuf<uint32_t> k0, k1, dSlotCount, dTileCount;
    DevBuf<uint64_t> v0, v1, dSlotBase, dTileBase;
    DevBuf<uint8_t> dSortTmp, dScanTmp;
    SD_HIP(ctx, k0.alloc(bufN));
    SD_HIP(ctx, k1.alloc(bufN));
    SD_HIP(ctx, v0.alloc(bufN));
    SD_HIP(ctx, v1.alloc(bufN));
    SD_HIP(ctx, dSlotCount.alloc((size_t) nSlots + 1));   // one more than the generators write: it stays zero, its scanned value is the total
    SD_HIP(ctx, dSlotBase.alloc((size_t) nSlots + 1));
    SD_HIP(ctx, dTileCount.alloc(maxTiles + 1));
    SD_HIP(ctx, dTileBase.alloc(maxTiles + 1));
    SD_HIP(ctx, dSortTmp.alloc(sdRadixSortCountsBytes()));   // the radix sort's count matrix (sd_scan_sort.h)
    SD_HIP(ctx, dScanTmp.alloc(sdScanTmpBytes(std::max<uint64_t>(nSlots, maxTiles) + 1)));
    notePeak();
    SD_HIP(ctx, hipMemsetAsync(dSlotCount.p + nSlots, 0, sizeof(uint32_t), ctx->stream));
    uint32_t bin = 0;
    while (bin < IB_COARSE_BINS) {
        uint32_t e = bin;
        uint64_t n = 0;
        while (e < IB_COARSE_BINS && n + coarse[e] <= cap) n += coarse[e++];
        const uint32_t lo = bin * binWidth;
        const uint32_t hi = (uint32_t) std::min<uint64_t>((uint64_t) e * binWidth, t->tableSize);
        bin = e;
        if (n == 0) continue;
        nPasses++;
        ProfScope ps(ctx, "index_pass");
        int rc = countFn(lo, hi, dSlotCount.p);
        if (rc != SD_OK) return rc;
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, ibScan(ctx, dSlotCount.p, nSlots, dSlotBase.p, (uint64_t *) dScanTmp.p));
        SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        uint64_t got = 0;
        SD_HIP(ctx, hipMemcpy(&got, dSlotBase.p + nSlots, sizeof(got), hipMemcpyDeviceToHost));
        if (got != n) return sdFail(ctx, SD_EHIP, "%s: k-mer range [%u, %u) holds %llu records, the histogram said %llu", who, lo, hi,
                                    (unsigned long long) got, (unsigned long long) n);
        rc = emitFn(lo, hi, (const uint64_t *) dSlotBase.p, k0.p, v0.p);
        if (rc != SD_OK) return rc;
        SD_HIP(ctx, hipGetLastError());
        int bits = 1;
        while (bits < 32 && (1ull << bits) < (uint64_t) (hi - lo)) bits++;
        // stable LSD radix sort of (k-mer, record) pairs by the range's k-mer bits (sd_scan_sort.h, 8 bits per pass), ping-pong between
        // the two buffer pairs: with an odd number of passes the input pair doubles as the scratch pair (it is read by the first pass
        // only and first written by the second) and the result lands in (k1, v1), with an even number in (k0, v0)
        const int passes = std::max(1, (bits + 7) / 8);
        const uint32_t *sk;
        const uint64_t *sv;
        if (passes & 1) {
            SD_HIP(ctx, sdRadixSortPairs<uint64_t>(ctx->stream, k0.p, v0.p, k1.p, v1.p, k0.p, v0.p, (uint32_t) n, 0, bits, (uint32_t *) dSortTmp.p));
            sk = k1.p;
            sv = v1.p;
        } else {
            SD_HIP(ctx, sdRadixSortPairs<uint64_t>(ctx->stream, k0.p, v0.p, k0.p, v0.p, k1.p, v1.p, (uint32_t) n, 0, bits, (uint32_t *) dSortTmp.p));
            sk = k0.p;
            sv = v0.p;
        }
        const unsigned tiles = (unsigned) ((n + IK_TILE - 1) / IK_TILE);
        hipLaunchKernelGGL(ib_keep_count, dim3(tiles), dim3(IK_NT), 0, ctx->stream, sk, sv, n, dTileCount.p);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, hipMemsetAsync(dTileCount.p + tiles, 0, sizeof(uint32_t), ctx->stream));   // (a longer pass left its last count there)
        SD_HIP(ctx, ibScan(ctx, dTileCount.p, tiles, dTileBase.p, (uint64_t *) dScanTmp.p));
        SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        uint64_t kept = 0;
        SD_HIP(ctx, hipMemcpy(&kept, dTileBase.p + tiles, sizeof(kept), hipMemcpyDeviceToHost));
        hipLaunchKernelGGL(ib_place, dim3(tiles), dim3(IK_NT), 0, ctx->stream, sk, sv, n, (const uint64_t *) dTileBase.p, nEntries, lo,
                           t->dEntries, t->dOffsets);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        nEntries += kept;
    }
    return SD_OK;
}

// list starts from the per-k-mer counts the passes left in t->dOffsets (tableSize of them and a zero: the scan's total)
int ibListStarts(sd_ctx *ctx, sd_target *t, const char *who, uint64_t nEntries, bool forceWide, const PeakNote &notePeak) {
    DevBuf<uint64_t> dStart;
    DevBuf<uint8_t> dScanTmp;
    SD_HIP(ctx, dStart.alloc(t->tableSize + 1));
    SD_HIP(ctx, dScanTmp.alloc(sdScanTmpBytes(t->tableSize + 1)));
    notePeak();
    SD_HIP(ctx, ibScan(ctx, t->dOffsets, t->tableSize, dStart.p, (uint64_t *) dScanTmp.p));
    SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t sum = 0;
    SD_HIP(ctx, hipMemcpy(&sum, dStart.p + t->tableSize, sizeof(sum), hipMemcpyDeviceToHost));
    if (sum != nEntries) return sdFail(ctx, SD_EHIP, "%s: %llu entries placed, %llu counted", who, (unsigned long long) nEntries,
                                       (unsigned long long) sum);
    const int wide = nEntries > 0xFFFFFFFFull || forceWide;
    if (wide) SD_HIP(ctx, hipMalloc((void **) &t->dBlockBase, (((t->tableSize + 2) >> 16) + 1) * sizeof(uint64_t)));
    if (wide) SD_HIP(ctx, hipMemsetAsync(t->dBlockBase, 0, (((t->tableSize + 2) >> 16) + 1) * sizeof(uint64_t), ctx->stream));
    hipLaunchKernelGGL(ib_offsets, dim3((unsigned) ((t->tableSize + 1 + 255) / 256)), dim3(256), 0, ctx->stream, (const uint64_t *) dStart.p,
                       t->tableSize + 1, wide, t->dOffsets, t->dBlockBase);
    SD_HIP(ctx, hipGetLastError());
    SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SD_OK;
}

template <int MODE>
using IbMode = std::integral_constant<int, MODE>;

// what a builder says in its own words
struct IbWords {
    const char *who;           // the exported function
    const char *unit;          // what the length of a target counts
    const char *window;        // the kind of its windows (windowed builders)
    const char *histScope;     // profiling scope of the generator's mode 0
    const char *listTooLong;   // a window whose list the reference would cut: format of (target, position, IP_LIST_MAX)
};

// The frame of the three builders.  open() checks the lengths, creates the target (destroyed again unless finish() hands it over) and
// uploads the offsets -- for a windowed builder (span > 0: one generator slot per window of `span` positions) the window prefix as
// well; a builder then uploads what is its own and calls passes() with its generator
//     gen(IbMode<M>(), lo, hi, slotCount, slotBase, keys, vals) -> SD_* code
// which launches its records kernel(s) in mode M on ctx->stream with dCoarse.p, dErr.p and binWidth of the frame (mode 0 counts
// every record into dCoarse, and a windowed generator leaves the first window it refuses in dErr[0]; dErr[1] is the generator's
// own); finish() makes the list starts and fills the statistics.
struct IndexBuild {
    sd_ctx *const ctx;
    const IbWords words;
    const IndexKnobs knobs;
    sd_target *t = nullptr;
    PeakNote notePeak;
    std::vector<uint64_t> winBase;   // windowed builders: the first window of every target, nSeq + 1
    uint64_t nWin = 0;
    uint32_t binWidth = 0;
    DevBuf<uint64_t> dWinBase;
    DevBuf<unsigned long long> dCoarse, dErr;   // mode 0 only: released once the histogram is on the host
    DevBuf<uint32_t> dMode0Count;               // the per-slot counts of mode 0, where a generator leaves them
    uint64_t nRecords = 0, nEntries = 0, nPasses = 0;

    IndexBuild(sd_ctx *c, const IbWords &w) : ctx(c), words(w) {}
    ~IndexBuild() { if (t) sd_target_destroy(t); }
    IndexBuild(const IndexBuild &) = delete;

    template <typename T>
    static hipError_t up(T *&d, const void *h, size_t bytes) {
        hipError_t e = hipMalloc((void **) &d, bytes + 64);
        if (e != hipSuccess) return e;
        return hipMemcpy(d, h, bytes, hipMemcpyDefault);
    }

    int open(int k, uint64_t tableSize, const uint64_t *offsets, uint32_t nSeq, int span) {
        if (span) winBase.assign((size_t) nSeq + 1, 0);
        for (uint32_t i = 0; i < nSeq; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (len > 65535)
                return sdFail(ctx, SD_EINVAL, "target %u has %llu %s; index positions are 16 bit (limit 65535, --max-seq-len)", i,
                              (unsigned long long) len, words.unit);
            if (span) winBase[i + 1] = winBase[i] + (len >= (uint64_t) span ? len - span + 1 : 0);
        }
        if (span) nWin = winBase[nSeq];
        if (nWin >= 0xFFFFFFFFull)
            return sdFail(ctx, SD_EUNSUPPORTED, "%llu %s windows (limit 2^32 per target)", (unsigned long long) nWin, words.window);
        (void) hipSetDevice(ctx->device);
        t = new sd_target();
        t->ctx = ctx;
        t->k = k;
        t->nSeq = nSeq;
        t->tableSize = tableSize;
        t->hSeqOff.assign(offsets, offsets + nSeq + 1);
        binWidth = (uint32_t) ((tableSize + IB_COARSE_BINS - 1) / IB_COARSE_BINS);
        notePeak.begin(t);
        SD_HIP(ctx, up(t->dSeqOff, offsets, ((size_t) nSeq + 1) * sizeof(uint64_t)));
        if (span) {
            SD_HIP(ctx, up(dWinBase.p, winBase.data(), winBase.size() * sizeof(uint64_t)));
            const unsigned long long errInit[2] = {~0ull, 0ull};
            SD_HIP(ctx, dErr.alloc(2));
            SD_HIP(ctx, hipMemcpy(dErr.p, errInit, sizeof(errInit), hipMemcpyHostToDevice));
        }
        return SD_OK;
    }

    // mode0Counts: the generator's mode 0 leaves the records of every slot in slotCount, so a single pass over the whole k-mer space
    // takes its counts from there instead of running mode 1
    template <typename Gen>
    int passes(uint32_t nSlots, bool mode0Counts, Gen gen) {
        std::vector<unsigned long long> coarse(IB_COARSE_BINS, 0);
        if (nSlots) {
            SD_HIP(ctx, dCoarse.alloc(IB_COARSE_BINS));
            SD_HIP(ctx, hipMemsetAsync(dCoarse.p, 0, IB_COARSE_BINS * sizeof(unsigned long long), ctx->stream));
            if (mode0Counts) {
                SD_HIP(ctx, dMode0Count.alloc(nSlots));
                SD_HIP(ctx, hipMemsetAsync(dMode0Count.p, 0, (size_t) nSlots * sizeof(uint32_t), ctx->stream));
            }
            {
                ProfScope ps(ctx, words.histScope);
                if (int rc = gen(IbMode<0>(), 0u, 0u, dMode0Count.p, (const uint64_t *) nullptr, (uint32_t *) nullptr, (uint64_t *) nullptr)) return rc;
            }
            SD_HIP(ctx, hipGetLastError());
            SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (dErr.p) {
                unsigned long long first = ~0ull;
                SD_HIP(ctx, hipMemcpy(&first, dErr.p, sizeof(first), hipMemcpyDeviceToHost));
                if (first != ~0ull) {
                    const uint32_t q = (uint32_t) (std::upper_bound(winBase.begin(), winBase.end(), (uint64_t) first) - winBase.begin() - 1);
                    return sdFail(ctx, SD_EUNSUPPORTED, words.listTooLong, q, (unsigned long long) (first - winBase[q]), IP_LIST_MAX);
                }
            }
            SD_HIP(ctx, hipMemcpy(coarse.data(), dCoarse.p, IB_COARSE_BINS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            dCoarse.release();
            dErr.release();
        }
        uint64_t cap = 0;
        if (int rc = ibPassCap(ctx, knobs, coarse, cap, nRecords)) return rc;
        // the entry array is sized by the counted records (the dedupe only ever removes): one per residue at most in sd_target_build,
        // hundreds per position in the other two
        if (hipMalloc((void **) &t->dEntries, (std::max<uint64_t>(nRecords, 1) + 8) * sizeof(uint2)) != hipSuccess) {
            t->dEntries = nullptr;
            (void) hipGetLastError();
            return sdFail(ctx, SD_ENOMEM, "%s: the entry array of %llu index records (%llu bytes) does not fit the device memory; a higher "
                          "--k-score (fewer k-mers per target) or a smaller target database is the way out", words.who,
                          (unsigned long long) nRecords, (unsigned long long) ((std::max<uint64_t>(nRecords, 1) + 8) * sizeof(uint2)));
        }
        SD_HIP(ctx, hipMalloc((void **) &t->dOffsets, (t->tableSize + 1) * sizeof(uint32_t) + 64));
        SD_HIP(ctx, hipMemsetAsync(t->dOffsets, 0, (t->tableSize + 1) * sizeof(uint32_t), ctx->stream));   // counts first
        if (!nRecords) return SD_OK;
        auto countFn = [&](uint32_t lo, uint32_t hi, uint32_t *slotCount) -> int {
            if (mode0Counts && lo == 0 && hi >= t->tableSize) {   // one pass holds every record: reuse the histogram's counts
                SD_HIP(ctx, hipMemcpyAsync(slotCount, dMode0Count.p, (size_t) nSlots * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
                return SD_OK;
            }
            return gen(IbMode<1>(), lo, hi, slotCount, (const uint64_t *) nullptr, (uint32_t *) nullptr, (uint64_t *) nullptr);
        };
        auto emitFn = [&](uint32_t lo, uint32_t hi, const uint64_t *slotBase, uint32_t *keys, uint64_t *vals) -> int {
            return gen(IbMode<2>(), lo, hi, (uint32_t *) nullptr, slotBase, keys, vals);
        };
        return ibPasses(ctx, t, words.who, coarse, binWidth, nRecords, cap, nSlots, countFn, emitFn, notePeak, nEntries, nPasses);
    }

    int finish(uint64_t nMaskedResidues, sd_target **out, uint64_t *stats) {
        if (int rc = ibListStarts(ctx, t, words.who, nEntries, knobs.wide, notePeak)) return rc;
        t->nEntries = nEntries;
        if (stats) {
            stats[0] = nEntries;
            stats[1] = nMaskedResidues;
            stats[2] = nPasses;
            stats[3] = nRecords;
        }
        *out = t;
        t = nullptr;
        return SD_OK;
    }
};

// the kernels read their tables (seed positions, powers, tantan constants) from __constant__ memory: one build at a time
std::mutex &ibBuildMutex() {
    static std::mutex m;
    return m;
}

}  // namespace

extern "C" int sd_target_build(sd_ctx *ctx, int kmerSize, int kmerThr, int mask, double maskProb, const uint8_t *residues,
                               const uint64_t *seqOffsets, uint32_t nSeq, const double *maskRatios, const int8_t *selfScore,
                               const int16_t *ext2Score, const uint16_t *ext2Index, const int16_t *ext3Score,
                               const uint16_t *ext3Index, sd_target **out, uint64_t *stats) {
    if (!ctx || !out || !residues || !seqOffsets || !maskRatios || !selfScore || !ext3Score || !ext3Index) return SD_EINVAL;
    const SdKmerShape *shape = sdKmerShape(kmerSize);
    if (!shape) return sdFail(ctx, SD_EUNSUPPORTED, "k=%d: the device implements k=5, k=6 and k=7", kmerSize);
    if (kmerSize != 6 && (!ext2Score || !ext2Index)) return sdFail(ctx, SD_EINVAL, "k=%d needs the 2-mer score matrix", kmerSize);
    std::lock_guard<std::mutex> buildLock(ibBuildMutex());
    IndexBuild b(ctx, {"sd_target_build", "residues", nullptr, "index_kmer_histogram", nullptr});
    if (int rc = b.open(kmerSize, shape->tableSize, seqOffsets, nSeq, 0)) return rc;
    sd_target *t = b.t;
    const int span = shape->span;
    {
        uint32_t pw[8] = {0};
        uint32_t p = 1;
        for (int i = 0; i < kmerSize; i++) {
            pw[i] = p;
            p *= 20;
        }
        int self[IB_ALPH];
        for (int a = 0; a < IB_ALPH; a++) self[a] = selfScore[a];
        SD_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_ibSeed), shape->seed, 8));
        SD_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_ibPow), pw, sizeof(pw)));
        SD_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_ibSelf), self, sizeof(self)));
    }
    SD_HIP(ctx, b.up(t->dExt3Score, ext3Score, (size_t) 8000 * 8000 * sizeof(int16_t)));
    SD_HIP(ctx, b.up(t->dExt3Index, ext3Index, (size_t) 8000 * 8000 * sizeof(uint16_t)));
    if (int rc = sdBuildExt3Cum(ctx, t)) return rc;
    if (ext2Score && ext2Index) {
        SD_HIP(ctx, b.up(t->dExt2Score, ext2Score, (size_t) 400 * 400 * sizeof(int16_t)));
        SD_HIP(ctx, b.up(t->dExt2Index, ext2Index, (size_t) 400 * 400 * sizeof(uint16_t)));
    }
    SD_HIP(ctx, hipMalloc((void **) &t->dMasked, std::max<uint64_t>(seqOffsets[nSeq], 1) + 64));
    uint64_t nMaskedResidues = 0;
    if (int rc = ibMaskPhase(ctx, t, b.knobs, residues, seqOffsets, nSeq, mask, maskProb, maskRatios, b.notePeak, nMaskedResidues)) return rc;
    // a slot: the IB_SEQ_PER_WAVE sequences of one wavefront
    const uint32_t nWavesR = (uint32_t) (((uint64_t) nSeq + IB_SEQ_PER_WAVE - 1) / IB_SEQ_PER_WAVE);
    auto generate = [&](auto mode, uint32_t lo, uint32_t hi, uint32_t *waveCount, const uint64_t *waveBase, uint32_t *keys, uint64_t *vals) -> int {
        constexpr int MODE = decltype(mode)::value;
        const auto kernel = kmerSize == 5 ? ib_records_kernel<5, MODE> : kmerSize == 6 ? ib_records_kernel<6, MODE> : ib_records_kernel<7, MODE>;
        hipLaunchKernelGGL(kernel, dim3((nWavesR + 3) / 4), dim3(256), 0, ctx->stream, (const uint8_t *) t->dMasked, (const uint64_t *) t->dSeqOff,
                           nSeq, span, kmerThr, b.binWidth, b.dCoarse.p, lo, hi, waveCount, waveBase, keys, vals);
        return SD_OK;
    };
    if (int rc = b.passes(nWavesR, false, generate)) return rc;
    return b.finish(nMaskedResidues, out, stats);
}

// The masking phase alone, for tests/ (tests/test_gpu_tantan.py reads the kernel's float posteriors through maskProb): ibMaskPhase as
// sd_target_build calls it -- same knobs, same dealing of the sequences, same launches of ib_mask_kernel -- on a target that holds
// the offsets and the masked residues only; the bytes and the count are copied out.
extern "C" int sd_selftest_mask(sd_ctx *ctx, sd_host *host, const uint8_t *residues, const uint64_t *seqOffsets, uint32_t nSeq, double maskProb,
                                uint8_t *maskedOut, uint64_t *nMaskedOut) {
    if (!ctx || !host || !residues || !seqOffsets || !maskedOut) return SD_EINVAL;
    double ratios[IB_ALPH * IB_ALPH];
    int8_t self[IB_ALPH];
    if (int rc = sd_host_index_tables(host, ratios, self)) return rc;
    std::lock_guard<std::mutex> buildLock(ibBuildMutex());
    IndexBuild b(ctx, {"sd_selftest_mask", "residues", nullptr, nullptr, nullptr});
    if (int rc = b.open(6, 0, seqOffsets, nSeq, 0)) return rc;
    sd_target *t = b.t;
    const uint64_t total = seqOffsets[nSeq];
    SD_HIP(ctx, hipMalloc((void **) &t->dMasked, std::max<uint64_t>(total, 1) + 64));
    uint64_t nMaskedResidues = 0;
    if (int rc = ibMaskPhase(ctx, t, b.knobs, residues, seqOffsets, nSeq, 1, maskProb, ratios, b.notePeak, nMaskedResidues)) return rc;
    SD_HIP(ctx, hipMemcpy(maskedOut, t->dMasked, total, hipMemcpyDeviceToHost));
    if (nMaskedOut) *nMaskedOut = nMaskedResidues;
    return SD_OK;
}

// The index of a *profile* target DB (the profile branch of IndexBuilder::fillDatabase, IndexBuilder.cpp:61-62,94-128,200-219): the lists
// hold the similar k-mers of every profile window at threshold kmerThr, one entry per (k-mer, target) at the smallest position, in
// (target, position) order; nothing is masked (Prefiltering.cpp:172-174) and the lookup holds the consensus letters
// (IndexBuilder.cpp:125-127).  The arrays are Sequence::mapProfile's (sd_host_map_profiles).  A window yields hundreds to tens of
// thousands of records, so nothing here is sized by the record total except the entry array itself: the generator runs once for the
// histogram and list lengths and, when the records do not fit one pass (SD_INDEX_PASS, 2^30), once to count and once to write per pass.
extern "C" int sd_target_build_profile(sd_ctx *ctx, int kmerSize, int kmerThr, const uint8_t *queryLetters, const uint8_t *consensus,
                                       const int16_t *sortedScore, const uint8_t *sortedIndex, const uint64_t *posOffsets, uint32_t nSeq,
                                       sd_target **out, uint64_t *stats) {
    if (!ctx || !out || !queryLetters || !consensus || !sortedScore || !sortedIndex || !posOffsets) return SD_EINVAL;
    if (kmerSize == 7)
        return sdFail(ctx, SD_EUNSUPPORTED, "k=7: the index of a profile target is built at k=5 and k=6 only (no k=7 golden index of the reference to test against)");
    if (kmerSize != 5 && kmerSize != 6) return sdFail(ctx, SD_EUNSUPPORTED, "k=%d: the index of a profile target is built at k=5 and k=6", kmerSize);
    const SdKmerShape *shape = sdKmerShape(kmerSize);
    IndexBuild b(ctx, {"sd_target_build_profile", "positions", "profile", "index_profile_histogram",
                       "target %u, position %llu: more than %u similar k-mers in one profile window (the reference's buffer ends there, "
                       "KmerGenerator.h:45); raise the k-mer threshold"});
    if (int rc = b.open(kmerSize, shape->tableSize, posOffsets, nSeq, shape->span)) return rc;
    sd_target *t = b.t;
    t->similar = true;
    const uint64_t nWin = b.nWin, total = posOffsets[nSeq];
    SD_HIP(ctx, b.up(t->dMasked, consensus, total));   // what the diagonal scoring reads
    DevBuf<uint8_t> dLetters, dIndex, dBig;
    DevBuf<int16_t> dScore;
    DevBuf<uint2> dScratch, dScratchBig;
    const uint32_t grid = (uint32_t) std::min<uint64_t>(std::max<uint64_t>(nWin, 1), b.knobs.profileGrid);
    const uint32_t gridBig = (uint32_t) std::min<uint64_t>(std::max<uint64_t>(nWin, 1), IP_GRID_BIG);
    SD_HIP(ctx, b.up(dLetters.p, queryLetters, total));
    SD_HIP(ctx, b.up(dScore.p, sortedScore, total * 20 * sizeof(int16_t)));
    SD_HIP(ctx, b.up(dIndex.p, sortedIndex, total * 20));
    SD_HIP(ctx, dBig.alloc(nWin + 1));
    SD_HIP(ctx, dScratch.alloc((size_t) grid * 2 * PROFILE_PARTIAL_CAP));
    SD_HIP(ctx, hipMemsetAsync(dBig.p, 0, nWin + 1, ctx->stream));
    bool anyBig = false;
    // the generator in one of its modes, on the tier(s) the windows run in; b.dErr[1]: the windows mode 0 moved to the big tier
    auto generate = [&](auto mode, uint32_t lo, uint32_t hi, uint32_t *winCount, const uint64_t *recBase, uint32_t *keys, uint64_t *vals) -> int {
        constexpr int MODE = decltype(mode)::value;
        const auto kernel = kmerSize == 5 ? ib_profile_records_kernel<5, MODE> : ib_profile_records_kernel<6, MODE>;
        for (int bigTier = 0; bigTier <= (anyBig ? 1 : 0); bigTier++) {
            hipLaunchKernelGGL(kernel, dim3(bigTier ? gridBig : grid), dim3(64), 0, ctx->stream, nWin,
                               (const uint64_t *) b.dWinBase.p, nSeq, (const uint8_t *) dLetters.p, (const uint64_t *) t->dSeqOff,
                               (const int16_t *) dScore.p, (const uint8_t *) dIndex.p, kmerThr, bigTier ? dScratchBig.p : dScratch.p,
                               bigTier ? PROFILE_PARTIAL_CAP_BIG : PROFILE_PARTIAL_CAP, dBig.p, bigTier, b.binWidth, b.dCoarse.p, b.dErr.p, lo, hi,
                               winCount, recBase, keys, vals);
            if (MODE == 0 && !bigTier) {   // which windows outgrew the wide tier's lists is known only now: they get their scratch
                unsigned long long hErr[2] = {~0ull, 0ull};
                SD_HIP(ctx, hipGetLastError());
                SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
                SD_HIP(ctx, hipMemcpy(hErr, b.dErr.p, sizeof(hErr), hipMemcpyDeviceToHost));
                anyBig = hErr[1] != 0;
                if (anyBig) SD_HIP(ctx, dScratchBig.alloc((size_t) gridBig * 2 * PROFILE_PARTIAL_CAP_BIG));
            }
        }
        return SD_OK;
    };
    if (int rc = b.passes((uint32_t) nWin, true, generate)) return rc;
    return b.finish(0, out, stats);
}

// The similar-k-mer index of a *sequence* target DB (--target-search-mode 1; the sequence branch of the same reference code,
// IndexBuilder.cpp:62,100,120-127): the lists hold generateKmerList of every window without X at kmerThr -- the sequence threshold
// itself (Prefiltering.cpp:525-527) -- deduplicated and ordered like the profile index; nothing is masked and the lookup holds the
// residues as they came.  Same pass pipeline; the generator needs no scratch (ib_similar_records_kernel).
extern "C" int sd_target_build_similar(sd_ctx *ctx, int kmerSize, int kmerThr, const uint8_t *residues, const uint64_t *seqOffsets, uint32_t nSeq,
                                       const int16_t *ext3Score, const uint16_t *ext3Index, sd_target **out, uint64_t *stats) {
    if (!ctx || !out || !residues || !seqOffsets || !ext3Score || !ext3Index) return SD_EINVAL;
    if (kmerSize == 7)
        return sdFail(ctx, SD_EUNSUPPORTED, "k=7: the similar-k-mer index of a sequence target is built at k=6 only (the 3 x 3 array product; k=7 divides 2, 2, 3)");
    if (kmerSize != 6) return sdFail(ctx, SD_EUNSUPPORTED, "k=%d: the similar-k-mer index of a sequence target is built at k=6", kmerSize);
    IndexBuild b(ctx, {"sd_target_build_similar", "residues", "sequence", "index_similar_histogram",
                       "target %u, position %llu: %u similar k-mers or more in one sequence window (the reference's buffer ends there, "
                       "KmerGenerator.h:45); raise the k-mer threshold"});
    if (int rc = b.open(kmerSize, 64000000ull, seqOffsets, nSeq, 10)) return rc;
    sd_target *t = b.t;
    t->similar = true;
    t->similarSeq = true;
    const uint64_t nWin = b.nWin;
    SD_HIP(ctx, b.up(t->dMasked, residues, seqOffsets[nSeq]));   // the lookup of the diagonal scoring: unmasked (IndexBuilder.cpp:125-127)
    // the 3-mer tables serve the generator only: a query looks up its own k-mers, so they are released before the list starts are made
    SD_HIP(ctx, b.up(t->dExt3Score, ext3Score, (size_t) 8000 * 8000 * sizeof(int16_t)));
    SD_HIP(ctx, b.up(t->dExt3Index, ext3Index, (size_t) 8000 * 8000 * sizeof(uint16_t)));
    if (int rc = sdBuildExt3Cum(ctx, t)) return rc;
    const uint32_t grid = (uint32_t) std::min<uint64_t>(std::max<uint64_t>(nWin, 1), IS_GRID);
    auto generate = [&](auto mode, uint32_t lo, uint32_t hi, uint32_t *winCount, const uint64_t *recBase, uint32_t *keys, uint64_t *vals) -> int {
        constexpr int MODE = decltype(mode)::value;
        hipLaunchKernelGGL((ib_similar_records_kernel<MODE>), dim3(grid), dim3(64), 0, ctx->stream, nWin, (const uint64_t *) b.dWinBase.p, nSeq,
                           (const uint8_t *) t->dMasked, (const uint64_t *) t->dSeqOff, (const int16_t *) t->dExt3Score,
                           (const uint16_t *) t->dExt3Index, (const uint16_t *) t->dExt3Cum, t->ext3Lo, kmerThr, b.binWidth, b.dCoarse.p, b.dErr.p,
                           lo, hi, winCount, recBase, keys, vals);
        return SD_OK;
    };
    if (int rc = b.passes((uint32_t) nWin, true, generate)) return rc;
    for (void **p : {(void **) &t->dExt3Score, (void **) &t->dExt3Index, (void **) &t->dExt3Cum}) {
        if (*p) (void) hipFree(*p);
        *p = nullptr;
    }
    return b.finish(0, out, stats);
}

// The model behind `prefilter --split 0`: every hipMalloc of sd_target_build above, with the data-dependent sizes replaced by
// their ceilings -- one record per residue, a masking scratch that holds every wavefront at once (the build caps it at an eighth
// of the device) -- and each allocation rounded up to 2 MiB.  The phases release their scratch, so the peak is the largest of them.
extern "C" uint64_t sd_target_footprint(int kmerSize, uint64_t nSeq, uint64_t nResidues) {
    if (kmerSize != 6 && kmerSize != 7) return 0;
    const uint64_t G = 2ull << 20;
    auto a = [&](uint64_t bytes) { return (std::max<uint64_t>(bytes, 1) + G - 1) / G * G; };
    const uint64_t T = kmerSize == 6 ? 64000000ull : 1280000000ull, R = nResidues, S = nSeq;
    // resident from the start: sequence offsets, 3-mer and 2-mer matrices, the cumulative 3-mer table (+ its min/max pair), masked residues
    const uint64_t tables = a((S + 1) * 8 + 64) + 2 * a(8000ull * 8000 * 2 + 64) + a(8000ull * 256 * 2) + a(8) + 2 * a(400ull * 400 * 2 + 64) +
                            a(R + 64);
    // 1. masking (ibMaskPhase): the residues, the length order, and 64 lanes x (4 + 8 / TT_SCALE) bytes per row; a wavefront's rows are
    //    its longest sequence rounded up to TT_SCALE; sorted by length, 64 x the rows of a wave are at most the residues of the next full
    //    wave, which leaves the last two waves (at most 65 535 rows each) and the rounding
    const uint64_t nWaves = (S + 63) / 64;
    const uint64_t rows = (R + 63) / 64 + 2 * 65535 + (nWaves + 2) * TT_SCALE;
    const uint64_t maskPhase = a(R + 64) + a(S * 4) + a((nWaves + 1) * 8) + a(rows * 64 * sizeof(float)) + a((rows / TT_SCALE * 64 + 64) * sizeof(double)) +
                               a(IB_ALPH * IB_ALPH * 8) + a(8);
    // 2. records (IndexBuild::passes, ibPasses): the entries and counts stay; the histogram goes before the sort's two (k-mer, record)
    //    buffer pairs, the slot and tile counts with their scanned bases (one element more each) and the scan's tile sums come
    const uint64_t entries = a((std::max<uint64_t>(R, 1) + 8) * 8) + a((T + 1) * 4 + 64);
    const uint64_t bufN = std::min<uint64_t>(1ull << 30, std::max<uint64_t>(R, 1));
    const uint64_t nWavesR = (S + IB_SEQ_PER_WAVE - 1) / IB_SEQ_PER_WAVE, tiles = (bufN + IK_TILE - 1) / IK_TILE;
    const uint64_t sortPhase = std::max<uint64_t>(a(IB_COARSE_BINS * 8),
                                                  2 * a(bufN * 4) + 2 * a(bufN * 8) + a((nWavesR + 1) * 4) + a((nWavesR + 1) * 8) + a((tiles + 1) * 4) +
                                                      a((tiles + 1) * 8) + a(sdRadixSortCountsBytes()) + a(sdScanTmpBytes(std::max(nWavesR, tiles) + 1)));
    // 3. list starts (ibListStarts): 64-bit starts of the whole table, the scan's tile sums, the wide index's block bases
    const uint64_t startPhase = a((T + 1) * 8) + a(sdScanTmpBytes(T + 1)) + a((((T + 2) >> 16) + 1) * 8);
    // what the HIP runtime itself takes from the device when the build's kernels first run (code objects, kernel-argument and signal pools)
    const uint64_t runtime = 32ull << 20;
    return tables + std::max(maskPhase, entries + std::max(sortPhase, startPhase)) + runtime;
}

extern "C" int sd_target_build_peak(const sd_target *t, uint64_t *bytes) {
    if (!t || !bytes) return SD_EINVAL;
    *bytes = t->buildPeak;
    return SD_OK;
}

namespace {
// triple x = (k-mer, sequence, position): is it an entry of the index?  Lists are ordered by sequence.
__global__ void __launch_bounds__(256) ib_check_triples(const uint32_t *__restrict__ offsets, const uint64_t *__restrict__ blockBase,
                                                        const uint2 *__restrict__ entries, const uint32_t *__restrict__ kmer,
                                                        const uint32_t *__restrict__ seq, const uint32_t *__restrict__ pos, uint64_t n,
                                                        unsigned long long *__restrict__ missing) {
    const uint64_t x = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const uint64_t km = kmer[x];
    uint64_t lo = (blockBase ? blockBase[km >> 16] : 0) + offsets[km];
    uint64_t hi = (blockBase ? blockBase[(km + 1) >> 16] : 0) + offsets[km + 1];
    const uint32_t want = seq[x];
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (entries[mid].x < want) lo = mid + 1;
        else hi = mid;
    }
    const uint64_t end = (blockBase ? blockBase[(km + 1) >> 16] : 0) + offsets[km + 1];
    if (!(lo < end && entries[lo].x == want && entries[lo].y == pos[x])) atomicAdd(missing, 1ull);
}
// number of entries that belong to one of the (ascending) sample sequences
__global__ void __launch_bounds__(256) ib_count_sample(const uint2 *__restrict__ entries, uint64_t nEntries, const uint32_t *__restrict__ sample,
                                                       uint32_t nSample, unsigned long long *__restrict__ count) {
    unsigned long long mine = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < nEntries; i += (uint64_t) gridDim.x * 256) {
        const uint32_t s = entries[i].x;
        uint32_t lo = 0, hi = nSample;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (sample[mid] < s) lo = mid + 1;
            else hi = mid;
        }
        mine += (lo < nSample && sample[lo] == s) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}
}  // namespace

// Sampled check of an index too large to download (10^4 proteomes: 72 GB of entries): for n (k-mer, sequence, position)
// triples -- the complete entries of the nSample sequences `sample` (ascending), computed elsewhere -- *missing = how many are
// not entries of the index, *inSample = how many entries of the index belong to the sample sequences (equal to n exactly when
// the index holds nothing else for them); the masked residues of [resBegin, resEnd) are copied to maskedOut (nullable).
extern "C" int sd_target_sample_check(sd_ctx *ctx, const sd_target *t, const uint32_t *kmer, const uint32_t *seq, const uint32_t *pos,
                                      uint64_t n, const uint32_t *sample, uint32_t nSample, uint64_t *missing, uint64_t *inSample,
                                      uint64_t resBegin, uint64_t resEnd, uint8_t *maskedOut) {
    if (!ctx || !t || !missing || !inSample || (n && (!kmer || !seq || !pos)) || (nSample && !sample)) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    DevBuf<uint32_t> dK, dS, dP, dSample;
    DevBuf<unsigned long long> dOut;
    SD_HIP(ctx, dK.alloc(std::max<uint64_t>(n, 1)));   // (at least one element: the copies below take the pointers whatever n is)
    SD_HIP(ctx, dS.alloc(std::max<uint64_t>(n, 1)));
    SD_HIP(ctx, dP.alloc(std::max<uint64_t>(n, 1)));
    SD_HIP(ctx, dSample.alloc(std::max<uint32_t>(nSample, 1)));
    SD_HIP(ctx, dOut.alloc(2));
    SD_HIP(ctx, hipMemcpy(dK.p, kmer, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    SD_HIP(ctx, hipMemcpy(dS.p, seq, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    SD_HIP(ctx, hipMemcpy(dP.p, pos, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    SD_HIP(ctx, hipMemcpy(dSample.p, sample, (size_t) nSample * sizeof(uint32_t), hipMemcpyHostToDevice));
    SD_HIP(ctx, hipMemsetAsync(dOut.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
    if (n)
        hipLaunchKernelGGL(ib_check_triples, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t *) t->dOffsets,
                           (const uint64_t *) t->dBlockBase, (const uint2 *) t->dEntries, (const uint32_t *) dK.p, (const uint32_t *) dS.p,
                           (const uint32_t *) dP.p, n, dOut.p);
    if (t->nEntries && nSample)
        hipLaunchKernelGGL(ib_count_sample, dim3(8192), dim3(256), 0, ctx->stream, (const uint2 *) t->dEntries, t->nEntries,
                           (const uint32_t *) dSample.p, nSample, dOut.p + 1);
    SD_HIP(ctx, hipGetLastError());
    SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long h[2] = {0, 0};
    SD_HIP(ctx, hipMemcpy(h, dOut.p, sizeof(h), hipMemcpyDeviceToHost));
    *missing = h[0];
    *inSample = h[1];
    if (maskedOut && resEnd > resBegin) SD_HIP(ctx, hipMemcpy(maskedOut, t->dMasked + resBegin, resEnd - resBegin, hipMemcpyDeviceToHost));
    return SD_OK;
}

// the pieces of a target as the device holds them (tests: device-built index against the host-built one).  Any pointer may
// be NULL; entries = nEntries x (sequence id, position); starts = absolute list starts, tableSize + 1 of them
extern "C" int sd_target_download(sd_ctx *ctx, const sd_target *t, uint64_t *nEntries, uint64_t *tableSize, uint8_t *masked,
                                  uint64_t *starts, uint32_t *entrySeq, uint16_t *entryPos) {
    if (!ctx || !t) return SD_EINVAL;
    if (nEntries) *nEntries = t->nEntries;
    if (tableSize) *tableSize = t->tableSize;
    if (masked) SD_HIP(ctx, hipMemcpy(masked, t->dMasked, t->hSeqOff.back(), hipMemcpyDeviceToHost));
    if (starts) {
        std::vector<uint32_t> off(t->tableSize + 1);
        SD_HIP(ctx, hipMemcpy(off.data(), t->dOffsets, off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::vector<uint64_t> bb;
        if (t->dBlockBase) {
            bb.resize(((t->tableSize + 2) >> 16) + 1);
            SD_HIP(ctx, hipMemcpy(bb.data(), t->dBlockBase, bb.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        }
        for (uint64_t i = 0; i <= t->tableSize; i++) starts[i] = (bb.empty() ? 0 : bb[i >> 16]) + off[i];
    }
    if (entrySeq || entryPos) {
        const uint64_t CH = 1ull << 24;
        std::vector<uint2> buf(CH);
        for (uint64_t b = 0; b < t->nEntries; b += CH) {
            const uint64_t n = std::min(CH, t->nEntries - b);
            SD_HIP(ctx, hipMemcpy(buf.data(), t->dEntries + b, n * sizeof(uint2), hipMemcpyDeviceToHost));
            for (uint64_t i = 0; i < n; i++) {
                if (entrySeq) entrySeq[b + i] = buf[i].x;
                if (entryPos) entryPos[b + i] = (uint16_t) buf[i].y;
            }
        }
    }
    return SD_OK;
}
