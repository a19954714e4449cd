// Exhaustive ungapped prefilter (`ungappedprefilter`, `search --prefilter-mode 1`): every query of a set against every
// target of a resident set with the byte-saturated ungapped scan SmithWaterman::ungapped_alignment
// (M/src/alignment/StripedSmithWaterman.cpp:1722-1781), followed by the list rule of runFilterOnCpu with alignment mode 0
// (M/src/prefiltering/ungappedprefilter.cpp:338-477).  DESIGN.md 4.8 has the layout and the instruction count.
//
//   S(i, j) = max(0, min(255 - bias, S(i-1, j-1) + M[t_j][q_i] + cb_i)),  score = max S
//
// The reference's two saturating byte operations (adds bias-shifted profile, subs bias) equal one min and one max on wider
// lanes, so the recurrence runs on packed int16 halves and stays bit-exact.
//
// Mapping onto a CDNA4 wavefront
//   * a workgroup of four wavefronts shares ONE query: its profile (21 residue rows x ROWS int16 entries, two query rows per
//     dword) is built once in LDS; every wavefront scans targets of its own against it;
//   * lane l owns RT consecutive query rows, two per VGPR (row 2r in the low half, 2r + 1 in the high half).  The recurrence
//     only moves along diagonals, so all lanes work on the SAME target column: no systolic skew, no fill or drain steps;
//   * per column: one v_readlane of the target residue (fetched 64 columns at a time, coalesced), one LDS read of RT/2 dwords
//     of the profile row, one DPP wave_shr:1 move that hands row RT-1 of lane l-1 to lane l, and per VGPR (two cells)
//     v_alignbit (the diagonal shift inside the lane), v_pk_add_u16, v_pk_min_i16 (ceiling), v_pk_max_i16 (floor 0),
//     v_pk_max_u16 (running best);
//   * queries longer than one strip (64 * RT rows) are scanned strip by strip; the bottom row of a strip goes through a
//     per-wavefront boundary line in global memory: one store per column and strip, read back 64 columns at a time.
// The scores (a byte each: the ceiling is below 256) of a sub-batch of queries stay in a device workspace; the select kernel
// right behind the scan applies the list rule and only the kept hits (at most --max-seqs per query) leave the device.
#include "sd_common.h"
#include "sd_sw_pk.h"

#include <cmath>
#include <memory>

namespace {

using sdpk::pkAdd;
using sdpk::pkMax;
using sdpk::dppShr1;
using sdpk::readLane;

__device__ __forceinline__ uint32_t pkMin(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(sdpk::s16x2, a), __builtin_bit_cast(sdpk::s16x2, b)));
}

constexpr int UG_WAVES = 4;          // wavefronts per workgroup (one query, four targets at a time)
constexpr int UG_OFF_ROW = -512;     // profile entry of the rows past the query's end: any S + this is below 0

// Util::canBeCovered (M/src/commons/Util.cpp:477-494), as sd::canBeCovered states it on the host
__host__ __device__ inline bool ugCanBeCovered(float covThr, int covMode, float queryLength, float targetLength) {
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

// rows[blockIdx.y]: row of the score workspace = query q0 + row of the set.  MULTI: queries of more than one strip.
// boundary (MULTI): per wavefront two lines of lineLen dwords (ping-pong between consecutive strips).
template <int RT, bool MULTI>
__global__ void __launch_bounds__(64 * UG_WAVES)
ungapped_scan_kernel(const uint32_t *__restrict__ rows, uint32_t q0, const uint8_t *__restrict__ qRes, const int8_t *__restrict__ qBias,
                     const uint64_t *__restrict__ qOff, const int32_t *__restrict__ capOfRow, const uint8_t *__restrict__ tRes,
                     const uint64_t *__restrict__ tOff, uint32_t nT, const int8_t *__restrict__ mat, uint8_t *__restrict__ scores,
                     uint64_t rowStride, uint32_t *__restrict__ boundary, uint32_t lineLen) {
    constexpr int ROWS = 64 * RT;
    constexpr int R = RT / 2;            // packed registers per lane
    constexpr int PSTRIDE = ROWS / 2;    // dwords per residue row of the profile
    __shared__ __attribute__((aligned(16))) uint32_t prof[21][PSTRIDE];
    __shared__ int8_t smat[441];
    for (int i = threadIdx.x; i < 441; i += 64 * UG_WAVES) smat[i] = mat[i];

    const uint32_t row = rows[blockIdx.y];
    const uint32_t q = q0 + row;
    const uint64_t qo = qOff[q];
    const int qLen = (int) (qOff[q + 1] - qo);
    const int cap = capOfRow[row];
    const uint32_t capP = (uint32_t) cap | ((uint32_t) cap << 16);
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)), l = threadIdx.x & 63;   // (uniform: target, length and loop bounds live in SGPRs)
    const int nStrips = MULTI ? (qLen + ROWS - 1) / ROWS : (qLen > 0 ? 1 : 0);
    uint32_t *line[2] = {nullptr, nullptr};
    if (MULTI) {
        line[0] = boundary + ((size_t) (blockIdx.y * gridDim.x + blockIdx.x) * UG_WAVES + wave) * 2 * lineLen;
        line[1] = line[0] + lineLen;
    }
    const uint32_t *myProf = &prof[0][0] + l * R;
    uint8_t *outRow = scores + (size_t) row * rowStride;

    bool built = false;
    for (uint32_t g = blockIdx.x; (uint64_t) g * UG_WAVES < nT; g += gridDim.x) {
        const uint32_t t = g * UG_WAVES + wave;
        const bool haveT = t < nT;
        const uint64_t to = haveT ? tOff[t] : 0;
        const int tL = haveT ? (int) (tOff[t + 1] - to) : 0;
        uint32_t best = 0;
        for (int strip = 0; strip < nStrips; strip++) {
            if (MULTI || !built) {
                // ---- the strip's profile: entry (a, i) = M[a][q_i] + cb_i, two rows per dword
                __syncthreads();   // (the previous strip's reads are done; smat is complete)
                for (int idx = threadIdx.x; idx < 21 * PSTRIDE; idx += 64 * UG_WAVES) {
                    const int a = idx / PSTRIDE, w = idx % PSTRIDE;
                    const int i0 = strip * ROWS + 2 * w;
                    int v0 = UG_OFF_ROW, v1 = UG_OFF_ROW;
                    if (i0 < qLen) v0 = (int) smat[a * 21 + min((int) qRes[qo + i0], 20)] + (int) qBias[qo + i0];
                    if (i0 + 1 < qLen) v1 = (int) smat[a * 21 + min((int) qRes[qo + i0 + 1], 20)] + (int) qBias[qo + i0 + 1];
                    prof[a][w] = ((uint32_t) v0 & 0xFFFFu) | ((uint32_t) v1 << 16);
                }
                __syncthreads();
                built = true;
            }
            if (tL == 0) continue;   // (wave-uniform)
            uint32_t S[R];
#pragma unroll
            for (int r = 0; r < R; r++) S[r] = 0;
            const uint32_t *lineIn = MULTI ? line[(strip + 1) & 1] : nullptr;
            uint32_t *lineOut = MULTI ? line[strip & 1] : nullptr;
            const bool readB = MULTI && strip > 0, writeB = MULTI && strip + 1 < nStrips;
            for (int c0 = 0; c0 < tL; c0 += 64) {
                const int col = c0 + l;
                uint32_t tChunk = 0, bChunk = 0;
                if (col < tL) tChunk = min((uint32_t) tRes[to + col], 20u);
                // lane 0 of column j continues the diagonal from row -1 of this strip at column j - 1
                if (readB && col >= 1 && col <= tL)
                    bChunk = __hip_atomic_load(&lineIn[col - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int steps = min(64, tL - c0);
                auto step = [&](int k) {
                    const uint32_t tj = readLane(tChunk, k);
                    uint32_t p[R];
                    const uint32_t *pr = myProf + tj * PSTRIDE;
                    if constexpr (R == 4) {   // one ds_read_b128 / b64 / b32 per column
                        const uint4 v = *(const uint4 *) pr;
                        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
                    } else if constexpr (R == 2) {
                        const uint2 v = *(const uint2 *) pr;
                        p[0] = v.x; p[1] = v.y;
                    } else {
                        p[0] = pr[0];
                    }
                    uint32_t prev = dppShr1(S[R - 1]);   // row RT-1 of lane l-1 in the high half; lane 0: 0
                    if (MULTI) {
                        const uint32_t inb = readLane(bChunk, k);
                        prev = l == 0 ? inb : prev;
                    }
#pragma unroll
                    for (int r = R - 1; r >= 0; r--) {
                        // diagonal shift: low half <- row 2r-1 (high half of the register below), high half <- row 2r
                        const uint32_t d = __builtin_amdgcn_alignbit(S[r], r ? S[r - 1] : prev, 16);
                        S[r] = pkMax(pkMin(pkAdd(d, p[r]), capP), 0u);
                        best = pkMax(best, S[r]);
                    }
                    if (MULTI && writeB && l == 63) lineOut[c0 + k] = S[R - 1] & 0xFFFF0000u;
                };
                int k = 0;
                for (; k + 4 <= steps; k += 4) {   // four columns per trip: their profile reads issue ahead of the arithmetic
                    step(k);
                    step(k + 1);
                    step(k + 2);
                    step(k + 3);
                }
                for (; k < steps; k++) step(k);
            }
            if (MULTI) __threadfence();   // the boundary line is read by the other lanes of this wavefront in the next strip
        }
        if (haveT) {
            uint32_t m = max(best & 0xFFFFu, best >> 16);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t) __shfl_xor((int) m, off, 64));
            if (l == 0) outRow[t] = (uint8_t) m;
        }
    }
}

// The list rule for one query per workgroup, over its row of scores: coverage, threshold / identity, and the cut to maxHits
// by (score descending, target key ascending) -- a histogram of the scores finds the score at the cut, a four-round radix
// select over the keys of the targets with that score the key at the cut.  The kept hits are written unordered.
__global__ void __launch_bounds__(256)
ungapped_select_kernel(const uint8_t *__restrict__ scores, uint64_t rowStride, uint32_t nT, uint32_t q0, const uint64_t *__restrict__ qOff,
                       const uint32_t *__restrict__ tLen, const uint32_t *__restrict__ tKeys, const uint32_t *__restrict__ ident,
                       int covMode, float covThr, int minScore, uint32_t maxHits, sd_hit *__restrict__ out, uint32_t *__restrict__ outCount) {
    __shared__ uint32_t hist[256];
    __shared__ int sCut;
    __shared__ uint32_t sNeed, sPrefix, sCount;
    const uint32_t row = blockIdx.x, q = q0 + row;
    const uint8_t *sc = scores + (size_t) row * rowStride;
    const float qLen = (float) (qOff[q + 1] - qOff[q]);
    const uint32_t idn = ident ? ident[q] : 0xFFFFFFFFu;
    auto passes = [&](uint32_t t, int s) {
        return ugCanBeCovered(covThr, covMode, qLen, (float) tLen[t]) && (s > minScore || t == idn);
    };
    hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) sCount = 0;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < nT; t += 256) {
        const int s = sc[t];
        if (passes(t, s)) atomicAdd(&hist[s], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t cum = 0;
        int cut = -1;
        uint32_t need = 0;
        for (int s = 255; s >= 0; s--) {
            if (cum + hist[s] >= maxHits) {   // the cut falls inside score s: `need` of its targets are kept
                cut = s;
                need = maxHits - cum;
                break;
            }
            cum += hist[s];
        }
        sCut = cut;
        sNeed = (cut >= 0 && hist[cut] > need) ? need : 0;   // 0: every target with the cut score is kept
        sPrefix = 0;
    }
    __syncthreads();
    const int cut = sCut;
    uint32_t keyMax = 0xFFFFFFFFu;
    if (sNeed) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[threadIdx.x] = 0;
            __syncthreads();
            const uint32_t prefix = sPrefix;
            for (uint32_t t = threadIdx.x; t < nT; t += 256) {
                if ((int) sc[t] != cut || !passes(t, cut)) continue;
                const uint32_t key = tKeys ? tKeys[t] : t;
                if (shift < 24 && (key >> (shift + 8)) != (prefix >> (shift + 8))) continue;
                atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t need = sNeed, b = 0;
                for (; b < 255; b++) {
                    if (hist[b] >= need) break;
                    need -= hist[b];
                }
                sNeed = need;
                sPrefix = prefix | (b << shift);
            }
            __syncthreads();
        }
        keyMax = sPrefix;   // the key of the last kept target with the cut score
    }
    sd_hit *o = out + (size_t) row * maxHits;
    for (uint32_t t = threadIdx.x; t < nT; t += 256) {
        const int s = sc[t];
        if (s < cut || !passes(t, s)) continue;
        if (s == cut && (tKeys ? tKeys[t] : t) > keyMax) continue;
        const uint32_t slot = atomicAdd(&sCount, 1u);
        if (slot < maxHits) {
            sd_hit h;
            h.seqId = t;
            h.score = s;
            h.diagonal = 0;
            h.pad = 0;
            o[slot] = h;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) outCount[row] = min(sCount, maxHits);
}

// Scores of the queries [q0, q1) against every target into the workspace `dScores` (row stride `rowStride` bytes).
int ugScanRange(sd_ctx *ctx, const int8_t *dMat, int matMin, const sd_seqset *queries, const sd_seqset *targets, uint32_t q0, uint32_t q1,
                uint8_t *dScores, uint64_t rowStride, uint32_t maxTLen) {
    const uint32_t nq = q1 - q0, nT = targets->n;
    // classes by query length: 128, 256, 512 rows per strip; longer queries take several strips of 512
    std::vector<uint32_t> rows[4];
    std::vector<int32_t> cap(nq);
    for (uint32_t i = 0; i < nq; i++) {
        const uint64_t len = queries->hOff[q0 + i + 1] - queries->hOff[q0 + i];
        cap[i] = 255 - (std::abs(matMin) + std::abs(queries->hMinBias[q0 + i]));   // ssw_init's bias
        if (len == 0) continue;   // (its row stays 0)
        rows[len <= 128 ? 0 : (len <= 256 ? 1 : (len <= 512 ? 2 : 3))].push_back(i);
    }
    uint32_t *dRows = nullptr;
    int32_t *dCap = nullptr;
    SD_HIP(ctx, wsGet(ctx, "ug.rows", (size_t) nq, &dRows));
    SD_HIP(ctx, wsGet(ctx, "ug.cap", (size_t) nq, &dCap));
    SD_HIP(ctx, hipMemcpyAsync(dCap, cap.data(), (size_t) nq * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemsetAsync(dScores, 0, (size_t) nq * rowStride, ctx->stream));
    std::vector<uint32_t> flat;
    for (int c = 0; c < 4; c++) flat.insert(flat.end(), rows[c].begin(), rows[c].end());
    if (!flat.empty()) SD_HIP(ctx, hipMemcpyAsync(dRows, flat.data(), flat.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));   // (cap / flat are locals of this call)
    const uint32_t groups = (nT + UG_WAVES - 1) / UG_WAVES;
    const uint32_t gx = std::max(1u, std::min(1024u, (groups + 15) / 16));
    size_t at = 0;
    for (int c = 0; c < 4; c++) {
        const uint32_t n = (uint32_t) rows[c].size();
        if (n == 0) continue;
        ProfScope ps(ctx, "ungapped_scan");
        if (c < 3) {
            for (uint32_t y0 = 0; y0 < n; y0 += 65535) {
                const dim3 grid(gx, std::min(65535u, n - y0));
                const uint32_t *r = dRows + at + y0;
#define UG_LAUNCH(RT_)                                                                                                                       \
    hipLaunchKernelGGL((ungapped_scan_kernel<RT_, false>), grid, dim3(64 * UG_WAVES), 0, ctx->stream, r, q0, queries->dRes, queries->dBias,    \
                       queries->dOff, dCap, targets->dRes, targets->dOff, nT, dMat, dScores, rowStride, (uint32_t *) nullptr, 0u)
                if (c == 0) UG_LAUNCH(2);
                else if (c == 1) UG_LAUNCH(4);
                else UG_LAUNCH(8);
#undef UG_LAUNCH
            }
        } else {
            // boundary lines: two of lineLen dwords per wavefront; the launches are cut so that they stay within 256 MB
            const uint32_t lineLen = (maxTLen + 63) & ~63u;
            // workgroups along the targets: about 2 048 in a launch when the long queries are few (one 65 535-residue query still
            // fills the device), at least 32, and no more than leave a query's lines within the budget
            const uint32_t want = std::max(32u, (2048u + n - 1) / n);
            const uint32_t fit = (uint32_t) std::max<size_t>(1, ((size_t) 64 << 20) / ((size_t) UG_WAVES * 2 * lineLen));
            const uint32_t gxm = std::max(1u, std::min(std::min(want, fit), groups));
            const size_t perRow = (size_t) gxm * UG_WAVES * 2 * lineLen;   // dwords
            const uint32_t rowsPer = (uint32_t) std::max<size_t>(1, std::min<size_t>(4096, ((size_t) 64 << 20) / perRow));
            uint32_t *dLines = nullptr;
            SD_HIP(ctx, wsGet(ctx, "ug.boundary", perRow * std::min(rowsPer, n), &dLines));
            for (uint32_t y0 = 0; y0 < n; y0 += rowsPer) {
                const dim3 grid(gxm, std::min(rowsPer, n - y0));
                hipLaunchKernelGGL((ungapped_scan_kernel<8, true>), grid, dim3(64 * UG_WAVES), 0, ctx->stream, dRows + at + y0, q0, queries->dRes,
                                   queries->dBias, queries->dOff, dCap, targets->dRes, targets->dOff, nT, dMat, dScores, rowStride, dLines, lineLen);
            }
        }
        SD_HIP(ctx, hipGetLastError());
        at += n;
    }
    return SD_OK;
}

int ugCheckSets(sd_ctx *ctx, const sd_seqset *queries, const sd_seqset *targets) {
    if (queries->dProf || targets->dProf) return sdFail(ctx, SD_EUNSUPPORTED, "the ungapped scan takes sequence sets (profile sets are not implemented)");
    return SD_OK;   // (sd_seqset_create admits no sequence above 65 535 residues)
}

uint32_t ugMaxLen(const sd_seqset *s) {
    uint64_t m = 1;
    for (uint32_t i = 0; i < s->n; i++) m = std::max<uint64_t>(m, s->hOff[i + 1] - s->hOff[i]);
    return (uint32_t) m;
}

int ugMatrix(sd_ctx *ctx, const int8_t *matrix, int8_t **dMat, int *matMin) {
    SD_HIP(ctx, wsGet(ctx, "ug.matrix", (size_t) 448, dMat));
    SD_HIP(ctx, hipMemcpyAsync(*dMat, matrix, 441, hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    int m = 0;
    for (int i = 0; i < 441; i++) m = std::min(m, (int) matrix[i]);
    *matMin = m;
    return SD_OK;
}

}  // namespace

extern "C" {

int sd_ungapped_last_cells(sd_ctx *ctx, uint64_t *cells) {
    if (!ctx || !cells) return SD_EINVAL;
    *cells = ctx->cellsUngapped;
    return SD_OK;
}

int sd_ungapped_score_matrix(sd_ctx *ctx, const int8_t *matrix, const sd_seqset *queries, const sd_seqset *targets, uint8_t *out) {
    if (!ctx || !matrix || !queries || !targets || !out) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    ctx->cellsUngapped = 0;
    if (int rc = ugCheckSets(ctx, queries, targets)) return rc;
    if (queries->n == 0 || targets->n == 0) return SD_OK;
    int8_t *dMat = nullptr;
    int matMin = 0;
    if (int rc = ugMatrix(ctx, matrix, &dMat, &matMin)) return rc;
    const uint32_t nT = targets->n, maxT = ugMaxLen(targets);
    const uint64_t stride = ((uint64_t) nT + 3) & ~(uint64_t) 3;
    const uint32_t sub = (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>(65535, ((uint64_t) 1 << 30) / stride));
    for (uint32_t q0 = 0; q0 < queries->n; q0 += sub) {
        const uint32_t q1 = std::min(queries->n, q0 + sub);
        uint8_t *dScores = nullptr;
        SD_HIP(ctx, wsGet(ctx, "ug.scores", (size_t) (q1 - q0) * stride, &dScores));
        if (int rc = ugScanRange(ctx, dMat, matMin, queries, targets, q0, q1, dScores, stride, maxT)) return rc;
        SD_HIP(ctx, hipMemcpy2DAsync(out + (size_t) q0 * nT, nT, dScores, stride, nT, q1 - q0, hipMemcpyDeviceToHost, ctx->stream));
        SD_HIP(ctx, sdStreamSync(ctx));
    }
    ctx->cellsUngapped = queries->total * targets->total;
    return SD_OK;
}

int sd_ungapped_prefilter_batch(sd_ctx *ctx, const sd_ungapped_params *par, const sd_seqset *queries, const sd_seqset *targets,
                                const uint32_t *targetKeys, const uint32_t *identityId, sd_hit *outHits, uint32_t *outCount) {
    if (!ctx || !par || !queries || !targets || !outHits || !outCount) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    ctx->cellsUngapped = 0;
    if (par->maxHitsPerQuery < 1) return sdFail(ctx, SD_EINVAL, "maxHitsPerQuery must be >= 1");
    if (int rc = ugCheckSets(ctx, queries, targets)) return rc;
    const uint32_t nQ = queries->n, nT = targets->n, W = (uint32_t) par->maxHitsPerQuery;
    for (uint32_t i = 0; i < nQ; i++) outCount[i] = 0;
    if (nQ == 0 || nT == 0) return SD_OK;
    if (identityId)
        for (uint32_t i = 0; i < nQ; i++)
            if (identityId[i] != UINT32_MAX && identityId[i] >= nT) return sdFail(ctx, SD_EINVAL, "identityId[%u] out of range", i);
    int8_t *dMat = nullptr;
    int matMin = 0;
    if (int rc = ugMatrix(ctx, par->matrix, &dMat, &matMin)) return rc;
    const uint32_t maxT = ugMaxLen(targets);
    // what the select kernel reads of the targets: lengths and (optionally) DB keys
    std::vector<uint32_t> tLen(nT);
    for (uint32_t i = 0; i < nT; i++) tLen[i] = (uint32_t) (targets->hOff[i + 1] - targets->hOff[i]);
    uint32_t *dTLen = nullptr, *dKeys = nullptr, *dIdent = nullptr, *dCount = nullptr;
    SD_HIP(ctx, wsGet(ctx, "ug.tlen", (size_t) nT, &dTLen));
    SD_HIP(ctx, hipMemcpyAsync(dTLen, tLen.data(), (size_t) nT * 4, hipMemcpyHostToDevice, ctx->stream));
    if (targetKeys) {
        SD_HIP(ctx, wsGet(ctx, "ug.tkeys", (size_t) nT, &dKeys));
        SD_HIP(ctx, hipMemcpyAsync(dKeys, targetKeys, (size_t) nT * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (identityId) {
        SD_HIP(ctx, wsGet(ctx, "ug.ident", (size_t) nQ, &dIdent));
        SD_HIP(ctx, hipMemcpyAsync(dIdent, identityId, (size_t) nQ * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    SD_HIP(ctx, sdStreamSync(ctx));
    // queries per pass: their rows of scores (nT bytes each) stay within 1 GB of workspace and never leave the device
    const uint64_t stride = ((uint64_t) nT + 3) & ~(uint64_t) 3;
    const uint32_t sub = (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>(65535, ((uint64_t) 1 << 30) / stride));
    sd_hit *dHits = nullptr;
    SD_HIP(ctx, wsGet(ctx, "ug.hits", (size_t) std::min(sub, nQ) * W, &dHits));
    SD_HIP(ctx, wsGet(ctx, "ug.count", (size_t) std::min(sub, nQ), &dCount));
    for (uint32_t q0 = 0; q0 < nQ; q0 += sub) {
        const uint32_t q1 = std::min(nQ, q0 + sub), nq = q1 - q0;
        uint8_t *dScores = nullptr;
        SD_HIP(ctx, wsGet(ctx, "ug.scores", (size_t) nq * stride, &dScores));
        if (int rc = ugScanRange(ctx, dMat, matMin, queries, targets, q0, q1, dScores, stride, maxT)) return rc;
        {
            ProfScope ps(ctx, "ungapped_select");
            hipLaunchKernelGGL(ungapped_select_kernel, dim3(nq), dim3(256), 0, ctx->stream, dScores, stride, nT, q0, queries->dOff, dTLen, dKeys,
                               dIdent, par->covMode, par->covThr, par->minScore, W, dHits, dCount);
            SD_HIP(ctx, hipGetLastError());
        }
        SD_HIP(ctx, hipMemcpyAsync(outCount + q0, dCount, (size_t) nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        SD_HIP(ctx, hipMemcpyAsync(outHits + (size_t) q0 * W, dHits, (size_t) nq * W * sizeof(sd_hit), hipMemcpyDeviceToHost, ctx->stream));
        SD_HIP(ctx, sdStreamSync(ctx));
    }
    // hit_t::compareHitsByScoreAndId: score descending, then target key ascending
#pragma omp parallel for schedule(dynamic, 64)
    for (uint32_t i = 0; i < nQ; i++) {
        sd_hit *r = outHits + (size_t) i * W;
        std::sort(r, r + outCount[i], [targetKeys](const sd_hit &a, const sd_hit &b) {
            if (a.score != b.score) return a.score > b.score;
            return (targetKeys ? targetKeys[a.seqId] : a.seqId) < (targetKeys ? targetKeys[b.seqId] : b.seqId);
        });
    }
    ctx->cellsUngapped = queries->total * targets->total;
    return SD_OK;
}

}  // extern "C"
