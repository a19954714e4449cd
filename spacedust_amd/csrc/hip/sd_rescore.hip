// Rescoring of prefilter hits along their own diagonal (`rescorediagonal`, `search --alignment-mode 4`):
// DistanceCalculator::computeUngappedAlignment -> ungappedAlignmentByDiagonal (M/src/alignment/DistanceCalculator.h:94-201,276-295)
// for a batch of (query, target, 16-bit diagonal) hits, bit for bit, plus the identity count of rescorediagonal.cpp:284-291.
//
// Layout.  One wavefront owns one hit and walks that hit's candidate diagonals in the reference's order, so the
// "strictly greater replaces" rule between candidates is a wave-uniform compare and needs no merge between wavefronts (of the
// 2 + tLen / 32768 candidates at most two overlap the sequences at all: the others cost a compare).  A workgroup holds four
// wavefronts and walks the hit list with a grid stride, so the letter -> matrix-row table is built in LDS once per workgroup
// and serves many hits.  A diagonal is cut into chunks of 256 positions; lane l takes positions 4 l .. 4 l + 3 of the chunk from
// one dword per side.  The two sides start at unrelated byte addresses, so each side is read as two aligned dwords and put
// together with v_alignbyte_b32.  The recurrence
//     s = s + c;  if (s <= 0) { s = 0; minPos = pos; }  if (s > max) { max = s; end = pos; start = minPos + 1; }
// is a scan: with the inclusive prefix sums P (P[-1] = 0), s[pos] = P[pos] - min_{-1 <= k <= pos} P[k]; "s <= 0" holds exactly
// where pos attains that running minimum, so minPos is the LATEST index attaining it, and "s > max" keeps the EARLIEST position
// of the global maximum.  Per chunk: a prefix sum and a prefix (min, latest index) over the wavefront, moved by DPP (row shifts and
// row broadcasts, no LDS traffic), and a reduction (max, earliest index); the carries (sum, min, index, best) are wave-uniform
// between chunks.
#include "sd_common.h"

namespace {

constexpr int RS_WAVES = 4;          // wavefronts (= hits in flight) per workgroup
constexpr int RS_CHUNK = 256;        // positions per wavefront step: 64 lanes x 4 bytes
constexpr size_t RS_PAD = 64;        // bytes behind the letters: the aligned dword pairs read up to 7 bytes past a diagonal's end

// DPP moves of the scans: a shift inside each row of 16 lanes, the last lane of a row broadcast to the next row (row_bcast:15, rows 1
// and 3) and lane 31 to the upper half (row_bcast:31, rows 2 and 3).  bound_ctrl is off: a lane without a source keeps `ident`.
template <int N>
__device__ __forceinline__ int rsRowShr(int v, int ident) {
    return __builtin_amdgcn_update_dpp(ident, v, 0x110 + N, 0xf, 0xf, false);
}
__device__ __forceinline__ int rsBcast15(int v, int ident) { return __builtin_amdgcn_update_dpp(ident, v, 0x142, 0xa, 0xf, false); }
__device__ __forceinline__ int rsBcast31(int v, int ident) { return __builtin_amdgcn_update_dpp(ident, v, 0x143, 0xc, 0xf, false); }
// lane l - 1 of the wavefront (wave_shr:1); lane 0 keeps `first`
__device__ __forceinline__ int rsWaveShr1(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ int rsPrefixSum(int v) {
    v += rsRowShr<1>(v, 0);
    v += rsRowShr<2>(v, 0);
    v += rsRowShr<4>(v, 0);
    v += rsRowShr<8>(v, 0);
    v += rsBcast15(v, 0);
    v += rsBcast31(v, 0);
    return v;
}

// (earlier, later) -> the later element where it is not larger: the latest index of the minimum
#define RS_MIN_STEP(MOVE)                                         \
    {                                                             \
        const int ov = MOVE(m, INT32_MAX);                        \
        const int oi = MOVE(mi, 0);                               \
        if (!(m <= ov)) {                                         \
            m = ov;                                               \
            mi = oi;                                              \
        }                                                         \
    }

__device__ __forceinline__ int rsWaveSum(int v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// four letters of one side at byte offset `off` (any alignment) of the letters `base` (a device allocation: dword aligned): two
// aligned dwords, realigned.  The dword index is formed on the kernel argument itself, so the loads stay global loads.
__device__ __forceinline__ uint32_t rsLoad4(const uint8_t *__restrict__ base, uint64_t off) {
    const uint32_t *w = (const uint32_t *) __builtin_assume_aligned(base, 4) + (off >> 2);
    const uint32_t lo = w[0], hi = w[1];
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t) off & 3u);
}

struct RsBest {
    int score, start, end, diagLen, dist, diag;
};

// mode: 0 inverse Hamming, 1 substitution score, 2 substitution score with start / end
__global__ __launch_bounds__(64 * RS_WAVES) void rescore_diagonal_kernel(
    const uint8_t *__restrict__ qLet, const uint64_t *__restrict__ qOff, const uint8_t *__restrict__ tLet,
    const uint64_t *__restrict__ tOff, const int8_t *__restrict__ matrix, const uint8_t *__restrict__ aa2num, uint32_t nHits,
    const uint32_t *__restrict__ hitQ, const uint32_t *__restrict__ hitT, const uint16_t *__restrict__ hitDiag, int mode,
    sd_rescore_result *__restrict__ out) {
    __shared__ int8_t sMat[448];
    __shared__ uint16_t sRow[256];   // letter -> 21 * matrix code
    __shared__ uint8_t sCol[256];    // letter -> matrix code
    for (int i = threadIdx.x; i < 441; i += blockDim.x) sMat[i] = matrix[i];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        const uint8_t c = aa2num[i];
        sCol[i] = c;
        sRow[i] = (uint16_t) (c * 21);
    }
    __syncthreads();
    // (the wavefront index and everything read per hit are wave-uniform: scalar registers, uniform loops around the DPP moves)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t hit = blockIdx.x * RS_WAVES + wave; hit < nHits; hit += gridDim.x * RS_WAVES) {
        const uint32_t q = hitQ[hit], t = hitT[hit];
        const int d16 = (int) hitDiag[hit];
        const uint64_t q0 = qOff[q], t0 = tOff[t];
        const int qLen = (int) (qOff[q + 1] - q0), tLen = (int) (tOff[t + 1] - t0);
        RsBest best = {0, -1, -1, 0, 0, 0};
        uint64_t bq = 0, bt = 0;   // offsets of the winner's first letters (identity count)
        const int nNeg = 1 + tLen / 32768, nPos = qLen / 65536;
        for (int cand = 0; cand < nNeg + nPos + 1; cand++) {
            const int diag = cand < nNeg ? d16 - 65536 * (cand + 1) : d16 + 65536 * (cand - nNeg);
            const int dist = diag < 0 ? -diag : diag;
            int len;
            uint64_t pq, pt;   // offsets of the diagonal's first letters in qLet / tLet
            if (diag >= 0 && dist < qLen) {
                len = min(tLen, qLen - dist);
                pq = q0 + dist;
                pt = t0;
            } else if (diag < 0 && dist < tLen) {
                len = min(tLen - dist, qLen);
                pq = q0;
                pt = t0 + dist;
            } else {
                continue;
            }
            int cScore = 0, cStart = -1, cEnd = -1;
            if (mode == 0) {
                int cnt = 0;
                for (int b = 0; b < len; b += RS_CHUNK) {
                    const int p0 = b + 4 * lane;
                    if (p0 < len) {
                        const uint32_t a = rsLoad4(qLet, pq + p0), c = rsLoad4(tLet, pt + p0);
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            cnt += (p0 + j < len && ((a >> (8 * j)) & 0xff) == ((c >> (8 * j)) & 0xff)) ? 1 : 0;
                    }
                }
                cScore = __builtin_amdgcn_readfirstlane(rsWaveSum(cnt));
            } else {
                int pCarry = 0, mCarry = 0, iCarry = -1;     // P[-1] = 0 at index -1
                unsigned long long bestKey = 0;               // score << 40 | (0xFFFFF - end) << 20 | start
                for (int b = 0; b < len; b += RS_CHUNK) {
                    const int p0 = b + 4 * lane;
                    int c[4] = {0, 0, 0, 0};
                    if (p0 < len) {
                        const uint32_t a = rsLoad4(qLet, pq + p0), w = rsLoad4(tLet, pt + p0);
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            if (p0 + j < len) c[j] = sMat[sRow[(a >> (8 * j)) & 0xff] + sCol[(w >> (8 * j)) & 0xff]];
                    }
                    const int t1 = c[0] + c[1], t2 = t1 + c[2], t3 = t2 + c[3];
                    const int incl = rsPrefixSum(t3);
                    const int base = pCarry + incl - t3;
                    const int P[4] = {base + c[0], base + t1, base + t2, base + t3};
                    // the lane's own (minimum, latest index); lanes past the end hold the identity
                    int m = INT32_MAX, mi = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (p0 + j < len && P[j] <= m) {
                            m = P[j];
                            mi = p0 + j;
                        }
                    if (lane == 0 && !(m <= mCarry)) {   // the carry stands in front of lane 0
                        m = mCarry;
                        mi = iCarry;
                    }
                    RS_MIN_STEP(rsRowShr<1>)
                    RS_MIN_STEP(rsRowShr<2>)
                    RS_MIN_STEP(rsRowShr<4>)
                    RS_MIN_STEP(rsRowShr<8>)
                    RS_MIN_STEP(rsBcast15)
                    RS_MIN_STEP(rsBcast31)
                    // exclusive: what stands in front of this lane (the carry in front of lane 0)
                    int xm = rsWaveShr1(m, mCarry), xi = rsWaveShr1(mi, iCarry);
                    int ls = 0, le = 0, lst = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (p0 + j < len) {
                            if (P[j] <= xm) {
                                xm = P[j];
                                xi = p0 + j;
                            }
                            const int s = P[j] - xm;
                            if (s > ls) {
                                ls = s;
                                le = p0 + j;
                                lst = xi + 1;
                            }
                        }
                    // (largest score, earliest end) of the chunk; a later chunk replaces only with a strictly greater score
                    unsigned long long key = ((unsigned long long) (uint32_t) ls << 40) | ((unsigned long long) (0xFFFFFu - (uint32_t) le) << 20) |
                                             (unsigned long long) (uint32_t) lst;
                    for (int off = 32; off >= 1; off >>= 1) {
                        const unsigned long long o = __shfl_xor(key, off, 64);
                        key = o > key ? o : key;
                    }
                    if ((key >> 40) > (bestKey >> 40)) bestKey = key;
                    pCarry += __builtin_amdgcn_readlane(incl, 63);
                    mCarry = __builtin_amdgcn_readlane(m, 63);
                    iCarry = __builtin_amdgcn_readlane(mi, 63);
                }
                bestKey = ((unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int) (bestKey >> 32)) << 32) |
                          (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) bestKey);
                cScore = (int) (bestKey >> 40);
                if (mode == 2) {   // computeSubstitutionStartEndDistance leaves (0, 0) where nothing scores
                    cEnd = cScore > 0 ? (int) (0xFFFFFu - (uint32_t) ((bestKey >> 20) & 0xFFFFFu)) : 0;
                    cStart = cScore > 0 ? (int) (bestKey & 0xFFFFFu) : 0;
                }
            }
            if (cScore > best.score) {
                best = {cScore, cStart, cEnd, len, dist, diag};
                bq = pq;
                bt = pt;
            }
        }
        // rescorediagonal.cpp:284-291: letters compared without their case bit over [start, end] of the winner
        int idCnt = mode == 0 ? best.score : 0;
        if (mode == 2 && best.score > 0) {
            int cnt = 0;
            for (int b = best.start; b <= best.end; b += RS_CHUNK) {
                const int p0 = b + 4 * lane;
                if (p0 <= best.end) {
                    const uint32_t a = rsLoad4(qLet, bq + p0) & 0xDFDFDFDFu, c = rsLoad4(tLet, bt + p0) & 0xDFDFDFDFu;
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        cnt += (p0 + j >= best.start && p0 + j <= best.end && ((a >> (8 * j)) & 0xff) == ((c >> (8 * j)) & 0xff)) ? 1 : 0;
                }
            }
            idCnt = rsWaveSum(cnt);
        }
        if (lane == 0) {
            sd_rescore_result r;
            r.score = best.score;
            r.startPos = best.start;
            r.endPos = best.end;
            r.diagonalLen = best.diagLen;
            r.distToDiagonal = best.dist;
            r.diagonal = best.diag;
            r.idCnt = idCnt;
            r.pad = 0;
            out[hit] = r;
        }
    }
}

}  // namespace

extern "C" {

int sd_seqset_set_letters(sd_seqset *s, const char *letters) {
    if (!s || !letters) return SD_EINVAL;
    sd_ctx *ctx = s->ctx;
    (void) hipSetDevice(ctx->device);
    if (!s->dLet && poolGet(ctx, (size_t) s->total + RS_PAD, (void **) &s->dLet, &s->bLet) != hipSuccess) {
        (void) hipGetLastError();
        s->dLet = nullptr;
        return sdFail(ctx, SD_ENOMEM, "sd_seqset_set_letters: device allocation of %llu bytes failed", (unsigned long long) s->total);
    }
    SD_HIP(ctx, hipMemsetAsync(s->dLet + s->total, 0, RS_PAD, ctx->stream));
    if (s->total) SD_HIP(ctx, hipMemcpyAsync(s->dLet, letters, (size_t) s->total, hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    return SD_OK;
}

int sd_rescore_diagonal_batch(sd_ctx *ctx, const sd_rescore_params *par, const sd_seqset *queries, const sd_seqset *targets,
                              uint32_t nHits, const uint32_t *hitQuery, const uint32_t *hitTarget, const uint16_t *hitDiagonal,
                              sd_rescore_result *out) {
    if (!ctx || !par || !queries || !targets) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    if (queries->dProf || targets->dProf)
        return sdFail(ctx, SD_EUNSUPPORTED, "sd_rescore_diagonal_batch takes sequence sets (profile sets are not implemented)");
    if (par->mode < 0 || par->mode > 2)
        return sdFail(ctx, SD_EUNSUPPORTED, "rescore mode %d: 0 (Hamming), 1 (substitution) and 2 (alignment) are implemented", par->mode);
    if (!queries->dLet || !targets->dLet)
        return sdFail(ctx, SD_EINVAL, "sd_rescore_diagonal_batch: a set carries no letters (sd_seqset_set_letters)");
    if (nHits == 0) return SD_OK;
    if (!hitQuery || !hitTarget || !hitDiagonal || !out) return SD_EINVAL;
    for (uint32_t i = 0; i < nHits; i++)
        if (hitQuery[i] >= queries->n || hitTarget[i] >= targets->n)
            return sdFail(ctx, SD_EINVAL, "sd_rescore_diagonal_batch: hit %u names sequence (%u, %u) of (%u, %u)", i, hitQuery[i], hitTarget[i],
                          queries->n, targets->n);
    for (int i = 0; i < 256; i++)
        if (par->aa2num[i] > 20) return sdFail(ctx, SD_EINVAL, "sd_rescore_diagonal_batch: aa2num[%d] = %d is no matrix code", i, (int) par->aa2num[i]);
    int8_t *dTab = nullptr;   // matrix (448 bytes) followed by the letter map
    uint32_t *dQ = nullptr, *dT = nullptr;
    uint16_t *dD = nullptr;
    sd_rescore_result *dOut = nullptr;
    SD_HIP(ctx, wsGet(ctx, "rs.tables", (size_t) 448 + 256, &dTab));
    SD_HIP(ctx, wsGet(ctx, "rs.hitq", (size_t) nHits, &dQ));
    SD_HIP(ctx, wsGet(ctx, "rs.hitt", (size_t) nHits, &dT));
    SD_HIP(ctx, wsGet(ctx, "rs.hitd", (size_t) nHits, &dD));
    SD_HIP(ctx, wsGet(ctx, "rs.out", (size_t) nHits, &dOut));
    SD_HIP(ctx, hipMemcpyAsync(dTab, par->matrix, 441, hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemcpyAsync(dTab + 448, par->aa2num, 256, hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemcpyAsync(dQ, hitQuery, (size_t) nHits * 4, hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemcpyAsync(dT, hitTarget, (size_t) nHits * 4, hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemcpyAsync(dD, hitDiagonal, (size_t) nHits * 2, hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "rescore_diagonal");
        // eight workgroups per compute unit walk the list with a grid stride
        const uint32_t want = (nHits + RS_WAVES - 1) / RS_WAVES;
        const uint32_t grid = std::max(1u, std::min(want, (uint32_t) std::max(1, ctx->prop.multiProcessorCount) * 8u));
        hipLaunchKernelGGL(rescore_diagonal_kernel, dim3(grid), dim3(64 * RS_WAVES), 0, ctx->stream, queries->dLet, queries->dOff, targets->dLet,
                           targets->dOff, dTab, (const uint8_t *) (dTab + 448), nHits, dQ, dT, dD, (int) par->mode, dOut);
        SD_HIP(ctx, hipGetLastError());
    }
    SD_HIP(ctx, hipMemcpyAsync(out, dOut, (size_t) nHits * sizeof(sd_rescore_result), hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    return SD_OK;
}

}  // extern "C"
