// Smith-Waterman on gfx950: score/end pass, start-position (reverse) pass and banded traceback.
//
// Semantics are those of the reference's striped SSE/AVX2 kernels, restated in scalar form in
// oracle/sd_oracle.cpp (swPass) and derived in DESIGN.md:
//     Hpre(q) = max(0, G[c-1][q-1] + P, E[q], Fl)        Fl: vertical gap opened inside the same SIMD segment
//     G(q)    = max(Hpre(q), Ff)                          Ff: exact vertical gap (what the lazy-F loop produces)
//     E'(q)   = max(E[q]-ge, Hpre(q)-go, 0)               E is opened from Hpre, NOT from G
//     Fl'     = max(Fl-ge, Hpre(q)-go, 0)  (reset to 0 where q % segLen == 0),  Ff' = max(Ff-ge, G(q)-go, 0)
// (M/src/alignment/StripedSmithWaterman.cpp:713-871 byte kernel, :1013-1149 word kernel).
// Fl is carried by the int32 kernel of this file (sw_score_kernel: every call with go < ge, SD_SW_INT32=1, tasks beyond the
// int16 range, and sd_sw_score_batch) only.  The packed kernels of sd_sw_pk.h, which run everything else, evaluate
// Hpre = max(0, G[c-1][q-1] + P, E[q]) without it: for go >= ge, G is the same in every cell (see there).
//
// Mapping to CDNA4: integer DP, no MFMA.  A task (one pair, one pass) is owned by a 32-lane half
// wavefront; lane l holds RT consecutive query rows in VGPRs and the half-wave sweeps the target as a
// systolic array (lane l works on column k-l at step k), handing (G, Ff, residue -- and Fl in the int32 kernel) of its
// last row to lane l+1 each step.  The per-task query profile (int8 [21][32*RT]) lives in LDS and is the only
// indexed operand; every lane reads only its own RT bytes of the row selected by its current target
// residue.  HBM traffic is the two residue streams (algorithmic bytes qLen + tLen per task), so the
// kernel is VALU bound; bench.py reports it in GCUPS.
#include "sd_common.h"
#include <unistd.h>


#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <omp.h>
#include <numeric>

#include "../host/sd_host.h"
#include "sd_sw_pk.h"

namespace {

using sdpk::SwTask;
using sdpk::NARROW_EXACT;

template <int RT>
__global__ void __launch_bounds__(64)
sw_score_kernel(const SwTask *__restrict__ tasks, uint32_t nTasks, const uint8_t *__restrict__ qRes,
                const int8_t *__restrict__ qBias, const uint8_t *__restrict__ tRes, const int8_t *__restrict__ mat,
                int go, int ge, int32_t *__restrict__ out, uint2 *__restrict__ boundary,
                const uint32_t *__restrict__ order /* nullable: task = tasks[order[x]] */,
                const int8_t *__restrict__ qProf /* nullable: profile queries, int8 [position][21] */) {
    constexpr int ROWS = 32 * RT;          // rows per strip
    constexpr int WORDS = RT / 4;          // profile dwords per lane per residue
    __shared__ uint32_t prof[2][21][ROWS / 4];
    __shared__ int8_t smat[441];
    for (int i = threadIdx.x; i < 441; i += 64) smat[i] = mat[i];
    __syncthreads();

    const int grp = threadIdx.x >> 5;
    const int l = threadIdx.x & 31;
    const uint32_t taskId = blockIdx.x * 2 + grp;
    SwTask tk;
    if (taskId < nTasks) {
        tk = tasks[order ? order[taskId] : taskId];
    } else {
        tk.n = 0; tk.tL = 0; tk.qOff = 0; tk.tOff = 0; tk.qStep = 1; tk.tStep = 1; tk.segLen = 1; tk.slot = 0; tk.boundOff = 0;
    }
    const int n = tk.n, tL = tk.tL;
    const int nStrips = (n + ROWS - 1) / ROWS;

    int bestVal = 0, bestCol = -1, bestRow = 0;

    for (int strip = 0; strip < nStrips; strip++) {
        const int q0 = strip * ROWS + l * RT;
        // ---- build this lane's slice of the query profile (SmithWaterman::createQueryProfile, :163-187)
        uint32_t segMask = 0;
        {
            int8_t *pb = (int8_t *) &prof[grp][0][0];
#pragma unroll
            for (int r = 0; r < RT; r++) {
                const int qi = q0 + r;
                const bool valid = qi < n;
                int res = 20, cb = 0;
                int64_t pidx = 0;
                if (valid) {
                    const int64_t idx = (int64_t) tk.qOff + (int64_t) qi * tk.qStep;
                    res = qRes[idx];
                    cb = qBias[idx];
                    pidx = idx * 21;
                }
                if (valid && (qi % tk.segLen) == 0) segMask |= (1u << r);
                if (qProf) {
#pragma unroll
                    for (int a = 0; a < 21; a++) pb[a * ROWS + l * RT + r] = (int8_t) (valid ? (int) qProf[pidx + a] : -64);
                } else {
#pragma unroll
                    for (int a = 0; a < 21; a++) {
                        int v = valid ? (int) smat[a * 21 + res] + cb : -64;
                        pb[a * ROWS + l * RT + r] = (int8_t) v;
                    }
                }
            }
        }
        int H[RT], E[RT];
#pragma unroll
        for (int r = 0; r < RT; r++) {
            H[r] = 0;
            E[r] = 0;
        }
        int outG = 0, outFf = 0, outFl = 0, curT = 20, prevInG = 0;
        const bool firstStrip = (strip == 0);
        const bool lastStrip = (strip == nStrips - 1);
        uint2 *bnd = boundary + tk.boundOff;
        if (!firstStrip) __threadfence();   // boundary values of the previous strip must be visible
        const int steps = (n > 0 && tL > 0) ? tL + 31 : 0;
        for (int k = 0; k < steps; k++) {
            const int c = k - l;
            int inG = __shfl_up(outG, 1, 32);
            int inFf = __shfl_up(outFf, 1, 32);
            int inFl = __shfl_up(outFl, 1, 32);
            int inT = __shfl_up(curT, 1, 32);
            const bool active = (c >= 0) && (c < tL);
            if (l == 0) {
                inG = 0; inFf = 0; inFl = 0;
                if (active) {
                    inT = tRes[(int64_t) tk.tOff + (int64_t) c * tk.tStep];
                    if (!firstStrip) {
                        unsigned long long w = __hip_atomic_load((unsigned long long *) &bnd[c], __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_AGENT);
                        inG = (int) (w & 0xFFFFu);
                        inFf = (int) ((w >> 16) & 0xFFFFu);
                        inFl = (int) ((w >> 32) & 0xFFFFu);
                    }
                }
            }
            if (active) {
                curT = inT;
                int diag = (c == 0) ? 0 : prevInG;
                prevInG = inG;
                int Fl = inFl, Ff = inFf;
                uint32_t pw[WORDS];
#pragma unroll
                for (int w = 0; w < WORDS; w++) pw[w] = prof[grp][curT][l * WORDS + w];
                int cm = 0;
#pragma unroll
                for (int r = 0; r < RT; r++) {
                    const int s = (int) (int8_t) (pw[r >> 2] >> (8 * (r & 3)));
                    if (segMask & (1u << r)) Fl = 0;
                    const int old = H[r];
                    const int h = min(diag + s, 32767);   // simdi16_adds: the word kernel's H saturates (sw_sse2_word, :1069)
                    const int hpre = max(max(h, E[r]), Fl);
                    const int g = max(hpre, Ff);
                    const int open = hpre - go;
                    E[r] = max(max(E[r] - ge, open), 0);
                    Fl = max(max(Fl - ge, open), 0);
                    Ff = max(max(Ff - ge, g - go), 0);
                    H[r] = g;
                    diag = old;
                    cm = max(cm, (g << 5) | (31 - r));
                }
                outG = H[RT - 1];
                outFf = Ff;
                outFl = Fl;
                if (l == 31 && !lastStrip) {
                    unsigned long long w = (unsigned long long) (uint32_t) outG | ((unsigned long long) (uint32_t) outFf << 16) |
                                           ((unsigned long long) (uint32_t) outFl << 32);
                    __hip_atomic_store((unsigned long long *) &bnd[c], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                const int colVal = cm >> 5;
                if (colVal > bestVal) {
                    bestVal = colVal;
                    bestCol = c;
                    bestRow = q0 + 31 - (cm & 31);
                }
            }
        }
    }
    // ---- reduce over the 32 lanes: max value, then smallest column, then smallest row
    unsigned long long key = ((unsigned long long) (uint32_t) bestVal << 40) |
                             ((unsigned long long) (uint32_t) (0xFFFFF - (bestCol < 0 ? 0xFFFFF : bestCol)) << 20) |
                             (unsigned long long) (uint32_t) (0xFFFFF - bestRow);
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
        unsigned long long o = __shfl_xor(key, off, 32);
        key = o > key ? o : key;
    }
    if (l == 0 && taskId < nTasks) {
        const int v = (int) (key >> 40);
        const int col = 0xFFFFF - (int) ((key >> 20) & 0xFFFFF);
        const int row = 0xFFFFF - (int) (key & 0xFFFFF);
        out[3 * tk.slot + 0] = v;
        out[3 * tk.slot + 1] = (v == 0 || col == 0xFFFFF) ? -1 : col;
        out[3 * tk.slot + 2] = (v == 0) ? n - 1 : row;
    }
}

// ---------------------------------------------------------------------------------------------
// Banded traceback, one thread per alignment: SmithWaterman::banded_sw (StripedSmithWaterman.cpp:1348-1600)
// with its band-coordinate bookkeeping kept literally (what the band-edge cells hold decides ties).
// One launch evaluates one band width; the host doubles the band of the tasks whose maximum has not
// reached the alignment score (the reference's do/while, :1492-1493).
// ---------------------------------------------------------------------------------------------
struct TbTask {
    uint64_t qAbs;      // absolute index of query[qStart]
    uint64_t tAbs;      // absolute index of target[tStart]
    int32_t qLen, tLen; // sub-rectangle
    int32_t score;
    int32_t band;
    int32_t maxv;       // carried over band doublings
    uint32_t slot;
    uint64_t intOff;    // scratch: 3*(width+1) ints
    uint64_t dirOff;    // scratch: width_d*qLen*3 bytes
    uint64_t btOff;     // output (reversed while walking, fixed up at the end)
};

// Wave-parallel form: a 32-lane half wavefront owns one alignment.  The three band arrays (h_b, e_b, h_c)
// live in LDS and are indexed exactly like the reference's; a row is processed 32 band cells at a time.
// The only loop-carried dependence inside a row is the horizontal gap f[j] = max(h_c[j-1]-go, f[j-1]-ge);
// with T = max(e1, diag) >= 0 it reduces to f[p] = max(-ge, max_{k<p}(T[k]-go+ge*(k+1))) - ge*p, i.e. an
// exclusive prefix maximum across lanes (cross-lane scan, carried between 32-cell chunks).  Directions are
// packed to one byte per cell (bit0 dirE==3, bit1 dirF==5, bits2-3: 0 diag / 1 take dirE / 2 take dirF) and
// written row-major (coalesced); lane 0 then walks the path.
// GLOBAL: bands beyond the LDS classes (2*band+3 > 2047: a gap of > 1 000 residues inside the alignment) keep the three
// band arrays in global scratch in front of the task's direction bytes; the lanes of the half wavefront exchange them
// through agent-scope accesses with a fence where the LDS version has a wave barrier.  Rare and slow by design --
// what matters is that the reference's do/while (band doubling, :1492-1493) has no width the device refuses.
template <bool GLOBAL> __device__ __forceinline__ int bandLd(const int32_t *p) {
    if constexpr (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool GLOBAL> __device__ __forceinline__ void bandSt(int32_t *p, int v) {
    if constexpr (GLOBAL) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
template <bool GLOBAL> __device__ __forceinline__ void bandSync() {
    if constexpr (GLOBAL) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __builtin_amdgcn_wave_barrier();
}
__host__ __device__ __forceinline__ uint64_t tbGlobalIntBytes(int band) { return ((uint64_t) 3 * (2 * (uint64_t) band + 4) * 4 + 15) & ~15ull; }

// DPP moves with compile-time control words (the traceback kernels' cross-lane traffic)
__device__ __forceinline__ int dppI(int oldv, int src, int ctrl, int rowMask) {
    switch (ctrl) {   // the control word must be a compile-time constant
        case 0x138: return __builtin_amdgcn_update_dpp(oldv, src, 0x138, 0xf, 0xf, false);   // wave_shr:1
        case 0x130: return __builtin_amdgcn_update_dpp(oldv, src, 0x130, 0xf, 0xf, false);   // wave_shl:1
        case 0x111: return __builtin_amdgcn_update_dpp(oldv, src, 0x111, 0xf, 0xf, false);   // row_shr:1
        case 0x112: return __builtin_amdgcn_update_dpp(oldv, src, 0x112, 0xf, 0xf, false);
        case 0x114: return __builtin_amdgcn_update_dpp(oldv, src, 0x114, 0xf, 0xf, false);
        case 0x118: return __builtin_amdgcn_update_dpp(oldv, src, 0x118, 0xf, 0xf, false);
        default: return __builtin_amdgcn_update_dpp(oldv, src, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    }
    (void) rowMask;
}

__device__ __forceinline__ int dppZ(int src, int ctrl) {   // lanes without a source read 0
    switch (ctrl) {
        case 0x138: return __builtin_amdgcn_update_dpp(0, src, 0x138, 0xf, 0xf, true);
        case 0x130: return __builtin_amdgcn_update_dpp(0, src, 0x130, 0xf, 0xf, true);
        case 0x111: return __builtin_amdgcn_update_dpp(0, src, 0x111, 0xf, 0xf, true);
        case 0x112: return __builtin_amdgcn_update_dpp(0, src, 0x112, 0xf, 0xf, true);
        case 0x114: return __builtin_amdgcn_update_dpp(0, src, 0x114, 0xf, 0xf, true);
        default: return __builtin_amdgcn_update_dpp(0, src, 0x118, 0xf, 0xf, true);
    }
}

template <bool PROF, bool GLOBAL = false>
__global__ void __launch_bounds__(64)
sw_traceback_kernel(TbTask *__restrict__ tasks, uint32_t nTasks, const uint8_t *__restrict__ qRes,
                    const int8_t *__restrict__ qBias, const uint8_t *__restrict__ tRes, const int8_t *__restrict__ mat,
                    int go, int ge, int ldsStride /* ints per array */, int8_t *__restrict__ dirs, char *__restrict__ bt,
                    int32_t *__restrict__ res /* per task: btLen (-2 = band too small, -1 = traceback error), identical */,
                    const uint32_t *__restrict__ order /* nullable */,
                    int maxWidthLoop /* 0: one attempt; else keep doubling the band inside the kernel while
                                        2*band+3 <= maxWidthLoop (scratch must be sized for that width) */,
                    const int8_t *__restrict__ qProf /* nullable: profile queries, int8 [position][21] */) {
    extern __shared__ int32_t lds[];
    __shared__ int8_t smat[441];
    for (int i = threadIdx.x; i < 441; i += 64) smat[i] = mat[i];
    __syncthreads();
    const int grp = threadIdx.x >> 5, l = threadIdx.x & 31;
    const uint32_t lid = blockIdx.x * 2 + grp;
    const bool have = lid < nTasks;
    const uint32_t id = have ? (order ? order[lid] : lid) : 0;
    TbTask tk;
    if (have) tk = tasks[id];
    else { tk.qLen = 0; tk.tLen = 0; tk.band = 1; tk.score = 0; tk.maxv = 0; tk.qAbs = 0; tk.tAbs = 0; tk.slot = 0; tk.dirOff = 0; tk.btOff = 0; }
    const int qLen = tk.qLen, tLen = tk.tLen;
    int band = tk.band;
    int32_t *h_b, *e_b, *h_c;
    int8_t *direction;
    if constexpr (GLOBAL) {   // one attempt at the task's band per launch: [3 x (width + 1) ints][direction bytes]
        const int stride = band * 2 + 4;
        h_b = reinterpret_cast<int32_t *>(dirs + tk.dirOff);
        e_b = h_b + stride;
        h_c = e_b + stride;
        direction = dirs + tk.dirOff + tbGlobalIntBytes(band);
    } else {
        h_b = lds + (size_t) grp * 3 * ldsStride;
        e_b = h_b + ldsStride;
        h_c = e_b + ldsStride;
        direction = dirs + tk.dirOff;
    }
    const uint8_t *q = qRes + tk.qAbs;
    const int8_t *cb = qBias + tk.qAbs;
    const uint8_t *t = tRes + tk.tAbs;
    int maxv = tk.maxv;
    int width, width_d;
  for (;;) {
    width = band * 2 + 3;
    width_d = band * 2 + 1;
    // (the idle half of an odd last wavefront owns no scratch: in the global class its stores would land in another task's arrays)
    for (int x = l; (have || !GLOBAL) && x <= width && x < ldsStride; x += 32) { bandSt<GLOBAL>(h_b + x, 0); bandSt<GLOBAL>(e_b + x, 0); bandSt<GLOBAL>(h_c + x, 0); }
    bandSync<GLOBAL>();
    // Operands of the substitution score two rows ahead, the score itself one row ahead: neither the global loads (query
    // letter, bias, target letter of the row's first 32 cells) nor the matrix / profile lookup sit on a row's critical path.
    auto rowClamp = [&](int r) -> int { return r < qLen ? r : qLen - 1; };
    auto loadT = [&](int r) -> int {   // target letter of cell l of row r's first chunk
        int jn = ((r - band) > 0 ? (r - band) : 0) + l;
        jn = jn >= tLen ? tLen - 1 : jn;
        jn = jn < 0 ? 0 : jn;
        return (int) t[jn];
    };
    auto scoreOf = [&](int r, int qv, int tv) -> int {   // (without the bias: an add right behind the read would wait for it at the row's top)
        if (PROF) return (int) qProf[(tk.qAbs + (uint64_t) r) * 21 + tv];
        return (int) smat[21 * qv + tv];
    };
    int qa = 0, cba = 0, qb = 0, cbb = 0, tb = 0, sNext = 0;
    if (have && qLen > 0 && tLen > 0) {
        qa = q[0];
        cba = PROF ? 0 : cb[0];
        sNext = scoreOf(0, qa, loadT(0));
        const int r1 = rowClamp(1);
        qb = q[r1];
        cbb = PROF ? 0 : cb[r1];
        tb = loadT(r1);
    }
    for (int i = 0; i < qLen; i++) {
        int beg = 0, end = tLen - 1;
        int jj = i - band; beg = beg > jj ? beg : jj;
        jj = i + band; end = end < jj ? end : jj;
        const int edge = end + 1 < width - 1 ? end + 1 : width - 1;
        if (l < 5) {   // h_b[0], e_b[0], h_b[edge], e_b[edge], h_c[0] = 0: one store of five lanes
            int32_t *z = l == 0 ? h_b : (l == 1 ? e_b : (l == 2 ? h_b + edge : (l == 3 ? e_b + edge : h_c)));
            bandSt<GLOBAL>(z, 0);
        }
        bandSync<GLOBAL>();
        const int sCur = sNext;
        const int r1 = rowClamp(i + 1), r2 = rowClamp(i + 2);
        sNext = scoreOf(r1, qb, tb);
        const int qc = q[r2], cbc = PROF ? 0 : (int) cb[r2], tc = loadT(r2);
        const int xi = (i - band) > 0 ? (i - band) : 0;
        const int xim = (i - 1 - band) > 0 ? (i - 1 - band) : 0;
        const int W = end - beg + 1;
        const int8_t *mrow = PROF ? qProf + (tk.qAbs + (uint64_t) i) * 21 : smat + 21 * qa;   // never a mixed (flat) pointer
        const int cbi = cba;
        int8_t *dl = direction + (long long) width_d * i;
        int carry = -ge, prevHc = 0, prevF = 0, uLast = 0;
        for (int p0 = 0; p0 < W; p0 += 32) {
            const int p = p0 + l;
            const bool valid = p < W;
            const int j = beg + p;
            const int u = j - xi + 1;
            int T = 0, eNew = 0, e1 = 0, diag = 0;
            bool dirE = false;
            if (valid) {
                const int e = j - xim + 1, d = (j - 1) - xim + 1;
                int t1 = i == 0 ? -go : bandLd<GLOBAL>(h_b + e) - go;
                int t2 = i == 0 ? -ge : bandLd<GLOBAL>(e_b + e) - ge;
                eNew = t1 > t2 ? t1 : t2;
                dirE = t1 > t2;
                e1 = eNew > 0 ? eNew : 0;
                const int sc = (p0 == 0 ? sCur : (int) mrow[t[j]]) + cbi;
                diag = bandLd<GLOBAL>(h_b + d) + sc;
                T = e1 > diag ? e1 : diag;
            }
            // exclusive prefix maximum of S = T - go + ge * (p + 1) over the 32 lanes by DPP moves (the half wavefront is two
            // rows of 16), carried as S + go + 1 >= 1 so that the 0 a zero-filled move delivers is the identity
            int incl = valid ? T + ge * (p + 1) + 1 : 0, o;
            o = dppZ(incl, 0x111); incl = incl > o ? incl : o;
            o = dppZ(incl, 0x112); incl = incl > o ? incl : o;
            o = dppZ(incl, 0x114); incl = incl > o ? incl : o;
            o = dppZ(incl, 0x118); incl = incl > o ? incl : o;
            o = dppI(0, incl, 0x142, 0xa); incl = incl > o ? incl : o;
            int excl = dppZ(incl, 0x138);
            excl = l == 0 ? 0 : excl;
            const int exclS = excl - go - 1;   // (no predecessor: -go - 1 < -ge <= carry)
            int g = carry > exclS ? carry : exclS;
            const int f = g - ge * p;
            const int hcv = T > f ? T : f;
            int hcP = dppZ(hcv, 0x138), fP = dppZ(f, 0x138);
            if (l == 0) { hcP = prevHc; fP = prevF; }
            if (valid) {
                const bool dirF = (hcP - go) > (fP - ge);
                const int f1 = f > 0 ? f : 0;
                const int tmp1 = e1 > f1 ? e1 : f1;
                int code = (dirE ? 1 : 0) | (dirF ? 2 : 0);
                if (!(tmp1 <= diag)) code |= (e1 > f1) ? 4 : 8;
                dl[j - xi] = (int8_t) code;
                bandSt<GLOBAL>(e_b + u, eNew);
                bandSt<GLOBAL>(h_c + u, hcv);
                maxv = hcv > maxv ? hcv : maxv;
            }
            // carries to the next chunk: lane 31 of this half (a full chunk whenever there is a next one)
            if (p0 + 32 < W) {
                const int cmA = __builtin_amdgcn_readlane(incl, 31), cmB = __builtin_amdgcn_readlane(incl, 63);
                const int hcA = __builtin_amdgcn_readlane(hcv, 31), hcB = __builtin_amdgcn_readlane(hcv, 63);
                const int fA = __builtin_amdgcn_readlane(f, 31), fB = __builtin_amdgcn_readlane(f, 63);
                const int cm = (grp ? cmB : cmA) - go - 1;
                carry = carry > cm ? carry : cm;
                prevHc = grp ? hcB : hcA;
                prevF = grp ? fB : fA;
            }
            const int lastValid = (W - p0) < 32 ? (W - p0 - 1) : 31;
            uLast = (beg + p0 + lastValid) - xi + 1;
            if constexpr (!GLOBAL) __builtin_amdgcn_wave_barrier();   // (GLOBAL: a lane only re-reads what other lanes wrote after the row's fence)
        }
        bandSync<GLOBAL>();
        // the reference copies h_c[1 .. uLast] to h_b here (:1477-1478).  The arrays are exchanged instead: the next row reads h_b at
        // indices 0 (zeroed above), 1 .. uLast (this row's values in either form) and, where its window grew by a column, uLast + 1 --
        // which is exactly the `edge` index it has just zeroed (end + 1 while the window still starts at column 0, width - 1
        // afterwards) -- so what the other entries hold never reaches a cell
        if (W > 0) {
            int32_t *sw = h_b;
            h_b = h_c;
            h_c = sw;
        }
        (void) uLast;
        qa = qb;
        cba = cbb;
        qb = qc;
        cbb = cbc;
        tb = tc;
    }
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
        int o = __shfl_xor(maxv, off, 32);
        maxv = o > maxv ? o : maxv;
    }
    if (maxv >= tk.score) break;
    band *= 2;   // the reference's do/while doubles the band (:1492-1493)
    if (band * 2 + 3 > maxWidthLoop) {
        if (have && l == 0) {
            tasks[id].maxv = maxv;
            tasks[id].band = band;
            res[2 * id] = -2;
        }
        return;
    }
  }
    if (!have || l != 0) return;
    tasks[id].maxv = maxv;
    tasks[id].band = band;
    res[2 * id] = -3;   // band found, directions written: sw_traceback_walk_kernel walks the path
}

// The walk of the LDS-band / global-band kernel's tasks: inside sw_traceback_kernel it was lane 0 of a half wavefront chasing
// ~qLen + tLen dependent loads with 31 lanes parked.  Here 16 lanes own a task (four tasks per wavefront): while the walk is in
// the match state the lanes look at the next 16 cells down the diagonal at once (16 independent loads instead of 16 dependent
// ones), the leading run of cells whose code says "diagonal" is taken in one step -- a coalesced store of 'M's, identities by
// popcount -- and the first cell that is anything else goes through the one-cell step, executed by all 16 lanes alike (same
// address: one request) so that the walk state stays uniform over the group.
// traceback (:1498-1558) + expansion / identity count (computerBacktrace, :548-581)
constexpr int TBW_LANES = 16;
template <bool GLOBAL>
__global__ void __launch_bounds__(256)
sw_traceback_walk_kernel(const TbTask *__restrict__ tasks, uint32_t nTasks, const uint8_t *__restrict__ qRes,
                         const uint8_t *__restrict__ tRes, const int8_t *__restrict__ dirs, char *__restrict__ bt,
                         int32_t *__restrict__ res, const uint32_t *__restrict__ order /* nullable */) {
    const uint32_t lid = (blockIdx.x * blockDim.x + threadIdx.x) / TBW_LANES;
    const int l = threadIdx.x & (TBW_LANES - 1), sh = threadIdx.x & 63 & ~(TBW_LANES - 1);
    uint32_t id = 0;
    bool have = lid < nTasks;
    if (have) {
        id = order ? order[lid] : lid;
        have = res[2 * id] == -3;
    }
    TbTask tk;
    if (have) tk = tasks[id];
    else { tk.qLen = 1; tk.tLen = 1; tk.band = 1; tk.qAbs = 0; tk.tAbs = 0; tk.dirOff = 0; tk.btOff = 0; }
    const int qLen = tk.qLen, tLen = tk.tLen, band = tk.band;
    const int width_d = band * 2 + 1;
    const uint8_t *q = qRes + tk.qAbs;
    const uint8_t *t = tRes + tk.tAbs;
    const int8_t *direction = dirs + tk.dirOff + (GLOBAL ? tbGlobalIntBytes(band) : 0);
    // the path is walked from its end, so the characters are written from the end of the task's region backwards:
    // the finished backtrace is the last `len` bytes of [btOff, btOff + qLen + tLen + 2)
    int i = qLen - 1, j = tLen - 1, state = 2;
    char *o = bt + tk.btOff + (qLen + tLen + 2);
    int len = 0, ids = 0;
    bool bad = false;
    bool going = have && (i > 0 || j > 0);
    while (__ballot(going)) {
        {
            const int ii = i - l, jj = j - l;
            bool ok = going && state == 2 && (ii > 0 || jj > 0) && ii >= 0 && jj >= 0;
            int x = ii - band;
            x = x > 0 ? x : 0;
            x = jj - x;
            ok = ok && x >= 0 && x < width_d;
            bool same = false;
            if (ok) {
                const int code = direction[(long long) width_d * ii + x];
                ok = (code & 12) == 0;
                same = q[ii] == t[jj];
            }
            const uint32_t okMask = (uint32_t) (__ballot(ok) >> sh) & ((1u << TBW_LANES) - 1u);
            const uint32_t sameMask = (uint32_t) (__ballot(same) >> sh);
            const int run = __builtin_ctz(~okMask);   // (bit 16 of ~okMask is set: run <= 16)
            const uint32_t runMask = (1u << run) - 1u;
            if (l < run) o[-1 - l] = 'M';
            ids += __builtin_popcount(sameMask & runMask);
            i -= run;
            j -= run;
            o -= run;
            len += run;
        }
        if (going && (i > 0 || j > 0)) {
            if (i < 0 || j < 0) bad = true;
            int x = i - band;
            x = x > 0 ? x : 0;
            x = j - x;
            if (x < 0 || x >= width_d) bad = true;
            if (!bad) {
                const int code = direction[(long long) width_d * i + x];
                int dcode;
                const int dE = (code & 1) ? 3 : 2, dF = (code & 2) ? 5 : 4;
                if (state == 0) dcode = dE;
                else if (state == 1) dcode = dF;
                else dcode = (code & 4) ? dE : ((code & 8) ? dF : 1);
                char c;
                switch (dcode) {
                    case 1: ids += (q[i] == t[j]); --i; --j; state = 2; c = 'M'; break;
                    case 2: --i; state = 0; c = 'I'; break;
                    case 3: --i; state = 2; c = 'I'; break;
                    case 4: --j; state = 1; c = 'D'; break;
                    default: --j; state = 2; c = 'D'; break;
                }
                --o;
                if (l == 0) *o = c;
                len++;
            }
        }
        going = going && !bad && (i > 0 || j > 0);
    }
    if (!have || l != 0) return;
    if (bad || i != 0 || j != 0) {
        res[2 * id] = -1;
        return;
    }
    ids += (q[0] == t[0]);
    *--o = 'M';
    len++;
    res[2 * id] = len;
    res[2 * id + 1] = ids;
}

// ---------------------------------------------------------------------------------------------
// Narrow bands (2*band+3 <= 32, i.e. almost every alignment): the same banded_sw arithmetic with the three band
// arrays held in registers -- lane p of a 32-lane half wavefront owns array index p -- so a row costs a few DPP
// moves instead of LDS round trips: h_b[e], e_b[e] and h_b[d] are the lane itself or a neighbour depending on
// whether the band window moved (xi != xim), the horizontal-gap prefix maximum is a DPP scan, and the band is
// doubled inside the kernel while it still fits.  The query slice, its bias, the target slice and the 4-bit
// direction codes (16 bytes per row) live in LDS; lane 0 walks the path out of LDS.
// qCap / tCap: LDS capacity per task (rows, columns) of this launch class.
// ---------------------------------------------------------------------------------------------
template <bool PROF>
__global__ void __launch_bounds__(64)
sw_traceback_narrow_kernel(TbTask *__restrict__ tasks, uint32_t nTasks, const uint8_t *__restrict__ qRes,
                           const int8_t *__restrict__ qBias, const uint8_t *__restrict__ tRes, const int8_t *__restrict__ mat,
                           int go, int ge, int qCap, int tCap, char *__restrict__ bt, int32_t *__restrict__ res,
                           const uint32_t *__restrict__ order, const int8_t *__restrict__ qProf /* nullable: profile queries */) {
    extern __shared__ uint8_t ldsRaw[];
    __shared__ int8_t smat[441];
    for (int i = threadIdx.x; i < 441; i += 64) smat[i] = mat[i];
    const int grp = threadIdx.x >> 5, l = threadIdx.x & 31;
    const uint32_t lid = blockIdx.x * 2 + grp;
    const bool have = lid < nTasks;
    const uint32_t id = have ? (order ? order[lid] : lid) : 0;
    TbTask tk;
    if (have) tk = tasks[id];
    else { tk.qLen = 0; tk.tLen = 0; tk.band = 1; tk.score = 0; tk.maxv = 0; tk.qAbs = 0; tk.tAbs = 0; tk.slot = 0; tk.dirOff = 0; tk.btOff = 0; }
    const int qLen = tk.qLen, tLen = tk.tLen;
    const size_t perTask = (size_t) 16 * qCap + 2 * (size_t) qCap + tCap;
    uint8_t *dirs = ldsRaw + grp * perTask;           // 16 bytes (32 nibbles) per row
    uint8_t *sq = dirs + (size_t) 16 * qCap;          // query residues
    int8_t *scb = (int8_t *) (sq + qCap);             // query bias
    uint8_t *st = (uint8_t *) (scb + qCap);           // target residues
    for (int x = l; x < qLen; x += 32) {
        sq[x] = qRes[tk.qAbs + x];
        scb[x] = qBias[tk.qAbs + x];
    }
    for (int x = l; x < tLen; x += 32) st[x] = tRes[tk.tAbs + x];
    __syncthreads();

    const int NEG = -(1 << 28);
    int band = tk.band, maxv = tk.maxv;
    bool reached = false;
    // both half wavefronts run the same number of attempts / rows (uniform control flow for the DPP moves)
    for (;;) {
        const int width = band * 2 + 3;
        const bool fits = width <= 32;
        int hb = 0, eb = 0;
        const int rows = (fits && !reached) ? qLen : 0;
        const int rowsOther = __shfl_xor(rows, 32, 64);
        const int nRows = max(rows, rowsOther);
        // substitution score of this lane's cell: its operands (query letter, bias, target letter) are read two rows ahead and
        // the matrix / profile entry one row ahead, so that neither of the two dependent LDS round trips is waited for inside a
        // row (a wavefront issues in order: a wait in front of the first use stalls the recurrence behind it as well)
        // (no branch around the reads -- a half without rows reads its first entries: every address stays inside the task's LDS
        // slice / the profile -- so that the only waits are in front of the uses)
        auto cellOps = [&](int row, int &qv, int &tv, int &cbv) {
            int r = row < qLen ? row : qLen - 1;
            r = r > 0 ? r : 0;
            const int x0 = (r - band) > 0 ? (r - band) : 0;
            int jn = x0 + l - 1;
            jn = jn >= tLen ? tLen - 1 : jn;
            jn = jn > 0 ? jn : 0;
            tv = st[jn];
            qv = 0;
            cbv = 0;
            if (!PROF) {
                qv = sq[r];
                cbv = scb[r];
            }
        };
        // (the matrix entry and the bias stay separate until the cell uses them: an add right behind the read would put the wait for
        // the read at the top of the row)
        auto cellLook = [&](int row, int qv, int tv) -> int {
            int r = row < qLen ? row : qLen - 1;
            r = r > 0 ? r : 0;
            if (PROF) return (int) qProf[(tk.qAbs + (uint64_t) r) * 21 + (tv < 21 ? tv : 20)];
            return (int) smat[21 * qv + tv];   // (an idle half may form any index from its unwritten slice: LDS, no cell takes the value)
        };
        int qb, tb, cbb;
        cellOps(0, qb, tb, cbb);
        int sNext = cellLook(0, qb, tb), cNext = cbb;
        cellOps(1, qb, tb, cbb);
        for (int i = 0; i < nRows; i++) {
            const bool live = i < rows;
            const int sCur = sNext, cCur = cNext;
            sNext = cellLook(i + 1, qb, tb);
            cNext = cbb;
            cellOps(i + 2, qb, tb, cbb);
            const int xi = (i - band) > 0 ? (i - band) : 0;
            const int delta = (i - band) >= 1 ? 1 : 0;     // xi - xim
            int end = tLen - 1;
            end = end < i + band ? end : i + band;
            const int edge = end + 1 < width - 1 ? end + 1 : width - 1;
            const int W = end - xi + 1;
            const bool zeroed = live && (l == 0 || l == edge);
            hb = zeroed ? 0 : hb;
            eb = zeroed ? 0 : eb;
            // previous-row values at index e = u + delta and d = e - 1 (zero-filled DPP moves, no exec masking: every
            // lane computes, `valid` selects what is kept)
            const int hbUp = dppZ(hb, 0x130), ebUp = dppZ(eb, 0x130), hbDn = dppZ(hb, 0x138);
            const int hE = delta ? hbUp : hb, eE = delta ? ebUp : eb, hD = delta ? hb : hbDn;
            const int u = l;
            const bool valid = live && u >= 1 && u <= W;
            const int t1 = i == 0 ? -go : hE - go;
            const int t2 = i == 0 ? -ge : eE - ge;
            const int eNew = t1 > t2 ? t1 : t2;
            const bool dirE = t1 > t2;
            const int e1 = eNew > 0 ? eNew : 0;
            const int diag = hD + sCur + cCur;
            const int T = e1 > diag ? e1 : diag;
            // prefix maximum of S = T - go + ge*u, carried as S + go + 1 >= 1 so that 0 (what a zero-filled DPP move
            // delivers where there is no source lane) is the identity
            int incl = valid ? T + ge * u + 1 : 0, o;
            o = dppZ(incl, 0x111); incl = incl > o ? incl : o;
            o = dppZ(incl, 0x112); incl = incl > o ? incl : o;
            o = dppZ(incl, 0x114); incl = incl > o ? incl : o;
            o = dppZ(incl, 0x118); incl = incl > o ? incl : o;
            o = dppI(0, incl, 0x142, 0xa); incl = incl > o ? incl : o;
            int excl = dppZ(incl, 0x138);
            excl = l == 0 ? 0 : excl;
            const int gx = excl - go - 1;
            const int g = (-ge) > gx ? (-ge) : gx;
            const int f = g - ge * (u - 1);
            const int hcv = T > f ? T : f;
            int hcP = dppZ(hcv, 0x138), fP = dppZ(f, 0x138);
            hcP = u <= 1 ? 0 : hcP;
            fP = u <= 1 ? 0 : fP;
            const bool dirF = (hcP - go) > (fP - ge);
            const int f1 = f > 0 ? f : 0;
            const int tmp1 = e1 > f1 ? e1 : f1;
            int code = (dirE ? 1 : 0) | (dirF ? 2 : 0) | ((tmp1 > diag) ? ((e1 > f1) ? 4 : 8) : 0);
            code = valid ? code : 0;
            eb = valid ? eNew : eb;
            hb = valid ? hcv : hb;
            maxv = (valid && hcv > maxv) ? hcv : maxv;
            // two cells per byte: cell x = u - 1; odd u carries the low nibble and fetches its right neighbour's
            const int codeUp = dppZ(code, 0x130);
            if (valid && (u & 1)) dirs[(size_t) 16 * i + ((u - 1) >> 1)] = (uint8_t) (code | (codeUp << 4));
        }
        if (!reached && fits) {
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) {
                const int o2 = __shfl_xor(maxv, off, 32);
                maxv = o2 > maxv ? o2 : maxv;
            }
            if (maxv >= tk.score) reached = true;
            else band *= 2;
        }
        const bool done = reached || band * 2 + 3 > 32 || !have;
        const bool doneOther = __shfl_xor(done ? 1 : 0, 32, 64) != 0;
        if (done && doneOther) break;
    }
    __syncthreads();
    if (have && l == 0) {
        tasks[id].maxv = maxv;
        tasks[id].band = band;
        if (!reached) res[2 * id] = -2;
    }
    // traceback (:1498-1558) + expansion / identity count (computerBacktrace, :548-581), written backwards.  The path is mostly
    // runs of diagonal steps: while the walk is in the match state the 32 lanes of the half wavefront look at the next 32 cells
    // down the diagonal at once, the leading run of cells whose code says "diagonal" is taken in one step (a coalesced store
    // of 'M's, identities by popcount), and the first cell that is anything else goes through the one-cell step below, which
    // every lane of the half executes redundantly (same LDS words: broadcasts) so that the walk state stays lane-uniform.
    const int width_d = band * 2 + 1;
    int i = qLen - 1, j = tLen - 1, state = 2;
    char *o = bt + tk.btOff + (qLen + tLen + 2);
    int len = 0, ids = 0;
    bool bad = false;
    bool going = have && reached && (i > 0 || j > 0);
    const int sh = grp * 32;
    while (__ballot(going)) {
        {
            const int ii = i - l, jj = j - l;
            bool ok = going && state == 2 && (ii > 0 || jj > 0) && ii >= 0 && jj >= 0;
            int x = ii - band;
            x = x > 0 ? x : 0;
            x = jj - x;
            ok = ok && x >= 0 && x < width_d;
            bool same = false;
            if (ok) {
                const int byte = dirs[(size_t) 16 * ii + (x >> 1)];
                const int code = (x & 1) ? (byte >> 4) : (byte & 15);
                ok = (code & 12) == 0;
                same = sq[ii] == st[jj];
            }
            const uint32_t okMask = (uint32_t) (__ballot(ok) >> sh);
            const uint32_t sameMask = (uint32_t) (__ballot(same) >> sh);
            const int run = okMask == 0xFFFFFFFFu ? 32 : __builtin_ctz(~okMask);
            const uint32_t runMask = run == 32 ? 0xFFFFFFFFu : ((1u << run) - 1u);
            if (l < run) o[-1 - l] = 'M';
            ids += __builtin_popcount(sameMask & runMask);
            i -= run;
            j -= run;
            o -= run;
            len += run;
        }
        if (going && (i > 0 || j > 0)) {
            if (i < 0 || j < 0) bad = true;
            int x = i - band;
            x = x > 0 ? x : 0;
            x = j - x;
            if (x < 0 || x >= width_d) bad = true;
            if (!bad) {
                const int byte = dirs[(size_t) 16 * i + (x >> 1)];
                const int code = (x & 1) ? (byte >> 4) : (byte & 15);
                int dcode;
                const int dE = (code & 1) ? 3 : 2, dF = (code & 2) ? 5 : 4;
                if (state == 0) dcode = dE;
                else if (state == 1) dcode = dF;
                else dcode = (code & 4) ? dE : ((code & 8) ? dF : 1);
                char c;
                switch (dcode) {
                    case 1: ids += (sq[i] == st[j]); --i; --j; state = 2; c = 'M'; break;
                    case 2: --i; state = 0; c = 'I'; break;
                    case 3: --i; state = 2; c = 'I'; break;
                    case 4: --j; state = 1; c = 'D'; break;
                    default: --j; state = 2; c = 'D'; break;
                }
                --o;
                if (l == 0) *o = c;
                len++;
            }
        }
        going = going && !bad && (i > 0 || j > 0);
    }
    if (!have || !reached || l != 0) return;
    if (bad || i != 0 || j != 0) {
        res[2 * id] = -1;
        return;
    }
    ids += (sq[0] == st[0]);
    *--o = 'M';
    len++;
    res[2 * id] = len;
    res[2 * id + 1] = ids;
}

// ---- score kernels: one launcher signature for all three families (n: entries of dOrder; dBound: strip hand-over space of the
// multi-strip classes, unused by the others)
using ScoreLaunch = void (*)(sd_ctx *ctx, const SwTask *dTasks, const uint32_t *dOrder, uint32_t n, const sd_seqset *q, const sd_seqset *t,
                             const int8_t *dMat, int go, int ge, int32_t *dOut, uint2 *dBound);

template <int RT, int LW, bool MULTI, bool WIDE, bool SHARED>
void launchScorePk(sd_ctx *ctx, const SwTask *dTasks, const uint32_t *dOrder, uint32_t n, const sd_seqset *q,
                   const sd_seqset *t, const int8_t *dMat, int go, int ge, int32_t *dOut, uint2 *dBound) {
    if (n == 0) return;
    constexpr uint32_t perWave = 2 * (64 / LW);
    dim3 grid((n + perWave - 1) / perWave), block(64);
    hipLaunchKernelGGL((sdpk::sw_score_pk_kernel<RT, LW, MULTI, WIDE, SHARED>), grid, block, 0, ctx->stream, dTasks, n, q->dRes, q->dBias,
                       t->dRes, dMat, go, ge, dOut, dBound, dOrder, (const int8_t *) q->dProf);
}

// Task pairs per wavefront of the shared side of class ci: two 32-lane groups, or -- sd_sw_set_group16, forward passes, the aligned
// classes of up to GROUP16_ROWS_MAX rows, a_seg5 .. a_seg14 -- four 16-lane groups (defined beside pairedClass; the pairing kernels pad a query's run
// of pairs to this many, and the launcher of the aligned kernel sizes its grid by it)
// (the row code allows 2 * RT <= 32 rows per lane, i.e. up to 512 rows; a_seg15 and a_seg16 were measured no faster on 16 lanes than
// on 32 -- DESIGN.md 4.1, profiles/sw_group16.json -- and stay there)
constexpr int GROUP16_ROWS_MAX = 448;
constexpr __host__ __device__ uint32_t pairsPerWave(uint32_t ci, int startOnly, int group16);
constexpr uint32_t alignedClass(int RT) { return (uint32_t) RT - 4; }   // a_seg<RT>, checked below the class table

template <int RT, bool SHARED, bool START = false>
void launchScorePkAligned(sd_ctx *ctx, const SwTask *dTasks, const uint32_t *dOrder, uint32_t n, const sd_seqset *q, const sd_seqset *t,
                          const int8_t *dMat, int go, int ge, int32_t *dOut, uint2 * /* dBound: one strip */) {
    if (n == 0) return;
    // a task pair per group of lanes: two 32-lane groups, or four 16-lane ones (shared forward side only)
    const uint32_t perWave = (SHARED && !START) ? 2 * pairsPerWave(alignedClass(RT), 0, ctx->group16 ? 1 : 0) : 4;
    dim3 grid((n + perWave - 1) / perWave), block(64);
    if constexpr (SHARED && !START && 32 * RT <= GROUP16_ROWS_MAX) {
        if (perWave == 8) {
            hipLaunchKernelGGL((sdpk::sw_score_pk_aligned_kernel<RT, true, false, 16>), grid, block, 0, ctx->stream, dTasks, n, q->dRes, q->dBias,
                               t->dRes, dMat, go, ge, dOut, dOrder, (const int8_t *) q->dProf);
            return;
        }
    }
    hipLaunchKernelGGL((sdpk::sw_score_pk_aligned_kernel<RT, SHARED, START>), grid, block, 0, ctx->stream, dTasks, n, q->dRes, q->dBias, t->dRes,
                       dMat, go, ge, dOut, dOrder, (const int8_t *) q->dProf);
}

// dOrder nullable: the tasks in their own order
template <int RT>
void launchScoreIdx(sd_ctx *ctx, const SwTask *dTasks, const uint32_t *dOrder, uint32_t n, const sd_seqset *q,
                    const sd_seqset *t, const int8_t *dMat, int go, int ge, int32_t *dOut, uint2 *dBound) {
    if (n == 0) return;
    dim3 grid((n + 1) / 2), block(64);
    hipLaunchKernelGGL(sw_score_kernel<RT>, grid, block, 0, ctx->stream, dTasks, n, q->dRes, q->dBias, t->dRes, dMat,
                       go, ge, dOut, dBound, dOrder, (const int8_t *) q->dProf);
}

// ---------------------------------------------------------------------------------------------
// The score-class table: a class is a row limit of one of three forms, and per form of pairing (tasks of one query two by two --
// shared -- or every task alone) the kernel instantiation that runs it and the profile scope that names that kernel.  Everything
// that has to know a class reads it here: the class of a task (scoreClassOf, checked against the limits below for every row count),
// the strip hand-over space (k_bound_need), the launches (devRunScore, runScoreTasks) and sd_selftest_score_class.
//   narrow    pass 1 and the start positions of its results: <= 128 rows on the general packed kernel, 129 .. 768 rows in steps of 32
//             on the aligned one (RT = ceil(n / 32) = 5 .. 24: a task pays for the rows of its class, and the reference's 32 SIMD
//             segments are the 32 lanes), then 2 / 3 / more strips of 512 rows.  Unshared tasks (two profiles per pair in LDS) beyond
//             384 rows keep their class of 32 rows and run on the general kernel of 512 / 640 / 768 rows
//   wide      the general packed kernel with the wide row code: word-kernel reruns and their start positions
//   int32     every call the packed kernels do not take (usePk), and word tasks beyond wideRowLimit
//   start     sd_sw_set_shared_start: the narrow start-position tasks of a query of 129 .. 768 rows, on the start-row form of the
//             aligned kernel.  The class is the QUERY's (n = its length: the profile of the whole reversed query serves every task
//             of the query, k_gate_rev), always paired by query, so there is one side.  The forms before it keep their indices
// The pair sort carries the class in six bits: fewer than 64 classes.
enum ScoreKernel { SCORE_PK = 0, SCORE_PK_WIDE = 1, SCORE_INT32 = 2, SCORE_PK_START = 3 };
constexpr int START_ROWS_MIN = 129, START_ROWS_MAX = 768;
constexpr int SCORE_ROWS_ANY = 0x7FFFFFFF;
constexpr int I32_STRIP_ROWS = 1024;   // sw_score_kernel<32>: a task of more rows hands its last row from strip to strip
struct ScoreSide { const char *scope; ScoreLaunch launch; };
struct ScoreClass {
    ScoreKernel form;
    int rows;        // the class holds the tasks of its form with more rows than the class before it and at most this many
    int boundNeed;   // strip hand-over space, uint2 per target column: the packed kernels hand over 16 bytes, the int32 kernel 8
    ScoreSide shared, unshared;
};
constexpr ScoreClass SCORE_CLASSES[] = {
    {SCORE_PK, 128, 0, {"sw_score_pk.rt4x32", launchScorePk<4, 32, false, false, true>}, {"sw_score_pk.rt4x32", launchScorePk<4, 32, false, false, false>}},
    {SCORE_PK, 160, 0, {"sw_score_pk.a_seg5", launchScorePkAligned<5, true>}, {"sw_score_pk.a_seg5", launchScorePkAligned<5, false>}},
    {SCORE_PK, 192, 0, {"sw_score_pk.a_seg6", launchScorePkAligned<6, true>}, {"sw_score_pk.a_seg6", launchScorePkAligned<6, false>}},
    {SCORE_PK, 224, 0, {"sw_score_pk.a_seg7", launchScorePkAligned<7, true>}, {"sw_score_pk.a_seg7", launchScorePkAligned<7, false>}},
    {SCORE_PK, 256, 0, {"sw_score_pk.a_seg8", launchScorePkAligned<8, true>}, {"sw_score_pk.a_seg8", launchScorePkAligned<8, false>}},
    {SCORE_PK, 288, 0, {"sw_score_pk.a_seg9", launchScorePkAligned<9, true>}, {"sw_score_pk.a_seg9", launchScorePkAligned<9, false>}},
    {SCORE_PK, 320, 0, {"sw_score_pk.a_seg10", launchScorePkAligned<10, true>}, {"sw_score_pk.a_seg10", launchScorePkAligned<10, false>}},
    {SCORE_PK, 352, 0, {"sw_score_pk.a_seg11", launchScorePkAligned<11, true>}, {"sw_score_pk.a_seg11", launchScorePkAligned<11, false>}},
    {SCORE_PK, 384, 0, {"sw_score_pk.a_seg12", launchScorePkAligned<12, true>}, {"sw_score_pk.a_seg12", launchScorePkAligned<12, false>}},
    {SCORE_PK, 416, 0, {"sw_score_pk.a_seg13", launchScorePkAligned<13, true>}, {"sw_score_pk.rt8x64", launchScorePk<8, 64, false, false, false>}},
    {SCORE_PK, 448, 0, {"sw_score_pk.a_seg14", launchScorePkAligned<14, true>}, {"sw_score_pk.rt8x64", launchScorePk<8, 64, false, false, false>}},
    {SCORE_PK, 480, 0, {"sw_score_pk.a_seg15", launchScorePkAligned<15, true>}, {"sw_score_pk.rt8x64", launchScorePk<8, 64, false, false, false>}},
    {SCORE_PK, 512, 0, {"sw_score_pk.a_seg16", launchScorePkAligned<16, true>}, {"sw_score_pk.rt8x64", launchScorePk<8, 64, false, false, false>}},
    {SCORE_PK, 544, 0, {"sw_score_pk.a_seg17", launchScorePkAligned<17, true>}, {"sw_score_pk.rt10x64", launchScorePk<10, 64, false, false, false>}},
    {SCORE_PK, 576, 0, {"sw_score_pk.a_seg18", launchScorePkAligned<18, true>}, {"sw_score_pk.rt10x64", launchScorePk<10, 64, false, false, false>}},
    {SCORE_PK, 608, 0, {"sw_score_pk.a_seg19", launchScorePkAligned<19, true>}, {"sw_score_pk.rt10x64", launchScorePk<10, 64, false, false, false>}},
    {SCORE_PK, 640, 0, {"sw_score_pk.a_seg20", launchScorePkAligned<20, true>}, {"sw_score_pk.rt10x64", launchScorePk<10, 64, false, false, false>}},
    {SCORE_PK, 672, 0, {"sw_score_pk.a_seg21", launchScorePkAligned<21, true>}, {"sw_score_pk.rt12x64", launchScorePk<12, 64, false, false, false>}},
    {SCORE_PK, 704, 0, {"sw_score_pk.a_seg22", launchScorePkAligned<22, true>}, {"sw_score_pk.rt12x64", launchScorePk<12, 64, false, false, false>}},
    {SCORE_PK, 736, 0, {"sw_score_pk.a_seg23", launchScorePkAligned<23, true>}, {"sw_score_pk.rt12x64", launchScorePk<12, 64, false, false, false>}},
    {SCORE_PK, 768, 0, {"sw_score_pk.a_seg24", launchScorePkAligned<24, true>}, {"sw_score_pk.rt12x64", launchScorePk<12, 64, false, false, false>}},
    {SCORE_PK, 1024, 2, {"sw_score_pk.rt8x64s2", launchScorePk<8, 64, true, false, true>}, {"sw_score_pk.rt8x64s2", launchScorePk<8, 64, true, false, false>}},
    {SCORE_PK, 1536, 2, {"sw_score_pk.rt8x64s3", launchScorePk<8, 64, true, false, true>}, {"sw_score_pk.rt8x64s3", launchScorePk<8, 64, true, false, false>}},
    {SCORE_PK, SCORE_ROWS_ANY, 2, {"sw_score_pk.rt8x64sN", launchScorePk<8, 64, true, false, true>}, {"sw_score_pk.rt8x64sN", launchScorePk<8, 64, true, false, false>}},
    {SCORE_PK_WIDE, 128, 0, {"sw_score_pk.w_rt4x32", launchScorePk<4, 32, false, true, true>}, {"sw_score_pk.w_rt4x32", launchScorePk<4, 32, false, true, false>}},
    {SCORE_PK_WIDE, 192, 0, {"sw_score_pk.w_rt6x32", launchScorePk<6, 32, false, true, true>}, {"sw_score_pk.w_rt6x32", launchScorePk<6, 32, false, true, false>}},
    {SCORE_PK_WIDE, 224, 0, {"sw_score_pk.w_rt7x32", launchScorePk<7, 32, false, true, true>}, {"sw_score_pk.w_rt7x32", launchScorePk<7, 32, false, true, false>}},
    {SCORE_PK_WIDE, 256, 0, {"sw_score_pk.w_rt8x32", launchScorePk<8, 32, false, true, true>}, {"sw_score_pk.w_rt8x32", launchScorePk<8, 32, false, true, false>}},
    {SCORE_PK_WIDE, 288, 0, {"sw_score_pk.w_rt9x32", launchScorePk<9, 32, false, true, true>}, {"sw_score_pk.w_rt9x32", launchScorePk<9, 32, false, true, false>}},
    {SCORE_PK_WIDE, 320, 0, {"sw_score_pk.w_rt10x32", launchScorePk<10, 32, false, true, true>}, {"sw_score_pk.w_rt10x32", launchScorePk<10, 32, false, true, false>}},
    {SCORE_PK_WIDE, 352, 0, {"sw_score_pk.w_rt11x32", launchScorePk<11, 32, false, true, true>}, {"sw_score_pk.w_rt11x32", launchScorePk<11, 32, false, true, false>}},
    {SCORE_PK_WIDE, 384, 0, {"sw_score_pk.w_rt12x32", launchScorePk<12, 32, false, true, true>}, {"sw_score_pk.w_rt12x32", launchScorePk<12, 32, false, true, false>}},
    {SCORE_PK_WIDE, 512, 0, {"sw_score_pk.w_rt8x64", launchScorePk<8, 64, false, true, true>}, {"sw_score_pk.w_rt8x64", launchScorePk<8, 64, false, true, false>}},
    {SCORE_PK_WIDE, 640, 0, {"sw_score_pk.w_rt10x64", launchScorePk<10, 64, false, true, true>}, {"sw_score_pk.w_rt10x64", launchScorePk<10, 64, false, true, false>}},
    {SCORE_PK_WIDE, 768, 0, {"sw_score_pk.w_rt12x64", launchScorePk<12, 64, false, true, true>}, {"sw_score_pk.w_rt12x64", launchScorePk<12, 64, false, true, false>}},
    {SCORE_PK_WIDE, 1024, 2, {"sw_score_pk.w_rt8x64s2", launchScorePk<8, 64, true, true, true>}, {"sw_score_pk.w_rt8x64s2", launchScorePk<8, 64, true, true, false>}},
    {SCORE_PK_WIDE, 1536, 2, {"sw_score_pk.w_rt8x64s3", launchScorePk<8, 64, true, true, true>}, {"sw_score_pk.w_rt8x64s3", launchScorePk<8, 64, true, true, false>}},
    {SCORE_PK_WIDE, SCORE_ROWS_ANY, 2, {"sw_score_pk.w_rt8x64sN", launchScorePk<8, 64, true, true, true>}, {"sw_score_pk.w_rt8x64sN", launchScorePk<8, 64, true, true, false>}},
    // (tasks of the int32 classes are never paired; of the last class only those of more than I32_STRIP_ROWS rows hand over)
    {SCORE_INT32, 128, 0, {"sw_score.rt4", launchScoreIdx<4>}, {"sw_score.rt4", launchScoreIdx<4>}},
    {SCORE_INT32, 256, 0, {"sw_score.rt8", launchScoreIdx<8>}, {"sw_score.rt8", launchScoreIdx<8>}},
    {SCORE_INT32, 512, 0, {"sw_score.rt16", launchScoreIdx<16>}, {"sw_score.rt16", launchScoreIdx<16>}},
    {SCORE_INT32, SCORE_ROWS_ANY, 1, {"sw_score.rt32", launchScoreIdx<32>}, {"sw_score.rt32", launchScoreIdx<32>}},
    // (whole queries of START_ROWS_MIN .. START_ROWS_MAX rows, RT = 5 .. 24; launched with explicit pairs only)
    {SCORE_PK_START, 160, 0, {"sw_score_pk.s_seg5", launchScorePkAligned<5, true, true>}, {"sw_score_pk.s_seg5", launchScorePkAligned<5, true, true>}},
    {SCORE_PK_START, 192, 0, {"sw_score_pk.s_seg6", launchScorePkAligned<6, true, true>}, {"sw_score_pk.s_seg6", launchScorePkAligned<6, true, true>}},
    {SCORE_PK_START, 224, 0, {"sw_score_pk.s_seg7", launchScorePkAligned<7, true, true>}, {"sw_score_pk.s_seg7", launchScorePkAligned<7, true, true>}},
    {SCORE_PK_START, 256, 0, {"sw_score_pk.s_seg8", launchScorePkAligned<8, true, true>}, {"sw_score_pk.s_seg8", launchScorePkAligned<8, true, true>}},
    {SCORE_PK_START, 288, 0, {"sw_score_pk.s_seg9", launchScorePkAligned<9, true, true>}, {"sw_score_pk.s_seg9", launchScorePkAligned<9, true, true>}},
    {SCORE_PK_START, 320, 0, {"sw_score_pk.s_seg10", launchScorePkAligned<10, true, true>}, {"sw_score_pk.s_seg10", launchScorePkAligned<10, true, true>}},
    {SCORE_PK_START, 352, 0, {"sw_score_pk.s_seg11", launchScorePkAligned<11, true, true>}, {"sw_score_pk.s_seg11", launchScorePkAligned<11, true, true>}},
    {SCORE_PK_START, 384, 0, {"sw_score_pk.s_seg12", launchScorePkAligned<12, true, true>}, {"sw_score_pk.s_seg12", launchScorePkAligned<12, true, true>}},
    {SCORE_PK_START, 416, 0, {"sw_score_pk.s_seg13", launchScorePkAligned<13, true, true>}, {"sw_score_pk.s_seg13", launchScorePkAligned<13, true, true>}},
    {SCORE_PK_START, 448, 0, {"sw_score_pk.s_seg14", launchScorePkAligned<14, true, true>}, {"sw_score_pk.s_seg14", launchScorePkAligned<14, true, true>}},
    {SCORE_PK_START, 480, 0, {"sw_score_pk.s_seg15", launchScorePkAligned<15, true, true>}, {"sw_score_pk.s_seg15", launchScorePkAligned<15, true, true>}},
    {SCORE_PK_START, 512, 0, {"sw_score_pk.s_seg16", launchScorePkAligned<16, true, true>}, {"sw_score_pk.s_seg16", launchScorePkAligned<16, true, true>}},
    {SCORE_PK_START, 544, 0, {"sw_score_pk.s_seg17", launchScorePkAligned<17, true, true>}, {"sw_score_pk.s_seg17", launchScorePkAligned<17, true, true>}},
    {SCORE_PK_START, 576, 0, {"sw_score_pk.s_seg18", launchScorePkAligned<18, true, true>}, {"sw_score_pk.s_seg18", launchScorePkAligned<18, true, true>}},
    {SCORE_PK_START, 608, 0, {"sw_score_pk.s_seg19", launchScorePkAligned<19, true, true>}, {"sw_score_pk.s_seg19", launchScorePkAligned<19, true, true>}},
    {SCORE_PK_START, 640, 0, {"sw_score_pk.s_seg20", launchScorePkAligned<20, true, true>}, {"sw_score_pk.s_seg20", launchScorePkAligned<20, true, true>}},
    {SCORE_PK_START, 672, 0, {"sw_score_pk.s_seg21", launchScorePkAligned<21, true, true>}, {"sw_score_pk.s_seg21", launchScorePkAligned<21, true, true>}},
    {SCORE_PK_START, 704, 0, {"sw_score_pk.s_seg22", launchScorePkAligned<22, true, true>}, {"sw_score_pk.s_seg22", launchScorePkAligned<22, true, true>}},
    {SCORE_PK_START, 736, 0, {"sw_score_pk.s_seg23", launchScorePkAligned<23, true, true>}, {"sw_score_pk.s_seg23", launchScorePkAligned<23, true, true>}},
    {SCORE_PK_START, 768, 0, {"sw_score_pk.s_seg24", launchScorePkAligned<24, true, true>}, {"sw_score_pk.s_seg24", launchScorePkAligned<24, true, true>}},
};
constexpr uint32_t N_SCORE_CLASSES = sizeof(SCORE_CLASSES) / sizeof(SCORE_CLASSES[0]);
static_assert(N_SCORE_CLASSES < 63, "class boundaries are found by one 64-lane wavefront; six class bits in the pair key");
constexpr uint32_t firstScoreClass(ScoreKernel form) {
    uint32_t ci = 0;
    while (SCORE_CLASSES[ci].form != form) ci++;
    return ci;
}
constexpr uint32_t FIRST_WIDE_CLASS = firstScoreClass(SCORE_PK_WIDE), FIRST_INT32_CLASS = firstScoreClass(SCORE_INT32);
constexpr uint32_t FIRST_START_CLASS = firstScoreClass(SCORE_PK_START);
constexpr uint32_t KEY_INVALID = N_SCORE_CLASSES * 1024u;   // sorts after every class
// the classes whose tasks need `need` uint2 of hand-over space per column, one bit each (device code reads the table through constants)
constexpr uint64_t scoreBoundMask(int need) {
    uint64_t m = 0;
    for (uint32_t ci = 0; ci < N_SCORE_CLASSES; ci++) m |= (uint64_t) (SCORE_CLASSES[ci].boundNeed == need) << ci;
    return m;
}
// the class of a task in closed form (the gate kernels run it per pair).
// wideRowLimit: int16 cells hold a score for certain while min(n, tL) * (largest entry of this call's query profiles) <= 32 767
// (no saturation of the reference's word kernel to reproduce, no wrap); longer pairs take the int32 kernel
constexpr __host__ __device__ uint32_t scoreClassOf(int n, int tL, int kernel, int wideRowLimit) {
    if (kernel == SCORE_PK_START) {   // (outside its rows, or beyond 16-bit columns: the narrow form's class)
        if (n >= START_ROWS_MIN && n <= START_ROWS_MAX && tL <= 65535) return FIRST_START_CLASS + (n + 31) / 32 - 5;
        kernel = SCORE_PK;
    }
    if (kernel == SCORE_PK_WIDE && (n < tL ? n : tL) > wideRowLimit) kernel = SCORE_INT32;
    if (kernel == SCORE_INT32 || tL > 65535) return FIRST_INT32_CLASS + (n <= 128 ? 0 : (n <= 256 ? 1 : (n <= 512 ? 2 : 3)));
    const int strips = (n + 511) / 512 < 4 ? (n + 511) / 512 : 4;   // beyond 768 rows: 2, 3, more
    if (kernel == SCORE_PK_WIDE) {
        if (n <= 192) return FIRST_WIDE_CLASS + (n <= 128 ? 0 : 1);
        if (n <= 384) return FIRST_WIDE_CLASS + 2 + (n - 193) / 32;   // 224, 256, 288, 320, 352, 384 rows
        if (n <= 768) return FIRST_WIDE_CLASS + (n <= 512 ? 8 : (n <= 640 ? 9 : 10));
        return FIRST_WIDE_CLASS + 11 + strips - 2;
    }
    if (n <= 128) return 0;
    if (n <= 768) return (n + 31) / 32 - 4;   // RT = 5 .. 24
    return 21 + strips - 2;
}
constexpr bool scoreClassesAreTheTables() {
    for (int form = SCORE_PK; form <= SCORE_INT32; form++)
        for (int n = 1; n <= 2049; n++) {
            const uint32_t ci = scoreClassOf(n, 1, form, SCORE_ROWS_ANY);
            if (ci >= N_SCORE_CLASSES || SCORE_CLASSES[ci].form != form || n > SCORE_CLASSES[ci].rows) return false;
            if (ci > 0 && SCORE_CLASSES[ci - 1].form == form && n <= SCORE_CLASSES[ci - 1].rows) return false;
        }
    for (int n = 1; n <= 2049; n++) {   // the start form: its own classes inside its rows, the narrow form's outside
        const uint32_t ci = scoreClassOf(n, 1, SCORE_PK_START, SCORE_ROWS_ANY);
        if (n < START_ROWS_MIN || n > START_ROWS_MAX) {
            if (ci != scoreClassOf(n, 1, SCORE_PK, SCORE_ROWS_ANY)) return false;
            continue;
        }
        if (ci >= N_SCORE_CLASSES || SCORE_CLASSES[ci].form != SCORE_PK_START || n > SCORE_CLASSES[ci].rows) return false;
        if (SCORE_CLASSES[ci - 1].form == SCORE_PK_START && n <= SCORE_CLASSES[ci - 1].rows) return false;
    }
    return true;
}
static_assert(scoreClassesAreTheTables(), "scoreClassOf: n lies in (rows of the class before, rows of its class] for every n, in every form");
static_assert(SCORE_CLASSES[N_SCORE_CLASSES - 1].form == SCORE_PK_START && SCORE_CLASSES[FIRST_START_CLASS - 1].form == SCORE_INT32 &&
              SCORE_CLASSES[FIRST_INT32_CLASS - 1].form == SCORE_PK_WIDE, "forms in order");
__device__ __forceinline__ uint32_t scoreKey(int n, int tL, int kernel, int wideRowLimit = 800) {
    return scoreClassOf(n, tL, kernel, wideRowLimit) * 1024u + (uint32_t) (1023 - min(tL >> 4, 1023));
}

// run a list of score tasks (any mix of sizes); results land in hOut[3*slot..]
// Tasks are ordered by (RT class, tL descending) with a parallel stable counting sort straight into a pinned
// staging buffer (two tasks share a wavefront, so neighbours should have similar lengths; biggest first).
int runScoreTasks(sd_ctx *ctx, std::vector<SwTask> &tasks, const sd_seqset *q, const sd_seqset *t, const int8_t *dMat,
                  int go, int ge, std::vector<int32_t> &hOut, uint32_t nSlots, uint64_t *cells, const char *tag = "a") {
    hOut.assign((size_t) nSlots * 3, 0);
    if (tasks.empty()) return SD_OK;
    HostScope hsAll(ctx, "score.total");
    const size_t n = tasks.size();
    constexpr int N_I32 = FIRST_START_CLASS - FIRST_INT32_CLASS, NB = N_I32 * 1024;
    auto keyOf = [](const SwTask &t) {
        const uint32_t ci = scoreClassOf(t.n, t.tL, SCORE_INT32, 0) - FIRST_INT32_CLASS;
        return ci * 1024u + (uint32_t) (1023 - std::min(t.tL >> 4, 1023));
    };
    SwTask *sorted = nullptr;
    SD_HIP(ctx, pinGet(ctx, (std::string("sw.tasks.") + tag).c_str(), n, &sorted));
    uint64_t boundTotal = 0, cellSum = 0;
    size_t classBegin[N_I32 + 1] = {};
    {
        int T = 1;
#pragma omp parallel
        {
#pragma omp single
            T = omp_get_num_threads();
        }
        T = std::max(1, std::min(T, 64));
        std::vector<uint32_t> hist((size_t) T * NB, 0);
#pragma omp parallel num_threads(T) reduction(+ : cellSum)
        {
            const int th = omp_get_thread_num();
            const size_t lo = n * th / T, hi = n * (th + 1) / T;
            uint32_t *hh = &hist[(size_t) th * NB];
            for (size_t i = lo; i < hi; i++) {
                hh[keyOf(tasks[i])]++;
                cellSum += (uint64_t) tasks[i].n * (uint64_t) tasks[i].tL;
            }
        }
        // exclusive prefix over (bucket major, thread minor)
        uint64_t run = 0;
        for (int bkt = 0; bkt < NB; bkt++) {
            if ((bkt & 1023) == 0) classBegin[bkt >> 10] = run;
            for (int th = 0; th < T; th++) {
                const uint32_t c = hist[(size_t) th * NB + bkt];
                hist[(size_t) th * NB + bkt] = (uint32_t) run;
                run += c;
            }
        }
        classBegin[N_I32] = run;
#pragma omp parallel num_threads(T)
        {
            const int th = omp_get_thread_num();
            const size_t lo = n * th / T, hi = n * (th + 1) / T;
            uint32_t *hh = &hist[(size_t) th * NB];
            for (size_t i = lo; i < hi; i++) sorted[hh[keyOf(tasks[i])]++] = tasks[i];
        }
    }
    *cells += cellSum;
    for (size_t i = classBegin[N_I32 - 1]; i < classBegin[N_I32]; i++) {   // multi-strip tasks exist in the last class only
        if (sorted[i].n > I32_STRIP_ROWS) {
            sorted[i].boundOff = boundTotal;
            boundTotal += (uint64_t) sorted[i].tL;
        }
    }
    SwTask *dTasks = nullptr;
    int32_t *dOut = nullptr;
    uint2 *dBound = nullptr;
    int32_t *hPin = nullptr;
    SD_HIP(ctx, wsGet(ctx, "sw.tasks", n, &dTasks));
    SD_HIP(ctx, wsGet(ctx, "sw.out", (size_t) nSlots * 3, &dOut));
    SD_HIP(ctx, wsGet(ctx, "sw.bound", std::max<uint64_t>(boundTotal, 1), &dBound));
    SD_HIP(ctx, pinGet(ctx, "sw.hout", (size_t) nSlots * 3, &hPin));
    SD_HIP(ctx, hipMemcpyAsync(dTasks, sorted, n * sizeof(SwTask), hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemsetAsync(dOut, 0, (size_t) nSlots * 3 * sizeof(int32_t), ctx->stream));
    for (int ci = 0; ci < N_I32; ci++) {
        const size_t begin = classBegin[ci], end = classBegin[ci + 1];
        if (end == begin) continue;
        {
            ProfScope ps(ctx, "sw_score");
            SCORE_CLASSES[FIRST_INT32_CLASS + ci].unshared.launch(ctx, dTasks + begin, nullptr, (uint32_t) (end - begin), q, t, dMat, go, ge, dOut, dBound);
        }
        SD_HIP(ctx, hipGetLastError());
    }
    SD_HIP(ctx, hipMemcpyAsync(hPin, dOut, (size_t) nSlots * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    memcpy(hOut.data(), hPin, (size_t) nSlots * 3 * sizeof(int32_t));
    return SD_OK;
}


// ---------------------------------------------------------------------------------------------
// Device-resident orchestration of a batch of pairs: task construction, the gates between the passes and
// the ordering of tasks all happen on the GPU; the host only launches, reads six class boundaries per pass
// and receives the finished result records + a dense backtrace pool.
// ---------------------------------------------------------------------------------------------
struct DevGateParams {
    int go, ge, matMin, swMode, covMode, wideRowLimit;
    float covThr;
    double evalThr;
    // Gumbel parameters (sd::Evaluer) for the device-side E-value gate
    double lambda, K, aI, bI, alphaI, betaI, aJ, bJ, alphaJ, betaJ, sigma, tau, viThr, vjThr, cThr, dbResidues;
};

__device__ double devEvalue(const DevGateParams &e, double y_, double qLen) {
    const double m_ = e.dbResidues, n_ = qLen;
    const double const_val = 0.3989422804014327;   // 1/sqrt(2 pi)
    double tmp = e.aI * y_ + e.bI;
    double m_li_y = m_ - tmp;
    double vi_y = fmax(e.viThr, e.alphaI * y_ + e.betaI);
    double sqrt_vi_y = sqrt(vi_y);
    double m_F = sqrt_vi_y == 0.0 ? 1e100 : m_li_y / sqrt_vi_y;
    double P_m_F = 0.5 * erfc(-sqrt(0.5) * m_F);
    double E_m_F = -const_val * exp(-0.5 * m_F * m_F);
    double p1 = m_li_y * P_m_F - sqrt_vi_y * E_m_F;
    tmp = e.aJ * y_ + e.bJ;
    double n_lj_y = n_ - tmp;
    double vj_y = fmax(e.vjThr, e.alphaJ * y_ + e.betaJ);
    double sqrt_vj_y = sqrt(vj_y);
    double n_F = sqrt_vj_y == 0.0 ? 1e100 : n_lj_y / sqrt_vj_y;
    double P_n_F = 0.5 * erfc(-sqrt(0.5) * n_F);
    double E_n_F = -const_val * exp(-0.5 * n_F * n_F);
    double p2 = n_lj_y * P_n_F - sqrt_vj_y * E_n_F;
    double c_y = fmax(e.cThr, e.sigma * y_ + e.tau);
    double area = p1 * p2 + c_y * (P_m_F * P_n_F);
    return e.K * exp(-e.lambda * y_) * area;
}

__device__ __forceinline__ float devCov(unsigned int startPos, unsigned int endPos, unsigned int len) {
    return (min(len, max(startPos, endPos)) - min(startPos, endPos) + 1) / (float) len;
}
__device__ __forceinline__ bool devHasCoverage(float covThr, int covMode, float qCov, float tCov) {
    switch (covMode) {
        case 0: return (qCov >= covThr) && (tCov >= covThr);
        case 2: return qCov >= covThr;
        case 1: return tCov >= covThr;
        default: return true;
    }
}

// A pair whose byte-kernel score is CERTAIN to saturate needs no byte-structure pass: the reference discards that pass's
// result and reruns the pair with the word kernel (:360-368), and the score of any ungapped stretch of one diagonal is a lower
// bound of the byte kernel's maximum (a diagonal-only path never meets the lane structure's vertical-gap quirk).  With the
// prefilter's diagonal at hand, k_pre_word walks that diagonal with the alignment's own scoring (matrix row + composition bias,
// or the profile row) and marks the pairs whose bound already reaches 255 - bias; they skip pass 1 and go straight to pass 2.
// On proteome-scale searches that is most true homologs, i.e. the longest-running tasks of pass 1.
// sd_sw_set_narrow_final (narrowFinal): the bound is NARROW_EXACT instead.  The packed kernels of pass 1 do not saturate at 255: they
// evaluate the cells the rerun evaluates and choose the end cell by its rule, so below NARROW_EXACT their (score, tEnd, qEnd) is the
// rerun's and pass 1 is the cheaper way to it; a pair skips pass 1 only when it is certain to need the wide kernel all the same.
__global__ void __launch_bounds__(256)
k_pre_word(uint32_t nPairs, const uint32_t *__restrict__ pairQ, const uint32_t *__restrict__ pairT, const uint16_t *__restrict__ pairDiag,
           const uint32_t *__restrict__ fwdKeys, const uint64_t *__restrict__ qOff, const uint64_t *__restrict__ tOff,
           const uint8_t *__restrict__ qRes, const int8_t *__restrict__ qBias, const uint8_t *__restrict__ tRes, const int8_t *__restrict__ mat,
           const int8_t *__restrict__ qProf, const int32_t *__restrict__ minBias, int matMin, uint8_t *__restrict__ preWord,
           uint32_t *__restrict__ pass1Keys, int narrowFinal) {
    __shared__ int8_t smat[441];
    for (int x = threadIdx.x; x < 441; x += blockDim.x) smat[x] = mat[x];
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs) return;
    uint8_t pw = 0;
    const uint32_t key = fwdKeys[i];
    if (key != KEY_INVALID) {
        const uint64_t qo = qOff[pairQ[i]], to = tOff[pairT[i]];
        const int qL = (int) (qOff[pairQ[i] + 1] - qo), tL = (int) (tOff[pairT[i] + 1] - to);
        if (qL < 32768 && tL < 32768 && pairDiag[i] != 0x8000) {   // (longer sequences: the 16-bit diagonal is ambiguous; 0x8000 = caller has no hint)
            const int d = (int) (int16_t) pairDiag[i];
            int q0 = d >= 0 ? d : 0, t0 = d >= 0 ? 0 : -d;
            const int n = min(qL - q0, tL - t0);
            const int need = narrowFinal ? NARROW_EXACT : 255 - (abs(matMin) + abs(minBias[pairQ[i]]));
            int run = 0, best = 0;
            for (int x = 0; x < n && best < need; x++) {
                const int qr = qRes[qo + q0 + x], tr = tRes[to + t0 + x];
                run += qProf ? (int) qProf[(qo + q0 + x) * 21 + tr] : (int) smat[tr * 21 + qr] + (int) qBias[qo + q0 + x];
                run = run < 0 ? 0 : run;
                best = run > best ? run : best;
            }
            pw = best >= need ? 1 : 0;
        }
    }
    preWord[i] = pw;
    pass1Keys[i] = pw ? KEY_INVALID : key;
}

// forward tasks (32-lane structure) for every non-identity pair
__global__ void __launch_bounds__(256)
k_make_fwd(uint32_t nPairs, const uint32_t *__restrict__ pairQ, const uint32_t *__restrict__ pairT,
           const uint8_t *__restrict__ ident, const uint64_t *__restrict__ qOff, const uint64_t *__restrict__ tOff,
           SwTask *__restrict__ tasks, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
           sd_sw_result *__restrict__ res, int usePk) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs) return;
    const uint64_t qo = qOff[pairQ[i]], to = tOff[pairT[i]];
    const int qL = (int) (qOff[pairQ[i] + 1] - qo), tL = (int) (tOff[pairT[i] + 1] - to);
    SwTask tk;
    tk.qOff = qo; tk.tOff = to; tk.n = qL; tk.tL = tL; tk.qStep = 1; tk.tStep = 1;
    tk.segLen = max(1, (qL + 31) / 32);
    tk.slot = i; tk.boundOff = 0;
    const bool valid = !(ident && ident[i]) && qL > 0 && tL > 0;
    tasks[i] = tk;
    keys[i] = valid ? scoreKey(qL, tL, usePk ? SCORE_PK : SCORE_INT32) : KEY_INVALID;
    vals[i] = i;
    sd_sw_result r;
    r.score = 0; r.qStart = -1; r.qEnd = -1; r.tStart = -1; r.tEnd = -1; r.identical = 0; r.btLen = 0; r.flags = 0;
    r.evalue = 0.0; r.btOffset = 0;
    res[i] = r;
}

// class boundaries of a sorted key array: b[c] = lower_bound(c*1024), c = 0..4 (b[4] = number of valid tasks)
__global__ void k_bounds(const uint32_t *__restrict__ keys, uint32_t n, uint32_t step, uint32_t *__restrict__ b, int nb) {
    const int c = threadIdx.x;
    if (c >= nb) return;
    const uint64_t want = (uint64_t) c * step;   // (32 classes x 2^27: the end bound does not fit 32 bits)
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t) keys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    b[c] = lo;
}

// after the 32-lane pass: pairs whose byte score saturates get a 16-lane task (:881,916,360-368)
__global__ void __launch_bounds__(256)
k_gate_word(uint32_t nPairs, const uint32_t *__restrict__ pairQ, const int32_t *__restrict__ out32,
            const int32_t *__restrict__ minBias, int matMin, SwTask *__restrict__ tasks, uint32_t *__restrict__ keys,
            uint32_t *__restrict__ vals, uint8_t *__restrict__ word, const uint32_t *__restrict__ fwdKeys, int usePk, int wideRowLimit,
            const uint8_t *__restrict__ preWord /* nullable: pairs that skipped pass 1 because their byte score saturates for certain */,
            uint8_t *__restrict__ wide /* nullable (sd_sw_set_narrow_final, packed calls): of the word pairs, those that pass 1 does not
                                          answer -- it was skipped, it reports the saturated row code, or it ran on the int32 kernel */,
            unsigned long long *__restrict__ wordCount /* with wide: {word pairs, of them wide} are added here */) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool w = false, rerun = false;
    if (i < nPairs) {
        vals[i] = i;
        if (fwdKeys[i] != KEY_INVALID) {
            const int mb = minBias[pairQ[i]];
            const int bias = abs(matMin) + abs(mb);
            const bool pre = preWord && preWord[i];
            w = pre || out32[3 * i] + bias >= 255;
            rerun = w && (!wide || pre || out32[3 * i] >= NARROW_EXACT || tasks[i].tL > 65535);
        }
        word[i] = w ? 1 : 0;
        if (wide) wide[i] = rerun ? 1 : 0;
        if (w) tasks[i].segLen = max(1, (tasks[i].n + 15) / 16);
        keys[i] = rerun ? scoreKey(tasks[i].n, tasks[i].tL, usePk ? SCORE_PK_WIDE : SCORE_INT32, wideRowLimit) : KEY_INVALID;
    }
    if (wide) {   // (no thread has returned: the ballots see the whole wavefront)
        const int nw = __popcll(__ballot(w)), nr = __popcll(__ballot(rerun));
        if ((threadIdx.x & (warpSize - 1)) == 0 && nw) {
            atomicAdd(&wordCount[0], (unsigned long long) nw);
            if (nr) atomicAdd(&wordCount[1], (unsigned long long) nr);
        }
    }
}

// gates after the score pass (:389-398) and reverse tasks
__global__ void __launch_bounds__(256)
k_gate_rev(uint32_t nPairs, DevGateParams gp, const uint32_t *__restrict__ pairQ, const uint32_t *__restrict__ pairT,
           const uint64_t *__restrict__ qOff, const uint64_t *__restrict__ tOff, const int32_t *__restrict__ out32,
           const int32_t *__restrict__ out16, const uint8_t *__restrict__ word, const uint32_t *__restrict__ fwdKeys,
           SwTask *__restrict__ tasks, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
           sd_sw_result *__restrict__ res, int usePk,
           const uint8_t *__restrict__ wide /* nullable (k_gate_word): the word pairs that were rerun; null: all of them */,
           int sharedStart /* sd_sw_set_shared_start, packed calls whose tasks are paired by query */) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs) return;
    vals[i] = i;
    keys[i] = KEY_INVALID;
    if (fwdKeys[i] == KEY_INVALID) return;
    // a word pair that was not rerun: pass 1's result is the rerun's, and its start-position task stays in the narrow classes whatever
    // wideRowLimit is -- no cell of a reverse pass exceeds the forward score, which is below NARROW_EXACT
    const bool rerun = wide ? wide[i] != 0 : word[i] != 0;
    const int32_t *src = rerun ? &out16[3 * i] : &out32[3 * i];
    sd_sw_result r = res[i];
    r.score = src[0];
    r.tEnd = src[1];
    r.qEnd = src[2];
    r.flags = word[i] ? 1 : 0;
    if (word[i] && r.tEnd == -1) r.tEnd = 0;   // the word kernel initialises end_ref to 0 (:962)
    if (r.score == 0) r.qEnd = 0;   // no cell scored: the saved column is all zero and the first row matches it (:903-913)
    if (r.tEnd == -1) { res[i] = r; return; }
    const uint64_t qo = qOff[pairQ[i]], to = tOff[pairT[i]];
    const int qL = (int) (qOff[pairQ[i] + 1] - qo), tL = (int) (tOff[pairT[i] + 1] - to);
    const double ev = devEvalue(gp, (double) r.score, (double) qL);
    r.evalue = ev;   // provisional (gate only); the host recomputes it with the reference's arithmetic
    // a result within 1e-9 of the threshold is passed on and decided by the host's exact value
    const bool lowE = ev > gp.evalThr * (1.0 + 1e-9);
    const float qCov = devCov(0, r.qEnd, qL), tCov = devCov(0, r.tEnd, tL);
    const bool lowCov = !devHasCoverage(gp.covThr, gp.covMode, qCov, tCov);
    res[i] = r;
    if (gp.swMode == 0 || lowE || lowCov) return;
    SwTask tk;
    tk.qOff = qo + r.qEnd; tk.tOff = to + r.tEnd;
    tk.n = r.qEnd + 1; tk.tL = r.tEnd + 1; tk.qStep = -1; tk.tStep = -1;
    const int lanes = word[i] ? 16 : 32;
    tk.segLen = max(1, (tk.n + lanes - 1) / lanes);
    tk.slot = i; tk.boundOff = 0;
    // a narrow task of a query in the start form's rows: the class is the query's, the task carries the profile row it begins at
    // (segLen is free: only the int32 kernel reads it as a segment length).  tk.n stays the task's rows (k_cells, k_gate_tb)
    const bool start = sharedStart && usePk && !rerun && scoreClassOf(qL, tk.tL, SCORE_PK_START, 0) >= FIRST_START_CLASS;
    if (start) tk.segLen = qL - 1 - r.qEnd;
    tasks[i] = tk;
    keys[i] = start ? scoreKey(qL, tk.tL, SCORE_PK_START)
                    : scoreKey(tk.n, tk.tL, !usePk ? SCORE_INT32 : (rerun ? SCORE_PK_WIDE : SCORE_PK), gp.wideRowLimit);
}

// traceback task classes: N_TB_NARROW register-band classes by query rows, then three LDS-band classes by band width
// (<=127, <=511, <=2047) and the global-band class for everything wider
// The register-band kernel keeps a task's direction codes (16 B per row), query / bias / target slices in LDS, and
// it is latency bound, so its throughput is its occupancy: classes by query rows keep the LDS request close to what
// the tasks need (a band <= 14 means |tLen - qLen| <= 13, so qCap + 16 target columns always suffice).
// TB_CLASSES is that table for the device (tbKey, tbDirBytes) and the host (the launches of both orchestrations).
// cap: query rows of a register-band class; band cells per row of an LDS-band class, whose widest band is cap - 1; 0: the global class
struct TbClass { int cap; const char *scope; };
constexpr int N_TB_NARROW = 9;
constexpr TbClass TB_CLASSES[] = {
    {128, "sw_traceback.narrow128"}, {192, "sw_traceback.narrow192"}, {256, "sw_traceback.narrow256"},
    {320, "sw_traceback.narrow320"}, {384, "sw_traceback.narrow384"}, {512, "sw_traceback.narrow512"},
    {640, "sw_traceback.narrow640"}, {768, "sw_traceback.narrow768"}, {1024, "sw_traceback.narrow1024"},
    {128, "sw_traceback.lds128"},    {512, "sw_traceback.lds512"},    {2048, "sw_traceback.lds2048"},
    {0, "sw_traceback.global"},
};
constexpr uint32_t N_TB_CLASSES = sizeof(TB_CLASSES) / sizeof(TB_CLASSES[0]), TB_GLOBAL = N_TB_CLASSES - 1;
constexpr uint32_t TBKEY_INVALID = N_TB_CLASSES * 4096u;
constexpr int TB_NARROW_ROWS = TB_CLASSES[N_TB_NARROW - 1].cap;
static_assert(TB_CLASSES[N_TB_NARROW].cap < TB_CLASSES[N_TB_NARROW - 1].cap && TB_CLASSES[TB_GLOBAL].cap == 0, "nine register-band classes first, the global class last");
__host__ __device__ __forceinline__ bool tbNarrow(int band, int qLen, int tLen) { return band * 2 + 3 <= 32 && qLen <= TB_NARROW_ROWS && tLen <= TB_NARROW_ROWS + 13; }
// the class of a task that is not a register-band task
__host__ __device__ __forceinline__ uint32_t tbBandClass(int band) {
    uint32_t ci = N_TB_NARROW;
    while (ci < TB_GLOBAL && band * 2 + 3 > TB_CLASSES[ci].cap - 1) ci++;
    return ci;
}
__device__ __forceinline__ uint32_t tbKey(int band, int qLen, int tLen) {
    if (tbNarrow(band, qLen, tLen)) {
        uint32_t ci = 0;
        while (qLen > TB_CLASSES[ci].cap) ci++;
        // register-band kernel: the two tasks of a wavefront run in lock step through max(attempts) x max(rows).  Tasks with the
        // same number of bands the kernel can try (initial band 1: 1, 2, 4, 8; 2-3: three; 4-7: two; 8-14: one) sit together,
        // most attempts first, longest query first inside
        const int tries = band <= 1 ? 4 : (band <= 3 ? 3 : (band <= 7 ? 2 : 1));
        return ci * 4096u + (uint32_t) (4 - tries) * 1024u + (uint32_t) (1023 - min(max(qLen - 1, 0), 1023));
    }
    const unsigned long long work = (unsigned long long) ((2 * band + 1 + 31) / 32) * (unsigned long long) qLen;
    return tbBandClass(band) * 4096u + (uint32_t) (4095 - (int) min(work >> 3, 4095ull));
}
// global direction scratch (LDS-band kernel only), sized for the widest band of the task's class because the
// kernel keeps doubling the band inside its class
__device__ __forceinline__ uint64_t tbDirBytes(int band, int qLen, int tLen) {
    if (tbNarrow(band, qLen, tLen)) return 0ull;
    const uint32_t ci = tbBandClass(band);
    if (ci == TB_GLOBAL)   // one attempt per round at exactly this band, band arrays in front of the directions
        return (tbGlobalIntBytes(band) + (uint64_t) (band * 2 + 1) * (uint64_t) qLen + 31) & ~15ull;
    return ((uint64_t) (TB_CLASSES[ci].cap - 3) * (uint64_t) qLen + 31) & ~15ull;   // multiples of 16: every task's region stays aligned
}
// the launches of a traceback class, one function per kernel family; PROF follows the query set.  order nullable
void launchTbNarrow(sd_ctx *ctx, const sd_seqset *q, const sd_seqset *t, const int8_t *dMat, int go, int ge, const TbClass &cls, TbTask *dTb,
                    uint32_t cnt, char *dBt, int32_t *dTbRes, const uint32_t *order) {
    const int qCap = cls.cap, tCap = qCap + 16;
    const size_t ldsBytes = 2 * ((size_t) 16 * qCap + 2 * (size_t) qCap + tCap);
    auto *kernel = q->dProf ? sw_traceback_narrow_kernel<true> : sw_traceback_narrow_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((cnt + 1) / 2), dim3(64), ldsBytes, ctx->stream, dTb, cnt, q->dRes, q->dBias, t->dRes, dMat, go, ge, qCap,
                       tCap, dBt, dTbRes, order, (const int8_t *) q->dProf);
}
// an LDS-band class or the global class (band arrays in global scratch, one attempt per round), and the walk through the directions
void launchTbBand(sd_ctx *ctx, const sd_seqset *q, const sd_seqset *t, const int8_t *dMat, int go, int ge, const TbClass &cls,
                  int maxWidthLoop, TbTask *dTb, uint32_t cnt, int8_t *dDir, char *dBt, int32_t *dTbRes, const uint32_t *order) {
    const bool global = cls.cap == 0;
    const int ldsStride = global ? INT_MAX : cls.cap + 1;
    const size_t ldsBytes = global ? 0 : (size_t) 2 * 3 * ldsStride * sizeof(int32_t);
    auto *band = global ? (q->dProf ? sw_traceback_kernel<true, true> : sw_traceback_kernel<false, true>)
                        : (q->dProf ? sw_traceback_kernel<true, false> : sw_traceback_kernel<false, false>);
    hipLaunchKernelGGL(band, dim3((cnt + 1) / 2), dim3(64), ldsBytes, ctx->stream, dTb, cnt, q->dRes, q->dBias, t->dRes, dMat, go, ge, ldsStride,
                       dDir, dBt, dTbRes, order, maxWidthLoop, (const int8_t *) q->dProf);
    auto *walk = global ? sw_traceback_walk_kernel<true> : sw_traceback_walk_kernel<false>;
    hipLaunchKernelGGL(walk, dim3((cnt + 256 / TBW_LANES - 1) / (256 / TBW_LANES)), dim3(256), 0, ctx->stream, dTb, cnt, q->dRes, t->dRes, dDir,
                       dBt, dTbRes, order);
}

// start positions (:475-476), second coverage gate (:483-489) and traceback tasks
__global__ void __launch_bounds__(256)
k_gate_tb(uint32_t nPairs, DevGateParams gp, const uint32_t *__restrict__ pairQ, const uint32_t *__restrict__ pairT,
          const uint64_t *__restrict__ qOff, const uint64_t *__restrict__ tOff, const int32_t *__restrict__ outRev,
          const uint32_t *__restrict__ revKeys, TbTask *__restrict__ tb, uint32_t *__restrict__ keys,
          uint32_t *__restrict__ vals, uint64_t *__restrict__ dirBytes, uint64_t *__restrict__ btBytes,
          sd_sw_result *__restrict__ res, int *__restrict__ errFlag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs) return;
    vals[i] = i;
    keys[i] = TBKEY_INVALID;
    dirBytes[i] = 0;
    btBytes[i] = 0;
    if (revKeys[i] == KEY_INVALID) return;
    sd_sw_result r = res[i];
    if (outRev[3 * i] != r.score) {
        r.flags |= 2;
        res[i] = r;
        atomicExch(errFlag, 1);
        return;
    }
    r.tStart = r.tEnd - outRev[3 * i + 1];
    r.qStart = r.qEnd - outRev[3 * i + 2];
    res[i] = r;
    const uint64_t qo = qOff[pairQ[i]], to = tOff[pairT[i]];
    const int qL = (int) (qOff[pairQ[i] + 1] - qo), tL = (int) (tOff[pairT[i] + 1] - to);
    const float qCov = devCov(r.qStart, r.qEnd, qL), tCov = devCov(r.tStart, r.tEnd, tL);
    const bool lowCov = !devHasCoverage(gp.covThr, gp.covMode, qCov, tCov);
    if (gp.swMode == 1 || lowCov) return;
    TbTask t;
    t.qAbs = qo + r.qStart; t.tAbs = to + r.tStart;
    t.qLen = r.qEnd - r.qStart + 1; t.tLen = r.tEnd - r.tStart + 1;
    t.score = r.score;
    t.band = abs(t.tLen - t.qLen) + 1;
    t.maxv = 0; t.slot = i; t.intOff = 0; t.dirOff = 0; t.btOff = 0;
    tb[i] = t;
    keys[i] = tbKey(t.band, t.qLen, t.tLen);
    dirBytes[i] = tbDirBytes(t.band, t.qLen, t.tLen);
    btBytes[i] = (uint64_t) t.qLen + t.tLen + 2;
}

// this round's tasks: everything whose direction scratch ends inside the budget (prefix of the pending tasks in pair
// order: the first one starts at 0); the others keep their keys and come again
__global__ void __launch_bounds__(256)
k_tb_round(uint32_t nPairs, const uint32_t *__restrict__ keys, const uint64_t *__restrict__ dirOff,
           const uint64_t *__restrict__ dirBytes, uint64_t budget, uint32_t *__restrict__ keysRound) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs) return;
    const uint32_t k = keys[i];
    keysRound[i] = (k != TBKEY_INVALID && dirOff[i] + dirBytes[i] <= budget) ? k : TBKEY_INVALID;
}

__global__ void __launch_bounds__(256)
k_tb_offsets(uint32_t nPairs, const uint32_t *__restrict__ keys, const uint64_t *__restrict__ dirOff,
             const uint64_t *__restrict__ btOff, TbTask *__restrict__ tb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs || keys[i] == TBKEY_INVALID) return;
    tb[i].dirOff = dirOff[i];
    tb[i].btOff = btOff[i];
}

// after a traceback round: finished tasks publish their result, the others double their band (:1492-1493)
__global__ void __launch_bounds__(256)
k_tb_collect(uint32_t nPairs, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals, TbTask *__restrict__ tb,
             const int32_t *__restrict__ tbRes, uint64_t *__restrict__ dirBytes, uint64_t *__restrict__ btLenOut,
             sd_sw_result *__restrict__ res, int *__restrict__ errFlag, int maxBand,
             const uint32_t *__restrict__ keysRound /* what this round ran: deferred tasks keep key and scratch size */) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs) return;
    vals[i] = i;
    if (keys[i] == TBKEY_INVALID) { dirBytes[i] = 0; return; }
    if (keysRound[i] == TBKEY_INVALID) return;
    const int len = tbRes[2 * i];
    if (len == -2) {
        const int band = tb[i].band;   // already doubled by the kernel that gave up
        // the full rectangle is inside the band once band >= max(qLen, tLen): a task that still misses its score then is
        // a traceback error, not a reason to double again
        if (band > maxBand) { atomicExch(errFlag, 2); keys[i] = TBKEY_INVALID; dirBytes[i] = 0; return; }
        keys[i] = tbKey(band, tb[i].qLen, tb[i].tLen);
        dirBytes[i] = tbDirBytes(band, tb[i].qLen, tb[i].tLen);
    } else if (len < 0) {
        atomicExch(errFlag, 2);
        keys[i] = TBKEY_INVALID;
        dirBytes[i] = 0;
    } else {
        res[i].btLen = len;
        res[i].identical = tbRes[2 * i + 1];
        btLenOut[i] = (uint64_t) len;
        keys[i] = TBKEY_INVALID;
        dirBytes[i] = 0;
    }
}

__global__ void __launch_bounds__(256)
k_bt_pack(uint32_t nPairs, const uint64_t *__restrict__ btLen, const uint64_t *__restrict__ dense,
          const TbTask *__restrict__ tb, const char *__restrict__ bt, char *__restrict__ pool, uint64_t poolBase,
          sd_sw_result *__restrict__ res) {
    // one wavefront per pair copies its backtrace into the dense pool
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= nPairs) return;
    const uint64_t len = btLen[i];
    if (len == 0) return;
    const char *src = bt + tb[i].btOff + ((uint64_t) (tb[i].qLen + tb[i].tLen + 2) - len);   // written backwards from the end
    char *dst = pool + dense[i];
    for (uint64_t x = lane; x < len; x += 64) dst[x] = src[x];
    if (lane == 0) res[i].btOffset = poolBase + dense[i];
}

// ---- Matcher::compressAlignment on the device (M/src/alignment/Matcher.cpp:166-185; sd_sw_set_cigar_pool): the run-length text
// of a backtrace -- "57M2I103M" -- instead of its letters.  State 'M' with a count of 0 at the start (a backtrace that does not begin
// with a match begins "0M"), every run as decimal count + letter.  One wavefront per pair, 64 letters per step: a lane whose right
// neighbour differs ends a run, the run began at the last lane at or below it whose left neighbour differs (a ballot; the last start
// of the earlier steps is carried), and a scan of the text lengths of the step's runs places them.  WRITE = false: the text's length
// only (the pool offsets are a scan of these), WRITE = true: the text, the record's offset and -- flags bits 8.. -- its length.
template <bool WRITE>
__global__ void __launch_bounds__(256)
k_bt_cigar(uint32_t nPairs, const uint64_t *__restrict__ btLen, const uint64_t *__restrict__ dense, const TbTask *__restrict__ tb,
           const char *__restrict__ bt, char *__restrict__ pool, uint64_t *__restrict__ cigLen, sd_sw_result *__restrict__ res) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= nPairs) return;
    const uint32_t len = (uint32_t) btLen[i];
    if (len == 0) {
        if (!WRITE && lane == 0) cigLen[i] = 0;
        return;
    }
    const char *src = bt + tb[i].btOff + ((uint64_t) (tb[i].qLen + tb[i].tLen + 2) - len);   // written backwards from the end
    char *dst = WRITE ? pool + dense[i] : nullptr;
    uint32_t out = 0;
    uint32_t runStart = 0;
    int left = src[0];   // the letter in front of the step's first one (in front of the first letter: itself, position 0 starts a run anyway)
    if (left != 'M') {
        if (WRITE && lane == 0) {
            dst[0] = '0';
            dst[1] = 'M';
        }
        out = 2;
    }
    for (uint32_t base = 0; base < len; base += 64) {
        const uint32_t x = base + (uint32_t) lane;
        const bool valid = x < len;
        const int c = valid ? (int) src[x] : -1;
        const int after = base + 64 < len ? (int) src[base + 64] : -2;   // the letter behind the step's last one (or the end)
        int prv = __shfl_up(c, 1, 64);
        if (lane == 0) prv = left;
        int nxt = __shfl_down(c, 1, 64);
        if (lane == 63) nxt = after;
        if (valid && x + 1 == len) nxt = -2;
        const bool isStart = valid && (x == 0 || prv != c);
        const bool isEnd = valid && nxt != c;
        const unsigned long long starts = __ballot(isStart);
        const unsigned long long mine = starts & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const uint32_t from = mine ? base + (uint32_t) (63 - __clzll((long long) mine)) : runStart;
        uint32_t count = 0, nd = 0;
        if (isEnd) {
            count = x - from + 1;
            nd = count < 10 ? 1 : count < 100 ? 2 : count < 1000 ? 3 : count < 10000 ? 4 : count < 100000 ? 5 : count < 1000000 ? 6 : 7;
        }
        uint32_t incl = isEnd ? nd + 1 : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (WRITE && isEnd) {
            char *o = dst + out + incl - 1;   // the run's letter; the digits go in front of it
            *o = (char) c;
            uint32_t v = count;
            for (uint32_t d = 0; d < nd; d++) {
                *--o = (char) ('0' + v % 10);
                v /= 10;
            }
        }
        out += __shfl(incl, 63, 64);
        if (starts) runStart = base + (uint32_t) (63 - __clzll((long long) starts));
        left = __shfl(c, 63, 64);
    }
    if (lane == 0) {
        if (WRITE) {
            res[i].btOffset = dense[i];
            res[i].flags = (res[i].flags & 0xFF) | (int32_t) (out << 8);
        } else {
            cigLen[i] = out;
        }
    }
}

// ---- besthitbyset on the device (sd_sw_align_batch_best_by_group).  Matcher::compareHits orders a query's accepted alignments by
// E-value, rounded bit score, target length, target key; for one query the E-value is a strictly decreasing function of the score
// and the bit score a function of it, so the first of a (query, target set) cell is the maximum of
//   score << 44 | (0xFFFF - target length) << 28 | (0x0FFFFFFF - key)
// over the cell's accepted pairs: one atomic maximum per pair into a table of queries x target sets, then a second look.
// "Strictly decreasing" ends where the double does: K m n exp(-lambda S) is 0.0 from a raw score of ~2 700 on (about 520
// identical residues: two near-identical paralogs of a long protein in one target genome) and collides in the last
// subnormals below that, and compareHits then decides by the ROUNDED bit score (0.39 bit per score unit: neighbouring scores
// tie), the shorter target, the smaller key -- not by the raw score.  So every accepted pair whose E-value is below
// BB_EVAL_EXACT (far above the first subnormal, far below anything two different scores can share) is kept whatever the
// cell's maximum is, and the host's selection -- compareHits itself -- decides among them as it does without the device's
// help; a pair above the bound can only lose to them (smaller score) and is dropped as before.
constexpr double BB_EVAL_EXACT = 1e-290;
struct BestByGroup {
    const uint32_t *groupOf, *groupKey;   // per target sequence (groupKey nullable: the index)
    uint32_t nGroups;
    float seqIdThr, covThr;
    int alnLenThr, covMode;
    double evalThr;
    double evalExact;   // BB_EVAL_EXACT (SD_BEST_EXACT=0 in the environment: 0.0, the round-5 behaviour, for the A/B of the test)
};
__device__ __forceinline__ float bbCov(uint32_t startPos, uint32_t endPos, uint32_t len) {   // sd::computeCov (Util::computeCov)
    return (float) (min(len, max(startPos, endPos)) - min(startPos, endPos) + 1u) / (float) len;
}
__device__ __forceinline__ bool bbAccepted(const sd_sw_result &r, const BestByGroup &B, uint32_t qL, uint32_t tL) {
    if (r.btLen <= 0 || r.qStart < 0 || r.tStart < 0) return false;   // stopped at a gate
    const float qcov = bbCov((uint32_t) r.qStart, (uint32_t) r.qEnd, qL), dbcov = bbCov((uint32_t) r.tStart, (uint32_t) r.tEnd, tL);
    const float seqId = (float) r.identical / (float) r.btLen;
    bool cov = true;
    if (B.covMode == 0) cov = qcov >= B.covThr && dbcov >= B.covThr;
    else if (B.covMode == 2) cov = qcov >= B.covThr;
    else if (B.covMode == 1) cov = dbcov >= B.covThr;
    // (the device's E-value stands within 1e-15 of the host's: a pair inside that band of the threshold is the worst of its cell
    // and can only be the maximum where nothing better exists, so keeping it costs a record and never displaces one)
    return r.evalue <= B.evalThr * (1.0 + 1e-9) && seqId >= B.seqIdThr && cov && r.btLen >= B.alnLenThr;
}
__device__ __forceinline__ unsigned long long bbPack(const sd_sw_result &r, uint32_t tL, uint32_t key) {
    return ((unsigned long long) min((uint32_t) r.score, 0xFFFFFu) << 44) | ((unsigned long long) (0xFFFFu - min(tL, 0xFFFFu)) << 28) |
           (unsigned long long) (0x0FFFFFFFu - min(key, 0x0FFFFFFFu));
}
__global__ void __launch_bounds__(256)
k_best_mark(uint32_t nPairs, const sd_sw_result *__restrict__ res, const uint8_t *__restrict__ ident, const uint32_t *__restrict__ pq,
            const uint32_t *__restrict__ pt, const uint64_t *__restrict__ qOff, const uint64_t *__restrict__ tOff, BestByGroup B,
            unsigned long long *__restrict__ table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs || ident[i]) return;
    const uint32_t q = pq[i], t = pt[i];
    const uint32_t qL = (uint32_t) (qOff[q + 1] - qOff[q]), tL = (uint32_t) (tOff[t + 1] - tOff[t]);
    const sd_sw_result r = res[i];
    if (!bbAccepted(r, B, qL, tL)) return;
    atomicMax(&table[(size_t) q * B.nGroups + B.groupOf[t]], bbPack(r, tL, B.groupKey ? B.groupKey[t] : t));
}
// a pair that is neither an identity pair nor the first of its cell leaves no record and no backtrace
__global__ void __launch_bounds__(256)
k_best_keep(uint32_t nPairs, sd_sw_result *__restrict__ res, const uint8_t *__restrict__ ident, const uint32_t *__restrict__ pq,
            const uint32_t *__restrict__ pt, const uint64_t *__restrict__ qOff, const uint64_t *__restrict__ tOff, BestByGroup B,
            const unsigned long long *__restrict__ table, uint64_t *__restrict__ btLen) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs || ident[i]) return;
    const uint32_t q = pq[i], t = pt[i];
    const uint32_t qL = (uint32_t) (qOff[q + 1] - qOff[q]), tL = (uint32_t) (tOff[t + 1] - tOff[t]);
    const sd_sw_result r = res[i];
    const bool keep = bbAccepted(r, B, qL, tL) &&
                      (r.evalue < B.evalExact || table[(size_t) q * B.nGroups + B.groupOf[t]] == bbPack(r, tL, B.groupKey ? B.groupKey[t] : t));
    if (!keep) {
        res[i].btLen = 0;
        btLen[i] = 0;
    }
}

// compact mode: which records go back to the host
__global__ void __launch_bounds__(256)
k_accept(uint32_t nPairs, const sd_sw_result *__restrict__ res, const uint8_t *__restrict__ ident, uint8_t *__restrict__ acc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs) return;
    const sd_sw_result &r = res[i];
    acc[i] = (ident[i] || (r.btLen > 0 && r.qStart >= 0 && r.tStart >= 0)) ? 1 : 0;
}
__global__ void __launch_bounds__(256)
k_accept_compact(uint32_t nPairs, const sd_sw_result *__restrict__ res, const uint8_t *__restrict__ acc,
                 const uint64_t *__restrict__ pos, sd_sw_result *__restrict__ outRes, uint32_t *__restrict__ outIdx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs || !acc[i]) return;
    outRes[pos[i]] = res[i];
    outIdx[pos[i]] = i;
}
// device-wide scans and the radix sort of the task keys: this library's own kernels (sd_scan_sort.h), 256-thread workgroups
// without inter-workgroup waiting -- they run between the score wavefronts of the other lanes
#include "sd_scan_sort.h"

__global__ void __launch_bounds__(256)
k_bound_need(uint32_t nPairs, const SwTask *__restrict__ tasks, const uint32_t *__restrict__ keys, uint64_t *__restrict__ need) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs) return;
    // units of uint2: the packed kernel hands over 16 bytes per column (strips of 512 rows beyond 768 rows), the
    // int32 kernel 8 bytes (strips of 1024 rows)
    uint64_t v = 0;
    if (keys[i] != KEY_INVALID) {
        const uint32_t ci = keys[i] >> 10;
        constexpr uint64_t TWO = scoreBoundMask(2), ONE = scoreBoundMask(1);   // (the classes of SCORE_CLASSES with that boundNeed)
        if ((TWO >> ci) & 1) v = 2ull * (uint64_t) tasks[i].tL;
        else if (((ONE >> ci) & 1) && tasks[i].n > I32_STRIP_ROWS) v = (uint64_t) tasks[i].tL;
    }
    need[i] = v;
}
__global__ void __launch_bounds__(256)
k_bound_apply(uint32_t nPairs, SwTask *__restrict__ tasks, const uint64_t *__restrict__ off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPairs) return;
    tasks[i].boundOff = off[i];
}

// ---- tasks of one query two by two (shared-profile kernels) --------------------------------------------------------
// key = class (6 bits) | query (17 bits) | target-length bucket (9 bits): one stable sort puts the tasks of a
// (class, query) run together, longest target first; inside a run of a packed class consecutive tasks form pairs, an
// odd last task stays alone.  Invalid tasks sort last (all ones).
constexpr uint32_t PAIR_NONE = 0xFFFFFFFFu;
constexpr int PAIR_QUERY_BITS = 17;
// The classes whose tasks are paired.  Forward passes: every packed class.  The start-position pass (startOnly): the start
// form's classes alone -- its other tasks scan per-pair prefixes, have no profile to share and keep the plain order.
__host__ __device__ __forceinline__ bool pairedClass(uint32_t ci, int startOnly) {
    return startOnly ? ci >= FIRST_START_CLASS && ci < N_SCORE_CLASSES : ci < FIRST_INT32_CLASS;
}
// Pairs per wavefront of a paired class (declared above launchScorePkAligned): a (class, query) run is padded to a multiple of it
constexpr __host__ __device__ uint32_t pairsPerWave(uint32_t ci, int startOnly, int group16) {
    return group16 && !startOnly && ci >= alignedClass(5) && ci <= alignedClass(GROUP16_ROWS_MAX / 32) ? 4u : 2u;
}
static_assert(SCORE_CLASSES[alignedClass(5)].form == SCORE_PK && SCORE_CLASSES[alignedClass(5)].rows == 5 * 32 &&
              SCORE_CLASSES[alignedClass(24)].form == SCORE_PK && SCORE_CLASSES[alignedClass(24)].rows == 24 * 32,
              "alignedClass: a_seg5 .. a_seg24 are the classes 1 .. 20");
__global__ void __launch_bounds__(256)
k_pair_keys(uint32_t n, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ pairQ, uint32_t *__restrict__ key2, int startOnly) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    // class (6 bits) | query (17 bits) | target length code (9 bits): invalid entries sort behind the last class
    uint32_t v = k == KEY_INVALID ? 0xFFFFFFFFu : ((k >> 10) << 26) | (pairQ[i] << 9) | ((k & 1023u) >> 1);
    // startOnly, unpaired classes: class | the ten bits of the target length code, i.e. the order of the plain sort of `keys`
    if (startOnly && k != KEY_INVALID && !pairedClass(k >> 10, startOnly)) v = ((k >> 10) << 26) | ((k & 1023u) << 16);
    key2[i] = v;
}
__global__ void __launch_bounds__(256)
k_pair_heads(uint32_t n, const uint32_t *__restrict__ keyS, uint32_t *__restrict__ headPos) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const bool head = p == 0 || (keyS[p] >> 9) != (keyS[p - 1] >> 9);
    headPos[p] = head ? p : 0u;
}
// leader[p] = pairs that start at sorted position p: 1 for every second task of a (class, query) run; the run's last task adds
// the EMPTY pairs that fill the run up to whole wavefronts (pairsPerWave: two pairs, or four on 16-lane groups), so that every
// wavefront stays inside one query (sw_score_pk_aligned_kernel<.., SHARED = true>: one profile per wavefront)
__global__ void __launch_bounds__(256)
k_pair_leaders(uint32_t n, const uint32_t *__restrict__ keyS, const uint32_t *__restrict__ runStart, uint8_t *__restrict__ leader,
               int startOnly, int group16) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    uint8_t v = 0;
    if (p < n && pairedClass(keyS[p] >> 26, startOnly)) {
        const uint32_t o = p - runStart[p];
        v = (o & 1u) == 0 ? 1 : 0;
        const bool lastOfRun = p + 1 >= n || (keyS[p + 1] >> 9) != (keyS[p] >> 9);
        const uint32_t pairs = (o + 1 + 1) / 2;   // pairs of the run = ceil((o + 1) / 2)
        const uint32_t ppw = pairsPerWave(keyS[p] >> 26, startOnly, group16);
        if (lastOfRun) v += (uint8_t) ((ppw - pairs % ppw) % ppw);
    }
    leader[p] = v;
}
__global__ void __launch_bounds__(256)
k_pair_emit(uint32_t n, const uint32_t *__restrict__ keyS, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ runStartOf,
            const uint64_t *__restrict__ pairIdx, uint32_t *__restrict__ order2, int startOnly) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || !pairedClass(keyS[p] >> 26, startOnly) || ((p - runStartOf[p]) & 1u)) return;   // the first task of every pair (paired classes) writes it
    const uint64_t w = pairIdx[p];
    order2[2 * w] = vals[p];
    const bool mate = p + 1 < n && (keyS[p + 1] >> 9) == (keyS[p] >> 9);
    order2[2 * w + 1] = mate ? vals[p + 1] : PAIR_NONE;
}
// pair-index boundaries of the classes: b[c] = number of pairs of classes < c
__global__ void k_pair_bounds(const uint32_t *__restrict__ keyS, uint32_t n, const uint64_t *__restrict__ pairIdx,
                              uint32_t *__restrict__ b, int nb) {
    const int c = threadIdx.x;
    if (c >= nb) return;
    const uint32_t want = (uint32_t) c << 26;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keyS[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    b[c] = (uint32_t) pairIdx[lo];
}

// the workspace of one alignBatchImpl call (alignWsInit)
struct AlignWs {
    size_t N;
    unsigned grid;
    int8_t *dMat;
    uint32_t *dPQ, *dPT, *dKeys, *dVals, *dKeysS, *dOrder, *dBounds, *dFwdKeys, *dRevKeys;
    uint8_t *dIdent, *dWord;
    int32_t *dMinBias, *dOut32, *dOut16, *dOutRev, *dTbRes;
    int *dErr;
    SwTask *dTasks;
    TbTask *dTb;
    sd_sw_result *dRes;
    uint64_t *dScanA, *dScanB, *dDirBytes, *dDirOff, *dBtBytes, *dBtOff, *dBtLen, *dDense;
    unsigned long long *dCells;
    char *dBt;   // backtrace scratch of the traceback tasks (sized after k_gate_tb)
};

// sort (keys,vals) -> order, read the class boundaries, launch the kernel of every class that has a task (SCORE_CLASSES)
int devRunScore(sd_ctx *ctx, const AlignWs &w, uint32_t nPairs, const uint32_t *dKeys, const sd_seqset *q, const sd_seqset *t, int go, int ge,
                int32_t *dOut, const uint32_t *dPairQ /* non-null: pair the tasks of the paired classes by query */,
                int startOnly = 0 /* pairedClass: the start-position pass pairs the start form's classes only */) {
    const uint32_t *dOrder = w.dOrder;
    const unsigned grid = (nPairs + 255) / 256;
    int rc = SD_OK;
    uint32_t *dOrder2 = nullptr, *dPairBounds = nullptr;
    if (dPairQ) {
        // one sort serves both the pairing of the packed classes and the plain order of the int32 classes
        uint32_t *dKey2 = nullptr, *dVals2 = nullptr, *dHead = nullptr, *dRunStart = nullptr;
        uint64_t *dPairIdx = nullptr;
        uint8_t *dLeader = nullptr;
        SD_HIP(ctx, wsGet(ctx, "sp.key2", (size_t) nPairs, &dKey2));
        SD_HIP(ctx, wsGet(ctx, "sp.vals2", (size_t) nPairs, &dVals2));
        SD_HIP(ctx, wsGet(ctx, "sp.head", (size_t) nPairs, &dHead));
        SD_HIP(ctx, wsGet(ctx, "sp.runstart", (size_t) nPairs, &dRunStart));
        SD_HIP(ctx, wsGet(ctx, "sp.leader", (size_t) nPairs + 1, &dLeader));
        SD_HIP(ctx, wsGet(ctx, "sp.pairidx", (size_t) nPairs + 1, &dPairIdx));
        const size_t order2Cap = (size_t) 8 * nPairs + 16;   // worst case: every run one task, padded to a wavefront (four pairs)
        SD_HIP(ctx, wsGet(ctx, "sp.order2", order2Cap, &dOrder2));
        SD_HIP(ctx, hipMemsetAsync(dOrder2, 0xFF, order2Cap * sizeof(uint32_t), ctx->stream));   // empty pairs: PAIR_NONE
        SD_HIP(ctx, wsGet(ctx, "sp.bounds", 64, &dPairBounds));
        hipLaunchKernelGGL(k_pair_keys, dim3(grid), dim3(256), 0, ctx->stream, nPairs, dKeys, dPairQ, dKey2, startOnly);
        rc = sdCtxSortPairs(ctx, "al.sort", dKey2, w.dKeysS, w.dVals, dVals2, nPairs, 32);
        if (rc != SD_OK) return rc;
        dOrder = dVals2;
        hipLaunchKernelGGL(k_pair_heads, dim3(grid), dim3(256), 0, ctx->stream, nPairs, w.dKeysS, dHead);
        rc = sdCtxInclusiveMax(ctx, "al.scantmp32", dHead, dRunStart, nPairs);
        if (rc != SD_OK) return rc;
        hipLaunchKernelGGL(k_pair_leaders, dim3((nPairs + 256) / 256), dim3(256), 0, ctx->stream, nPairs, w.dKeysS, dRunStart, dLeader, startOnly,
                           ctx->group16 ? 1 : 0);
        rc = sdCtxExclusiveScan(ctx, "al.scantmp", (const uint8_t *) dLeader, dPairIdx, (size_t) nPairs + 1);
        if (rc != SD_OK) return rc;
        hipLaunchKernelGGL(k_pair_emit, dim3(grid), dim3(256), 0, ctx->stream, nPairs, w.dKeysS, dVals2, dRunStart, dPairIdx, dOrder2, startOnly);
        hipLaunchKernelGGL(k_pair_bounds, dim3(1), dim3(64), 0, ctx->stream, w.dKeysS, nPairs, dPairIdx, dPairBounds,
                           (int) N_SCORE_CLASSES + 1);
        hipLaunchKernelGGL(k_bounds, dim3(1), dim3(64), 0, ctx->stream, w.dKeysS, nPairs, 1u << 26, w.dBounds, (int) N_SCORE_CLASSES + 1);
    } else {
        rc = sdCtxSortPairs(ctx, "al.sort", dKeys, w.dKeysS, w.dVals, w.dOrder, nPairs, 16);
        if (rc != SD_OK) return rc;
        hipLaunchKernelGGL(k_bounds, dim3(1), dim3(64), 0, ctx->stream, w.dKeysS, nPairs, 1024u, w.dBounds, (int) N_SCORE_CLASSES + 1);
    }
    // strip hand-off workspace for queries longer than one 1024-row strip
    hipLaunchKernelGGL(k_bound_need, dim3(grid), dim3(256), 0, ctx->stream, nPairs, w.dTasks, dKeys, w.dScanA);
    SD_HIP(ctx, hipMemsetAsync(w.dScanA + nPairs, 0, sizeof(uint64_t), ctx->stream));
    rc = sdCtxExclusiveScan(ctx, "al.scantmp", w.dScanA, w.dScanB, (size_t) nPairs + 1);
    if (rc != SD_OK) return rc;
    hipLaunchKernelGGL(k_bound_apply, dim3(grid), dim3(256), 0, ctx->stream, nPairs, w.dTasks, w.dScanB);
    uint32_t hb[N_SCORE_CLASSES + 1], hpb[N_SCORE_CLASSES + 1];
    uint64_t boundTotal = 0;
    if (dPairQ) SD_HIP(ctx, sdD2H(ctx, hpb, dPairBounds, sizeof(hpb)));
    SD_HIP(ctx, sdD2H(ctx, hb, w.dBounds, sizeof(hb)));
    SD_HIP(ctx, sdD2H(ctx, &boundTotal, w.dScanB + nPairs, sizeof(uint64_t)));
    SD_HIP(ctx, sdStreamSync(ctx));
    uint2 *dBound = nullptr;
    SD_HIP(ctx, wsGet(ctx, "sw.bound", std::max<uint64_t>(boundTotal, 1), &dBound));
    for (uint32_t ci = 0; ci < N_SCORE_CLASSES; ci++) {
        const uint32_t begin = hb[ci], cnt = hb[ci + 1] - hb[ci];
        if (cnt == 0) continue;
        const bool shared = dPairQ != nullptr && pairedClass(ci, startOnly);
        const ScoreSide &side = shared ? SCORE_CLASSES[ci].shared : SCORE_CLASSES[ci].unshared;
        ProfScope ps(ctx, side.scope);
        if (shared)   // explicit pairs: two entries per pair of the class
            side.launch(ctx, w.dTasks, dOrder2 + 2 * (size_t) hpb[ci], 2 * (hpb[ci + 1] - hpb[ci]), q, t, w.dMat, go, ge, dOut, dBound);
        else
            side.launch(ctx, w.dTasks, dOrder + begin, cnt, q, t, w.dMat, go, ge, dOut, dBound);
    }
    SD_HIP(ctx, hipGetLastError());
    return SD_OK;
}

__global__ void __launch_bounds__(256)
k_cells(uint32_t nPairs, const SwTask *__restrict__ tasks, const uint32_t *__restrict__ keys, unsigned long long *__restrict__ acc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long c = 0;
    if (i < nPairs && keys[i] != KEY_INVALID) c = (unsigned long long) tasks[i].n * (unsigned long long) tasks[i].tL;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(acc, c);
}

}  // namespace

// =============================================================================================
int sdFail(sd_ctx *ctx, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->lastError = buf;
    else fprintf(stderr, "spacedust_gpu: %s\n", buf);
    return code;
}

extern "C" {

int sd_ctx_create(int device, sd_ctx **out) { return sd_ctx_create_prio(device, 0, out); }

int sd_ctx_create_prio(int device, int priority, sd_ctx **out) { return sd_ctx_create_masked(device, priority, 0, out); }

int sd_ctx_create_masked(int device, int priority, int reserveCUs, sd_ctx **out) {
    if (out == nullptr) return SD_EINVAL;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        fprintf(stderr, "spacedust_gpu: no HIP device visible (%s); this library has no CPU fallback\n",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        return SD_ENODEVICE;
    }
    if (device < 0 || device >= count) return SD_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return SD_ENODEVICE;
    sd_ctx *c = new sd_ctx();
    c->device = device;
    int least = 0, greatest = 0;   // numerically: least priority >= greatest priority
    (void) hipDeviceGetStreamPriorityRange(&least, &greatest);
    const int prio = priority < 0 ? greatest : (priority > 0 ? least : (least + greatest) / 2);
    hipError_t se = hipSuccess;
    (void) hipGetDeviceProperties(&c->prop, device);
    const int nCU = c->prop.multiProcessorCount;
    if (reserveCUs > 0 && nCU > 0 && reserveCUs < nCU) {
        // the queue's CU mask: the driver deals the bits round the XCDs (bit i -> XCD i mod 8), so clearing the top bits takes the
        // same number of CUs from every XCD.  (A masked stream has the default priority: the masked-stream call takes none.)
        std::vector<uint32_t> mask((size_t) (nCU + 31) / 32, 0u);
        for (int b = 0; b < nCU - reserveCUs; b++) mask[(size_t) b / 32] |= 1u << (b % 32);
        se = hipExtStreamCreateWithCUMask(&c->stream, (uint32_t) mask.size(), mask.data());
    } else {
        se = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio);
    }
    if (se != hipSuccess) {
        delete c;
        return SD_EHIP;
    }
    // SD_SYNC=spin keeps hipStreamSynchronize's busy wait (lowest wake-up latency, one core per waiting thread)
    const char *syncMode = getenv("SD_SYNC");
    const bool spin = syncMode && strcmp(syncMode, "spin") == 0;
    (void) hipEventCreate(&c->evStart);
    (void) hipEventCreate(&c->evStop);
    if (!spin) (void) hipEventCreateWithFlags(&c->evSync, hipEventDisableTiming);
    (void) hipGetDeviceProperties(&c->prop, device);
    *out = c;
    return SD_OK;
}

void sd_ctx_destroy(sd_ctx *ctx) {
    if (!ctx) return;
    (void) hipSetDevice(ctx->device);
    if (ctx->evStart) (void) hipEventDestroy(ctx->evStart);
    if (ctx->evStop) (void) hipEventDestroy(ctx->evStop);
    if (ctx->evSync) (void) hipEventDestroy(ctx->evSync);
    for (auto &pp : ctx->profPending) {
        (void) hipEventDestroy(pp.a);
        (void) hipEventDestroy(pp.b);
    }
    for (hipEvent_t e : ctx->evPool) (void) hipEventDestroy(e);
    if (ctx->stream) (void) hipStreamDestroy(ctx->stream);
    for (auto &kv : ctx->ws) if (kv.second.p) (void) hipFree(kv.second.p);
    for (auto &b : ctx->pool) if (b.p) (void) hipFree(b.p);
    for (auto &kv : ctx->pinned) if (kv.second.p) (void) hipHostFree(kv.second.p);
    for (auto &b : ctx->bounce) if (b.p) (void) hipHostFree(b.p);
    delete ctx;
}

const char *sd_last_error(sd_ctx *ctx) { return ctx ? ctx->lastError.c_str() : "no context"; }

int sd_device_memory(sd_ctx *ctx, uint64_t *freeBytes, uint64_t *totalBytes) {
    if (!ctx) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    size_t f = 0, t = 0;
    SD_HIP(ctx, hipMemGetInfo(&f, &t));
    if (freeBytes) *freeBytes = f;
    if (totalBytes) *totalBytes = t;
    return SD_OK;
}

int sd_workspace_report(sd_ctx *ctx, uint64_t *deviceBytes, uint64_t *pinnedBytes, char *buf, size_t cap) {
    if (!ctx) return SD_EINVAL;
    uint64_t dev = 0, pin = 0;
    std::vector<std::pair<size_t, std::string> > rows;
    for (auto &kv : ctx->ws) {
        dev += kv.second.bytes;
        rows.push_back(std::make_pair(kv.second.bytes, kv.first));
    }
    for (auto &kv : ctx->pinned) pin += kv.second.bytes;
    const size_t pooled = poolBytes(ctx);   // device buffers of destroyed sequence sets kept for the next one (poolPut)
    if (pooled) {
        dev += pooled;
        rows.push_back(std::make_pair(pooled, std::string("pool(seqset buffers)")));
    }
    if (deviceBytes) *deviceBytes = dev;
    if (pinnedBytes) *pinnedBytes = pin;
    if (buf && cap) {
        std::sort(rows.begin(), rows.end(), [](const std::pair<size_t, std::string> &a, const std::pair<size_t, std::string> &b) { return a.first > b.first; });
        std::string s;
        for (auto &r : rows) s += r.second + " " + std::to_string(r.first) + "\n";
        snprintf(buf, cap, "%s", s.c_str());
    }
    return SD_OK;
}

int sd_workspace_release(sd_ctx *ctx) {
    if (!ctx) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    SD_HIP(ctx, sdStreamSync(ctx));
    for (auto &kv : ctx->ws)
        if (kv.second.p) (void) hipFree(kv.second.p);
    ctx->ws.clear();
    {
        std::lock_guard<std::mutex> lock(ctx->poolMutex);
        for (auto &b : ctx->pool)
            if (b.p) (void) hipFree(b.p);
        ctx->pool.clear();
    }
    ctx->biasTablesUploaded = false;
    return SD_OK;
}

// identity of a physical GPU across processes and nodes: FNV-1a of the host name and the device's PCI bus id
int sd_device_identity(int device, uint64_t *id) {
    if (!id) return SD_EINVAL;
    char host[256] = {0}, bus[64] = {0};
    (void) gethostname(host, sizeof(host) - 1);
    if (hipDeviceGetPCIBusId(bus, (int) sizeof(bus), device) != hipSuccess) return SD_ENODEVICE;
    uint64_t h = 1469598103934665603ull;
    for (const char *p = host; *p; p++) h = (h ^ (uint8_t) *p) * 1099511628211ull;
    h = (h ^ 0xFFu) * 1099511628211ull;
    for (const char *p = bus; *p; p++) h = (h ^ (uint8_t) *p) * 1099511628211ull;
    *id = h;
    return SD_OK;
}

int sd_device_name(sd_ctx *ctx, char *buf, size_t cap) {
    if (!ctx || !buf || cap == 0) return SD_EINVAL;
    snprintf(buf, cap, "%s (%s, %d CUs)", ctx->prop.name, ctx->prop.gcnArchName, ctx->prop.multiProcessorCount);
    return SD_OK;
}

int sd_synchronize(sd_ctx *ctx) {
    SD_HIP(ctx, sdStreamSync(ctx));
    return SD_OK;
}

int sd_profile_enable(sd_ctx *ctx, int on) {
    ctx->profiling = on != 0;
    return SD_OK;
}
int sd_profile_reset(sd_ctx *ctx) {
    sdProfDrain(ctx, true);
    ctx->profile.clear();
    return SD_OK;
}
int sd_profile_get(sd_ctx *ctx, const char *name, double *totalMs, uint64_t *launches) {
    sdProfDrain(ctx, true);
    auto it = ctx->profile.find(name);
    if (it == ctx->profile.end()) {
        *totalMs = 0;
        *launches = 0;
        return SD_OK;
    }
    *totalMs = it->second.ms;
    *launches = it->second.launches;
    return SD_OK;
}
int sd_profile_names(sd_ctx *ctx, char *buf, size_t cap) {
    sdProfDrain(ctx, true);
    std::string s;
    for (auto &kv : ctx->profile) {
        if (!s.empty()) s += ",";
        s += kv.first;
    }
    snprintf(buf, cap, "%s", s.c_str());
    return SD_OK;
}

int sd_seqset_create(sd_ctx *ctx, const uint8_t *residues, const uint64_t *offsets, uint32_t n, const int8_t *swCompBias,
                     sd_seqset **out) {
    if (!ctx || !residues || !offsets || !out) return SD_EINVAL;
    for (uint32_t i = 0; i < n; i++)
        if (offsets[i + 1] - offsets[i] > 65535)
            return sdFail(ctx, SD_EINVAL, "sequence %u has %llu residues; the limit is 65535 (--max-seq-len)", i,
                          (unsigned long long) (offsets[i + 1] - offsets[i]));
    (void) hipSetDevice(ctx->device);
    sd_seqset *s = new sd_seqset();
    s->ctx = ctx;
    s->n = n;
    s->total = offsets[n];
    s->hOff.assign(offsets, offsets + n + 1);
    s->hRes.assign(residues, residues + s->total);
    if (swCompBias) s->hBias.assign(swCompBias, swCompBias + s->total);
    else s->hBias.assign(s->total, 0);
    s->hMinBias.assign(n, 0);
    s->maxEntryAdd = 0;
    if (swCompBias) {   // (a set without a bias -- the target side, 9 * 10^8 residues at 1 000 proteomes -- has nothing to scan)
        int mx = 0;
#pragma omp parallel for schedule(static) reduction(max : mx)
        for (uint32_t i = 0; i < n; i++) {
            int m = 0;
            for (uint64_t x = offsets[i]; x < offsets[i + 1]; x++) {
                m = std::min(m, (int) swCompBias[x]);
                mx = std::max(mx, (int) swCompBias[x]);
            }
            s->hMinBias[i] = m;
        }
        s->maxEntryAdd = mx;
    }
    const size_t pad = 64;
    if (poolGet(ctx, s->total + pad, (void **) &s->dRes, &s->bRes) != hipSuccess ||
        poolGet(ctx, s->total + pad, (void **) &s->dBias, &s->bBias) != hipSuccess ||
        poolGet(ctx, (n + 1) * sizeof(uint64_t), (void **) &s->dOff, &s->bOff) != hipSuccess) {
        (void) hipGetLastError();
        sd_seqset_destroy(s);
        return sdFail(ctx, SD_ENOMEM, "sd_seqset_create: device allocation of %llu bytes failed", (unsigned long long) s->total);
    }
    // on the context's stream (the set is used there), one wait for the three copies; a failed upload hands the half-built set
    // back (host copies freed, device buffers to the pool) instead of leaking it
    hipError_t e = hipMemcpyAsync(s->dRes, s->hRes.data(), s->total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = swCompBias ? hipMemcpyAsync(s->dBias, s->hBias.data(), s->total, hipMemcpyHostToDevice, ctx->stream)
                       : hipMemsetAsync(s->dBias, 0, s->total, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s->dOff, s->hOff.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = sdStreamSync(ctx);
    if (e != hipSuccess) {
        (void) sdStreamSyncRaw(ctx);   // nothing may still read the host copies
        sd_seqset_destroy(s);
        *out = nullptr;
        return sdFail(ctx, SD_EHIP, "sd_seqset_create: upload failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return SD_OK;
}

// Profile queries (Sequence::mapProfile output, Sequence.cpp:241-292; ssw_init's PROFILE branch, StripedSmithWaterman.cpp:1238-1301):
// the query letters stand in for the residues (identity counting, computerBacktrace :558) and the int8 alignment
// profile [position][21] (profile score / 4, X column 0) replaces "matrix row + composition bias" in every kernel.
int sd_profileset_create(sd_ctx *ctx, const uint8_t *queryLetters, const uint64_t *offsets, uint32_t n,
                         const int8_t *alnProfile, sd_seqset **out) {
    if (!alnProfile) return SD_EINVAL;
    int rc = sd_seqset_create(ctx, queryLetters, offsets, n, nullptr, out);
    if (rc != SD_OK) return rc;
    sd_seqset *s = *out;
    const size_t bytes = (size_t) s->total * 21;
    if (poolGet(ctx, bytes + 64, (void **) &s->dProf, &s->bProf) != hipSuccess) {
        (void) hipGetLastError();
        sd_seqset_destroy(s);
        *out = nullptr;
        return sdFail(ctx, SD_ENOMEM, "sd_profileset_create: device allocation of %llu bytes failed", (unsigned long long) bytes);
    }
    s->hProf.assign(alnProfile, alnProfile + bytes);
    {
        hipError_t e = hipMemcpyAsync(s->dProf, s->hProf.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = sdStreamSync(ctx);
        if (e != hipSuccess) {
            (void) sdStreamSyncRaw(ctx);
            sd_seqset_destroy(s);
            *out = nullptr;
            return sdFail(ctx, SD_EHIP, "sd_profileset_create: upload failed: %s", hipGetErrorString(e));
        }
    }
    s->hProfBias.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        int m = 0;   // min over the 20 amino-acid columns (matSize = L * PROFILE_AA_SIZE, :1277-1279)
        for (uint64_t x = offsets[i]; x < offsets[i + 1]; x++)
            for (int a = 0; a < 20; a++) m = std::min(m, (int) alnProfile[x * 21 + a]);
        s->hProfBias[i] = -m;
    }
    {
        int mx = 1;
        for (size_t x = 0; x < bytes; x++) mx = std::max(mx, (int) alnProfile[x]);
        s->maxEntryAdd = mx;
    }
    return SD_OK;
}

void sd_seqset_destroy(sd_seqset *s) {
    if (!s) return;
    // (a set is destroyed before its context, include/spacedust_gpu.h: its buffers go back to that context's pool)
    poolPut(s->ctx, s->dRes, s->bRes);
    poolPut(s->ctx, s->dProf, s->bProf);
    poolPut(s->ctx, s->dBias, s->bBias);
    poolPut(s->ctx, s->dOff, s->bOff);
    poolPut(s->ctx, s->dGroupOf, s->bGroupOf);
    poolPut(s->ctx, s->dGroupKey, s->bGroupKey);
    poolPut(s->ctx, s->dLet, s->bLet);
    delete s;
}

int sd_seqset_set_groups(sd_seqset *s, const uint32_t *groupOf, uint32_t nGroups, const uint32_t *keys) {
    if (!s || !groupOf || nGroups == 0) return SD_EINVAL;
    sd_ctx *ctx = s->ctx;
    (void) hipSetDevice(ctx->device);
    for (uint32_t i = 0; i < s->n; i++)
        if (groupOf[i] >= nGroups) return sdFail(ctx, SD_EINVAL, "sd_seqset_set_groups: sequence %u is in group %u of %u", i, groupOf[i], nGroups);
    // the selection key carries 28 bits of the DB key (or of the index): larger keys cannot break ties there, so such a set keeps
    // every accepted record for the caller's own selection (sd_sw_align_batch_best_by_group then returns what _compact_diag returns)
    bool keysFit = s->n <= 0x0FFFFFFFu;
    if (keys)
        for (uint32_t i = 0; i < s->n && keysFit; i++) keysFit = keys[i] < 0x0FFFFFFFu;
    if (!s->dGroupOf && poolGet(ctx, (size_t) (s->n + 1) * sizeof(uint32_t), (void **) &s->dGroupOf, &s->bGroupOf) != hipSuccess)
        return sdFail(ctx, SD_ENOMEM, "sd_seqset_set_groups: device allocation failed");
    if (keys && !s->dGroupKey && poolGet(ctx, (size_t) (s->n + 1) * sizeof(uint32_t), (void **) &s->dGroupKey, &s->bGroupKey) != hipSuccess)
        return sdFail(ctx, SD_ENOMEM, "sd_seqset_set_groups: device allocation failed");
    SD_HIP(ctx, hipMemcpyAsync(s->dGroupOf, groupOf, (size_t) s->n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (keys) SD_HIP(ctx, hipMemcpyAsync(s->dGroupKey, keys, (size_t) s->n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    s->nGroups = keysFit ? nGroups : 0;
    return SD_OK;
}

int sd_sw_last_cells(sd_ctx *ctx, uint64_t *f, uint64_t *r, uint64_t *t) {
    if (f) *f = ctx->cellsFwd;
    if (r) *r = ctx->cellsRev;
    if (t) *t = ctx->cellsTb;
    return SD_OK;
}

// forward task of a pair: the whole query against the whole target in `lanes` segments (32: byte structure, 16: word structure)
static SwTask fwdTask(const sd_seqset *queries, const sd_seqset *targets, uint32_t q, uint32_t t, uint32_t slot, int lanes) {
    SwTask tk;
    tk.qOff = queries->hOff[q]; tk.tOff = targets->hOff[t];
    tk.n = (int) (queries->hOff[q + 1] - tk.qOff); tk.tL = (int) (targets->hOff[t + 1] - tk.tOff); tk.qStep = 1; tk.tStep = 1;
    tk.segLen = std::max(1, (tk.n + lanes - 1) / lanes);
    tk.slot = slot; tk.boundOff = 0;
    return tk;
}

// scoreIdentical (StripedSmithWaterman.cpp:1675-1710), host side, O(L): the record of identity pair i but for its backtrace (btLen
// letters 'M', which the caller puts into its pool)
static int scoreIdentical(sd_ctx *ctx, const sd_sw_params *par, const sd::Evaluer &ev, const sd_seqset *queries, const sd_seqset *targets,
                          uint32_t i, uint32_t pq, uint32_t pt, sd_sw_result &r) {
    const int L = (int) (targets->hOff[pt + 1] - targets->hOff[pt]);
    const int qL = (int) (queries->hOff[pq + 1] - queries->hOff[pq]);
    if (qL != L) return sdFail(ctx, SD_EINVAL, "scoreIdentical has different lengths for pair %u", i);
    const uint8_t *q = queries->hRes.data() + queries->hOff[pq];
    const int8_t *cb = queries->hBias.data() + queries->hOff[pq];
    const uint8_t *t = targets->hRes.data() + targets->hOff[pt];
    short score = 0;
    if (queries->dProf) {   // profile_word_linear[target letter][position] (:1700-1703, :1293-1298)
        const int8_t *pr = queries->hProf.data() + queries->hOff[pq] * 21;
        for (int p = 0; p < L; p++) score += (short) pr[(size_t) p * 21 + t[p]];
    } else {
        for (int p = 0; p < L; p++) score += (short) (par->matrix[t[p] * 21 + q[p]] + cb[p]);
    }
    r.score = (int32_t) (uint32_t) (int) score;
    r.qStart = par->swMode == 0 ? -1 : 0;
    r.tStart = par->swMode == 0 ? -1 : 0;
    r.qEnd = L - 1; r.tEnd = L - 1; r.identical = L; r.btLen = L; r.flags = 0;
    r.evalue = sd::computeEvalue(ev, (double) (uint32_t) r.score, qL);
    r.btOffset = 0;
    return SD_OK;
}

int sd_sw_score_batch(sd_ctx *ctx, const sd_sw_params *par, const sd_seqset *queries, const sd_seqset *targets,
                      uint32_t nPairs, const uint32_t *pairQ, const uint32_t *pairT, int lanes, int reverse,
                      const int32_t *qEnd, const int32_t *tEnd, int32_t *out) {
    if (!ctx || !par || !queries || !targets || (lanes != 16 && lanes != 32)) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    DevBuf<int8_t> dMat;
    SD_HIP(ctx, dMat.alloc(441));
    SD_HIP(ctx, hipMemcpy(dMat.p, par->matrix, 441, hipMemcpyHostToDevice));
    std::vector<SwTask> tasks;
    tasks.reserve(nPairs);
    for (uint32_t i = 0; i < nPairs; i++) {
        SwTask tk = fwdTask(queries, targets, pairQ[i], pairT[i], i, lanes);
        if (reverse) {
            if (qEnd[i] < 0 || tEnd[i] < 0 || qEnd[i] >= tk.n || tEnd[i] >= tk.tL) return sdFail(ctx, SD_EINVAL, "bad end position for pair %u", i);
            tk.qOff += qEnd[i]; tk.tOff += tEnd[i]; tk.n = qEnd[i] + 1; tk.tL = tEnd[i] + 1; tk.qStep = -1; tk.tStep = -1;
            tk.segLen = std::max(1, (tk.n + lanes - 1) / lanes);
        }
        if (tk.n > 0 && tk.tL > 0) tasks.push_back(tk);
    }
    std::vector<int32_t> h;
    uint64_t cells = 0;
    int rc = runScoreTasks(ctx, tasks, queries, targets, dMat.p, par->gapOpen, par->gapExtend, h, nPairs, &cells);
    if (rc != SD_OK) return rc;
    if (reverse) ctx->cellsRev = cells; else ctx->cellsFwd = cells;
    for (uint32_t i = 0; i < nPairs; i++) {
        int v = h[3 * i], col = h[3 * i + 1], row = h[3 * i + 2];
        out[3 * i] = v;
        if (!reverse) {
            out[3 * i + 1] = col;
            out[3 * i + 2] = row;
        } else {
            out[3 * i + 1] = col < 0 ? -1 : tEnd[i] - col;   // scan position -> target index
            out[3 * i + 2] = row;                            // rows counted from qEnd downwards (reference: qStart = qEnd - read)
        }
    }
    return SD_OK;
}

// ---- alignBatchImpl: the arguments of a call, its workspace, and its stages in the order they run
struct AlignCall {
    const sd_sw_params *par;
    const sd_seqset *queries, *targets;
    uint32_t nPairs;
    const uint32_t *pairQ, *pairT;
    const uint8_t *isIdentity;
    sd_sw_result *out;
    char *btPool;
    uint64_t btCap, *btUsed;
    uint32_t *compactIdx, *nCompact;
    const uint16_t *pairDiag;   // the prefilter's diagonal of every pair (nullable)
    const float *bestBy;        // non-null: {seqIdThr, alnLenThr}: sd_sw_align_batch_best_by_group
};
// what downloadRecords brought back (pinned buffers of the context)
struct AlignRecords {
    uint32_t nRec, *hIdx;   // hIdx: compact mode, the pair of every record
    sd_sw_result *hRes;
    char *hPool;
    uint64_t poolBytes;
    bool cigarPool;
};

static int alignWsInit(sd_ctx *ctx, const AlignCall &a, AlignWs &w) {
    const sd_seqset *queries = a.queries;
    const size_t N = w.N = a.nPairs;
    w.grid = (unsigned) ((N + 255) / 256);
    SD_HIP(ctx, wsGet(ctx, "al.mat", 448, &w.dMat));
    SD_HIP(ctx, wsGet(ctx, "al.pq", N, &w.dPQ));
    SD_HIP(ctx, wsGet(ctx, "al.pt", N, &w.dPT));
    SD_HIP(ctx, wsGet(ctx, "al.ident", N, &w.dIdent));
    SD_HIP(ctx, wsGet(ctx, "al.word", N, &w.dWord));
    SD_HIP(ctx, wsGet(ctx, "al.keys", N, &w.dKeys));
    SD_HIP(ctx, wsGet(ctx, "al.vals", N, &w.dVals));
    SD_HIP(ctx, wsGet(ctx, "al.keyss", N, &w.dKeysS));
    SD_HIP(ctx, wsGet(ctx, "al.order", N, &w.dOrder));
    SD_HIP(ctx, wsGet(ctx, "al.fwdkeys", N, &w.dFwdKeys));
    SD_HIP(ctx, wsGet(ctx, "al.revkeys", N, &w.dRevKeys));
    SD_HIP(ctx, wsGet(ctx, "al.bounds", 64, &w.dBounds));
    SD_HIP(ctx, wsGet(ctx, "al.minbias", queries->n, &w.dMinBias));
    SD_HIP(ctx, wsGet(ctx, "al.out32", N * 3, &w.dOut32));
    SD_HIP(ctx, wsGet(ctx, "al.out16", N * 3, &w.dOut16));
    SD_HIP(ctx, wsGet(ctx, "al.outrev", N * 3, &w.dOutRev));
    SD_HIP(ctx, wsGet(ctx, "al.tbres", N * 2, &w.dTbRes));
    SD_HIP(ctx, wsGet(ctx, "al.err", 4, &w.dErr));
    SD_HIP(ctx, wsGet(ctx, "al.tasks", N, &w.dTasks));
    SD_HIP(ctx, wsGet(ctx, "al.tb", N, &w.dTb));
    SD_HIP(ctx, wsGet(ctx, "al.res", N, &w.dRes));
    ctx->alignDevRes = w.dRes;
    ctx->alignDevResN = N;
    SD_HIP(ctx, wsGet(ctx, "al.scana", N + 1, &w.dScanA));
    SD_HIP(ctx, wsGet(ctx, "al.scanb", N + 1, &w.dScanB));
    SD_HIP(ctx, wsGet(ctx, "al.dirbytes", N + 1, &w.dDirBytes));
    SD_HIP(ctx, wsGet(ctx, "al.diroff", N + 1, &w.dDirOff));
    SD_HIP(ctx, wsGet(ctx, "al.btbytes", N + 1, &w.dBtBytes));
    SD_HIP(ctx, wsGet(ctx, "al.btoff", N + 1, &w.dBtOff));
    SD_HIP(ctx, wsGet(ctx, "al.btlen", N + 1, &w.dBtLen));
    SD_HIP(ctx, wsGet(ctx, "al.dense", N + 1, &w.dDense));
    SD_HIP(ctx, wsGet(ctx, "al.cells", 4, &w.dCells));
    SD_HIP(ctx, hipMemcpyAsync(w.dMat, a.par->matrix, 441, hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemcpyAsync(w.dPQ, a.pairQ, N * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemcpyAsync(w.dPT, a.pairT, N * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (a.isIdentity) SD_HIP(ctx, hipMemcpyAsync(w.dIdent, a.isIdentity, N, hipMemcpyHostToDevice, ctx->stream));
    else SD_HIP(ctx, hipMemsetAsync(w.dIdent, 0, N, ctx->stream));
    // byte-kernel bias (ssw_init, :1276-1287): |min(matrix)| + |min(0, composition bias)| for sequences, |min(0, profile)| for profiles
    SD_HIP(ctx, hipMemcpyAsync(w.dMinBias, queries->dProf ? queries->hProfBias.data() : queries->hMinBias.data(),
                               queries->n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemsetAsync(w.dErr, 0, 4 * sizeof(int), ctx->stream));
    SD_HIP(ctx, hipMemsetAsync(w.dCells, 0, 4 * sizeof(unsigned long long), ctx->stream));
    SD_HIP(ctx, hipMemsetAsync(w.dOut32, 0, N * 3 * sizeof(int32_t), ctx->stream));
    SD_HIP(ctx, hipMemsetAsync(w.dOut16, 0, N * 3 * sizeof(int32_t), ctx->stream));
    SD_HIP(ctx, hipMemsetAsync(w.dOutRev, 0, N * 3 * sizeof(int32_t), ctx->stream));
    SD_HIP(ctx, hipMemsetAsync(w.dBtLen, 0, (N + 1) * sizeof(uint64_t), ctx->stream));
    return SD_OK;
}

// pass 4: banded traceback, band doubling on the device, in slices of what the direction scratch holds at a time
static int runTracebackRounds(sd_ctx *ctx, const AlignCall &a, const AlignWs &w) {
    const sd_seqset *queries = a.queries, *targets = a.targets;
    const uint32_t nPairs = a.nPairs;
    const size_t N = w.N;
    const int go = a.par->gapOpen, ge = a.par->gapExtend;
    // direction scratch of the LDS-band kernel (1 B per band cell, sized for the widest band of the task's class): a
    // quarter of the device memory at most (288 GB HBM: 72 GB), the rest belongs to the index and the prefilter workspace
    uint64_t SCRATCH_BUDGET = 16ull << 30;
    {
        size_t freeB = 0, totalB = 0;
        // a quarter of the device at most -- and no more than a third of what is free right now (the index, the prefilter
        // lanes and the other alignment lane hold the rest)
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && totalB > 0)
            SCRATCH_BUDGET = std::max<uint64_t>(1ull << 30, std::min<uint64_t>(totalB / 4, freeB / 3));
        if (const char *e = getenv("SD_TB_BUDGET")) SCRATCH_BUDGET = std::max<uint64_t>(1u << 20, strtoull(e, nullptr, 10));   // tests: force slices
    }
    uint32_t *dKeysRound = nullptr;
    SD_HIP(ctx, wsGet(ctx, "tb.keysRound", N + 1, &dKeysRound));
    bool budgetRaised = false;
    for (int round = 0; round < 4096; round++) {   // band doublings, and slices of what the direction scratch holds at a time
        SD_HIP(ctx, hipMemsetAsync(w.dDirBytes + N, 0, sizeof(uint64_t), ctx->stream));
        int rc = sdCtxExclusiveScan(ctx, "al.scantmp", w.dDirBytes, w.dDirOff, N + 1);
        if (rc != SD_OK) return rc;
        hipLaunchKernelGGL(k_tb_round, dim3(w.grid), dim3(256), 0, ctx->stream, nPairs, w.dKeys, w.dDirOff, w.dDirBytes, SCRATCH_BUDGET, dKeysRound);
        hipLaunchKernelGGL(k_tb_offsets, dim3(w.grid), dim3(256), 0, ctx->stream, nPairs, dKeysRound, w.dDirOff, w.dBtOff, w.dTb);
        rc = sdCtxSortPairs(ctx, "al.sort", dKeysRound, w.dKeysS, w.dVals, w.dOrder, nPairs, 16);
        if (rc != SD_OK) return rc;
        hipLaunchKernelGGL(k_bounds, dim3(1), dim3(64), 0, ctx->stream, w.dKeysS, nPairs, 4096u, w.dBounds, (int) N_TB_CLASSES + 1);
        uint32_t hb[N_TB_CLASSES + 1];
        uint64_t dirTotal = 0;
        SD_HIP(ctx, sdD2H(ctx, hb, w.dBounds, sizeof(hb)));
        SD_HIP(ctx, sdD2H(ctx, &dirTotal, w.dDirOff + N, sizeof(uint64_t)));
        SD_HIP(ctx, sdStreamSync(ctx));
        if (hb[N_TB_CLASSES] == 0) {
            if (dirTotal == 0) return SD_OK;   // nothing left
            // tasks are pending but not even the first fits the budget (a global-band task of a long protein, or a budget halved
            // after an allocation failure): the budget grows to what a single task needs -- or the call fails, never a silent exit
            if (SCRATCH_BUDGET >= dirTotal) return sdFail(ctx, SD_EHIP, "traceback: pending tasks but an empty round (budget %llu, pending %llu bytes)",
                                                          (unsigned long long) SCRATCH_BUDGET, (unsigned long long) dirTotal);
            SCRATCH_BUDGET = std::min<uint64_t>(dirTotal, SCRATCH_BUDGET * 2);
            budgetRaised = true;
            continue;
        }
        if (getenv("SD_DEBUG_TB")) {
            fprintf(stderr, "[tb] round %d: narrow", round);
            for (int ci = 0; ci < N_TB_NARROW; ci++) fprintf(stderr, " %u", hb[ci + 1] - hb[ci]);
            fprintf(stderr, " lds %u %u %u global %u dir %.1f MB\n", hb[N_TB_NARROW + 1] - hb[N_TB_NARROW], hb[N_TB_NARROW + 2] - hb[N_TB_NARROW + 1],
                    hb[N_TB_NARROW + 3] - hb[N_TB_NARROW + 2], hb[N_TB_NARROW + 4] - hb[N_TB_NARROW + 3], dirTotal / 1e6);
        }
        // more direction bytes than the budget (long result lists of homologs, e.g. --max-seqs 4000 on a 10 000-proteome target):
        // this round runs the prefix that fits (k_tb_round), the rest follows in later rounds
        int8_t *dDir = nullptr;
        if (wsGet(ctx, "tb.dir", std::min<uint64_t>(dirTotal, SCRATCH_BUDGET) + 64, &dDir) != hipSuccess) {
            (void) hipGetLastError();
            if (SCRATCH_BUDGET <= (256ull << 20) || budgetRaised)   // (a raised budget is what one task needs: halving it would only come back here)
                return sdFail(ctx, SD_ENOMEM, "traceback direction scratch: out of device memory (%llu bytes for one round)",
                              (unsigned long long) std::min<uint64_t>(dirTotal, SCRATCH_BUDGET));
            SCRATCH_BUDGET /= 2;   // another lane took the memory meanwhile: smaller slices
            continue;
        }
        for (uint32_t ci = 0; ci < N_TB_CLASSES; ci++) {
            const uint32_t begin = hb[ci], cnt = hb[ci + 1] - hb[ci];
            if (cnt == 0) continue;
            const TbClass &cls = TB_CLASSES[ci];
            ProfScope ps(ctx, cls.scope);
            if (ci < N_TB_NARROW) launchTbNarrow(ctx, queries, targets, w.dMat, go, ge, cls, w.dTb, cnt, w.dBt, w.dTbRes, w.dOrder + begin);
            else launchTbBand(ctx, queries, targets, w.dMat, go, ge, cls, std::max(0, cls.cap - 1), w.dTb, cnt, dDir, w.dBt, w.dTbRes, w.dOrder + begin);
        }
        SD_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_tb_collect, dim3(w.grid), dim3(256), 0, ctx->stream, nPairs, w.dKeys, w.dVals, w.dTb, w.dTbRes, w.dDirBytes, w.dBtLen,
                           w.dRes, w.dErr, 4 * 65536, dKeysRound);
    }
    return sdFail(ctx, SD_EHIP, "traceback: tasks still pending after 4096 rounds");
}

// SD_DEBUG_TB: band statistics of the finished tasks
static int printTracebackStats(sd_ctx *ctx, const AlignWs &w, uint32_t nPairs) {
    std::vector<TbTask> hT(nPairs);
    std::vector<uint64_t> hL(nPairs);
    SD_HIP(ctx, hipMemcpy(hT.data(), w.dTb, (size_t) nPairs * sizeof(TbTask), hipMemcpyDeviceToHost));
    SD_HIP(ctx, hipMemcpy(hL.data(), w.dBtLen, (size_t) nPairs * sizeof(uint64_t), hipMemcpyDeviceToHost));
    uint64_t nDone = 0, init6 = 0, init6final6 = 0, init6final14 = 0, final14 = 0;
    static const int lim[8] = {1, 2, 3, 4, 6, 8, 14, 1 << 30};
    uint64_t hi[8] = {0}, hf[8] = {0}, rowsF[8] = {0};
    for (uint32_t i = 0; i < nPairs; i++) {
        if (hL[i] == 0) continue;
        nDone++;
        const int ib = abs(hT[i].tLen - hT[i].qLen) + 1, fb = hT[i].band;
        if (ib <= 6) { init6++; if (fb <= 6) init6final6++; else if (fb <= 14) init6final14++; }
        if (fb <= 14) final14++;
        int x = 0, y = 0;
        while (ib > lim[x]) x++;
        while (fb > lim[y]) y++;
        hi[x]++;
        hf[y]++;
        rowsF[y] += (uint64_t) hT[i].qLen;
    }
    const uint64_t *const hist[3] = {hi, hf, rowsF};
    static const char *const head[3] = {"[tb] band <=1 <=2 <=3 <=4 <=6 <=8 <=14 >14: initial", " | final", " | rows by final"};
    for (int h = 0; h < 3; h++) {
        fprintf(stderr, "%s", head[h]);
        for (int x = 0; x < 8; x++) fprintf(stderr, " %llu", (unsigned long long) hist[h][x]);
    }
    fprintf(stderr, "\n");
    fprintf(stderr, "[tb] done %llu: final band<=14 %llu; initial<=6 %llu of which final<=6 %llu, final 7..14 %llu\n",
            (unsigned long long) nDone, (unsigned long long) final14, (unsigned long long) init6, (unsigned long long) init6final6,
            (unsigned long long) init6final14);
    return SD_OK;
}

// besthitbyset on the device: only identity pairs and the first accepted alignment of every (query, target set) cell keep
// their record and their backtrace (a table of queries x target sets)
static int markBestByGroup(sd_ctx *ctx, const AlignCall &a, const AlignWs &w) {
    const sd_seqset *queries = a.queries, *targets = a.targets;
    BestByGroup B;
    B.groupOf = targets->dGroupOf;
    B.groupKey = targets->dGroupKey;
    B.nGroups = targets->nGroups;
    B.seqIdThr = a.bestBy[0];
    B.alnLenThr = (int) a.bestBy[1];
    B.covThr = a.par->covThr;
    B.covMode = a.par->covMode;
    B.evalThr = a.par->evalThr;
    B.evalExact = (getenv("SD_BEST_EXACT") && atof(getenv("SD_BEST_EXACT")) == 0.0) ? 0.0 : BB_EVAL_EXACT;
    unsigned long long *dTable = nullptr;
    const size_t cellsN = (size_t) queries->n * targets->nGroups;
    SD_HIP(ctx, wsGet(ctx, "al.besttable", cellsN, &dTable));
    SD_HIP(ctx, hipMemsetAsync(dTable, 0, cellsN * sizeof(unsigned long long), ctx->stream));
    ProfScope ps(ctx, "align_best_by_group");
    hipLaunchKernelGGL(k_best_mark, dim3(w.grid), dim3(256), 0, ctx->stream, a.nPairs, (const sd_sw_result *) w.dRes, (const uint8_t *) w.dIdent,
                       (const uint32_t *) w.dPQ, (const uint32_t *) w.dPT, (const uint64_t *) queries->dOff, (const uint64_t *) targets->dOff, B, dTable);
    hipLaunchKernelGGL(k_best_keep, dim3(w.grid), dim3(256), 0, ctx->stream, a.nPairs, w.dRes, (const uint8_t *) w.dIdent, (const uint32_t *) w.dPQ,
                       (const uint32_t *) w.dPT, (const uint64_t *) queries->dOff, (const uint64_t *) targets->dOff, B,
                       (const unsigned long long *) dTable, w.dBtLen);
    return SD_OK;
}

// dense backtrace pool + records back to the host: all records, or (compact mode) only identity pairs and pairs that passed every gate
static int downloadRecords(sd_ctx *ctx, const AlignCall &a, const AlignWs &w, bool narrowFinal, AlignRecords &rec) {
    const uint32_t nPairs = a.nPairs;
    const size_t N = w.N;
    // (sd_sw_set_cigar_pool: the pool holds run-length text, its offsets are a scan of the text lengths)
    const bool cigarPool = rec.cigarPool = ctx->cigarPool && a.btPool != nullptr;
    uint64_t *dCigLen = nullptr;
    if (cigarPool) {
        SD_HIP(ctx, wsGet(ctx, "al.ciglen", N + 1, &dCigLen));
        SD_HIP(ctx, hipMemsetAsync(dCigLen + nPairs, 0, (N + 1 - nPairs) * sizeof(uint64_t), ctx->stream));
        hipLaunchKernelGGL(k_bt_cigar<false>, dim3((nPairs + 3) / 4), dim3(256), 0, ctx->stream, nPairs, (const uint64_t *) w.dBtLen,
                           (const uint64_t *) nullptr, (const TbTask *) w.dTb, (const char *) w.dBt, (char *) nullptr, dCigLen, (sd_sw_result *) nullptr);
    }
    const int rc = sdCtxExclusiveScan(ctx, "al.scantmp", cigarPool ? dCigLen : w.dBtLen, w.dDense, N + 1);
    if (rc != SD_OK) return rc;
    uint64_t &poolBytes = rec.poolBytes = 0;
    int hErr[4] = {0, 0, 0, 0};
    unsigned long long hCells[4] = {0, 0, 0, 0};
    SD_HIP(ctx, sdD2H(ctx, &poolBytes, w.dDense + N, sizeof(uint64_t)));
    SD_HIP(ctx, sdD2H(ctx, hErr, w.dErr, sizeof(hErr)));
    SD_HIP(ctx, sdD2H(ctx, hCells, w.dCells, sizeof(hCells)));
    SD_HIP(ctx, sdStreamSync(ctx));
    if (hErr[0] == 1) return sdFail(ctx, SD_EMISMATCH, "Score of forward/backward SW differ (fatal in the reference, StripedSmithWaterman.cpp:466-473)");
    if (hErr[0] == 2) return sdFail(ctx, SD_EHIP, "Trace back error");
    ctx->cellsFwd = hCells[0];
    ctx->cellsRev = hCells[1];
    if (narrowFinal && ctx->profiling) {   // counters beside the kernel times (sums in `ms`): what the switch did to this call's word pairs
        const double add[3] = {(double) hCells[2], (double) hCells[3], (double) (hCells[2] - hCells[3])};
        static const char *const names[3] = {"stat.sw_word_pairs", "stat.sw_word_wide", "stat.sw_word_narrow_final"};
        for (int x = 0; x < 3; x++) {
            sd_profile_entry &pe = ctx->profile[names[x]];
            pe.ms += add[x];
            pe.launches += 1;
        }
    }
    // identity pairs need pool space too (scoreIdentical backtraces are written by the host: finishRecordsOnHost)
    uint64_t identBytes = 0;
    if (a.isIdentity && a.btPool)
        for (uint32_t i = 0; i < nPairs; i++)
            if (a.isIdentity[i]) identBytes += cigarPool ? 8 : a.targets->hOff[a.pairT[i] + 1] - a.targets->hOff[a.pairT[i]];
    if (poolBytes > 0 && a.btPool == nullptr) return sdFail(ctx, SD_EINVAL, "swMode 2 needs a backtrace pool");
    if (poolBytes + identBytes > a.btCap && a.btPool) return sdFail(ctx, SD_ENOMEM, "backtrace pool too small");
    char *dPool = nullptr;
    SD_HIP(ctx, wsGet(ctx, "al.pool", poolBytes + 64, &dPool));
    if (poolBytes > 0 && cigarPool)
        hipLaunchKernelGGL(k_bt_cigar<true>, dim3((nPairs + 3) / 4), dim3(256), 0, ctx->stream, nPairs, (const uint64_t *) w.dBtLen,
                           (const uint64_t *) w.dDense, (const TbTask *) w.dTb, (const char *) w.dBt, dPool, (uint64_t *) nullptr, w.dRes);
    else if (poolBytes > 0)
        hipLaunchKernelGGL(k_bt_pack, dim3((nPairs + 3) / 4), dim3(256), 0, ctx->stream, nPairs, w.dBtLen, w.dDense, w.dTb, w.dBt, dPool,
                           (uint64_t) 0, w.dRes);
    uint32_t &nRec = rec.nRec = nPairs;
    sd_sw_result *dRecSrc = w.dRes;
    rec.hIdx = nullptr;
    if (a.compactIdx) {
        uint8_t *dAcc = nullptr;
        uint64_t *dAccPos = nullptr;
        sd_sw_result *dResC = nullptr;
        uint32_t *dIdxC = nullptr;
        SD_HIP(ctx, wsGet(ctx, "al.acc", N + 1, &dAcc));
        SD_HIP(ctx, wsGet(ctx, "al.accpos", N + 1, &dAccPos));
        SD_HIP(ctx, wsGet(ctx, "al.resc", N, &dResC));
        SD_HIP(ctx, wsGet(ctx, "al.idxc", N, &dIdxC));
        hipLaunchKernelGGL(k_accept, dim3(w.grid), dim3(256), 0, ctx->stream, nPairs, w.dRes, w.dIdent, dAcc);
        SD_HIP(ctx, hipMemsetAsync(dAcc + N, 0, 1, ctx->stream));
        const int rcS = sdCtxExclusiveScan(ctx, "al.scantmp", (const uint8_t *) dAcc, dAccPos, N + 1);
        if (rcS != SD_OK) return rcS;
        hipLaunchKernelGGL(k_accept_compact, dim3(w.grid), dim3(256), 0, ctx->stream, nPairs, w.dRes, dAcc, dAccPos, dResC, dIdxC);
        uint64_t nAcc = 0;
        SD_HIP(ctx, sdD2H(ctx, &nAcc, dAccPos + N, sizeof(uint64_t)));
        SD_HIP(ctx, sdStreamSync(ctx));
        nRec = (uint32_t) nAcc;
        dRecSrc = dResC;
        SD_HIP(ctx, pinGet(ctx, "al.hidx", std::max<uint32_t>(nRec, 1), &rec.hIdx));
        SD_HIP(ctx, hipMemcpyAsync(rec.hIdx, dIdxC, (size_t) nRec * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    SD_HIP(ctx, pinGet(ctx, "al.hres", std::max<uint32_t>(nRec, 1), &rec.hRes));
    SD_HIP(ctx, pinGet(ctx, "al.hpool", poolBytes + 64, &rec.hPool));
    SD_HIP(ctx, hipMemcpyAsync(rec.hRes, dRecSrc, (size_t) nRec * sizeof(sd_sw_result), hipMemcpyDeviceToHost, ctx->stream));
    if (poolBytes > 0) SD_HIP(ctx, hipMemcpyAsync(rec.hPool, dPool, poolBytes, hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    return SD_OK;
}

// the pool into the caller's, exact E-values (the device value only served the gate), the rare results the device let through
// because they sat within 1e-9 of the E-value threshold, and identity pairs
static int finishRecordsOnHost(sd_ctx *ctx, const AlignCall &a, const sd::Evaluer &ev, const AlignRecords &rec) {
    const sd_sw_params *par = a.par;
    const sd_seqset *queries = a.queries;
    const uint8_t *isIdentity = a.isIdentity;
    const uint32_t *pairQ = a.pairQ, *hIdx = rec.hIdx;
    const uint32_t nRec = rec.nRec;
    char *btPool = a.btPool;
    const uint64_t poolBytes = rec.poolBytes;
    {
        const int nth = std::max(1, std::min(omp_get_max_threads(), 64));
        const size_t blk = (poolBytes + nth - 1) / nth;
#pragma omp parallel for schedule(static) num_threads(nth)
        for (int t = 0; t < nth; t++) {
            const size_t lo = std::min<size_t>(poolBytes, (size_t) t * blk), hi = std::min<size_t>(poolBytes, lo + blk);
            if (hi > lo) memcpy(btPool + lo, rec.hPool + lo, hi - lo);
        }
    }
    uint64_t btPos = poolBytes;
#pragma omp parallel for schedule(static)
    for (uint32_t x = 0; x < nRec; x++) {
        const uint32_t i = hIdx ? hIdx[x] : x;
        sd_sw_result r = rec.hRes[x];
        if (!(isIdentity && isIdentity[i])) {
            const int qL = (int) (queries->hOff[pairQ[i] + 1] - queries->hOff[pairQ[i]]);
            if (r.tEnd != -1 && qL > 0) {
                // the device's value (same formula, device libm: relative error ~1e-15) stands for pairs far above the
                // threshold -- the reference computes but never reports those; everything that can be reported gets
                // the host's bit-exact value
                if (!(r.evalue > 2.0 * par->evalThr)) r.evalue = sd::computeEvalue(ev, r.score, qL);
                if (r.evalue > par->evalThr && r.qStart != -1) {   // decided by the host's exact value
                    r.qStart = -1; r.tStart = -1; r.identical = 0; r.btLen = 0; r.btOffset = 0; r.flags &= 1;
                }
            } else {
                r.evalue = 0.0;
            }
        }
        a.out[x] = r;
        if (a.compactIdx) a.compactIdx[x] = i;
    }
    if (a.nCompact) *a.nCompact = nRec;
    if (isIdentity) {
        for (uint32_t x = 0; x < nRec; x++) {
            const uint32_t i = hIdx ? hIdx[x] : x;
            if (!isIdentity[i]) continue;
            sd_sw_result &r = a.out[x];
            const int rc = scoreIdentical(ctx, par, ev, queries, a.targets, i, pairQ[i], a.pairT[i], r);
            if (rc != SD_OK) return rc;
            const int L = r.btLen;
            if (btPool && rec.cigarPool) {   // "<L>M"
                char txt[16];
                const int nTxt = snprintf(txt, sizeof(txt), "%dM", L);
                memcpy(btPool + btPos, txt, (size_t) nTxt);
                r.btOffset = btPos;
                r.flags = nTxt << 8;
                btPos += (uint64_t) nTxt;
            } else if (btPool) {
                memset(btPool + btPos, 'M', L);
                r.btOffset = btPos;
                btPos += L;
            }
        }
    }
    if (a.btUsed) *a.btUsed = btPos;
    ctx->d2hRecordBytes += (uint64_t) nRec * (sizeof(sd_sw_result) + (a.compactIdx ? sizeof(uint32_t) : 0));
    ctx->d2hPoolBytes += poolBytes;
    return SD_OK;
}

// compactIdx != nullptr: only the pairs that reached a result worth reporting (identity pairs and pairs that were
// not stopped at a gate) are returned, out[x] being the record of pair compactIdx[x], x < *nCompact
// Of the target set this path reads the device side only (n, dRes, dOff, dProf), except for identity pairs, whose targets' host copies
// (hOff, hRes) it reads as well: sd_sw_align_alt_batch relies on that when it passes a device-only view of its scratch set
// without identity pairs (sdDeviceSeqView, sd_sw_alt.hip).  ctx->alignDevRes is left pointing at the per-pair records.
static int alignBatchImpl(sd_ctx *ctx, const AlignCall &a) {
    const sd_sw_params *par = a.par;
    const sd_seqset *queries = a.queries, *targets = a.targets;
    const uint32_t nPairs = a.nPairs;
    if (!ctx || !par || !queries || !targets || !a.out) return SD_EINVAL;
    if (a.compactIdx && (!a.nCompact || par->swMode != 2)) return sdFail(ctx, SD_EINVAL, "the compact variants need swMode 2 (records with backtraces)");
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);   // (reads an earlier, failed call left pending)
    if (a.btUsed) *a.btUsed = 0;
    if (a.nCompact) *a.nCompact = 0;
    if (nPairs == 0) return SD_OK;
    const int go = par->gapOpen, ge = par->gapExtend;
    ctx->cellsFwd = ctx->cellsRev = ctx->cellsTb = 0;
    sd::Evaluer ev;
    sd::initEvaluer(ev, par->dbResidues);
    int matMin = 0;
    for (int i = 0; i < 441; i++) matMin = std::min(matMin, (int) par->matrix[i]);
    for (uint32_t i = 0; i < nPairs; i++)
        if (a.pairQ[i] >= queries->n || a.pairT[i] >= targets->n) return sdFail(ctx, SD_EINVAL, "pair %u out of range", i);
    if (targets->dProf) return sdFail(ctx, SD_EUNSUPPORTED, "profile targets are not implemented (profile queries are)");
    std::unique_ptr<HostScope> hs(new HostScope(ctx, "align.upload"));
    DevGateParams gp;
    gp.go = go; gp.ge = ge; gp.matMin = matMin; gp.swMode = par->swMode; gp.covMode = par->covMode; gp.covThr = par->covThr;
    {   // the int16 kernels are exact while no cell can exceed 32 767: rows x the largest entry of a query profile of this call
        int matMax = 0;
        for (int x = 0; x < 441; x++) matMax = std::max(matMax, (int) par->matrix[x]);
        const int maxEntry = std::max(1, queries->dProf ? queries->maxEntryAdd : matMax + queries->maxEntryAdd);
        gp.wideRowLimit = 32767 / maxEntry;
    }
    gp.evalThr = par->evalThr;
    gp.lambda = ev.lambda; gp.K = ev.K; gp.aI = ev.aI; gp.bI = ev.bI; gp.alphaI = ev.alphaI; gp.betaI = ev.betaI;
    gp.aJ = ev.aJ; gp.bJ = ev.bJ; gp.alphaJ = ev.alphaJ; gp.betaJ = ev.betaJ; gp.sigma = ev.sigma; gp.tau = ev.tau;
    gp.viThr = ev.viThr; gp.vjThr = ev.vjThr; gp.cThr = ev.cThr; gp.dbResidues = ev.dbResidues;
    AlignWs w = {};
    int rc = alignWsInit(ctx, a, w);
    if (rc != SD_OK) return rc;
    const size_t N = w.N;
    const unsigned grid = w.grid;

    // ---- pass 1: forward, byte-kernel lane structure
    hs.reset(new HostScope(ctx, "align.fwd32"));
    // the packed-int16 kernels need go >= ge twice over (see sd_sw_pk.h): for their F update, and for leaving out the lane-structure
    // chain Fl, which changes no G only then.  This is the one place that admits them -- the class keys of all three passes are made
    // with usePk, and runScoreTasks (sd_sw_score_batch, the host path) launches the int32 kernel only.  SD_SW_INT32=1 forces the int32 kernel
    const int usePk = (go >= ge && go < 1024 && ge >= 0 && getenv("SD_SW_INT32") == nullptr) ? 1 : 0;
    hipLaunchKernelGGL(k_make_fwd, dim3(grid), dim3(256), 0, ctx->stream, nPairs, w.dPQ, w.dPT, w.dIdent, queries->dOff, targets->dOff,
                       w.dTasks, w.dFwdKeys, w.dVals, w.dRes, usePk);
    // pairs whose byte score saturates for certain (k_pre_word) skip this pass
    uint32_t *dPass1Keys = w.dFwdKeys;
    uint8_t *dPreWord = nullptr, *dWide = nullptr;
    const bool narrowFinal = ctx->narrowFinal && usePk;   // sd_sw_set_narrow_final
    if (narrowFinal) SD_HIP(ctx, wsGet(ctx, "al.wide", N, &dWide));
    if (a.pairDiag && usePk) {
        uint16_t *dDiag = nullptr;
        SD_HIP(ctx, wsGet(ctx, "al.diag", N, &dDiag));
        SD_HIP(ctx, wsGet(ctx, "al.preword", N, &dPreWord));
        SD_HIP(ctx, wsGet(ctx, "al.pass1keys", N, &dPass1Keys));
        SD_HIP(ctx, hipMemcpyAsync(dDiag, a.pairDiag, N * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_pre_word, dim3(grid), dim3(256), 0, ctx->stream, nPairs, (const uint32_t *) w.dPQ, (const uint32_t *) w.dPT,
                           (const uint16_t *) dDiag, (const uint32_t *) w.dFwdKeys, (const uint64_t *) queries->dOff, (const uint64_t *) targets->dOff,
                           (const uint8_t *) queries->dRes, (const int8_t *) queries->dBias, (const uint8_t *) targets->dRes, (const int8_t *) w.dMat,
                           (const int8_t *) queries->dProf, (const int32_t *) w.dMinBias, queries->dProf ? 0 : matMin, dPreWord, dPass1Keys,
                           narrowFinal ? 1 : 0);
    }
    hipLaunchKernelGGL(k_cells, dim3(grid), dim3(256), 0, ctx->stream, nPairs, w.dTasks, dPass1Keys, w.dCells + 0);
    const uint32_t *dShare = queries->n >= (1u << PAIR_QUERY_BITS) ? nullptr : w.dPQ;   // forward passes scan whole queries: pair by query
    rc = devRunScore(ctx, w, nPairs, dPass1Keys, queries, targets, go, ge, w.dOut32, dShare);
    if (rc != SD_OK) return rc;
    // ---- pass 2: saturated pairs again with the word kernel's 16-lane structure
    hs.reset(new HostScope(ctx, "align.fwd16"));
    hipLaunchKernelGGL(k_gate_word, dim3(grid), dim3(256), 0, ctx->stream, nPairs, w.dPQ, w.dOut32, w.dMinBias, queries->dProf ? 0 : matMin, w.dTasks, w.dKeys,
                       w.dVals, w.dWord, w.dFwdKeys, usePk, gp.wideRowLimit, (const uint8_t *) dPreWord, dWide, w.dCells + 2);
    hipLaunchKernelGGL(k_cells, dim3(grid), dim3(256), 0, ctx->stream, nPairs, w.dTasks, w.dKeys, w.dCells + 0);
    rc = devRunScore(ctx, w, nPairs, w.dKeys, queries, targets, go, ge, w.dOut16, dShare);
    if (rc != SD_OK) return rc;
    // ---- gates + pass 3: start positions
    hs.reset(new HostScope(ctx, "align.rev"));
    // Start-position tasks scan per-pair prefixes of the reversed query.  sd_sw_set_shared_start: the narrow ones of a query of
    // 129 .. 768 rows run as suffixes of the profile of the whole reversed query, four tasks of one query per wavefront, paired by
    // the same sort that orders the others (k_pair_keys): still one sort and one boundary read-back in this pass.  Every other
    // task builds its own profile, as all of them do with the switch off
    const bool sharedStart = ctx->sharedStart && usePk && dShare != nullptr;
    hipLaunchKernelGGL(k_gate_rev, dim3(grid), dim3(256), 0, ctx->stream, nPairs, gp, w.dPQ, w.dPT, queries->dOff, targets->dOff, w.dOut32,
                       w.dOut16, w.dWord, w.dFwdKeys, w.dTasks, w.dRevKeys, w.dVals, w.dRes, usePk, (const uint8_t *) dWide, sharedStart ? 1 : 0);
    hipLaunchKernelGGL(k_cells, dim3(grid), dim3(256), 0, ctx->stream, nPairs, w.dTasks, w.dRevKeys, w.dCells + 1);
    rc = devRunScore(ctx, w, nPairs, w.dRevKeys, queries, targets, go, ge, w.dOutRev, sharedStart ? dShare : nullptr, 1);
    if (rc != SD_OK) return rc;
    // ---- pass 4: banded traceback, band doubling on the device
    hs.reset(new HostScope(ctx, "align.traceback"));
    hipLaunchKernelGGL(k_gate_tb, dim3(grid), dim3(256), 0, ctx->stream, nPairs, gp, w.dPQ, w.dPT, queries->dOff, targets->dOff, w.dOutRev,
                       w.dRevKeys, w.dTb, w.dKeys, w.dVals, w.dDirBytes, w.dBtBytes, w.dRes, w.dErr);
    SD_HIP(ctx, hipMemsetAsync(w.dBtBytes + N, 0, sizeof(uint64_t), ctx->stream));
    rc = sdCtxExclusiveScan(ctx, "al.scantmp", w.dBtBytes, w.dBtOff, N + 1);
    if (rc != SD_OK) return rc;
    uint64_t btScratch = 0;
    SD_HIP(ctx, sdD2H(ctx, &btScratch, w.dBtOff + N, sizeof(uint64_t)));
    SD_HIP(ctx, sdStreamSync(ctx));
    SD_HIP(ctx, wsGet(ctx, "tb.bt", btScratch + 64, &w.dBt));
    rc = runTracebackRounds(ctx, a, w);
    if (rc != SD_OK) return rc;
    if (getenv("SD_DEBUG_TB")) {
        rc = printTracebackStats(ctx, w, nPairs);
        if (rc != SD_OK) return rc;
    }
    // (beyond 2^27 cells of queries x target sets the call returns everything)
    if (a.bestBy && a.compactIdx && targets->dGroupOf && targets->nGroups > 0 && (uint64_t) queries->n * targets->nGroups <= (1ull << 27)) {
        rc = markBestByGroup(ctx, a, w);
        if (rc != SD_OK) return rc;
    }
    hs.reset(new HostScope(ctx, "align.download"));
    AlignRecords rec;
    rc = downloadRecords(ctx, a, w, narrowFinal, rec);
    if (rc != SD_OK) return rc;
    hs.reset(new HostScope(ctx, "align.finish"));
    return finishRecordsOnHost(ctx, a, ev, rec);
}

int sd_sw_set_cigar_pool(sd_ctx *ctx, int on) {
    if (!ctx) return SD_EINVAL;
    ctx->cigarPool = on != 0;
    return SD_OK;
}

int sd_sw_set_narrow_final(sd_ctx *ctx, int on) {
    if (!ctx) return SD_EINVAL;
    ctx->narrowFinal = on != 0;
    return SD_OK;
}

int sd_sw_set_shared_start(sd_ctx *ctx, int on) {
    if (!ctx) return SD_EINVAL;
    ctx->sharedStart = on != 0;
    return SD_OK;
}

int sd_sw_set_group16(sd_ctx *ctx, int on) {
    if (!ctx) return SD_EINVAL;
    ctx->group16 = on != 0;
    return SD_OK;
}

int sd_sw_download_bytes(sd_ctx *ctx, uint64_t *recordBytes, uint64_t *poolBytes) {
    if (!ctx) return SD_EINVAL;
    if (recordBytes) *recordBytes = ctx->d2hRecordBytes;
    if (poolBytes) *poolBytes = ctx->d2hPoolBytes;
    return SD_OK;
}

int sd_sw_align_batch(sd_ctx *ctx, const sd_sw_params *par, const sd_seqset *queries, const sd_seqset *targets,
                      uint32_t nPairs, const uint32_t *pairQ, const uint32_t *pairT, const uint8_t *isIdentity,
                      sd_sw_result *out, char *btPool, uint64_t btCap, uint64_t *btUsed) {
    return alignBatchImpl(ctx, {par, queries, targets, nPairs, pairQ, pairT, isIdentity, out, btPool, btCap, btUsed, nullptr, nullptr, nullptr, nullptr});
}

int sd_sw_align_batch_compact(sd_ctx *ctx, const sd_sw_params *par, const sd_seqset *queries, const sd_seqset *targets,
                              uint32_t nPairs, const uint32_t *pairQ, const uint32_t *pairT, const uint8_t *isIdentity,
                              uint32_t *outIdx, sd_sw_result *out, uint32_t *nOut, char *btPool, uint64_t btCap,
                              uint64_t *btUsed) {
    if (!outIdx || !nOut) return SD_EINVAL;
    return alignBatchImpl(ctx, {par, queries, targets, nPairs, pairQ, pairT, isIdentity, out, btPool, btCap, btUsed, outIdx, nOut, nullptr, nullptr});
}

int sd_sw_align_batch_compact_diag(sd_ctx *ctx, const sd_sw_params *par, const sd_seqset *queries, const sd_seqset *targets,
                                   uint32_t nPairs, const uint32_t *pairQ, const uint32_t *pairT, const uint16_t *pairDiag,
                                   const uint8_t *isIdentity, uint32_t *outIdx, sd_sw_result *out, uint32_t *nOut, char *btPool,
                                   uint64_t btCap, uint64_t *btUsed) {
    if (!outIdx || !nOut) return SD_EINVAL;
    return alignBatchImpl(ctx, {par, queries, targets, nPairs, pairQ, pairT, isIdentity, out, btPool, btCap, btUsed, outIdx, nOut, pairDiag, nullptr});
}

int sd_selftest_sort_pairs(sd_ctx *ctx, const uint32_t *keys, const uint32_t *vals, uint32_t n, int beginBit, int endBit, uint32_t *outKeys,
                           uint32_t *outVals) {
    if (!ctx || (n && (!keys || !vals || !outKeys || !outVals)) || beginBit < 0 || endBit > 32 || beginBit >= endBit) return SD_EINVAL;
    if (n == 0) return SD_OK;
    (void) hipSetDevice(ctx->device);
    DevBuf<uint32_t> kIn, vIn, kOut, vOut, kTmp, vTmp, cnt;
    SD_HIP(ctx, kIn.alloc(n));
    SD_HIP(ctx, vIn.alloc(n));
    SD_HIP(ctx, kOut.alloc(n));
    SD_HIP(ctx, vOut.alloc(n));
    SD_HIP(ctx, kTmp.alloc(n));
    SD_HIP(ctx, vTmp.alloc(n));
    SD_HIP(ctx, cnt.alloc(sdRadixSortCountsBytes() / sizeof(uint32_t)));
    SD_HIP(ctx, hipMemcpy(kIn.p, keys, (size_t) n * 4, hipMemcpyHostToDevice));
    SD_HIP(ctx, hipMemcpy(vIn.p, vals, (size_t) n * 4, hipMemcpyHostToDevice));
    SD_HIP(ctx, sdRadixSortPairs(ctx->stream, kIn.p, vIn.p, kOut.p, vOut.p, kTmp.p, vTmp.p, n, beginBit, endBit, cnt.p));
    SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SD_HIP(ctx, hipMemcpy(outKeys, kOut.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    SD_HIP(ctx, hipMemcpy(outVals, vOut.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_selftest_scan(sd_ctx *ctx, const uint32_t *in, uint32_t n, uint64_t *exclusiveSum, uint32_t *runningMax) {
    if (!ctx || !in || !exclusiveSum || n == 0) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    DevBuf<uint32_t> dIn, dMax;
    DevBuf<uint64_t> dOut;
    SD_HIP(ctx, dIn.alloc((size_t) n + 1));
    SD_HIP(ctx, dOut.alloc((size_t) n + 1));
    SD_HIP(ctx, hipMemset(dIn.p, 0, ((size_t) n + 1) * 4));
    SD_HIP(ctx, hipMemcpy(dIn.p, in, (size_t) n * 4, hipMemcpyHostToDevice));
    int rc = sdCtxExclusiveScan(ctx, "al.scantmp", (const uint32_t *) dIn.p, dOut.p, (size_t) n + 1);
    if (rc != SD_OK) return rc;
    if (runningMax) {
        SD_HIP(ctx, dMax.alloc(n));
        rc = sdCtxInclusiveMax(ctx, "al.scantmp32", dIn.p, dMax.p, n);
        if (rc != SD_OK) return rc;
    }
    SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SD_HIP(ctx, hipMemcpy(exclusiveSum, dOut.p, ((size_t) n + 1) * 8, hipMemcpyDeviceToHost));
    if (runningMax) SD_HIP(ctx, hipMemcpy(runningMax, dMax.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_selftest_score_class(int kernel, int32_t n, int32_t tL, int shared, int32_t wideRowLimit, uint32_t *klass, char *scope, size_t cap) {
    if (kernel < SCORE_PK || kernel > SCORE_PK_START || n < 1 || tL < 1 || !klass || (cap && !scope)) return SD_EINVAL;
    const uint32_t ci = scoreClassOf(n, tL, kernel, wideRowLimit);
    const ScoreSide &side = shared && (ci < FIRST_INT32_CLASS || ci >= FIRST_START_CLASS) ? SCORE_CLASSES[ci].shared : SCORE_CLASSES[ci].unshared;   // (devRunScore)
    *klass = ci;
    if (cap) snprintf(scope, cap, "%s", side.scope);
    return SD_OK;
}

int sd_sw_align_batch_best_by_group(sd_ctx *ctx, const sd_sw_params *par, const sd_seqset *queries, const sd_seqset *targets,
                                    uint32_t nPairs, const uint32_t *pairQ, const uint32_t *pairT, const uint16_t *pairDiag,
                                    const uint8_t *isIdentity, float seqIdThr, int32_t alnLenThr, uint32_t *outIdx, sd_sw_result *out,
                                    uint32_t *nOut, char *btPool, uint64_t btCap, uint64_t *btUsed) {
    if (!outIdx || !nOut || !targets) return SD_EINVAL;
    if (!targets->dGroupOf) return sdFail(ctx, SD_EINVAL, "sd_sw_align_batch_best_by_group: the target set has no groups (sd_seqset_set_groups)");
    const float bb[2] = {seqIdThr, (float) alnLenThr};
    return alignBatchImpl(ctx, {par, queries, targets, nPairs, pairQ, pairT, isIdentity, out, btPool, btCap, btUsed, outIdx, nOut, pairDiag, bb});
}

int sd_sw_align_batch_hostpath(sd_ctx *ctx, const sd_sw_params *par, const sd_seqset *queries, const sd_seqset *targets,
                      uint32_t nPairs, const uint32_t *pairQ, const uint32_t *pairT, const uint8_t *isIdentity,
                      sd_sw_result *out, char *btPool, uint64_t btCap, uint64_t *btUsed) {
    if (!ctx || !par || !queries || !targets || !out) return SD_EINVAL;
    if (queries->dProf || targets->dProf) return sdFail(ctx, SD_EUNSUPPORTED, "the host-orchestrated A/B path takes sequence sets only");
    (void) hipSetDevice(ctx->device);
    const int go = par->gapOpen, ge = par->gapExtend;
    ctx->cellsFwd = ctx->cellsRev = ctx->cellsTb = 0;
    sd::Evaluer ev;
    sd::initEvaluer(ev, par->dbResidues);
    int matMin = 0;
    for (int i = 0; i < 441; i++) matMin = std::min(matMin, (int) par->matrix[i]);
    DevBuf<int8_t> dMat;
    SD_HIP(ctx, dMat.alloc(441));
    SD_HIP(ctx, hipMemcpy(dMat.p, par->matrix, 441, hipMemcpyHostToDevice));
    if (btUsed) *btUsed = 0;
    uint64_t btPos = 0;

    std::unique_ptr<HostScope> hs(new HostScope(ctx, "align.init"));
    std::vector<int> qLv(nPairs), tLv(nPairs);
    for (uint32_t i = 0; i < nPairs; i++) {
        if (pairQ[i] >= queries->n || pairT[i] >= targets->n) return sdFail(ctx, SD_EINVAL, "pair %u out of range", i);
        qLv[i] = (int) (queries->hOff[pairQ[i] + 1] - queries->hOff[pairQ[i]]);
        tLv[i] = (int) (targets->hOff[pairT[i] + 1] - targets->hOff[pairT[i]]);
        sd_sw_result &r = out[i];
        r.score = 0; r.qStart = -1; r.qEnd = -1; r.tStart = -1; r.tEnd = -1; r.identical = 0; r.btLen = 0; r.flags = 0;
        r.evalue = 0.0; r.btOffset = 0;
    }
    // ---- identity pairs
    for (uint32_t i = 0; i < nPairs; i++) {
        if (!(isIdentity && isIdentity[i])) continue;
        sd_sw_result &r = out[i];
        const int rcI = scoreIdentical(ctx, par, ev, queries, targets, i, pairQ[i], pairT[i], r);
        if (rcI != SD_OK) return rcI;
        if (btPool) {
            if (btPos + (uint64_t) r.btLen > btCap) return sdFail(ctx, SD_ENOMEM, "backtrace pool too small");
            memset(btPool + btPos, 'M', r.btLen);
            r.btOffset = btPos;
            btPos += r.btLen;
        }
    }
    hs.reset(new HostScope(ctx, "align.fwd32"));
    // ---- pass 1: forward, byte-kernel lane structure (32 lanes)
    std::vector<SwTask> tasks;
    {
        // every pair gets a slot-ordered task; identity / empty pairs are dropped with a parallel compaction
        std::vector<uint32_t> keepIdx(nPairs);
        uint32_t nKeep = 0;
        for (uint32_t i = 0; i < nPairs; i++)
            if (!(isIdentity && isIdentity[i]) && qLv[i] > 0 && tLv[i] > 0) keepIdx[nKeep++] = i;
        tasks.resize(nKeep);
#pragma omp parallel for schedule(static)
        for (uint32_t x = 0; x < nKeep; x++) tasks[x] = fwdTask(queries, targets, pairQ[keepIdx[x]], pairT[keepIdx[x]], keepIdx[x], 32);
    }
    std::vector<int32_t> h;
    int rc = runScoreTasks(ctx, tasks, queries, targets, dMat.p, go, ge, h, nPairs, &ctx->cellsFwd, "f32");
    if (rc != SD_OK) return rc;
    hs.reset(new HostScope(ctx, "align.fwd16"));
    // ---- pass 2: pairs whose byte score saturates (max + bias >= 255, :881,916,360-368) rerun with the
    //      word kernel's 16-lane structure
    std::vector<SwTask> tasks2;
    std::vector<uint8_t> word(nPairs, 0);
    for (size_t x = 0; x < tasks.size(); x++) {
        const uint32_t i = tasks[x].slot;
        const int bias = std::abs(matMin) + std::abs(queries->hMinBias[pairQ[i]]);
        if (h[3 * i] + bias >= 255) {
            word[i] = 1;
            tasks2.push_back(fwdTask(queries, targets, pairQ[i], pairT[i], i, 16));
        }
    }
    std::vector<int32_t> h2;
    rc = runScoreTasks(ctx, tasks2, queries, targets, dMat.p, go, ge, h2, nPairs, &ctx->cellsFwd, "f16");
    if (rc != SD_OK) return rc;
    hs.reset(new HostScope(ctx, "align.gates"));
    // ---- gates after the score pass (:389-398); E-values in parallel, task list built serially
    std::vector<SwTask> rtasks;
    std::vector<uint8_t> goRev(nPairs, 0), hasTask(nPairs, 0);
    for (size_t x = 0; x < tasks.size(); x++) hasTask[tasks[x].slot] = 1;
    // pair-major (contiguous) so that threads do not share cache lines of out[] / goRev[]
#pragma omp parallel for schedule(static)
    for (uint32_t i = 0; i < nPairs; i++) {
        if (!hasTask[i]) continue;
        const int32_t *src = word[i] ? &h2[3 * i] : &h[3 * i];
        sd_sw_result &r = out[i];
        r.score = src[0];
        r.tEnd = src[1];
        r.qEnd = src[2];
        r.flags = word[i] ? 1 : 0;
        if (word[i] && r.tEnd == -1) r.tEnd = 0;   // the word kernel initialises end_ref to 0 (:962)
        if (r.score == 0) r.qEnd = 0;
        if (r.tEnd == -1) { r.evalue = 0.0; continue; }
        r.evalue = sd::computeEvalue(ev, r.score, qLv[i]);
        const bool lowE = r.evalue > par->evalThr;
        const float qCov = sd::computeCov(0, r.qEnd, qLv[i]), tCov = sd::computeCov(0, r.tEnd, tLv[i]);
        const bool lowCov = !sd::hasCoverage(par->covThr, par->covMode, qCov, tCov);
        if (par->swMode == 0 || lowE || lowCov) continue;
        goRev[i] = 1;
    }
    for (size_t x = 0; x < tasks.size(); x++) {
        const uint32_t i = tasks[x].slot;
        if (!goRev[i]) continue;
        const sd_sw_result &r = out[i];
        SwTask tk;
        tk.qOff = queries->hOff[pairQ[i]] + r.qEnd; tk.tOff = targets->hOff[pairT[i]] + r.tEnd;
        tk.n = r.qEnd + 1; tk.tL = r.tEnd + 1; tk.qStep = -1; tk.tStep = -1;
        tk.segLen = std::max(1, (tk.n + (word[i] ? 16 : 32) - 1) / (word[i] ? 16 : 32));
        tk.slot = i; tk.boundOff = 0;
        rtasks.push_back(tk);
    }
    hs.reset(new HostScope(ctx, "align.rev"));
    // ---- pass 3: start positions (reverse pass, :400-476)
    std::vector<int32_t> hr;
    rc = runScoreTasks(ctx, rtasks, queries, targets, dMat.p, go, ge, hr, nPairs, &ctx->cellsRev, "rev");
    if (rc != SD_OK) return rc;
    std::vector<TbTask> tb;
    for (size_t x = 0; x < rtasks.size(); x++) {
        const uint32_t i = rtasks[x].slot;
        sd_sw_result &r = out[i];
        if (hr[3 * i] != r.score) {
            r.flags |= 2;
            return sdFail(ctx, SD_EMISMATCH, "Score of forward/backward SW differ: %d %d (pair %u)", r.score, hr[3 * i], i);
        }
        r.tStart = r.tEnd - hr[3 * i + 1];
        r.qStart = r.qEnd - hr[3 * i + 2];
        const float qCov = sd::computeCov(r.qStart, r.qEnd, qLv[i]), tCov = sd::computeCov(r.tStart, r.tEnd, tLv[i]);
        const bool lowCov = !sd::hasCoverage(par->covThr, par->covMode, qCov, tCov);
        if (par->swMode == 1 || lowCov) continue;
        TbTask t;
        t.qAbs = queries->hOff[pairQ[i]] + r.qStart;
        t.tAbs = targets->hOff[pairT[i]] + r.tStart;
        t.qLen = r.qEnd - r.qStart + 1;
        t.tLen = r.tEnd - r.tStart + 1;
        t.score = r.score;
        t.band = std::abs(t.tLen - t.qLen) + 1;
        t.maxv = 0;
        t.slot = i;
        tb.push_back(t);
    }
    hs.reset(new HostScope(ctx, "align.traceback"));
    // ---- pass 4: banded traceback in chunks that fit the scratch budget
    if (!tb.empty() && btPool == nullptr) return sdFail(ctx, SD_EINVAL, "swMode 2 needs a backtrace pool");
    const uint64_t SCRATCH_BUDGET = 8ull << 30;
    std::vector<TbTask> pending = tb;
    while (!pending.empty()) {
        for (size_t x = 0; x < pending.size(); x++)
            if (pending[x].band > 4 * 65536) return sdFail(ctx, SD_EHIP, "Trace back error (pair %u)", pending[x].slot);
        {   // order: LDS width class, then work (row chunks x rows) descending -- stable counting sort
            auto keyOf = [&](const TbTask &t) {
                const uint32_t ci = tbBandClass(t.band) - N_TB_NARROW;
                const uint64_t work = (uint64_t) ((2 * t.band + 1 + 31) / 32) * (uint64_t) t.qLen;
                return ci * 4096u + (uint32_t) (4095 - std::min<uint64_t>(work >> 3, 4095));
            };
            std::vector<uint32_t> cnt((N_TB_CLASSES - N_TB_NARROW) * 4096 + 1, 0);
            for (size_t i = 0; i < pending.size(); i++) cnt[keyOf(pending[i]) + 1]++;
            for (size_t i = 1; i < cnt.size(); i++) cnt[i] += cnt[i - 1];
            std::vector<TbTask> sortedTb(pending.size());
            for (size_t i = 0; i < pending.size(); i++) sortedTb[cnt[keyOf(pending[i])]++] = pending[i];
            pending.swap(sortedTb);
        }
        std::vector<TbTask> next;
        size_t pos = 0;
        while (pos < pending.size()) {
            uint64_t nDir = 0, nBt = 0;
            size_t end = pos;
            const uint32_t cls = tbBandClass(pending[pos].band);
            while (end < pending.size() && tbBandClass(pending[end].band) == cls) {
                TbTask &t = pending[end];
                const uint64_t width_d = (uint64_t) t.band * 2 + 1;
                const uint64_t ad = ((cls != TB_GLOBAL ? 0 : tbGlobalIntBytes(t.band)) + width_d * (uint64_t) t.qLen + 31) & ~15ull, ab = (uint64_t) t.qLen + t.tLen + 2;
                if (end > pos && (nDir + ad) > SCRATCH_BUDGET) break;
                t.intOff = 0; t.dirOff = nDir; t.btOff = nBt;
                nDir += ad; nBt += ab;
                ctx->cellsTb += width_d * (uint64_t) t.qLen;
                end++;
            }
            const uint32_t cnt = (uint32_t) (end - pos);
            struct { TbTask *p; } dT;
            struct { int32_t *p; } dRes;
            struct { int8_t *p; } dDir;
            struct { char *p; } dBt;
            if (wsGet(ctx, "tb.tasks", cnt, &dT.p) != hipSuccess || wsGet(ctx, "tb.dir", nDir, &dDir.p) != hipSuccess ||
                wsGet(ctx, "tb.bt", nBt, &dBt.p) != hipSuccess || wsGet(ctx, "tb.res", (size_t) cnt * 2, &dRes.p) != hipSuccess)
                return sdFail(ctx, SD_ENOMEM, "traceback scratch allocation failed (%llu bytes)", (unsigned long long) nDir);
            SD_HIP(ctx, hipMemcpyAsync(dT.p, &pending[pos], cnt * sizeof(TbTask), hipMemcpyHostToDevice, ctx->stream));
            {
                ProfScope ps(ctx, TB_CLASSES[cls].scope);
                launchTbBand(ctx, queries, targets, dMat.p, go, ge, TB_CLASSES[cls], 0, dT.p, cnt, dDir.p, dBt.p, dRes.p, nullptr);
            }
            SD_HIP(ctx, hipGetLastError());
            TbTask *back = nullptr;
            char *hbt = nullptr;
            int32_t *hres = nullptr;
            SD_HIP(ctx, pinGet(ctx, "tb.back", cnt, &back));
            SD_HIP(ctx, pinGet(ctx, "tb.hbt", nBt, &hbt));
            SD_HIP(ctx, pinGet(ctx, "tb.hres", (size_t) cnt * 2, &hres));
            SD_HIP(ctx, hipMemcpyAsync(back, dT.p, cnt * sizeof(TbTask), hipMemcpyDeviceToHost, ctx->stream));
            SD_HIP(ctx, hipMemcpyAsync(hbt, dBt.p, nBt, hipMemcpyDeviceToHost, ctx->stream));
            SD_HIP(ctx, hipMemcpyAsync(hres, dRes.p, (size_t) cnt * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            SD_HIP(ctx, sdStreamSync(ctx));
            // pool offsets serially (cheap), payload copies in parallel
            std::vector<uint64_t> dst(cnt, 0);
            for (uint32_t x = 0; x < cnt; x++) {
                const TbTask &t = back[x];
                const int len = hres[2 * x];
                if (len == -2) {
                    TbTask nt = t;
                    nt.band = t.band;   // doubled by the kernel
                    next.push_back(nt);
                } else if (len < 0) {
                    return sdFail(ctx, SD_EHIP, "Trace back error for pair %u", t.slot);
                } else {
                    if (btPos + (uint64_t) len > btCap) return sdFail(ctx, SD_ENOMEM, "backtrace pool too small");
                    dst[x] = btPos;
                    btPos += len;
                }
            }
#pragma omp parallel for schedule(static)
            for (uint32_t x = 0; x < cnt; x++) {
                const int len = hres[2 * x];
                if (len < 0) continue;
                const TbTask &t = back[x];
                sd_sw_result &r = out[t.slot];
                memcpy(btPool + dst[x], hbt + t.btOff + ((size_t) (t.qLen + t.tLen + 2) - (size_t) len), len);
                r.btOffset = dst[x];
                r.btLen = len;
                r.identical = hres[2 * x + 1];
            }
            pos = end;
        }
        pending.swap(next);
    }
    hs.reset();
    if (btUsed) *btUsed = btPos;
    return SD_OK;
}

}  // extern "C"
