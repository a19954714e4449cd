// Alignment expansion (`expandaln`): BacktraceTranslator::translateResult (M/src/commons/BacktraceTranslator.h:51-153) for a batch of
// (A -> B row, B -> C row) pairs, on run lists.
//
// Layout.  The reference advances both backtraces one column per step and maps the two states through a 3 x 3 table, so
// over run lists the translation is a merge: the next min(rest of the AB run, rest of the BC run) columns share one table entry.  Only
// the start alignment in B is a search, and it too goes run by run.  One lane owns one pair and never touches an expanded column;
// consecutive pairs share their AB row (all members of one cluster do), so the lanes of a wavefront read the same AB runs and the
// BC rows of one cluster, which lie back to back.  Pass 1 writes a fixed-size record per pair; pass 2 walks the kept pairs again and
// prints their runs as Matcher::compressAlignment does (M/src/alignment/Matcher.cpp:166-185), at the offsets an exclusive scan of the
// records' text lengths gives.
#include "sd_common.h"

namespace {

#include "sd_scan_sort.h"

constexpr int EX_BLOCK = 256;
enum { EX_M = 0, EX_I = 1, EX_D = 2, EX_NONE = 3 };
// transitions[ab][bc] (BacktraceTranslator.h:25-33), two bits per entry at 2 * (3 * ab + bc)
constexpr uint32_t EX_TABLE = (EX_M << 0) | (EX_I << 2) | (EX_D << 4) |      // ab = M
                              (EX_I << 6) | (EX_I << 8) | (EX_NONE << 10) |  // ab = I
                              (EX_D << 12) | (EX_NONE << 14) | (EX_D << 16); // ab = D

struct ExCursor {
    const uint32_t *runs;
    uint32_t i, n, rem, st;
    __device__ __forceinline__ void load() {
        if (i < n) {
            const uint32_t r = runs[i];
            st = r & 3u;
            rem = r >> 2;
        } else {
            rem = 0;
        }
    }
    __device__ __forceinline__ void take(uint32_t cols) {
        rem -= cols;
        if (rem == 0) {
            i++;
            load();
        }
    }
};

__device__ __forceinline__ uint32_t exDigits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}

// The walk of one pair: the start alignment in B (:66-97), then the lock-step loop (:107-137).  emit(state, columns) receives every
// emitted stretch in order and returns false to end the walk.
template <typename F>
__device__ __forceinline__ void exWalk(ExCursor a, ExCursor b, int startAab, int startBab, int startBbc, int startCbc, int &startA,
                                       int &startC, F &&emit) {
    a.i = 0;
    b.i = 0;
    a.load();
    b.load();
    uint32_t offA = 0, offC = 0;
    if (startBab < startBbc) {
        // AB starts earlier: its columns are passed until `dist` of them moved in B (M or D), or it ends
        const uint64_t dist = (uint64_t) ((int64_t) startBbc - (int64_t) startBab);
        uint64_t inB = 0;
        while (inB < dist && a.i < a.n) {
            uint32_t cols = a.rem;
            if (a.st != EX_I) {
                if ((uint64_t) cols > dist - inB) cols = (uint32_t) (dist - inB);
                inB += cols;
            }
            if (a.st != EX_D) offA += cols;
            a.take(cols);
        }
    } else if (startBab > startBbc) {
        // BC starts earlier: M and I move in B, M and D in C
        const uint64_t dist = (uint64_t) ((int64_t) startBab - (int64_t) startBbc);
        uint64_t inB = 0;
        while (inB < dist && b.i < b.n) {
            uint32_t cols = b.rem;
            if (b.st != EX_D) {
                if ((uint64_t) cols > dist - inB) cols = (uint32_t) (dist - inB);
                inB += cols;
            }
            if (b.st != EX_I) offC += cols;
            b.take(cols);
        }
    }
    startA = (int) ((uint32_t) startAab + offA);
    startC = (int) ((uint32_t) startCbc + offC);
    while (a.i < a.n && b.i < b.n) {
        const uint32_t cols = min(a.rem, b.rem);
        const uint32_t t = (EX_TABLE >> (2u * (3u * a.st + b.st))) & 3u;
        if (t != EX_NONE && !emit(t, cols)) return;
        a.take(cols);
        b.take(cols);
    }
}

struct ExIn {
    const int32_t *abStartA, *abStartB, *bcStartB, *bcStartC;
    const uint64_t *abRunOff, *bcRowOff, *bcRunOff, *pairOff;
    const uint32_t *abRuns, *bcRuns, *abCluster;
    uint32_t nAB;
    // mode 1 only
    int mode, gapOpen, gapExtend;
    const uint8_t *qRes, *tRes;
    const int8_t *qBias, *matrix;
    const uint64_t *qOff, *tOff;
    const uint32_t *abQuery, *bcTarget;
};

// the AB row of pair p: the last row whose first pair is <= p (rows without pairs share their successor's first pair)
__device__ __forceinline__ uint32_t exRowOfPair(const uint64_t *__restrict__ pairOff, uint32_t nAB, uint64_t p) {
    uint32_t lo = 0, hi = nAB;   // pairOff[lo] <= p < pairOff[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pairOff[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void exCursors(const ExIn &in, uint32_t ab, uint64_t bc, ExCursor &a, ExCursor &b) {
    const uint64_t a0 = in.abRunOff[ab], b0 = in.bcRunOff[bc];
    a.runs = in.abRuns + a0;
    a.n = (uint32_t) (in.abRunOff[ab + 1] - a0);
    b.runs = in.bcRuns + b0;
    b.n = (uint32_t) (in.bcRunOff[bc + 1] - b0);
}

__global__ __launch_bounds__(EX_BLOCK) void expand_records_kernel(ExIn in, uint64_t nPairs, sd_expand_result *__restrict__ out) {
    const uint64_t p = (uint64_t) blockIdx.x * EX_BLOCK + threadIdx.x;
    if (p >= nPairs) return;
    const uint32_t ab = exRowOfPair(in.pairOff, in.nAB, p);
    const uint64_t bc = in.bcRowOff[in.abCluster[ab]] + (p - in.pairOff[ab]);
    ExCursor a, b;
    exCursors(in, ab, bc, a, b);
    // the text is counted as compressAlignment forms it: it starts in state M with no column, so a first run of another state
    // leaves "0M" behind
    uint32_t cols = 0, lastM = 0, qAln = 0, dbAln = 0, cur = EX_M, curLen = 0, doneRuns = 0, doneText = 0, runsAtM = 0, textAtM = 0;
    int startA, startC;
    // mode 1, rescoreResultByBacktrace (expandaln.cpp:27-76) along the way: the walk's own positions (I moves the query, D the target),
    // its running score and identities, and their values behind the last M -- what the walk over the printed backtrace ends with.  Every M
    // stretch is printed, so every residue that is read belongs to the printed walk; one that lies outside a sequence is not read
    const bool walk = in.mode == 1;
    int64_t wq = 0, wt = 0, aLen = 0, cLen = 0;
    int sc = 0, id = 0, scAtM = 0, idAtM = 0;
    bool leaves = false;
    const uint8_t *qr = nullptr, *tr = nullptr;
    const int8_t *qb = nullptr;
    if (walk) {
        const uint32_t qs = in.abQuery[ab], ts = in.bcTarget[bc];
        const uint64_t q0 = in.qOff[qs], t0 = in.tOff[ts];
        aLen = (int64_t) (in.qOff[qs + 1] - q0);
        cLen = (int64_t) (in.tOff[ts + 1] - t0);
        qr = in.qRes + q0;
        tr = in.tRes + t0;
        qb = in.qBias ? in.qBias + q0 : nullptr;
    }
    exWalk(a, b, in.abStartA[ab], in.abStartB[ab], in.bcStartB[bc], in.bcStartC[bc], startA, startC, [&](uint32_t t, uint32_t n) {
        if (t == cur) {
            curLen += n;
        } else {
            doneRuns++;
            doneText += exDigits(curLen) + 1u;
            cur = t;
            curLen = n;
        }
        if (walk) {
            if (t == EX_M) {
                const int64_t q = (int64_t) startA + wq, c = (int64_t) startC + wt;
                if (q < 0 || c < 0 || q + n > aLen || c + n > cLen) {
                    leaves = true;
                } else if (!leaves) {
                    for (uint32_t j = 0; j < n; j++) {
                        const uint32_t x = min((uint32_t) qr[q + j], 20u), y = min((uint32_t) tr[c + j], 20u);   // the matrix has 21 codes
                        sc += in.matrix[x * 21u + y] + (qb ? qb[q + j] : 0);
                        id += x == y ? 1 : 0;
                    }
                }
                wq += n;
                wt += n;
            } else {
                // the first column of a gap run opens (curLen == n: the run began with this stretch)
                sc -= curLen == n ? in.gapOpen + (int) (n - 1u) * in.gapExtend : (int) n * in.gapExtend;
                if (t == EX_I) wq += n;
                else wt += n;
            }
        }
        cols += n;
        if (t != EX_I) qAln += n;     // qAlnLength: M and D (:117-124)
        if (t != EX_D) dbAln += n;    // dbAlnLength: M and I
        if (t == EX_M) {
            lastM = cols;
            runsAtM = doneRuns + 1u;
            textAtM = doneText + exDigits(curLen) + 1u;
            scAtM = sc;
            idAtM = id;
        }
        return true;
    });
    sd_expand_result r;
    r.aStart = startA;
    r.aEnd = (int) ((uint32_t) startA + qAln - 1u);
    r.cStart = startC;
    r.cEnd = (int) ((uint32_t) startC + dbAln - 1u);
    r.btLen = (int) lastM;
    r.nRuns = (int) runsAtM;
    r.textLen = (int) textAtM;
    r.flags = (lastM == 0 ? SD_EXPAND_EMPTY : 0) | (leaves ? SD_EXPAND_LEAVES_SEQUENCE : 0);
    r.rawScore = leaves ? 0 : scAtM;
    r.identities = leaves ? 0 : idAtM;
    r.abRow = ab;
    r.bcRow = (uint32_t) bc;
    out[p] = r;
}

__global__ __launch_bounds__(EX_BLOCK) void expand_text_len_kernel(const sd_expand_result *__restrict__ res, const uint64_t *__restrict__ kept,
                                                                   uint64_t nKept, uint32_t *__restrict__ len) {
    const uint64_t k = (uint64_t) blockIdx.x * EX_BLOCK + threadIdx.x;
    if (k < nKept) len[k] = (uint32_t) res[kept[k]].textLen;
}

struct ExWriter {
    char *at, *end;
    __device__ __forceinline__ void put(char c) {
        if (at < end) *at = c;
        at++;
    }
    __device__ __forceinline__ void run(uint32_t len, uint32_t st) {
        char d[10];
        int n = 0;
        do {
            d[n++] = (char) ('0' + len % 10u);
            len /= 10u;
        } while (len);
        while (n) put(d[--n]);
        put(st == EX_M ? 'M' : st == EX_I ? 'I' : 'D');
    }
};

__global__ __launch_bounds__(EX_BLOCK) void expand_text_kernel(ExIn in, const sd_expand_result *__restrict__ res, const uint64_t *__restrict__ kept,
                                                               uint64_t nKept, const uint64_t *__restrict__ poolOff, char *__restrict__ pool) {
    const uint64_t k = (uint64_t) blockIdx.x * EX_BLOCK + threadIdx.x;
    if (k >= nKept) return;
    const sd_expand_result r = res[kept[k]];
    ExCursor a, b;
    exCursors(in, r.abRow, r.bcRow, a, b);
    // never past the pair's own slot, whatever the record says
    ExWriter w = {pool + poolOff[k], pool + poolOff[k] + (uint32_t) r.textLen};
    const uint32_t want = (uint32_t) r.btLen;   // the printed backtrace ends behind the last M
    uint32_t cols = 0, cur = EX_M, curLen = 0;
    int startA, startC;
    exWalk(a, b, in.abStartA[r.abRow], in.abStartB[r.abRow], in.bcStartB[r.bcRow], in.bcStartC[r.bcRow], startA, startC,
           [&](uint32_t t, uint32_t n) {
               n = min(n, want - cols);
               if (t == cur) {
                   curLen += n;
               } else {
                   w.run(curLen, cur);
                   cur = t;
                   curLen = n;
               }
               cols += n;
               return cols < want;
           });
    w.run(curLen, cur);
}

template <typename T>
int exUpload(sd_ctx *ctx, const char *key, const T *src, size_t n, const T **out) {
    T *d = nullptr;
    SD_HIP(ctx, wsGet(ctx, key, n, &d));
    if (n) SD_HIP(ctx, hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *out = d;
    return SD_OK;
}

ExIn exInOf(const sd_ctx::ExpandState &s) {
    ExIn in;
    memset(&in, 0, sizeof(in));
    in.abStartA = s.abStartA;
    in.abStartB = s.abStartB;
    in.bcStartB = s.bcStartB;
    in.bcStartC = s.bcStartC;
    in.abRunOff = s.abRunOff;
    in.bcRowOff = s.bcRowOff;
    in.bcRunOff = s.bcRunOff;
    in.pairOff = s.pairOff;
    in.abRuns = s.abRuns;
    in.bcRuns = s.bcRuns;
    in.abCluster = s.abCluster;
    in.nAB = s.nAB;
    return in;
}

// 0 when the runs [0, n) are all M / I / D of at least one column, else 1 + the index of the first that is not
uint64_t exBadRun(const uint32_t *runs, uint64_t n) {
    uint64_t first = UINT64_MAX;
#pragma omp parallel for schedule(static) reduction(min : first) if (n > (1u << 16))
    for (uint64_t i = 0; i < n; i++)
        if (((runs[i] & 3u) == 3u || (runs[i] >> 2) == 0) && i < first) first = i;
    return first == UINT64_MAX ? 0 : first + 1;
}

}  // namespace

extern "C" {

int sd_expand_batch(sd_ctx *ctx, const sd_expand_params *par, uint32_t nAB, const int32_t *abStartA, const int32_t *abStartB,
                    const uint64_t *abRunOff, const uint32_t *abRuns, const uint32_t *abCluster, uint32_t nClusters,
                    const uint64_t *bcRowOff, const int32_t *bcStartB, const int32_t *bcStartC, const uint64_t *bcRunOff,
                    const uint32_t *bcRuns, const sd_seqset *queries, const sd_seqset *targets, const uint32_t *abQuery,
                    const uint32_t *bcTarget, uint64_t resultCap, sd_expand_result *results, uint64_t *nPairsOut) {
    if (!ctx || !par) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    ctx->expand = sd_ctx::ExpandState();
    if (nPairsOut) *nPairsOut = 0;
    if (par->mode != 0 && par->mode != 1) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: expansion mode %d", (int) par->mode);
    const bool walk = par->mode == 1;
    if (walk) {
        if (!queries || !targets) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: expansion mode 1 takes both sequence sets");
        if (queries->dProf || targets->dProf)
            return sdFail(ctx, SD_EUNSUPPORTED, "sd_expand_batch: expansion mode 1 takes sequence sets (profile sets are not implemented)");
    }
    if (nAB == 0) return SD_OK;
    if (!abStartA || !abStartB || !abRunOff || !abCluster || !bcRowOff || !bcRunOff) return SD_EINVAL;
    // the tables the kernels index with: checked here, so that no lane reads or writes outside its arrays
    for (uint32_t c = 0; c < nClusters; c++)
        if (bcRowOff[c + 1] < bcRowOff[c]) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: bcRowOff descends at cluster %u", c);
    const uint64_t nBC = bcRowOff[nClusters];
    if (bcRowOff[0] != 0 || nBC > UINT32_MAX) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: bcRowOff must start at 0 and name fewer than 2^32 rows");
    if (nBC && (!bcStartB || !bcStartC)) return SD_EINVAL;
    for (uint64_t r = 0; r < nBC; r++)
        if (bcRunOff[r + 1] < bcRunOff[r]) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: bcRunOff descends at row %llu", (unsigned long long) r);
    for (uint32_t i = 0; i < nAB; i++)
        if (abRunOff[i + 1] < abRunOff[i]) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: abRunOff descends at row %u", i);
    const uint64_t nAbRuns = abRunOff[nAB] - abRunOff[0], nBcRuns = bcRunOff[nBC] - bcRunOff[0];
    if (abRunOff[0] != 0 || bcRunOff[0] != 0) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: run offsets must start at 0");
    if ((nAbRuns && !abRuns) || (nBcRuns && !bcRuns)) return SD_EINVAL;
    if (const uint64_t bad = exBadRun(abRuns, nAbRuns))
        return sdFail(ctx, SD_EINVAL, "sd_expand_batch: AB run %llu is no M / I / D run of at least one column", (unsigned long long) (bad - 1));
    if (const uint64_t bad = exBadRun(bcRuns, nBcRuns))
        return sdFail(ctx, SD_EINVAL, "sd_expand_batch: BC run %llu is no M / I / D run of at least one column", (unsigned long long) (bad - 1));
    if (walk) {
        if (!abQuery || (nBC && !bcTarget)) return SD_EINVAL;
        for (uint32_t i = 0; i < nAB; i++)
            if (abQuery[i] >= queries->n) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: AB row %u names query %u of %u", i, abQuery[i], queries->n);
        for (uint64_t r = 0; r < nBC; r++)
            if (bcTarget[r] >= targets->n)
                return sdFail(ctx, SD_EINVAL, "sd_expand_batch: BC row %llu names target %u of %u", (unsigned long long) r, bcTarget[r], targets->n);
    }
    // (pinned and the context's own: the upload below may still read it when a later step of this call fails and returns)
    uint64_t *pairOff = nullptr;
    SD_HIP(ctx, pinGet(ctx, "ex.pairoff.host", (size_t) nAB + 1, &pairOff));
    pairOff[0] = 0;
    std::vector<uint64_t> clusterRuns((size_t) nClusters, 0);
    for (uint32_t c = 0; c < nClusters; c++) clusterRuns[c] = bcRunOff[bcRowOff[c + 1]] - bcRunOff[bcRowOff[c]];
    uint64_t runsRead = 0;
    for (uint32_t i = 0; i < nAB; i++) {
        const uint32_t c = abCluster[i];
        if (c != UINT32_MAX && c >= nClusters) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: AB row %u names cluster %u of %u", i, c, nClusters);
        const uint64_t rows = c == UINT32_MAX ? 0 : bcRowOff[c + 1] - bcRowOff[c];
        pairOff[i + 1] = pairOff[i] + rows;
        if (rows) runsRead += rows * (abRunOff[i + 1] - abRunOff[i]) + clusterRuns[c];
    }
    const uint64_t nPairs = pairOff[nAB];
    if (nPairs >= ((uint64_t) 1 << 32)) return sdFail(ctx, SD_EINVAL, "sd_expand_batch: %llu pairs in one call (2^32 and more are not taken)", (unsigned long long) nPairs);
    if (nPairsOut) *nPairsOut = nPairs;
    if (nPairs > resultCap) return sdFail(ctx, SD_ENOMEM, "sd_expand_batch: %llu pairs, room for %llu records", (unsigned long long) nPairs, (unsigned long long) resultCap);
    if (nPairs == 0) return SD_OK;
    if (!results) return SD_EINVAL;
    sd_ctx::ExpandState &s = ctx->expand;
    int rc;
    if ((rc = exUpload(ctx, "ex.absa", abStartA, nAB, &s.abStartA)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.absb", abStartB, nAB, &s.abStartB)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.abro", abRunOff, (size_t) nAB + 1, &s.abRunOff)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.abr", abRuns, nAbRuns, &s.abRuns)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.abc", abCluster, nAB, &s.abCluster)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.bcrow", bcRowOff, (size_t) nClusters + 1, &s.bcRowOff)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.bcsb", bcStartB, nBC, &s.bcStartB)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.bcsc", bcStartC, nBC, &s.bcStartC)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.bcro", bcRunOff, (size_t) nBC + 1, &s.bcRunOff)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.bcr", bcRuns, nBcRuns, &s.bcRuns)) != SD_OK) return rc;
    if ((rc = exUpload(ctx, "ex.pairoff", (const uint64_t *) pairOff, (size_t) nAB + 1, &s.pairOff)) != SD_OK) return rc;
    sd_expand_result *dRes = nullptr;
    SD_HIP(ctx, wsGet(ctx, "ex.res", (size_t) nPairs, &dRes));
    s.nAB = nAB;
    ExIn in = exInOf(s);
    if (walk) {
        const int8_t *dMat = nullptr;
        if ((rc = exUpload(ctx, "ex.matrix", par->matrix, (size_t) 441, &dMat)) != SD_OK) return rc;
        if ((rc = exUpload(ctx, "ex.abq", abQuery, nAB, &in.abQuery)) != SD_OK) return rc;
        if ((rc = exUpload(ctx, "ex.bct", bcTarget, nBC, &in.bcTarget)) != SD_OK) return rc;
        in.mode = 1;
        in.gapOpen = par->gapOpen;
        in.gapExtend = par->gapExtend;
        in.matrix = dMat;
        in.qRes = queries->dRes;
        in.qBias = queries->dBias;
        in.qOff = queries->dOff;
        in.tRes = targets->dRes;
        in.tOff = targets->dOff;
    }
    {
        ProfScope ps(ctx, "expand_records");
        hipLaunchKernelGGL(expand_records_kernel, dim3((unsigned) ((nPairs + EX_BLOCK - 1) / EX_BLOCK)), dim3(EX_BLOCK), 0, ctx->stream, in, nPairs, dRes);
        SD_HIP(ctx, hipGetLastError());
    }
    SD_HIP(ctx, hipMemcpyAsync(results, dRes, (size_t) nPairs * sizeof(sd_expand_result), hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    s.res = dRes;
    s.nPairs = nPairs;
    s.runsRead = runsRead;
    s.bytesWritten = nPairs * sizeof(sd_expand_result);
    return SD_OK;
}

int sd_expand_backtraces(sd_ctx *ctx, uint64_t nKept, const uint64_t *keptPairs, char *pool, uint64_t poolCap, uint64_t *poolOff) {
    if (!ctx || !poolOff) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    poolOff[0] = 0;
    if (nKept == 0) return SD_OK;
    const sd_ctx::ExpandState &s = ctx->expand;
    if (!keptPairs) return SD_EINVAL;
    if (!s.res) return sdFail(ctx, SD_EINVAL, "sd_expand_backtraces: no sd_expand_batch call on this context to take the pairs from");
    for (uint64_t k = 0; k < nKept; k++)
        if (keptPairs[k] >= s.nPairs)
            return sdFail(ctx, SD_EINVAL, "sd_expand_backtraces: kept pair %llu is pair %llu of %llu", (unsigned long long) k,
                          (unsigned long long) keptPairs[k], (unsigned long long) s.nPairs);
    uint64_t *dKept = nullptr, *dOff = nullptr, *dTmp = nullptr;
    uint32_t *dLen = nullptr;
    SD_HIP(ctx, wsGet(ctx, "ex.kept", (size_t) nKept, &dKept));
    SD_HIP(ctx, wsGet(ctx, "ex.len", (size_t) nKept + 1, &dLen));
    SD_HIP(ctx, wsGet(ctx, "ex.off", (size_t) nKept + 1, &dOff));
    SD_HIP(ctx, wsGet(ctx, "ex.scan", sdScanTmpBytes(nKept + 1) / sizeof(uint64_t), &dTmp));
    SD_HIP(ctx, hipMemcpyAsync(dKept, keptPairs, (size_t) nKept * 8, hipMemcpyHostToDevice, ctx->stream));
    SD_HIP(ctx, hipMemsetAsync(dLen + nKept, 0, 4, ctx->stream));
    const unsigned grid = (unsigned) ((nKept + EX_BLOCK - 1) / EX_BLOCK);
    hipLaunchKernelGGL(expand_text_len_kernel, dim3(grid), dim3(EX_BLOCK), 0, ctx->stream, s.res, (const uint64_t *) dKept, nKept, dLen);
    SD_HIP(ctx, hipGetLastError());
    // exclusive over nKept + 1 lengths (the last one 0): poolOff[nKept] is the total
    SD_HIP(ctx, (sdScanLaunch<uint32_t, ScanSum64, false, uint64_t>(ctx->stream, dLen, dOff, nKept + 1, dTmp)));
    SD_HIP(ctx, hipMemcpyAsync(poolOff, dOff, (size_t) (nKept + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    const uint64_t total = poolOff[nKept];
    if (total > poolCap) return sdFail(ctx, SD_ENOMEM, "sd_expand_backtraces: %llu bytes of text, room for %llu", (unsigned long long) total, (unsigned long long) poolCap);
    if (total == 0) return SD_OK;
    if (!pool) return SD_EINVAL;
    char *dPool = nullptr;
    SD_HIP(ctx, wsGet(ctx, "ex.pool", (size_t) total, &dPool));
    {
        ProfScope ps(ctx, "expand_text");
        hipLaunchKernelGGL(expand_text_kernel, dim3(grid), dim3(EX_BLOCK), 0, ctx->stream, exInOf(s), s.res, (const uint64_t *) dKept, nKept,
                           (const uint64_t *) dOff, dPool);
        SD_HIP(ctx, hipGetLastError());
    }
    SD_HIP(ctx, hipMemcpyAsync(pool, dPool, (size_t) total, hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    ctx->expand.bytesWritten += total;
    return SD_OK;
}

int sd_expand_last_stats(sd_ctx *ctx, uint64_t *pairs, uint64_t *runsRead, uint64_t *bytesWritten) {
    if (!ctx) return SD_EINVAL;
    if (pairs) *pairs = ctx->expand.nPairs;
    if (runsRead) *runsRead = ctx->expand.runsRead;
    if (bytesWritten) *bytesWritten = ctx->expand.bytesWritten;
    return SD_OK;
}

}  // extern "C"
