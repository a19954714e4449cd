// sd_clust_symmetrize: the graph half of the reference's `clust` module on the device -- what ClusteringAlgorithms::readInClusterData
// (M/src/clustering/ClusteringAlgorithms.cpp:368-464) leaves behind after AlignmentSymmetry::sortElements / findMissingLinks /
// addMissingLinks (M/src/clustering/AlignmentSymmetry.cpp:242-340): every row keeps its input entries in input order and gains one entry s
// for every input edge s -> c whose source s is not among the INPUT entries of row c, in (s, position in row s) order, with that edge's score.
//
// One stable sort of the edges by destination does both jobs.  The edge stream is in (source, position) order, so after the sort the
// edges into c lie together in (source, position) order: that is the append order of row c, and the sources of the edges into s, which
// are ascending, are exactly the set "who lists s" -- edge s -> c is missing iff c is not in it (a binary search).
//   clust_src_kernel      src[e] = row of edge e                                      (binary search in rowOff)
//   sdRadixSortPairs      (key elem[e], value e), stable, ceil(log2 n) key bits
//   clust_bounds_kernel   tOff[c] = first sorted position with destination >= c
//   gatherFields          tSrc[j] = src[value[j]]                                     (fs_gather_kernel, sd_field_sort.h)
//   clust_flag_kernel     flag[j] = destination c of j is not in tSrc[tOff[s] .. tOff[s + 1]), s = tSrc[j]
//   sdScanLaunch          fScan = exclusive sum of flag over E + 1 entries: outRowOff[c] = rowOff[c] + fScan[tOff[c]]
//   clust_copy_kernel     the input entries to their new places
//   clust_append_kernel   the flagged entries behind them
#include "sd_common.h"

#include <omp.h>

namespace {

#include "sd_scan_sort.h"
#include "sd_field_sort.h"

constexpr int CL_BLOCK = 256;

// the row r with off[r] <= e < off[r + 1] (rows may be empty)
__device__ __forceinline__ uint32_t clRowOf(const uint64_t *__restrict__ off, uint32_t n, uint64_t e) {
    uint64_t lo = 0, hi = (uint64_t) n + 1;   // first index with off[idx] > e
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= e) lo = mid + 1;
        else hi = mid;
    }
    return (uint32_t) (lo - 1);
}

__global__ void __launch_bounds__(CL_BLOCK)
clust_src_kernel(const uint64_t *__restrict__ rowOff, uint32_t n, uint32_t nEdges, uint32_t *__restrict__ src, uint32_t *__restrict__ edgeId) {
    const uint64_t e = (uint64_t) blockIdx.x * CL_BLOCK + threadIdx.x;
    if (e >= nEdges) return;
    src[e] = clRowOf(rowOff, n, e);
    edgeId[e] = (uint32_t) e;
}

__global__ void __launch_bounds__(CL_BLOCK)
clust_bounds_kernel(const uint32_t *__restrict__ sortedDst, uint32_t nEdges, uint32_t n, uint64_t *__restrict__ tOff) {
    const uint64_t c = (uint64_t) blockIdx.x * CL_BLOCK + threadIdx.x;
    if (c > n) return;
    uint64_t lo = 0, hi = nEdges;   // first position with sortedDst[pos] >= c
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t) sortedDst[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    tOff[c] = lo;
}

// flag has nEdges + 1 entries (the last one 0: the scan's total)
__global__ void __launch_bounds__(CL_BLOCK)
clust_flag_kernel(const uint32_t *__restrict__ sortedDst, const uint32_t *__restrict__ tSrc, const uint64_t *__restrict__ tOff, uint32_t nEdges,
                  uint32_t *__restrict__ flag) {
    const uint64_t j = (uint64_t) blockIdx.x * CL_BLOCK + threadIdx.x;
    if (j > nEdges) return;
    uint32_t missing = 0;
    if (j < nEdges) {
        const uint32_t c = sortedDst[j], s = tSrc[j];
        uint64_t lo = tOff[s], hi = tOff[s + 1];   // the sources of the edges into s, ascending: does c list s?
        const uint64_t end = hi;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (tSrc[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        missing = (lo < end && tSrc[lo] == c) ? 0u : 1u;
    }
    flag[j] = missing;
}

__global__ void __launch_bounds__(CL_BLOCK)
clust_offsets_kernel(const uint64_t *__restrict__ rowOff, const uint64_t *__restrict__ tOff, const uint64_t *__restrict__ fScan, uint32_t n,
                     uint64_t *__restrict__ outRowOff) {
    const uint64_t c = (uint64_t) blockIdx.x * CL_BLOCK + threadIdx.x;
    if (c <= n) outRowOff[c] = rowOff[c] + fScan[tOff[c]];
}

__global__ void __launch_bounds__(CL_BLOCK)
clust_copy_kernel(const uint64_t *__restrict__ rowOff, const uint64_t *__restrict__ outRowOff, const uint32_t *__restrict__ src,
                  const uint32_t *__restrict__ elem, const uint16_t *__restrict__ score, uint32_t nEdges, uint32_t *__restrict__ outElem,
                  uint16_t *__restrict__ outScore) {
    const uint64_t e = (uint64_t) blockIdx.x * CL_BLOCK + threadIdx.x;
    if (e >= nEdges) return;
    const uint32_t s = src[e];
    const uint64_t at = outRowOff[s] + (e - rowOff[s]);
    outElem[at] = elem[e];
    outScore[at] = score[e];
}

__global__ void __launch_bounds__(CL_BLOCK)
clust_append_kernel(const uint64_t *__restrict__ rowOff, const uint64_t *__restrict__ outRowOff, const uint64_t *__restrict__ tOff,
                    const uint64_t *__restrict__ fScan, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ sortedDst,
                    const uint32_t *__restrict__ sortedEdge, const uint32_t *__restrict__ tSrc, const uint16_t *__restrict__ score,
                    uint32_t nEdges, uint32_t *__restrict__ outElem, uint16_t *__restrict__ outScore) {
    const uint64_t j = (uint64_t) blockIdx.x * CL_BLOCK + threadIdx.x;
    if (j >= nEdges || flag[j] == 0) return;
    const uint32_t c = sortedDst[j];
    const uint64_t at = outRowOff[c] + (rowOff[c + 1] - rowOff[c]) + (fScan[j] - fScan[tOff[c]]);
    outElem[at] = tSrc[j];
    outScore[at] = score[sortedEdge[j]];
}

}  // namespace

extern "C" {

int sd_clust_symmetrize(sd_ctx *ctx, uint64_t n, const uint64_t *rowOff, const uint32_t *elem, const uint16_t *score, uint64_t outCap,
                        uint64_t *outRowOff, uint32_t *outElem, uint16_t *outScore, uint64_t *stats) {
    if (!ctx || !rowOff) return SD_EINVAL;
    (void) hipSetDevice(ctx->device);
    sdD2HReset(ctx);
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (n > (uint64_t) UINT32_MAX - 1)
        return sdFail(ctx, SD_EINVAL, "sd_clust_symmetrize: %llu rows (local ids are 32-bit and 4294967295 marks an unassigned one)", (unsigned long long) n);
    if (rowOff[0] != 0) return sdFail(ctx, SD_EINVAL, "sd_clust_symmetrize: rowOff must start at 0");
    for (uint64_t r = 0; r < n; r++)
        if (rowOff[r + 1] < rowOff[r]) return sdFail(ctx, SD_EINVAL, "sd_clust_symmetrize: rowOff descends at row %llu", (unsigned long long) r);
    const uint64_t nEdges = rowOff[n];
    if (nEdges > RS_MAX_ELEMENTS)
        return sdFail(ctx, SD_EUNSUPPORTED, "sd_clust_symmetrize: %llu entries in one call (the device sort counts in 32 bits: at most %llu)",
                      (unsigned long long) nEdges, (unsigned long long) RS_MAX_ELEMENTS);
    if (nEdges && (!elem || !score)) return SD_EINVAL;
    // checked here, so that no lane indexes outside its arrays
    {
        uint64_t first = UINT64_MAX;
#pragma omp parallel for schedule(static) reduction(min : first) if (nEdges > (1u << 16))
        for (uint64_t e = 0; e < nEdges; e++)
            if (elem[e] >= n && e < first) first = e;
        if (first != UINT64_MAX)
            return sdFail(ctx, SD_EINVAL, "sd_clust_symmetrize: entry %llu names element %u of %llu", (unsigned long long) first, elem[first],
                          (unsigned long long) n);
    }
    if (stats) stats[0] = nEdges;
    if (nEdges == 0) {   // (no rows, or only empty ones)
        if (outRowOff)
            for (uint64_t r = 0; r <= n; r++) outRowOff[r] = 0;
        return SD_OK;
    }
    const uint32_t n32 = (uint32_t) n, e32 = (uint32_t) nEdges;
    uint64_t *dRowOff = nullptr, *dTOff = nullptr, *dFScan = nullptr, *dOutOff = nullptr, *dScanTmp = nullptr;
    uint32_t *dElem = nullptr, *dSrc = nullptr, *dEdge = nullptr, *dKeyS = nullptr, *dValS = nullptr, *dKeyT = nullptr, *dValT = nullptr, *dCounts = nullptr;
    uint32_t *dFlag = nullptr;
    uint16_t *dScore = nullptr;
    SD_HIP(ctx, wsGet(ctx, "cl.rowoff", (size_t) n + 1, &dRowOff));
    SD_HIP(ctx, wsGet(ctx, "cl.toff", (size_t) n + 1, &dTOff));
    SD_HIP(ctx, wsGet(ctx, "cl.outoff", (size_t) n + 1, &dOutOff));
    SD_HIP(ctx, wsGet(ctx, "cl.elem", (size_t) nEdges, &dElem));
    SD_HIP(ctx, wsGet(ctx, "cl.score", (size_t) nEdges, &dScore));
    SD_HIP(ctx, wsGet(ctx, "cl.src", (size_t) nEdges, &dSrc));
    SD_HIP(ctx, wsGet(ctx, "cl.edge", (size_t) nEdges, &dEdge));
    SD_HIP(ctx, wsGet(ctx, "cl.keys", (size_t) nEdges, &dKeyS));
    SD_HIP(ctx, wsGet(ctx, "cl.vals", (size_t) nEdges, &dValS));
    SD_HIP(ctx, wsGet(ctx, "cl.keyt", (size_t) nEdges, &dKeyT));
    SD_HIP(ctx, wsGet(ctx, "cl.valt", (size_t) nEdges, &dValT));
    SD_HIP(ctx, wsGet(ctx, "cl.flag", (size_t) nEdges + 1, &dFlag));
    SD_HIP(ctx, wsGet(ctx, "cl.fscan", (size_t) nEdges + 1, &dFScan));
    SD_HIP(ctx, wsGet(ctx, "cl.scantmp", sdScanTmpBytes(nEdges + 1) / sizeof(uint64_t), &dScanTmp));
    SD_HIP(ctx, wsGet(ctx, "cl.counts", sdRadixSortCountsBytes() / sizeof(uint32_t), &dCounts));
    {
        HostScope hs(ctx, "clust_copy_in");
        SD_HIP(ctx, hipMemcpyAsync(dRowOff, rowOff, ((size_t) n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        SD_HIP(ctx, hipMemcpyAsync(dElem, elem, (size_t) nEdges * 4, hipMemcpyHostToDevice, ctx->stream));
        SD_HIP(ctx, hipMemcpyAsync(dScore, score, (size_t) nEdges * 2, hipMemcpyHostToDevice, ctx->stream));
        if (ctx->profiling) SD_HIP(ctx, sdStreamSync(ctx));
    }
    uint64_t added = 0;
    uint32_t *dTSrc = dValT;   // the sort's scratch pair is free once it has returned
    {
        HostScope hs(ctx, "clust_kernels");
        const int keyBits = bitsFor(n - 1);   // the destinations are 0 .. n - 1 (nEdges > 0 here, so n >= 1)
        hipLaunchKernelGGL(clust_src_kernel, dim3(gridFor(nEdges, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, (const uint64_t *) dRowOff, n32, e32, dSrc, dEdge);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, sdRadixSortPairs<uint32_t>(ctx->stream, dElem, dEdge, dKeyS, dValS, dKeyT, dValT, e32, 0, keyBits, dCounts));
        hipLaunchKernelGGL(clust_bounds_kernel, dim3(gridFor(n + 1, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, (const uint32_t *) dKeyS, e32, n32, dTOff);
        SD_HIP(ctx, gatherFields(ctx->stream, dValS, e32, 1, &dSrc, &dTSrc));
        hipLaunchKernelGGL(clust_flag_kernel, dim3(gridFor(nEdges + 1, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, (const uint32_t *) dKeyS,
                           (const uint32_t *) dTSrc, (const uint64_t *) dTOff, e32, dFlag);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, (sdScanLaunch<uint32_t, ScanSum64, false, uint64_t>(ctx->stream, dFlag, dFScan, nEdges + 1, dScanTmp)));
        hipLaunchKernelGGL(clust_offsets_kernel, dim3(gridFor(n + 1, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, (const uint64_t *) dRowOff,
                           (const uint64_t *) dTOff, (const uint64_t *) dFScan, n32, dOutOff);
        SD_HIP(ctx, hipGetLastError());
        SD_HIP(ctx, sdD2H(ctx, &added, dFScan + nEdges, 8));
        SD_HIP(ctx, sdStreamSync(ctx));
    }
    const uint64_t total = nEdges + added;
    if (stats) stats[1] = added;
    uint64_t *hOutOff = nullptr;   // (pinned: the offsets come back before the caller's array is touched)
    SD_HIP(ctx, pinGet(ctx, "cl.outoff.host", (size_t) n + 1, &hOutOff));
    SD_HIP(ctx, hipMemcpyAsync(hOutOff, dOutOff, ((size_t) n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    SD_HIP(ctx, sdStreamSync(ctx));
    if (stats) {
        uint64_t largest = 0;
        for (uint64_t r = 0; r < n; r++) largest = std::max(largest, hOutOff[r + 1] - hOutOff[r]);
        stats[2] = largest;
    }
    if (total > outCap)
        return sdFail(ctx, SD_ENOMEM, "sd_clust_symmetrize: %llu entries in the symmetric graph, room for %llu", (unsigned long long) total,
                      (unsigned long long) outCap);
    if (!outRowOff || !outElem || !outScore) return SD_EINVAL;
    uint32_t *dOutElem = nullptr;
    uint16_t *dOutScore = nullptr;
    SD_HIP(ctx, wsGet(ctx, "cl.outelem", (size_t) total, &dOutElem));
    SD_HIP(ctx, wsGet(ctx, "cl.outscore", (size_t) total, &dOutScore));
    {
        HostScope hs(ctx, "clust_kernels");
        hipLaunchKernelGGL(clust_copy_kernel, dim3(gridFor(nEdges, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, (const uint64_t *) dRowOff,
                           (const uint64_t *) dOutOff, (const uint32_t *) dSrc, (const uint32_t *) dElem, (const uint16_t *) dScore, e32, dOutElem,
                           dOutScore);
        hipLaunchKernelGGL(clust_append_kernel, dim3(gridFor(nEdges, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, (const uint64_t *) dRowOff,
                           (const uint64_t *) dOutOff, (const uint64_t *) dTOff, (const uint64_t *) dFScan, (const uint32_t *) dFlag,
                           (const uint32_t *) dKeyS, (const uint32_t *) dValS, (const uint32_t *) dTSrc, (const uint16_t *) dScore, e32, dOutElem,
                           dOutScore);
        SD_HIP(ctx, hipGetLastError());
        if (ctx->profiling) SD_HIP(ctx, sdStreamSync(ctx));
    }
    {
        HostScope hs(ctx, "clust_copy_out");
        SD_HIP(ctx, hipMemcpyAsync(outElem, dOutElem, (size_t) total * 4, hipMemcpyDeviceToHost, ctx->stream));
        SD_HIP(ctx, hipMemcpyAsync(outScore, dOutScore, (size_t) total * 2, hipMemcpyDeviceToHost, ctx->stream));
        SD_HIP(ctx, sdStreamSync(ctx));
    }
    memcpy(outRowOff, hOutOff, ((size_t) n + 1) * 8);
    return SD_OK;
}

}  // extern "C"
