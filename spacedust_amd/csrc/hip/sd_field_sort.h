// Sorting records by several 32-bit fields: chained stable sdRadixSortPairs passes over a permutation, least significant field first,
// and the gather of the fields into the sorted order behind it -- what the grouping modules (sd_kmermatch.hip, sd_clusthash.hip,
// sd_clust.hip) share.  Included like sd_scan_sort.h, inside the includer's anonymous namespace and after it.
#ifndef SD_FIELD_SORT_H
#define SD_FIELD_SORT_H

constexpr int FS_BLOCK = 256;

inline unsigned gridFor(uint64_t items, unsigned block) { return (unsigned) ((items + block - 1) / block); }
// key bits a sort needs for values up to maxValue (at least 1, at most 32)
inline int bitsFor(uint64_t maxValue) {
    int b = 1;
    while (b < 32 && ((uint64_t) 1 << b) <= maxValue) b++;
    return b;
}

// one link of the chain: keyOut[i] = f(field[perm[i]]) (perm null: the identity)
enum { FS_PLAIN = 0, FS_FROM_TOP = 1, FS_BIASED = 2 };   // v, arg - v (descending), v + arg (a signed value as an unsigned one)
__global__ void __launch_bounds__(FS_BLOCK)
fs_key_kernel(const uint32_t *__restrict__ field, const uint32_t *__restrict__ perm, uint32_t n, int mode, uint32_t arg,
              uint32_t *__restrict__ keyOut, uint32_t *__restrict__ permOut) {
    const uint64_t i = (uint64_t) blockIdx.x * FS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = perm ? perm[i] : (uint32_t) i;
    const uint32_t v = field[src];
    keyOut[i] = mode == FS_FROM_TOP ? arg - v : mode == FS_BIASED ? v + arg : v;
    if (permOut) permOut[i] = src;
}

__global__ void __launch_bounds__(FS_BLOCK)
fs_gather_kernel(const uint32_t *__restrict__ field, const uint32_t *__restrict__ perm, uint32_t n, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t) blockIdx.x * FS_BLOCK + threadIdx.x;
    if (i < n) out[i] = field[perm[i]];
}

// the chain's buffers: a link's (key, permutation) input and the sort's two buffer pairs, `count` elements each
struct FieldSortBufs {
    uint32_t *keyIn, *permIn, *keyA, *permA, *keyB, *permB, *counts;
};
// ... from the context's workspace, under the keys <prefix>keyin, permin, keya, perma, keyb, permb and counts
inline hipError_t fieldSortBufsGet(sd_ctx *ctx, const char *prefix, size_t count, FieldSortBufs *b) {
    const std::string p(prefix);
    uint32_t **const bufs[6] = {&b->keyIn, &b->permIn, &b->keyA, &b->permA, &b->keyB, &b->permB};
    const char *const names[6] = {"keyin", "permin", "keya", "perma", "keyb", "permb"};
    for (int i = 0; i < 6; i++) {
        const hipError_t e = wsGet(ctx, (p + names[i]).c_str(), count, bufs[i]);
        if (e != hipSuccess) return e;
    }
    return wsGet(ctx, (p + "counts").c_str(), sdRadixSortCountsBytes() / sizeof(uint32_t), &b->counts);
}

// the n records in their current order (perm, or the identity when null), stably sorted by f(field); the new order lands in b.permA
inline hipError_t sortByField(hipStream_t st, const FieldSortBufs &b, const uint32_t *field, const uint32_t *perm, uint32_t n, int mode,
                              uint32_t arg, int bits) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fs_key_kernel, dim3(gridFor(n, FS_BLOCK)), dim3(FS_BLOCK), 0, st, field, perm, n, mode, arg, b.keyIn, b.permIn);
    return sdRadixSortPairs<uint32_t>(st, b.keyIn, b.permIn, b.keyA, b.permA, b.keyB, b.permB, n, 0, bits, b.counts);
}

// dst[f][i] = src[f][perm[i]] for every field f: one launch per field
inline hipError_t gatherFields(hipStream_t st, const uint32_t *perm, uint32_t n, int nFields, const uint32_t *const *src, uint32_t *const *dst) {
    if (n == 0) return hipSuccess;
    for (int f = 0; f < nFields; f++)
        hipLaunchKernelGGL(fs_gather_kernel, dim3(gridFor(n, FS_BLOCK)), dim3(FS_BLOCK), 0, st, src[f], perm, n, dst[f]);
    return hipGetLastError();
}

#endif
