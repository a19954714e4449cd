// Host-side checks that the modules taking a whole sequence batch in one call share (sd_kmermatch.hip, sd_clusthash.hip): the input
// checks, whether the batch fits the device, and the join of a 64-bit value that left the device as two 32-bit arrays.
#ifndef SD_BATCH_CHECK_H
#define SD_BATCH_CHECK_H

#include "sd_common.h"

struct SdSeqBatch {
    uint64_t maxLen, total;   // longest sequence; residues of all
    uint8_t map[24];          // 21-letter code -> reduced code
};

// A batch of nSeq sequences (offsets[nSeq + 1] into residues, 21-letter codes) and its letter map onto alphabetSize codes: refuses, in this
// order, a letter mapped outside the alphabet, offsets that do not start at 0 or descend, a sequence beyond INT32_MAX / 2 residues and a
// residue code above 20 (checked here, so that no lane indexes outside its tables).  `who` names the entry point in messages.
inline int sdCheckSeqBatch(sd_ctx *ctx, const char *who, int alphabetSize, uint64_t nSeq, const uint8_t *residues, const uint64_t *offsets,
                           const uint8_t *letterMap, SdSeqBatch *out) {
    memset(out, 0, sizeof(*out));
    for (int a = 0; a < 21; a++) {
        if (letterMap[a] >= alphabetSize) return sdFail(ctx, SD_EINVAL, "%s: letter %d maps to %d of %d", who, a, letterMap[a], alphabetSize);
        out->map[a] = letterMap[a];
    }
    if (offsets[0] != 0) return sdFail(ctx, SD_EINVAL, "%s: offsets must start at 0", who);
    for (uint64_t s = 0; s < nSeq; s++) {
        if (offsets[s + 1] < offsets[s]) return sdFail(ctx, SD_EINVAL, "%s: offsets descend at sequence %llu", who, (unsigned long long) s);
        const uint64_t L = offsets[s + 1] - offsets[s];
        if (L > (uint64_t) INT32_MAX / 2) return sdFail(ctx, SD_EINVAL, "%s: sequence %llu has %llu residues", who, (unsigned long long) s, (unsigned long long) L);
        out->maxLen = std::max(out->maxLen, L);
    }
    const uint64_t total = out->total = offsets[nSeq];
    uint64_t bad = UINT64_MAX;
#pragma omp parallel for schedule(static) reduction(min : bad) if (total > (1u << 16))
    for (uint64_t i = 0; i < total; i++)
        if (residues[i] >= 21 && i < bad) bad = i;
    if (bad != UINT64_MAX) return sdFail(ctx, SD_EINVAL, "%s: residue %llu has code %u (0 .. 20)", who, (unsigned long long) bad, residues[bad]);
    return SD_OK;
}

// what the context's workspace holds under keys that start with prefix
inline uint64_t wsHeldBytes(sd_ctx *ctx, const char *prefix) {
    uint64_t held = 0;
    for (auto &e : ctx->ws)
        if (e.first.compare(0, strlen(prefix), prefix) == 0) held += e.second.bytes;
    return held;
}
// the bytes a module whose workspace keys start with prefix can fill: what is free on the device and what its workspace already holds
inline hipError_t wsAvailableBytes(sd_ctx *ctx, const char *prefix, uint64_t *avail) {
    size_t freeB = 0, totalB = 0;
    const hipError_t e = hipMemGetInfo(&freeB, &totalB);
    *avail = (uint64_t) freeB + wsHeldBytes(ctx, prefix);
    return e;
}

inline void sdJoinHiLo(const uint32_t *hi, const uint32_t *lo, uint64_t n, uint64_t *out) {
    for (uint64_t i = 0; i < n; i++) out[i] = ((uint64_t) hi[i] << 32) | lo[i];
}

#endif
