// A device target (the prefilter's k-mer index, resident in HBM) from sequences: the one place that fetches the tables sd_target_build
// needs and calls it.  Header-only over the C ABI, so the library's search object (sd_search.cpp) and the sdgpu modules (csrc/cli/) share
// it without a new exported symbol.
#ifndef SD_TARGET_BUILD_H
#define SD_TARGET_BUILD_H

#include "spacedust_gpu.h"

#include <cstdint>
#include <cstdlib>

// the extended 2-mer and 3-mer score tables every target carries
struct SdExtTables {
    const int16_t *s2, *s3;
    const uint16_t *i2, *i3;
    explicit SdExtTables(sd_host *host) {
        uint32_t z2, z3;
        sd_host_ext_matrix(host, 2, &s2, &i2, &z2);
        sd_host_ext_matrix(host, 3, &s3, &i3, &z3);
    }
};

// an index that exists in host arrays (read from TARGET.idx, or built by the host) uploaded as a target; kBase: the block bases of a
// wide index (>= 2^32 entries), else NULL
static inline int sdUploadTarget(sd_host *host, sd_ctx *ctx, int k, const uint32_t *kOff, const uint64_t *kBase, const uint32_t *eSeq,
                                 const uint16_t *ePos, uint64_t nEntries, const uint8_t *masked, const uint64_t *offsets, uint32_t n,
                                 sd_target **out) {
    const SdExtTables x(host);
    return sd_target_create_wide(ctx, k, kOff, kBase, eSeq, ePos, nEntries, masked, offsets, n, x.s2, x.i2, x.s3, x.i3, out);
}

// IndexBuilder::fillDatabase on the device (mask, k-mer lists, list starts); under SD_INDEX_HOST the host builds the index and the arrays
// are uploaded.  stats: {entries, masked residues}.  *what names the call a failure came from (sd_last_error(ctx) says why for the
// device's).
static inline int sdBuildTarget(sd_host *host, sd_ctx *ctx, int k, int indexThr, int mask, double maskProb, const uint8_t *residues,
                                const uint64_t *offsets, uint32_t n, sd_target **out, uint64_t stats[2], const char **what) {
    if (!getenv("SD_INDEX_HOST")) {
        const SdExtTables x(host);
        double ratios[21 * 21];
        int8_t self[21];
        sd_host_index_tables(host, ratios, self);
        uint64_t st[4] = {0, 0, 0, 0};
        *what = "sd_target_build";
        const int rc = sd_target_build(ctx, k, indexThr, mask, maskProb, residues, offsets, n, ratios, self, x.s2, x.i2, x.s3, x.i3, out, st);
        stats[0] = st[0];
        stats[1] = st[1];
        return rc;
    }
    sd_host_index *ix = nullptr;
    *what = "sd_host_index_build";
    int rc = sd_host_index_build(host, residues, offsets, n, k, indexThr, mask, maskProb, &ix);
    if (rc != SD_OK) return rc;
    const uint32_t *kOff, *eSeq;
    const uint16_t *ePos;
    const uint8_t *masked;
    const uint64_t *kBase;
    uint64_t tableSize = 0;
    sd_host_index_info(ix, &tableSize, &stats[0], &stats[1]);
    sd_host_index_arrays(ix, &kOff, &eSeq, &ePos, &masked);
    sd_host_index_block_base(ix, &kBase, nullptr);
    *what = "sd_target_create";
    rc = sdUploadTarget(host, ctx, k, kOff, kBase, eSeq, ePos, stats[0], masked, offsets, n, out);
    sd_host_index_destroy(ix);   // the host copy is not needed once the target is resident
    return rc;
}

// the index of a profile target DB (similar k-mers of every profile window at the profile threshold, consensus lookup; no masking, no
// extended tables) from Sequence::mapProfile's arrays.  stats: {entries, 0}.
static inline int sdBuildProfileTarget(sd_ctx *ctx, int k, int kmerThr, const uint8_t *letters, const uint8_t *consensus, const int16_t *sortedScore,
                                       const uint8_t *sortedIndex, const uint64_t *offsets, uint32_t n, sd_target **out, uint64_t stats[2]) {
    uint64_t st[4] = {0, 0, 0, 0};
    const int rc = sd_target_build_profile(ctx, k, kmerThr, letters, consensus, sortedScore, sortedIndex, offsets, n, out, st);
    stats[0] = st[0];
    stats[1] = st[1];
    return rc;
}

// the similar-k-mer index of a sequence target DB (--target-search-mode 1): similar k-mers of every window at the sequence threshold,
// unmasked lookup.  stats: {entries, 0}.
static inline int sdBuildSimilarTarget(sd_host *host, sd_ctx *ctx, int k, int kmerThr, const uint8_t *residues, const uint64_t *offsets, uint32_t n,
                                       sd_target **out, uint64_t stats[2]) {
    const SdExtTables x(host);
    uint64_t st[4] = {0, 0, 0, 0};
    const int rc = sd_target_build_similar(ctx, k, kmerThr, residues, offsets, n, x.s3, x.i3, out, st);
    stats[0] = st[0];
    stats[1] = st[1];
    return rc;
}

#endif
