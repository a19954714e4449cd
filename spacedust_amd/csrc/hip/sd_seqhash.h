// Util::hash (M/src/commons/Util.h: h = 31 h + x over the reduced codes, 64-bit wrapping) of one sequence by one wavefront.  Included by
// sd_kmermatch.hip (the identity record: XXH64 of this value) and sd_clusthash.hip (the value itself) inside their anonymous namespaces.
#ifndef SD_SEQHASH_H
#define SD_SEQHASH_H

__device__ __forceinline__ uint64_t sdPow31(uint32_t e) {
    uint64_t r = 1, b = 31;
    while (e) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

// sum x_i 31^(L - 1 - i) over 64 lane blocks of consecutive residues; every lane returns the whole sum.  map: 21-letter code -> reduced
// code (LDS or global); res: the sequence's 21-letter codes
__device__ __forceinline__ uint64_t sdSeqHash31(const uint8_t *map, const uint8_t *__restrict__ res, uint32_t L, int lane) {
    const uint32_t per = (L + 63) / 64;
    const uint32_t from = (uint32_t) lane * per < L ? (uint32_t) lane * per : L;
    const uint32_t to = from + per < L ? from + per : L;
    uint64_t h = 0;
    for (uint32_t i = from; i < to; i++) h = h * 31 + map[res[i]];
    h *= sdPow31(L - to);
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
    return h;
}

#endif
