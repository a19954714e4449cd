// Host stages of `clusthash` (M/src/util/clusthash.cpp): the identity threshold as an integer per length and the text of
// the alignment DB.  Hash, sort and the greedy pass over the groups are csrc/hip/sd_clusthash.hip.
#include "sd_host.h"
#include "spacedust_gpu.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

// clusthash.cpp:155-156, in the reference's types
inline bool reaches(uint32_t d, uint32_t L, float seqIdThr) {
    const float seqId = (static_cast<float>(d)) / static_cast<float>(L);
    return seqId >= seqIdThr;
}

// "\t0\t0\tL-1\tL\t0\tL-1\tL\n" behind the identity column
char *tail(uint32_t L, char *p) {
    memcpy(p, "\t0\t0\t", 5);
    p += 5;
    p = sd::u32toa(L - 1, p);
    *p++ = '\t';
    p = sd::u32toa(L, p);
    memcpy(p, "\t0\t", 3);
    p += 3;
    p = sd::u32toa(L - 1, p);
    *p++ = '\t';
    p = sd::u32toa(L, p);
    *p++ = '\n';
    return p;
}

}  // namespace

extern "C" {

uint32_t sd_host_clusthash_min_identical(float seqIdThr, uint32_t L) {
    if (L == 0 || !reaches(L, L, seqIdThr)) return L + 1;   // (a NaN threshold ends here too)
    // the quotient is monotone in d: start beside thr * L and walk to the boundary
    const double est = std::ceil((double) seqIdThr * (double) L);
    uint32_t d = est <= 0.0 ? 0 : est >= (double) L ? L : (uint32_t) est;
    while (d > 0 && reaches(d - 1, L, seqIdThr)) d--;
    while (!reaches(d, L, seqIdThr)) d++;   // (ends at L at the latest)
    return d;
}

int sd_host_clusthash_format(uint64_t nSeq, const uint32_t *keys, const uint64_t *offsets, const uint32_t *foundBy,
                             const uint32_t *identical, uint64_t *entryOff, uint64_t textCap, char *text, uint64_t *textBytes) {
    if (!textBytes || !offsets || (nSeq && (!keys || !foundBy || !identical))) return SD_EINVAL;
    if (text && !entryOff) return SD_EINVAL;
    // the rows of every entry: a stable counting sort of the found sequences by the one that found them
    std::vector<uint64_t> first(nSeq + 1, 0);
    for (uint64_t t = 0; t < nSeq; t++) {
        if (foundBy[t] == UINT32_MAX) continue;
        if (foundBy[t] >= nSeq) return SD_EINVAL;
        first[foundBy[t] + 1]++;
    }
    for (uint64_t s = 0; s < nSeq; s++) first[s + 1] += first[s];
    std::vector<uint32_t> rows(first[nSeq] ? first[nSeq] : 1);
    {
        std::vector<uint64_t> at(first.begin(), first.end() - 1);
        for (uint64_t t = 0; t < nSeq; t++)
            if (foundBy[t] != UINT32_MAX) rows[at[foundBy[t]]++] = (uint32_t) t;
    }
    uint64_t bytes = 0;
    char line[128];   // a row is at most 10 + 5 + 5 + 5 + 4 * 11 + 3 bytes
    for (uint64_t s = 0; s < nSeq; s++) {
        const uint32_t L = (uint32_t) (offsets[s + 1] - offsets[s]);
        if (text) entryOff[s] = bytes;
        for (uint64_t r = first[s]; r <= first[s + 1]; r++) {
            char *p = line;
            if (r == first[s]) {   // the self row
                p = sd::u32toa(keys[s], p);
                memcpy(p, "\t255\t1.00", 9);
                p += 9;
            } else {
                const uint32_t t = rows[r - 1];
                p = sd::u32toa(keys[t], p);
                memcpy(p, "\t255\t", 5);
                p += 5;
                // Util::fastSeqIdToBuffer's text up to its terminator, which clusthash appends as a C string: "1.000" for one (the
                // callers that overwrite the byte before the returned pointer print "1.00": sd::seqIdToBuffer)
                const float seqId = (static_cast<float>(identical[t])) / static_cast<float>(L);
                if (seqId == 1.0) {
                    memcpy(p, "1.000", 5);
                    p += 5;
                } else {
                    p = sd::seqIdToBuffer(seqId, p);
                }
            }
            p = tail(L, p);
            const uint64_t len = (uint64_t) (p - line);
            if (text) {
                if (bytes + len > textCap) return SD_ENOMEM;
                memcpy(text + bytes, line, (size_t) len);
            }
            bytes += len;
        }
    }
    if (text) entryOff[nSeq] = bytes;
    *textBytes = bytes;
    return SD_OK;
}

}  // extern "C"
