// Host stages of `kmermatcher` (M/src/linclust/kmermatcher.cpp): the reduced alphabet, the -k 0 rule and the text of
// the prefilter DB.  The records and their grouping are csrc/hip/sd_kmermatch.hip.
#include "sd_host.h"
#include "spacedust_gpu.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

typedef std::vector<std::vector<double> > Mat;

// BaseMatrix::generateSubMatrix(probMatrix, subMatrix, ..., size, false) (BaseMatrix.cpp:110-131) followed by
// ReducedMatrix::calculateMutualInformation (ReducedMatrix.cpp:160-169): sum p_ij log2(p_ij / (pBack_i pBack_j)), pBack = row sums
double mutualInformation(const Mat &p, int size) {
    std::vector<double> pBack(size);
    for (int i = 0; i < size; i++) {
        pBack[i] = 0;
        for (int j = 0; j < size; j++) pBack[i] += p[i][j];
    }
    double info = 0;
    for (int i = 0; i < size; i++)
        for (int j = 0; j < size; j++) info += p[i][j] * std::log2(p[i][j] / (pBack[i] * pBack[j]));
    return info;
}

// ReducedMatrix::coupleBases (ReducedMatrix.cpp:171-284): column b2 added to column b1, the columns behind b2 move one to the left and the
// last one is zero; then the same for the rows
void coupleBases(const Mat &in, Mat &out, int size, int b1, int b2) {
    Mat tmp(size, std::vector<double>(size, 0.0));
    for (int i = 0; i < size; i++) {
        for (int j = 0; j < b2; j++) tmp[i][j] = in[i][j];
        tmp[i][b1] = in[i][b1] + in[i][b2];
        for (int j = b2; j < size - 1; j++) tmp[i][j] = in[i][j + 1];
        tmp[i][size - 1] = 0.0;
    }
    for (int i = 0; i < b2; i++)
        for (int j = 0; j < size; j++) out[i][j] = tmp[i][j];
    for (int j = 0; j < size; j++) out[b1][j] = tmp[b1][j] + tmp[b2][j];
    for (int i = b2; i < size - 1; i++)
        for (int j = 0; j < size; j++) out[i][j] = tmp[i + 1][j];
    for (int j = 0; j < size; j++) out[size - 1][j] = 0.0;
}

}  // namespace

extern "C" {

int sd_host_reduced_alphabet(int which, int alphabetSize, uint8_t *letterMap, int *reducedSize) {
    if (!letterMap || (which != 0 && which != 1)) return SD_EINVAL;
    if (alphabetSize == sd::ALPH) {
        for (int a = 0; a < sd::ALPH; a++) letterMap[a] = (uint8_t) a;
        if (reducedSize) *reducedSize = sd::ALPH;
        return SD_OK;
    }
    if (alphabetSize < 2 || alphabetSize > sd::ALPH) return SD_EINVAL;
    // kmermatcherInner builds it over SubstitutionMatrix(..., 8.0, -0.2f); only the joint probabilities enter the merging
    sd::SubMat m;
    sd::initSubMat(m, which == 0 ? sd::MAT_BLOSUM62 : sd::MAT_VTML80, 8.0f, -0.2f);
    const int full = sd::ALPH - 1;   // the merging never touches X
    Mat prob(full, std::vector<double>(full)), next(full, std::vector<double>(full, 0.0)), trial(full, std::vector<double>(full, 0.0));
    for (int i = 0; i < full; i++)
        for (int j = 0; j < full; j++) prob[i][j] = m.probMatrix[i][j];
    // alphabet[x] = the letter code that stands for reduced class x; groupOf[letter] = that representative
    std::vector<int> alphabet(sd::ALPH), groupOf(sd::ALPH);
    for (int a = 0; a < sd::ALPH; a++) alphabet[a] = groupOf[a] = a;
    const int steps = sd::ALPH - alphabetSize;
    for (int step = 0; step < steps; step++) {
        const int size = full - step;
        // coupleWithBestInfo (ReducedMatrix.cpp:198-239): the pair whose merging keeps the most mutual information, first one on a tie
        double bestInfo = 0;
        int bestI = 0, bestJ = 0;
        for (int i = 0; i < size; i++)
            for (int j = i + 1; j < size; j++) {
                coupleBases(prob, trial, size, i, j);
                const double info = mutualInformation(trial, size - 1);
                if (info > bestInfo) {
                    bestInfo = info;
                    bestI = i;
                    bestJ = j;
                }
            }
        for (int i = 0; i < full; i++) std::fill(next[i].begin(), next[i].end(), 0.0);
        coupleBases(prob, next, size, bestI, bestJ);
        const int kept = alphabet[bestI], lost = alphabet[bestJ];
        alphabet.erase(alphabet.begin() + bestJ);
        for (int a = 0; a < sd::ALPH; a++)
            if (groupOf[a] == lost) groupOf[a] = kept;
        prob = next;
    }
    for (int a = 0; a < sd::ALPH; a++) {
        int code = -1;
        for (size_t x = 0; x < alphabet.size(); x++)
            if (alphabet[x] == groupOf[a]) code = (int) x;
        if (code < 0) return SD_EINVAL;
        letterMap[a] = (uint8_t) code;
    }
    if (reducedSize) *reducedSize = (int) alphabet.size();
    return SD_OK;
}

int sd_host_kmermatch_auto_k(float seqIdThr, uint64_t residues, int *kmerSize, int *alphabetSize) {
    if (!kmerSize || !alphabetSize) return SD_EINVAL;
    if ((seqIdThr + 0.001) >= 0.99) {
        *kmerSize = 14;
        *alphabetSize = 21;
    } else if ((seqIdThr + 0.001) >= 0.9) {
        *kmerSize = 14;
        *alphabetSize = 13;
    } else {
        *kmerSize = std::max(10, static_cast<int>(log(static_cast<float>(residues)) / log(8.7)));
        *alphabetSize = 13;
    }
    return SD_OK;
}

uint64_t sd_host_kmermatch_considered(int kmersPerSequence, float kmersPerSequenceScale, uint32_t seqLen) {
    // kmermatcher.cpp:206, `kmersPerSequence - 1 + (scale * seq.L)` in float.  The product is rounded to float before the sum (the
    // volatile keeps every compiler from contracting the two into one fused operation): a build of the reference that fuses them can
    // differ by one window where scale * L + kmersPerSequence - 1 lies within a rounding of an integer
    volatile float product = kmersPerSequenceScale * (float) (int) seqLen;
    const float want = (float) (kmersPerSequence - 1) + product;
    return want > 0.0f ? (uint64_t) want : 0;
}

int sd_host_kmermatch_format(uint64_t nSeq, const uint32_t *keys, uint64_t nHits, const uint32_t *rep, const uint32_t *member,
                             const uint32_t *score, const int32_t *diag, uint32_t *entryKey, uint64_t *entryOff, uint64_t textCap, char *text,
                             uint64_t *textBytes) {
    if ((nSeq && !keys) || (nHits && (!rep || !member || !score || !diag)) || !textBytes) return SD_EINVAL;
    std::vector<uint32_t> sorted(keys, keys + nSeq);
    std::sort(sorted.begin(), sorted.end());
    // first pass: sizes; second pass: text.  A line is at most 10 + 1 + 11 + 1 + 6 + 1 = 30 bytes
    uint64_t bytes = 0, h = 0;
    char line[48];
    const bool write = text != nullptr;
    if (write && (!entryKey || !entryOff)) return SD_EINVAL;
    for (uint64_t e = 0; e < nSeq; e++) {
        const uint32_t key = sorted[e];
        if (h < nHits && rep[h] < key) return SD_EINVAL;   // (a representative that is no sequence of the DB)
        if (write) {
            entryKey[e] = key;
            entryOff[e] = bytes;
        }
        int len = snprintf(line, sizeof(line), "%u\t0\t0\n", key);
        if (write) {
            if (bytes + (uint64_t) len > textCap) return SD_ENOMEM;
            memcpy(text + bytes, line, (size_t) len);
        }
        bytes += (uint64_t) len;
        for (; h < nHits && rep[h] == key; h++) {
            // hit_t::diagonal is an unsigned short that prefilterHitToBuffer prints as a short (QueryMatcher.h:118-130)
            len = snprintf(line, sizeof(line), "%u\t%d\t%d\n", member[h], (int) score[h], (int) (int16_t) (uint16_t) diag[h]);
            if (write) {
                if (bytes + (uint64_t) len > textCap) return SD_ENOMEM;
                memcpy(text + bytes, line, (size_t) len);
            }
            bytes += (uint64_t) len;
        }
    }
    if (h != nHits) return SD_EINVAL;
    if (write) entryOff[nSeq] = bytes;
    *textBytes = bytes;
    return SD_OK;
}

}  // extern "C"
