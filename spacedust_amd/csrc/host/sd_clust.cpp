// Host half of the `clust` module (M/src/clustering/{Clustering,ClusteringAlgorithms,AlignmentSymmetry}.cpp): the local order of the
// sequences, the result DB's lines as rows of local ids with a 16-bit score, the three clustering algorithms and the cluster DB's text.
// The symmetric graph between the parser and the set-cover / connected-component algorithms is sd_clust_symmetrize (csrc/hip/sd_clust.hip).
// The algorithms are sequential and order-dependent by definition: they are restated here statement by statement, the bucket array of the
// set cover and its swap order included, because the representatives depend on them.
#include "spacedust_gpu.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <utility>
#include <vector>

namespace {

constexpr int DBTYPE_ALIGNMENT_RES = 5, DBTYPE_CLUSTER_RES = 6, DBTYPE_PREFILTER_RES = 7, DBTYPE_PREFILTER_REV_RES = 14;

inline bool isBlank(char c) { return c == ' ' || c == '\t'; }
inline bool endsWord(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\0'; }

// Util::parseByColumnNumber: the word behind `column` runs of (word, blanks)
inline void columnWord(const char *line, int column, char *out, size_t cap) {
    const char *p = line;
    for (int i = 0; i < column; i++) {
        while (!endsWord(*p)) p++;
        while (isBlank(*p)) p++;
    }
    size_t len = 0;
    while (!endsWord(p[len]) && len + 1 < cap) len++;
    memcpy(out, p, len);
    out[len] = '\0';
}

// id of a key in keys sorted with their local ids (DBReader::getId: UINT_MAX when the key is absent)
struct KeyMap {
    std::vector<std::pair<uint32_t, uint32_t> > byKey;   // (key, local id)
    KeyMap(uint32_t n, const uint32_t *localKeys) : byKey(n) {
        for (uint32_t i = 0; i < n; i++) byKey[i] = std::make_pair(localKeys[i], i);
        std::sort(byKey.begin(), byKey.end());
    }
    uint32_t idOf(uint32_t key) const {
        std::vector<std::pair<uint32_t, uint32_t> >::const_iterator it = std::lower_bound(byKey.begin(), byKey.end(), std::make_pair(key, 0u));
        return (it == byKey.end() || it->first != key) ? UINT32_MAX : it->second;
    }
};

// the score of an entry without lines (AlignmentSymmetry.cpp:45-63)
inline uint16_t emptyScore(int base, int similarityType) {
    if (base == DBTYPE_ALIGNMENT_RES) return similarityType == 1 ? (uint16_t) USHRT_MAX : (uint16_t) (1.0 * 1000.0f);
    return (uint16_t) USHRT_MAX;
}

// the score of a line (AlignmentSymmetry.cpp:80-106)
inline uint16_t lineScore(const char *line, int base, int similarityType) {
    char word[256];
    if (base == DBTYPE_ALIGNMENT_RES) {
        if (similarityType == 1) {
            columnWord(line, 1, word, sizeof(word));
            return (unsigned short) (atof(word));
        }
        columnWord(line, 2, word, sizeof(word));
        return (unsigned short) (atof(word) * 1000.0f);
    }
    if (base == DBTYPE_PREFILTER_RES || base == DBTYPE_PREFILTER_REV_RES) {
        columnWord(line, 1, word, sizeof(word));
        short sim = (short) atoi(word);
        return (unsigned short) (sim > 0 ? sim : -sim);
    }
    return (unsigned short) USHRT_MAX;
}

// ClusteringAlgorithms::initClustersizes / removeClustersize / decreaseClustersize: the nodes bucketed by the size of their set
struct SizeBuckets {
    std::vector<int> clustersizes;
    std::vector<unsigned int> sorted, position, borders;
    SizeBuckets(uint32_t n, const uint64_t *rowOff) : clustersizes(n), sorted((size_t) n + 1, 0), position((size_t) n + 1, 0) {
        unsigned int maxClustersize = 0;
        for (uint32_t i = 0; i < n; i++) {
            const size_t elementCount = (size_t) (rowOff[i + 1] - rowOff[i]);
            maxClustersize = std::max((unsigned int) elementCount, maxClustersize);
            clustersizes[i] = (int) elementCount;
        }
        std::vector<unsigned int> abundance((size_t) maxClustersize + 1, 0);
        for (uint32_t i = 0; i < n; i++) abundance[clustersizes[i]]++;
        borders.assign((size_t) maxClustersize + 1, 0);
        for (unsigned int i = 1; i < maxClustersize + 1; i++) borders[i] = borders[i - 1] + abundance[i - 1];
        std::fill(abundance.begin(), abundance.end(), 0);
        for (uint32_t i = 0; i < n; i++) {
            const unsigned int at = borders[clustersizes[i]] + abundance[clustersizes[i]];
            sorted[at] = i;
            position[i] = at;
            abundance[clustersizes[i]]++;
        }
    }
    void remove(unsigned int id) {
        clustersizes[id] = 0;
        sorted[position[id]] = UINT_MAX;
        position[id] = UINT_MAX;
    }
    void decrease(unsigned int id) {
        const unsigned int oldposition = position[id];
        const unsigned int newposition = borders[clustersizes[id]];
        const unsigned int swapid = sorted[newposition];
        if (swapid != UINT_MAX) position[swapid] = oldposition;
        sorted[oldposition] = swapid;
        sorted[newposition] = id;
        position[id] = newposition;
        borders[clustersizes[id]]++;
        clustersizes[id]--;
    }
};

// Itoa::u32toa_sse2 + '\n' without its terminator
inline uint64_t putKeyLine(char *out, unsigned int key) {
    char digits[10];
    int len = 0;
    do {
        digits[len++] = (char) ('0' + key % 10);
        key /= 10;
    } while (key);
    for (int i = 0; i < len; i++) out[i] = digits[len - 1 - i];
    out[len] = '\n';
    return (uint64_t) len + 1;
}

inline bool badGraph(uint64_t n, const uint64_t *rowOff, const uint32_t *elem) {
    if (n > (uint64_t) UINT32_MAX - 1 || !rowOff || rowOff[0] != 0) return true;
    for (uint64_t i = 0; i < n; i++)
        if (rowOff[i + 1] < rowOff[i]) return true;
    if (rowOff[n] && !elem) return true;
    for (uint64_t e = 0; e < rowOff[n]; e++)
        if (elem[e] >= n) return true;
    return false;
}

}  // namespace

extern "C" {

// DBReader::open(SORT_BY_LENGTH) (M/src/commons/DBReader.cpp:325-342): index length descending, then id ascending
int sd_host_clust_order(uint64_t n, const uint64_t *indexLength, uint32_t *localToId) {
    if (n > (uint64_t) UINT32_MAX - 1 || (n && (!indexLength || !localToId))) return SD_EINVAL;
    for (uint64_t i = 0; i < n; i++) localToId[i] = (uint32_t) i;
    std::stable_sort(localToId, localToId + n, [&](uint32_t a, uint32_t b) { return (unsigned int) indexLength[a] > (unsigned int) indexLength[b]; });
    return SD_OK;
}

int sd_host_clust_parse(uint64_t n, const uint32_t *localKeys, const char *const *entries, int dbtype, int similarityType, uint64_t *rowOff,
                        uint64_t cap, uint32_t *elem, uint16_t *score, uint32_t *badKey) {
    if (n > (uint64_t) UINT32_MAX - 1 || !rowOff || (n && (!localKeys || !entries))) return SD_EINVAL;
    if (similarityType != 1 && similarityType != 2) return SD_EINVAL;
    const int base = dbtype & 0xFFFF;
    if (base != DBTYPE_ALIGNMENT_RES && base != DBTYPE_PREFILTER_RES && base != DBTYPE_PREFILTER_REV_RES && base != DBTYPE_CLUSTER_RES)
        return SD_EUNSUPPORTED;   // "Alignment format is not supported!"
    rowOff[0] = 0;
    for (uint64_t i = 0; i < n; i++)
        if (!entries[i]) return SD_EINVAL;
#pragma omp parallel for schedule(dynamic, 1000)
    for (uint64_t i = 0; i < n; i++) {
        const char *data = entries[i];
        uint64_t lines = 0;
        for (const char *p = data; (p = strchr(p, '\n')) != NULL; p++) lines++;
        rowOff[i + 1] = *data == '\0' ? 1 : lines;
    }
    for (uint64_t i = 0; i < n; i++) rowOff[i + 1] += rowOff[i];
    if (!elem && !score && cap == 0) return SD_OK;   // the count-only form
    if (rowOff[n] > cap) return SD_ENOMEM;
    if (rowOff[n] && (!elem || !score)) return SD_EINVAL;
    const KeyMap map((uint32_t) n, localKeys);
    uint64_t firstBad = UINT64_MAX;
#pragma omp parallel for schedule(dynamic, 100)
    for (uint64_t i = 0; i < n; i++) {
        const char *data = entries[i];
        uint64_t at = rowOff[i];
        if (*data == '\0') {
            elem[at] = (uint32_t) i;
            score[at] = emptyScore(base, similarityType);
            continue;
        }
        while (*data != '\0' && at < rowOff[i + 1]) {
            const uint32_t key = (uint32_t) strtoul(data, NULL, 10);
            const uint32_t id = map.idOf(key);
            if (id == UINT32_MAX) {
#pragma omp critical
                if (i < firstBad) {
                    firstBad = i;
                    if (badKey) *badKey = key;
                }
                elem[at] = 0;
            } else {
                elem[at] = id;
            }
            score[at] = lineScore(data, base, similarityType);
            at++;
            while (*data != '\n' && *data != '\0') data++;
            if (*data == '\n') data++;
        }
        for (; at < rowOff[i + 1]; at++) {   // (a last line without its line feed)
            elem[at] = (uint32_t) i;
            score[at] = 0;
        }
    }
    return firstBad == UINT64_MAX ? SD_OK : SD_EINVAL;
}

// ClusteringAlgorithms::setCover (ClusteringAlgorithms.cpp:213-278) over the symmetric graph; the score is read as a signed short (:228)
int sd_host_clust_setcover(uint64_t n, const uint64_t *rowOff, const uint32_t *elem, const uint16_t *score, uint32_t *assigned) {
    if (badGraph(n, rowOff, elem) || (rowOff[n] && !score) || (n && !assigned)) return SD_EINVAL;
    const uint32_t dbSize = (uint32_t) n;
    std::fill(assigned, assigned + n, UINT_MAX);
    std::vector<short> bestscore(n, SHRT_MIN);
    SizeBuckets b(dbSize, rowOff);
    for (int64_t cl_size = (int64_t) dbSize - 1; cl_size >= 0; cl_size--) {
        const unsigned int representative = b.sorted[cl_size];
        if (representative == UINT_MAX) continue;
        b.remove(representative);
        assigned[representative] = representative;
        const uint32_t *row = elem + rowOff[representative];
        const uint16_t *rowScore = score + rowOff[representative];
        const size_t elementSize = (size_t) (rowOff[representative + 1] - rowOff[representative]);
        for (size_t elementId = 0; elementId < elementSize; elementId++) {
            const unsigned int elementtodelete = row[elementId];
            const short seqId = (short) rowScore[elementId];
            if (seqId > bestscore[elementtodelete]) {
                assigned[elementtodelete] = representative;
                bestscore[elementtodelete] = seqId;
            }
            if (elementtodelete == representative) continue;
            if (b.clustersizes[elementtodelete] < 1) continue;
            b.remove(elementtodelete);
        }
        for (size_t elementId = 0; elementId < elementSize; elementId++) {
            const unsigned int elementtodelete = row[elementId];
            const unsigned int currElementSize = (unsigned int) (rowOff[elementtodelete + 1] - rowOff[elementtodelete]);
            if (elementtodelete == representative) {
                b.clustersizes[elementtodelete] = -1;
                continue;
            }
            if (b.clustersizes[elementtodelete] < 0) continue;
            b.clustersizes[elementtodelete] = -1;
            const uint32_t *other = elem + rowOff[elementtodelete];
            for (size_t elementId2 = 0; elementId2 < currElementSize; elementId2++) {
                const unsigned int elementtodecrease = other[elementId2];
                if (b.clustersizes[elementtodecrease] == 1) {
                    // ("there must be an error": the reference reports it and goes on)
                } else if (b.clustersizes[elementtodecrease] > 0) {
                    b.decrease(elementtodecrease);
                }
            }
        }
    }
    return SD_OK;
}

// the breadth-first walk of ClusteringAlgorithms::execute(3) (ClusteringAlgorithms.cpp:90-120), largest sets first
int sd_host_clust_connected(uint64_t n, const uint64_t *rowOff, const uint32_t *elem, int maxIterations, uint32_t *assigned) {
    if (badGraph(n, rowOff, elem) || (n && !assigned)) return SD_EINVAL;
    const uint32_t dbSize = (uint32_t) n;
    std::fill(assigned, assigned + n, UINT_MAX);
    SizeBuckets b(dbSize, rowOff);
    for (int64_t cl_size = (int64_t) dbSize - 1; cl_size >= 0; cl_size--) {
        const unsigned int representative = b.sorted[cl_size];
        if (assigned[representative] != UINT_MAX) continue;
        assigned[representative] = representative;
        std::queue<unsigned int> myqueue;
        std::queue<int> iterationcutoffs;
        myqueue.push(representative);
        iterationcutoffs.push(0);
        while (!myqueue.empty()) {
            const unsigned int currentid = myqueue.front();
            const int iterationcutoff = iterationcutoffs.front();
            assigned[currentid] = representative;
            myqueue.pop();
            iterationcutoffs.pop();
            for (uint64_t e = rowOff[currentid]; e < rowOff[currentid + 1]; e++) {
                const unsigned int elementtodelete = elem[e];
                if (assigned[elementtodelete] == UINT_MAX && iterationcutoff < maxIterations) {
                    myqueue.push(elementtodelete);
                    iterationcutoffs.push(iterationcutoff + 1);
                }
                assigned[elementtodelete] = representative;
            }
        }
    }
    return SD_OK;
}

// ClusteringAlgorithms::greedyIncrementalLowMem (ClusteringAlgorithms.cpp:280-366) over the parsed rows as they are (no symmetric graph): an
// entry of one line or none founds nothing, and an entry that does not list itself can found a cluster and still be a member elsewhere
int sd_host_clust_greedy(uint64_t n, const uint64_t *rowOff, const uint32_t *elem, uint32_t *assigned) {
    if (badGraph(n, rowOff, elem) || (n && !assigned)) return SD_EINVAL;
    std::fill(assigned, assigned + n, UINT_MAX);
    for (uint64_t i = 0; i < n; i++) {
        if (assigned[i] != UINT_MAX) continue;
        if (rowOff[i + 1] - rowOff[i] <= 1) continue;
        for (uint64_t e = rowOff[i]; e < rowOff[i + 1]; e++)
            if (assigned[elem[e]] == UINT_MAX) assigned[elem[e]] = (uint32_t) i;
    }
    for (uint64_t i = 0; i < n; i++)
        if (assigned[i] == UINT_MAX) assigned[i] = (uint32_t) i;
    return SD_OK;
}

// The tail of ClusteringAlgorithms::execute and Clustering::writeData (Clustering.cpp:237-266): the pairs (representative key, member key)
// sorted, one entry per representative: its own key, then the other members ascending.  A node without a cluster keeps the pair (0, 0) the
// reference's array was created with.  text holds at most 22 bytes per node (a representative that is a member elsewhere prints a line of its own).
int sd_host_clust_format(uint64_t n, const uint32_t *localKeys, const uint32_t *assigned, uint32_t *repKey, uint32_t *memberKey,
                         uint64_t *nEntries, uint32_t *entryKey, uint64_t *entryOff, char *text) {
    if (n > (uint64_t) UINT32_MAX - 1 || (n && (!localKeys || !assigned || !repKey || !memberKey))) return SD_EINVAL;
    std::vector<std::pair<unsigned int, unsigned int> > assignment(n);
    for (uint64_t i = 0; i < n; i++) {
        if (assigned[i] == UINT_MAX) continue;
        if (assigned[i] >= n) return SD_EINVAL;
        assignment[i] = std::make_pair(localKeys[assigned[i]], localKeys[i]);
    }
    std::sort(assignment.begin(), assignment.end());
    for (uint64_t i = 0; i < n; i++) {
        repKey[i] = assignment[i].first;
        memberKey[i] = assignment[i].second;
    }
    if (!nEntries) return SD_OK;
    if (!entryKey || !entryOff || (n && !text)) return SD_EINVAL;
    uint64_t entries = 0, at = 0;
    unsigned int prev = UINT_MAX;
    entryOff[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        const unsigned int cur = assignment[i].first;
        if (prev != cur) {
            if (prev != UINT_MAX) entryOff[++entries] = at;
            entryKey[entries] = cur;
            at += putKeyLine(text + at, cur);
        }
        if (assignment[i].second != cur) at += putKeyLine(text + at, assignment[i].second);
        prev = cur;
    }
    if (prev != UINT_MAX) entryOff[++entries] = at;
    *nEntries = entries;
    return SD_OK;
}

}  // extern "C"
