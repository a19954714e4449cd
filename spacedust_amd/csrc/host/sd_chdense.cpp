// clusterhits of one (query set, target set) entry by the reference's dense K x K loop, literally
// (R/src/util/ClusterHits.cpp:137-182,363-485).
//
// The device kernel (csrc/hip/sd_clusterhits.hip) keeps every node as a list sorted by query position and derives the
// conserved-pair count of a union from that order.  That is the reference's count only while the order is unique: where two
// hits of an entry share a query position, the reference's findConservedPairs hands the union to std::sort with operator<
// on qPos alone (:104-106), and which of two equal positions comes first is then a property of libstdc++'s introsort and of
// the order the hits arrive in -- node i1's members in the order they were merged, then node j's (groupNodes, :168-176).
// So such entries take this path: the same containers in the same order through the same std::sort (whose moves depend on
// the comparisons alone, not on the element type), the dense matrix, the merge-then-test do/while, the `j != 0` reset and
// the stale dmin.  The emitted members are written in the order the reference prints them, which sd_clusterhits_batch's
// shared emission (it sorts from index order) could not reproduce.  O(K^2) doubles and O(K * |node|) per score: meant for
// the rare entry, not for throughput.  The arithmetic is sd_chpval.cpp's.
#include "sd_host.h"

#include <algorithm>
#include <climits>

namespace sd {

namespace {

struct Box {
    unsigned int iMax = 0, iMin = INT_MAX, jMax = 0, jMin = INT_MAX;   // the reference's start values (:89-92,138-141)
    void add(const ClusterHit &h) {
        iMax = std::max(iMax, h.qPos); iMin = std::min(iMin, h.qPos);
        jMax = std::max(jMax, h.tPos); jMin = std::min(jMin, h.tPos);
    }
};

// clusterMatchScore (:120-134): sorts c by query position in place, as findConservedPairs does.  k hits over fewer than
// k - 1 genes (hits that share both positions) make the reference read lookup[span - k + 1] in front of its table: there is
// no result to reproduce, *outside is set and the entry fails
double matchScore(const double *lg, std::vector<ClusterHit> &c, bool asPval, bool *outside) {
    if (c.empty()) return 0.0;
    Box b;
    for (const ClusterHit &h : c) b.add(h);
    const int spanI = (int) (b.iMax - b.iMin + 1), spanJ = (int) (b.jMax - b.jMin + 1);
    const int span = spanI > spanJ ? spanI : spanJ;
    if (span - (int) c.size() + 1 < 0) {
        *outside = true;
        return 0.0;
    }
    std::sort(c.begin(), c.end(), [](const ClusterHit &x, const ClusterHit &y) { return x.qPos < y.qPos; });
    int m = 0;
    for (size_t l = 0; l + 1 < c.size(); l++) {
        const bool sameOrder = c[l + 1].tPos > c[l].tPos;
        if (((c[l].qS == c[l].tS) == sameOrder) && ((c[l + 1].qS == c[l + 1].tS) == sameOrder)) m++;
    }
    return asPval ? chClusterPvalOfShape(lg, (int) c.size(), span, m) : chMatchScoreOfShape(lg, (int) c.size(), span, m);
}

// groupNodes (:163-182) + clusterMatchScore: node i's members, then node j's, if their boxes are compatible (:137-160,
// unsigned gap arithmetic)
double groupScore(const double *lg, const std::vector<std::vector<uint32_t> > &nodes, const std::vector<ClusterHit> &match,
                  size_t i, size_t j, unsigned int d, std::vector<ClusterHit> &c, bool *outside) {
    c.clear();
    if (nodes[i].empty() || nodes[j].empty()) return 0.0;
    Box a, b;
    for (uint32_t h : nodes[i]) a.add(match[h]);
    for (uint32_t h : nodes[j]) b.add(match[h]);
    if (!(std::min(a.jMin - b.jMax, b.jMin - a.jMax) <= d && std::min(a.iMin - b.iMax, b.iMin - a.iMax) <= d)) return 0.0;
    for (uint32_t h : nodes[i]) c.push_back(match[h]);
    for (uint32_t h : nodes[j]) c.push_back(match[h]);
    return matchScore(lg, c, false, outside);
}

}  // namespace

uint32_t chDenseEntry(const double *lg, uint32_t K, const uint32_t *qPos, const uint32_t *tPos, const uint8_t *strands,
                      const double *pval, int Nq, uint32_t d, uint32_t cls, double alpha, float pCluThr, float pMHThr,
                      uint32_t *clusterOf, uint32_t *rank, double *pCO, double *pMH, uint32_t *size) {
    for (uint32_t h = 0; h < K; h++) {
        clusterOf[h] = UINT32_MAX;
        rank[h] = 0;
    }
    if (K <= 1) return 0;   // :359-361
    std::vector<ClusterHit> match(K), c;
    bool outside = false;
    for (uint32_t h = 0; h < K; h++) {
        match[h].pval = pval[h]; match[h].qPos = qPos[h]; match[h].tPos = tPos[h];
        match[h].qS = strands[h] & 1; match[h].tS = (strands[h] >> 1) & 1; match[h].idx = h;
    }
    std::vector<double> D((size_t) K * K, 0.0);
    std::vector<uint32_t> dmin(K, 0);
    std::vector<std::vector<uint32_t> > nodes(K);
    for (uint32_t n = 0; n < K; n++) nodes[n].push_back(n);
    auto at = [&](size_t i, size_t j) -> double & { return D[i * K + j]; };
    for (size_t i = 0; i < K; i++)
        for (size_t j = 0; j < K; j++) {
            at(i, j) = i == j ? 0.0 : groupScore(lg, nodes, match, i, j, d, c, &outside);
            if (at(i, j) > at(i, dmin[i])) dmin[i] = (uint32_t) j;
        }
    const double sMin = chMatchScoreOfShape(lg, 2, (int) d + 1, 1);
    double maxScore;
    do {
        size_t i1 = 0;
        for (size_t i = 0; i < K; i++)
            if (at(i, dmin[i]) > at(i1, dmin[i1])) i1 = i;
        const size_t i2 = dmin[i1];
        maxScore = at(i1, i2);
        if (maxScore == 0) break;
        nodes[i1].insert(nodes[i1].end(), nodes[i2].begin(), nodes[i2].end());   // merged first, tested after (:395,453)
        nodes[i2].clear();
        for (size_t j = 0; j < K; j++) {
            if (i1 == j || i2 == j) {
                at(i1, j) = 0.0;
                at(j, i1) = 0.0;
            } else {
                at(i1, j) = groupScore(lg, nodes, match, i1, j, d, c, &outside);
                at(j, i1) = at(i1, j);
            }
            at(i2, j) = 0.0;
            at(j, i2) = 0.0;
            if (j != 0) {
                if (at(i1, j) > at(i1, dmin[i1])) dmin[i1] = (uint32_t) j;
            } else {
                dmin[i1] = 0;   // the `j != 0` reset (:439-444)
            }
            if (j != i1 && j != i2 && at(j, i1) > at(j, dmin[j])) dmin[j] = (uint32_t) i1;   // other rows keep a stale dmin
        }
    } while (maxScore >= sMin && !outside);
    if (outside) return UINT32_MAX;
    uint32_t nClu = 0;
    for (size_t n = 0; n < K; n++) {
        if (nodes[n].size() < cls || nodes[n].empty()) continue;
        c.clear();
        for (uint32_t h : nodes[n]) c.push_back(match[h]);
        const double co = matchScore(lg, c, true, &outside);   // leaves c in the printed order (:462,475-477)
        const double mh = chMultihitPval(lg, c, Nq, alpha);
        if (co <= pCluThr && mh <= pMHThr) {
            pCO[nClu] = co;
            pMH[nClu] = mh;
            size[nClu] = (uint32_t) c.size();
            for (size_t r = 0; r < c.size(); r++) {
                clusterOf[c[r].idx] = nClu;
                rank[c[r].idx] = (uint32_t) r;
            }
            nClu++;
        }
    }
    return outside ? UINT32_MAX : nClu;
}

}  // namespace sd
