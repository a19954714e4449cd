"""A plain restatement of clusterhits_kernel's incremental algorithm (csrc/hip/sd_clusterhits.hip), for the CPU: nodes as
lists in query order with bounding boxes, cached conserved-pair counts, the seam shortcut of chPairScore, the end-to-end
joins of the merge and the literal replay of the stale-dmin rules -- not the reference's dense K x K loop, whose compiled
form supplies the expected rows (tests/golden/ch_classes.npz).  Every branch counts how often it is taken, so that the
constructed cases of chgen.class_entries can be shown to reach it (tests/test_ch_classes.py):

    score_append / score_prepend      chPairScore: a's members all before b's / all behind
    score_interleaved                 neither: the kernel has no such branch any more (its invariant), this must stay 0
    merge_append / merge_prepend / merge_interleaved      the same three for the merge
    stale_absorbed                    a live row whose dmin pointed at the absorbed node i2 (its cached score becomes 0)
    stale_absorbing, .._fell          ... at the absorbing node i1 (its cached score becomes the new one / a smaller one)
    stale_third                       ... at a third node with a score above 0 (kept, although it may no longer be the maximum)
    takeover                          the new score D[j][i1] beats what the row holds: dmin[j] = i1
    stop_zero / stop_smin             the loop ends on score 0 / after a merge whose score was below sMin
    tied_argmax                       the selected score is held by more than one row (the first index has to win)
    init_tie                          a row's first arg-max at init had an equal score behind it (`>` keeps the first)

`mutant` switches one rule to a wrong form; the mutants are the ones DESIGN lists for the kernel."""
import math

import numpy as np

NIL = -1
M32 = 0xFFFFFFFF
BRANCHES = ('score_append', 'score_prepend', 'score_interleaved', 'merge_append', 'merge_prepend', 'merge_interleaved',
            'stale_absorbed', 'stale_absorbing', 'stale_absorbing_fell', 'stale_third', 'takeover', 'stop_zero', 'stop_smin',
            'tied_argmax', 'init_tie')
MUTANTS = ('argmax_block', 'argmax_stride', 'keep_absorbed', 'init_ge', 'no_seam', 'box_d1')


def new_counts():
    return dict.fromkeys(BRANCHES, 0)


class _Entry:
    def __init__(self, q, t, s, d, lg, counts, mutant):
        self.q = [int(x) for x in q]
        self.t = [int(x) for x in t]
        self.eq = [((int(x) & 1) != 0) == ((int(x) & 2) != 0) for x in s]
        self.d, self.lg, self.c, self.mutant = int(d), lg, counts, mutant
        self.box_d = self.d + 1 if mutant == 'box_d1' else self.d
        K = self.K = len(self.q)
        order = sorted(range(K), key=lambda h: (self.q[h], h))   # rank by (qPos, index)
        self.rank = [0] * K
        for r, h in enumerate(order):
            self.rank[h] = r
        self.next = [NIL] * K
        self.head = list(range(K))
        self.tail = list(range(K))
        self.mcnt = [0] * K
        self.size = np.ones(K, np.int64)
        self.iMin = np.array(self.q, np.int64)
        self.iMax = self.iMin.copy()
        self.jMin = np.array(self.t, np.int64)
        self.jMax = self.jMin.copy()
        self.logq0, self.ln2 = math.log(0.001), math.log(2.0)

    def score_ksm(self, k, span, m):
        lg = self.lg
        logp_clu = 2 * lg[span + 1] - 2 * lg[span - k + 1] - lg[k + 1] + k * self.logq0
        logp_ord = math.log(1 - 1.0 * m / k) - m * self.ln2 - lg[m + 1]
        return -0.5 * logp_clu - 0.5 * logp_ord

    def conserved(self, prev, cur):
        same_order = self.t[cur] > self.t[prev]
        return int(self.eq[prev] == same_order and self.eq[cur] == same_order)

    def compatible(self, b):
        """the unsigned box test of node b against every node at once (ClusterHits.cpp:158); empty nodes excluded"""
        gj = np.minimum((self.jMin - self.jMax[b]) & M32, (self.jMin[b] - self.jMax) & M32)
        gi = np.minimum((self.iMin - self.iMax[b]) & M32, (self.iMin[b] - self.iMax) & M32)
        ok = (gj <= self.box_d) & (gi <= self.box_d) & (self.size > 0)
        ok[b] = False
        return ok

    def pair_score(self, a, b):
        """chPairScore of two compatible, non-empty nodes"""
        k = int(self.size[a] + self.size[b])
        span = int(max(max(self.iMax[a], self.iMax[b]) - min(self.iMin[a], self.iMin[b]),
                       max(self.jMax[a], self.jMax[b]) - min(self.jMin[a], self.jMin[b]))) + 1
        ta, hb, tb, ha = self.tail[a], self.head[b], self.tail[b], self.head[a]
        seam = None
        if self.rank[ta] < self.rank[hb]:
            self.c['score_append'] += 1
            seam = self.conserved(ta, hb)
        elif self.rank[tb] < self.rank[ha]:
            self.c['score_prepend'] += 1
            seam = self.conserved(tb, ha)
        if seam is not None:
            return self.score_ksm(k, span, self.mcnt[a] + self.mcnt[b] + (0 if self.mutant == 'no_seam' else seam))
        self.c['score_interleaved'] += 1   # what the kernel's removed walk computed: the count over the rank-sorted union
        members = sorted(self.members(a) + self.members(b), key=lambda h: self.rank[h])
        return self.score_ksm(k, span, sum(self.conserved(x, y) for x, y in zip(members, members[1:])))

    def members(self, n):
        out, h = [], self.head[n]
        while h != NIL:
            out.append(h)
            h = self.next[h]
        return out

    def merge(self, i1, i2):
        h1, t1, h2, t2 = self.head[i1], self.tail[i1], self.head[i2], self.tail[i2]
        if h2 == NIL:
            raise IndexError('merge with an empty node')   # the kernel would read rank[NIL]
        if self.rank[t1] < self.rank[h2]:
            self.c['merge_append'] += 1
            self.next[t1] = h2
            self.tail[i1] = t2
            self.mcnt[i1] += self.mcnt[i2] + self.conserved(t1, h2)
        elif self.rank[t2] < self.rank[h1]:
            self.c['merge_prepend'] += 1
            self.next[t2] = h1
            self.head[i1] = h2
            self.mcnt[i1] += self.mcnt[i2] + self.conserved(t2, h1)
        else:
            self.c['merge_interleaved'] += 1
            members = sorted(self.members(i1) + self.members(i2), key=lambda h: self.rank[h])
            for x, y in zip(members, members[1:]):
                self.next[x] = y
            self.next[members[-1]] = NIL
            self.head[i1], self.tail[i1] = members[0], members[-1]
            self.mcnt[i1] = sum(self.conserved(x, y) for x, y in zip(members, members[1:]))
        self.head[i2] = NIL
        self.size[i1] += self.size[i2]
        self.size[i2] = 0
        self.iMin[i1] = min(self.iMin[i1], self.iMin[i2]); self.iMax[i1] = max(self.iMax[i1], self.iMax[i2])
        self.jMin[i1] = min(self.jMin[i1], self.jMin[i2]); self.jMax[i1] = max(self.jMax[i1], self.jMax[i2])


def _first_argmax(v, mutant=None):
    """index of the maximum, ties to the smaller index, as the kernel finds it: every thread keeps the first maximum of its
    indices i = thread + 256 n (the strided pre-reduction), blockArgMax the smallest index among the threads' maxima.
    The two mutants turn one of the two tie directions round."""
    m = v.max()
    at = np.nonzero(v == m)[0]
    per_thread = {}
    for i in at:
        if mutant == 'argmax_stride' or int(i) % 256 not in per_thread:
            per_thread[int(i) % 256] = int(i)
    return (max if mutant == 'argmax_block' else min)(per_thread.values()), float(m), len(at)


def cluster(q, t, s, d, lg, counts=None, mutant=None):
    """-> (node_of[K]: the node every hit ends in, merges).  q, t, s: positions and strand codes of one entry"""
    assert mutant is None or mutant in MUTANTS
    counts = new_counts() if counts is None else counts
    K = len(q)
    node_of = np.full(K, NIL, np.int64)
    if K <= 1:
        node_of[:] = 0
        return node_of, 0
    e = _Entry(q, t, s, d, lg, counts, mutant)
    dmin = np.zeros(K, np.int64)
    cached = np.zeros(K)
    for i in range(K):   # init: dmin[i] = first arg-max_j D[i][j], starting from D[i][0]
        best, bj, tie = 0.0, 0, False
        for j in np.nonzero(e.compatible(i))[0]:
            sc = e.pair_score(i, int(j))
            if j == 0 or sc > best or (mutant == 'init_ge' and sc >= best):
                best, bj, tie = sc, int(j), False
            elif sc == best and sc > 0:
                tie = True
        if mutant == 'init_ge' and best == 0.0:
            bj = K - 1   # `>=` walks a row of zeros to its end
        counts['init_tie'] += tie
        dmin[i], cached[i] = bj, best
    s_min = e.score_ksm(2, e.d + 1, 1)
    merges = 0
    while True:
        i1, max_score, holders = _first_argmax(cached, mutant)
        i2 = int(dmin[i1])
        if max_score == 0.0:
            counts['stop_zero'] += 1
            break
        counts['tied_argmax'] += holders > 1
        e.merge(i1, i2)
        merges += 1
        sc = np.zeros(K)
        for j in np.nonzero(e.compatible(i1))[0]:
            sc[j] = e.pair_score(int(j), i1)
        rows = np.ones(K, bool)
        rows[[i1, i2]] = False
        to_i2, to_i1 = rows & (dmin == i2), rows & (dmin == i1)
        live = rows & (e.size > 0)
        counts['stale_absorbed'] += int((to_i2 & live).sum())
        counts['stale_absorbing'] += int((to_i1 & live).sum())
        counts['stale_absorbing_fell'] += int((to_i1 & live & (sc < cached)).sum())
        counts['stale_third'] += int((live & ~to_i2 & ~to_i1 & (cached > 0)).sum())
        cur = np.where(to_i1, sc, cached)
        if mutant != 'keep_absorbed':
            cur = np.where(to_i2, 0.0, cur)
        take = rows & (sc > cur)
        counts['takeover'] += int(take.sum())
        dmin[take] = i1
        cached = np.where(take, sc, cur)
        cached[i2] = 0.0
        rj, rv, _ = _first_argmax(sc, mutant)
        dmin[i1], cached[i1] = rj, rv
        if not max_score >= s_min:
            counts['stop_smin'] += 1
            break
    for n in range(K):
        if e.size[n]:
            node_of[e.members(n)] = n
    return node_of, merges


def emit(L, lg, q, t, s, p, nq, node_of, cls, alpha, p_clu, p_mh):
    """the emission loop of sd_clusterhits_batch over a finished partition: nodes in index order, size >= cls, the two
    P-values from the product's host function, the float thresholds -> (cluster_of, rank, sizes, pCO, pMH)"""
    import ctypes as C
    from spacedust_amd._lib import ptr
    K = len(q)
    cof, rank = np.full(K, M32, np.uint32), np.zeros(K, np.uint32)
    sizes, pco, pmh = [], [], []
    if K > 1:
        for n in range(K):
            m = np.nonzero(node_of == n)[0]
            if len(m) < cls or len(m) == 0:
                continue
            co, mh = C.c_double(), C.c_double()
            order = np.zeros(len(m), np.uint32)
            qq, tt, ss, pp = (np.ascontiguousarray(a[m]) for a in (q, t, s, p))
            assert L.sd_host_cluster_pvalues(len(m), ptr(qq), ptr(tt), ptr(ss), ptr(pp), int(nq), float(alpha), ptr(lg), len(lg),
                                             C.byref(co), C.byref(mh), ptr(order)) == 0
            if co.value <= float(np.float32(p_clu)) and mh.value <= float(np.float32(p_mh)):
                cof[m[order]] = len(sizes)
                rank[m[order]] = np.arange(len(m))
                sizes.append(len(m))
                pco.append(co.value)
                pmh.append(mh.value)
    return cof, rank, np.array(sizes, np.uint32), np.array(pco, np.float64), np.array(pmh, np.float64)


def load_golden(path=None):
    """tests/golden/ch_classes.npz (tools/make_golden_ch_classes.py) -> (archive, rows): rows[(set, case)] = (cluster_of[K],
    rank[K], sizes[n], pCO bits[n], pMH bits[n]) for parameter set `set` of chgen.param_sets() and case index `case`"""
    import os
    import chgen
    g = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ch_classes.npz'))
    K, ncl = g['K'], g['n_clusters']
    rows, h, c, e = {}, 0, 0, 0
    for si, (ps, idx) in enumerate(chgen.param_sets()):
        assert tuple(g['params'][si]) == (ps['d'], ps['cls'], ps['alpha'], ps['p_clu'], ps['p_mh'], len(idx)), si
        for x in idx:
            k, n = int(K[x]), int(ncl[e])
            cof = g['cluster_of'][h:h + k].astype(np.uint32)
            rank = g['rank'][h:h + k].astype(np.uint32)
            none = cof == 0xFFFF
            cof[none], rank[none] = M32, 0
            rows[(si, x)] = (cof, rank, g['size'][c:c + n], g['pCO'][c:c + n], g['pMH'][c:c + n])
            h, c, e = h + k, c + n, e + 1
    assert (h, c, e) == (len(g['cluster_of']), len(g['size']), len(ncl))
    return g, rows
