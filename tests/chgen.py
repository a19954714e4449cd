"""Synthetic clusterhits entries shared by the CPU and GPU clusterhits tests: hits with unique query positions, syntenic
chains in both orientations with jitter, noise, random strands, P-values over the whole range the workflow produces."""
import numpy as np


def entry(rng, K, genome=600, chain_frac=0.6):
    q = np.sort(rng.choice(genome, size=K, replace=False)).astype(np.uint32)
    t = np.zeros(K, np.uint32)
    i = 0
    while i < K:
        run = int(rng.integers(1, 12))
        if rng.random() < chain_frac:
            start = int(rng.integers(0, genome))
            sign = 1 if rng.random() < 0.5 else -1
            for r in range(min(run, K - i)):
                t[i + r] = (start + sign * int(q[i + r] - q[i]) + int(rng.integers(-1, 2))) % genome
        else:
            t[i:i + run] = rng.integers(0, genome, size=min(run, K - i))
        i += run
    strands = rng.integers(0, 4, size=K).astype(np.uint8)
    pval = 10.0 ** rng.uniform(-60, -6.5, size=K)
    perm = rng.permutation(K)
    return q[perm], t[perm], strands[perm], pval[perm]


def many_entries(seed, n, kmax=120):
    """n entries, mostly small (the size distribution of real genome pairs), a few large"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 97 == 0:
            K = int(rng.integers(200, 500))
        else:
            K = int(min(kmax, 2 + rng.geometric(0.08)))
        genome = int(rng.choice([150, 600, 3000]))
        out.append(entry(rng, min(K, genome), genome=genome, chain_frac=float(rng.uniform(0.2, 0.9))) + (genome,))
    return out


# ---- constructed classes (tests/test_ch_classes.py, tests/test_gpu_clusterhits_classes.py) ---------------------------------
# Named entries aimed at single lines of csrc/hip/sd_clusterhits.hip (K) and of sd_clusterhits_batch (H); the expected rows
# come from the reference's compiled code (tools/make_golden_ch_classes.py -> tests/golden/ch_classes.npz).  Strand codes:
# bit 0 query, bit 1 target, so 0 and 3 pair equal strands (a conserved pair has to ascend on the target), 1 and 2 unequal
# ones (it must not ascend).  Unless a case says otherwise: strands 0, P-values 1e-20, Nq 600.

DEFAULT = dict(d=3, cls=2, alpha=1.0, p_clu=0.01, p_mh=0.01)
# every case runs with these three: the workflow's flags; both thresholds open, so that each cluster's P-values show
# (multihitPval's 1.0 is above 0.01); and the per-hit threshold theta = alpha / (Nq + 1) a hundred times lower
WIDE_SETS = (DEFAULT, dict(DEFAULT, p_clu=1.0, p_mh=1.0), dict(DEFAULT, alpha=0.01, p_clu=1.0, p_mh=1.0))
# the cases of GRID_CASES also run with d x cls x both thresholds: d enters sMin, the init gate and the box test of the
# kernel, cls and the float thresholds the emission loop
GRID_SETS = tuple(dict(d=d, cls=cls, alpha=1.0, p_clu=thr, p_mh=thr) for d in (1, 3, 10) for cls in (1, 2, 3, 5)
                  for thr in (0.01, 1.0, 1e-10))


def _case(name, q, t, s=0, p=1e-20, nq=600):
    q, t = np.asarray(q, np.uint32), np.asarray(t, np.uint32)
    s = np.full(len(q), s, np.uint8) if np.isscalar(s) else np.asarray(s, np.uint8)
    p = np.full(len(q), p, np.float64) if np.isscalar(p) else np.asarray(p, np.float64)
    assert len(q) == len(t) == len(s) == len(p)
    return dict(name=name, q=q, t=t, s=s, p=p, nq=int(nq), repeats=len(np.unique(q)) != len(q))


def _groups(*groups, gap=100):
    """several small constellations in one entry, `gap` positions apart on both axes so that they never interact"""
    q, t, s = [], [], []
    for g, (gq, gt, gs) in enumerate(groups):
        gs = [gs] * len(gq) if np.isscalar(gs) else gs
        q += [x + gap * g for x in gq]
        t += [x + gap * g for x in gt]
        s += list(gs)
    return q, t, s


def class_entries():
    """the named entries, in the order they form one batch"""
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    # H: K = 0 and K = 1 entries open, sit inside and close the batch (the kernel's `K <= 1` exit, the emission's `continue`)
    add('k0_first', [], [])
    add('k1_first', [5], [5])
    # K: the 256-thread stride of every `for (h = t; h < K; h += 256)` loop and of the pre-reduction before blockArgMax
    for K in (2, 3, 255, 256, 257, 511, 512, 513, 1030):
        e = entry(np.random.default_rng(1000 + K), K, genome=600 if K <= 513 else 3000, chain_frac=0.7)
        add('stride_%d' % K, e[0], e[1], e[2], e[3], nq=3000)
    # K: exact score ties across threads.  65 copies of one 8-hit chain, 40 positions apart: equal (k, span, m), so equal
    # doubles, at indices 8 c + i -- copies 32 apart share a thread (the strided pre-reduction has to keep the first), all
    # others meet in blockArgMax; then the same hits under a fixed permutation
    lq = np.array([40 * c + i for c in range(65) for i in range(8)])
    add('tie_lattice', lq, lq + 7)
    perm = np.random.default_rng(65).permutation(len(lq))
    add('tie_lattice_perm', lq[perm], lq[perm] + 7)
    # K: one collinear chain: counts accumulated over long lists (mcnt, the seam term), every row's dmin stale for long
    add('collinear_600', np.arange(600), np.arange(600) + 11)
    # K: the box test `gj <= d && gi <= d` at gaps of exactly d and d + 1 on either axis, for every d of the grid; position 0
    for d in (1, 3, 10):
        add('gaps_d%d' % d, *_groups(([0, d], [0, 1], 0), ([0, d + 1], [0, 1], 0), ([0, 1], [0, d], 0), ([0, 1], [0, d + 1], 0),
                                    ([0, d], [0, d], 0), ([0, d + 1], [0, d + 1], 0), ([0, 1, 1 + d], [0, 1, 2], 0),
                                    ([0, 1, 2 + d], [0, 1, 2], 0)))
    # K: the unsigned gap of two ranges on the target axis: touching (0), nested and overlapping (both differences wrap: never
    # compatible), after the two chains have formed
    add('box_touching', [0, 1, 2, 4, 5, 6], [10, 11, 12, 12, 13, 14])
    add('box_nested', [0, 1, 2, 3, 5, 6], [10, 12, 14, 16, 12, 13])
    add('box_overlap', [0, 1, 2, 4, 5, 6], [10, 12, 14, 13, 15, 17])
    add('box_query_nested', [0, 2, 4, 6, 1, 3], [10, 12, 14, 16, 30, 31])
    # H/K: positions near 100 000: a long logGamma table (the guard `maxPos + 3 > lGammaLen`), lg[] read far out
    add('far_positions', [99990, 99991, 99993, 99996, 0, 1, 2], [99980, 99981, 99982, 99983, 99999, 99998, 99997], [0, 0, 3, 3, 1, 2, 1])
    # K: chConserved's strict `tPos[cur] > tPos[prev]`: equal target positions inside a chain and at the seam of two chains
    add('tpos_repeat_inside', *_groups(([0, 1, 2, 3], [5, 5, 6, 7], 0), ([0, 1, 2, 3], [7, 6, 6, 5], 1)))
    add('tpos_repeat_seam', *_groups(([0, 1, 3, 4], [5, 6, 6, 7], 0), ([0, 1, 3, 4], [7, 6, 6, 5], 2)))
    # K: the four strand codes on either side of a seam
    add('strands_seam', *_groups(*[([0, 1, 3, 4], [5, 6, 8, 9], [0, a, b, 0]) for a in range(4) for b in range(4)]))
    # K: descending chains under every strand code (conserved only for 1 and 2), ascending ones beside them
    add('strands_descending', *_groups(*[([0, 1, 2, 3, 4], [9, 8, 7, 6, 5], c) for c in range(4)]
                                      + [([0, 1, 2, 3, 4], [5, 6, 7, 8, 9], c) for c in range(4)]))
    # K: `if (!(maxScore >= sMin)) break` after the merge: one pair, span d + 1, not conserved (score sMin - ln 2): merged,
    # then the loop stops although a conserved pair waits
    add('stop_below_smin', *_groups(([0, 3], [1, 0], 0), ([0, 1], [0, 1], 1)))
    # K: `if (maxScore == 0.0) break`: nothing left to merge / nothing to merge at all
    add('stop_zero', [0, 1, 2], [0, 1, 2])
    add('stop_zero_at_once', [0, 10, 20, 30], [0, 10, 20, 30])
    # K: the stale dmin rules (`dj == i2 ? 0.0 : (dj == i1 ? s : cached[j])`).  A row that pointed at the absorbed node: hits
    # 1 and 2 are each other's best, 0 and 3 point at them from the outside
    add('stale_absorbed', [0, 2, 3, 5, 40], [0, 2, 3, 5, 40])
    # a row that pointed at the absorbing node and whose score falls: hit 2's best is hit 0, whose union with hit 1 then
    # spans hit 2's target position (nested ranges are incompatible: the score falls to 0)
    add('stale_absorbing_falls', [3, 4, 0, 40], [3, 5, 4, 40])
    # a row whose dmin stays on a third node while the merged node would now be its best
    add('stale_third', [0, 1, 3, 4, 6, 7, 9], [0, 1, 3, 4, 6, 7, 9])
    # K: a tie at init: `s > best` keeps the first of two equal scores in row 0, whose hit has a neighbour d genes away on
    # either side, both unconserved (score sMin - ln 2): the first is merged, then the loop stops, so the choice shows
    add('init_tie', [3, 0, 6], [3, 4, 2])
    add('k0_mid', [], [])
    add('k1_mid', [7], [9], 3)
    # two ordinary small entries for the parameter grid (chains, noise, all strand codes; 30 and 64 hits)
    for nm, K, seed in (('grid_random_a', 30, 31), ('grid_random_b', 64, 32)):
        e = entry(np.random.default_rng(seed), K, genome=150, chain_frac=0.7)
        add(nm, e[0], e[1], e[2], e[3], nq=150)
    # H: repeated query positions (two or three hits per position): the dense host path, unions below and above the 16 elements
    # at which libstdc++'s std::sort changes from insertion sort to introsort.  Target positions stay distinct: a union of k
    # hits then spans at least k genes, and the reference reads lookup[span - k + 1] inside its table
    for K, npos, seed in ((4, 2, 1), (9, 4, 2), (14, 6, 3), (16, 7, 4), (24, 10, 5), (33, 20, 6), (40, 20, 7), (48, 60, 8), (60, 20, 9),
                          (60, 60, 10), (59, 150, 11)):
        rng = np.random.default_rng(7000 + seed)
        q = rng.integers(0, npos, size=K)
        if len(np.unique(q)) == K:
            q[-1] = q[0]
        if seed % 2:   # collinear, equal positions in random order, a few hits displaced
            t = np.empty(K, np.int64)
            t[np.lexsort((rng.random(K), q))] = np.arange(K) + 30
            x = rng.choice(K, size=max(2, K // 8), replace=False)
            t[x] = t[np.roll(x, 1)]
        else:
            t = rng.choice(npos + K, size=K, replace=False)
        add('repeat_q_%d_%d' % (K, npos), q, t, rng.integers(0, 4, size=K), 10.0 ** rng.uniform(-40, -3, size=K), nq=npos + 50)
    add('repeat_q_chain', [0, 1, 1, 2, 3, 3, 3, 4, 5, 6, 6, 7, 8, 9, 9, 10, 11, 12, 12, 13], [0, 1, 2, 3, 4, 6, 5, 7, 8, 9, 10, 11, 12, 14, 13, 15, 16, 17, 18, 19])
    # H: multihitPval's edges.  theta = alpha / (Nq + 1) = 0.1 at Nq 9, alpha 1: no hit below it (-> 1.0), exactly one (the
    # sum runs over k - 1 = 0 terms -> 0.0), a P-value of 0 (r infinite -> 0.0), r so large that exp(-r) underflows (-> 0.0), and
    # an ordinary value beside them
    chain = ([0, 1, 2, 3], [0, 1, 2, 3])
    add('pmh_none_below', *chain, 0, [0.5, 0.2, 0.9, 0.11], nq=9)
    add('pmh_one_below', *chain, 0, [0.5, 0.05, 0.9, 0.11], nq=9)
    add('pmh_pval_zero', *chain, 0, [0.5, 0.0, 1e-5, 0.11], nq=9)
    add('pmh_underflow', *chain, 0, [1e-300, 1e-300, 1e-200, 1e-3], nq=9)
    add('pmh_ordinary', *chain, 0, [1e-3, 2e-4, 0.05, 0.2], nq=9)
    add('pmh_at_alpha', *chain, 0, [1e-3, 1.5e-3, 0.9e-3, 1e-4], nq=9)   # around theta = 0.001 at alpha 0.01
    add('k0_last', [], [])
    add('k1_last', [0], [0])
    assert len({c['name'] for c in out}) == len(out)
    return out


# the cases of the parameter grid: everything small whose outcome depends on d, cls or a threshold
GRID_CASES = ('stride_2', 'stride_3', 'gaps_d1', 'gaps_d3', 'gaps_d10', 'box_touching', 'box_nested', 'box_overlap', 'box_query_nested',
              'tpos_repeat_inside', 'tpos_repeat_seam', 'strands_seam', 'strands_descending', 'stop_below_smin', 'stop_zero',
              'stale_absorbed', 'stale_absorbing_falls', 'stale_third', 'init_tie', 'repeat_q_16_7', 'repeat_q_40_20', 'repeat_q_chain',
              'pmh_ordinary', 'k0_mid', 'k1_mid', 'grid_random_a', 'grid_random_b')


def param_sets():
    """[(parameters, indices of the cases they run on)], the cases in class_entries order"""
    names = [c['name'] for c in class_entries()]
    grid = [names.index(n) for n in GRID_CASES]
    every = list(range(len(names)))
    return [(ps, every) for ps in WIDE_SETS] + [(ps, grid) for ps in GRID_SETS if ps != DEFAULT]


def digest(cases):
    """a digest of everything the generator supplies (the golden rows carry it: a changed generator fails loudly)"""
    import hashlib
    h = hashlib.sha256()
    for c in cases:
        h.update(c['name'].encode() + b'\0')
        for k in ('q', 't', 's', 'p'):
            h.update(np.ascontiguousarray(c[k]).tobytes())
        h.update(np.uint32(c['nq']).tobytes())
    for ps, idx in param_sets():
        h.update(repr((ps['d'], ps['cls'], float(ps['alpha']), float(ps['p_clu']), float(ps['p_mh']), idx)).encode())
    return h.hexdigest()
