"""The paths of the exhaustive ungapped prefilter (sd_ungapped.hip) that only large or ragged inputs take, each against the numpy
restatement of tests/ungapped_ref.py, every pair and every list compared exactly:

  A  query sub-batches (q0 > 0) over 2^20 + 1 pooled targets: the scan, the select kernel and the host copies of every pass;
  B  the multi-strip class with a grid stride: a wavefront scans several ragged targets one after the other;
  C  coverage modes 0 to 5 with pairs exactly at the float32 threshold, over more than 256 targets with permuted keys;
  D  residue codes above 20 on either side.

Every test states the condition that makes it reach its path as an assertion on its inputs (number of passes, groups per
workgroup, size of the tie class at the cut, high key bytes, both outcomes of every coverage mode), computed from the
restatement or from the launch arithmetic quoted from the source."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ungapped_ref as ur

pytestmark = pytest.mark.gpu

UG_WAVES = 4
X = 20
W = ur.ALPHABET.index('W')
GOLDEN_PATHS = os.path.join(ur.ROOT, 'tests', 'golden', 'ungapped_paths.npz')


@pytest.fixture(scope='module')
def env():
    from spacedust_amd.api import Host, Context
    return Host(), Context(0)


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    res = np.concatenate([np.asarray(s, np.uint8) for s in seqs]) if len(seqs) else np.zeros(0, np.uint8)
    return res.astype(np.uint8), off


def sub_batch(n_t):
    """queries per pass, as both entry points of sd_ungapped.hip compute it:
        const uint64_t stride = ((uint64_t) nT + 3) & ~(uint64_t) 3;
        const uint32_t sub = (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>(65535, ((uint64_t) 1 << 30) / stride));"""
    stride = (n_t + 3) & ~3
    return max(1, min(65535, (1 << 30) // stride))


def multi_grid_x(n_t, max_t_len, n_long):
    """workgroups along the targets of a multi-strip launch over n_long queries, as ugScanRange computes it:
        const uint32_t groups = (nT + UG_WAVES - 1) / UG_WAVES;
        const uint32_t lineLen = (maxTLen + 63) & ~63u;
        const uint32_t want = std::max(32u, (2048u + n - 1) / n);
        const uint32_t fit = (uint32_t) std::max<size_t>(1, ((size_t) 64 << 20) / ((size_t) UG_WAVES * 2 * lineLen));
        const uint32_t gxm = std::max(1u, std::min(std::min(want, fit), groups));
    Returns (groups, gxm)."""
    groups = (n_t + UG_WAVES - 1) // UG_WAVES
    line_len = (max(1, max_t_len) + 63) & ~63
    want = max(32, (2048 + n_long - 1) // n_long)
    fit = max(1, (64 << 20) // (UG_WAVES * 2 * line_len))
    return groups, max(1, min(want, fit, groups))


def length_class(n):
    """the scan kernel's class of a query: 128, 256, 512 rows per strip, several strips (ugScanRange)"""
    return 0 if n <= 128 else (1 if n <= 256 else (2 if n <= 512 else 3))


# ---------------------------------------------------------------------------------------------------------------- A: sub-batches

N_T_BIG = (1 << 20) + 1
N_Q_BIG = 2200
DEEP_MIN = 0.15        # share of the queries whose composition bias has one very negative entry: a low ceiling


def make_big_case(M):
    """test A's input.  Targets: N_T_BIG draws from a pool of distinct sequences of 0 to 12 residues -- a few `common` ones
    (empty, single residues, all-X, a residue next to an X) make up nearly all targets, every other pool member is drawn a
    handful of times, so a score is shared by ~10^5 targets and only a few hundred targets score above the common ones.
    Queries: all four length classes shuffled, windows of pool members planted in them, a synthetic composition bias in
    [-3, 2] with one entry per query far lower (the ceiling 255 - bias differs from query to query)."""
    rng = np.random.default_rng(20261017)
    pool, weight = [], []

    def add(s, w):
        pool.append(np.asarray(s, np.uint8))
        weight.append(w)
    add([], 5.0)
    for a in range(20):
        add([a], {W: 12.0, 4: 10.0, 8: 8.0}.get(a, 2.5))   # W, C (4), H (8)
    for n, w in ((1, 2.0), (2, 2.0), (5, 6.0), (12, 14.0)):
        add([X] * n, w)
    for a in (0, 9, 10, 15, 17):                            # A, I, L, S, V next to an X
        add([a, X], 1.5)
        add([X, a], 1.5)
    n_common = len(pool)
    add([W] * 12, 0.0)
    runs = len(pool) - 1
    seen = {bytes(p) for p in pool}
    while len(pool) < 260:
        s = rng.integers(0, 20, int(rng.integers(2, 13))).astype(np.uint8)
        if rng.random() < 0.2:
            s[int(rng.integers(0, len(s)))] = X
        if bytes(s) not in seen:
            seen.add(bytes(s))
            add(s, 0.0)
    n_rare = len(pool) - n_common
    rare_ids = np.concatenate([np.arange(n_common, len(pool)), [runs] * 4])   # once each, the run of W five times
    p = np.asarray(weight) / np.sum(weight)
    pool_id = np.concatenate([rare_ids, rng.choice(len(pool), N_T_BIG - len(rare_ids), p=p)]).astype(np.int64)
    pool_id = pool_id[rng.permutation(N_T_BIG)]
    # unique keys over the whole uint32 range, in no order
    keys = np.unique(rng.integers(0, 1 << 32, N_T_BIG + (N_T_BIG >> 2), dtype=np.uint64))
    keys = keys[rng.permutation(len(keys))[:N_T_BIG]].astype(np.uint32)

    lens = [0, 1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1100]
    lens += rng.integers(513, 1101, 60).tolist()
    rest = N_Q_BIG - len(lens)
    lens += rng.integers(1, 129, rest // 3).tolist() + rng.integers(129, 257, rest // 3).tolist()
    lens += rng.integers(257, 513, N_Q_BIG - len(lens)).tolist()
    lens = [lens[i] for i in rng.permutation(N_Q_BIG)]
    queries, biases = [], []
    for n in lens:
        q = rng.integers(0, 20, n).astype(np.uint8)
        cb = rng.integers(-3, 3, n).astype(np.int8)
        for _ in range(n // 40):                            # windows of rare pool members
            s = pool[int(rng.integers(n_common, len(pool)))]
            at = int(rng.integers(0, n - len(s) + 1))
            q[at:at + len(s)] = s
        if n > 0:
            deep = n >= 30 and rng.random() < DEEP_MIN
            if deep:                                        # a run of W that reaches the low ceiling
                at = int(rng.integers(0, n - 12))
                q[at:at + 12] = W
                cb[at:at + 12] = 2
                low = int(rng.choice(np.setdiff1d(np.arange(n), np.arange(at, at + 12))))
            else:
                low = int(rng.integers(0, n))
            cb[low] = -int(rng.integers(100, 126)) if deep else -int(rng.integers(4, 10))
        queries.append(q)
        biases.append(cb)
    q_res, q_off = pack(queries)
    q_cb = np.concatenate(biases).astype(np.int8)
    pool_res, pool_off = pack(pool)
    ident = rng.integers(0, N_T_BIG, N_Q_BIG).astype(np.uint32)
    small = ur.restate_matrix(M, q_res, q_off, q_cb, pool_res, pool_off)
    return dict(pool=pool, pool_res=pool_res, pool_off=pool_off, pool_id=pool_id, keys=keys, n_common=n_common, n_rare=n_rare,
                q_res=q_res, q_off=q_off, q_cb=q_cb, q_len=np.asarray(lens, np.int64), ident=ident, small=small,
                caps=np.array([255 - ur.bias_of(M, cb) for cb in biases]))


# the three list rules of test A: (max_seqs, min_score)
BIG_CASES = ((1, 15), (300, 0), (1000, 15))


def cut_class(small_row, copies, max_seqs, min_score):
    """where the cut of one query falls (identity aside): (targets in the score class of the last kept hit, how many of them
    are kept); (0, 0) where the list is not cut"""
    hist = np.bincount(small_row, weights=copies, minlength=256).astype(np.int64)
    cum = 0
    for s in range(255, min_score, -1):
        if cum + hist[s] >= max_seqs:
            return int(hist[s]), max_seqs - cum
        cum += int(hist[s])
    return 0, 0


def check_big_conditions(c):
    """the conditions on test A's input, from the restatement and the source's arithmetic alone"""
    n_q, n_t = N_Q_BIG, N_T_BIG
    sub = sub_batch(n_t)
    assert n_t > (1 << 20) and n_t % 4 != 0
    assert n_q > 2 * sub and n_q % sub != 0 and n_q % sub < sub // 2          # three passes or more, a short last one
    classes = np.array([length_class(n) for n in c['q_len']])
    for q0 in range(0, n_q, sub):                                             # every pass holds every class
        assert set(classes[q0:q0 + sub].tolist()) == {0, 1, 2, 3}, q0
    assert (c['q_len'] == 0).sum() == 1 and (c['q_len'] > 512).sum() >= 3
    assert (c['caps'][sub:] != c['caps'][:n_q - sub]).mean() > 0.5             # the ceiling of row r and of row r + sub differ
    assert (c['ident'][sub:] != c['ident'][:n_q - sub]).all()
    pool_len = (c['pool_off'][1:] - c['pool_off'][:-1]).astype(np.int64)
    assert 200 <= len(c['pool']) <= 400 and pool_len.min() == 0 and pool_len.max() == 12
    assert len({bytes(p) for p in c['pool']}) == len(c['pool'])
    assert any(len(p) > 1 and (p == X).all() for p in c['pool']) and sum(len(p) == 1 for p in c['pool']) >= 20
    copies = np.bincount(c['pool_id'], minlength=len(c['pool']))
    assert (copies > 0).all()
    t_len = pool_len[c['pool_id']]
    assert 2 << 20 < int(t_len.sum()) < 8 << 20 and (t_len == 0).sum() > 1000
    # the ceiling is reached, in more than one pass and at different values
    at_cap = (c['small'] == c['caps'][:, None]).any(axis=1)
    assert at_cap[:sub].any() and at_cap[sub:2 * sub].any() and at_cap[2 * sub:].any()
    assert len(set(c['caps'][at_cap].tolist())) > 5
    keys = c['keys']
    assert len(np.unique(keys)) == n_t and (keys >= 1 << 24).any() and (keys >= 1 << 31).any() and (keys < 1 << 24).any()
    assert (np.diff(keys.astype(np.int64)) < 0).sum() > n_t // 3              # not in index order
    # max_seqs = 300: the cut falls strictly inside a score class of more than 65 536 targets, for most queries
    inside = 0
    for q in range(n_q):
        size, kept = cut_class(c['small'][q], copies, 300, 0)
        inside += size > 65536 and 0 < kept < size
    assert inside > n_q * 3 // 4, inside
    # max_seqs = 1 cuts nearly every list, max_seqs = 1000 none: whole lists are far shorter than the rows of 10^6 scores
    longest = max(int(copies[c['small'][q] > 15].sum()) for q in range(n_q)) + 1
    assert 1 < longest < 1000, longest
    return sub


@pytest.fixture(scope='module')
def big(env):
    host, gpu = env
    M = host.matrix(0)[0]
    c = make_big_case(M)
    c['M'] = M
    c['sub'] = check_big_conditions(c)
    return c


@pytest.fixture(scope='module')
def big_sets(env, big):
    """the two sequence sets of test A on the device, built and uploaded once: (queries, targets, target lengths, residues)"""
    host, gpu = env
    c = big
    pool_len = (c['pool_off'][1:] - c['pool_off'][:-1]).astype(np.int64)
    t_len = pool_len[c['pool_id']]
    t_off = np.zeros(N_T_BIG + 1, np.uint64)
    np.cumsum(t_len, out=t_off[1:])
    # residue x of target t is residue x of its pool member
    start = c['pool_off'][:-1].astype(np.int64)[c['pool_id']]
    within = np.arange(int(t_off[-1]), dtype=np.int64) - np.repeat(t_off[:-1].astype(np.int64), t_len)
    t_res = c['pool_res'][np.repeat(start, t_len) + within]
    return gpu.seqset(c['q_res'], c['q_off'], c['q_cb']), gpu.seqset(t_res, t_off, None), t_len, int(t_off[-1])


def test_sub_batches_score_every_pair(env, big, big_sets):
    """A (i), (iii): sd_ungapped_score_matrix over three passes of queries (q0 = 0, sub, 2 sub; the last one short): every one
    of the 2 200 x 1 048 577 scores against the restatement expanded from the pool, row by row"""
    from spacedust_amd import api
    host, gpu = env
    c = big
    q_set, t_set, t_len, t_total = big_sets
    # 2 200 x 1 048 577 bytes = 2.3 GB on the host.  No smaller input takes three passes: sub is at most 2^30 / nT, so
    # nQ > 2 sub with nT > 2^20 means more than 2^31 pairs.  N_Q_BIG must not be trimmed to save memory.
    got = api.ungapped_scores(gpu, c['M'], q_set, t_set)
    assert got.shape == (N_Q_BIG, N_T_BIG)
    assert api.ungapped_last_cells(gpu) == len(c['q_res']) * t_total
    small8 = c['small'].astype(np.uint8)
    bad = []
    for q in range(N_Q_BIG):
        exp = ur.expand_pooled(small8[q], c['pool_id'])
        if not np.array_equal(got[q], exp):
            t = int(np.flatnonzero(got[q] != exp)[0])
            bad.append((q, q // c['sub'], t, int(got[q, t]), int(exp[t]), int((got[q] != exp).sum())))
    print('%d x %d pairs in passes of %d queries: %d rows differ' % (N_Q_BIG, N_T_BIG, c['sub'], len(bad)))
    assert not bad, bad[:10]   # (query, pass, first target, got, expected, differing targets of the row)


@pytest.mark.parametrize('max_seqs,min_score', BIG_CASES)
def test_sub_batches_lists_follow_the_list_rule(env, big, big_sets, max_seqs, min_score):
    """A (ii): sd_ungapped_prefilter_batch over the same passes: the list of every query against list_rule_fast -- unique
    keys over the whole uint32 range, an arbitrary identity target per query, the cut inside a tie class of ~10^5 targets"""
    from spacedust_amd import api
    host, gpu = env
    c = big
    q_set, t_set, t_len, _ = big_sets
    keys, ident = c['keys'], c['ident']
    keys64 = keys.astype(np.uint64)
    small8 = c['small'].astype(np.uint8)
    par = api.ungapped_params(host, max_hits=max_seqs, min_score=min_score)
    hits, counts = api.ungapped_prefilter(gpu, par, q_set, t_set, target_keys=keys, identity_id=ident)
    assert (hits['diagonal'] == 0).all()

    def one(q):
        ek, es = ur.list_rule_fast(ur.expand_pooled(small8[q], c['pool_id']), keys64, c['q_len'][q], t_len, min_score=min_score,
                                   max_seqs=max_seqs, identity_key=int(keys[ident[q]]))
        h = hits[q, :counts[q]]
        if len(h) == len(ek) and np.array_equal(keys[h['seqId']], ek) and np.array_equal(h['score'].astype(np.int32), es):
            return None
        return (q, q // c['sub'], int(counts[q]), len(ek), [(int(keys[x['seqId']]), int(x['score'])) for x in h[:3]],
                list(zip(ek[:3].tolist(), es[:3].tolist())))
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        bad = [b for b in ex.map(one, range(N_Q_BIG)) if b is not None]
    print('max_seqs %d, min_score %d: %d hits, %d lists differ' % (max_seqs, min_score, int(counts.sum()), len(bad)))
    assert not bad, bad[:5]   # (query, pass, got length, expected length, got head, expected head)
    assert (counts == max_seqs).mean() > 0.9 if max_seqs <= 300 else 1 < counts.max() < max_seqs   # cut nearly everywhere / nowhere


# ------------------------------------------------------------------------------------- B: several strips, several targets per wavefront

@pytest.fixture(scope='module')
def paths():
    return np.load(GOLDEN_PATHS)


def check_paths_conditions(g):
    q_len = (g['q_off'][1:] - g['q_off'][:-1]).astype(np.int64)
    t_len = (g['t_off'][1:] - g['t_off'][:-1]).astype(np.int64)
    n_q, n_t = len(q_len), len(t_len)
    assert n_q == 64 and q_len.min() == 513 and q_len.max() > 1600
    for n in (1023, 1024, 1025, 1535, 1536, 1537):
        assert n in q_len, n
    assert (q_len % 2 == 1).any() and (q_len % 512 == 0).sum() >= 2
    assert n_t >= 300
    assert (t_len == 0).sum() >= 5 and t_len.max() >= 1100 and ((t_len > 0) & (t_len < 64)).sum() > 20
    # all 64 queries are in one multi-strip launch; a workgroup scans the target groups g, g + gxm, g + 2 gxm, ...
    groups, gxm = multi_grid_x(n_t, int(t_len.max()), n_q)
    assert groups > gxm and groups >= 2 * gxm   # every workgroup scans two groups or more
    # the wavefront that scanned target t scans target t + 4 gxm next: a long one right before a short one, and before an empty one
    step = UG_WAVES * gxm
    before, after = t_len[:-step], t_len[step:]
    assert ((after > 0) & (before >= 4 * after) & (before > 512)).sum() >= 3
    assert ((after == 0) & (before > 512)).any() and ((before == 0) & (after > 512)).any()
    # the generator planted its pairs at this step (its STEP), and a scan whose first strip read the boundary line the
    # wavefront's previous target left behind -- simulated there, lines zero at the start -- would score differently
    # (multi_grid_x is a copy by hand of the quoted lines of ugScanRange: a change of the constants in sd_ungapped.hip has to be
    # made there as well, and then this step, the fixture's STEP and its planted pairs change with it)
    assert step == 128
    for name, stale in (('score_cb', 'stale_cb'), ('score_nocb', 'stale_nocb')):
        changed = g[stale] != g[name]
        assert changed.sum() >= 40 and changed.any(axis=1).sum() >= 8, name
        assert not changed[q_len <= 1024].any()   # (two strips: the line strip 0 would read is never written)
    for name, cb in (('score_cb', g['q_cb']), ('score_nocb', None)):
        caps = np.array([255 - ur.bias_of(g['M'], None if cb is None else cb[int(g['q_off'][q]):int(g['q_off'][q + 1])]) for q in range(n_q)])
        at_cap = g[name] == caps[:, None]
        assert at_cap.sum() > 100 and (g[name] < caps[:, None]).sum() > 1000 and at_cap.any(axis=1).sum() > n_q // 2, name
    return gxm


def test_multi_strip_queries_over_a_grid_stride(env, paths):
    """B: 64 queries of two to four strips against 300 ragged targets, three target groups per workgroup, with and without
    composition bias: the full matrix against tests/golden/ungapped_paths.npz (tools/make_golden_ungapped_paths.py wrote it
    from ungapped_ref.restate_matrix)"""
    from spacedust_amd import api
    host, gpu = env
    g = paths
    check_paths_conditions(g)
    assert np.array_equal(host.matrix(0)[0].reshape(21, 21), g['M'])
    t_set = gpu.seqset(g['t_res'], g['t_off'], None)
    for name, cb in (('score_cb', g['q_cb']), ('score_nocb', None)):
        q_set = gpu.seqset(g['q_res'], g['q_off'], cb)
        got = api.ungapped_scores(gpu, g['M'].reshape(-1), q_set, t_set)
        diff = np.argwhere(got != g[name])
        print('%s: %d pairs, %d mismatches' % (name, got.size, len(diff)))
        assert len(diff) == 0, [(int(a), int(b), int(got[a, b]), int(g[name][a, b])) for a, b in diff[:10]]


# -------------------------------------------------------------------------------------------------- C: coverage modes, > 256 targets

COV_THR = 0.8


def make_coverage_case(M):
    """queries and pool members are windows of one master sequence starting at its first residue, mutated lightly, so nearly
    every pair scores above the threshold and only the coverage decides; the lengths put pairs exactly at 0.8 (40/50, 80/100,
    100/125, 200/250), just below and just above it, and at ratio 1"""
    rng = np.random.default_rng(77)
    master = rng.integers(0, 20, 400).astype(np.uint8)

    def window(n):
        s = master[:n].copy()
        hit = rng.random(n) < 0.05
        s[hit] = rng.integers(0, 20, int(hit.sum()))
        return s
    q_lens = [100, 80, 125, 50, 250, 99, 101, 40, 200, 64, 0, 1, 129, 160]
    pool_lens = [0, 1, 32, 39, 40, 41, 50, 63, 64, 65, 79, 80, 81, 99, 100, 101, 124, 125, 126, 128, 156, 157, 160, 199, 200, 201,
                 250, 251, 312, 313, 400]
    queries = [window(n) for n in q_lens]
    pool = [window(n) for n in pool_lens]
    n_t = 1003
    pool_id = np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), n_t - len(pool))])[rng.permutation(n_t)]
    keys = (rng.permutation(n_t).astype(np.uint32) * np.uint32(4282663) + np.uint32(0x7F000000))   # odd multiplier: still unique
    q_res, q_off = pack(queries)
    q_cb = rng.integers(-2, 3, len(q_res)).astype(np.int8)
    pool_res, pool_off = pack(pool)
    small = ur.restate_matrix(M, q_res, q_off, q_cb, pool_res, pool_off)
    t_res, t_off = pack([pool[i] for i in pool_id])
    return dict(q_res=q_res, q_off=q_off, q_cb=q_cb, q_len=np.asarray(q_lens), t_res=t_res, t_off=t_off,
                t_len=np.asarray(pool_lens)[pool_id], pool_id=pool_id, keys=keys, small=small)


def check_coverage_conditions(c, min_score):
    n_t = len(c['pool_id'])
    assert n_t > 3 * 256 and n_t % 4 != 0 and len(np.unique(c['keys'])) == n_t and (c['keys'] >= 1 << 31).any()
    thr = np.float32(COV_THR)
    full = ur.expand_pooled(c['small'], c['pool_id'])
    scoring = full > min_score
    for mode in range(6):
        kept = np.array([ur.covered_mask(COV_THR, mode, c['q_len'][q], c['t_len']) for q in range(len(c['q_len']))])
        assert (kept & scoring).sum() > 100 and (~kept & scoring).sum() > 100, mode          # both outcomes, among scoring pairs
        # pairs whose ratio is the float32 threshold itself are kept: a quotient one ulp low would drop them
        q, t = np.meshgrid(c['q_len'].astype(np.float32), c['t_len'].astype(np.float32), indexing='ij')
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = {0: np.minimum(q / t, t / q), 1: q / t, 2: t / q, 3: t / q, 4: q / t, 5: np.minimum(t, q) / np.maximum(t, q)}[mode]
        exact = (ratio == thr) & scoring
        assert exact.sum() > 20 and kept[exact].all(), mode
        if mode in (3, 4):   # the upper bound 1 both keeps (ratio 1) and drops (ratio above 1, threshold met)
            assert ((ratio == 1) & kept & scoring).any() and ((ratio > 1) & ~kept & scoring).sum() > 100, mode
    return full


def test_coverage_modes_over_more_than_256_targets(env):
    """C: every coverage mode of ugCanBeCovered (0 to 5) at threshold 0.8 with pairs exactly at the threshold, over 1 003 pooled
    targets with permuted keys above 2^31: the select kernel's thread loops take four trips, its radix rounds see every byte"""
    from spacedust_amd import api
    host, gpu = env
    M = host.matrix(0)[0]
    c = make_coverage_case(M)
    min_score = 15
    full = check_coverage_conditions(c, min_score)
    n_q, n_t = full.shape
    q_set, t_set = gpu.seqset(c['q_res'], c['q_off'], c['q_cb']), gpu.seqset(c['t_res'], c['t_off'], None)
    got = api.ungapped_scores(gpu, M, q_set, t_set)
    assert np.array_equal(got, full)
    keys = c['keys']
    ident = np.random.default_rng(3).integers(0, n_t, n_q).astype(np.uint32)
    cut = 0
    for mode in range(6):
        for max_seqs in (n_t, 50):
            par = api.ungapped_params(host, max_hits=max_seqs, min_score=min_score, cov_mode=mode, cov_thr=COV_THR)
            hits, counts = api.ungapped_prefilter(gpu, par, q_set, t_set, target_keys=keys, identity_id=ident)
            for q in range(n_q):
                exp = ur.list_rule(full[q], keys, c['q_len'][q], c['t_len'], min_score=min_score, max_seqs=max_seqs, cov_mode=mode,
                                   cov_thr=COV_THR, identity_key=keys[ident[q]])
                have = [(int(keys[h['seqId']]), int(h['score'])) for h in hits[q, :counts[q]]]
                assert have == exp, (mode, max_seqs, q, have[:5], exp[:5])
                cut += max_seqs < n_t and len(exp) == max_seqs
    assert cut > 30   # the cut to 50 was applied under every mode


# ------------------------------------------------------------------------------------------------------ D: residue codes above 20

def test_residue_codes_above_20_count_as_x(env):
    """D: sd_seqset_create admits any byte as a residue; the scan clamps it to 20 on both sides (min(..., 20) where the
    profile is built and where the target chunk is fetched), which is the restatement with every code above 20 replaced by X"""
    from spacedust_amd import api
    host, gpu = env
    M = host.matrix(0)[0]
    rng = np.random.default_rng(21)
    master = rng.integers(0, 20, 1300).astype(np.uint8)

    def dirty(s, rate):
        s = s.copy()
        hit = rng.random(len(s)) < rate
        s[hit] = rng.choice([21, 22, 25, 26, 31, 32, 63, 64, 127, 128, 200, 254, 255], int(hit.sum()))
        return s
    queries = [dirty(master[:n], 0.1) for n in (1, 5, 128, 129, 256, 300, 512, 513, 1025, 1300)]
    queries.append(np.full(70, 255, np.uint8))
    targets = []
    for n in rng.integers(0, 700, 120):
        a = int(rng.integers(0, 1300 - n))
        targets.append(dirty(master[a:a + n], 0.1))
    targets += [np.full(40, 21, np.uint8), np.full(3, 255, np.uint8), np.zeros(0, np.uint8)]
    q_res, q_off = pack(queries)
    t_res, t_off = pack(targets)
    q_cb = rng.integers(-3, 4, len(q_res)).astype(np.int8)
    for res in (q_res, t_res):
        assert (res == 21).any() and (res == 255).any() and (res > 20).mean() > 0.05
    exp = ur.restate_matrix(M, np.minimum(q_res, X), q_off, q_cb, np.minimum(t_res, X), t_off)
    assert (exp > 100).sum() > 100
    got = api.ungapped_scores(gpu, M, gpu.seqset(q_res, q_off, q_cb), gpu.seqset(t_res, t_off, None))
    diff = np.argwhere(got != exp)
    assert len(diff) == 0, [(int(a), int(b), int(got[a, b]), int(exp[a, b])) for a, b in diff[:10]]
    # ... and the clean sets with X in those places give the same matrix
    clean = api.ungapped_scores(gpu, M, gpu.seqset(np.minimum(q_res, X), q_off, q_cb), gpu.seqset(np.minimum(t_res, X), t_off, None))
    assert np.array_equal(clean, got)
