"""Constructed pairs with a known band history for the banded traceback (sd_sw.hip), shared by the CPU and GPU tests and by
tools/make_golden_tb_classes.py, plus a restatement of which traceback task class a band reaches (tbKey / tbBandClass over TB_CLASSES).

Three random segments A, B, C and independent random inserts X, Y:
  doubling  q = A X B C, t = A B Y C, |X| = |Y| = g: a square rectangle (first band 1) whose optimal path leaves the main
            diagonal by g, so the band doubles until it is >= g.
  skew      the same with |X| - |Y| = d (or |Y| - |X| = d): first band d + 1, the path leaves the diagonal by max(|X|, d).
  boundary  q = A B, t = A Y B (and transposed), |Y| = D: one gap, first band D + 1, which already suffices.
  rowcap    near-identical pairs whose aligned query length is a narrow class's row cap c or c + 1; 'gap' ones with one insert.
  tcap      target lengths 1037 / 1038 next to the narrow classes' column cap.
  tie       diverged pairs (30 % substitutions, five indels) whose path walks a horizontal gap through a cell where opening
            and extending it score the same: sub-seeds kept because a restatement that compares dirF with >= instead of >
            gives another backtrace for them; four end in lds128, one in a narrow class.
Everything is deterministic from the seed."""
import os
from collections import Counter

import numpy as np

AA = 'ACDEFGHIKLMNPQRSTVWY'
NARROW_Q = (128, 192, 256, 320, 384, 512, 640, 768, 1024)
CLASSES = tuple('narrow%d' % c for c in NARROW_Q) + ('lds128', 'lds512', 'lds2048', 'global')

# (g, L, LB) of the doubling pairs, LB the length of B: A and C each outscore one gap (5 L > 10 + g), B outscores both
# (5 LB > 2 (10 + g)), and L + LB + L + g <= 1024 wherever the pair is to start in a narrow class
DOUBLING = ((0, 40, 40), (2, 60, 60), (4, 100, 100), (8, 120, 120), (9, 150, 150), (16, 200, 200), (17, 230, 230), (32, 300, 300),
            (33, 80, 80), (64, 100, 100), (65, 100, 100), (128, 100, 100), (129, 100, 100), (256, 120, 120), (512, 120, 230),
            (513, 120, 230), (1024, 250, 420), (1025, 250, 430))
# (|X|, |Y|, L): first bands 2, 3, 6, 11 (the narrow kernel's attempt groups 2-3, 4-7, 8-14), both orientations
SKEW = ((3, 2, 50), (8, 7, 90), (6, 4, 70), (12, 10, 110), (4, 6, 130), (10, 5, 60), (20, 15, 100), (15, 20, 180), (11, 1, 100),
        (14, 4, 150))
TIE_SEEDS = (30, 53, 105, 157, 340)
BOUNDARY = ((13, 100), (14, 100), (61, 100), (62, 100), (253, 120), (254, 120), (1021, 300), (1022, 300))


def _rnd(rng, n):
    return ''.join(AA[i] for i in rng.integers(0, 20, n))


def _mutate(rng, s, rate, keep=4):
    """substitutions only, the first and last `keep` residues stay (the alignment spans the pair end to end)"""
    s = list(s)
    for p in np.flatnonzero(rng.random(len(s)) < rate):
        if keep <= p < len(s) - keep:
            s[p] = AA[rng.integers(20)]
    return ''.join(s)


def _tie_pair(seed, n=260, net=16):
    rng = np.random.default_rng(seed)
    q = _rnd(rng, n)
    t = list(_mutate(rng, q, 0.3))
    for _ in range(4):
        p, k = int(rng.integers(20, len(t) - 20)), int(rng.integers(1, 6))
        if rng.random() < 0.5:
            del t[p:p + k]
        else:
            t[p:p] = list(_rnd(rng, k))
    p = int(rng.integers(40, len(t) - 40))
    t[p:p] = list(_rnd(rng, net))
    return q, ''.join(t)


def pairs(seed=20261018):
    """[dict(name, kind, q, t, dev)]: dev is the distance from the main diagonal that the optimal path reaches by construction"""
    rng = np.random.default_rng(seed)
    out = []
    for g, L, LB in DOUBLING:
        a, b, c, x, y = _rnd(rng, L), _rnd(rng, LB), _rnd(rng, L), _rnd(rng, g), _rnd(rng, g)
        out.append(dict(name='double_g%d' % g, kind='doubling', q=a + x + b + c, t=a + b + y + c, dev=g, gap=g))
    for nx, ny, L in SKEW:
        a, b, c, x, y = _rnd(rng, L), _rnd(rng, L), _rnd(rng, L), _rnd(rng, nx), _rnd(rng, ny)
        out.append(dict(name='skew_%d_%d' % (nx, ny), kind='skew', q=a + x + b + c, t=a + b + y + c, dev=max(nx, abs(nx - ny)), gap=(nx, ny)))
    for d, L in BOUNDARY:
        a, b, y = _rnd(rng, L), _rnd(rng, L), _rnd(rng, d)
        out.append(dict(name='bound_t%d' % d, kind='boundary', q=a + b, t=a + y + b, dev=d, gap=d))
        a, b, y = _rnd(rng, L), _rnd(rng, L), _rnd(rng, d)
        out.append(dict(name='bound_q%d' % d, kind='boundary', q=a + y + b, t=a + b, dev=d, gap=d))
    for x, c in enumerate(NARROW_Q):
        for n, gap in ((c, 0), (c + 1, 0), (c, 2 + x % 4)):
            q = _rnd(rng, n)
            t = _mutate(rng, q, 0.12)
            if gap:
                p = n // 3 + 7 * x
                t = t[:p] + _rnd(rng, gap) + t[p:]
            out.append(dict(name='rows_%d%s' % (n, '_gap%d' % gap if gap else ''), kind='rowcap', q=q, t=t, dev=gap, gap=gap))
    for nq, d in ((1024, 13), (1025, 13), (1024, 14)):
        a, b, y = _rnd(rng, 512), _rnd(rng, nq - 512), _rnd(rng, d)
        out.append(dict(name='tcap_%d_%d' % (nq, nq + d), kind='tcap', q=a + b, t=a + y + b, dev=d, gap=d))
    for sd in TIE_SEEDS:
        q, t = _tie_pair(sd)
        out.append(dict(name='tie_%d' % sd, kind='tie', q=q, t=t, dev=None, gap=None))
    return out


def runs(bt):
    """[(letter, length)] of a backtrace"""
    out = []
    for ch in bt:
        if out and out[-1][0] == ch:
            out[-1][1] += 1
        else:
            out.append([ch, 1])
    return [(a, n) for a, n in out]


def deviation(bt):
    """max |i - j| over the cells of the path: the smallest band that holds it ('I' consumes a query residue, 'D' a target one)"""
    d = dev = 0
    for ch in bt:
        d += (ch == 'I') - (ch == 'D')
        dev = max(dev, abs(d))
    return dev


def _narrow(band, q_len, t_len):
    return band * 2 + 3 <= 32 and q_len <= 1024 and t_len <= 1024 + 13


def _width_class(band):
    w = band * 2 + 3
    return 'lds128' if w <= 127 else 'lds512' if w <= 511 else 'lds2048' if w <= 2047 else 'global'


def history(q_len, t_len, dev, hostpath=False):
    """the traceback class of every launch that a task of q_len x t_len aligned residues takes part in, whose path needs a band
    of dev: the first band is |t_len - q_len| + 1, a band fails while it is < dev and doubles.  Device orchestration: one launch
    per round, the narrow kernel tries every band that fits 32 lanes, an LDS class every band up to its width, the global class
    one band per round.  Host orchestration: no narrow classes, one band per launch."""
    band = abs(t_len - q_len) + 1
    out = []
    while True:
        if hostpath:
            out.append(_width_class(band))
            if band >= dev:
                return tuple(out)
            band *= 2
            continue
        if _narrow(band, q_len, t_len):
            out.append('narrow%d' % min(c for c in NARROW_Q if q_len <= c))
            limit = 32
        else:
            out.append(_width_class(band))
            limit = {'lds128': 127, 'lds512': 511, 'lds2048': 2047, 'global': 0}[out[-1]]
        while True:
            if band >= dev:
                return tuple(out)
            band *= 2
            if band * 2 + 3 > limit:
                break


def final_band(q_len, t_len, dev):
    band = abs(t_len - q_len) + 1
    while band < dev:
        band *= 2
    return band


def compress_alignment(bt):
    """Matcher::compressAlignment (M/src/alignment/Matcher.cpp:166-185), letter by letter"""
    out, state, count = [], 'M', 0
    for ch in bt:
        if ch != state:
            out.append('%d%s' % (count, state))
            state, count = ch, 1
        else:
            count += 1
    out.append('%d%s' % (count, state))
    return ''.join(out)


def golden():
    """tests/golden/tb_classes.npz: the reference's records for pairs() (tools/make_golden_tb_classes.py)"""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tb_classes.npz'))


def golden_history(g, x, hostpath=False):
    """history() of the task that the reference's record of pair x describes"""
    r = g['res'][x]
    return history(int(r[2] - r[1] + 1), int(r[4] - r[3] + 1), deviation(str(g['bt'][x])), hostpath)


def groups(g, hostpath=False):
    """{history: [pair indices]}: the path groups, pairs that run through the same classes in the same rounds"""
    out = {}
    for x in range(len(g['name'])):
        out.setdefault(golden_history(g, x, hostpath), []).append(x)
    return out


def padded(idx, odd):
    """idx repeated up to an odd count of at least three, or up to an even count"""
    idx = list(idx)
    out = list(idx)
    while (len(out) % 2 == 0 or len(out) < 3) if odd else (len(out) % 2 == 1):
        out.append(idx[(len(out) - len(idx)) % len(idx)])
    return out


def shuffled(g, seed=3):
    """every pair once or twice in random order, with further copies so that every class starts its first round with an odd
    count of at least three tasks"""
    rng = np.random.default_rng(seed)
    n = len(g['name'])
    order = list(range(n)) + [int(x) for x in rng.choice(n, n // 2, replace=False)]
    first = [golden_history(g, x)[0] for x in range(n)]
    for c in CLASSES:
        have = sum(first[x] == c for x in order)
        members = [x for x in range(n) if first[x] == c]
        while have < 3 or have % 2 == 0:
            order.append(members[have % len(members)])
            have += 1
    return [order[i] for i in rng.permutation(len(order))]


def round_counts(g, order, hostpath=False):
    """Counter{(round, class): tasks} of one call with the pairs of `order` when nothing is deferred"""
    out = Counter()
    for x in order:
        for r, c in enumerate(golden_history(g, x, hostpath)):
            out[(r, c)] += 1
    return out
