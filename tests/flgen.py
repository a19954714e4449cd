"""The packed Smith-Waterman score kernels without the lane-structure F chain (Fl): a scalar model of their recurrence with
and without Fl, and the constructed "F-then-E" pairs that tests/test_sw_fl_equivalence.py (CPU, against the model and the
oracle) and tests/test_gpu_sw_fl.py (GPU, through Context.sw_align) share.

Recurrence of one column (sd_sw_pk.h; every subtraction saturates at 0), rows q = 0 .. n-1:
    h     = max(0, G[c-1][q-1] + P[t_c][q])
    Hpre  = max(h, E[q], Fl)         Fl: vertical gap opened inside the same SIMD segment (reset where q % segLen == 0)
    G     = max(Hpre, Ff)            Ff: the exact vertical gap
    open  = Hpre - go
    E[q]  = max(E[q] - ge, open),  Fl' = max(Fl - ge, open),  Ff' = max(Ff - ge, open)
Without Fl, Hpre = max(h, E[q]).  The claim under test: G is the same in every cell for go >= ge.
"""
import numpy as np

GAPS = [(11, 1), (5, 1), (3, 3), (2, 1), (4, 2), (1, 1), (7, 3)]
AA = 'ACDEFGHIKLMNPQRSTVWY'


def model(prof, t, go, ge, seg_len=None):
    """the recurrence cell by cell in Python integers.  prof[a][q]: score of query row q against residue a; seg_len None: no
    Fl.  Returns (G, Hpre, E) as int arrays [len(t)][n], E being the value a cell leaves for the next column."""
    prof = [[int(v) for v in row] for row in np.asarray(prof)]
    n = len(prof[0])
    H, E = [0] * n, [0] * n
    Gs, Hs, Es = [], [], []
    for a in t:
        p = prof[int(a)]
        Hn, Hp = [0] * n, [0] * n
        fl = ff = 0
        for q in range(n):
            if seg_len is not None and q % seg_len == 0:
                fl = 0
            h = (H[q - 1] if q else 0) + p[q]
            if h < 0:
                h = 0
            hpre = max(h, E[q], fl) if seg_len is not None else max(h, E[q])
            Hp[q] = hpre
            Hn[q] = max(hpre, ff)
            op = max(hpre - go, 0)
            E[q] = max(E[q] - ge, op)
            fl = max(fl - ge, op)
            ff = max(ff - ge, op)
        H = Hn
        Gs.append(Hn)
        Hs.append(Hp)
        Es.append(list(E))
    return np.array(Gs, np.int64), np.array(Hs, np.int64), np.array(Es, np.int64)


def model_np(prof, t, go, ge, seg_len=None):
    """the same three matrices with a column at a time in numpy, for the long pairs.  A chain F' = max(F - ge, open) started at
    0 is F[q] = max(0, max over p < q of open[p] - (q-1-p) ge), a running maximum of Hpre[p] + p ge; inside a segment the
    Fl chain is the running maximum of max(h, E)[p] + p ge, because a gap opened from an Fl value never beats the extended one
    while go >= ge.  test_sw_fl_equivalence checks this form against model() cell by cell on every small pair."""
    assert go >= ge
    prof = np.asarray(prof, np.int64)
    n = prof.shape[1]
    idx = np.arange(n, dtype=np.int64)
    H, E = np.zeros(n, np.int64), np.zeros(n, np.int64)
    Gs, Hs, Es = [], [], []
    NEG = -(1 << 40)

    def chain(src, width):   # F[q] of rows grouped in segments of `width` rows
        pad = (-n) % width
        a = np.concatenate([src + idx * ge, np.full(pad, NEG, np.int64)]).reshape(-1, width)
        cm = np.maximum.accumulate(a, axis=1)
        f = np.full_like(a, NEG)
        f[:, 1:] = cm[:, :-1]
        f = f.reshape(-1)[:n] - go - (idx - 1) * ge
        return np.maximum(f, 0)

    for a in t:
        h = np.maximum(np.concatenate([[0], H[:-1]]) + prof[int(a)], 0)
        hpre = np.maximum(h, E)
        if seg_len is not None:
            hpre = np.maximum(hpre, chain(hpre, seg_len))
        H = np.maximum(hpre, chain(hpre, n))
        E = np.maximum(np.maximum(E - ge, hpre - go), 0)
        Gs.append(H)
        Hs.append(hpre)
        Es.append(E)
    return np.array(Gs), np.array(Hs), np.array(Es)


def best(G):
    """(score, target end, query end) the way every score pass reports them: the first column that reaches the maximum, the
    smallest row inside it; (0, 0, n - 1) when nothing scores"""
    mx = int(G.max()) if G.size else 0
    if mx == 0:
        return 0, 0, G.shape[1] - 1
    col = int(np.argmax(G.max(axis=1) == mx))
    return mx, col, int(np.argmax(G[col] == mx))


def random_pair(rng, alphabet, n_min=5, n_max=80):
    """a random query and a target derived from it by substitutions, insertions and deletions"""
    q = rng.integers(0, alphabet, int(rng.integers(n_min, n_max + 1)))
    t = []
    for r in q:
        u = rng.random()
        if u < 0.08:
            continue
        if u < 0.16:
            t.extend(rng.integers(0, alphabet, int(rng.integers(1, 6))))
        t.append(int(rng.integers(0, alphabet)) if rng.random() < 0.25 else int(r))
    if not t:
        t = [0]
    return q.astype(np.uint8), np.array(t, np.uint8)


def random_matrix(rng, alphabet):
    """a symmetric substitution matrix with a positive diagonal and mostly negative rest"""
    m = rng.integers(-4, 2, (alphabet, alphabet))
    m = np.minimum(m, m.T)
    m[np.arange(alphabet), np.arange(alphabet)] = rng.integers(3, 9, alphabet)
    return m.astype(np.int64)


def fte_letters(rng, n, gap_row, k, ms, core, related):
    """a query of n residues and one target per entry of ms: identical around query row gap_row, where the query carries k
    residues the target lacks and the target, at the same place, m residues the query lacks -- a vertical gap followed at once
    by a horizontal one.  `related`: the pair is identical over its whole length apart from that; otherwise only `core`
    residues on either side of the gaps are shared and the rest of the two sequences is unrelated."""
    pick = lambda letters, c: ''.join(letters[int(x)] for x in rng.integers(0, len(letters), c))
    left, right = pick(AA, gap_row), pick(AA, n - gap_row - k)
    targets = []
    for m in ms:
        tl, tr = left, right
        if not related:
            tl = pick(AA, max(0, gap_row - core)) + left[max(0, gap_row - core):]
            tr = right[:core] + pick(AA, max(0, len(right) - core))
        targets.append(tl + pick('GPD', m) + tr)   # (the inserted residues of the two sides score badly against each other)
    return left + pick('WCF', k) + right, targets


# name, query rows, query row of the first inserted residue, k, m of every target, shared residues per side, related, what for
FTE_SPECS = [
    ('rt4x32', 100, 49, 2, (3,), 16, False, 'general kernel, <= 128 rows (segments of 4 rows)'),
    ('rt4x32_full', 128, 65, 2, (1, 2), 16, False, 'general kernel, a full 128 rows, two targets'),
    ('a_seg10', 300, 151, 6, (3, 5), 16, False, 'aligned kernel, forward shared; start positions on the aligned kernel unshared'),
    ('a_seg19', 600, 457, 9, (4, 2), 16, False, 'aligned kernel of 19 rows per lane; start positions on the 64-lane kernel'),
    ('strips2', 800, 509, 8, (3,), 16, False, 'two strips of 512 rows: the vertical gap covers rows 509 .. 516'),
    ('strips3', 1200, 1021, 5, (3, 1), 16, False, 'three strips: the vertical gap covers rows 1021 .. 1025'),
    ('wide7', 220, 113, 6, (3,), 0, True, 'score beyond the byte range: word rerun on the wide kernel'),
    ('wide64', 450, 225, 10, (4, 2), 0, True, 'wide kernel of 64 lanes'),
    ('wide_strips', 800, 509, 8, (3,), 0, True, 'wide kernel, two strips, the vertical gap across row 512'),
]


def fte_pairs():
    """(sequences as letters, [(name, index of the query, index of the target)]) of FTE_SPECS"""
    rng = np.random.default_rng(20260)
    seqs, pairs = [], []
    for name, n, gap_row, k, ms, core, related, _ in FTE_SPECS:
        q, targets = fte_letters(rng, n, gap_row, k, ms, core, related)
        seqs.append(q)
        for x, t in enumerate(targets):
            seqs.append(t)
            pairs.append(('%s/%d' % (name, x), len(seqs) - 2 - x, len(seqs) - 1))
    return seqs, pairs


def fte_small(rng, alphabet):
    """a small F-then-E pair in numbers for the scalar model: identical sides of 12 .. 20 residues around the two gaps"""
    side = int(rng.integers(12, 21))
    k, m = int(rng.integers(1, 6)), int(rng.integers(1, 6))
    left, right = rng.integers(0, alphabet, side), rng.integers(0, alphabet, side)
    x, y = rng.integers(0, alphabet, k), rng.integers(0, alphabet, m)
    return np.concatenate([left, x, right]).astype(np.uint8), np.concatenate([left, y, right]).astype(np.uint8), side, k
