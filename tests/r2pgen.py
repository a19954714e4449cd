"""The constructed alignments behind tests/test_r2p_restatement.py (CPU) and tests/test_gpu_r2p_weights.py: cell matrices
(uint8 [nRows, L]; 0..19 residue, 20 any residue, 21 gap; row 0 the centre) built directly, so that the columns where rows start
and end -- and with them the change columns, the number of active rows and the window jmin..jmax of r2p_column_weights_kernel --
are what a case says they are.  A row is a residue run [start, end) over random residues, optionally with inner gaps and X from
column `inner_from` on (an inner gap or X ends the run at its column and starts another behind it: two more change columns).
Seeded; cases() builds every case once.  tests/test_r2p_restatement.py asserts each case's declared shape from the restatement's
facts (tests/r2p_ref.py)."""
import functools

import numpy as np

ANY, GAP = 20, 21
NT, ACT, LDSCOLS = 512, 768, 320   # R2P_NT, R2P_ACT, the kernel's LDSCOLS

ROW_PASS_ROWS = (1, 2, 63, 64, 65, 511, 512, 513, 1024, 1025)
COLUMN_CLASS_L = (1, 19, 20, 21, 35, 36, 37, 319, 320, 321, 511, 512, 513, 639, 640, 641, 961)
ACTIVE_COUNTS = (767, 768, 769, 775, 776, 777, 783, 784, 785, 1537)
TIE_PARTICIPATING = (10, 20, 30, 640)


def rows_from_runs(rng, L, runs, inner=0.0, inner_from=0, similar=0.7):
    """rows with residues in [start, end); residues follow a random consensus with probability `similar` (so that columns have
    between one and a few distinct residues and counts above one); `inner`: rate of inner gaps and (a third of it) X"""
    n = len(runs)
    cons = rng.integers(0, 20, L)
    m = np.full((n, L), GAP, np.uint8)
    for r, (a, b) in enumerate(runs):
        row = np.where(rng.random(L) < similar, cons, rng.integers(0, 20, L))
        if inner > 0:
            u = rng.random(L)
            ok = np.arange(L) >= inner_from
            ok[:a + 1] = False
            ok[max(b - 1, 0):] = False
            row = np.where(ok & (u < inner), GAP, row)
            row = np.where(ok & (u >= inner) & (u < inner * 4 / 3), ANY, row)
        m[r, a:b] = row[a:b]
    return m


def ragged(rng, L, n, inner=0.01, full=0.6):
    """the general alignment: the centre and a share `full` of the rows span every column, the others start in the first and end
    in the last quarter (never at column 0: at column 0 only whole rows are active, so its window is all L columns)"""
    runs = [(0, L)]
    for _ in range(n - 1):
        if rng.random() < full or L < 8:
            runs.append((0, L))
        else:
            runs.append((int(rng.integers(1, L // 4 + 1)), int(rng.integers(L - L // 4, L + 1))))
    return rows_from_runs(rng, L, runs, inner=inner, inner_from=1)


def row_pass_case(rng, n):
    """L = 48.  At 513 / 1 025 rows: every row (the centre too, behind two X) starts at column 2 -- more than 512 rows start at
    once --, and rows of the second (and third) pass of 512 end at column 40"""
    L = 48
    if n in (513, 1025):
        runs = [(2, L)] * n
        m = rows_from_runs(rng, L, runs, inner=0.004, inner_from=8)
        m[0, :2] = ANY
        for r in ([512] if n == 513 else list(range(600, 700)) + [1024]):
            m[r, 40:] = GAP
            m[r, 39] = rng.integers(0, 20)
        return m
    return ragged(rng, L, n, inner=0.01)


def active_case(rng):
    """1 537 rows, L = 64, nested: 767 rows start at column 0, then 1, 1, 6, 1, 1, 6, 1, 1 and 752 more at columns 1..9; all end
    with the alignment.  Inner gaps from column 16 on add change columns with a few rows fewer than 1 537"""
    add = (767, 1, 1, 6, 1, 1, 6, 1, 1, 752)
    runs = [(c, 64) for c, k in enumerate(add) for _ in range(k)]
    assert len(runs) == 1537
    return rows_from_runs(rng, 64, runs, inner=0.0005, inner_from=16)


def window_case(rng, a, b, n_inner=8, n_full=2, L=48):
    """n_full rows over every column and n_inner rows over [a, b): at column a the window is exactly [a, b)"""
    return rows_from_runs(rng, L, [(0, L)] * n_full + [(a, b)] * n_inner)


def narrowest_case(rng):
    """a window of one column: at column 7 nine rows with that single residue join one whole row -- every other column has nine
    end gaps among ten participating rows.  (A window of NO column cannot be built: see DESIGN 4.6)"""
    return rows_from_runs(rng, 30, [(0, 30)] + [(7, 8)] * 9)


def tie_case(rng, P):
    """P rows take part at column 2: P - P/10 - 1 span [0, 48), one [1, 47), P/10 [2, 46).  Columns 1 and 46 have exactly P/10 end
    gaps (the tie: inside the window), columns 0 and 47 one more (outside)"""
    t = P // 10
    return rows_from_runs(rng, 48, [(0, 48)] * (P - t - 1) + [(1, 47)] + [(2, 46)] * t)


def degenerate_case(rng):
    """L = 40: a centre with X at columns 0 and 13, an all-gap row, an all-X row, a row with one residue, and column 20 with only
    X and gaps below the centre; column 0 changes nothing (eff 0, background frequencies)"""
    L = 40
    m = rows_from_runs(rng, L, [(0, L)] + [(1, L)] * 4 + [(3, 33)] * 4 + [(0, 0), (0, 0), (17, 18)], inner=0.02, inner_from=4)
    m[0, 0] = m[0, 13] = ANY
    m[10, :] = ANY
    m[1:, 20] = np.where(np.arange(1, 12) % 2 == 0, ANY, GAP)
    m[0, 20] = 5
    return m


def identical_case(rng):
    """50 rows identical to the centre: one distinct residue per column, count x distinct = nRows"""
    return np.repeat(rng.integers(0, 20, (1, 33)).astype(np.uint8), 50, axis=0)


def unchanged_case(rng):
    """no inner gaps: the only change columns are the five where rows start or end"""
    return rows_from_runs(rng, 70, [(0, 70)] * 6 + [(9, 61)] * 3 + [(30, 70)] * 2)


EXTRA_SHAPES = ((37, 65), (321, 63), (77, 513), (129, 130), (23, 3), (325, 129), (45, 257), (19, 70), (21, 1), (333, 2), (99, 190))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> list of cell matrices (the tasks of one call)"""
    rng = np.random.default_rng(20240611)
    out = {}
    for n in ROW_PASS_ROWS:
        out['rows_%d' % n] = [row_pass_case(rng, n)]
    out['active_1537'] = [active_case(rng)]
    for L in COLUMN_CLASS_L:
        out['cols_%d' % L] = [ragged(rng, L, 40, inner=0.01 if L < 400 else 0.003)]
    out['width_19'] = [window_case(rng, 10, 29)]
    out['width_20'] = [window_case(rng, 10, 30)]
    out['width_1'] = [narrowest_case(rng)]
    for P in TIE_PARTICIPATING:
        out['tie_%d' % P] = [tie_case(rng, P)]
    out['degenerate'] = [degenerate_case(rng), identical_case(rng), unchanged_case(rng)]
    pool = [t for ts in out.values() for t in ts] + [ragged(rng, L, n, inner=0.01) for L, n in EXTRA_SHAPES]
    pick = rng.permutation(len(pool))[:48]
    out['mixed_48'] = [pool[k] for k in pick]
    return out


def all_tasks():
    """[(case name, index in the case, cells)] over every case but the mixed batch (whose tasks are among them)"""
    return [(name, k, t) for name, ts in cases().items() if name != 'mixed_48' for k, t in enumerate(ts)]
