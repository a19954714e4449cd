"""A plain float64 restatement of result2profile's weights stage (global position-based weights, then per column
the weights of the sub-alignment of the rows that have a residue there, its number of effective sequences, the column's weighted
residue frequencies).  Written from the description, not from the kernel: every change column is recomputed from scratch (no
running counts, no compaction, no tiles), shares are exact quotients and every sum runs in float64.  Only the DECISIONS are taken as
the code takes them, in float32: the end-gap limit 0.1f * participating and the > 1e-10 gate of an entropy term.  flog2 / fpow2
are the same polynomials evaluated in float64 -- they define the operation.

Cells: uint8 [nRows, L], row 0 the centre; 0..19 residue, 20 any residue (X), 21 gap.

Besides freq / eff, column_weights returns the facts the tests assert their input conditions on: the change columns and, per
change column, nActive, width, jmin, jmax, the rows that start / end a residue run there and the end-gap counts around the window."""
import numpy as np

ANY, GAP, ENDGAP, CODES = 20, 21, 22, 23
MIN_COLUMNS = 20
F32_1E8 = float(np.float32(1e-8))
F32_1E6 = float(np.float32(1e-6))


def flog2(x):
    """MathUtil::flog2's form: exponent + a degree-5 polynomial in (mantissa - 1)"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(np.where(x > 0, x, 1.0))   # x = m * 2^e, m in [0.5, 1)
    d = 2.0 * m - 1.0
    return np.where(x > 0, d * (1.441740 + d * (-0.7077702 + d * (0.4123442 + d * (-0.1903190 + d * 0.0440047)))) + (e - 1), -128.0)


def fpow2(x):
    """MathUtil::fpow2's form: 2^round(x - 0.5) times a degree-4 polynomial in the rest"""
    if x >= 128:
        return float(np.finfo(np.float32).max)
    if x <= -125:
        return 0.0
    lx = float(np.rint(x - 0.5))
    dx = x - lx
    return (1.0 + dx * (0.693019 + dx * (0.241404 + dx * (0.0520749 + dx * 0.0134929)))) * 2.0 ** lx


def global_weights(cells):
    """Henikoff position-based weights with the length prior: a residue shared by c of the rows in a column of d distinct
    residues gives each of them 1 / (c * d * (non-gap cells of the row + 30)); scaled to sum 1"""
    n, L = cells.shape
    w = np.full(n, F32_1E6, np.float64)
    row_cells = (cells != GAP).sum(axis=1).astype(np.float64)
    for i in range(L):
        col = cells[:, i]
        res = col < ANY
        seen = np.bincount(col[res], minlength=20)
        d = int((seen != 0).sum())
        if d == 0:
            continue
        w[res] += 1.0 / (seen[col[res]].astype(np.float64) * d * (row_cells[res] + 30.0))
    total = w.sum()
    return w / total if total != 0 else w


def with_end_gaps(cells):
    """gaps before a row's first / behind its last non-gap cell become end gaps (code 22)"""
    c = cells.copy()
    n, L = c.shape
    for r in range(n):
        nz = np.nonzero(c[r] != GAP)[0]
        if len(nz) == 0:
            c[r, :] = ENDGAP
        else:
            c[r, :nz[0]] = ENDGAP
            c[r, nz[-1] + 1:] = ENDGAP
    return c


def change_columns(cells):
    """the columns where a row starts or ends a residue run"""
    res = np.asarray(cells) < ANY
    before = np.concatenate([np.zeros((len(res), 1), bool), res[:, :-1]], axis=1)
    return [int(i) for i in np.nonzero((res != before).any(axis=0))[0]]


def column_weights(cells, background, jmax_shift=0):
    """-> freq float64 [L, 20], eff float64 [L], facts.  jmax_shift moves the window's last column at every change column whose
    window has at least MIN_COLUMNS columns (only to show what one column of the window is worth, tests/test_r2p_restatement.py)"""
    cells = np.asarray(cells, np.uint8)
    n, L = cells.shape
    gw = global_weights(cells)
    c = with_end_gaps(cells).astype(np.int64)
    res = c < ANY
    cols = np.arange(L)
    freq = np.zeros((L, 20), np.float64)
    eff = np.zeros(L, np.float64)
    local = np.zeros(n, np.float64)
    facts = dict(change=[], nActive={}, width={}, jmin={}, jmax={}, starts={}, ends={}, edge={})
    for i in range(L):
        here = res[:, i]
        before = res[:, i - 1] if i else np.zeros(n, bool)
        starts, ends = np.nonzero(here & ~before)[0], np.nonzero(before & ~here)[0]
        if len(starts) or len(ends):
            act = np.nonzero(here)[0]
            participating = len(act)
            sub_cells = c[act]                                         # the sub-alignment: [participating, L]
            flat = (cols[None, :] * CODES + sub_cells).ravel()
            count = np.bincount(flat, minlength=L * CODES).reshape(L, CODES)
            limit = np.float32(0.1) * np.float32(participating)        # float32, as the code decides it
            passing = np.nonzero(~(count[:, ENDGAP].astype(np.float32) > limit))[0]
            jmin, jmax = (int(passing[0]), int(passing[-1])) if len(passing) else (L, -1)
            eg = count[:, ENDGAP]
            facts['edge'][i] = (int(eg[jmin - 1]) if 0 < jmin <= L else -1, int(eg[jmin]) if jmin < L else -1,
                                int(eg[jmax]) if jmax >= 0 else -1, int(eg[jmax + 1]) if -1 <= jmax < L - 1 else -1)
            if jmax - jmin + 1 >= MIN_COLUMNS:
                jmax = min(L - 1, jmax + jmax_shift)
            width = jmax - jmin + 1
            if width < MIN_COLUMNS:
                local = np.where(here, gw, 0.0)
            else:
                distinct = (count[:, :ANY] != 0).sum(axis=1)
                share = np.zeros((L, CODES), np.float64)
                nz = count[:, :ANY] != 0
                share[:, :ANY][nz] = 1.0 / (distinct[:, None] * count[:, :ANY])[nz].astype(np.float64)
                local = np.full(n, F32_1E8, np.float64)
                w = slice(jmin, jmax + 1)
                local[act] += share[cols[w][None, :], sub_cells[:, w]].sum(axis=1)
            e = 0.0
            if width > 0:
                w = slice(jmin, jmax + 1)
                nw = jmax + 1 - jmin
                flat = (np.arange(nw)[None, :] * CODES + sub_cells[:, w]).ravel()
                sub = np.bincount(flat, weights=np.repeat(local[act], nw), minlength=nw * CODES).reshape(nw, CODES)[:, :ANY]
                total = sub.sum(axis=1)
                sub = np.where(total[:, None] != 0, sub / np.where(total == 0, 1.0, total)[:, None], sub)
                v = sub[sub.astype(np.float32).astype(np.float64) > 1e-10]   # the gate, on the float32 value
                e = -float((v * flog2(v)).sum())
            eff[i] = fpow2(e / width) if width > 0 else 1.0
            facts['change'].append(i)
            facts['nActive'][i], facts['width'][i], facts['jmin'][i], facts['jmax'][i] = participating, width, jmin, jmax
            facts['starts'][i], facts['ends'][i] = starts, ends
        else:
            eff[i] = 0.0 if i == 0 else eff[i - 1]
        f = np.bincount(c[here, i], weights=local[here], minlength=20)[:20]
        total = f.sum()
        freq[i] = f / total if total != 0 else background
    return freq, eff, facts


_RESTATED = {}


def restated():
    """(case name, index) -> (cells, freq, eff, facts) for every task of tests/r2pgen.py, computed once per process"""
    if not _RESTATED:
        import r2pgen
        from spacedust_amd.api import Host
        background = Host().matrix(0)[1][:20].copy()
        for name, k, cells in r2pgen.all_tasks():
            _RESTATED[(name, k)] = (cells,) + column_weights(cells, background)
    return _RESTATED
