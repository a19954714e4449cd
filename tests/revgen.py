"""Constructed pairs for sd_sw_set_shared_start (sd_sw.hip: k_gate_rev, k_pair_keys; sd_sw_pk.h: the start-row form of the
aligned kernel), shared by the CPU and the GPU test, plus a restatement of the routing the switch leaves.

With the switch on, the narrow start-position task of a pair whose query has 129 .. 768 rows scans rows j0 = qLen - 1 - qEnd ..
qLen - 1 of ONE profile of the whole reversed query: its chain begins in lane s = j0 // RT (RT = ceil(qLen / 32)), at row
j0 % RT of that lane.  Per class (RT = 5, 12 and 24) one query and targets that hold one exact segment of it, q[a .. e], so
that the forward pass ends at qEnd = e by construction (the flanks score badly against the query residues they face):
  e % RT = 0, 1, RT - 1     the chain begins at the first, second and last row of a lane
  e = qLen - 1              j0 = 0: nothing is masked
  e = 29                    j0 close to the end of the profile: the chain begins in one of the last lanes
  one column                the target is the single letter W: tEnd + 1 = 1
Flanks of 7 and 8 letters in front of the segment make tEnd + 1 odd and even.  Two periodic queries:
  per_RT12   M M with |M| = 190 against 40 residues of M (a whole M would saturate the byte score and leave the narrow
             classes): the forward pass ends in the first copy (same column, smaller row), mid-lane
  tan_RT24   P U U R against F U with |U| = 14 hot letters: the forward pass ends in the first U, and the second U lies in
             the rows just before j0 INSIDE the lane the chain begins in -- unmasked they would reach the task's score in the
             same column at a smaller row, so a kernel without the row mask reports another start
All gates are opened (E-value 1e9, coverage 0) so that every pair reaches the start-position pass, and the sequences are used
WITHOUT composition bias (a bias of zero in the sequence set, comp_bias=False in the oracle): the bias depends on the
neighbourhood of a residue and would break the ties of the periodic queries.  Everything is deterministic; expected records come from the oracle at test time."""
from collections import Counter

import numpy as np

import scgen
from tbgen import _rnd

CLASSES = ((5, 150), (12, 370), (24, 760))     # (RT, query rows)
SEG = 40                                       # residues of the copied segment (30 for e = 29)
DB_RESIDUES = 10 ** 7
EVAL_THR, COV_THR = 1e9, 0.0            # (a single W scores 11: an E-value of a few millions)
FIRST_START_CLASS = 42                         # the start form's classes follow the 24 + 14 + 4 of scgen.klass
PER_M, PER_CUT, TAN_U, TAN_P = 190, (110, 150), 14, 396


def _bad(q, first, k, step=1):
    """k letters that score badly against q[first], q[first + step], ...: no diagonal leads on past the segment"""
    return ''.join('P' if not 0 <= first + step * i < len(q) or q[first + step * i] != 'P' else 'G' for i in range(k))


def ends(rt, n):
    base = (n // 2 // rt) * rt
    return (('mod0', base), ('mod1', base + 1), ('modlast', base + rt - 1), ('whole', n - 1), ('late', 29))


def build(seed=20261101):
    """(seqs, pairs): the sequences and [dict(name, q, t, rt, e)] with q, t indices into seqs; e: the intended qEnd"""
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []

    def add(s):
        seqs.append(s)
        return len(seqs) - 1

    for rt, n in CLASSES:
        qs = list(_rnd(rng, n))
        qs[n // 2 + 3] = 'W'
        qs = ''.join(qs)
        q = add(qs)
        for k, (what, e) in enumerate(ends(rt, n)):
            a = max(0, e + 1 - (SEG if e > 29 else 30))
            t = _bad(qs, a - 1, 7 + (k & 1), -1)[::-1] + qs[a:e + 1] + _bad(qs, e + 1, 5 + 3 * k)
            pairs.append(dict(name='%s_RT%d' % (what, rt), q=q, t=add(t), rt=rt, e=e))
        pairs.append(dict(name='onecol_RT%d' % rt, q=q, t=add('W'), rt=rt, e=None))
    m = _rnd(rng, PER_M)
    pairs.append(dict(name='per_RT12', q=add(m + m), t=add(m[PER_CUT[0]:PER_CUT[1]]), rt=12, e=PER_CUT[1] - 1))
    u = scgen._hot(rng, TAN_U)
    n = CLASSES[2][1]
    qs = _rnd(rng, TAN_P - 1) + 'P' + u + u + 'P' + _rnd(rng, n - TAN_P - 2 * TAN_U - 1)   # (G against P and the hot letters: negative)
    pairs.append(dict(name='tan_RT24', q=add(qs), t=add('G' * 9 + u + 'G' * 7), rt=24, e=TAN_P + TAN_U - 1))
    return seqs, pairs


def start_row(prof_rev_whole, rt, j0, t_rev, go=11, ge=1, mask=True, zero=True):
    """The start-row scheme, lane by lane as the kernel lays it out but without its number formats: (score, column, row) of the
    task that begins at row j0 of the profile of the whole reversed query (prof_rev_whole[a][row]).  Lane s = j0 // rt takes
    nothing from lane s - 1 (zero), its rows before j0 score -64 against everything (mask), lanes before s are left out of the
    maximum, the row is reported from j0.  The largest G wins, then the first column, then the smallest row."""
    prof = np.asarray(prof_rev_whole, np.int64)
    n = prof.shape[1]
    s = j0 // rt
    first = s * rt if zero else 0                 # without the hand-off zero the chain comes down from row 0
    sub = prof[:, first:].copy()
    if mask:
        sub[:, :j0 - first] = -64
    rows = n - first
    G, E = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    idx = np.arange(rows, dtype=np.int64)
    best = (0, -1, 0)
    for col, a in enumerate(t_rev):
        h = np.empty(rows, np.int64)
        h[0] = 0
        h[1:] = G[:-1]
        hpre = np.maximum(np.maximum(h + sub[int(a)], E), 0)
        run = np.maximum.accumulate(hpre + idx * ge)
        ff = np.zeros(rows, np.int64)
        ff[1:] = np.maximum(run[:-1] - go - (idx[1:] - 1) * ge, 0)
        G = np.maximum(hpre, ff)
        E = np.maximum(np.maximum(E - ge, hpre - go), 0)
        seen = G[s * rt - first:]                 # the lanes from s on
        m = int(seen.max())
        if m > best[0]:
            best = (m, col, int(np.argmax(seen == m)) + s * rt - j0)
    return best


def start_klass(qlen, n, tl, wrl, wide, packed=True, shared_queries=True):
    """(class, scope) of a start-position task with the switch on: the start form for a narrow task of a query of 129 .. 768
    rows and up to 65 535 columns when tasks are paired by query, scgen.klass's 'start' for every other task"""
    if packed and shared_queries and not wide and 129 <= qlen <= 768 and tl <= 65535:
        rt = (qlen + 31) // 32
        return FIRST_START_CLASS + rt - 5, 'sw_score_pk.s_seg%d' % rt
    return scgen.klass('start', n, False, wrl, packed, word=wide, tl=tl)


def tasks_on(rows, x, mode, narrow_final=False, shared=True, shared_start=True):
    """[(pass number, class, scope)] of pair x of a scgen.Rows-like table with sd_sw_set_shared_start on (narrow_final: and
    sd_sw_set_narrow_final, whose word pairs below 1023 stay narrow; shared_start=False: the routing without the switch)"""
    n, tl = int(rows.qlen[x]), int(rows.tlen[x])
    r = rows.res[mode][x]
    wide = bool(rows.word[x]) and (not narrow_final or int(r[0]) >= 1023)
    out = [(0, scgen.klass('fwd', n, shared, rows.wrl))]
    if wide:
        out.append((1, scgen.klass('word', n, shared, rows.wrl, tl=tl)))
    if mode >= 1 and r[1] >= 0:
        out.append((2, start_klass(n, int(r[2]) + 1, int(r[4]) + 1, rows.wrl, wide, shared_queries=shared and shared_start)))
    return [(p, c, s) for p, (c, s) in out]


def launches_on(rows, idx, mode, narrow_final=False, shared=True, shared_start=True):
    """Counter{scope: launches} of one call with the switch on: one launch per pass and non-empty class"""
    return Counter(s for _, _, s in set(tk for x in idx for tk in tasks_on(rows, x, mode, narrow_final, shared, shared_start)))


def in_range(rows, x, mode, narrow_final=False):
    """pair x has a start-position task that the switch moves to the start form"""
    return any(p == 2 and s.startswith('sw_score_pk.s_seg') for p, _, s in tasks_on(rows, x, mode, narrow_final))
