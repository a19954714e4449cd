"""Constructed pairs at the boundary of sd_sw_set_narrow_final (sd_sw.hip: k_gate_word, NARROW_EXACT), shared by the CPU and GPU
tests and by tools/make_golden_narrow_final.py.

With the switch on, a pair whose byte score saturates is rerun on the wide kernels only when the narrow forward pass reports
1023, the value its row-coded column maximum saturates to: 1022 is the last score the narrow pass answers alone, 1023 (exact,
but not told apart from saturation) and 1024 (saturated) are the first two that are rerun.  Per set one query and three
targets with exactly these forward scores:
  nf32   a query of 300 rows: aligned narrow class a_seg10, wide rerun in w_rt10x32 (32 lanes per task)
  nf64   a query of 450 rows: aligned narrow class a_seg15, wide rerun in w_rt8x64 (64 lanes), start positions in the unshared
         rt8x64 (1022) and w_rt8x64 (1023, 1024)
A target is a flank of random letters, then the query with substitutions: a bulk at a fixed rate from the set's seed, then the
few of TUNE, found by search() with the oracle (a random descent that accepts a substitution while the score stays at or above
the wanted one); 1023 continues from 1024's target and 1022 from 1023's.  The reference's rows confirm the scores
(tests/golden/narrow_final.npz).  Everything is deterministic; the fixture holds the digest of the letters."""
import os
from collections import Counter

import numpy as np

import scgen
from tbgen import AA, _mutate, _rnd

WANT = (1024, 1023, 1022)          # (in the order of the descent)
FLANK = 17
# (name, query rows, seed, bulk substitution rate)
SETS = (('nf32', 300, 9100, 0.27), ('nf64', 450, 9200, 0.44))
# (set, score) -> the substitutions (position in the query, letter) on top of the previous target of the set
TUNE = {
    ('nf32', 1024): ((142, 'M'), (14, 'D'), (244, 'W'), (79, 'K'), (256, 'S'), (248, 'M'), (136, 'S'), (40, 'H'), (115, 'K'), (267, 'F'),
                     (22, 'G'), (149, 'L'), (38, 'Y'), (222, 'Y'), (30, 'R'), (89, 'M'), (274, 'G'), (215, 'E'), (98, 'Y'), (128, 'A'),
                     (173, 'M'), (272, 'A')),
    ('nf32', 1023): ((139, 'V'),),
    ('nf32', 1022): ((171, 'L'),),
    ('nf64', 1024): ((213, 'M'), (367, 'W'), (388, 'K'), (41, 'A'), (386, 'S'), (374, 'M'), (365, 'H'), (204, 'S'), (58, 'L'), (435, 'D'),
                     (173, 'K'), (403, 'F'), (225, 'G'), (12, 'S'), (224, 'L'), (335, 'Y'), (44, 'R'), (133, 'M'), (146, 'Y'), (164, 'P'),
                     (321, 'M'), (389, 'L'), (166, 'C'), (344, 'V'), (359, 'G'), (156, 'T'), (261, 'M'), (301, 'M'), (437, 'S'), (339, 'S'),
                     (249, 'T'), (162, 'E'), (215, 'C'), (299, 'V'), (276, 'G'), (377, 'T'), (399, 'E'), (251, 'I')),
    ('nf64', 1023): ((343, 'I'),),
    ('nf64', 1022): ((345, 'D'),),
}
DB_RESIDUES = 10 ** 7


def _base(name):
    (n, seed, rate), = [(n, s, r) for k, n, s, r in SETS if k == name]
    rng = np.random.default_rng(seed)
    qs = _rnd(rng, n)
    return qs, _rnd(rng, FLANK), _mutate(rng, qs, rate)


def build(tune=None):
    """(seqs, pairs): the sequences and [dict(name, q, t, want)] with q, t indices into seqs"""
    tune = TUNE if tune is None else tune
    seqs, pairs = [], []
    for name, _, _, _ in SETS:
        qs, flank, t = _base(name)
        seqs.append(qs)
        q = len(seqs) - 1
        t = list(t)
        for want in WANT:
            for p, c in tune[name, want]:
                t[p] = c
            seqs.append(flank + ''.join(t))
            pairs.append(dict(name='%s_%d' % (name, want), q=q, t=len(seqs) - 1, want=want))
    return seqs, pairs


def search(oracle, seed=1):
    """TUNE, found again: per target a random descent from the previous one"""
    out = {}
    for name, _, _, _ in SETS:
        qs, flank, t = _base(name)
        q = oracle.map_sequence(qs)
        score = lambda letters: oracle.sw_align(q, oracle.map_sequence(flank + ''.join(letters)), DB_RESIDUES, sw_mode=0)['score']
        rng = np.random.default_rng(seed)
        t = list(t)
        s = score(t)
        assert s >= WANT[0], (name, s, 'lower the bulk rate')
        for want in WANT:
            subs = []
            while s > want:
                p, c = int(rng.integers(4, len(t) - 4)), AA[int(rng.integers(20))]
                if c == t[p] or any(p == x for x, _ in subs):
                    continue
                old, t[p] = t[p], c
                s2 = score(t)
                if want <= s2 < s:
                    s = s2
                    subs.append((p, c))
                else:
                    t[p] = old
            out[name, want] = tuple(subs)
    return out


NARROW_EXACT = 1023


def forward(prof, t, go=11, ge=1):
    """(score, tEnd, qEnd) of the recurrence without any layout and without saturation: Hpre = max(h, E, 0), both gaps open from
    Hpre, G = max(Hpre, Ff); the largest G wins, then the first column, then the smallest row.  prof[a][q]: score of query row
    q against residue a.  A column at a time: Ff[q] = max over p < q of Hpre[p] - go - (q - 1 - p) ge is a running maximum of
    Hpre[p] + p ge.  Nothing scores: (0, -1, 0), as the records have it"""
    assert go >= ge
    prof = np.asarray(prof, np.int64)
    n = prof.shape[1]
    idx = np.arange(n, dtype=np.int64)
    G, E = np.zeros(n, np.int64), np.zeros(n, np.int64)
    best = (0, -1, 0)
    for col, a in enumerate(t):
        h = np.empty(n, np.int64)
        h[0] = 0
        h[1:] = G[:-1]
        hpre = np.maximum(np.maximum(h + prof[int(a)], E), 0)
        run = np.maximum.accumulate(hpre + idx * ge)
        ff = np.zeros(n, np.int64)
        ff[1:] = np.maximum(run[:-1] - go - (idx[1:] - 1) * ge, 0)
        G = np.maximum(hpre, ff)
        E = np.maximum(np.maximum(E - ge, hpre - go), 0)
        m = int(G.max())
        if m > best[0]:
            best = (m, col, int(np.argmax(G == m)))
    return best


def tasks_on(rows, x, mode, shared=True, pre_word=False):
    """scgen.Rows.tasks with sd_sw_set_narrow_final on: [(pass number, class, scope)] of pair x.  The rerun and the wide start
    classes are for the pairs the narrow pass reports at NARROW_EXACT (word := score >= 1023 in scgen.klass); pre_word: the
    pair's diagonal proves that much and the pair skips the forward pass"""
    n, tl = int(rows.qlen[x]), int(rows.tlen[x])
    r = rows.res[mode][x]
    wide = bool(rows.word[x]) and int(r[0]) >= NARROW_EXACT
    assert wide or not pre_word
    out = [] if pre_word else [(0, scgen.klass('fwd', n, shared, rows.wrl))]
    if wide:
        out.append((1, scgen.klass('word', n, shared, rows.wrl, tl=tl)))
    if mode >= 1 and r[1] >= 0:
        out.append((2, scgen.klass('start', int(r[2]) + 1, False, rows.wrl, word=wide, tl=int(r[4]) + 1)))
    return [(p, c, s) for p, (c, s) in out]


def launches_on(rows, idx, mode, shared=True):
    """Counter{scope: launches} of one call with the switch on: one launch per pass and non-empty class"""
    return Counter(s for _, _, s in set(tk for x in idx for tk in tasks_on(rows, x, mode, shared)))


def golden():
    """tests/golden/narrow_final.npz: the reference's rows for build() (tools/make_golden_narrow_final.py), in the layout of
    score_classes.npz (scgen.Rows reads both)"""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'narrow_final.npz'))
