"""Constructed pairs for the Smith-Waterman score passes (sd_sw.hip: the SCORE_CLASSES table, scoreClassOf / devRunScore; sd_sw_pk.h), shared by the CPU and
GPU tests and by tools/make_golden_score_classes.py, plus a restatement of the class table: which kernel instantiation and
which profile scope a task of a pass runs in.

One query per length on both sides of every row limit of the forward table (128 | 129, every multiple of 32 up to 768 | 769,
1024 | 1025, 1536 | 1537), one interior length per class (n % 32 = 19), one of five strips.  Per query
  hom      a homolog (12 % substitutions) over the whole query whose byte score saturates: rerun in the wide class of the same
           rows, start positions in the unshared wide class.  q = A X B C, t = A' B' Y C': X is a run of query residues against
           a gap of 2 ceil(n / 16) + 1 rows (through two whole lanes of the rerun's 16 segments, the more so of the 32 of the
           byte pass), Y a run of 41 target residues against a gap (more than a 32-column chunk of the residue fetch)
  core     the last 24 query residues at the end of a target of random letters: the byte score stays below saturation, the
           packed narrow result is final, and qEnd + 1 is the query length exactly (the target ends with the core), so the
           start-position task lands in the unshared narrow class of the same rows.  At the interior lengths ('coregap') the
           core is c1 X c2 in the query and c1 c2 in the target, X a run of 2 ceil(n / 32) + 1 rows against a gap
  unrel    a random target; the target lengths run through 1, 5, 31, 32, 33, 63, 64, 65 (fewer columns than lanes) and 1100
  frag     (every fourth length) the last 63 / 64 / 65 query residues as the target: saturates with few columns
  tie      (every eighth length) a second random target of the length of the first
and beside them
  tail_*   queries P + unrelated tail with a core / a homolog of P that ends where P ends: qEnd + 1 = |P| on both sides of the
           limits of the unshared table (128 | 129, 384 | 385, 512 | 513, 640 | 641, 768 | 769), narrow and wide, in a forward
           class of more rows
  lastseg  the run against a gap ends in the last used segment, one per kernel family
  cov_*    pairs that stop at the coverage gate (qEnd + 1 < 0.8 |q|), below saturation and above
  wrl_*    the wideRowLimit switch: a saturating 2348 x 2348 pair (int32 kernel) and 2348 x 300 (stays in the wide class), and
           a target whose composition bias reaches 3, the largest any residue in any neighbourhood reaches, which puts the
           limit at 32767 / (11 + 3) = 2340 rows: no pair of at most 2300 residues can cross it
  edge_*   byte score + bias is 255 exactly (the first that saturates) and 254 (the last that does not)
  tie_rows a query of period 7 against nine / three periods: the maximum stands in every seventh row of the last column, the
           reference reports the first (row 85, and row 92 is in the same 12-row lane of the wide kernel; rows 43 and 50 in
           neighbouring lanes of the narrow one)
Everything is deterministic from the seed; the letters are reproduced from the code, the fixture holds their digest."""
import hashlib
import os
from collections import Counter

import numpy as np

from tbgen import AA, _mutate, _rnd, padded, runs  # noqa: F401  (padded, runs: used by the tests through this module)

ROW_LIMITS = tuple(range(128, 769, 32)) + (1024, 1536)
LENGTHS = tuple(sorted([c + d for c in ROW_LIMITS for d in (0, 1)] + [33, 77, 900, 1300, 2100] + [32 * rt - 13 for rt in range(5, 25)]))
INTERIOR = frozenset([77, 900, 1300, 2100] + [32 * rt - 13 for rt in range(5, 25)])
CORE_T = (31, 32, 33, 63, 64, 65, 150, 1100)
UNREL_T = (1, 5, 31, 32, 33, 63, 64, 65, 300, 1100)
TAIL_ROWS = (128, 129, 384, 385, 512, 513, 640, 641, 768, 769)
# (name, rows, lanes, saturating): the crossing at the last used segment of the narrow (32 segments) and the wide (16) form
LASTSEG = (('rt4x32', 128, 32, False), ('aligned', 760, 32, False), ('multi', 928, 32, False), ('w_rt4x32', 128, 16, True),
           ('w_32lane', 380, 16, True), ('w_64lane', 600, 16, True), ('w_multi', 900, 16, True))
WRL_LEN = 2348
# (byte score + bias, sub-seed, core length): found by a search with the oracle, the reference's rows confirm them
EDGE = ((255, 7000, 42), (254, 7010, 48))
PERIOD = 'WCHYFPM'
PROFILE_TWINS = ('hom_77', 'core_77', 'hom_307', 'core_307', 'hom_499', 'core_499', 'hom_900', 'core_900')
MODES = (0, 1, 2)
FIELDS = ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'identical', 'btLen')

PK_NAMES = ('rt4x32', 'rt6x32', 'rt7x32', 'rt8x32', 'rt9x32', 'rt10x32', 'rt11x32', 'rt12x32', 'rt8x64', 'rt10x64', 'rt12x64',
            'rt8x64s2', 'rt8x64s3', 'rt8x64sN')
I32_NAMES = ('rt4', 'rt8', 'rt16', 'rt32')


def klass(pass_, n, shared, wide_row_limit, packed=True, word=False, tl=65535):
    """(task class, profile scope) of a score task of n rows and tl columns (scoreClassOf and the scopes of SCORE_CLASSES in sd_sw.hip; written by hand, never derived from that table).  pass_: 'fwd' (the
    forward byte pass), 'word' (the rerun of a saturated pair with the word structure) or 'start' (start positions: of a
    rerun pair when word is set).  shared: tasks paired by query (forward and rerun passes of a query set below 2^17
    sequences).  packed: False when the int32 kernel is forced or the gap costs demand it.  The unshared classes of 385 .. 768
    rows keep their class of 32 rows each and run on three kernels: several classes, one launch each, in one scope."""
    assert pass_ in ('fwd', 'word', 'start') and n >= 1 and tl >= 1
    wide = pass_ == 'word' or (pass_ == 'start' and word)
    if pass_ == 'start':
        shared = False
    if not packed or tl > 65535 or (wide and min(n, tl) > wide_row_limit):
        ci = 0 if n <= 128 else 1 if n <= 256 else 2 if n <= 512 else 3
        return 38 + ci, 'sw_score.' + I32_NAMES[ci]
    strips = min((n + 511) // 512, 4)
    if wide:
        if n <= 192:
            ci = 0 if n <= 128 else 1
        elif n <= 384:
            ci = 2 + (n - 193) // 32
        elif n <= 768:
            ci = 8 if n <= 512 else 9 if n <= 640 else 10
        else:
            ci = 11 + strips - 2
        return 24 + ci, 'sw_score_pk.w_' + PK_NAMES[ci]
    if n <= 128:
        return 0, 'sw_score_pk.rt4x32'
    if n > 768:
        return 21 + strips - 2, 'sw_score_pk.' + PK_NAMES[11 + strips - 2]
    rt = (n + 31) // 32
    if shared or rt <= 12:
        return rt - 4, 'sw_score_pk.a_seg%d' % rt
    return rt - 4, 'sw_score_pk.' + ('rt8x64' if rt <= 16 else 'rt10x64' if rt <= 20 else 'rt12x64')


def scope(*args, **kw):
    return klass(*args, **kw)[1]


def instantiation(scope_name, shared):
    """(kernel template instance, shared): the three strip scopes of a form are one instantiation, the int32 kernel has no
    shared form"""
    k = scope_name.split('.', 1)[1]
    if scope_name.startswith('sw_score.'):
        return 'i32_' + k, False
    for s in ('s2', 's3', 'sN'):
        if k.endswith('x64' + s):
            k = k[:-2] + 'multi'
    return k, bool(shared)


def instantiations():
    """the 63 kernels that the SCORE_CLASSES table of sd_sw.hip instantiates"""
    out = [('a_seg%d' % rt, True) for rt in range(5, 25)] + [('a_seg%d' % rt, False) for rt in range(5, 13)]
    out += [('rt4x32', True), ('rt4x32', False), ('rt8x64', False), ('rt10x64', False), ('rt12x64', False), ('rt8x64multi', True),
            ('rt8x64multi', False)]
    out += [('w_' + k, s) for k in PK_NAMES[:11] + ('rt8x64multi',) for s in (True, False)]
    out += [('i32_' + k, False) for k in I32_NAMES]
    assert len(out) == len(set(out)) == 63
    return out


def _hot(rng, n):
    """letters with a large score against themselves"""
    return ''.join('WCHYFPM'[i] for i in rng.integers(0, 7, n))


def _hom(rng, q, lanes=16):
    """q = A X B C against A' B' Y C' (see the module text); plain substitutions where the parts would be under 20 residues"""
    n = len(q)
    g = 2 * ((n + lanes - 1) // lanes) + 1
    part = (n - g) // 3
    if part < 20:
        return _mutate(rng, q, 0.12), None
    a, b, c = q[:part], q[part + g:2 * part + g], q[2 * part + g:]
    return _mutate(rng, a, 0.12) + _mutate(rng, b, 0.12) + _rnd(rng, 41) + _mutate(rng, c, 0.12), (part, g)


def _core_len(cost):
    return max(16, int(np.ceil((cost + 20) / 5.2)))


def build(seed=20261019):
    """(seqs, pairs): the sequences and [dict(name, kind, q, t, sat, rows, igap, dgap, gate)] with q, t indices into seqs.
    sat: the byte score is meant to saturate (None: whatever happens); rows: the intended qEnd + 1; igap = (first row, length,
    lanes) of the run of query residues against a gap, dgap the length of the run of target residues against one; gate: the
    gate the pair is meant to stop at"""
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []

    def add(s):
        seqs.append(s)
        return len(seqs) - 1

    def pair(name, kind, q, t, sat=None, rows=None, igap=None, dgap=None, gate=None):
        pairs.append(dict(name=name, kind=kind, q=q, t=t, sat=sat, rows=rows, igap=igap, dgap=dgap, gate=gate))

    for x, n in enumerate(LENGTHS):
        qs = _rnd(rng, n)
        q = add(qs)
        t, gap = _hom(rng, qs)
        pair('hom_%d' % n, 'hom', q, add(t), sat=True if n >= 60 else None, rows=n, igap=gap + (16,) if gap else None, dgap=41 if gap else None)
        want = CORE_T[x % len(CORE_T)]
        if n in INTERIOR and n >= 77:
            g = 2 * ((n + 31) // 32) + 1
            k = _core_len(10 + g)
            core = qs[n - 2 * k - g:n - k - g] + qs[n - k:]
            pair('core_%d' % n, 'coregap', q, add(_rnd(rng, max(0, want - 2 * k)) + core), sat=False, rows=n, igap=(n - k - g, g, 32))
        else:
            k = min(24, n)
            pair('core_%d' % n, 'core', q, add(_rnd(rng, max(0, want - k)) + qs[n - k:]), sat=False, rows=n)
        tl = UNREL_T[x % len(UNREL_T)]
        pair('unrel_%d' % n, 'unrel', q, add(_rnd(rng, tl)))
        if x % 4 == 0 and n >= 80:
            pair('frag_%d' % n, 'frag', q, add(qs[n - (63, 64, 65)[(x // 4) % 3]:]), sat=True, rows=n)
        if x % 8 == 4:
            pair('tie_%d' % n, 'unrel', q, add(_rnd(rng, tl)))
    for n in TAIL_ROWS:
        p = _rnd(rng, n)
        q = add(p + _rnd(rng, n // 8))
        pair('tail_core_%d' % n, 'tail_core', q, add(_rnd(rng, 40) + p[n - 24:]), sat=False, rows=n)
        pair('tail_hom_%d' % n, 'tail_hom', q, add(_mutate(rng, p, 0.12)), sat=True, rows=n)
    for name, n, lanes, sat in LASTSEG:
        seg = (n + lanes - 1) // lanes
        k2 = n - ((n + seg - 1) // seg - 1) * seg - 1
        g = 2 * seg + 1
        c2 = _hot(rng, k2) if k2 < 12 else _rnd(rng, k2)
        if sat:
            a = _rnd(rng, n - g - k2)
            q = add(a + _rnd(rng, g) + c2)
            pair('lastseg_' + name, 'lastseg', q, add(_mutate(rng, a, 0.12) + c2), sat=True, rows=n, igap=(n - g - k2, g, lanes))
        else:
            k1 = _core_len(10 + g)
            c1 = _rnd(rng, k1)
            q = add(_rnd(rng, n - k1 - g - k2) + c1 + _rnd(rng, g) + c2)
            pair('lastseg_' + name, 'lastseg', q, add(_rnd(rng, 50) + c1 + c2), sat=False, rows=n, igap=(n - g - k2, g, lanes))
    qs = _rnd(rng, 300)
    q = add(qs)
    pair('cov_core', 'gate', q, add(_rnd(rng, 60) + qs[40:64] + _rnd(rng, 30)), sat=False, gate='coverage')
    pair('cov_hom', 'gate', q, add(qs[20:120]), sat=True, gate='coverage')
    pair('cov_late', 'gate', q, add(_rnd(rng, 20) + qs[200:230] + _rnd(rng, 200)), sat=False, gate='coverage')
    for k in range(3):
        pair('evalue_%d' % k, 'gate', q, add(_rnd(rng, (40, 300, 700)[k])), gate='evalue')
    qs = _rnd(rng, WRL_LEN)
    q = add(qs)
    pair('wrl_square', 'wrl', q, add(_mutate(rng, qs, 0.12)), sat=True, rows=WRL_LEN)
    pair('wrl_flat', 'wrl', q, add(qs[WRL_LEN - 300:]), sat=True, rows=WRL_LEN)
    pair('wrl_bias3', 'unrel', q, add('G' * 30 + 'L' + 'G' * 30))
    for want, sub_seed, k in EDGE:
        r2 = np.random.default_rng(sub_seed)
        qs, flank = _rnd(r2, 200), _rnd(r2, 30)
        pair('edge_%d' % want, 'edge', add(qs), add(flank + qs[200 - k:]), sat=want >= 255, rows=200)
    q = add(PERIOD[-2:] + PERIOD * 54)
    pair('tie_rows_w', 'tie_rows', q, add(PERIOD * 9), sat=True, rows=86)
    pair('tie_rows_n', 'tie_rows', q, add(PERIOD * 3), sat=False, rows=44)
    return seqs, pairs


def digest(seqs):
    return hashlib.sha256('\n'.join(seqs).encode()).hexdigest()


def profile_record(seq_num, mat, seed):
    """the query as a profile: its own matrix rows (in the record's quarter units) plus noise of up to one unit, 25 bytes per
    position (the recipe of test_profile_queries_double_their_band without its factor 5 / 4, so that the twin keeps its classes)"""
    m = np.array([mat[i] for i in range(441)], np.int32).reshape(21, 21)
    rng = np.random.default_rng(seed)
    rows = m[np.minimum(seq_num.astype(np.int64), 19), :20] * 4 + rng.integers(-4, 5, (len(seq_num), 20))
    rec = np.zeros((len(seq_num), 25), np.uint8)
    rec[:, :20] = np.clip(rows, -128, 127).astype(np.int8).view(np.uint8)
    rec[:, 20] = seq_num
    rec[:, 21] = np.argmax(rows, axis=1)
    return rec.tobytes()


def golden():
    """tests/golden/score_classes.npz: the reference's rows for build() (tools/make_golden_score_classes.py)"""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'score_classes.npz'))


class Rows:
    """the golden rows of the plain pairs (prefix '') or of the profile twins (prefix 'p_') with what the class table needs"""

    def __init__(self, g, prefix=''):
        self.res = g[prefix + 'res']              # [mode, pair, FIELDS]
        self.evalue = g[prefix + 'evalue']        # [mode, pair]
        self.word = g[prefix + 'word']
        self.bt = str(g[prefix + 'bt']).split('\n')
        self.bt_nocov = str(g[prefix + 'bt_nocov']).split('\n')   # (mode 2 without the coverage gate: the path of every pair)
        self.start_nocov = g[prefix + 'start_nocov']
        self.qlen, self.tlen = g[prefix + 'qlen'], g[prefix + 'tlen']
        self.wrl = int(g[prefix + 'wide_row_limit'])
        self.n = len(self.word)

    def tasks(self, x, mode, shared=True, packed=True):
        """[(pass number, class, scope, instantiation)] of pair x in a call of alignment mode `mode`, from the reference's row: the
        forward byte pass, the rerun when the byte score saturated, the start-position pass when the row has start positions"""
        n, tl = int(self.qlen[x]), int(self.tlen[x])
        r = self.res[mode][x]
        word = bool(self.word[x])
        out = [(0, klass('fwd', n, shared, self.wrl, packed), shared)]
        if word:
            out.append((1, klass('word', n, shared, self.wrl, packed, tl=tl), shared))
        if mode >= 1 and r[1] >= 0:
            out.append((2, klass('start', int(r[2]) + 1, False, self.wrl, packed, word=word, tl=int(r[4]) + 1), False))
        return [(p, c, s, instantiation(s, sh)) for p, (c, s), sh in out]

    def launches(self, idx, mode, shared=True, packed=True):
        """Counter{scope: launches} of one call on the pairs idx: one launch per pass and non-empty class"""
        seen = set((p, c, s) for x in idx for p, c, s, _ in self.tasks(x, mode, shared, packed))
        return Counter(s for _, _, s in seen)

    def groups(self, mode, shared=True, packed=True):
        """{classes: [pairs]}: the pairs that share their class in every pass"""
        out = {}
        for x in range(self.n):
            out.setdefault(tuple((p, c, s) for p, c, s, _ in self.tasks(x, mode, shared, packed)), []).append(x)
        return out


def shuffled(n, seed=5):
    return [int(x) for x in np.random.default_rng(seed).permutation(n)]


def gap_runs(bt, q_start):
    """[(letter, first query row, length)] of the gap runs of a backtrace ('I' consumes a query residue, 'D' a target one)"""
    out, row = [], q_start
    for a, k in runs(bt):
        if a != 'M':
            out.append((a, row, k))
        if a != 'D':
            row += k
    return out
