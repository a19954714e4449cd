"""Yardsticks of the exhaustive ungapped prefilter (`ungappedprefilter`, `search --prefilter-mode 1`):

  * a plain numpy restatement of SmithWaterman::ungapped_alignment (M/src/alignment/StripedSmithWaterman.cpp:1722-1781)
        S(i, j) = max(0, min(255 - bias, S(i-1, j-1) + M[t_j][q_i] + cb_i)),  score = max S
    with bias = |min M| + |min(0, min cb)| as ssw_init sets it;
  * the list rule of runFilterOnCpu with alignment mode 0 (M/src/prefiltering/ungappedprefilter.cpp:338-477);
  * RefUngapped: the reference's own function, reached in oracle/_ref/libsdref.so (present only where the reference tree was
    built) through the handle ref_sw_create returns -- its second pointer is the SmithWaterman object.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ungapped_vectors.npz')
REF_LIB = os.path.join(ROOT, 'oracle', '_ref', 'libsdref.so')
ALPHABET = 'ACDEFGHIKLMNPQRSTVWYX'   # Sequence::mapSequence's numeric alphabet (X = 20)


def bias_of(M, cb):
    """ssw_init's bias: |min M| + |min(0, min cb)|"""
    lo = int(np.min(cb)) if cb is not None and len(cb) else 0
    return abs(int(np.min(M))) + abs(min(lo, 0))


def restate_score(M, q, t, cb=None):
    """score of one pair: M [21, 21] ints, q / t numeric residues, cb the query's int8 composition bias (None: zero)"""
    M = np.asarray(M, np.int32).reshape(21, 21)
    q = np.asarray(q, np.int64)
    cbi = np.zeros(len(q), np.int32) if cb is None else np.asarray(cb, np.int32)
    cap = 255 - bias_of(M, cbi)
    S = np.zeros(len(q) + 1, np.int32)
    best = 0
    for tj in np.asarray(t, np.int64):
        S[1:] = np.clip(S[:-1] + M[tj, q] + cbi, 0, cap)
        best = max(best, int(S.max()))
    return best


def restate_matrix(M, q_res, q_off, q_cb, t_res, t_off):
    """scores of every query against every target, [nQ, nT] (one pass per query over all targets at once)"""
    M = np.asarray(M, np.int16).reshape(21, 21)
    nq, nt = len(q_off) - 1, len(t_off) - 1
    t_len = (np.asarray(t_off[1:], np.int64) - np.asarray(t_off[:-1], np.int64))
    lmax = int(t_len.max()) if nt else 0
    T = np.full((nt, lmax), 21, np.int64)   # 21: past the target's end
    for x in range(nt):
        T[x, :t_len[x]] = t_res[int(t_off[x]):int(t_off[x + 1])]
    out = np.zeros((nq, nt), np.int32)
    for x in range(nq):
        q = np.asarray(q_res[int(q_off[x]):int(q_off[x + 1])], np.int64)
        cb = np.zeros(len(q), np.int16) if q_cb is None else np.asarray(q_cb[int(q_off[x]):int(q_off[x + 1])], np.int16)
        cap = 255 - bias_of(M, cb)
        prof = np.full((22, len(q)), -1000, np.int16)
        prof[:21] = M[:, q] + cb
        S = np.zeros((nt, len(q) + 1), np.int16)
        best = np.zeros(nt, np.int16)
        for j in range(lmax):
            S[:, 1:] = np.clip(S[:, :-1] + prof[T[:, j]], 0, cap)
            np.maximum(best, S.max(axis=1), out=best)
        out[x] = best
    return out


def can_be_covered(cov_thr, cov_mode, q_len, t_len):
    """Util::canBeCovered (M/src/commons/Util.cpp:477-494), float arithmetic"""
    c, q, t = np.float32(cov_thr), np.float32(q_len), np.float32(t_len)
    with np.errstate(divide='ignore', invalid='ignore'):   # (a zero length: inf or nan, as in the reference)
        return _can_be_covered(c, cov_mode, q, t)


def _can_be_covered(c, cov_mode, q, t):
    if cov_mode == 0:
        return bool(q / t >= c and t / q >= c)
    if cov_mode == 1:
        return bool(q / t >= c)
    if cov_mode == 2:
        return bool(t / q >= c)
    if cov_mode == 3:
        return bool(t / q >= c and t / q <= np.float32(1.0))
    if cov_mode == 4:
        return bool(q / t >= c and q / t <= np.float32(1.0))
    if cov_mode == 5:
        return bool(min(t, q) / max(t, q) >= c)
    return True


def list_rule(scores, t_keys, q_len, t_lens, min_score=15, max_seqs=300, cov_mode=0, cov_thr=0.0, identity_key=None):
    """the hits of one query as [(target key, score)]: canBeCovered, score > min_score or identity, order by score descending
    then key ascending (hit_t::compareHitsByScoreAndId), cut to max_seqs"""
    hits = []
    for s, k, tl in zip(scores, t_keys, t_lens):
        if not can_be_covered(cov_thr, cov_mode, q_len, tl):
            continue
        if int(s) > min_score or (identity_key is not None and int(k) == int(identity_key)):
            hits.append((int(k), int(s)))
    hits.sort(key=lambda h: (-h[1], h[0]))
    return hits[:max_seqs]


def expand_pooled(small, pool_id):
    """scores against targets drawn from a pool: with target t = pool[pool_id[t]], the scores of queries x targets are the
    columns pool_id of `small` = restate_matrix(queries x pool) ([nQ, nPool] -> [nQ, nT]; one row [nPool] -> [nT])"""
    return np.asarray(small)[..., np.asarray(pool_id, np.int64)]


def covered_mask(cov_thr, cov_mode, q_len, t_lens):
    """can_be_covered for one query against every target at once, in float32 as the reference computes it (a zero length
    divides to inf or nan; a comparison with nan is false)"""
    c, q = np.float32(cov_thr), np.float32(q_len)
    t = np.asarray(t_lens).astype(np.float32)
    one = np.float32(1.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        if cov_mode == 0:
            return (q / t >= c) & (t / q >= c)
        if cov_mode == 1:
            return q / t >= c
        if cov_mode == 2:
            return t / q >= c
        if cov_mode == 3:
            return (t / q >= c) & (t / q <= one)
        if cov_mode == 4:
            return (q / t >= c) & (q / t <= one)
        if cov_mode == 5:
            return np.minimum(t, q) / np.maximum(t, q) >= c
    return np.ones(len(t), bool)


def list_rule_fast(scores_row, keys, q_len, t_lens, min_score=15, max_seqs=300, cov_mode=0, cov_thr=0.0, identity_key=None):
    """list_rule for rows of 10^6 targets: the same hits in the same order, as (keys uint32 [n], scores int32 [n]).  The order
    (score descending, key ascending) is the ascending order of the composite (255 - score) << 32 | key; np.partition finds
    the max_seqs smallest, a sort orders that head only.  The keys are unique wherever an identity key is given."""
    s = np.asarray(scores_row).astype(np.int64)
    k = np.asarray(keys).astype(np.uint64)
    assert len(s) == len(k) == len(t_lens) and (len(s) == 0 or (0 <= s.min() and s.max() <= 255 and k.max() < (1 << 32)))
    keep = s > min_score
    if identity_key is not None:
        keep |= k == np.uint64(identity_key)
    keep &= covered_mask(cov_thr, cov_mode, q_len, t_lens)
    comp = ((255 - s[keep]).astype(np.uint64) << np.uint64(32)) | k[keep]
    if len(comp) > max_seqs:
        comp = np.partition(comp, max_seqs - 1)[:max_seqs]
    comp.sort()
    return (comp & np.uint64(0xFFFFFFFF)).astype(np.uint32), (255 - (comp >> np.uint64(32)).astype(np.int64)).astype(np.int32)


def list_text(hits):
    """QueryMatcher::prefilterHitToBuffer with diagonal 0"""
    return ''.join('%d\t%d\t0\n' % h for h in hits)


def have_ref():
    return os.path.exists(REF_LIB)


class RefUngapped:
    """SmithWaterman::ungapped_alignment of the reference, query set up by ssw_init exactly as the module does"""
    SYMBOL = '_ZN13SmithWaterman18ungapped_alignmentEPKhi'

    def __init__(self, comp_bias, max_len=70000):
        import sys
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        from oracle import pyoracle as po
        self.ref = po.Ref()
        self.sw = po.RefSW(self.ref, max_len, 10 ** 7, comp_bias=comp_bias)
        self.obj = C.c_void_p.from_address(self.sw.h + 8).value
        self.fn = getattr(self.ref.lib, self.SYMBOL)
        self.fn.restype = C.c_int
        self.fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]

    def set_query(self, q_num):
        self.sw.set_query(''.join(ALPHABET[int(x)] for x in q_num))

    def score(self, t_num):
        t = np.ascontiguousarray(t_num, np.uint8)
        return int(self.fn(self.obj, t.ctypes.data, len(t)))
