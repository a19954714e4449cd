"""Yardsticks of the rescoring on the diagonal (`rescorediagonal`, `search --alignment-mode 4`): a plain-Python restatement of

  * DistanceCalculator::computeUngappedAlignment -> ungappedAlignmentByDiagonal (M/src/alignment/DistanceCalculator.h:94-201,276-295),
    the candidate diagonals of a 16-bit diagonal included;
  * the identity count and the row logic of doRescorediagonal (M/src/alignment/rescorediagonal.cpp:194-363).

Three forms of the per-diagonal rule, which the CPU tests hold against each other: `seq_rule` (the reference's loop, statement by
statement: the authority), `fast_rule` (numpy, one diagonal) and `rescore_batch` (numpy, many short hits at once).
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rescore_diag_vectors.npz')
ALPHABET = 'ACDEFGHIKLMNPQRSTVWYX'   # Sequence::mapSequence's numeric alphabet (X = 20)
DEFAULT = (0, -1, -1, 0, 0, 0)       # LocalAlignment(): score, startPos, endPos, diagonalLen, distToDiagonal, diagonal
FIELDS = ('score', 'startPos', 'endPos', 'diagonalLen', 'distToDiagonal', 'diagonal')


def aa2num():
    """letter -> matrix code (SubstitutionMatrix::setupLetterMapping, SubstitutionMatrix.cpp:257-298): case folded, J = L, Z = E,
    B = D, U / O and everything unknown = X"""
    t = np.full(256, 20, np.uint8)
    alias = {'J': 'L', 'Z': 'E', 'B': 'D', 'U': 'X', 'O': 'X'}
    for c in range(256):
        up = chr(c).upper() if c < 128 else '?'
        up = alias.get(up, up)
        if up in ALPHABET:
            t[c] = ALPHABET.index(up)
    return t


A2N = aa2num()


def as_bytes(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), np.uint8)


def candidates(d16, q_len, t_len):
    """the diagonals computeUngappedAlignment tries for the unsigned short d16, in its order"""
    d16 = int(d16) & 0xFFFF
    out = [d16 - 65536 * k for k in range(1, 1 + t_len // 32768 + 1)]
    out += [d16 + 65536 * k for k in range(0, q_len // 65536 + 1)]
    return out


def overlap(q_len, t_len, diag):
    """(query start, target start, length) of a diagonal, or None where it passes beside the sequences"""
    dist = abs(diag)
    if diag >= 0 and dist < q_len:
        return dist, 0, min(t_len, q_len - dist)
    if diag < 0 and dist < t_len:
        return 0, dist, min(t_len - dist, q_len)
    return None


def seq_rule(c):
    """computeSubstitutionStartEndDistance over the scores c: (maxScore, maxStartPos, maxEndPos)"""
    max_score = max_end = max_start = 0
    min_pos = -1
    score = 0
    for pos, cur in enumerate(c):
        score = int(cur) + score
        if score <= 0:
            score = 0
            min_pos = pos
        if score > max_score:
            max_end = pos
            max_start = min_pos + 1
            max_score = score
    return max_score, max_start, max_end


def fast_rule(c):
    """seq_rule as a scan: s = P - running min of P (P[-1] = 0); the earliest maximum; behind the latest minimum before it"""
    c = np.asarray(c, np.int64)
    if len(c) == 0:
        return 0, 0, 0
    pext = np.concatenate([[0], np.cumsum(c)])
    run = np.minimum.accumulate(pext)
    s = (pext - run)[1:]
    best = int(s.max())
    if best <= 0:
        return 0, 0, 0
    end = int(np.argmax(s))
    start = int(np.nonzero(pext[:end + 2] == run[end + 1])[0][-1])
    return best, start, end


def by_diagonal(M, q, t, diag, mode, rule=fast_rule):
    """ungappedAlignmentByDiagonal: the six LocalAlignment fields, or None where the diagonal contributes nothing"""
    ov = overlap(len(q), len(t), diag)
    if ov is None:
        return None
    qs, ts, n = ov
    a, b = q[qs:qs + n], t[ts:ts + n]
    if mode == 0:
        return int((a == b).sum()), -1, -1, n, abs(diag), diag
    sc, st, en = rule(M[A2N[a], A2N[b]])
    if mode == 1:
        return sc, -1, -1, n, abs(diag), diag
    return sc, st, en, n, abs(diag), diag


def compute(M, q, t, d16, mode, rule=fast_rule):
    """computeUngappedAlignment + the identity count of rescorediagonal.cpp:284-291: the six fields and idCnt (mode 2: letters of
    [startPos, endPos] equal without their case bit; mode 0: the score; mode 1: 0)"""
    M = np.asarray(M, np.int64).reshape(21, 21)
    q, t = as_bytes(q), as_bytes(t)
    best = DEFAULT
    for diag in candidates(d16, len(q), len(t)):
        r = by_diagonal(M, q, t, diag, mode, rule)
        if r is not None and r[0] > best[0]:
            best = r
    id_cnt = best[0] if mode == 0 else 0
    if mode == 2 and best[0] > 0:
        qs, ts, _ = overlap(len(q), len(t), best[5])
        a = q[qs + best[1]:qs + best[2] + 1] & 0xDF
        b = t[ts + best[1]:ts + best[2] + 1] & 0xDF
        id_cnt = int((a == b).sum())
    return best + (id_cnt,)


def rescore_batch(M, q_seqs, t_seqs, hit_q, hit_t, hit_d, mode, rows=4096):
    """compute() for many hits over SHORT sequences at once (padded rows): an int64 array [n, 7]"""
    M = np.asarray(M, np.int64).reshape(21, 21)

    def pack(seqs):
        arr = [as_bytes(s) for s in seqs]
        off = np.zeros(len(arr) + 1, np.int64)
        np.cumsum([len(a) for a in arr], out=off[1:])
        return np.concatenate(arr + [np.zeros(1, np.uint8)]), off

    qb, qo = pack(q_seqs)
    tb, to = pack(t_seqs)
    hit_q, hit_t = np.asarray(hit_q, np.int64), np.asarray(hit_t, np.int64)
    d16 = np.asarray(hit_d, np.int64) & 0xFFFF
    ql, tl = (qo[1:] - qo[:-1])[hit_q], (to[1:] - to[:-1])[hit_t]
    assert ql.max() < 32768 and tl.max() < 32768
    n = len(hit_q)
    out = np.zeros((n, 7), np.int64)
    out[:, 1:3] = -1
    by_len = np.argsort(np.minimum(ql, tl), kind='stable')   # rows of similar length share a chunk: little padding
    for r0 in range(0, n, rows):
        sel = by_len[r0:r0 + rows]
        lmax = int(np.minimum(ql, tl)[sel].max())
        pos = np.arange(lmax, dtype=np.int64)[None, :]
        k = np.arange(lmax + 1, dtype=np.int64)[None, :]
        cur = out[sel]
        for diag in (d16[sel] - 65536, d16[sel]):   # the candidates of sequences below 32 768 residues, in order
            dist = np.abs(diag)
            fwd = (diag >= 0) & (dist < ql[sel])
            bwd = (diag < 0) & (dist < tl[sel])
            ln = np.where(fwd, np.minimum(tl[sel], ql[sel] - dist), np.where(bwd, np.minimum(tl[sel] - dist, ql[sel]), 0))
            qs, ts = np.where(fwd, dist, 0), np.where(bwd, dist, 0)
            mask = pos < ln[:, None]
            a = qb[np.minimum((qo[hit_q[sel]] + qs)[:, None] + pos, len(qb) - 1)]
            b = tb[np.minimum((to[hit_t[sel]] + ts)[:, None] + pos, len(tb) - 1)]
            st = np.full(len(sel), -1, np.int64)
            en = st.copy()
            if mode == 0:
                sc = ((a == b) & mask).sum(axis=1)
            else:
                c = np.where(mask, M[A2N[a], A2N[b]], 0)
                pext = np.concatenate([np.zeros((len(sel), 1), np.int64), np.cumsum(c, axis=1)], axis=1)
                run = np.minimum.accumulate(pext, axis=1)
                s = np.where(mask, (pext - run)[:, 1:], -1)
                sc = np.maximum(s.max(axis=1), 0) if lmax else np.zeros(len(sel), np.int64)
                if mode == 2 and lmax:
                    en = np.argmax(s, axis=1)
                    eq = (pext == run[np.arange(len(sel)), en + 1][:, None]) & (k <= (en + 1)[:, None])
                    st = lmax - np.argmax(eq[:, ::-1], axis=1)
            win = sc > cur[:, 0]
            rec = np.stack([sc, st, en, ln, dist, diag], axis=1)
            cur[win, :6] = rec[win]
            if mode == 2:
                inside = mask & (pos >= st[:, None]) & (pos <= en[:, None])
                cur[win, 6] = (((a & 0xDF) == (b & 0xDF)) & inside).sum(axis=1)[win]
        out[sel] = cur
    if mode == 0:
        out[:, 6] = out[:, 0]
    return out


# ---- the row logic of doRescorediagonal ----------------------------------------------------------------------------------------

def can_be_covered(cov_thr, cov_mode, q_len, t_len):
    """Util::canBeCovered (M/src/commons/Util.cpp:477-494), float arithmetic"""
    c, q, t = np.float32(cov_thr), np.float32(q_len), np.float32(t_len)
    with np.errstate(divide='ignore', invalid='ignore'):
        if cov_mode == 0:
            return bool(q / t >= c and t / q >= c)
        if cov_mode == 1:
            return bool(q / t >= c)
        if cov_mode == 2:
            return bool(t / q >= c)
        if cov_mode == 3:
            return bool(q / t >= c and q / t <= 1.0)
        if cov_mode == 4:
            return bool(t / q >= c and t / q <= 1.0)
        if cov_mode == 5:
            return bool(min(t, q) / max(t, q) >= c)
    return True


def has_coverage(cov_thr, cov_mode, q_cov, t_cov):
    """Util::hasCoverage (Util.cpp:496-511)"""
    c = np.float32(cov_thr)
    if cov_mode == 0:
        return bool(q_cov >= c and t_cov >= c)
    if cov_mode == 1:
        return bool(q_cov >= c)
    if cov_mode == 2:
        return bool(t_cov >= c)
    return True


def compute_cov(start, end, length):
    """SmithWaterman::computeCov (StripedSmithWaterman.cpp:1671-1673): unsigned arithmetic, float division"""
    u = lambda v: int(v) & 0xFFFFFFFF
    s, e, n = u(start), u(end), u(length)
    return np.float32(u(min(n, max(s, e)) - min(s, e) + 1)) / np.float32(n)


def seq_id(mode, ids, q_len, t_len, aln_len):
    """Util::computeSeqId (Util.cpp:532-542)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        den = {1: min(q_len, t_len), 2: max(q_len, t_len)}.get(mode, aln_len)
        return np.float32(ids) / np.float32(den)


def seq_id_text(v):
    """Util::fastSeqIdToBuffer as the alignment DB shows it: truncation, "1.00" for an identity of one"""
    v = np.float32(v)
    if v == 1.0:
        return '1.00'
    s = '0.'
    if v < 0.10:
        s += '0'
    if v < 0.01:
        s += '0'
    return s + str(int(v * np.float32(1000)))


def rows(M, q, t_of_key, q_key, pref_rows, evalue, bitscore, mode=2, e=0.001, c=0.0, cov_mode=0, a=False, min_seq_id=0.0,
         min_aln_len=0, seq_id_mode=0, same_db=True, add_self=False, sort=False, fields=None):
    """the entry doRescorediagonal writes for one query: q its letters, pref_rows [(target key, score, diagonal)],
    t_of_key(key) the target's letters; evalue(score, qLen) / bitscore(score) the E-value computation; fields (optional): per
    row the seven values compute() gives, from elsewhere (the reference's own, or rescore_batch's).  Returns the text."""
    q = as_bytes(q)
    aln, short = [], []
    for x, (key, _, diag) in enumerate(pref_rows):
        t = as_bytes(t_of_key(key))
        identity = key == q_key and (add_self or same_db)
        if not can_be_covered(c, cov_mode, len(q), len(t)):
            continue
        score, start, end, diag_len, dist, diagonal, ids = (int(v) for v in fields[x]) if fields is not None else compute(M, q, t, diag, mode)
        sid, ev, bits, aln_len = np.float32(0), 0.0, 0, 0
        with np.errstate(divide='ignore', invalid='ignore'):
            t_cov, q_cov = np.float32(diag_len) / np.float32(len(t)), np.float32(diag_len) / np.float32(len(q))
        rec = None
        if mode == 0:
            sid = seq_id(seq_id_mode, score, len(q), len(t), diag_len)
            aln_len = diag_len
        else:
            ev = evalue(score, len(q))
            bits = int(bitscore(score) + 0.5)
            if mode == 2:
                aln_len = end - start + 1
                if diagonal >= 0:
                    qs, qe, ts, te = start + dist, end + dist, start, end
                else:
                    qs, qe, ts, te = start, end, start + dist, end + dist
                if ev <= e or identity:
                    sid = seq_id(seq_id_mode, ids, len(q), len(t), aln_len)
                q_cov, t_cov = compute_cov(qs, qe, len(q)), compute_cov(ts, te, len(t))
                rec = (ev, bits, len(t), key, '%d\t%d\t%s\t%.3E\t%d\t%d\t%d\t%d\t%d\t%d%s\n' % (
                    key, bits, seq_id_text(sid), ev, qs, qe, len(q), ts, te, len(t), ('\t%dM' % aln_len) if a else ''))
        ok = (has_coverage(c, cov_mode, q_cov, t_cov) and float(sid) >= float(np.float32(min_seq_id) - np.finfo(np.float32).eps)
              and ev <= e and aln_len >= min_aln_len)
        if not (identity or ok):
            continue
        if mode == 2:
            aln.append(rec)
        else:
            # hit.prefScore = 100 * seqId with seqId a double (rescorediagonal.cpp:243,336)
            short.append((bits if mode == 1 else int(100.0 * float(sid)), key, diagonal))
    if sort:
        aln.sort(key=lambda r: (r[0], -r[1], r[2], r[3]))        # Matcher::compareHits
        short.sort(key=lambda h: (-abs(h[0]), h[1]))             # hit_t::compareHitsByScoreAndId
    text = ''.join(r[4] for r in aln)
    # QueryMatcher::prefilterHitToBuffer: key, score, diagonal as a signed 16-bit value (hit_t::diagonal is an unsigned short)
    text += ''.join('%d\t%d\t%d\n' % (k, p, ((d & 0xFFFF) ^ 0x8000) - 0x8000) for p, k, d in short)
    return text
