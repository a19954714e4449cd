"""Plain-Python restatement of Alignment::computeAlternativeAlignment (M/src/alignment/Alignment.cpp:569-601) for one seed:
the mask / align / accept loop around a Smith-Waterman function that the caller supplies (the scalar oracle's sw_align, the
reference's matcher, or records that came from the GPU), with Alignment::checkCriteria (:548-567) on the fields
Matcher::getSWResult derives (Matcher.cpp:88-126).  tests/golden/altali_vectors.npz (tools/make_golden_altali.py) holds what the
reference's matcher returns when it is driven through the same loop."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'altali_vectors.npz')
F32 = np.float32
X = 20                      # numeric code of 'X' (Sequence.cpp:307-324)
REC_FIELDS = ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'identical', 'btLen')
PAR_FIELDS = ('sw_mode', 'cov_mode', 'cov_thr', 'eval_thr', 'seq_id_thr', 'aln_len_thr', 'seq_id_mode')


def params(row):
    """a row of the golden `params` table -> dict; the E-value threshold goes through a float as the reference's signature has it"""
    p = dict(zip(PAR_FIELDS, row))
    for k in ('sw_mode', 'cov_mode', 'aln_len_thr', 'seq_id_mode'):
        p[k] = int(p[k])
    p['eval_thr'] = float(F32(p['eval_thr']))
    return p


def _cov(start, end, length):   # Util::computeCov
    return F32(min(length, max(start, end)) - min(start, end) + 1) / F32(length)


def _has_coverage(thr, mode, qcov, dbcov):   # Util::hasCoverage
    thr = F32(thr)
    if mode == 0:
        return qcov >= thr and dbcov >= thr
    if mode == 2:
        return qcov >= thr
    if mode == 1:
        return dbcov >= thr
    return True


def accepted(r, qlen, tlen, p):
    """Alignment::checkCriteria on a Smith-Waterman record.  A record without positions was stopped at the E-value or the
    coverage gate of ssw_align and fails the same criterion here (a record without an end position carries uninitialised
    fields in the reference: there is nothing to restate)."""
    if r['tEnd'] < 0 or r['qStart'] < 0 or r['tStart'] < 0:
        return False
    qcov, dbcov = _cov(r['qStart'], r['qEnd'], qlen), _cov(r['tStart'], r['tEnd'], tlen)
    aln_len = max(abs(r['qEnd'] - r['qStart']), abs(r['tEnd'] - r['tStart'])) + 1      # Matcher::computeAlnLength
    if p['sw_mode'] == 2:
        if r['btLen'] <= 0:
            return False
        aln_len = r['btLen']
        den = {1: min(qlen, tlen), 2: max(qlen, tlen)}.get(p['seq_id_mode'], aln_len)  # Util::computeSeqId
        seq_id = F32(r['identical']) / F32(den)
    else:                                                                               # Matcher::estimateSeqIdByScorePerCol
        q_aln, t_aln = max(r['qEnd'] - r['qStart'], 1), max(r['tEnd'] - r['tStart'], 1)
        e = F32(float(F32(r['score'] & 0xFFFF) / F32(max(q_aln, t_aln))) * 0.1656 + 0.1141)
        seq_id = max(F32(0.0), min(e, F32(1.0)))
    return bool(r['evalue'] <= p['eval_thr'] and seq_id >= F32(p['seq_id_thr']) and _has_coverage(p['cov_thr'], p['cov_mode'], qcov, dbcov)
                and aln_len >= p['aln_len_thr'])


def alternatives(align, target, t_start, t_end, n, qlen, p, identity=False):
    """up to n alternative alignments of a seed whose accepted alignment covers target positions [t_start, t_end].
    align(masked target as numeric codes) -> record dict.  The mask's end is exclusive (Alignment.cpp:586,595)."""
    if identity:
        return []
    t = np.array(target, np.uint8, copy=True)
    t[t_start:t_end] = X
    out = []
    for _ in range(n):
        r = align(t)
        if not accepted(r, qlen, len(t), p):
            break
        out.append(r)
        t[r['tStart']:r['tEnd']] = X
    return out


def alternatives_many(align_many, targets, intervals, n, qlens, p):
    """`alternatives` for many seeds at once, round by round, for an aligner that works on batches:
    align_many(list of seed numbers, list of their masked targets) -> one record per listed seed.  Seed s has the target
    targets[s], the accepted interval intervals[s] and a query of qlens[s] residues."""
    masked = []
    for t, (b, e) in zip(targets, intervals):
        m = np.array(t, np.uint8, copy=True)
        m[b:e] = X
        masked.append(m)
    out = [[] for _ in targets]
    live = list(range(len(targets)))
    for _ in range(n):
        if not live:
            break
        recs = align_many(live, [masked[s] for s in live])
        nxt = []
        for s, r in zip(live, recs):
            if accepted(r, qlens[s], len(masked[s]), p):
                out[s].append(r)
                masked[s][r['tStart']:r['tEnd']] = X
                nxt.append(s)
        live = nxt
    return out


def compare_key(r, tlen, tkey, bitscore):
    """Matcher::compareHits: E-value, rounded bit score (descending), target length, target key"""
    return (r['evalue'], -int(bitscore(r['score']) + 0.5), tlen, tkey)


def load():
    """the golden file as python objects: seqs (ASCII bytes), cases (q, t, params index, N, identity), params dicts, seeds,
    and per case the reference's alternatives (records as dicts with evalue and backtrace)"""
    g = np.load(GOLDEN)
    letters, off = g['letters'].tobytes(), g['off']
    seqs = [letters[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    bts = g['bts'].tobytes().decode().split('\n') if len(g['recs']) else []
    want, x = [], 0
    for c in g['counts']:
        rows = []
        for _ in range(int(c)):
            r = dict(zip(REC_FIELDS, (int(v) for v in g['recs'][x])))
            r['evalue'] = float(g['evalues'][x])
            r['backtrace'] = bts[x]
            rows.append(r)
            x += 1
        want.append(rows)
    return dict(seqs=seqs, cases=[tuple(int(v) for v in c) for c in g['cases']], cls=[str(c) for c in g['cls']],
                params=[params(row) for row in g['params']], db_residues=int(g['db_residues']),
                seeds=[tuple(int(v) for v in s) for s in g['seeds']], want=want)


def same(a, b):
    """two records equal in every field, E-value bits and backtrace included (identical only where a backtrace exists)"""
    return all(a[f] == b[f] for f in REC_FIELDS) and a['evalue'] == b['evalue'] and a.get('backtrace', '') == b.get('backtrace', '')
