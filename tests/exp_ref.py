"""Plain Python restatement of `expandaln` in both expansion modes (M/src/util/expandaln.cpp:27-76,236-397 with returnAlnRes = true) and of
BacktraceTranslator::translateResult (M/src/commons/BacktraceTranslator.h:51-153), in two forms: on expanded columns, as the reference
works, and on run lists, as the device kernels do.  tests/test_expandaln.py holds both against the reference's own rows
(tests/golden/expand_vectors.npz); the GPU tests take their expectations from here only where the golden file has none."""
import numpy as np

STATES = 'MID'
# transitions[ab][bc] (BacktraceTranslator.h:25-33); None emits no column
TABLE = {('M', 'M'): 'M', ('I', 'M'): 'I', ('D', 'M'): 'D', ('M', 'D'): 'D', ('I', 'D'): None, ('D', 'D'): 'D', ('M', 'I'): 'I',
         ('I', 'I'): 'I', ('D', 'I'): None}
DEFAULTS = dict(e=0.001, c=0.0, cov_mode=0, min_seq_id=0.0, min_aln_len=0, mode=0, seq_id_mode=0, comp_bias_corr=1)


def uncompress(cigar):
    """Matcher::uncompressAlignment (Matcher.cpp:187-201): a count of 0 is one column"""
    bt, n = [], 0
    for ch in cigar:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            bt.append(ch * (n if n else 1))
            n = 0
    return ''.join(bt)


def compress(bt):
    """Matcher::compressAlignment (Matcher.cpp:166-185): starts in state M with no column"""
    out, st, c = [], 'M', 0
    for ch in bt:
        if ch != st:
            out.append('%d%s' % (c, st))
            st, c = ch, 1
        else:
            c += 1
    out.append('%d%s' % (c, st))
    return ''.join(out)


def runs_of(cigar):
    """run-length text -> [(state, length)] as the text holds them (a count of 0 is one column; equal neighbours stay apart)"""
    runs, n = [], 0
    for ch in cigar:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            runs.append((ch, n if n else 1))
            n = 0
    return runs


def translate_columns(ab_start_a, ab_start_b, ab_bt, bc_start_b, bc_start_c, bc_bt):
    """translateResult on expanded backtraces.  Returns (aStart, aEnd, cStart, cEnd, printed backtrace)."""
    off_ab = off_bc = 0
    start_a, start_c = ab_start_a, bc_start_c
    dist = abs(ab_start_b - bc_start_b)
    if ab_start_b < bc_start_b:
        a = b = 0
        while b < dist and off_ab < len(ab_bt):
            b += ab_bt[off_ab] in 'MD'
            a += ab_bt[off_ab] in 'MI'
            off_ab += 1
        start_a += a
    elif ab_start_b > bc_start_b:
        b = c = 0
        while b < dist and off_bc < len(bc_bt):
            b += bc_bt[off_bc] in 'MI'
            c += bc_bt[off_bc] in 'MD'
            off_bc += 1
        start_c += c
    out, last_m, q_aln, db_aln = [], 0, 0, 0
    while off_ab < len(ab_bt) and off_bc < len(bc_bt):
        t = TABLE[(ab_bt[off_ab], bc_bt[off_bc])]
        off_ab += 1
        off_bc += 1
        if t is None:
            continue
        out.append(t)
        if t == 'M':
            last_m = len(out)
        q_aln += t in 'MD'
        db_aln += t in 'MI'
    return start_a, start_a + q_aln - 1, start_c, start_c + db_aln - 1, ''.join(out[:last_m])


def translate_runs(ab_start_a, ab_start_b, ab_runs, bc_start_b, bc_start_c, bc_runs):
    """the same on run lists [(state, length)]: a merge, never a column.  Returns (aStart, aEnd, cStart, cEnd, printed columns,
    run-length text of the printed backtrace or '' when there is none)."""
    class Cur:
        def __init__(self, runs):
            self.runs, self.i = runs, 0
            self.load()

        def load(self):
            self.st, self.rem = self.runs[self.i] if self.i < len(self.runs) else (None, 0)

        def take(self, n):
            self.rem -= n
            if self.rem == 0:
                self.i += 1
                self.load()

        def live(self):
            return self.i < len(self.runs)
    a, b = Cur(ab_runs), Cur(bc_runs)
    off_a = off_c = 0
    dist, in_b = abs(ab_start_b - bc_start_b), 0
    if ab_start_b < bc_start_b:
        while in_b < dist and a.live():
            n = a.rem
            if a.st != 'I':
                n = min(n, dist - in_b)
                in_b += n
            if a.st != 'D':
                off_a += n
            a.take(n)
    elif ab_start_b > bc_start_b:
        while in_b < dist and b.live():
            n = b.rem
            if b.st != 'D':
                n = min(n, dist - in_b)
                in_b += n
            if b.st != 'I':
                off_c += n
            b.take(n)
    out = []   # merged output runs
    cols = last_m = q_aln = db_aln = 0
    runs_at_m = 0
    while a.live() and b.live():
        n = min(a.rem, b.rem)
        t = TABLE[(a.st, b.st)]
        if t is not None:
            if out and out[-1][0] == t:
                out[-1][1] += n
            else:
                out.append([t, n])
            cols += n
            q_aln += n if t != 'I' else 0
            db_aln += n if t != 'D' else 0
            if t == 'M':
                last_m, runs_at_m = cols, len(out)
        a.take(n)
        b.take(n)
    text = ''
    if last_m:
        text = ('0M' if out[0][0] != 'M' else '') + ''.join('%d%s' % (n, s) for s, n in out[:runs_at_m])
    start_a, start_c = ab_start_a + off_a, bc_start_c + off_c
    return start_a, start_a + q_aln - 1, start_c, start_c + db_aln - 1, last_m, text


def parse_row(line):
    c = line.split('\t')
    return dict(key=int(c[0]), score=int(c[1]), seqid_text=c[2], seqid=np.float32(float(c[2])), eval_text=c[3], eval=float(c[3]),
                q_start=int(c[4]), q_end=int(c[5]), q_len=int(c[6]), db_start=int(c[7]), db_end=int(c[8]), db_len=int(c[9]),
                cigar=c[10] if len(c) > 10 else None)


def rows_of(text):
    return [parse_row(l) for l in text.decode().splitlines() if l]


def can_be_covered(thr, mode, q_len, t_len):
    """Util::canBeCovered (Util.cpp:477-494), float arithmetic"""
    thr, q, t = np.float32(thr), np.float32(q_len), np.float32(t_len)
    if mode == 0:
        return bool(q / t >= thr and t / q >= thr)
    if mode == 1:
        return bool(q / t >= thr)
    if mode == 2:
        return bool(t / q >= thr)
    if mode == 3:
        return bool(t / q >= thr and t / q <= 1.0)
    if mode == 4:
        return bool(q / t >= thr and q / t <= 1.0)
    if mode == 5:
        return bool(min(t, q) / max(t, q) >= thr)
    return True


def cov(start, end, length):
    """SmithWaterman::computeCov on unsigned ints"""
    u = lambda v: v & 0xFFFFFFFF
    start, end, length = u(start), u(end), u(length)
    return np.float32(u(min(length, max(start, end)) - min(start, end) + 1)) / np.float32(length)


def has_coverage(thr, mode, q_cov, t_cov):
    thr = np.float32(thr)
    if mode == 0:
        return bool(q_cov >= thr and t_cov >= thr)
    if mode == 1:
        return bool(t_cov >= thr)
    if mode == 2:
        return bool(q_cov >= thr)
    return True


def seqid_text(seqid):
    """Util::fastSeqIdToBuffer as Matcher::resultToBuffer leaves it"""
    seqid = np.float32(seqid)
    if seqid == np.float32(1.0):
        return '1.00'
    return '0.' + ('0' if seqid < 0.10 else '') + ('0' if seqid < 0.01 else '') + str(int(np.float32(seqid * np.float32(1000))))


def bc_aln_length(r):
    qs, ds = (0 if r['q_start'] == -1 else r['q_start']), (0 if r['db_start'] == -1 else r['db_start'])
    return max(abs(r['q_end'] - qs), abs(r['db_end'] - ds)) + 1


def walk(bt, a_start, c_start, a_res, c_res, a_bias, matrix, gap_open=11, gap_extend=1):
    """rescoreResultByBacktrace (expandaln.cpp:27-76) over the printed backtrace: I advances the query, D the target.  a_res / c_res:
    numeric residues, a_bias: the rounded composition bias per query position (or None), matrix: 21 x 21.  Returns (raw score,
    identities), or None when an M column lies outside either sequence (the reference reads stale memory there)."""
    q, t, score, ident, last = a_start, c_start, 0, 0, ''
    for ch in bt:
        if ch == 'M':
            if q < 0 or t < 0 or q >= len(a_res) or t >= len(c_res):
                return None
            score += int(matrix[int(a_res[q])][int(c_res[t])]) + (int(a_bias[q]) if a_bias is not None else 0)
            ident += int(a_res[q] == c_res[t])
            q += 1
            t += 1
        else:
            score -= gap_extend if last == ch else gap_open
            if ch == 'I':
                q += 1
            else:
                t += 1
        last = ch
    return score, ident


def seq_id(mode, ids, q_len, t_len, aln_len):
    """Util::computeSeqId (Util.cpp:532-542)"""
    if mode == 1:
        return np.float32(ids) / np.float32(min(q_len, t_len))
    if mode == 2:
        return np.float32(ids) / np.float32(max(q_len, t_len))
    if mode == 0:
        return np.float32(ids) / np.float32(aln_len)
    return np.float32(0.0)


def expand(ab_db, bc_db, params=None, pairs=None, run_form=True, seqs=None):
    """ab_db / bc_db: dict key -> bytes of an alignment DB entry.  Returns dict key -> bytes of the entries expandaln writes.
    pairs (a list): receives (aStart, aEnd, cStart, cEnd, printed columns, text or '') of every translated pair, in order.
    mode 1 (params['mode'] = 1) needs seqs = dict(a=key -> residues, c=key -> residues, a_bias=key -> rounded bias, matrix=21 x 21,
    evalue=f(raw, aLen), bitscore=f(raw)); seqs['walks'] (a list, optional) receives walk()'s result of every pair that is walked."""
    p = dict(DEFAULTS)
    p.update(params or {})
    bc_rows = {k: rows_of(t) for k, t in bc_db.items()}
    out = {}
    for q in sorted(ab_db):
        kept_keys, lines = set(), []
        for ab in rows_of(ab_db[q]):
            assert ab['cigar'] is not None, 'Alignment must contain a backtrace'
            if ab['key'] not in bc_rows:
                continue
            for bc in bc_rows[ab['key']]:
                assert bc['cigar'] is not None, 'Alignment must contain a backtrace'
                if run_form:
                    a0, a1, c0, c1, n, text = translate_runs(ab['q_start'], ab['db_start'], runs_of(ab['cigar']), bc['q_start'], bc['db_start'],
                                                             runs_of(bc['cigar']))
                else:
                    a0, a1, c0, c1, bt = translate_columns(ab['q_start'], ab['db_start'], uncompress(ab['cigar']), bc['q_start'], bc['db_start'],
                                                           uncompress(bc['cigar']))
                    n, text = len(bt), (compress(bt) if bt else '')
                if pairs is not None:
                    pairs.append((a0, a1, c0, c1, n, text))
                if n == 0:
                    continue
                if not can_be_covered(p['c'], p['cov_mode'], ab['q_len'], bc['db_len']):
                    continue
                if bc['key'] in kept_keys:   # overlapping or not (expandaln.cpp:329-334)
                    continue
                score, seqid, ev = ab['score'], ab['seqid'], ab['eval']
                if p['mode'] == 1:
                    a_res, c_res = seqs['a'][q], seqs['c'][bc['key']]
                    w = walk(uncompress(text), a0, c0, a_res, c_res, seqs['a_bias'][q] if p['comp_bias_corr'] else None, seqs['matrix'])
                    if 'walks' in seqs:
                        seqs['walks'].append(w)
                    if w is None or w[0] < -6:   # (None: no reference row exists for such a pair; the module drops and counts it)
                        continue
                    ev = seqs['evalue'](w[0], len(a_res))
                    score = int(seqs['bitscore'](w[0]) + 0.5)
                    seqid = seq_id(p['seq_id_mode'], w[1], len(a_res), len(c_res), n)
                ok = has_coverage(p['c'], p['cov_mode'], cov(a0, a1, ab['q_len']), cov(c0, c1, bc['db_len']))
                ok = ok and bool(np.float32(seqid) >= np.float32(p['min_seq_id']) - np.finfo(np.float32).eps)
                ok = ok and ev <= p['e'] and bc_aln_length(bc) >= p['min_aln_len']
                if ok:
                    kept_keys.add(bc['key'])
                    lines.append('%d\t%d\t%s\t%.3E\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n' % (bc['key'], score, seqid_text(seqid), ev, a0, a1,
                                                                                   ab['q_len'], c0, c1, bc['db_len'], text))
        out[q] = ''.join(lines).encode()
    return out
