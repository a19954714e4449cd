"""A plain numpy restatement of linclust's kmermatcher for amino-acid sequences in one split (M/src/linclust/kmermatcher.cpp):
the reduced alphabet, the records of every sequence, the two sorts, assignGroup, writeKmerMatcherResult and the entries of the prefilter DB.
It is what tests/test_kmermatch.py holds against the vectors recorded from the reference's own object code (tools/make_golden_kmermatch.py)
and what the GPU tests hold the device against where nothing is recorded.  selection_info gives the selection of one sequence by itself
(kmerConsidered, threshold, excess, last bin): the generator asserts its class properties with it, the GPU tests hold km_select_kernel's
per-sequence output against it.

`drop` names one of the reference's quirks to leave out -- the generator asserts that each omission changes a recorded entry:
  'last_bin'   lines 288-296: take every window below the threshold until kmerConsidered are taken
  'tie'        writeKmerMatcherResult's `>=`: the first of the longest diagonal runs wins, not the last
  'len_desc'   compareRepSequenceAndIdAndPos without its seqLen-descending field
"""
import numpy as np

P1, P2, P3, P4, P5 = (np.uint64(x) for x in (11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579,
                                            2870177450012600261))
U64 = np.uint64


def _rotl(x, r):
    return (x << U64(r)) | (x >> U64(64 - r))


def xxh64_word(v, seed):
    """XXH64 of 8-byte little-endian words (published specification, input shorter than 32 bytes); v: uint64 array"""
    with np.errstate(over='ignore'):
        v = np.asarray(v, np.uint64)
        h = U64(seed & 0xFFFFFFFFFFFFFFFF) + P5 + U64(8)
        h = h ^ (_rotl(v * P2, 31) * P1)
        h = _rotl(h, 27) * P1 + P4
        h ^= h >> U64(33)
        h = h * P2
        h ^= h >> U64(29)
        h = h * P3
        h ^= h >> U64(32)
        return h


def auto_k(min_seq_id, residues):
    """setKmerLengthAndAlphabet, amino acids, -k 0 -> (k, alphabet size)"""
    if (np.float32(min_seq_id) + 0.001) >= 0.99:
        return 14, 21
    if (np.float32(min_seq_id) + 0.001) >= 0.9:
        return 14, 13
    return max(10, int(np.float64(np.log(np.float32(residues))) / np.log(8.7))), 13


def params(k=0, alph_size=13, kmer_per_seq=0, kmer_per_seq_scale=0.0, hash_shift=67, cov_mode=0, c=0.8, include_only_extendable=False,
           min_seq_id=0.0, residues=0):
    if k == 0:
        k, alph_size = auto_k(min_seq_id, residues)
    return dict(k=int(k), alph_size=int(alph_size), kmer_per_seq=int(kmer_per_seq) if kmer_per_seq else 20,
                kmer_per_seq_scale=float(kmer_per_seq_scale), hash_shift=int(hash_shift), cov_mode=int(cov_mode), c=float(c),
                include_only_extendable=bool(include_only_extendable))


def matrix_prob(text):
    """the joint probabilities of a matrix in the .out layout (sd_host_matrix_text), as SubstitutionMatrix::readProbMatrix rebuilds them"""
    lines = text.splitlines()
    back = np.array([float(x) for x in lines[0].split(':')[1].split()])
    lam = float(lines[1].split(':')[1])
    half = np.array([[float(x) for x in l.split()[1:]] for l in lines[3:24]])
    if not ((half[20] > 0).any() or (half[:, 20] > 0).any()):
        back[:20] = back[:20] * (1.0 - back[20])
    return np.exp(lam * half) * np.outer(back, back)


def reduced_alphabet(prob, alph_size):
    """ReducedMatrix's merging over the joint probabilities prob [21, 21] -> letter map uint8 [21] (X the last code)"""
    if alph_size == 21:
        return np.arange(21, dtype=np.uint8)
    full = 20
    p = np.array(prob, np.float64)[:full, :full].copy()
    alphabet, group = list(range(21)), list(range(21))

    def couple(m, size, b1, b2):
        t = np.zeros((size, size))
        t[:, :b2] = m[:size, :b2]
        t[:, b1] = m[:size, b1] + m[:size, b2]
        t[:, b2:size - 1] = m[:size, b2 + 1:size]
        o = np.zeros((size, size))
        o[:b2] = t[:b2]
        o[b1] = t[b1] + t[b2]
        o[b2:size - 1] = t[b2 + 1:size]
        return o

    for step in range(21 - alph_size):
        size = full - step
        best, bi, bj = 0.0, 0, 0
        for i in range(size):
            for j in range(i + 1, size):
                t = couple(p, size, i, j)[:size - 1, :size - 1]
                back = t.sum(axis=1)
                info = float((t * np.log2(t / np.outer(back, back))).sum())
                if info > best:
                    best, bi, bj = info, i, j
        p = couple(p, size, bi, bj)
        kept, lost = alphabet[bi], alphabet[bj]
        del alphabet[bj]
        group = [kept if g == lost else g for g in group]
    return np.array([alphabet.index(g) for g in group], np.uint8)


def can_be_covered(cov_thr, cov_mode, q_len, t_len):
    q, t, c = np.asarray(q_len, np.float32), np.asarray(t_len, np.float32), np.float32(cov_thr)
    with np.errstate(divide='ignore', invalid='ignore'):
        if cov_mode == 0:
            return (q / t >= c) & (t / q >= c)
        if cov_mode == 1:
            return q / t >= c
        if cov_mode == 2:
            return t / q >= c
        if cov_mode == 3:
            return (t / q >= c) & (t / q <= np.float32(1.0))
        if cov_mode == 4:
            return (q / t >= c) & (q / t <= np.float32(1.0))
        if cov_mode == 5:
            return np.minimum(t, q) / np.maximum(t, q) >= c
    return np.ones(np.shape(q), bool)


def selection_info(par, seq, letter_map):
    """(windows without X, kmerConsidered, threshold, excess e, size c of the last bin) of one sequence, as records() selects"""
    k, A = par['k'], par['alph_size']
    codes = np.asarray(letter_map)[seq].astype(np.uint64)
    L = len(seq)
    if L < k:
        return 0, 0, 0, 0, 0
    with np.errstate(over='ignore'):
        idx = np.zeros(L - k + 1, np.uint64)
        pw = np.uint64(1)
        for j in range(k):
            idx += codes[j:j + L - k + 1] * pw
            pw = pw * np.uint64(A - 1)
    xc = np.concatenate([[0], np.cumsum(codes == A - 1)])
    ok = (xc[k:] - xc[:L - k + 1]) == 0
    score = (xxh64_word(idx[ok], par['hash_shift']) & np.uint64(0xFFFF)).astype(np.int64)
    want = np.float32(par['kmer_per_seq'] - 1) + np.float32(par['kmer_per_seq_scale']) * np.float32(L)
    considered = min(int(want) if want > 0 else 0, len(score))
    if considered == 0:
        return len(score), 0, 0, 0, 0
    thr = int(np.sort(score)[considered - 1]) + 1
    in_bins = int((score < thr).sum())
    return len(score), considered, thr, in_bins - considered, int((score == thr - 1).sum())


def records(par, residues, offsets, keys, letter_map, drop=None):
    """fillKmerPositionArray: per sequence the identity record, then the selected windows in position order ->
    (key uint64, id uint32, seq_len int64, pos int64, rec_off int64 [n + 1])"""
    k, A, seed = par['k'], par['alph_size'], par['hash_shift']
    residues = np.asarray(residues, np.uint8)
    offsets = np.asarray(offsets, np.int64)
    n, total = len(offsets) - 1, int(offsets[-1])
    codes = np.asarray(letter_map, np.uint8)[residues].astype(np.uint64)
    x_code = A - 1
    with np.errstate(over='ignore'):
        idx = np.zeros(total, np.uint64)
        pw = U64(1)
        for j in range(k):
            idx[:max(total - j, 0)] += codes[j:] * pw
            pw = pw * U64(A - 1)
        x_cum = np.concatenate([[0], np.cumsum(codes == x_code)])
        max_len = int(np.diff(offsets).max()) if n else 0
        pw31 = np.ones(max(max_len, 1), np.uint64)
        for i in range(1, max_len):
            pw31[i] = pw31[i - 1] * U64(31)
    score_all = (xxh64_word(idx, seed) & U64(0xFFFF)).astype(np.int64)
    out_key, out_id, out_len, out_pos, rec_off = [], [], [], [], [0]
    for s in range(n):
        a, b = int(offsets[s]), int(offsets[s + 1])
        L = b - a
        with np.errstate(over='ignore'):
            h = (codes[a:b] * pw31[:L][::-1]).sum(dtype=np.uint64) if L else U64(0)
        out_key.append(xxh64_word(np.array([h], np.uint64), seed))
        out_id.append(np.array([keys[s]], np.uint32))
        out_len.append(np.array([L], np.int64))
        out_pos.append(np.array([0], np.int64))
        n_rec = 1
        if L >= k:
            pos = np.arange(L - k + 1)
            ok = (x_cum[a + pos + k] - x_cum[a + pos]) == 0
            pos = pos[ok]
            score = score_all[a + pos]
            want = np.float32(par['kmer_per_seq'] - 1) + np.float32(par['kmer_per_seq_scale']) * np.float32(L)
            considered = min(int(want) if want > 0 else 0, len(pos))
            if considered > 0:
                thr = int(np.sort(score)[considered - 1]) + 1   # the walk of lines 208-220: first t with #(score < t) >= considered
                in_bins = int((score < thr).sum())
                excess = in_bins - considered
                is_last = score == thr - 1
                if drop == 'last_bin':
                    take = score < thr
                else:
                    last_rank = np.cumsum(is_last) - 1
                    take = (score < thr - 1) | (is_last & ((excess == 0) | (last_rank < excess)))
                sel = np.nonzero(take)[0][:considered]
                out_key.append(idx[a + pos[sel]])
                out_id.append(np.full(len(sel), keys[s], np.uint32))
                out_len.append(np.full(len(sel), L, np.int64))
                out_pos.append(pos[sel].astype(np.int64))
                n_rec += len(sel)
        rec_off.append(rec_off[-1] + n_rec)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(out_key, np.uint64), cat(out_id, np.uint32), cat(out_len, np.int64), cat(out_pos, np.int64), np.array(rec_off, np.int64)


def group(par, key, ids, lens, pos, drop=None):
    """the first sort, assignGroup, the second sort, writeKmerMatcherResult -> (hits [h, 4] int64: rep, member, score, diagonal; stats)"""
    n = len(key)
    ids64 = ids.astype(np.int64)
    order = np.lexsort((pos, ids64, key)) if drop == 'len_desc' else np.lexsort((pos, ids64, -lens, key))
    key, ids64, lens, pos = key[order], ids64[order], lens[order], pos[order]
    stats = dict(records=n, grouped=0, hits=0, largest_group=0)
    if n == 0:
        return np.zeros((0, 4), np.int64), stats
    start = np.ones(n, bool)
    start[1:] = key[1:] != key[:-1]
    run_id = np.cumsum(start) - 1
    first = np.nonzero(start)[0]
    run_len = np.diff(np.append(first, n))
    stats['largest_group'] = int(run_len.max())
    rep_at = first[run_id]
    diagonal = pos[rep_at] - pos
    rep_len, mem_len = lens[rep_at], lens
    if par['include_only_extendable']:
        emit = (diagonal < 0) | (diagonal > rep_len - mem_len)
    else:
        emit = can_be_covered(par['c'], par['cov_mode'], rep_len, mem_len)
    emit &= run_len[run_id] > 1
    g_rep, g_id, g_diag = ids64[rep_at][emit], ids64[emit], diagonal[emit]
    w = len(g_rep)
    stats['grouped'] = w
    o2 = np.lexsort((g_diag, g_id, g_rep))
    g_rep, g_id, g_diag = g_rep[o2], g_id[o2], g_diag[o2]
    # what the reference's array holds: the grouped records, then the first sort's records w .. n - 1 with id and pos untouched
    all_id = np.concatenate([g_id, ids64[w:]]).tolist()
    all_d = np.concatenate([g_diag, pos[w:]]).tolist()
    reps, mems = g_rep.tolist(), g_id.tolist()
    hits = []
    for j in range(w):
        if j > 0 and reps[j] == reps[j - 1] and mems[j] == mems[j - 1]:
            continue
        member = mems[j]
        if member == reps[j]:
            continue
        diag, prev, best, run, score, x = all_d[j], all_d[j], 0, 0, 0, j
        while x < n and all_id[x] == member:   # (the walk follows the member id alone)
            d = all_d[x]
            run = run + 1 if d == prev else 1
            if (run > best) if drop == 'tie' else (run >= best):
                diag, best = d, run
            prev = d
            score += 1
            x += 1
        hits.append((reps[j], member, score, diag))
    stats['hits'] = len(hits)
    return np.array(hits, np.int64).reshape(-1, 4), stats


def entries(keys, hits):
    """the prefilter DB: dict key -> bytes, one entry per sequence (the diagonal printed through a short, QueryMatcher.h:118-130)"""
    db = {int(k): b'%d\t0\t0\n' % int(k) for k in keys}
    for rep, member, score, diag in np.asarray(hits, np.int64).reshape(-1, 4).tolist():
        d16 = ((diag + 32768) & 0xFFFF) - 32768
        db[rep] += b'%d\t%d\t%d\n' % (member, score, d16)
    return db


def kmermatch(par, residues, offsets, keys, letter_map, drop=None):
    """-> (hits, stats, records tuple)"""
    rec = records(par, residues, offsets, keys, letter_map, drop=drop)
    hits, stats = group(par, rec[0], rec[1], rec[2], rec[3], drop=drop)
    return hits, stats, rec
