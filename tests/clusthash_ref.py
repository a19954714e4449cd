"""A restatement of clusthash (M/src/util/clusthash.cpp:64-181, the amino-acid branch) in Python: hash, groups, the greedy loop and the
text.  tests/golden/clusthash_vectors.npz (tools/make_golden_clusthash.py: the reference's own object code) holds what it must equal;
the tests hold the device (sd_clusthash_batch) and the host stages against both.

Sequences are the DB's own bytes (`letters`, uint8) with offsets; ids are positions; `map256` is the reduced matrix's aa2num (byte ->
reduced code), as Sequence::mapSequence(const char *, unsigned) applies it to all L bytes.

A note on the loop.  The reference walks every j != i that is not found, j < i included.  The comparison is symmetric (same two
sequences, same length, same threshold), and a j < i that is not found has had its own turn while i was not found either: it compared
itself with i and failed.  So a j < i never passes, the entries are those of a loop over j > i alone, and only the number of comparisons
differs (`pairs`).  drop='j_gt_i' and drop='skip_reps' state the two misreadings; the generator asserts that they change `pairs` and no
entry, and that drop='codes' (reduced codes compared instead of bytes) changes entries."""
import numpy as np

NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1


def hashes(letters, offsets, map256):
    """Util::hash over the reduced codes: h = 31 h + code, 64-bit wrapping -> uint64 [n]"""
    off = np.asarray(offsets, np.int64)
    n = len(off) - 1
    codes = np.asarray(map256, np.uint8)[np.asarray(letters, np.uint8)].astype(np.uint64)
    longest = int(np.diff(off).max()) if n else 0
    with np.errstate(over='ignore'):
        pw = np.ones(longest + 1, np.uint64)
        for i in range(1, longest + 1):
            pw[i] = pw[i - 1] * np.uint64(31)
        out = np.zeros(n, np.uint64)
        for s in range(n):
            c = codes[off[s]:off[s + 1]]
            out[s] = np.sum(c * pw[len(c) - 1::-1][:len(c)] if len(c) else c, dtype=np.uint64)
    return out


def hash_one(codes):
    """the loop itself, for the tests of hashes()"""
    h = 0
    for c in codes:
        h = (h * 31 + int(c)) & M64
    return h


def reaches(d, length, thr):
    """clusthash.cpp:155-156 in float32; 0 / 0 is not >= anything"""
    if length == 0:
        return False
    with np.errstate(all='ignore'):
        return bool(np.float32(d) / np.float32(length) >= np.float32(thr))


def min_identical(thr, length):
    for d in range(length + 1):
        if reaches(d, length, thr):
            return d
    return length + 1


def clusthash(letters, offsets, map256, thr, drop=None):
    """-> (found_by uint32 [n], identical uint32 [n], hashes uint64 [n], stats dict(unique_hashes, groups, pairs, largest_group))
    groups / largest_group count runs of equal (hash, length), which is what interacts"""
    letters = np.asarray(letters, np.uint8)
    off = np.asarray(offsets, np.int64)
    n = len(off) - 1
    lens = np.diff(off)
    h = hashes(letters, off, map256)
    cmp_bytes = np.asarray(map256, np.uint8)[letters] if drop == 'codes' else letters
    found_by = np.full(n, NONE, np.uint32)
    identical = np.zeros(n, np.uint32)
    by_hash = {}
    for s in range(n):   # ids ascending inside every hash
        by_hash.setdefault(int(h[s]), []).append(s)
    pairs = 0
    sizes = {}
    for s in range(n):
        sizes[(int(h[s]), int(lens[s]))] = sizes.get((int(h[s]), int(lens[s])), 0) + 1
    for ids in by_hash.values():
        if len(ids) == 1:
            continue
        has_list = set()
        for i in ids:
            if found_by[i] != NONE:
                continue
            a = cmp_bytes[off[i]:off[i + 1]]
            for j in ids:
                if found_by[j] != NONE:
                    continue
                if drop == 'j_gt_i' and j < i:
                    continue
                if drop == 'skip_reps' and j in has_list:
                    continue
                if i != j and lens[i] == lens[j]:
                    pairs += 1
                    d = int(np.count_nonzero(a == cmp_bytes[off[j]:off[j + 1]]))
                    if reaches(d, int(lens[i]), thr):
                        found_by[j] = i
                        identical[j] = d
                        has_list.add(i)
    stats = dict(unique_hashes=len(by_hash), groups=sum(1 for v in sizes.values() if v > 1), pairs=pairs,
                 largest_group=max(sizes.values()) if sizes else 0)
    return found_by, identical, h, stats


def seq_id_text(d, length):
    """Util::fastSeqIdToBuffer up to its terminator (clusthash appends the buffer as a C string): "1.000" for one, else three truncated
    decimals"""
    seq_id = np.float32(d) / np.float32(length)
    if seq_id == np.float32(1.0):
        return b'1.000'
    out = b'0.'
    if float(seq_id) < 0.10:   # (the reference compares the float with double constants)
        out += b'0'
    if float(seq_id) < 0.01:
        out += b'0'
    return out + str(int(np.float32(seq_id * np.float32(1000)))).encode()


def entries(keys, offsets, found_by, identical):
    """dict key -> text: the self row, then a row for every t with found_by[t] == s, ascending t"""
    off = np.asarray(offsets, np.int64)
    n = len(off) - 1
    rows = {}
    for t in range(n):
        if found_by[t] != NONE:
            rows.setdefault(int(found_by[t]), []).append(t)
    out = {}
    for s in range(n):
        length = int(off[s + 1] - off[s])
        lm1 = (length - 1) & 0xFFFFFFFF   # unsigned int arithmetic
        tail = b'\t0\t0\t%d\t%d\t0\t%d\t%d\n' % (lm1, length, lm1, length)
        text = b'%d\t255\t1.00' % int(keys[s]) + tail
        for t in rows.get(s, []):
            text += b'%d\t255\t' % int(keys[t]) + seq_id_text(int(identical[t]), length) + tail
        out[int(keys[s])] = text
    return out
