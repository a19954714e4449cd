#!/usr/bin/env python3
"""Golden posteriors for the tantan masking tests (tests/test_tantan_posteriors.py, tests/test_gpu_tantan.py) into
tests/golden/tantan_vectors.npz: per residue the float posterior of the reference's own Masker (oracle/_ref/libsdref.so), which
returns mask bytes only -- read through its threshold by bisection over the floats (tests/ttgold.py: recover).

  A  the ladder: one sequence of every length 1..72, then 100, 127, 128, 129 and 260; tandem repeats of period 1..50 with 5-20 %
     substitutions -- of six sequences one is a repeat of many copies, one plain random, four are runs of short repeats (a period
     and 3..10 residues more) between random residues.  No X.  At least a quarter of the residues have a posterior strictly
     between 0.05 and 0.95 and at least a quarter one below 0.05 (asserted; repeats of many copies alone leave 12 % between).
  B  two sequences of about 3 000 residues (repeat, random, repeat) whose lengths differ modulo 4 and modulo 16.  No X.
  C  sequences of A with X planted: the reference's mask bytes and masked counts at 0.2, 0.5, 0.9 and 0.99 (an X stays X at any
     threshold, so no posterior can be read there).

Writes the archive with fixed time stamps: it regenerates byte for byte.  Dev container only:  python tools/make_golden_tantan.py"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.pyoracle import Ref  # noqa: E402
import ttgold  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
SEED_A, SEED_B, SEED_C = 6, 23, 5
EXTRAS = (100, 127, 128, 129, 260)
B_LENGTHS = (2999, 3010)          # 3 and 2 modulo 4, 7 and 2 modulo 16
C_FROM = (5, 30, 52, 53, 64, 72, 129, 260)   # lengths of the sequences of A that get X


def save(path, arrays):
    with zipfile.ZipFile(path, 'w') as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED, 9)


def repeat(rng, n, period, subst):
    unit = rng.integers(0, 20, period).astype(np.uint8)
    s = np.tile(unit, n // period + 1)[:n]
    return np.where(rng.random(n) < subst, rng.integers(0, 20, n).astype(np.uint8), s)


def ladder_sequence(rng, L, kind):
    """kind 5: plain random.  kind 2: one repeat of many copies over half of the sequence or more (posteriors near 1).  Else short
    repeats one after the other, each a period plus 3..10 residues long with random residues between them: evidence at the
    border of what tantan takes for a repeat, which is where the posteriors between 0.05 and 0.95 come from"""
    s = rng.integers(0, 20, L).astype(np.uint8)
    if kind == 5 or L < 4:
        return s
    if kind == 2:
        period = int(rng.integers(1, min(50, max(1, L // 3)) + 1))
        n = int(rng.integers(max(2 * period + 1, L // 2), L + 1))
        a = int(rng.integers(0, L - n + 1))
        s[a:a + n] = repeat(rng, n, period, rng.uniform(0.05, 0.20))
        return s
    at = int(rng.integers(0, 4))
    while at < L:
        period = int(rng.integers(1, min(50, max(1, (L - at) // 2)) + 1))
        n = min(L - at, period + int(rng.integers(3, 11)))
        s[at:at + n] = repeat(rng, n, period, rng.uniform(0.05, 0.20))
        at += n + int(rng.integers(3, 11))
    return s


def long_sequence(rng, L):
    s = rng.integers(0, 20, L).astype(np.uint8)
    s[:L // 3] = repeat(rng, L // 3, int(rng.integers(20, 51)), 0.12)
    s[L - L // 3:] = repeat(rng, L // 3, int(rng.integers(2, 20)), 0.18)
    return s


def cat(parts, dt):
    return np.concatenate([np.asarray(p, dt) for p in parts])


def offsets(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return off


def main():
    ref = Ref()
    rng = np.random.default_rng(SEED_A)
    lengths = list(range(1, 73)) + list(EXTRAS)
    a_seqs = [ladder_sequence(rng, L, i % 6) for i, L in enumerate(lengths)]
    a_post = [ttgold.recover(ref.mask, s) for s in a_seqs]
    p = cat(a_post, np.float32)
    middle, low = float(((p > 0.05) & (p < 0.95)).mean()), float((p < 0.05).mean())
    print('A: %d sequences, %d residues, %d distinct posteriors; %.1f %% in (0.05, 0.95), %.1f %% below 0.05, %d exactly 0, %d exactly 1, '
          '%d at or above 0.9' % (len(a_seqs), len(p), len(np.unique(p)), 100 * middle, 100 * low, int((p == 0).sum()), int((p == 1).sum()),
                                  int((p >= np.float32(0.9)).sum())))
    assert middle >= 0.25 and low >= 0.25, 'choose another SEED_A'
    assert p.min() >= 0 and p.max() <= 1

    rng = np.random.default_rng(SEED_B)
    assert B_LENGTHS[0] % 4 != B_LENGTHS[1] % 4 and B_LENGTHS[0] % 16 != B_LENGTHS[1] % 16
    b_seqs = [long_sequence(rng, L) for L in B_LENGTHS]
    b_post = [ttgold.recover(ref.mask, s) for s in b_seqs]
    pb = cat(b_post, np.float32)
    print('B: lengths %s, %d distinct posteriors, %d at or above 0.9' % (B_LENGTHS, len(np.unique(pb)), int((pb >= np.float32(0.9)).sum())))

    rng = np.random.default_rng(SEED_C)
    c_seqs = []
    for L in C_FROM:
        s = a_seqs[lengths.index(L)].copy()
        at = rng.choice(L, max(1, L // 12), replace=False)
        s[at] = ttgold.X
        if L >= 52:
            s[[0, L - 1]] = ttgold.X
        c_seqs.append(s)
    c_mask, c_count = [], []
    for t in ttgold.C_THRESHOLDS:
        out = [ref.mask(s, t) for s in c_seqs]
        c_mask.append(cat([m for m, _ in out], np.uint8))
        c_count.append([n for _, n in out])
    print('C: %d sequences, masked counts per threshold %s' % (len(c_seqs), [int(sum(c)) for c in c_count]))

    path = os.path.join(GOLD, 'tantan_vectors.npz')
    save(path, dict(A_res=cat(a_seqs, np.uint8), A_off=offsets(a_seqs), A_post=p,
                    B_res=cat(b_seqs, np.uint8), B_off=offsets(b_seqs), B_post=pb,
                    C_res=cat(c_seqs, np.uint8), C_off=offsets(c_seqs), C_thr=np.array(ttgold.C_THRESHOLDS, np.float64),
                    C_mask=np.array(c_mask, np.uint8), C_count=np.array(c_count, np.uint32)))
    print(os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
