"""tantan's float posteriors on the host (csrc/host/sd_tantan.cpp), bit for bit against the reference's own Masker.

The posteriors are never returned, only compared with --mask-prob; tests/golden/tantan_vectors.npz holds them as read from the
reference through that threshold (tests/ttgold.py, tools/make_golden_tantan.py).  The restatement is read the same way: for every
distinct posterior v of a sequence, a run at (double) v must mask exactly the residues with p >= v and a run at the next float
above v exactly those with p >= up(v) -- which holds iff every residue's posterior has the reference's bits, whatever the
compiler made of the multiply-adds.  tests/test_gpu_tantan.py does the same to ib_mask_kernel; its docstring says what such a
check catches (an error of a float ulp: hundreds of residues) and what it cannot (the last bits of the doubles: another order of
the partial sums or a build without fused multiply-adds changes none of the 9 381 posteriors here)."""
import numpy as np
import pytest

import ttgold
from oracle.pyoracle import ref_available


def _pin(mask_fn, seq, post):
    """-> [(threshold, residues that differ)] over two runs per distinct posterior"""
    bad = []
    for v in np.unique(post):
        for t in (v, ttgold.up(v)):
            want, n = ttgold.expected(seq, post, t)
            got, m = mask_fn(seq, float(t))
            if m != n or not np.array_equal(got, want):
                bad.append((float(t), np.nonzero(got != want)[0][:4].tolist(), m, n))
    return bad


def test_fixture_holds_what_the_tests_rely_on():
    _, off, post = ttgold.seqset('A')
    lens = (off[1:] - off[:-1]).astype(int).tolist()
    assert lens == list(range(1, 73)) + [100, 127, 128, 129, 260]
    assert ((post > 0.05) & (post < 0.95)).mean() >= 0.25 and (post < 0.05).mean() >= 0.25
    assert post.min() == 0 and post.max() == 1 and len(np.unique(post)) > 2500
    assert not (ttgold.seqset('A')[0] == ttgold.X).any() and not (ttgold.seqset('B')[0] == ttgold.X).any()
    _, boff, _ = ttgold.seqset('B')
    la, lb = int(boff[1]), int(boff[2] - boff[1])
    assert la % 4 != lb % 4 and la % 16 != lb % 16 and min(la, lb) > 2900


@pytest.mark.parametrize('name', ['A', 'B'])
def test_restatement_has_the_reference_posteriors_bit_for_bit(oracle, name):
    for i, (seq, post) in enumerate(ttgold.sequences(name)):
        bad = _pin(oracle.mask, seq, post)
        assert not bad, ('set %s sequence %d of %d residues: (threshold, first positions, count, expected count)' % (name, i, len(seq)), bad[:3])


@pytest.mark.parametrize('name', ['A', 'B'])
def test_edge_thresholds(oracle, name):
    for thr in ttgold.edge_thresholds():
        for i, (seq, post) in enumerate(ttgold.sequences(name)):
            want, n = ttgold.expected(seq, post, thr)
            got, m = oracle.mask(seq, thr)
            assert m == n and np.array_equal(got, want), (name, i, thr)
    _, _, post = ttgold.seqset('A')
    assert 0 < (post >= 1).sum() < (post > 0).sum() < len(post)   # the edges tell: posteriors of exactly 1 and of exactly 0


def test_x_on_input(oracle):
    """an X stays X at every threshold and counts as masked where its posterior reaches the threshold (masked++ of tantanMask)"""
    res, off, masks, counts = ttgold.set_c()
    assert (res == ttgold.X).sum() >= len(off) - 1
    for k, thr in enumerate(ttgold.C_THRESHOLDS):
        for i in range(len(off) - 1):
            a, b = int(off[i]), int(off[i + 1])
            got, n = oracle.mask(res[a:b], thr)
            assert np.array_equal(got, masks[k, a:b]) and n == int(counts[k, i]), (thr, i)
    assert len({int(c.sum()) for c in counts}) == len(counts)   # the thresholds tell


@pytest.mark.skipif(not ref_available(), reason='the reference build (oracle/_ref/libsdref.so) is not present')
def test_fixture_is_what_the_reference_gives():
    from oracle.pyoracle import Ref
    ref = Ref()
    a, b = ttgold.sequences('A'), ttgold.sequences('B')
    for seq, post in (a[16], a[51], a[76], b[1]):
        assert np.array_equal(ttgold.recover(ref.mask, seq).view(np.uint32), post.view(np.uint32)), len(seq)
    res, off, masks, counts = ttgold.set_c()
    got, n = ref.mask(res[int(off[-2]):], 0.5)
    assert np.array_equal(got, masks[1, int(off[-2]):]) and n == int(counts[1, -1])


def test_mask_prob_reaches_the_host_index_builder(host):
    """sd_host_index_build at thresholds other than 0.9: the masked residues and their count are the fixture's"""
    res, off, post = ttgold.seqset('A')
    v = np.unique(post[(post > 0.3) & (post < 0.6)])[0]
    seen = set()
    for thr in (0.5, float(v), float(ttgold.up(v)), 0.9):
        want, n = ttgold.expected(res, post, thr)
        h = host.build_index(res, off, k=5, kmer_thr=0, mask_prob=thr)
        assert h.masked_residues == n and np.array_equal(h.masked, want), thr
        seen.add(n)
    assert len(seen) == 4
