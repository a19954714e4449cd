"""The yardstick of the exhaustive ungapped prefilter, without a GPU: the numpy restatement of the scan and of the list rule
(tests/ungapped_ref.py) against tests/golden/ungapped_vectors.npz, which tools/make_golden_ungapped.py wrote from the
reference's own SmithWaterman::ungapped_alignment; where oracle/_ref/libsdref.so exists the live reference is asked again."""
import numpy as np
import pytest

import ungapped_ref as ur


@pytest.fixture(scope='module')
def gold():
    return np.load(ur.GOLDEN)


def _seq(g, i):
    return g['res'][int(g['off'][i]):int(g['off'][i + 1])]


def _cb(g, i):
    return g['cb'][int(g['off'][i]):int(g['off'][i + 1])]


def test_golden_file_covers_what_the_kernel_tests_need(gold):
    g = gold
    lens = (g['off'][1:] - g['off'][:-1]).astype(np.int64)
    ql, tl = lens[g['pq']], lens[g['pt']]
    for b in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 65535):
        assert (ql == b).any() and (tl == b).any(), b
    caps = np.array([255 - ur.bias_of(g['M'], _cb(g, q) if c else None) for q, c in zip(g['pq'], g['comp'])])
    at_cap = g['score'] == caps
    assert (at_cap & (g['comp'] == 1)).sum() > 20 and (at_cap & (g['comp'] == 0)).sum() > 20
    assert len(set(caps[at_cap].tolist())) > 1          # different bias, different ceiling
    assert (g['score'] < caps).sum() > 100
    has_x = np.array([(_seq(g, i) == 20).any() for i in range(len(lens))])
    assert has_x[g['pq']].any() and has_x[g['pt']].any()


def test_numpy_restatement_reproduces_every_golden_score(gold):
    g = gold
    bad = []
    for q, t, c, s in zip(g['pq'], g['pt'], g['comp'], g['score']):
        mine = ur.restate_score(g['M'], _seq(g, q), _seq(g, t), _cb(g, q) if c else None)
        if mine != int(s):
            bad.append((int(q), int(t), int(c), int(s), mine))
    assert not bad, bad[:10]


def test_matrix_restatement_equals_the_pair_restatement(gold):
    g = gold
    rng = np.random.default_rng(3)
    pick = [i for i in rng.permutation(len(g['off']) - 1) if g['off'][i + 1] - g['off'][i] <= 600][:12]
    off = np.zeros(len(pick) + 1, np.uint64)
    np.cumsum([len(_seq(g, i)) for i in pick], out=off[1:])
    res = np.concatenate([_seq(g, i) for i in pick])
    cb = np.concatenate([_cb(g, i) for i in pick])
    full = ur.restate_matrix(g['M'], res, off, cb, res, off)
    for a, i in enumerate(pick):
        for b, j in enumerate(pick):
            assert full[a, b] == ur.restate_score(g['M'], _seq(g, i), _seq(g, j), _cb(g, i)), (i, j)


@pytest.mark.skipif(not ur.have_ref(), reason='oracle/_ref/libsdref.so is built only where the reference tree exists')
def test_live_reference_reproduces_every_golden_score(gold):
    g = gold
    for use_cb in (1, 0):
        ref = ur.RefUngapped(bool(use_cb))
        last = None
        for q, t, c, s in zip(g['pq'], g['pt'], g['comp'], g['score']):
            if c != use_cb:
                continue
            if q != last:
                ref.set_query(_seq(g, q))
                last = q
            assert ref.score(_seq(g, t)) == int(s), (int(q), int(t), use_cb)


def test_list_rule_on_a_hand_made_score_table():
    #          key: 10  11  12  13  14  15  16
    scores = [40, 15, 16, 40, 90, 40, 3]
    keys = [10, 11, 12, 13, 14, 15, 16]
    lens = [100, 100, 100, 100, 100, 100, 100]
    # strictly above the threshold: 15 is out, 16 is in
    assert ur.list_rule(scores, keys, 100, lens) == [(14, 90), (10, 40), (13, 40), (15, 40), (12, 16)]
    # two of the three targets with 40 survive the cut: the smaller keys
    assert ur.list_rule(scores, keys, 100, lens, max_seqs=3) == [(14, 90), (10, 40), (13, 40)]
    assert ur.list_rule(scores, keys, 100, lens, max_seqs=2) == [(14, 90), (10, 40)]
    # the identity pair is a hit whatever it scores, at the place its score gives it
    assert ur.list_rule(scores, keys, 100, lens, identity_key=16) == [(14, 90), (10, 40), (13, 40), (15, 40), (12, 16), (16, 3)]
    assert ur.list_rule(scores, keys, 100, lens, min_score=254, identity_key=11) == [(11, 15)]
    assert ur.list_rule(scores, keys, 100, lens, min_score=0)[-1] == (16, 3)
    # coverage: a pair that cannot be covered is skipped, the identity pair included
    lens2 = [100, 100, 100, 70, 100, 130, 100]
    assert ur.list_rule(scores, keys, 100, lens2, cov_mode=0, cov_thr=0.8) == [(14, 90), (10, 40), (12, 16)]
    assert ur.list_rule(scores, keys, 100, lens2, cov_mode=1, cov_thr=0.8) == [(14, 90), (10, 40), (13, 40), (12, 16)]
    assert ur.list_rule(scores, keys, 100, lens2, cov_mode=2, cov_thr=0.8) == [(14, 90), (10, 40), (15, 40), (12, 16)]
    assert ur.list_rule(scores, keys, 100, lens2, cov_mode=2, cov_thr=0.8, identity_key=13) == [(14, 90), (10, 40), (15, 40), (12, 16)]
    assert ur.list_text([(14, 90), (10, 40)]) == '14\t90\t0\n10\t40\t0\n'


def test_golden_example_lists_are_well_formed(gold):
    g = gold
    max_seqs = int(g['ex_par'][0])
    assert len(g['ex_query']) == 32
    for x in range(len(g['ex_query'])):
        a, b = int(g['ex_off'][x]), int(g['ex_off'][x + 1])
        assert 0 < b - a <= max_seqs
        order = sorted(zip(-g['ex_score'][a:b], g['ex_key'][a:b]))
        assert [(int(k), int(-s)) for s, k in order] == list(zip(g['ex_key'][a:b].tolist(), g['ex_score'][a:b].tolist()))
        assert int(g['ex_query'][x]) in g['ex_key'][a:b]   # same DB on both sides: the identity pair
