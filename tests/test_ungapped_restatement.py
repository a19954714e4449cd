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


def test_list_rule_fast_equals_list_rule():
    """the vectorised list rule of the 10^6-target tests against the plain one: heavy score ties, every coverage mode, keys
    above 2^31, the cut at, before and behind the edge of a tie class, the identity pair above and below the threshold"""
    rng = np.random.default_rng(8)
    rows = 3000
    seen_modes, seen_ident, seen_edge, seen_high = set(), set(), set(), 0
    for x in range(rows):
        n = int(rng.integers(1, 120))
        scores = rng.choice([0, 3, 15, 16, 17, 40, 40, 40, 90, 255], n)                        # few values: large tie classes
        keys = rng.choice(np.arange(1 << 12, dtype=np.uint64) * ((1 << 20) + 7) % (1 << 32), n, replace=False).astype(np.uint32)
        t_lens = rng.choice([0, 1, 40, 50, 64, 80, 99, 100, 101, 125, 200], n)
        q_len = int(rng.choice([0, 1, 50, 80, 100, 125]))
        mode = int(rng.integers(0, 7))                                                         # 6: no coverage rule
        thr = float(rng.choice([0.0, 0.5, 0.8, 1.0]))
        min_score = int(rng.choice([0, 15, 16, 254]))
        idk = None if x % 3 == 0 else int(keys[int(rng.integers(0, n))])
        whole = ur.list_rule(scores, keys, q_len, t_lens, min_score=min_score, max_seqs=n + 5, cov_mode=mode, cov_thr=thr, identity_key=idk)
        # the edge of a tie class: the number of hits down to the end of a score class that has more hits behind it
        ends = [i + 1 for i in range(len(whole) - 1) if whole[i][1] != whole[i + 1][1]]
        edge = int(rng.choice(ends)) if ends else max(1, len(whole))
        for max_seqs in {1, max(1, edge - 1), edge, edge + 1, n + 5}:
            exp = whole[:max_seqs]
            k, s = ur.list_rule_fast(scores, keys, q_len, t_lens, min_score=min_score, max_seqs=max_seqs, cov_mode=mode, cov_thr=thr,
                                     identity_key=idk)
            assert k.dtype == np.uint32 and list(zip(k.tolist(), s.tolist())) == exp, (x, max_seqs)
            assert exp == ur.list_rule(scores, keys, q_len, t_lens, min_score=min_score, max_seqs=max_seqs, cov_mode=mode, cov_thr=thr,
                                       identity_key=idk)
            if ends and max_seqs in (edge - 1, edge, edge + 1) and max_seqs < len(whole):
                seen_edge.add(max_seqs - edge)
        seen_modes.add(mode)
        seen_high += bool((keys >= 1 << 31).any())
        if idk is not None and any(kk == idk for kk, _ in whole):
            seen_ident.add(int(scores[list(keys).index(idk)]) > min_score)
    assert seen_modes == set(range(7)) and seen_ident == {True, False} and seen_edge == {-1, 0, 1} and seen_high > rows // 2
    # the mask itself, pair by pair, zero lengths included
    for mode in range(7):
        for thr in (0.0, 0.5, 0.8, 1.0):
            for q_len in (0, 1, 80, 100):
                t_lens = np.array([0, 1, 64, 79, 80, 81, 100, 125, 126])
                assert ur.covered_mask(thr, mode, q_len, t_lens).tolist() == [ur.can_be_covered(thr, mode, q_len, t) for t in t_lens]


def test_expand_pooled_equals_the_direct_restatement(gold):
    g = gold
    rng = np.random.default_rng(4)
    ids = [i for i in rng.permutation(len(g['off']) - 1) if g['off'][i + 1] - g['off'][i] <= 300][:10]

    def packed(which):
        off = np.zeros(len(which) + 1, np.uint64)
        np.cumsum([len(_seq(g, i)) for i in which], out=off[1:])
        return np.concatenate([_seq(g, i) for i in which]), off, np.concatenate([_cb(g, i) for i in which])
    q_res, q_off, q_cb = packed(ids[:4])
    p_res, p_off, _ = packed(ids[4:])
    pool_id = rng.integers(0, 6, 40)
    t_res, t_off, _ = packed([ids[4 + p] for p in pool_id])
    small = ur.restate_matrix(g['M'], q_res, q_off, q_cb, p_res, p_off)
    direct = ur.restate_matrix(g['M'], q_res, q_off, q_cb, t_res, t_off)
    assert len(set(pool_id.tolist())) == 6 and direct.max() > 0
    assert np.array_equal(ur.expand_pooled(small, pool_id), direct)
    assert np.array_equal(ur.expand_pooled(small[2], pool_id), direct[2])


def test_golden_paths_file_holds_the_restatement():
    """tests/golden/ungapped_paths.npz (tools/make_golden_ungapped_paths.py): a sample of its rows recomputed; the GPU test
    compares all of them"""
    import os
    g = np.load(os.path.join(ur.ROOT, 'tests', 'golden', 'ungapped_paths.npz'))
    q_len = (g['q_off'][1:] - g['q_off'][:-1]).astype(np.int64)
    assert g['score_cb'].shape == g['score_nocb'].shape == (len(q_len), len(g['t_off']) - 1) and q_len.max() > 1536
    for q in (int(np.argmin(q_len)), int(np.flatnonzero(q_len == 1025)[0]), int(np.argmax(q_len))):   # two, three, four strips
        a, b = int(g['q_off'][q]), int(g['q_off'][q + 1])
        off = np.array([0, b - a], np.uint64)
        assert np.array_equal(ur.restate_matrix(g['M'], g['q_res'][a:b], off, g['q_cb'][a:b], g['t_res'], g['t_off'])[0], g['score_cb'][q])
        assert np.array_equal(ur.restate_matrix(g['M'], g['q_res'][a:b], off, None, g['t_res'], g['t_off'])[0], g['score_nocb'][q])
