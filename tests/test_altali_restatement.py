"""tests/altali_ref.py (the plain-Python restatement of Alignment::computeAlternativeAlignment) around the scalar oracle's
Smith-Waterman reproduces every case of tests/golden/altali_vectors.npz, which the reference's own matcher wrote; where the
reference build is present the loop is also run around the live matcher."""
import numpy as np
import pytest

import altali_ref as ar


@pytest.fixture(scope='module')
def gold():
    return ar.load()


def test_golden_set_holds_the_cases_the_feature_is_about(gold):
    g = gold
    assert 120 <= len(g['cases']) <= 200
    assert {'copies2', 'copies3', 'copies4', 'single', 'identity', 'start0', 'endlast', 'exclusive', 'saturate', 'tie', 'queryx'} <= set(g['cls'])
    assert all(60 <= len(g['seqs'][c[0]]) for c in g['cases']) and max(len(s) for s in g['seqs']) <= 900
    n_of = {c[3] for c in g['cases']}
    assert {1, 2, 3, 10} <= n_of
    by_n = sum(1 for c, w in zip(g['cases'], g['want']) if not c[4] and len(w) == c[3])
    by_reject = sum(1 for c, w in zip(g['cases'], g['want']) if not c[4] and len(w) < c[3])
    assert by_n > 10 and by_reject > 10
    assert any(not c[4] and len(w) == 0 for c, w in zip(g['cases'], g['want']))                 # first alternative rejected
    assert all(len(w) == 0 for c, w in zip(g['cases'], g['want']) if c[4]) and any(c[4] for c in g['cases'])
    assert any(s[0] == 0 for s, c in zip(g['seeds'], g['cases']) if not c[4])
    assert any(s[1] == len(g['seqs'][c[1]]) - 1 for s, c in zip(g['seeds'], g['cases']) if not c[4])
    assert any(r['score'] >= 255 for w in g['want'] for r in w)                                 # a masked round on the word kernel
    assert any(len({r['score'] for r in w}) < len(w) for w in g['want'])                        # equal scores within one target
    assert {g['params'][c[2]]['sw_mode'] for c in g['cases']} == {1, 2}
    assert any(b'X' in g['seqs'][c[0]] and w for c, w in zip(g['cases'], g['want']))


def test_exclusive_end_is_what_the_golden_cases_need(gold, oracle):
    """masking [tStart, tEnd] inclusive instead of [tStart, tEnd) changes at least one golden case: the set can tell the two apart"""
    g = gold
    changed = 0
    for (qi, ti, pi, n, ident), seed, want in zip(g['cases'], g['seeds'], g['want']):
        if ident:
            continue
        p = g['params'][pi]
        q, t = oracle.map_sequence(g['seqs'][qi]), oracle.map_sequence(g['seqs'][ti])

        def align(num, q=q, p=p):
            return oracle.sw_align(q, num, g['db_residues'], sw_mode=p['sw_mode'], eval_thr=p['eval_thr'], cov_mode=p['cov_mode'], cov_thr=p['cov_thr'])
        got = ar.alternatives(align, t, seed[0], seed[1] + 1, n, len(q), p)
        changed += len(got) != len(want) or any(not ar.same(a, b) for a, b in zip(got, want))
    print('an inclusive end changes', changed, 'cases')
    assert changed >= 1


def test_restatement_around_the_oracle_equals_every_golden_case(gold, oracle):
    g = gold
    bad = []
    for ci, ((qi, ti, pi, n, ident), seed, want) in enumerate(zip(g['cases'], g['seeds'], g['want'])):
        p = g['params'][pi]
        q, t = oracle.map_sequence(g['seqs'][qi]), oracle.map_sequence(g['seqs'][ti])

        def align(num, q=q, p=p):
            r = oracle.sw_align(q, num, g['db_residues'], sw_mode=p['sw_mode'], eval_thr=p['eval_thr'], cov_mode=p['cov_mode'], cov_thr=p['cov_thr'])
            if r['btLen'] <= 0:
                r['identical'] = 0
            return r
        got = ar.alternatives(align, t, seed[0], seed[1], n, len(q), p, identity=bool(ident))
        if len(got) != len(want) or any(not ar.same(a, b) for a, b in zip(got, want)):
            bad.append((ci, g['cls'][ci], len(got), len(want)))
    print('%d cases, %d alternatives, %d mismatches' % (len(g['cases']), sum(len(w) for w in g['want']), len(bad)))
    assert not bad, bad[:8]


def test_restatement_around_the_live_reference_equals_every_golden_case(gold):
    from oracle.pyoracle import ref_available
    if not ref_available():
        pytest.skip('the reference build (oracle/_ref/libsdref.so) is not present')
    from oracle.pyoracle import Ref, RefSW
    g = gold
    sw = RefSW(Ref(6), 1200, g['db_residues'])
    bad = []
    for ci, ((qi, ti, pi, n, ident), seed, want) in enumerate(zip(g['cases'], g['seeds'], g['want'])):
        p = g['params'][pi]
        t = g['seqs'][ti]
        sw.set_query(g['seqs'][qi])

        def align(num, t=t, p=p):
            masked = bytes(ord('X') if c == ar.X else a for a, c in zip(t, num))
            r = sw.align(masked, sw_mode=p['sw_mode'], eval_thr=p['eval_thr'], cov_mode=p['cov_mode'], cov_thr=p['cov_thr'])
            if r['btLen'] <= 0:
                r['identical'] = 0
            return r
        got = ar.alternatives(align, np.zeros(len(t), np.uint8), seed[0], seed[1], n, len(g['seqs'][qi]), p, identity=bool(ident))
        if len(got) != len(want) or any(not ar.same(a, b) for a, b in zip(got, want)):
            bad.append((ci, g['cls'][ci], len(got), len(want)))
    assert not bad, bad[:8]


def test_round_by_round_restatement_equals_the_seed_by_seed_one(gold, oracle):
    """alternatives_many (what the module tests drive with a batch aligner) gives what alternatives gives, on every golden case"""
    g = gold
    for pi, p in enumerate(g['params']):
        for n in sorted({c[3] for c in g['cases'] if c[2] == pi}):
            idx = [i for i, c in enumerate(g['cases']) if c[2] == pi and c[3] == n and not c[4]]
            qs = [oracle.map_sequence(g['seqs'][g['cases'][i][0]]) for i in idx]
            ts = [oracle.map_sequence(g['seqs'][g['cases'][i][1]]) for i in idx]

            def align_many(seeds, masked):
                out = []
                for s, m in zip(seeds, masked):
                    r = oracle.sw_align(qs[s], m, g['db_residues'], sw_mode=p['sw_mode'], eval_thr=p['eval_thr'], cov_mode=p['cov_mode'],
                                        cov_thr=p['cov_thr'])
                    if r['btLen'] <= 0:
                        r['identical'] = 0
                    out.append(r)
                return out
            got = ar.alternatives_many(align_many, ts, [g['seeds'][i] for i in idx], n, [len(q) for q in qs], p)
            for i, rows in zip(idx, got):
                assert len(rows) == len(g['want'][i]) and all(ar.same(a, b) for a, b in zip(rows, g['want'][i])), (i, g['cls'][i])
