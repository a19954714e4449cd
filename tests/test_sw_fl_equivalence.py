"""CPU: the premise of the packed score kernels without the lane-structure F chain (sd_sw_pk.h).

The reference's striped kernels carry, beside the exact vertical gap Ff, a vertical gap Fl that may only have started inside
the same SIMD segment.  Fl feeds Hpre only; results are read from G = max(Hpre, Ff).  For go >= ge every path through an Fl
value (a vertical gap, then possibly a horizontal one opened from it) has a twin with the two gaps in the other order that
costs the same and runs through Ff, so G does not depend on Fl -- nor on the segment length, i.e. on the lane count.  Checked
here against the scalar model of tests/flgen.py, against the oracle's restated striped pass (pinned on the compiled reference
by tests/test_oracle_golden.py) and, where it has been built, against the reference library itself."""
import numpy as np
import pytest

import flgen

SEG_LENS = (1, 2, 3, 5, 8)


def _prof(mat, q, bias=None):
    p = np.asarray(mat, np.int64)[:, np.asarray(q, np.int64)]
    return p if bias is None else p + np.asarray(bias, np.int64)[None, :]


def _cases():
    """(profile [alphabet or 21][n], target, go, ge): random pairs under random matrices of alphabets 4 / 6 / 20, the same under
    position-specific tables, and small F-then-E pairs, every gap cost of flgen.GAPS in turn"""
    rng = np.random.default_rng(4711)
    out = []
    for x in range(420):
        alphabet = (4, 6, 20)[x % 3]
        go, ge = flgen.GAPS[x % len(flgen.GAPS)]
        kind = x % 4
        if kind == 3:
            q, t, _, _ = flgen.fte_small(rng, alphabet)
        else:
            q, t = flgen.random_pair(rng, alphabet, 5, 48)
        if kind == 2:   # profile style: every position its own column of scores, loosely tied to the residue
            prof = _prof(flgen.random_matrix(rng, alphabet), q) + rng.integers(-2, 3, (alphabet, len(q)))
        else:
            prof = _prof(flgen.random_matrix(rng, alphabet), q)
        out.append((prof, t, go, ge))
    return out


@pytest.fixture(scope='module')
def cases():
    return _cases()


def test_g_is_independent_of_fl(cases):
    """the full G matrices with Fl (segments of 1, 2, 3, 5, 8 rows and of the reference's ceil(n / 32)) and without are equal
    in every cell; the column-at-a-time form used for the long pairs equals the cell-by-cell model"""
    n_hpre = 0
    for prof, t, go, ge in cases:
        G0, H0, E0 = flgen.model(prof, t, go, ge, None)
        Gn, Hn, En = flgen.model_np(prof, t, go, ge, None)
        assert (G0 == Gn).all() and (H0 == Hn).all() and (E0 == En).all()
        for seg in SEG_LENS + (max(1, (prof.shape[1] + 31) // 32),):
            G1, H1, E1 = flgen.model(prof, t, go, ge, seg)
            assert (G1 == G0).all(), (seg, go, ge)
            assert (H1 >= H0).all() and (E1 >= E0).all()
            n_hpre += int((H1 != H0).any())
            if seg in (3, 8):
                Gn, Hn, En = flgen.model_np(prof, t, go, ge, seg)
                assert (G1 == Gn).all() and (H1 == Hn).all() and (E1 == En).all()
    assert len(cases) >= 400 and n_hpre > len(cases)   # (the removed term was at work in most of them)


def test_premise_fails_below_ge():
    """go < ge is outside the claim -- the kernels' F update itself needs go >= ge -- and the dispatch keeps such calls on the
    int32 kernel; the model shows at least one pair where dropping Fl changes G there, so the guard is not decoration"""
    rng = np.random.default_rng(5)
    differs = 0
    for _ in range(60):
        q, t, _, _ = flgen.fte_small(rng, 6)
        prof = _prof(flgen.random_matrix(rng, 6), q)
        G0, _, _ = flgen.model(prof, t, 1, 3, None)
        G1, _, _ = flgen.model(prof, t, 1, 3, 8)
        differs += int((G0 != G1).any())
    assert differs > 0


def test_oracle_pass_is_independent_of_the_lane_count(oracle, cases):
    """oracle.sw_pass (the restated striped pass, Fl included) returns the same (score, target end, query end) with 32, 16 and
    1 lanes -- segments of ceil(n / 32), ceil(n / 16) and n rows -- and they are what the model without Fl gives"""
    for prof, t, go, ge in cases:
        ref = [oracle.sw_pass(prof, t, lanes, go=go, ge=ge) for lanes in (32, 16, 1)]
        assert ref[0] == ref[1] == ref[2], (ref, go, ge)
        G0, _, _ = flgen.model(prof, t, go, ge, None)
        assert ref[0] == flgen.best(G0), (ref[0], flgen.best(G0))


@pytest.fixture(scope='module')
def fte(oracle, host):
    letters, pairs = flgen.fte_pairs()
    seqs = [oracle.map_sequence(s) for s in letters]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    bias, _, _ = host.comp_bias(np.concatenate(seqs), off)
    mat = oracle.matrix(0)[0]
    bias = [bias[int(off[i]):int(off[i + 1])] for i in range(len(seqs))]
    return letters, seqs, bias, mat, pairs


def _uses_fl(prof, t, seg):
    G0, H0, E0 = flgen.model_np(prof, t, 11, 1, None)
    G1, H1, E1 = flgen.model_np(prof, t, 11, 1, seg)
    return (G0 == G1).all(), int((H0 != H1).sum()), int((E0 != E1).sum()), G0


def test_constructed_pairs_exercise_the_removed_term(fte):
    """every F-then-E pair of flgen.fte_pairs (the pairs of tests/test_gpu_sw_fl.py), with the composition-bias corrected
    BLOSUM62 profile the GPU test runs on: in the forward pass (segments of the byte and of the word kernel) and in the
    start-position pass (the reversed prefixes up to the end cell) Hpre and E differ between the two models in at least one
    cell each, while G differs in none.  The straddling pairs hold their vertical gap across row 512 / 1024."""
    letters, seqs, bias, mat, pairs = fte
    assert len(pairs) >= 12
    for name, qi, ti in pairs:
        q, t = seqs[qi], seqs[ti]
        prof = _prof(mat, q, bias[qi])
        for lanes in (32, 16):
            same, dh, de, G = _uses_fl(prof, t, (len(q) + lanes - 1) // lanes)
            assert same and dh > 0 and de > 0, (name, lanes, same, dh, de)
        if len(q) <= 300:   # the cell-by-cell model itself where it is quick
            seg = (len(q) + 31) // 32
            (G0, H0, _), (G1, H1, _) = flgen.model(prof, t, 11, 1, None), flgen.model(prof, t, 11, 1, seg)
            assert (G0 == G1).all() and (H0 != H1).any() and (G0 == G).all(), name
        score, t_end, q_end = flgen.best(G)
        rprof, rt = prof[:, q_end::-1], t[t_end::-1]
        for lanes in (32, 16):
            same, dh, de, Gr = _uses_fl(rprof, rt, (q_end + 1 + lanes - 1) // lanes)
            assert same and dh > 0 and de > 0, (name, 'start positions', lanes, same, dh, de)
        assert int(Gr.max()) == score
    spec = {s[0]: s for s in flgen.FTE_SPECS}
    for name, boundary in (('strips2', 512), ('strips3', 1024), ('wide_strips', 512)):
        _, n, gap_row, k, _, _, _, _ = spec[name]
        assert gap_row - 1 < boundary <= gap_row + k - 1 and n > boundary


def test_constructed_pairs_byte_and_word_split(oracle, fte):
    """the oracle's rows of the constructed pairs: the `wide` ones, and only they, leave the byte range (word flag), which is
    what sends them to the wide kernels; every pair aligns across its gaps"""
    letters, seqs, bias, mat, pairs = fte
    db = int(sum(len(s) for s in seqs))
    spec = {s[0]: s for s in flgen.FTE_SPECS}
    for name, qi, ti in pairs:
        o = oracle.sw_align(seqs[qi], seqs[ti], db, cov_thr=0.0)
        assert (o['flags'] & 1) == int(name.startswith('wide')), (name, o['score'])
        _, n, gap_row, k, _, _, _, _ = spec[name.split('/')[0]]
        assert o['qStart'] < gap_row - 1 and o['qEnd'] > gap_row + k and o['btLen'] > 0, (name, o)


def test_reference_library_agrees(oracle, fte):
    """where oracle/_ref/libsdref.so was built: the compiled reference (its striped kernels with their own lane structure)
    gives the score and the end positions of the model without Fl, on the constructed pairs and on random protein pairs"""
    from oracle import pyoracle
    if not pyoracle.ref_available():
        pytest.skip('oracle/_ref/libsdref.so has not been built')
    letters, seqs, bias, mat, pairs = fte
    ref = pyoracle.Ref()
    db = int(sum(len(s) for s in seqs))
    sw = pyoracle.RefSW(ref, 4096, db, comp_bias=False)
    todo = [(letters[qi], letters[ti]) for _, qi, ti in pairs]
    rng = np.random.default_rng(77)
    for _ in range(60):
        q, t = flgen.random_pair(rng, 20, 30, 200)
        todo.append((''.join(flgen.AA[int(x)] for x in q), ''.join(flgen.AA[int(x)] for x in t)))
    for ql, tl in todo:
        sw.set_query(ql)
        r = sw.align(tl, sw_mode=1, eval_thr=1e30, cov_thr=0.0)
        q, t = oracle.map_sequence(ql), oracle.map_sequence(tl)
        G0, _, _ = flgen.model_np(_prof(mat, q), t, 11, 1, None)
        assert (r['score'], r['tEnd'], r['qEnd']) == flgen.best(G0), (r, flgen.best(G0))
