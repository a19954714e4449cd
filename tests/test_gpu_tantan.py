"""ib_mask_kernel's float posteriors (csrc/hip/sd_index_build.hip), bit for bit against the reference's own Masker.

The kernel compares its posterior with --mask-prob and writes mask bytes; nothing is read out of it.  With the posteriors of
tests/golden/tantan_vectors.npz (tests/ttgold.py: read from the reference through the same threshold) every expectation here is
`fixture posterior >= threshold`, residue by residue and as a count: a run at (double) v and one at the next float above it, for a
distinct posterior v, pass iff every residue's device posterior lies on the same side of both as the reference's -- over all
distinct v, iff it has the reference's bits.  The runs go through sd_selftest_mask (the masking phase exactly as sd_target_build
calls it, without the 20^k tables of an index) and, for three thresholds, through sd_target_build itself.

What this sees and what it does not (measured with the same check on mutated builds, CPU and MI355X): an error of the size of a
float ulp is caught at once -- one operand of the forward step rounded to float flips 296 of the ladder's 3 372 residues and 777
of set B's 6 009.  A difference in the last bits of the doubles is not: the four partial sums of fwdFull combined as
(s0 + s1) + (s2 + s3) on the device, the same on the host, and a host build without fused multiply-adds each change 0 of the
9 381 posteriors -- a relative 1e-16 reaches a float's rounding boundary about once in 1e9 residues.  So these tests pin indexing,
the ramp and the blocks, rescaling, lane ends, the launch layout and the compare itself, to the bit; they do not tell one
summation order from another, and neither does anything else in the suite.

Seconds per test on an MI355X: full pin 4.1 (5 962 runs; 6.75 with the sequence of 260 residues, which is therefore pinned in the
layouts only), through sd_target_build 1.9, layouts 0.81 (short lanes beside a long one), 0.79 (two long sequences), 0.14 (one
wavefront per launch), 0.10 (no idle lane), < 0.01 (one residue), edge thresholds 0.01 (A) and 0.07 (B), X on input < 0.01."""
import numpy as np
import pytest

import ttgold
from spacedust_amd import api

pytestmark = pytest.mark.gpu


def _lanes(off):
    """where ibMaskPhase puts the sequences: (wavefront of every sequence, longest sequence of every wavefront) -- dealt out by
    length (stable), 64 to a wavefront"""
    lens = (off[1:] - off[:-1]).astype(np.int64)
    order = np.argsort(lens, kind='stable')
    wave = np.zeros(len(lens), np.int64)
    wave[order] = np.arange(len(lens)) // 64
    longest = np.array([lens[wave == w].max() for w in range(int(wave.max()) + 1)])
    return wave, longest


def _run(gpu, host, res, off, post, thr, pair):
    """one run at thr; pair: the (v, up(v)) it belongs to, for the message"""
    want, n = ttgold.expected(res, post, thr)
    got, m = api.mask_on_device(gpu, host, res, off, thr)
    bad = np.nonzero(got != want)[0]
    if len(bad) or m != n:
        wave, longest = _lanes(off)
        rows = []
        for r in bad[:8]:
            s = int(np.searchsorted(off, r, side='right')) - 1
            rows.append(dict(sequence=s, position=int(r - int(off[s])), length=int(off[s + 1] - off[s]), wavefront=int(wave[s]),
                             wavefront_longest=int(longest[wave[s]]), posterior=float(post[r]), masked=bool(got[r] == ttgold.X)))
        pytest.fail('threshold %r of the pair (%r, %r): %d residues differ, %d masked where the fixture gives %d; the first: %s'
                    % (float(thr), float(pair[0]), float(pair[1]), len(bad), m, n, rows))


def _pin(gpu, host, res, off, post, values):
    for v in values:
        u = ttgold.up(v)
        _run(gpu, host, res, off, post, v, (v, u))
        _run(gpu, host, res, off, post, u, (v, u))


def _pinned_ladder():
    """set A without its sequence of 260 residues: with it the full pin took 6.75 s on the MI355X, without it 4.14 s (the 260 are
    pinned at 48 values in the layouts below instead)"""
    return ttgold.concat([x for x in ttgold.sequences('A') if len(x[0]) != 260])


def test_the_ladder_covers_the_kernel_s_cases():
    """what the full pin below pins, from the fixture: every ramp position and the first blocks of four, every phase of a block, a
    rescaling position, and sequence ends inside a wavefront that goes on"""
    res, off, post = _pinned_ladder()
    wave, longest = _lanes(off)
    lens = (off[1:] - off[:-1]).astype(np.int64)
    assert lens.tolist() == list(range(1, 73)) + [100, 127, 128, 129]
    assert wave.max() == 1 and (wave == 1).sum() == 12   # 12 live lanes and 52 without a sequence
    pos = np.concatenate([np.arange(n) for n in lens])
    for p in (0, 49, 50, 51, 52):
        assert (pos == p).any()
    assert {int(x) for x in (pos[pos >= 52] - 52) % 4} == {0, 1, 2, 3}
    assert (pos % 16 == 15).any()
    assert (lens < longest[wave]).sum() == 74     # their last residues are pinned like every other
    # both sides of 0.9 are populated and most residues have a posterior of their own, so a run tells something
    assert 100 < (post >= np.float32(0.9)).sum() < len(post) - 100 and len(np.unique(post)) > 2900


def test_full_pin_of_the_ladder(gpu, host):
    """the ladder as one DB: two wavefronts (lengths 1..64; 65..72, 100, 127, 128, 129 and 52 lanes without a sequence), two runs
    per distinct posterior (5 962 runs): every residue's device posterior has the reference's bits"""
    res, off, post = _pinned_ladder()
    _pin(gpu, host, res, off, post, np.unique(post))


def _with_copies():
    a = ttgold.sequences('A')
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.float32))
    return ttgold.concat(a + [empty] + a[22:72])   # 77 + 1 + 50 copies (lengths 23..72) = two full wavefronts


def _one_wavefront_with_a_long_lane():
    a = ttgold.sequences('A')
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.float32))
    return ttgold.concat(a[:31] + [ttgold.sequences('B')[0]] + a[31:62] + [empty])


LAYOUTS = {
    'one_wavefront_per_launch': lambda: ttgold.seqset('A'),                # SD_INDEX_MASK_BUDGET=1: the second launch has waveBase 1
    'no_idle_lane': _with_copies,                                          # 128 sequences, one of them empty
    'short_lanes_beside_a_long_one': _one_wavefront_with_a_long_lane,      # lengths 0..62 idle through ~2 900 positions of the 64th lane
    'two_long_sequences': lambda: ttgold.seqset('B'),
    'one_residue': lambda: ttgold.concat(ttgold.sequences('A')[:1]),
}


@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_the_same_posteriors_in_other_layouts(gpu, host, monkeypatch, layout):
    res, off, post = LAYOUTS[layout]()
    n = len(off) - 1
    assert n == {'one_wavefront_per_launch': 77, 'no_idle_lane': 128, 'short_lanes_beside_a_long_one': 64, 'two_long_sequences': 2,
                 'one_residue': 1}[layout]
    if layout == 'one_wavefront_per_launch':
        monkeypatch.setenv('SD_INDEX_MASK_BUDGET', '1')
    values = ttgold.pick(post, 48)
    assert len(values) == min(48, len(np.unique(post)))
    _pin(gpu, host, res, off, post, values)


@pytest.mark.parametrize('name', ['A', 'B'])
def test_edge_thresholds(gpu, host, name):
    res, off, post = ttgold.seqset(name)
    for thr in ttgold.edge_thresholds():
        _run(gpu, host, res, off, post, thr, (thr, thr))


def test_x_on_input(gpu, host):
    """an X stays X at every threshold and counts where its posterior reaches the threshold (nX of ib_mask_kernel)"""
    res, off, masks, counts = ttgold.set_c()
    for k, thr in enumerate(ttgold.C_THRESHOLDS):
        got, n = api.mask_on_device(gpu, host, res, off, thr)
        bad = np.nonzero(got != masks[k])[0]
        assert len(bad) == 0 and n == int(counts[k].sum()), (thr, bad[:8], n, int(counts[k].sum()))


def test_mask_prob_through_sd_target_build(gpu, host, oracle):
    """the production entry at thresholds other than 0.9: masked bytes, count and index entries; at 0.5 the prefilter on that target"""
    res, off, post = ttgold.seqset('A')
    v = np.unique(post[(post > 0.3) & (post < 0.6)])[0]
    counts = {}
    for thr in (0.5, float(v), float(ttgold.up(v))):
        want, n = ttgold.expected(res, post, thr)
        t = api.Target.build_on_device(gpu, host, res, off, k=6, kmer_thr=0, mask_prob=thr)
        dev = t.download()
        assert t.build_stats['masked_residues'] == n and np.array_equal(dev['masked'], want), thr
        h = host.build_index(res, off, k=6, kmer_thr=0, mask_prob=thr)
        assert h.masked_residues == n and dev['n_entries'] == h.n_entries
        assert np.array_equal(dev['starts'], h.kmer_offsets.astype(np.uint64))
        assert np.array_equal(dev['entry_seq'], h.entry_seq) and np.array_equal(dev['entry_pos'], h.entry_pos)
        counts[thr] = n
        if thr != 0.5:
            continue
        qs = [i for i in range(len(off) - 1) if int(off[i + 1] - off[i]) >= 30]
        q = ttgold.concat([ttgold.sequences('A')[i] for i in qs])
        _, dg_b, km_b = host.comp_bias(q[0], q[1])
        par = api.prefilter_params(host, len(off) - 1, max_hits=50, cov_thr=0.0, bin_size=2)
        hits, cnt, _ = api.prefilter(gpu, t, par, q[0], q[1], km_b, dg_b, np.array(qs, np.uint32))
        ot = oracle.target(res, off, k=6, kmer_thr=0, mask_prob=0.5)
        assert ot.masked_residues == n
        total = 0
        for x, i in enumerate(qs):
            ids, sc, dg, _ = ot.prefilter(ttgold.sequences('A')[i][0], identity_id=i, max_hits=50, bin_size=2)
            m = int(cnt[x])
            assert m == len(ids), (i, m, len(ids))
            assert (hits[x, :m]['seqId'] == ids).all() and (hits[x, :m]['score'] == sc).all() and (hits[x, :m]['diagonal'] == dg).all(), i
            total += m
        assert total >= len(qs)
    assert len(set(counts.values())) == 3 and ttgold.expected(res, post, 0.9)[1] not in counts.values()
