"""CPU: the restatement tests/kmm_ref.py and the host stages of `kmermatcher` (sd_host_reduced_alphabet, sd_host_kmermatch_auto_k,
sd_host_kmermatch_format) against what tools/make_golden_kmermatch.py recorded from the reference's own object code
(tests/golden/kmermatch_vectors.npz), and the module's refusals."""
import ctypes as C

import numpy as np
import pytest

import kmm_ref
import kmmgold
from dbutil import sdgpu, write_db
from spacedust_amd import _lib, api


@pytest.fixture(scope='module')
def prob():
    buf = C.create_string_buffer(1 << 16)
    L = _lib.load()
    L.sd_host_matrix_text.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    L.sd_host_matrix_text(0, buf, 1 << 16)
    return kmm_ref.matrix_prob(buf.value.decode())


def test_letter_maps_equal_the_reference(prob):
    seen = set()
    for tag in kmmgold.ALL_RUNS:
        size = kmmgold.par(tag)['alph_size']
        want = kmmgold.letter_map(tag)
        got, reduced = api.reduced_alphabet(size)
        assert np.array_equal(got, want) and reduced == size and int(want.max()) == size - 1 and int(want[20]) == size - 1
        if size not in seen:   # (the restatement walks every pair of every step in Python: once per size)
            assert np.array_equal(kmm_ref.reduced_alphabet(prob, size), want)
        seen.add(size)
    assert seen == {13, 21}
    # the thirteen classes the reference prints for blosum62: (A S T) (C) (D N) (E Q) (F Y) (G) (H) (I V) (K R) (L M) (P) (W) (X)
    m = dict(zip(kmmgold.LETTERS, api.reduced_alphabet(13)[0].tolist()))
    assert m['A'] == m['S'] == m['T'] and m['D'] == m['N'] and m['E'] == m['Q'] and m['F'] == m['Y'] and m['I'] == m['V']
    assert m['K'] == m['R'] and m['L'] == m['M'] and len({m[c] for c in 'CGHPWX'} | {m['A'], m['D'], m['E'], m['F'], m['I'], m['K'], m['L']}) == 13


def test_reduced_alphabet_refuses_other_sizes():
    L = _lib.load()
    out = np.zeros(21, np.uint8)
    assert L.sd_host_reduced_alphabet(0, 22, _lib.ptr(out), None) == _lib.SD_EINVAL
    assert L.sd_host_reduced_alphabet(0, 1, _lib.ptr(out), None) == _lib.SD_EINVAL
    assert L.sd_host_reduced_alphabet(2, 13, _lib.ptr(out), None) == _lib.SD_EINVAL


def test_auto_k_is_the_recorded_one():
    total = int(kmmgold.sequences('A')[1][-1])
    for r, m in ((4, 0.5), (5, 0.9), (6, 1.0)):
        p = kmmgold.par('A_r%d' % r)
        assert api.kmermatch_auto_k(m, total) == (p['k'], p['alph_size']) == kmm_ref.auto_k(m, total)
    assert [kmmgold.par('A_r%d' % r)['alph_size'] for r in (4, 5, 6)] == [13, 13, 21]
    p = kmmgold.par('C1_r0')
    assert api.kmermatch_auto_k(0.0, int(kmmgold.sequences('C1')[1][-1])) == (p['k'], 13)
    # the rule's float arithmetic on either side of a step of the logarithm
    for residues in (10 ** 9, 8.7 ** 11 - 1e5, 8.7 ** 11 + 1e5, 2 * 10 ** 11):
        assert api.kmermatch_auto_k(0.0, int(residues)) == kmm_ref.auto_k(0.0, int(residues))


def test_kmer_considered_rounds_the_product_before_the_sum():
    """sd_host_kmermatch_considered against float32 arithmetic with the product rounded first, as kmm_ref.records has it"""
    L = _lib.load()
    rng = np.random.default_rng(23)
    cases = [(20, 0.0, 300), (1, 0.0, 50), (20, 0.013, 90), (20, 0.05, 32767), (2000, 0.0, 3000)]
    cases += [(int(rng.integers(1, 60)), float(np.float32(rng.uniform(0, 1))), int(rng.integers(0, 40000))) for _ in range(20000)]
    for kps, scale, length in cases:
        want = np.float32(kps - 1) + np.float32(scale) * np.float32(length)
        assert L.sd_host_kmermatch_considered(kps, scale, length) == (int(want) if want > 0 else 0), (kps, scale, length)


@pytest.mark.parametrize('tag', kmmgold.ALL_RUNS)
def test_restatement_equals_the_reference(tag):
    name = tag.split('_')[0]
    res, off = kmmgold.sequences(name)
    par, keys = kmmgold.par(tag), kmmgold.keys(tag)
    hits, stats, rec = kmm_ref.kmermatch(par, res, off, keys, kmmgold.letter_map(tag))
    if name != 'C1':
        want_key, want_pos, want_off = kmmgold.records(tag)
        order = np.argsort(keys, kind='stable')
        got_key = np.concatenate([rec[0][rec[4][i]:rec[4][i + 1]] for i in order])
        got_pos = np.concatenate([rec[3][rec[4][i]:rec[4][i + 1]] for i in order])
        assert np.array_equal(np.concatenate([[0], np.cumsum(np.diff(rec[4])[order])]), want_off.astype(np.int64))
        assert np.array_equal(got_key, want_key) and np.array_equal(got_pos, want_pos)
    want = kmmgold.entries(tag)
    assert kmm_ref.entries(keys, hits) == want
    assert sorted(want) == sorted(int(k) for k in keys)          # every sequence has its entry
    assert stats['hits'] == len(kmmgold.hits_of(want))


@pytest.mark.parametrize('tag', kmmgold.SMALL_RUNS)
def test_entry_formatter_equals_the_reference(tag):
    want = kmmgold.entries(tag)
    res, off = kmmgold.sequences(tag.split('_')[0])
    keys = kmmgold.keys(tag)
    hits = kmm_ref.kmermatch(kmmgold.par(tag), res, off, keys, kmmgold.letter_map(tag))[0]
    assert api.kmermatch_format(keys, hits[:, 0], hits[:, 1], hits[:, 2], hits[:, 3].astype(np.int32)) == want


def test_entry_formatter_prints_the_diagonal_through_a_short():
    got = api.kmermatch_format([5, 2], [2, 2], [5, 9], [3, 1], np.array([40000, -40000], np.int32))
    assert got == {2: b'2\t0\t0\n5\t3\t-25536\n9\t1\t25536\n', 5: b'5\t0\t0\n'}
    L = _lib.load()
    nbytes = C.c_uint64()
    one = np.array([7], np.uint32)
    # a representative that is no sequence of the DB
    assert L.sd_host_kmermatch_format(1, _lib.ptr(one), 1, _lib.ptr(np.array([8], np.uint32)), _lib.ptr(one), _lib.ptr(one),
                                      _lib.ptr(np.zeros(1, np.int32)), None, None, 0, None, C.byref(nbytes)) == _lib.SD_EINVAL


REFUSED = [('--mask', '1', '--mask 1'), ('--spaced-kmer-mode', '1', '--spaced-kmer-mode 1'), ('--spaced-kmer-pattern', '1101', '--spaced-kmer-pattern'),
           ('--ignore-multi-kmer', '1', '--ignore-multi-kmer'), ('--weights', 'w.tsv', '--weights'), ('--adjust-kmer-len', '1', '--adjust-kmer-len'),
           ('--compressed', '1', '--compressed 1'), ('--world-size', '2', 'one rank')]


@pytest.mark.parametrize('flag,value,named', REFUSED)
def test_module_refuses_by_name(tmp_path, flag, value, named):
    seq = str(tmp_path / 'seq')
    write_db(seq, [(0, b'MKVLAAGIVGLLLAQ\n')], 0)
    p = sdgpu('kmermatcher', seq, tmp_path / 'out', flag, value, check=False)
    assert p.returncode != 0 and named in p.stderr + p.stdout


@pytest.mark.parametrize('dbtype,named', [(1, 'nucleotide'), (2, 'profile')])
def test_module_refuses_other_db_types(tmp_path, dbtype, named):
    seq = str(tmp_path / 'seq')
    write_db(seq, [(0, b'ACGTACGTACGTACGT\n')], dbtype)
    p = sdgpu('kmermatcher', seq, tmp_path / 'out', check=False)
    assert p.returncode != 0 and named in p.stderr + p.stdout


def test_help_lists_the_module():
    assert 'kmermatcher' in sdgpu('--help').stdout
