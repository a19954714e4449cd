"""Host side of `clust` (no GPU): the restatement of the graph half (tests/clust_ref.py), the parser and the three algorithms against the
reference's own graphs and clusterings (tests/golden/clust_vectors.npz, tools/make_golden_clust.py), `sdgpu clust --cluster-mode 2 / 3` on
DB files, and what the module and the C ABI declare or refuse without a device."""
import numpy as np
import pytest

import clust_ref
import clustgold
from dbutil import read_db, sdgpu, write_db
from spacedust_amd import _lib, api


@pytest.mark.parametrize('t', [1, 2])
@pytest.mark.parametrize('name', clustgold.SETS)
def test_parser_gives_the_reference_rows(name, t):
    keys, entries = clustgold.local(name)
    got = api.clust_parse(keys, entries, clustgold.inputs(name)[3], t)
    for g, w in zip(got, clustgold.input_rows(name, t)):
        assert np.array_equal(g, w)


@pytest.mark.parametrize('t', [1, 2])
@pytest.mark.parametrize('name', clustgold.SETS)
def test_restatement_reproduces_the_reference_graph(name, t):
    got = clust_ref.symmetrize(*clustgold.input_rows(name, t))
    want = clustgold.graph(name, t)
    assert len(want[1]) > 0
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_constructed_classes_are_what_they_are_named():
    g = clustgold.golden()
    classes = dict(zip(g['K_class_names'].tolist(), g['K_class_keys'].tolist()))
    keys, entries = clustgold.local('K_aln')
    id_of = {int(k): i for i, k in enumerate(keys)}
    off, elem, score = clustgold.graph('K_aln', 1)
    row = lambda c: (elem[int(off[id_of[classes[c]]]):int(off[id_of[classes[c]] + 1])].tolist(),
                     score[int(off[id_of[classes[c]]]):int(off[id_of[classes[c]] + 1])].tolist())
    me = lambda c: id_of[classes[c]]
    assert entries[me('empty')] == b'' and row('empty') == ([me('empty')], [65535])
    assert row('self_only')[0] == [me('self_only')]
    assert me('not_listing_itself') not in row('not_listing_itself')[0]
    a = me('one_way')
    b = row('one_way')[0][1]
    assert elem[int(off[b]):int(off[b + 1])].tolist() == [b, a] and score[int(off[b + 1]) - 1] == 123   # the score travels
    a = me('two_way_different_scores')
    b = row('two_way_different_scores')[0][1]
    assert row('two_way_different_scores') == ([a, b], [100, 300]) and score[int(off[b]):int(off[b + 1])].tolist() == [100, 200]
    a = me('target_twice')
    b = row('target_twice')[0][1]
    assert row('target_twice')[0] == [a, b, b] and elem[int(off[b]):int(off[b + 1])].tolist() == [b, a, a]
    assert score[int(off[b]):int(off[b + 1])].tolist() == [100, 50, 60]
    assert len(row('already_symmetric')[0]) == 3
    assert row('short_cast')[1] == [100, 32767, 32768, 40000]
    off2, _, score2 = clustgold.graph('K_aln', 2)
    a = me('seq_id_rounding')
    assert score2[int(off2[a]):int(off2[a + 1])].tolist() == [500, 290, 570, 1000]
    assert int(off[me('hub') + 1] - off[me('hub')]) == 5000
    lens = dict(zip(g['K_keys'].tolist(), g['K_lens'].tolist()))
    assert lens[classes['equal_lengths']] == lens[classes['equal_lengths'] + 3]
    # the signed read of the score: 32768 never beats SHRT_MIN, so that member stays without a cluster and prints as the pair (0, 0)
    assert [0, 0] in clustgold.pairs('K_aln', 1, 'm0').tolist() and [0, 0] not in clustgold.pairs('K_aln', 2, 'm0').tolist()
    # the tie of equal set sizes went the other way in the copy with the tied pair in the other local order
    rep = {m: r for r, m in clustgold.pairs('K_aln', 2, 'm0').tolist()}
    b1, b2 = classes['tie_bc'], classes['tie_cb']
    assert (rep[b1] == b1) != (rep[b2] == b2)
    # the chain is cut by a depth cap of 1
    c0 = classes['chain']
    chain = [c0 + 3 * i for i in range(6)]
    rep_cap = {m: r for r, m in clustgold.pairs('K_aln', 2, 'm1c1').tolist()}
    rep_all = {m: r for r, m in clustgold.pairs('K_aln', 2, 'm1').tolist()}
    assert len({rep_all[c] for c in chain}) == 1 and len({rep_cap[c] for c in chain}) > 1


@pytest.mark.parametrize('run', sorted(clustgold.RUNS))
@pytest.mark.parametrize('t', [1, 2])
@pytest.mark.parametrize('name', clustgold.SETS)
def test_algorithms_reproduce_the_reference(name, t, run):
    mode, cap = clustgold.RUNS[run]
    keys, _ = clustgold.local(name)
    off, elem, score = clustgold.input_rows(name, t) if mode == 2 else clustgold.graph(name, t)
    assigned = api.clust_assign(mode, off, elem, score, max_iterations=cap)
    got_pairs, got_db = api.clust_format(keys, assigned)
    assert np.array_equal(got_pairs, clustgold.pairs(name, t, run))
    assert got_db == clustgold.cluster_db(name, t, run)


def test_greedy_mode_3_is_mode_2():
    off, elem, _ = clustgold.input_rows('R_aln', 2)
    assert np.array_equal(api.clust_assign(3, off, elem), api.clust_assign(2, off, elem))


def test_parser_refusals():
    keys = np.array([4, 9], np.uint32)
    with pytest.raises(api.SdError, match='Element 5 contained in some alignment list'):
        api.clust_parse(keys, [b'4\t10\t0.5\n5\t10\t0.5\n', b''], 5, 2)
    with pytest.raises(api.SdError):
        api.clust_parse(keys, [b'', b''], 0, 2)   # a sequence DB is no result DB
    off, elem, score = api.clust_parse(keys, [b'', b'9\t-7\t3\n4\t12\t0\n'], 7, 2)
    assert off.tolist() == [0, 1, 3] and elem.tolist() == [0, 1, 0] and score.tolist() == [65535, 7, 12]
    off, elem, score = api.clust_parse(keys, [b'4\n9\n', b'9\n'], 6, 2)
    assert elem.tolist() == [0, 1, 1] and score.tolist() == [65535] * 3


@pytest.mark.parametrize('mode', [2, 3])
@pytest.mark.parametrize('name', ['K_aln', 'R_pref', 'C1_aln'])
def test_module_greedy_modes_need_no_device(tmp_path, name, mode):
    seq, res = clustgold.write_inputs(tmp_path, name)
    out = str(tmp_path / 'clu')
    sdgpu('clust', seq, res, out, '--cluster-mode', mode, '--threads', '2', '-v', '0')
    assert read_db(out) == clustgold.cluster_db(name, 2, 'm2')
    assert open(out + '.dbtype', 'rb').read() == b'\x06\x00\x00\x00'


def test_module_is_registered_and_clusterdb_is_not():
    p = sdgpu('clust', check=False)
    assert p.returncode != 0 and 'usage: clust <sequenceDB> <resultDB> <clusterDB>' in p.stderr
    assert 'clust ' in sdgpu('--help').stdout
    p = sdgpu('clusterdb', check=False)
    assert p.returncode != 0 and 'unknown module' in p.stderr


@pytest.mark.parametrize('flags,words', [
    (['--set-mode', '1'], '--set-mode 1'),
    (['--weights', 'w.tsv'], '--weights'),
    (['--compressed', '1'], '--compressed 1'),
    (['--cluster-mode', '4'], 'Wrong clustering mode!'),
    (['--similarity-type', '3'], '--similarity-type'),
])
def test_module_refusals(tmp_path, flags, words):
    seq, res = clustgold.write_inputs(tmp_path, 'K1_aln')
    out = str(tmp_path / 'refused')
    p = sdgpu('clust', seq, res, out, '--cluster-mode', '2', *flags, check=False)
    assert p.returncode != 0 and words in p.stderr, p.stderr
    assert not (tmp_path / 'refused.index').exists() and not (tmp_path / 'refused').exists()


def test_module_refuses_what_the_reference_refuses(tmp_path):
    seq, res = clustgold.write_inputs(tmp_path, 'K1_aln')
    write_db(str(tmp_path / 'two'), [(5, b'AAA\n'), (6, b'AAAA\n')], 0)
    p = sdgpu('clust', tmp_path / 'two', res, tmp_path / 'o1', '--cluster-mode', '2', check=False)
    assert p.returncode != 0 and 'Sequence db size != result db size' in p.stderr
    write_db(str(tmp_path / 'lists7'), [(5, b'7\t10\t0.5\n')], 5)
    p = sdgpu('clust', seq, tmp_path / 'lists7', tmp_path / 'o2', '--cluster-mode', '2', check=False)
    assert p.returncode != 0 and 'Element 7 contained in some alignment list, but not contained in the sequence database!' in p.stderr
    write_db(str(tmp_path / 'generic'), [(5, b'5\n')], 12)
    p = sdgpu('clust', seq, tmp_path / 'generic', tmp_path / 'o3', '--cluster-mode', '2', check=False)
    assert p.returncode != 0 and 'Alignment format is not supported!' in p.stderr
    assert not any((tmp_path / o).exists() for o in ('o1', 'o2', 'o3'))


@pytest.mark.parametrize('mode', [0, 1])
def test_graph_modes_have_no_cpu_fallback(tmp_path, mode):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    seq, res = clustgold.write_inputs(tmp_path, 'K1_aln')
    p = sdgpu('clust', seq, res, tmp_path / 'clu', '--cluster-mode', mode, check=False)
    assert p.returncode != 0 and 'no usable HIP device' in p.stderr and not (tmp_path / 'clu').exists()


def test_header_declares_the_clust_calls():
    for name in ('sd_clust_symmetrize', 'sd_host_clust_order', 'sd_host_clust_parse', 'sd_host_clust_setcover', 'sd_host_clust_connected',
                 'sd_host_clust_greedy', 'sd_host_clust_format'):
        assert name in _lib.DECLARED_SYMBOLS and hasattr(_lib.load(), name)
