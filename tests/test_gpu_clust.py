"""GPU: sd_clust_symmetrize against the reference's own symmetric graphs (tests/golden/clust_vectors.npz) and against the restatement
tests/clust_ref.py on graphs made here, `sdgpu clust --cluster-mode 0 / 1` against the reference's cluster DBs, and the chain from a set DB
to a profile cluster search with `sdgpu` alone."""
import os
import sys

import numpy as np
import pytest

import clust_ref
import clustgold
from dbutil import ROOT, read_db, sdgpu
from spacedust_amd import _lib, api
from spacedust_amd._lib import ptr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('t', [1, 2])
@pytest.mark.parametrize('name', clustgold.SETS)
def test_symmetric_graph_equals_the_reference(gpu, name, t):
    off, elem, score = clustgold.input_rows(name, t)
    got_off, got_elem, got_score, stats = api.clust_symmetrize(gpu, off, elem, score)
    want = clustgold.graph(name, t)
    assert np.array_equal(got_off, want[0]) and np.array_equal(got_elem, want[1]) and np.array_equal(got_score, want[2])
    assert stats == dict(entries_in=len(elem), added=len(want[1]) - len(elem), largest_row=int(np.diff(want[0].astype(np.int64)).max()))


@pytest.mark.parametrize('n', [4095, 4096, 4097])
def test_symmetric_graph_equals_the_restatement(gpu, n):
    off, elem, score = clust_ref.random_graph(n, 20000, seed=n)
    want = clust_ref.symmetrize(off, elem, score)
    got = api.clust_symmetrize(gpu, off, elem, score, cap=len(want[1]) + 7)   # (a capacity larger than needed: one call)
    assert len(want[1]) > len(elem) and int(np.diff(off.astype(np.int64)).max()) > 256
    for g, w in zip(got[:3], want):
        assert np.array_equal(g, w)
    assert got[3]['added'] == len(want[1]) - len(elem)


def test_empty_graphs(gpu):
    off, elem, score, stats = api.clust_symmetrize(gpu, np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    assert off.tolist() == [0] and len(elem) == 0 and stats['added'] == 0
    off, elem, score, stats = api.clust_symmetrize(gpu, np.zeros(4, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    assert off.tolist() == [0, 0, 0, 0] and len(elem) == 0
    # rows without entries between rows with: 0 -> 2, 2 -> (nothing), 3 -> 0
    off, elem, score, stats = api.clust_symmetrize(gpu, [0, 1, 1, 1, 2], [2, 0], [11, 12])
    assert off.tolist() == [0, 2, 2, 3, 4] and elem.tolist() == [2, 3, 0, 0] and score.tolist() == [11, 12, 11, 12]


def test_refusals_leave_the_output_untouched(gpu):
    L = _lib.load()
    off, elem, score = clustgold.input_rows('R_aln', 2)
    want = clustgold.graph('R_aln', 2)
    total = len(want[1])
    out_off, out_elem, out_score = np.full(len(off), 77, np.uint64), np.full(total, 77, np.uint32), np.full(total, 77, np.uint16)
    stats = np.zeros(3, np.uint64)
    rc = L.sd_clust_symmetrize(gpu.h, len(off) - 1, ptr(off), ptr(elem), ptr(score), total - 1, ptr(out_off), ptr(out_elem), ptr(out_score), ptr(stats))
    assert rc == _lib.SD_ENOMEM and 'room for %d' % (total - 1) in L.sd_last_error(gpu.h).decode()
    assert stats.tolist()[:2] == [len(elem), total - len(elem)]
    assert (out_off == 77).all() and (out_elem == 77).all() and (out_score == 77).all()
    bad = elem.copy()
    bad[1234] = len(off) - 1
    rc = L.sd_clust_symmetrize(gpu.h, len(off) - 1, ptr(off), ptr(bad), ptr(score), total, ptr(out_off), ptr(out_elem), ptr(out_score), ptr(stats))
    assert rc == _lib.SD_EINVAL and 'entry 1234 names element 300 of 300' in L.sd_last_error(gpu.h).decode()
    assert (out_off == 77).all() and (out_elem == 77).all() and (out_score == 77).all()
    # more entries than the device sort counts: refused from the offsets alone, before an entry is read
    huge = np.array([0, 2 ** 32 - 4096], np.uint64)
    rc = L.sd_clust_symmetrize(gpu.h, 1, ptr(huge), ptr(elem), ptr(score), total, ptr(out_off), ptr(out_elem), ptr(out_score), ptr(stats))
    assert rc == _lib.SD_EUNSUPPORTED and '4294963200 entries in one call' in L.sd_last_error(gpu.h).decode()
    assert (out_off == 77).all() and (out_elem == 77).all() and (out_score == 77).all()
    rc = L.sd_clust_symmetrize(gpu.h, len(off) - 1, ptr(off), ptr(elem), ptr(score), total, ptr(out_off), ptr(out_elem), ptr(out_score), ptr(stats))
    assert rc == 0 and np.array_equal(out_elem, want[1]) and np.array_equal(out_off, want[0])


@pytest.mark.parametrize('run,t', [('m0', 2), ('m0', 1), ('m1', 2), ('m1c1', 2)])
@pytest.mark.parametrize('name', ['K_aln', 'R_pref', 'C1_aln'])
def test_module_equals_the_reference(tmp_path, name, run, t):
    mode, cap = clustgold.RUNS[run]
    seq, res = clustgold.write_inputs(tmp_path, name)
    out = str(tmp_path / 'clu')
    sdgpu('clust', seq, res, out, '--cluster-mode', mode, '--max-iterations', cap, '--similarity-type', t, '--threads', '4', '-v', '0')
    assert read_db(out) == clustgold.cluster_db(name, t, run)
    assert open(out + '.dbtype', 'rb').read() == b'\x06\x00\x00\x00'


def test_set_db_to_profile_cluster_search(tmp_path):
    """prefilter -> align -> clust -> align -a 1 -> result2profile -> clustersearch --profile-cluster-search 1, with sdgpu alone"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from iter3_scale import _write_fasta
    from spacedust_amd.synth import ALPHABET, make_proteomes
    from test_gpu_profile_cluster_search import SEARCH, _chain_by_hand
    tmp = tmp_path
    ps = make_proteomes(4, genes_per_proteome=55, n_families=70, seed=41)
    lut = np.frombuffer(ALPHABET.encode(), np.uint8)
    os.makedirs(tmp / 'fa')
    files = [_write_fasta(ps, s, str(tmp / 'fa'), lut) for s in range(4)]
    t = str(tmp / 't')
    common = ['--threads', '8', '-v', '0']
    sdgpu('createsetdb', *files, t, tmp / 'tmp', '-v', '0')
    sdgpu('prefilter', t, t, tmp / 'pref', '-s', '5.7', '-k', '6', '--max-seqs', '300', '-c', '0.8', '--cov-mode', '0', *common)
    sdgpu('align', t, t, tmp / 'pref', tmp / 'aln', '-e', '0.001', '-c', '0.8', '--cov-mode', '0', '--alignment-mode', '3', *common)
    sdgpu('clust', t, tmp / 'aln', tmp / 'clu', *common)
    clu = read_db(str(tmp / 'clu'))
    members = sorted(int(l) for text in clu.values() for l in text.splitlines())
    assert members == list(range(ps.n))                                   # a partition of the set
    assert all(int(text.split(b'\n')[0]) == rep for rep, text in clu.items())
    assert sum(text.count(b'\n') > 1 for text in clu.values()) >= 1       # at least one cluster of more than one member
    sdgpu('align', t, t, tmp / 'clu', t + '_clu_aln', '-a', '1', '-e', '0.001', '-v', '0')
    sdgpu('result2profile', t, t, t + '_clu_aln', t + '_clu_rep_profile', '-v', '0')
    sdgpu('clustersearch', t, t, tmp / 'wf.tsv', tmp / 'wf_tmp', '--profile-cluster-search', '1', '--exhaustive-search', '0', '-k', '6', *common)
    h = str(tmp / 'hand_tmp')
    os.makedirs(h)
    sdgpu('search', t, t + '_clu_rep_profile', h + '/result_clu', h + '/search', *SEARCH, *common)
    sdgpu('expandaln', t, t + '_clu_rep_profile', h + '/result_clu', t + '_clu_aln', h + '/result', *common)
    _chain_by_hand(t, h, str(tmp / 'hand.tsv'))
    tsv = open(tmp / 'wf.tsv').read()
    assert tsv == open(tmp / 'hand.tsv').read() and tsv.count('\n') > 0
