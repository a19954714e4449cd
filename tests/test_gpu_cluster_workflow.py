"""GPU: `sdgpu cluster --single-step-clustering 1` against its seven modules run one after another with the parameter strings the
workflow derives (tests/cluglue_ref.py), on 300 sequences: 60 families of the example proteins, each a root, an exact copy, a near copy
(1 .. 3 % of the letters substituted) and two diverged copies (20 .. 40 %).  The chain reads a soft-linked DB in prefilter, align /
rescorediagonal and clust."""
import functools
import os

import numpy as np
import pytest

import chgold
import cluglue_ref as ref
from dbutil import read_db, sdgpu, write_db

pytestmark = pytest.mark.gpu

AA = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', np.uint8)
CASES = {'cov0': dict(cov_mode=0), 'cov1': dict(cov_mode=1), 'ungapped': dict(alignment_mode=4, min_seq_id=0.9)}


@functools.lru_cache(None)
def families():
    """-> (entries [(key, letters + newline)], family of key, kind of key); keys ascend in shuffled sequence order"""
    let, off = chgold.sequences('C1')
    off = off.astype(np.int64)
    rng = np.random.default_rng(61)
    # roots that are unrelated to each other by the CPU oracle's Smith-Waterman (E > 1 against the 300 sequences' residues; the workflow
    # keeps hits up to 0.001): the example proteomes hold paralogues, which cluster together rightly
    from oracle.pyoracle import Oracle
    from spacedust_amd.api import Host
    aa2num, orc = np.asarray(Host().matrix(0)[2], np.uint8), Oracle(4)
    roots = []
    for i in range(0, len(off) - 1, 17):
        if len(roots) < 60 and 120 <= off[i + 1] - off[i] - 1 <= 350:
            cand = aa2num[let[off[i]:off[i + 1] - 1]]
            if all(orc.sw_align(cand, aa2num[let[off[j]:off[j + 1] - 1]], 75000, identity=False)['evalue'] > 1.0 for j in roots):
                roots.append(i)
    assert len(roots) == 60
    seqs = []
    for f, i in enumerate(roots):
        root = let[off[i]:off[i + 1] - 1].copy()   # (without the stop letter)
        seqs.append((f, 'root', root))
        seqs.append((f, 'exact', root.copy()))
        for kind, lo, hi in (('near', 0.01, 0.03), ('far', 0.2, 0.4), ('far', 0.2, 0.4)):
            s = root.copy()
            pos = rng.permutation(len(s))[:max(1, int(len(s) * rng.uniform(lo, hi)))]
            s[pos] = AA[rng.integers(0, 20, len(pos))]
            seqs.append((f, kind, s))
    order = rng.permutation(len(seqs))
    entries, family, kind = [], {}, {}
    for n, x in enumerate(order):
        key = 7 + 2 * n
        entries.append((key, seqs[x][2].tobytes() + b'\n'))
        family[key], kind[key] = seqs[x][0], seqs[x][1]
    return entries, family, kind


def both(tmp, case):
    """runs the workflow and the seven modules -> (workflow's cluster DB path, chain's cluster DB path, the chain's tmp dir)"""
    entries, _, _ = families()
    seq = os.path.join(str(tmp), 'seq')
    write_db(seq, entries, 0)
    par = CASES[case]
    wf = os.path.join(str(tmp), 'wf_clu')
    flags = ['--single-step-clustering', 1, '--threads', 4, '-v', 0]
    for k, f in (('cov_mode', '--cov-mode'), ('alignment_mode', '--alignment-mode'), ('min_seq_id', '--min-seq-id')):
        if k in par:
            flags += [f, par[k]]
    sdgpu('cluster', seq, wf, os.path.join(str(tmp), 'wf_tmp'), *flags)
    t = os.path.join(str(tmp), 'chain_tmp')
    os.mkdir(t)
    p = ref.step_flags(4, **par)
    sdgpu('clusthash', seq, t + '/aln_redundancy', *p['clusthash'])
    sdgpu('clust', seq, t + '/aln_redundancy', t + '/clu_redundancy', *p['clust'])
    sdgpu('createsubdb', t + '/clu_redundancy', seq, t + '/input_step_redundancy', *p['createsubdb'])
    sub = t + '/input_step_redundancy'
    sdgpu('prefilter', sub, sub, t + '/pref', *p['prefilter'])
    sdgpu(p['align'][0], sub, sub, t + '/pref', t + '/aln', *p['align'][1])
    sdgpu('clust', sub, t + '/aln', t + '/clu_step0', *p['clust'])
    chain = os.path.join(str(tmp), 'chain_clu')
    sdgpu('mergeclusters', seq, chain, t + '/clu_redundancy', t + '/clu_step0', *p['mergeclusters'])
    return wf, chain, t


@pytest.mark.parametrize('case', sorted(CASES))
def test_workflow_equals_its_modules(tmp_path, case):
    wf, chain, t = both(tmp_path, case)
    for suffix in ('', '.index', '.dbtype'):
        assert open(wf + suffix, 'rb').read() == open(chain + suffix, 'rb').read(), suffix
    assert open(wf + '.dbtype', 'rb').read() == b'\x06\x00\x00\x00'
    entries, family, kind = families()
    clu = {rep: [int(x) for x in text.split()] for rep, text in read_db(wf).items()}
    members = sorted(m for v in clu.values() for m in v)
    assert members == sorted(k for k, _ in entries)                       # every sequence in exactly one cluster
    assert all(v[0] == rep for rep, v in clu.items())                      # the representative is the first member
    cluster_of = {m: rep for rep, v in clu.items() for m in v}
    for f in range(60):
        same = [k for k in family if family[k] == f and kind[k] in ('root', 'exact')]
        assert len(same) == 2 and cluster_of[same[0]] == cluster_of[same[1]]   # exact copies share a cluster
    assert all(len({family[m] for m in v}) == 1 for v in clu.values())     # unrelated families do not
    assert len(clu) < len(entries) - 60
    # the chain ran on a soft-linked DB: fewer entries than the input, the input's offsets, the input's data file
    sub = t + '/input_step_redundancy'
    sub_index = ref.read_index(sub)
    assert os.path.islink(sub) and os.path.realpath(sub) == os.path.realpath(os.path.join(str(tmp_path), 'seq'))
    assert 0 < len(sub_index) <= len(entries) - 60 and set(sub_index) <= set(ref.read_index(os.path.join(str(tmp_path), 'seq')))
    assert len(read_db(t + '/pref')) == len(sub_index) == len(read_db(t + '/aln'))
    expected = {'cov0': b'0', 'cov1': b'2', 'ungapped': b'0'}   # --cluster-mode: set cover, or greedy under --cov-mode 1
    assert ref.step_flags(4, **CASES[case])['clust'][-1].encode() == expected[case]


def test_remove_tmp_files(tmp_path):
    entries, _, _ = families()
    seq = str(tmp_path / 'seq')
    write_db(seq, entries[:40], 0)
    tmp = str(tmp_path / 'tmp')
    sdgpu('cluster', seq, tmp_path / 'clu', tmp, '--single-step-clustering', 1, '--remove-tmp-files', 1, '--threads', 4, '-v', 0)
    assert sorted(os.listdir(tmp)) == [] and len(read_db(str(tmp_path / 'clu'))) > 0 and read_db(seq) == dict(entries[:40])


def test_refusals(tmp_path):
    seq = str(tmp_path / 'seq')
    write_db(seq, [(0, b'MKVLAAGIVGLLLAQ\n')], 0)
    p = sdgpu('cluster', seq, tmp_path / 'clu', tmp_path / 'tmp', check=False)
    assert p.returncode != 0 and '--filter-hits' in p.stderr + p.stdout and 'linclust' in p.stderr + p.stdout
    for dbtype, named in ((1, 'nucleotide'), (2, 'profile')):
        other = str(tmp_path / ('db%d' % dbtype))
        write_db(other, [(0, b'ACGTACGTACGT\n')], dbtype)
        p = sdgpu('cluster', other, tmp_path / 'clu', tmp_path / 'tmp', '--single-step-clustering', 1, check=False)
        assert p.returncode != 0 and named in p.stderr + p.stdout
    p = sdgpu('cluster', seq, tmp_path / 'clu', tmp_path / 'tmp', '--single-step-clustering', 1, '--cluster-reassign', 1, check=False)
    assert p.returncode != 0 and '--cluster-reassign' in p.stderr + p.stdout
