"""GPU: `sdgpu align -a` on a cluster DB against the reference's rows, and `sdgpu makeclusterdb --single-step-clustering 1` against its five
steps run one after another with the parameter strings of tests/clusterdb_ref.py; the DBs it leaves serve
`clustersearch --profile-cluster-search 1`."""
import os
import sys

import numpy as np
import pytest

import cdbgold
import clusterdb_ref as ref
from dbutil import ROOT, read_db, sdgpu

pytestmark = pytest.mark.gpu

OUTPUTS = ('_clu_rep_profile', '_clu', '_clu_aln')
ANCILLARY = ('_h', '_h.index', '_h.dbtype', '.lookup', '.source')


def test_align_on_a_cluster_db(tmp_path):
    """one-column rows: no diagonal is read, the row of the entry's own key is an identity pair (both DBs are one path)"""
    t, _, r = cdbgold.write_inputs(tmp_path)
    out = str(tmp_path / 'aln')
    sdgpu('align', t, t, r, out, '-a', '--threads', 4, '-v', 0)
    assert cdbgold.read_files(out) == cdbgold.db_files(cdbgold.aln_db(), 5)
    aln = dict(cdbgold.aln_db())
    assert all(aln[k].split(b'\t')[0] == b'%d' % k and aln[k].count(b'\t') >= 10 for k in aln)   # the self row first, with a backtrace


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    """a set DB of 3 proteomes x 50 proteins in close families; `clusterdb` on it, and its five steps by hand on the same DB under another name"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from iter3_scale import _write_fasta
    from spacedust_amd.synth import ALPHABET, make_proteomes
    tmp = tmp_path_factory.mktemp('cdb')
    # (families within 2 .. 12 % of their ancestor: most pairs of members lie above the workflow's --min-seq-id 0.7)
    ps = make_proteomes(3, genes_per_proteome=50, n_families=60, seed=43, div_range=(0.02, 0.12), indel_rate=0.004)
    lut = np.frombuffer(ALPHABET.encode(), np.uint8)
    os.makedirs(tmp / 'fa')
    files = [_write_fasta(ps, s, str(tmp / 'fa'), lut) for s in range(3)]
    t = str(tmp / 't')
    sdgpu('createsetdb', *files, t, tmp / 'tmp', '-v', '0')
    assert len(read_db(t)) == ps.n == 150
    h = str(tmp / 'h')   # the same set DB under another name: the hand-made chain writes h_clu* beside it
    for f in os.listdir(tmp):
        if os.path.isfile(tmp / f) and (f == 't' or f[:2] in ('t.', 't_')):
            os.symlink(tmp / f, tmp / ('h' + f[1:]))
    wf_tmp, h_tmp = str(tmp / 'wf_tmp'), str(tmp / 'h_tmp')
    said = sdgpu('makeclusterdb', t, wf_tmp, '--single-step-clustering', 1, '--threads', 4).stdout
    os.makedirs(h_tmp)
    steps = ref.step_args(h, h_tmp, 4, user={'--single-step-clustering': '1'})
    for module, pos, flags in steps:
        sdgpu(module, *pos, *flags)
    return tmp, t, h, wf_tmp, h_tmp, said, steps


def test_workflow_equals_its_five_steps(work):
    tmp, t, h, wf_tmp, h_tmp, said, steps = work
    for suffix in OUTPUTS:
        assert cdbgold.read_files(t + suffix) == cdbgold.read_files(h + suffix), suffix
    for db in ('cluster_mmseqs', 'db_clu'):
        assert cdbgold.read_files(wf_tmp + '/' + db) == cdbgold.read_files(h_tmp + '/' + db), db
    assert [l for l in said.splitlines() if l.startswith('makeclusterdb runs: ')] == \
        [l.replace(h_tmp, wf_tmp).replace(h + ' ', t + ' ').replace(h + '_', t + '_') for l in ref.plan_lines(steps)]
    assert 'pairs realigned' in said
    # one resident scope over the five steps, the cluster workflow's own included: the set of <T> that result2profile uploads for its
    # realignment is the one `align -a` finds on the device
    sets = [l.split('sequence set ')[1] for l in said.splitlines() if l.startswith('makeclusterdb: sequence set ')]
    assert [l for l in sets if l.endswith(' ' + t)] == ['uploaded ' + t, 'reused ' + t]
    assert sum(l.startswith('uploaded ') for l in sets) == 2   # (the other: the redundancy-filtered sub DB inside `cluster`)
    # what the three DBs are: a profile and a consensus per cluster, the members' alignments with backtraces
    clu = {rep: [int(x) for x in text.split()] for rep, text in read_db(wf_tmp + '/cluster_mmseqs').items()}
    assert 20 < len(clu) < 150 and sum(len(m) > 1 for m in clu.values()) > 10
    assert open(t + '_clu_rep_profile.dbtype', 'rb').read() == b'\x02\x00\x00\x00' and open(t + '_clu.dbtype', 'rb').read() == b'\x00\x00\x00\x00'
    assert open(t + '_clu_aln.dbtype', 'rb').read() == b'\x05\x00\x00\x00'
    seqs, prof, cons, aln = read_db(t), read_db(t + '_clu_rep_profile'), read_db(t + '_clu'), read_db(t + '_clu_aln')
    assert sorted(prof) == sorted(cons) == sorted(aln) == sorted(clu)
    assert all(len(prof[k]) == 25 * (len(seqs[k]) - 1) and len(cons[k]) == len(seqs[k]) for k in clu)
    assert all(sorted(int(l.split(b'\t')[0]) for l in aln[k].splitlines()) == sorted(clu[k]) and aln[k].count(b'\t') == 10 * len(clu[k]) for k in clu)
    for suffix in ANCILLARY:   # the profile DB shares db_clu's ancillary files, the consensus DB the profile DB's
        for db in ('_clu_rep_profile', '_clu'):
            assert os.path.lexists(t + db + suffix) == os.path.lexists(wf_tmp + '/db_clu' + suffix), db + suffix


def test_a_second_run_skips_what_is_there(work):
    tmp, t, h, wf_tmp, h_tmp, said, steps = work
    watched = [t + s for s in OUTPUTS] + [wf_tmp + '/cluster_mmseqs', wf_tmp + '/db_clu']
    before = [os.stat(p).st_mtime_ns for p in watched]
    os.remove(t + '_clu.dbtype')   # one step's output missing: that step alone runs again
    again = sdgpu('makeclusterdb', t, wf_tmp, '--single-step-clustering', 1, '--threads', 4).stdout
    plan = [l.split(':')[0] for l in again.splitlines() if l.startswith('makeclusterdb skips: ') or l.startswith('makeclusterdb runs: ')]
    assert plan == ['makeclusterdb skips'] * 3 + ['makeclusterdb runs'] + ['makeclusterdb skips']
    after = [os.stat(p).st_mtime_ns for p in watched]
    assert [a == b for a, b in zip(after, before)] == [True, False, True, True, True]
    assert cdbgold.read_files(t + '_clu') == cdbgold.read_files(h + '_clu')


def test_remove_tmp_files(work):
    tmp, t, h, wf_tmp, h_tmp, said, steps = work
    r = str(tmp / 'r')
    for f in os.listdir(tmp):
        if os.path.isfile(tmp / f) and (f == 't' or f[:2] in ('t.', 't_')) and not f.startswith('t_clu'):
            os.symlink(tmp / f, tmp / ('r' + f[1:]))
    r_tmp = str(tmp / 'r_tmp')
    sdgpu('makeclusterdb', r, r_tmp, '--single-step-clustering', 1, '--remove-tmp-files', 1, '--threads', 4, '-v', 0)
    for suffix in OUTPUTS:
        assert cdbgold.read_files(r + suffix) == cdbgold.read_files(t + suffix), suffix
    left = sorted(os.listdir(r_tmp))   # the script removes the cluster DB and the cluster workflow's directory; db_clu stays
    assert left and all(f == 'db_clu' or f.startswith('db_clu.') or f.startswith('db_clu_') for f in left), left


def test_profile_cluster_search_reads_what_clusterdb_wrote(work):
    tmp, t, h, wf_tmp, h_tmp, said, steps = work
    flags = ['--profile-cluster-search', '1', '--exhaustive-search', '0', '-k', '6', '--threads', '4', '-v', '0']
    sdgpu('clustersearch', t, t, tmp / 'wf.tsv', tmp / 'cs_wf', *flags)
    sdgpu('clustersearch', h, h, tmp / 'h.tsv', tmp / 'cs_h', *flags)
    tsv = open(tmp / 'wf.tsv').read()
    assert tsv == open(tmp / 'h.tsv').read() and tsv.count('\n') > 20
