"""GPU: `clustersearch --profile-cluster-search 1 --exhaustive-search 0` (R/data/clustersearch.sh:69-80) -- the queries searched against
the profiles of the target's cluster representatives, the hits carried over to the cluster members by `expandaln`, the module chain on
the expanded alignment DB -- against the same modules run one by one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dbutil import GOLD, ROOT, SDGPU, read_db, sdgpu, write_db

pytestmark = pytest.mark.gpu

SEARCH = ['-e', '0.001', '--max-seqs', '100', '-a', '1', '-c', '0.8', '--cov-mode', '2', '--min-aln-len', '30', '-s', '5.7', '-k', '6',
          '--alignment-mode', '2']
CHAIN_DBS = ('result', 'result_prefixed', 'aggregate', 'aggregate_merged', 'matches', 'clusters')


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    """a target set DB of 4 proteomes x 55 proteins in families, with a clustering made by hand (every family is a cluster, its first
    protein the representative), <T>_clu_aln from `align -a 1` and <T>_clu_rep_profile from `result2profile`"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from iter3_scale import _write_fasta
    from spacedust_amd.synth import ALPHABET, make_proteomes
    tmp = tmp_path_factory.mktemp('pcs')
    ps = make_proteomes(4, genes_per_proteome=55, n_families=70, seed=41)
    lut = np.frombuffer(ALPHABET.encode(), np.uint8)
    os.makedirs(tmp / 'fa')
    files = [_write_fasta(ps, s, str(tmp / 'fa'), lut) for s in range(4)]
    t = str(tmp / 't')
    sdgpu('createsetdb', *files, t, tmp / 'tmp', '-v', '0')
    assert len(read_db(t)) == ps.n
    rep_of = {}
    clusters = {}
    for p in range(ps.n):
        f = int(ps.family[p])
        rep = rep_of.setdefault(f, p) if f >= 0 else p
        clusters.setdefault(rep, []).append(p)
    # neither `align` nor `result2profile` takes one-column cluster entries: the clustering as prefilter rows
    write_db(str(tmp / 'clu'), [(rep, b''.join(b'%d\t0\t0\n' % m for m in members)) for rep, members in sorted(clusters.items())], 7)
    sdgpu('align', t, t, tmp / 'clu', t + '_clu_aln', '-a', '1', '-e', '0.001', '-v', '0')
    sdgpu('result2profile', t, t, t + '_clu_aln', t + '_clu_rep_profile', '-v', '0')
    aln = read_db(t + '_clu_aln')
    members = {rep: [int(l.split(b'\t')[0]) for l in text.splitlines()] for rep, text in aln.items()}
    assert sum(len(m) > 1 for m in members.values()) > 20            # clusters with members besides their representative
    sdgpu('clustersearch', t, t, tmp / 'wf.tsv', tmp / 'wf_tmp', '--profile-cluster-search', '1', '--exhaustive-search', '0', '-k', '6', '--keep-tmp', '1',
          '--threads', '8', '-v', '0')
    return tmp, t, members


def _chain_by_hand(t, tmp, out):
    common = ['--threads', '8', '-v', '0']
    sdgpu('prefixid', tmp + '/result', tmp + '/result_prefixed', *common)
    sdgpu('besthitbyset', t, t, tmp + '/result_prefixed', tmp + '/aggregate', *common, '--simple-best-hit', '1', '--suboptimal-hits', '0')
    sdgpu('mergeresultsbyset', t + '_set_to_member', tmp + '/aggregate', tmp + '/aggregate_merged', *common)
    sdgpu('combinehits', t, t, tmp + '/aggregate_merged', tmp + '/matches', tmp, *common, '--alpha', '1', '--aggregation-mode', '0',
          '--filter-self-match', '0')
    sdgpu('clusterhits', t, t, tmp + '/matches', tmp + '/clusters', *common, '--multihit-pval', '0.01', '--cluster-pval', '0.01', '--max-gene-gap', '3',
          '--cluster-size', '2', '--db-output', '1', '--alpha', '1')
    sdgpu('summarizeresults', t, t, tmp + '/clusters', out, *common)


def test_workflow_equals_the_modules_run_by_hand(work):
    tmp, t, members = work
    w = str(tmp / 'wf_tmp')
    h = str(tmp / 'hand_tmp')
    os.makedirs(h)
    sdgpu('search', t, t + '_clu_rep_profile', h + '/result_clu', h + '/search', *SEARCH, '--threads', '8', '-v', '0')
    sdgpu('expandaln', t, t + '_clu_rep_profile', h + '/result_clu', t + '_clu_aln', h + '/result', '--threads', '8', '-v', '0')
    _chain_by_hand(t, h, str(tmp / 'hand.tsv'))
    tsv = open(tmp / 'wf.tsv').read()
    assert tsv == open(tmp / 'hand.tsv').read() and tsv.count('\n') > 50
    for db in ('result_clu',) + CHAIN_DBS:
        assert read_db(w + '/' + db) == read_db(h + '/' + db), db
    for db in ('pref', 'pref_swapped', 'aln_swapped'):           # --keep-tmp 1: the search step's DBs stay too
        assert os.path.exists(w + '/search/' + db + '.index'), db
    # the representatives' hits reached the other members of their clusters, and those hits reach the TSV
    reps = set(members)
    result = read_db(w + '/result')
    clu_hits = read_db(w + '/result_clu')
    assert all(int(l.split(b'\t')[0]) in reps for text in clu_hits.values() for l in text.splitlines())
    non_rep_hits = [(q, int(l.split(b'\t')[0])) for q, text in result.items() for l in text.splitlines() if int(l.split(b'\t')[0]) not in reps]
    assert len(non_rep_hits) > 20
    names = {int(l.split('\t')[0]): l.split('\t')[1] for l in open(t + '.lookup')}
    assert any(names[c] in tsv for _, c in non_rep_hits)
    assert open(w + '/result.dbtype', 'rb').read() == b'\x05\x00\x02\x00'


def test_intermediates_are_removed_without_keep_tmp(work):
    tmp, t, _ = work
    w = str(tmp / 'clean_tmp')
    sdgpu('clustersearch', t, t, tmp / 'clean.tsv', w, '--profile-cluster-search', '1', '--exhaustive-search', '0', '-k', '6', '--threads', '8', '-v', '0')
    assert open(tmp / 'clean.tsv').read() == open(tmp / 'wf.tsv').read()
    for name in ('result_clu', 'search/pref', 'search/pref_swapped', 'search/aln_swapped'):
        for suffix in ('', '.index', '.dbtype'):
            assert not os.path.exists(os.path.join(w, name + suffix)), name + suffix


@pytest.mark.parametrize('flags,env,target,words', [
    ([], {}, 't', '--exhaustive-search 1'),
    (['--exhaustive-search', '1'], {}, 't', 'searchslicedtargetprofile'),
    (['--exhaustive-search', '0'], {}, 'bare', '_clu_rep_profile'),
    (['--exhaustive-search', '0'], {'WORLD_SIZE': '2', 'RANK': '0'}, 't', 'one rank'),
    (['--exhaustive-search', '0', '--num-iterations', '2'], {}, 't', 'Profile-profile cluster searches are currently not supported'),
])
def test_what_the_workflow_refuses(work, flags, env, target, words):
    tmp, t, _ = work
    if target == 'bare' and not os.path.exists(str(tmp / 'bare.index')):    # the same set DB without the cluster DBs beside it
        for f in os.listdir(tmp):
            if f.startswith('t') and not f.startswith('t_clu') and os.path.isfile(tmp / f) and (f == 't' or f[1] in '._'):
                os.symlink(tmp / f, tmp / ('bare' + f[1:]))
    out = str(tmp / ('refused' + ''.join(flags).replace('-', '_') + '_'.join(sorted(env)) + target + '.tsv'))
    p = subprocess.run([SDGPU, 'clustersearch', str(tmp / target), str(tmp / target), out, str(tmp / 'refused_tmp'), '--profile-cluster-search', '1',
                        '-k', '6'] + flags, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode != 0 and words in p.stderr, p.stderr
    assert not os.path.exists(out) and not os.path.exists(str(tmp / 'refused_tmp' / 'result_clu.index'))


def test_plain_clustersearch_is_unchanged(work):
    """without the flag the workflow takes the path it took before: the bytes of tests/golden/pcs_plain_clustersearch.tsv, which the commit
    before this feature wrote on the same (seeded) input"""
    tmp, t, _ = work
    sdgpu('clustersearch', t, t, tmp / 'plain.tsv', tmp / 'plain_tmp', '--threads', '8', '-v', '0')
    plain = open(tmp / 'plain.tsv', 'rb').read()
    assert plain == open(os.path.join(GOLD, 'pcs_plain_clustersearch.tsv'), 'rb').read() and plain.count(b'\n') > 50
    assert plain != open(tmp / 'wf.tsv', 'rb').read()
