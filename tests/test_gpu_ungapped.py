"""The exhaustive ungapped prefilter on the GPU (sd_ungapped.hip, `sdgpu ungappedprefilter`, `--prefilter-mode 1`) against
tests/golden/ungapped_vectors.npz (written from the reference's SmithWaterman::ungapped_alignment) and the numpy
restatement of tests/ungapped_ref.py; where oracle/_ref/libsdref.so is present the live reference is asked as well."""
import os
import subprocess

import numpy as np
import pytest

import ungapped_ref as ur
from dbutil import sorted_md5, sdgpu, example_fasta, read_db, SDGPU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return np.load(ur.GOLDEN)


@pytest.fixture(scope='module')
def env():
    from spacedust_amd.api import Host, Context
    return Host(), Context(0)


def _seq(g, i):
    return g['res'][int(g['off'][i]):int(g['off'][i + 1])]


def test_kernel_scores_equal_every_golden_pair(gold, env):
    """bit for bit, with and without composition bias: lengths 1, 2, both sides of 64 / 128 / 256 / 512 / 1024, 65 535 on
    either side, pairs at the ceiling 255 - bias, low complexity, X"""
    from spacedust_amd import api
    g = gold
    host, gpu = env
    assert np.array_equal(host.matrix(0)[0].reshape(21, 21), g['M'])
    for use_cb in (1, 0):
        sel = g['comp'] == use_cb
        qs = sorted(set(g['pq'][sel].tolist()))
        ts = sorted(set(g['pt'][sel].tolist()))

        def pack(ids, bias):
            off = np.zeros(len(ids) + 1, np.uint64)
            np.cumsum([len(_seq(g, i)) for i in ids], out=off[1:])
            res = np.concatenate([_seq(g, i) for i in ids])
            cb = np.concatenate([g['cb'][int(g['off'][i]):int(g['off'][i + 1])] for i in ids]) if bias else None
            return gpu.seqset(res, off, cb)
        q_set, t_set = pack(qs, use_cb), pack(ts, False)
        got = api.ungapped_scores(gpu, g['M'].reshape(-1), q_set, t_set)
        assert api.ungapped_last_cells(gpu) == sum(len(_seq(g, i)) for i in qs) * sum(len(_seq(g, i)) for i in ts)
        qi = {q: x for x, q in enumerate(qs)}
        ti = {t: x for x, t in enumerate(ts)}
        bad = [(int(q), int(t), int(s), int(got[qi[q], ti[t]])) for q, t, s in zip(g['pq'][sel], g['pt'][sel], g['score'][sel])
               if int(got[qi[q], ti[t]]) != int(s)]
        print('comp bias %d: %d pairs, %d mismatches' % (use_cb, int(sel.sum()), len(bad)))
        assert not bad, bad[:10]
        if ur.have_ref():   # the live reference where it is present, in addition
            ref = ur.RefUngapped(bool(use_cb))
            for q in qs[:8]:
                ref.set_query(_seq(g, q))
                for t in ts[::7]:
                    assert ref.score(_seq(g, t)) == int(got[qi[q], ti[t]]), (q, t)


@pytest.fixture(scope='module')
def synth(env):
    from spacedust_amd.synth import make_proteomes
    host, gpu = env
    ps = make_proteomes(2, genes_per_proteome=110, n_families=150, mean_len=150, seed=11)
    cb = host.comp_bias(ps.residues, ps.offsets)[0]
    M = host.matrix(0)[0]
    full = ur.restate_matrix(M, ps.residues, ps.offsets, cb, ps.residues, ps.offsets)
    return ps, cb, M, full


def test_full_score_matrix_of_a_synthetic_set(env, synth):
    """every pair of a few hundred synthetic proteins against the numpy restatement: none sampled"""
    from spacedust_amd import api
    host, gpu = env
    ps, cb, M, full = synth
    q_set, t_set = gpu.seqset(ps.residues, ps.offsets, cb), gpu.seqset(ps.residues, ps.offsets, None)
    got = api.ungapped_scores(gpu, M, q_set, t_set)
    assert got.shape == full.shape == (ps.n, ps.n) and ps.n >= 200
    diff = np.argwhere(got.astype(np.int32) != full)
    print('%d x %d pairs, %d mismatches, %d at 200 and above' % (ps.n, ps.n, len(diff), int((full >= 200).sum())))
    assert len(diff) == 0, [(int(a), int(b), int(got[a, b]), int(full[a, b])) for a, b in diff[:10]]


def _expected_lists(ps, full, keys, **kw):
    lens = ps.lengths()
    ident = kw.pop('ident', None)
    out = []
    for q in range(ps.n):
        out.append(ur.list_rule(full[q], keys, lens[q], lens, identity_key=None if ident is None or ident[q] == 0xFFFFFFFF else keys[ident[q]], **kw))
    return out


def _check_lists(hits, counts, keys, expected):
    for q, exp in enumerate(expected):
        got = [(int(keys[h['seqId']]), int(h['score'])) for h in hits[q, :counts[q]]]
        assert got == exp, (q, got[:5], exp[:5])
        assert all(int(h['diagonal']) == 0 for h in hits[q, :counts[q]])


def test_capi_lists_follow_the_list_rule(env, synth):
    from spacedust_amd import api
    host, gpu = env
    ps, cb, M, full = synth
    q_set, t_set = gpu.seqset(ps.residues, ps.offsets, cb), gpu.seqset(ps.residues, ps.offsets, None)
    # DB keys that do not follow the index order: the order and the cut use the key
    keys = np.random.default_rng(5).permutation(ps.n).astype(np.uint32) + 1000
    ident = np.arange(ps.n, dtype=np.uint32)
    none = np.full(ps.n, 0xFFFFFFFF, np.uint32)
    lens = ps.lengths()
    short = int(np.argmin(lens))
    cases = []
    for min_score in (0, 15, 254):
        for idn in (ident, none, None):
            cases.append(dict(min_score=min_score, max_seqs=ps.n, cov_mode=0, cov_thr=0.0, ident=idn))
    for cov_mode in (0, 1, 2, 3, 4, 5):
        cases.append(dict(min_score=15, max_seqs=ps.n, cov_mode=cov_mode, cov_thr=0.8, ident=ident))
        # the mode both keeps and drops pairs that score above the threshold
        kept = np.array([ur.covered_mask(0.8, cov_mode, lens[q], lens) for q in range(ps.n)])
        assert (kept & (full > 15)).sum() > ps.n and (~kept & (full > 15)).sum() > ps.n, cov_mode
    for max_seqs in (1, 7, 40):
        cases.append(dict(min_score=15, max_seqs=max_seqs, cov_mode=0, cov_thr=0.0, ident=ident))
    ties_at_cut = 0
    for c in cases:
        par = api.ungapped_params(host, max_hits=c['max_seqs'], min_score=c['min_score'], cov_mode=c['cov_mode'], cov_thr=c['cov_thr'])
        hits, counts = api.ungapped_prefilter(gpu, par, q_set, t_set, target_keys=keys, identity_id=c['ident'])
        exp = _expected_lists(ps, full, keys, min_score=c['min_score'], max_seqs=c['max_seqs'], cov_mode=c['cov_mode'], cov_thr=c['cov_thr'],
                              ident=c['ident'])
        _check_lists(hits, counts, keys, exp)
        if c['max_seqs'] < ps.n:
            whole = _expected_lists(ps, full, keys, min_score=c['min_score'], max_seqs=ps.n, cov_mode=0, cov_thr=0.0, ident=c['ident'])
            ties_at_cut += sum(1 for w in whole if len(w) > c['max_seqs'] and w[c['max_seqs'] - 1][1] == w[c['max_seqs']][1])
    assert ties_at_cut > 0   # a score tie at the cut was among the cases
    # the identity rule where the identity pair scores below the threshold (min 254: every self pair below the ceiling ...)
    par = api.ungapped_params(host, max_hits=ps.n, min_score=254)
    hits, counts = api.ungapped_prefilter(gpu, par, q_set, t_set, target_keys=keys, identity_id=ident)
    assert counts[short] == 1 and int(hits[short, 0]['seqId']) == short and int(hits[short, 0]['score']) == int(full[short, short]) < 254
    hits, counts = api.ungapped_prefilter(gpu, par, q_set, t_set, target_keys=keys, identity_id=none)
    assert counts[short] == 0
    # ... and where it scores above (min 15)
    par = api.ungapped_params(host, max_hits=ps.n, min_score=15)
    for idn in (ident, none):
        hits, counts = api.ungapped_prefilter(gpu, par, q_set, t_set, target_keys=keys, identity_id=idn)
        assert full[short, short] > 15 and short in hits[short, :counts[short]]['seqId']


UNGAPPED_PAR = ('--sub-mat aa:blosum62.out,nucl:nucleotide.out -c 0.8 -e 0.001 --cov-mode 2 --comp-bias-corr 1 --comp-bias-corr-scale 1 '
                '--min-ungapped-score 15 --max-seqs 300 --prefilter-mode 1 --db-load-mode 0 --threads 8 -v 3').split()
ALIGN_PAR = ('-a 1 --alignment-mode 2 -e 10 --min-aln-len 30 -c 0.8 --cov-mode 2 --comp-bias-corr 1 --threads 8').split()


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ungapped')
    fa = example_fasta(tmp)
    sdgpu('createsetdb', fa[0], fa[1], tmp / 'genome', tmp / 'tmp', '-v', '0')
    g = tmp / 'genome'
    sdgpu('ungappedprefilter', g, g, tmp / 'upref', *UNGAPPED_PAR)
    return tmp


def flat(work, db):
    sdgpu('prefixid', work / db, work / (os.path.basename(str(db)) + '.flat'), '--tsv', '--threads', '1')
    return open(work / (os.path.basename(str(db)) + '.flat')).readlines()


def test_module_on_the_example_genomes(gold, work):
    g = gold
    db = read_db(str(work / 'upref'))
    assert len(db) == int(g['ex_n'])
    assert open(str(work / 'upref') + '.dbtype', 'rb').read()[:1] == b'\x07'   # prefilter result type
    for x, q in enumerate(g['ex_query']):
        a, b = int(g['ex_off'][x]), int(g['ex_off'][x + 1])
        assert db[int(q)].decode() == ur.list_text(zip(g['ex_key'][a:b].tolist(), g['ex_score'][a:b].tolist())), int(q)
    for key, payload in db.items():
        lines = payload.decode().splitlines()
        assert len(lines) <= 300
        prev = None
        for l in lines:
            k, s, d = l.split('\t')
            assert 0 <= int(k) < len(db) and d == '0' and (int(s) > 15 or int(k) == key)
            assert prev is None or prev <= (-int(s), int(k))
            prev = (-int(s), int(k))
    # --gpu 1 runs the same path
    sdgpu('ungappedprefilter', work / 'genome', work / 'genome', work / 'upref_gpu1', *UNGAPPED_PAR, '--gpu', '1')
    assert read_db(str(work / 'upref_gpu1')) == db


def test_search_mode_1_equals_module_chain(work):
    g = work / 'genome'
    sdgpu('align', g, g, work / 'upref', work / 'ualn', *ALIGN_PAR)
    chain = flat(work, 'ualn')
    sdgpu('search', g, g, work / 'usearch', work / 'tmpus', '--prefilter-mode', '1', '--max-seqs', '300', '--min-ungapped-score', '15',
          *ALIGN_PAR)
    fused = flat(work, 'usearch')
    assert len(chain) > 1000 and (len(fused), sorted_md5(fused)) == (len(chain), sorted_md5(chain))
    assert sorted_md5(flat(work, 'tmpus/pref_0')) == sorted_md5(flat(work, 'upref'))
    # not the k-mer prefilter's result
    assert sorted_md5(flat(work, 'upref')) != '8109a70bdea70ee10e0dbd27ba6b7e37'


def test_clustersearch_mode_1_equals_module_chain(work):
    g = work / 'genome'
    sdgpu('clustersearch', g, g, work / 'ufused.tsv', work / 'tmpuf', '--prefilter-mode', '1', '--filter-self-match', '--keep-dbs', '1',
          '--threads', '8')
    assert sorted_md5(flat(work, 'tmpuf/pref_0')) == sorted_md5(flat(work, 'upref'))
    if not os.path.exists(work / 'ualn.index'):
        sdgpu('align', g, g, work / 'upref', work / 'ualn', *ALIGN_PAR)
    common = ['--threads', '8', '-v', '3']
    sdgpu('prefixid', work / 'ualn', work / 'u_prefixed', *common)
    sdgpu('besthitbyset', g, g, work / 'u_prefixed', work / 'u_aggregate', '--simple-best-hit', '1', '--suboptimal-hits', '0', *common)
    sdgpu('mergeresultsbyset', str(g) + '_set_to_member', work / 'u_aggregate', work / 'u_merged', *common)
    sdgpu('combinehits', g, g, work / 'u_merged', work / 'u_matches', work / 'tmp', '--alpha', '1', '--aggregation-mode', '0',
          '--filter-self-match', '1', *common)
    sdgpu('clusterhits', g, g, work / 'u_matches', work / 'u_clusters', '--multihit-pval', '0.01', '--cluster-pval', '0.01', '--max-gene-gap', '3',
          '--cluster-size', '2', '--db-output', '1', '--alpha', '1', *common)
    sdgpu('summarizeresults', g, g, work / 'u_clusters', work / 'uchain.tsv', *common)
    fused, chain = open(work / 'ufused.tsv').readlines(), open(work / 'uchain.tsv').readlines()
    assert sum(1 for l in chain if l.startswith('#')) > 50
    assert sorted_md5(fused, drop_first_column=True) == sorted_md5(chain, drop_first_column=True)


def test_refusals_and_mode_0(work):
    g = work / 'genome'

    def refused(*args):
        p = subprocess.run([SDGPU] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode != 0, args
        return p.stderr
    assert '--prefilter-mode 2' in refused('search', g, g, work / 'r1', work / 'tmpr', '--prefilter-mode', '2')
    assert '--prefilter-mode 3' in refused('search', g, g, work / 'r1', work / 'tmpr', '--prefilter-mode', '3')
    assert '--prefilter-mode 2' in refused('clustersearch', g, g, work / 'r1.tsv', work / 'tmpr', '--prefilter-mode', '2')
    assert '--num-iterations' in refused('search', g, g, work / 'r1', work / 'tmpr', '--prefilter-mode', '1', '--num-iterations', '2')
    assert '--num-iterations' in refused('clustersearch', g, g, work / 'r1.tsv', work / 'tmpr', '--prefilter-mode', '1', '--num-iterations', '3')
    assert '--compressed' in refused('ungappedprefilter', g, g, work / 'r2', '--compressed', '1')
    assert '--taxon-list' in refused('ungappedprefilter', g, g, work / 'r2', '--taxon-list', '562')
    assert '--gpu-server' in refused('ungappedprefilter', g, g, work / 'r2', '--gpu-server', '1')
    assert '--prefilter-mode 2' in refused('ungappedprefilter', g, g, work / 'r2', '--prefilter-mode', '2')
    # nucleotide and index (createindex) DBs: by their type
    import shutil
    import struct
    for name, dbtype in (('nucl', 1), ('idx', 9)):
        for ext in ('', '.index'):
            shutil.copy(str(g) + ext, str(work / name) + ext)
        open(str(work / name) + '.dbtype', 'wb').write(struct.pack('<i', dbtype))
    assert 'dbtype' in refused('ungappedprefilter', work / 'nucl', g, work / 'r3')
    assert 'dbtype' in refused('ungappedprefilter', g, work / 'nucl', work / 'r3')
    assert 'dbtype' in refused('ungappedprefilter', g, work / 'idx', work / 'r3')
    # --prefilter-mode 0 is the k-mer prefilter, as before (the checksum tests/test_gpu_cli.py pins)
    sdgpu('search', g, g, work / 'res0', work / 'tmp0', '--prefilter-mode', '0', '-a', '1', '--alignment-mode', '2', '-e', '10', '--min-aln-len', '30',
          '-c', '0.8', '--cov-mode', '2', '-s', '5.7', '--max-seqs', '300', '--threads', '8')
    lines = flat(work, 'res0')
    assert (len(lines), sorted_md5(lines)) == (15065, '2e917f0e9782e8a7412c7360aa7bf1b4')
    lines = flat(work, 'tmp0/pref_0')
    assert (len(lines), sorted_md5(lines)) == (98957, '8109a70bdea70ee10e0dbd27ba6b7e37')


def test_profile_dbs_are_refused(work):
    """profile DBs on either side: refused by value with a message, in the module and in the workflow (a real profile DB, made by
    result2profile from the alignments of the module chain)"""
    g = work / 'genome'
    if not os.path.exists(work / 'ualn.index'):
        sdgpu('align', g, g, work / 'upref', work / 'ualn', *ALIGN_PAR)
    sdgpu('result2profile', g, g, work / 'ualn', work / 'uprofile', '--threads', '8', '-v', '0', '-e', '0.001', '--e-profile', '0.001',
          '--mask-profile', '1', '--comp-bias-corr', '1', '--filter-msa', '1', '--filter-min-enable', '0', '--max-seq-id', '0.9', '--qid', '0.0',
          '--qsc', '-20', '--cov', '0', '--diff', '1000', '--pca', 'substitution:1.100,context:1.400', '--pcb', 'substitution:4.100,context:5.800')
    prof = work / 'uprofile'
    assert open(str(prof) + '.dbtype', 'rb').read()[:1] == b'\x02'

    def refused(*args):
        p = subprocess.run([SDGPU] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode != 0, args
        return p.stderr
    assert 'profile query databases are not implemented' in refused('ungappedprefilter', prof, g, work / 'rp1')
    assert 'profile target databases are not supported' in refused('ungappedprefilter', g, prof, work / 'rp2')
    assert 'profile query databases are not implemented' in refused('search', prof, g, work / 'rp3', work / 'tmprp', '--prefilter-mode', '1')
    assert 'profile target databases are not supported' in refused('search', g, prof, work / 'rp4', work / 'tmprp', '--prefilter-mode', '1')
    for name in ('rp1', 'rp2', 'rp3', 'rp4'):
        assert not os.path.exists(str(work / name) + '.index'), name
    # the C ABI: the pipeline constructor of this mode does not take profile queries
    import ctypes as C
    from spacedust_amd import _lib
    L = _lib.load()
    p = _lib.SearchParams()
    L.sd_search_default_params(C.byref(p))
    p.profileQueries = 1
    h = C.c_void_p()
    assert L.sd_search_create_ungapped(0, C.byref(p), None, C.byref(h)) == -5 and not h.value   # SD_EUNSUPPORTED


def test_python_pipeline_in_mode_1(env, synth):
    """pipeline.ClusterSearch(prefilter_mode=1): the scan is the prefilter stage, no index is held, and the prefilter rows the
    pipeline hands to the alignments are the lists of the C-ABI call"""
    from spacedust_amd import api
    from spacedust_amd.pipeline import SetDB, ClusterSearch
    host, gpu = env
    ps, cb, M, full = synth
    db = SetDB.from_proteomes(ps)
    cs = ClusterSearch(gpu, host, db, max_seqs=60, filter_self_match=True, prefilter_mode=1)
    assert cs.k == 0 and cs.index_entries == 0 and not cs.L.sd_search_target(cs.h)
    out = cs.search(db, same_db=True)
    par = api.ungapped_params(host, max_hits=60, min_score=15, cov_mode=2, cov_thr=0.8)
    q_set, t_set = gpu.seqset(ps.residues, ps.offsets, cb), gpu.seqset(ps.residues, ps.offsets, None)
    hits, counts = api.ungapped_prefilter(gpu, par, q_set, t_set, identity_id=np.arange(ps.n, dtype=np.uint32))
    st, _ = cs._raw_stats()
    assert int(st[4]) == int(counts.sum()) == int(st[5]) > 0   # prefilter hits = pairs aligned = the C-ABI lists
    assert out['entries'] > 0
    with pytest.raises(Exception):
        ClusterSearch(gpu, host, db, prefilter_mode=2)
