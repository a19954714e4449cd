"""GPU: k = 5 in the k-mer prefilter -- the device index builders, the 2 + 3 similar-k-mer enumerator, the exact lookup against a
profile target, profile queries with five steps -- against rows of the real reference (tests/golden/k5_vectors.npz,
tools/make_golden_k5.py), through the C ABI, the Python binding and the sdgpu modules and workflows."""
import os
import sys

import numpy as np
import pytest

import k5gold
import tpref
from dbutil import ROOT, read_db, sdgpu, write_db
from spacedust_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def db(host):
    seqs, n_small = k5gold.sequences()
    res, off = host.map_sequences(seqs)
    _, dg_b, km_b = host.comp_bias(res, off, 5)
    return dict(seqs=seqs, n_small=n_small, res=res, off=off, dg=dg_b, km=km_b)


@pytest.fixture(scope='module')
def host_index(host, db):
    return {thr: host.build_index(db['res'], db['off'], k=5, kmer_thr=thr) for thr in (88, 75)}


@pytest.fixture(scope='module')
def prof_dbs(tmp_path_factory):
    """the 144 sequences and the 18 profiles of profile_vectors.npz as DBs"""
    tmp = tmp_path_factory.mktemp('k5')
    profiles, pseqs = k5gold.profile_inputs()
    seq_db, prof_db = str(tmp / 'seq'), str(tmp / 'prof')
    write_db(seq_db, [(i, s.encode() + b'\n') for i, s in enumerate(pseqs)], 0)
    write_db(prof_db, [(i, p) for i, p in enumerate(profiles)], 2)
    return tmp, seq_db, prof_db


def _subset(db, queries):
    off, res = db['off'], db['res']
    qoff = k5gold.offsets_of([db['seqs'][q] for q in queries])
    cat = lambda a: np.concatenate([a[int(off[q]):int(off[q + 1])] for q in queries])
    return cat(res), qoff, cat(db['km']), cat(db['dg'])


def test_device_index_equals_host_index(gpu, host, db, host_index):
    """sd_target_build at k = 5 (ib_records_kernel<5>, 20^5 list starts): tantan-masked residues, X windows, the per-sequence dedupe of
    the 7 600 near-copies -- entry for entry what sd_host_index_build gives, which tests/test_k5_host.py holds against the reference"""
    h = host_index[88]
    t = api.Target.build_on_device(gpu, host, db['res'], db['off'], k=5, kmer_thr=88)
    d = t.download()
    assert t.build_stats['entries'] == d['n_entries'] == h.n_entries and t.build_stats['masked_residues'] == h.masked_residues > 0
    assert len(d['starts']) == k5gold.TABLE + 1 and np.array_equal(d['starts'], h.kmer_offsets.astype(np.uint64))
    assert np.array_equal(d['entry_seq'], h.entry_seq) and np.array_equal(d['entry_pos'], h.entry_pos)
    assert np.array_equal(d['masked'], h.masked)


def test_similar_kmer_lists_equal_reference_as_sets(gpu, host):
    """The enumerator's list of a window against the reference's list L: the target DB holds one 12-residue sequence per k-mer of L (the
    k-mer at the seed positions, indexed at threshold 0, unmasked), the query is the window with no composition bias.  The statistics
    then give |E| similar k-mers and |E n L| index hits for the emitted set E; both equal |L|, and the k-mers of a list are distinct,
    so E = L."""
    g = k5gold.golden()
    lo = g['list_off'].astype(np.int64)
    for i, (w, thr) in enumerate(zip(g['windows'], g['window_thr'])):
        L = g['lists'][lo[i]:lo[i + 1]].astype(np.int64)
        assert len(set(L.tolist())) == len(L)
        tres = np.zeros((len(L), k5gold.SPAN), np.uint8)
        for x, p in enumerate(k5gold.SEED):
            tres[:, p] = (L // 20 ** x) % 20
        toff = np.arange(len(L) + 1, dtype=np.uint64) * k5gold.SPAN
        idx = host.build_index(tres.reshape(-1), toff, k=5, kmer_thr=0, mask=False)
        assert idx.n_entries == len(L)
        tgt = api.Target(gpu, host, idx)
        q = np.zeros(k5gold.SPAN, np.uint8)
        q[list(k5gold.SEED)] = w
        par = api.prefilter_params(host, idx.n, kmer_thr=int(thr), max_hits=300, cov_thr=0.0, bin_size=2, k=5)
        _, _, st = api.prefilter(gpu, tgt, par, q, np.array([0, k5gold.SPAN], np.uint64), np.zeros(k5gold.SPAN, np.int16),
                                 np.zeros(k5gold.SPAN, np.int8), np.array([0xFFFFFFFF], np.uint32), want_stats=True)
        assert (int(st[0, 0]), int(st[0, 1])) == (len(L), len(L)), (i, st[0], len(L))


def test_prefilter_matches_restatement(gpu, host, oracle, small_proteomes):
    """the route of test_prefilter_k7_matches_oracle: rows and statistics of every query against oracle/sd_oracle.cpp at k = 5"""
    ps = small_proteomes
    ident = np.arange(ps.n, dtype=np.uint32)
    _, dg_b, km_b = host.comp_bias(ps.residues, ps.offsets, 5)
    idx = host.build_index(ps.residues, ps.offsets, 5, 88)
    tgt = api.Target(gpu, host, idx)
    par = api.prefilter_params(host, idx.n, kmer_thr=88, max_hits=50, cov_thr=0.0, bin_size=2, k=5)
    hits, cnt, st = api.prefilter(gpu, tgt, par, ps.residues, ps.offsets, km_b, dg_b, ident, want_stats=True)
    ot = oracle.target(ps.residues, ps.offsets, k=5, kmer_thr=88)
    assert ot.n_entries == idx.n_entries
    total = 0
    for q in range(0, ps.n, 2):
        seq = ps.residues[int(ps.offsets[q]):int(ps.offsets[q + 1])]
        ids, sc, dg, ost = ot.prefilter(seq, identity_id=q, kmer_thr=88, max_hits=50, bin_size=2)
        n = int(cnt[q])
        total += n
        assert n == len(ids), (q, n, len(ids))
        assert (hits[q, :n]['seqId'] == ids).all() and (hits[q, :n]['score'] == sc).all() and (hits[q, :n]['diagonal'] == dg).all(), q
        assert tuple(int(x) for x in st[q]) == tuple(int(x) for x in ost), (q, st[q], ost)
    assert total > ps.n // 2


@pytest.mark.parametrize('kmer_thr', [88, 75])
def test_prefilter_rows_equal_reference(gpu, host, db, host_index, kmer_thr):
    """sd_prefilter_batch at 88 = kmerThreshold(5.7, 5) and at a permissive 75: short sequences, X windows, the masked stretch, and the
    family base, whose index hits overflow the first hit buffer (the query_splits path) -- the statistics say so"""
    g = k5gold.golden()
    queries = [int(q) for q in g['queries']]
    tgt = api.Target(gpu, host, host_index[kmer_thr])
    par = api.prefilter_params(host, tgt.n, kmer_thr=kmer_thr, max_hits=300, cov_thr=0.0, bin_size=2, k=5)
    qres, qoff, qkm, qdg = _subset(db, queries)
    hits, cnt, st = api.prefilter(gpu, tgt, par, qres, qoff, qkm, qdg, g['query_identity'].astype(np.uint32), want_stats=True)
    assert (cnt != 0xFFFFFFFF).all()
    assert np.array_equal(st[:, 1].astype(np.int64), g['index_hits_%d' % kmer_thr])
    assert int(st[queries.index(db['n_small']), 1]) > k5gold.HIT_BUFFER
    assert np.array_equal(k5gold.rows_of(hits, cnt, queries), k5gold.expected_rows(g['pf_rows_%d' % kmer_thr]))


def test_profile_query_rows_equal_reference(gpu, host):
    """sd_prefilter_profile_batch with five one-residue steps (82 = the profile threshold at -s 5.7, and 70)"""
    g = k5gold.golden()
    profiles, pseqs = k5gold.profile_inputs()
    res, off = host.map_sequences(pseqs)
    prof = host.map_profiles(b''.join(profiles[:8]), k5gold.offsets_of(profiles[:8]))
    tgt = api.Target(gpu, host, host.build_index(res, off, 5, 0))
    ident = np.array([4 * q if q % 2 == 0 else 0xFFFFFFFF for q in range(8)], np.uint32)
    for thr in (82, 70):
        par = api.prefilter_params(host, tgt.n, kmer_thr=thr, max_hits=300, cov_thr=0.0, bin_size=2, k=5)
        hits, cnt, _ = api.prefilter_profile(gpu, tgt, par, prof, identity_id=ident)
        assert np.array_equal(k5gold.rows_of(hits, cnt, range(8)), k5gold.expected_rows(g['prof_rows_%d' % thr])), thr


@pytest.mark.parametrize('thr', [82, 75])
def test_profile_target_equals_reference(gpu, host, thr):
    """sd_target_build_profile(k = 5): counts and digest of the index, and the rows of sequence queries (exact lookup) against it"""
    g = k5gold.golden()
    profiles, pseqs = k5gold.profile_inputs()
    prof = host.map_profiles(b''.join(profiles), k5gold.offsets_of(profiles))
    t = api.Target.build_profile_on_device(gpu, host, prof, k=5, kmer_thr=thr)
    tag = 'PT%d' % thr
    assert t.build_stats['entries'] == int(g[tag + '_entries']) and t.build_stats['records'] == int(g[tag + '_records'])
    d = t.download()
    assert len(d['starts']) == k5gold.TABLE + 1
    assert np.array_equal(np.bincount(d['entry_seq'], minlength=len(profiles)), g[tag + '_per_target'])
    assert tpref.digest_of_download(d) == str(g[tag + '_digest'])
    res, off = host.map_sequences(pseqs)
    _, dg_b, km_b = host.comp_bias(res, off, 5)
    par = api.prefilter_params(host, len(profiles), kmer_thr=0, max_hits=300, min_diag=15, cov_mode=0, cov_thr=0.0, k=5)
    hits, cnt, st = api.prefilter(gpu, t, par, res, off, km_b, dg_b, np.full(len(pseqs), 0xFFFFFFFF, np.uint32), want_stats=True)
    assert np.array_equal(st[:, 0].astype(np.int64), g[tag + '_kmers'].astype(np.int64))   # the windows without X
    assert np.array_equal(k5gold.rows_of(hits, cnt, range(len(pseqs))), k5gold.expected_rows(g[tag + '_rows']))


def _text(rows, q):
    return ''.join('%d\t%d\t%d\n' % (t, s, int(np.int16(np.uint16(d & 0xFFFF)))) for _, t, s, d in rows[rows[:, 0] == q])


def test_cli_prefilter_prints_the_golden_rows(prof_dbs):
    g = k5gold.golden()
    tmp, seq_db, prof_db = prof_dbs
    sdgpu('prefilter', seq_db, prof_db, tmp / 'pt82', '-k', '5', '--k-score', 'seq:2147483647,prof:82', '--max-seqs', '300', '--min-ungapped-score',
          '15', '-c', '0', '--comp-bias-corr', '1', '-v', '0')
    out = read_db(str(tmp / 'pt82'))
    rows = g['PT82_rows'].astype(np.int64)
    assert sorted(out) == list(range(144))
    for q in range(144):
        assert out[q].decode() == _text(rows, q), q
    # -s 5.7 resolves to the same threshold, 82, through sd_host_profile_kmer_threshold(5.7, 5)
    sdgpu('prefilter', seq_db, prof_db, tmp / 'pt_s', '-k', '5', '-s', '5.7', '--max-seqs', '300', '-c', '0', '-v', '0')
    assert read_db(str(tmp / 'pt_s')) == out
    # profile queries against a sequence target at k = 5
    sdgpu('prefilter', prof_db, seq_db, tmp / 'pq82', '-k', '5', '--k-score', 'seq:2147483647,prof:82', '--max-seqs', '300', '-c', '0', '-v', '0')
    pq = read_db(str(tmp / 'pq82'))
    assert sorted(pq) == list(range(18)) and sum(len(v) > 0 for v in pq.values()) > 8


def test_cli_createindex_k5_is_read_back(tmp_path, db):
    """`createindex -k 5` and `prefilter -k 5` reading that file: the rows of the run that builds the index on the device"""
    t = str(tmp_path / 'small')
    write_db(t, [(i, s.encode() + b'\n') for i, s in enumerate(db['seqs'][:db['n_small']])], 0)
    par = ['-k', '5', '-s', '5.7', '--max-seqs', '300', '-c', '0', '--threads', '8']
    built = sdgpu('prefilter', t, t, tmp_path / 'built', *par, '-v', '3')
    assert 'k-mer size 5' in built.stdout and 'Use index' not in built.stdout
    sdgpu('createindex', t, tmp_path / 'tmp', '-k', '5', '-s', '5.7', '-v', '0')
    read = sdgpu('prefilter', t, t, tmp_path / 'read', *par, '-v', '3')
    assert 'Use index' in read.stdout
    a, b = read_db(str(tmp_path / 'built')), read_db(str(tmp_path / 'read'))
    assert a == b and sum(v.count(b'\n') for v in a.values()) > db['n_small']
    p = sdgpu('prefilter', t, t, tmp_path / 'split', *par, '--split', '2', check=False)
    assert p.returncode != 0 and 'a k=5 target index is searched unsplit' in p.stderr


def test_search_against_profile_db_equals_the_four_modules(prof_dbs):
    """`search <sequenceDB> <profileDB> -k 5 --keep-tmp 1` (searchtargetprofile.sh) against prefilter, swapresults, align, swapresults
    run one by one with -k 5; its prefilter rows are not the -k 6 run's, so a fall-back to 6 would show"""
    tmp, seq_db, prof_db = prof_dbs
    res, work = str(tmp / 'search5'), str(tmp / 'search5_tmp')
    sdgpu('search', seq_db, prof_db, res, work, '-k', '5', '-s', '5.7', '-e', '0.001', '--keep-tmp', '1', '--threads', '8', '-v', '0')
    w = str(tmp / 'mod_')
    sdgpu('prefilter', seq_db, prof_db, w + 'pref', '-k', '5', '-s', '5.7', '--max-seqs', '300', '-c', '0', '--cov-mode', '0', '--threads', '8', '-v', '0')
    sdgpu('swapresults', seq_db, prof_db, w + 'pref', w + 'pref_swapped', '-e', '0.001', '--threads', '8', '-v', '0')
    sdgpu('align', prof_db, seq_db, w + 'pref_swapped', w + 'aln_swapped', '-a', '1', '--alignment-mode', '2', '-e', '0.001', '-c', '0', '--cov-mode', '0',
          '--max-seqs', '2147483647', '--threads', '8', '-v', '0')
    sdgpu('swapresults', prof_db, seq_db, w + 'aln_swapped', w + 'final', '-e', '0.001', '--threads', '8', '-v', '0')
    for name in ('pref', 'pref_swapped', 'aln_swapped'):
        assert read_db(work + '/' + name) == read_db(w + name), name
    final = read_db(res)
    assert final == read_db(w + 'final') and sum(v.count(b'\n') for v in final.values()) > 50
    sdgpu('search', seq_db, prof_db, tmp / 'search6', tmp / 'search6_tmp', '-k', '6', '-s', '5.7', '-e', '0.001', '--keep-tmp', '1', '--threads', '8',
          '-v', '0')
    assert read_db(str(tmp / 'search6_tmp') + '/pref') != read_db(work + '/pref')


CHAIN = ('result', 'result_prefixed', 'aggregate', 'aggregate_merged', 'matches', 'clusters')


def test_profile_cluster_search_k5_equals_its_module_chain(tmp_path):
    """`clustersearch --profile-cluster-search 1 --exhaustive-search 0 -k 5`: the reference's k for that search (Search.cpp:251-257).
    A target set DB of 4 proteomes x 55 proteins in families with a clustering made by hand, as tests/test_gpu_profile_cluster_search.py
    makes it; the workflow's TSV and DBs against search -k 5, expandaln and the chain run one by one."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from iter3_scale import _write_fasta
    from spacedust_amd.synth import ALPHABET, make_proteomes
    tmp = tmp_path
    ps = make_proteomes(4, genes_per_proteome=55, n_families=70, seed=41)
    lut = np.frombuffer(ALPHABET.encode(), np.uint8)
    os.makedirs(tmp / 'fa')
    files = [_write_fasta(ps, s, str(tmp / 'fa'), lut) for s in range(4)]
    t = str(tmp / 't')
    sdgpu('createsetdb', *files, t, tmp / 'tmp', '-v', '0')
    rep_of, clusters = {}, {}
    for p in range(ps.n):
        f = int(ps.family[p])
        rep = rep_of.setdefault(f, p) if f >= 0 else p
        clusters.setdefault(rep, []).append(p)
    write_db(str(tmp / 'clu'), [(rep, b''.join(b'%d\t0\t0\n' % m for m in members)) for rep, members in sorted(clusters.items())], 7)
    sdgpu('align', t, t, tmp / 'clu', t + '_clu_aln', '-a', '1', '-e', '0.001', '-v', '0')
    sdgpu('result2profile', t, t, t + '_clu_aln', t + '_clu_rep_profile', '-v', '0')
    common = ['--threads', '8', '-v', '0']
    w, h = str(tmp / 'wf_tmp'), str(tmp / 'hand_tmp')
    sdgpu('clustersearch', t, t, tmp / 'wf.tsv', w, '--profile-cluster-search', '1', '--exhaustive-search', '0', '-k', '5', '--keep-tmp', '1', *common)
    os.makedirs(h)
    sdgpu('search', t, t + '_clu_rep_profile', h + '/result_clu', h + '/search', '-e', '0.001', '--max-seqs', '100', '-a', '1', '-c', '0.8', '--cov-mode', '2',
          '--min-aln-len', '30', '-s', '5.7', '-k', '5', '--alignment-mode', '2', '--keep-tmp', '1', *common)
    sdgpu('expandaln', t, t + '_clu_rep_profile', h + '/result_clu', t + '_clu_aln', h + '/result', *common)
    sdgpu('prefixid', h + '/result', h + '/result_prefixed', *common)
    sdgpu('besthitbyset', t, t, h + '/result_prefixed', h + '/aggregate', *common, '--simple-best-hit', '1', '--suboptimal-hits', '0')
    sdgpu('mergeresultsbyset', t + '_set_to_member', h + '/aggregate', h + '/aggregate_merged', *common)
    sdgpu('combinehits', t, t, h + '/aggregate_merged', h + '/matches', h, *common, '--alpha', '1', '--aggregation-mode', '0', '--filter-self-match', '0')
    sdgpu('clusterhits', t, t, h + '/matches', h + '/clusters', *common, '--multihit-pval', '0.01', '--cluster-pval', '0.01', '--max-gene-gap', '3',
          '--cluster-size', '2', '--db-output', '1', '--alpha', '1')
    sdgpu('summarizeresults', t, t, h + '/clusters', tmp / 'hand.tsv', *common)
    tsv = open(tmp / 'wf.tsv').read()
    assert tsv == open(tmp / 'hand.tsv').read() and tsv.count('\n') > 50
    for name in ('result_clu',) + CHAIN:
        assert read_db(w + '/' + name) == read_db(h + '/' + name), name
    assert read_db(w + '/search/pref') == read_db(h + '/search/pref')
    # k = 5 was searched: the prefilter rows of the same workflow at -k 6 differ
    sdgpu('clustersearch', t, t, tmp / 'wf6.tsv', tmp / 'wf6_tmp', '--profile-cluster-search', '1', '--exhaustive-search', '0', '-k', '6', '--keep-tmp', '1',
          *common)
    assert read_db(str(tmp / 'wf6_tmp') + '/search/pref') != read_db(w + '/search/pref')
