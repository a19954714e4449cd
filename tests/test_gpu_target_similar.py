"""GPU: `--target-search-mode 1` -- the similar-k-mer index of a sequence target DB (sd_target_build_similar) and the exact-k-mer query
mode of sd_prefilter_batch on it -- against the reference's own IndexTable::addSimilarSequence and QueryMatcher (takeOnlyBestKmer),
recorded by tools/make_golden_target_similar.py; through the C ABI, the Python binding, `sdgpu prefilter` and the two workflows."""
import glob
import gzip
import os

import numpy as np
import pytest

import tpref
import tsim
from dbutil import GOLD, read_db, sdgpu, write_db
from spacedust_amd import api

pytestmark = pytest.mark.gpu


def _build(gpu, host, name):
    g = tsim.golden()
    res, off = host.map_sequences(tsim.seqs_of(name))
    return api.Target.build_similar_on_device(gpu, host, res, off, k=6, kmer_thr=int(g[name + '_thr']) if name + '_thr' in g else 112), res


@pytest.fixture(scope='module')
def g_target(gpu, host):
    """set G, built once"""
    return _build(gpu, host, 'G')[0]


@pytest.fixture(scope='module')
def g_queries(host):
    seqs = tsim.seqs_of('Q')
    res, off = host.map_sequences(seqs)
    return seqs, res, off


@pytest.mark.parametrize('name', ['S', 'R'])
def test_full_index_equals_reference(gpu, host, name):
    """every (k-mer, target, position) triple in index order: R pins the record order -- a k-mer met at two positions of one target
    keeps the smaller one only if the records leave the generator in ascending (target, position) order"""
    g = tsim.golden()
    t, res = _build(gpu, host, name)
    d = t.download()
    exp = g[name + '_triples'].astype(np.int64)
    assert t.build_stats['entries'] == d['n_entries'] == len(exp)
    assert t.build_stats['records'] == int(g[name + '_records']) and t.build_stats['masked_residues'] == 0
    assert np.array_equal(tpref.triples_of_download(d), exp)
    assert int(d['starts'][-1]) == len(exp) and len(d['starts']) == 64000001
    assert np.array_equal(d['masked'], g[name + '_lookup']) and np.array_equal(d['masked'], res)
    if name == 'R':
        assert t.build_stats['records'] - t.build_stats['entries'] == int(g['R_removed'])


def test_b_digest(gpu, host):
    """set B: window lists beyond 65 536 k-mers (no partial list, so no scratch tier to outgrow)"""
    g = tsim.golden()
    t, _ = _build(gpu, host, 'B')
    assert t.build_stats['records'] == int(g['B_records']) == int(g['B_window_len'].sum())
    assert t.build_stats['entries'] == int(g['B_entries'])
    assert tpref.digest_of_download(t.download()) == str(g['B_digest'])


def test_g_index_counts_and_digest(g_target):
    g = tsim.golden()
    t = g_target
    assert t.build_stats['entries'] == int(g['G_entries']) and t.build_stats['records'] == int(g['G_records'])
    assert t.build_stats['passes'] == 1
    d = t.download()
    assert np.array_equal(np.bincount(d['entry_seq'], minlength=36), g['G_per_target'])
    assert int((np.diff(d['starts'].astype(np.int64)) > 0).sum()) == int(g['G_lists'])
    assert tpref.digest_of_download(d) == str(g['G_digest'])
    assert t.build_peak() > 0


@pytest.mark.parametrize('env', ['SD_INDEX_PASS', 'SD_INDEX_WIDE'])
def test_digests_in_many_passes_and_in_the_wide_form(gpu, host, monkeypatch, env):
    """SD_INDEX_PASS bounds the records of a pass (the generator recounts and rewrites per k-mer range); SD_INDEX_WIDE forces the form
    of an index of 2^32 entries and more"""
    g = tsim.golden()
    monkeypatch.setenv(env, '50000' if env == 'SD_INDEX_PASS' else '1')
    for name in ('B', 'G'):
        t, _ = _build(gpu, host, name)
        assert (t.build_stats['passes'] > 1) == (env == 'SD_INDEX_PASS')
        assert t.build_stats['entries'] == int(g[name + '_entries']) and t.build_stats['records'] == int(g[name + '_records'])
        assert tpref.digest_of_download(t.download()) == str(g[name + '_digest'])


def test_masking_plays_no_part(gpu, host):
    """set M: a low-complexity probe tantan would mask; the index and the lookup are those of the letters as they came"""
    g = tsim.golden()
    t, res = _build(gpu, host, 'M')
    d = t.download()
    assert t.build_stats['entries'] == int(g['M_entries']) and tpref.digest_of_download(d) == str(g['M_digest'])
    assert np.array_equal(d['masked'], res)


def _rows(gpu, host, target, g_queries, bias, kmer_thr):
    seqs, res, off = g_queries
    _, dg_b, km_b = host.comp_bias(res, off)
    if not bias:
        dg_b = np.zeros_like(dg_b)
    ident = np.full(len(seqs), 0xFFFFFFFF, np.uint32)
    par = api.prefilter_params(host, 36, kmer_thr=kmer_thr, max_hits=300, min_diag=15, cov_mode=0, cov_thr=0.0, k=6)
    hits, cnt, st = api.prefilter(gpu, target, par, res, off, km_b, dg_b, ident, want_stats=True)
    out = []
    for q in range(len(cnt)):
        for h in hits[q, :int(cnt[q])]:
            out.append((q, int(h['seqId']), int(h['score']), int(h['diagonal'])))
    return np.array(out, np.int64).reshape(-1, 4), st


@pytest.mark.parametrize('path', ['join', 'lookup'])
@pytest.mark.parametrize('bias', [1, 0])
def test_rows_equal_reference(gpu, host, g_target, g_queries, monkeypatch, bias, path):
    g = tsim.golden()
    if path == 'lookup':
        monkeypatch.setenv('SD_PF_JOIN', '0')
    else:
        monkeypatch.delenv('SD_PF_JOIN', raising=False)
    exp = g['rows_bias%d' % bias].astype(np.int64)
    exp[:, 3] &= 0xFFFF
    for kmer_thr in (0, 200):   # ignored: the mode belongs to the target
        got, st = _rows(gpu, host, g_target, g_queries, bias, kmer_thr)
        assert np.array_equal(st[:, 0].astype(np.int64), g['rows_bias%d_kmers' % bias])   # the reference's kmerListLen
        assert np.array_equal(got, exp), (bias, path, kmer_thr)
    assert len(exp) >= 36


def test_refusals(gpu, host, g_target):
    res, off = host.map_sequences(tsim.seqs_of('G'))
    data, poff = tpref.g_profiles()
    par = api.prefilter_params(host, 36, kmer_thr=112, max_hits=300, cov_thr=0.0, k=6)
    with pytest.raises(api.SdError) as e:
        api.prefilter_profile(gpu, g_target, par, host.map_profiles(data, poff))
    assert '(-5)' in str(e.value) and 'profile queries against a similar-k-mer sequence target' in str(e.value)
    with pytest.raises(api.SdError) as e:
        api.Target.build_similar_on_device(gpu, host, res, off, k=7, kmer_thr=112)
    assert '(-5)' in str(e.value) and 'k=7' in str(e.value) and 'k=6 only' in str(e.value)
    with pytest.raises(api.SdError) as e:   # 65 536 residues: as sd_target_build
        api.Target.build_similar_on_device(gpu, host, np.zeros(65536, np.uint8), np.array([0, 65536], np.uint64), k=6, kmer_thr=112)
    assert '(-3)' in str(e.value) and '65535' in str(e.value)


def test_sample_check_and_the_list_cap(gpu, host):
    """sd_target_sample_check reads this index as any other; a window whose list would reach 2^23 k-mers (where the reference's buffer
    cuts it) is refused by target and position before anything of it is counted"""
    import ctypes as C
    from spacedust_amd._lib import ptr
    g = tsim.golden()
    t, _ = _build(gpu, host, 'S')
    tr = g['S_triples'].astype(np.uint32)
    kmer, seq, pos = (np.ascontiguousarray(tr[:, i]) for i in range(3))
    sample = np.arange(4, dtype=np.uint32)
    missing, in_sample = C.c_uint64(), C.c_uint64()
    rc = gpu.L.sd_target_sample_check(gpu.h, t.h, ptr(kmer), ptr(seq), ptr(pos), len(tr), ptr(sample), 4, C.byref(missing), C.byref(in_sample), 0, 0, None)
    assert rc == 0 and missing.value == 0 and in_sample.value == len(tr)
    pos[0] += 1   # a triple that is no entry
    rc = gpu.L.sd_target_sample_check(gpu.h, t.h, ptr(kmer), ptr(seq), ptr(pos), len(tr), ptr(sample), 4, C.byref(missing), C.byref(in_sample), 0, 0, None)
    assert rc == 0 and missing.value == 1
    res, off = host.map_sequences(tsim.seqs_of('S'))
    with pytest.raises(api.SdError) as e:   # threshold -100: every parent and every child qualifies, 6.4 * 10^7 k-mers per window
        api.Target.build_similar_on_device(gpu, host, res, off, k=6, kmer_thr=-100)
    assert '(-5)' in str(e.value) and 'target 1, position 0' in str(e.value) and '8388608' in str(e.value)


def _pref_text(rows, q):
    return ''.join('%d\t%d\t%d\n' % (t, s, int(np.int16(np.uint16(d & 0xFFFF)))) for _, t, s, d in rows[rows[:, 0] == q])


COMMON = ['--k-score', 'seq:112,prof:2147483647', '--max-seqs', '300', '--min-ungapped-score', '15', '-c', '0', '--comp-bias-corr', '1']


@pytest.fixture(scope='module')
def g_dbs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('tsm_gpu')
    write_db(str(tmp / 'q'), [(i, s.encode() + b'\n') for i, s in enumerate(tsim.seqs_of('Q'))], 0)
    write_db(str(tmp / 't'), [(i, s.encode() + b'\n') for i, s in enumerate(tsim.seqs_of('G'))], 0)
    return tmp


def test_cli_prefilter_rows_and_messages(g_dbs):
    g = tsim.golden()
    q, t = g_dbs / 'q', g_dbs / 't'
    p = sdgpu('prefilter', q, t, g_dbs / 'out', '--target-search-mode', '1', *COMMON)
    assert 'Target search mode 1' in p.stdout and 'Index table k-mer threshold: 112 at k-mer size 6' in p.stdout
    assert ('Entries:          %d' % int(g['G_entries'])) in p.stdout
    db = read_db(str(g_dbs / 'out'))
    rows = g['rows_bias1'].astype(np.int64)
    assert sorted(db) == list(range(42))
    for i in range(42):
        assert db[i].decode() == _pref_text(rows, i), i
    # --mask and --mask-prob are ignored
    sdgpu('prefilter', q, t, g_dbs / 'out_m0', '--target-search-mode', '1', '--mask', '0', *COMMON, '-v', '0')
    sdgpu('prefilter', q, t, g_dbs / 'out_m1', '--target-search-mode', '1', '--mask', '1', '--mask-prob', '0.5', *COMMON, '-v', '0')
    assert read_db(str(g_dbs / 'out_m0')) == db == read_db(str(g_dbs / 'out_m1'))
    # a TARGET.idx beside the DB is neither looked for nor used
    sdgpu('createindex', t, g_dbs / 'ci_tmp', '--k-score', 'seq:112,prof:2147483647', '-k', '6', '-v', '0')
    p = sdgpu('prefilter', q, t, g_dbs / 'out_idx', '--target-search-mode', '1', *COMMON)
    assert 'Use index' not in p.stdout and 'Index file not used' not in p.stdout and read_db(str(g_dbs / 'out_idx')) == db
    for f in glob.glob(str(t) + '.idx*'):
        os.remove(f)
    p = sdgpu('prefilter', q, t, g_dbs / 'out_k7', '--target-search-mode', '1', '-k', '7', *COMMON, check=False)
    assert p.returncode != 0 and 'k=6 only' in p.stderr


def test_flag_is_moot_on_a_profile_target(g_dbs):
    """isProfile || targetSearchMode: a profile target DB is searched as without the flag"""
    data, poff = tpref.g_profiles()
    q, prof = g_dbs / 'q', g_dbs / 'prof'
    write_db(str(prof), [(i, data[int(poff[i]):int(poff[i + 1])]) for i in range(len(poff) - 1)], 2)
    common = ['--k-score', 'seq:2147483647,prof:110', '--max-seqs', '300', '-c', '0', '-v', '0']
    sdgpu('prefilter', q, prof, g_dbs / 'prof_plain', *common)
    sdgpu('prefilter', q, prof, g_dbs / 'prof_flag', '--target-search-mode', '1', *common)
    db = read_db(str(g_dbs / 'prof_plain'))
    assert read_db(str(g_dbs / 'prof_flag')) == db and sum(len(v) for v in db.values()) > 0


def test_plain_prefilter_is_the_mode_0_reference(g_dbs):
    """nothing else moved: without the flag, and with --target-search-mode 0, the module gives the reference's mode-0 rows"""
    g = tsim.golden()
    q, t = g_dbs / 'q', g_dbs / 't'
    rows = g['rows_mode0'].astype(np.int64)
    sdgpu('prefilter', q, t, g_dbs / 'plain', *COMMON, '-v', '0')
    db = read_db(str(g_dbs / 'plain'))
    for i in range(42):
        assert db[i].decode() == _pref_text(rows, i), i
    sdgpu('prefilter', q, t, g_dbs / 'plain0', '--target-search-mode', '0', *COMMON, '-v', '0')
    assert read_db(str(g_dbs / 'plain0')) == db


@pytest.fixture(scope='module')
def small_genomes(tmp_path_factory):
    """the first 250 proteins of the two example genomes as a set DB"""
    tmp = tmp_path_factory.mktemp('tsm_wf')
    fa = []
    for f in ('NC_000913.faa', 'NC_000915.faa'):
        text = gzip.open(os.path.join(GOLD, 'examples', f + '.gz'), 'rt').read()
        recs = text.split('\n>')
        dst = str(tmp / f)
        open(dst, 'w').write('\n>'.join(recs[:250]) + '\n')
        fa.append(dst)
    sdgpu('createsetdb', fa[0], fa[1], tmp / 'genome', tmp / 'tmp', '-v', '0')
    return tmp


ALIGN = ['-a', '1', '--alignment-mode', '2', '-e', '10', '--min-aln-len', '30', '-c', '0.8', '--cov-mode', '2', '--threads', '8', '-v', '3']
BANNER = 'Index table: k-mer size'        # what the streaming pipeline prints once its resident index stands


def test_search_workflow_runs_the_module_chain(small_genomes):
    work = small_genomes
    g = work / 'genome'
    flags = ['--target-search-mode', '1', '--max-seqs', '30', '-s', '5.7']
    p = sdgpu('search', g, g, work / 'wf_res', work / 'wf_tmp', *flags, *ALIGN)
    assert BANNER not in p.stdout and 'Target search mode 1' in p.stdout
    sdgpu('prefilter', g, g, work / 'wf_pref', *flags, '-c', '0.8', '--cov-mode', '2', '--threads', '8', '-v', '3')
    sdgpu('align', g, g, work / 'wf_pref', work / 'wf_aln', *ALIGN)
    want = read_db(str(work / 'wf_aln'))
    assert read_db(str(work / 'wf_res')) == want and sum(len(v) for v in want.values()) > 10000
    assert read_db(str(work / 'wf_tmp' / 'pref_0')) == read_db(str(work / 'wf_pref'))
    # and it is not the regular index's result
    sdgpu('prefilter', g, g, work / 'wf_pref0', '--max-seqs', '30', '-s', '5.7', '-c', '0.8', '--cov-mode', '2', '--threads', '8', '-v', '0')
    assert read_db(str(work / 'wf_pref0')) != read_db(str(work / 'wf_pref'))


def test_clustersearch_workflow_runs_the_module_chain(small_genomes):
    work = small_genomes
    g = work / 'genome'
    flags = ['--target-search-mode', '1', '--max-seqs', '30']
    p = sdgpu('clustersearch', g, g, work / 'cs.tsv', work / 'cs_tmp', *flags, '--threads', '8')
    assert BANNER not in p.stdout and 'Target search mode 1' in p.stdout
    # the module chain of clustersearch.sh by hand, with the workflow's defaults
    c = work / 'cs_chain'
    os.makedirs(c)
    common = ['--threads', '8', '-v', '3']
    sdgpu('prefilter', g, g, c / 'pref', *flags, '-s', '5.7', '-c', '0.8', '--cov-mode', '2', *common)
    sdgpu('align', g, g, c / 'pref', c / 'result', '-a', '1', '--alignment-mode', '2', '-e', '10', '--min-aln-len', '30', '-c', '0.8',
          '--cov-mode', '2', *common)
    sdgpu('prefixid', c / 'result', c / 'result_prefixed', *common)
    sdgpu('besthitbyset', g, g, c / 'result_prefixed', c / 'aggregate', '--simple-best-hit', '1', '--suboptimal-hits', '0', *common)
    sdgpu('mergeresultsbyset', str(g) + '_set_to_member', c / 'aggregate', c / 'aggregate_merged', *common)
    sdgpu('combinehits', g, g, c / 'aggregate_merged', c / 'matches', c, '--alpha', '1', '--aggregation-mode', '0', '--filter-self-match', '0', *common)
    sdgpu('clusterhits', g, g, c / 'matches', c / 'clusters', '--multihit-pval', '0.01', '--cluster-pval', '0.01', '--max-gene-gap', '3',
          '--cluster-size', '2', '--db-output', '1', '--alpha', '1', *common)
    sdgpu('summarizeresults', g, g, c / 'clusters', c / 'result.tsv', *common)
    tsv = open(work / 'cs.tsv').read()
    assert tsv == open(c / 'result.tsv').read() and tsv.count('\n#') + tsv.startswith('#') >= 1
