"""The target split (`sdgpu prefilter --split N --split-mode 0`, Prefiltering::setupSplit / runSplit / mergeTargetSplits) on the
GPU: one index per split, built, searched and destroyed in turn, a query's entry the sorted concatenation of its per-split lists.
A split run has its own expected output (shorter per-split lists, nothing cut after the merge), so it is checked against
  * golden rows of the reference's classes (tools/make_golden_split.py), and the live reference where oracle/_ref was built,
  * the unsplit module -- pinned to the reference binary's checksum elsewhere -- run on physically split target DBs,
and the automatic mode (--split 0, --split-memory-limit, sd_target_footprint) and the workflows on top of it."""
import os
import re

import numpy as np
import pytest

from dbutil import GOLD, write_db, read_db, sorted_md5, sdgpu, example_fasta

pytestmark = pytest.mark.gpu

# the regression command line's prefilter parameters (-k 0 is k = 6 at this size; the runs on physically split DBs pass -k 6)
PREF = ['-s', '5.7', '-c', '0.8', '--cov-mode', '2', '--threads', '8', '-v', '3']
ALIGN = ['-a', '1', '--alignment-mode', '2', '-e', '10', '--min-aln-len', '30', '-c', '0.8', '--cov-mode', '2', '--threads', '8', '-v', '3']
BANNER = 'Index table: k-mer size'        # what the streaming pipeline prints once its resident index stands


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('split')
    fa = example_fasta(tmp)
    sdgpu('createsetdb', fa[0], fa[1], tmp / 'genome', tmp / 'tmp', '-v', '0')
    return tmp


@pytest.fixture(scope='module')
def genome(work):
    """key -> sequence entry (b'...\\n'), and the index's length column in key order"""
    db = read_db(str(work / 'genome'))
    keys = sorted(db)
    assert keys == list(range(5898))
    return db, [len(db[k]) + 1 for k in keys]


def rows_of(payload):
    return [tuple(int(x) for x in l.split('\t')) for l in payload.decode().split('\n') if l]


def merge(lists):
    """mergeTargetSplits: the per-split lists one after the other, sorted by hit_t::compareHitsByScoreAndId"""
    return sorted((r for l in lists for r in l), key=lambda r: (-abs(r[1]), r[0]))


def plan_of(lengths, n, max_seqs):
    from spacedust_amd.api import Host
    p = Host(1).split_plan(lengths, n, max_seqs=max_seqs)
    return [(int(f), int(s)) for f, s in zip(p['db_from'], p['db_size'])], p['list_len']


def sub_dbs(work, genome, n, max_seqs, tag=''):
    """every split's sequences as a target DB of its own, keys preserved"""
    db, lengths = genome
    ranges, list_len = plan_of(lengths, n, max_seqs)
    paths = []
    for s, (f, size) in enumerate(ranges):
        path = str(work / ('sub%s_%d_%d' % (tag, n, s)))
        if size and not os.path.exists(path + '.index'):
            write_db(path, [(k, db[k]) for k in range(f, f + size)], 0)
        paths.append(path if size else None)
    return paths, list_len


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(GOLD, 'split_vectors.npz'))
    return {k: z[k] for k in z.files}


def test_golden_file_holds_its_three_conditions(gold):
    """what the generator asserted before writing, on the loaded file"""
    list_len, max_seqs = int(gold['list_len']), int(gold['max_seqs'])
    assert (gold['split_raw_count'] >= list_len).any()                       # a (query, split) list cut at the per-split length
    merged_len = np.diff(gold['merged_off'].astype(np.int64))
    assert (merged_len > max_seqs).any()                                     # a merged list longer than --max-seqs
    differs = 0
    for i in range(len(gold['queries'])):
        a, b = int(gold['merged_off'][i]), int(gold['merged_off'][i + 1])
        c, d = int(gold['unsplit_off'][i]), int(gold['unsplit_off'][i + 1])
        differs += not (np.array_equal(gold['merged_key'][a:b], gold['unsplit_key'][c:d]) and
                        np.array_equal(gold['merged_score'][a:b], gold['unsplit_score'][c:d]) and
                        np.array_equal(gold['merged_diag'][a:b], gold['unsplit_diag'][c:d]))
    assert differs > 0                                                       # a merged list that is not the unsplit list
    assert list_len == 22 and max_seqs == 30 and int(gold['n_splits']) == 3


@pytest.fixture(scope='module')
def split3(work):
    g = work / 'genome'
    p = sdgpu('prefilter', g, g, work / 'split3', '--split', '3', '--split-mode', '0', '--max-seqs', '30', *PREF)
    assert 'Target split mode. Searching through 3 splits' in p.stdout
    return p, read_db(str(work / 'split3'))


def test_golden_rows(split3, gold):
    p, got = split3
    starts = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r'Target db start (\d+) to (\d+)', p.stdout)]
    assert starts == [(int(f) + 1, int(f) + int(s)) for f, s in zip(gold['db_from'], gold['db_size'])]
    for i, q in enumerate(gold['queries']):
        a, b = int(gold['merged_off'][i]), int(gold['merged_off'][i + 1])
        want = list(zip(gold['merged_key'][a:b].tolist(), gold['merged_score'][a:b].tolist(), gold['merged_diag'][a:b].tolist()))
        assert rows_of(got[int(q)]) == want, int(q)


def test_live_reference(work, genome, split3, gold):
    """every query of the second genome against the reference's classes run here, split by split"""
    from oracle.pyoracle import ref_available, Ref
    if not ref_available():
        pytest.skip('oracle/_ref/libsdref.so not built (needs the reference tree at build time)')
    db, lengths = genome
    seqs = [db[k][:-1].decode() for k in range(len(db))]
    lens = np.array([len(s) for s in seqs])
    ranges, list_len = plan_of(lengths, 3, 30)
    assert list_len == int(gold['list_len'])
    ref = Ref(6)
    idx = []
    for f, size in ranges:
        off = np.zeros(size + 1, np.uint64)
        off[1:] = np.cumsum(lens[f:f + size])
        idx.append(ref.index(''.join(seqs[f:f + size]).encode(), off))
    got = split3[1]
    second = list(range(4319, len(seqs)))                   # NC_000915 follows the 4 319 proteins of NC_000913
    assert len(second) == 1579

    # (one thread: the reference driver's objects are not built for concurrent use; about 4 700 reference queries)
    pfs = [ix.prefilter(int(lens.max()), max_hits=list_len) for ix in idx]
    bad = []
    for q in second:
        lists = []
        for (f, size), pf in zip(ranges, pfs):
            ids, sc, dg, _ = pf.query(seqs[q], q - f if f <= q < f + size else 0xFFFFFFFF)
            keep = (lens[ids.astype(np.int64) + f].astype(np.float32) / np.float32(lens[q])) >= np.float32(0.8)
            lists.append([(int(t) + f, int(s), int(np.int16(np.uint16(d)))) for t, s, d in zip(ids[keep], sc[keep], dg[keep])])
        if rows_of(got[q]) != merge(lists):
            bad.append(q)
    assert bad == []


@pytest.mark.parametrize('n', [2, 3, 7])
def test_split_run_equals_unsplit_runs_on_physically_split_dbs(work, genome, n):
    g = work / 'genome'
    paths, list_len = sub_dbs(work, genome, n, 30)
    assert list_len == {2: 30, 3: 22, 7: 12}[n] and all(paths)
    per_split = []
    for s, path in enumerate(paths):
        out = work / ('phys_%d_%d' % (n, s))
        sdgpu('prefilter', g, path, out, '-k', '6', '--max-seqs', str(list_len), '--add-self-matches', '1', *PREF)
        per_split.append(read_db(str(out)))
    out = work / ('split_%d' % n)
    p = sdgpu('prefilter', g, g, out, '--split', str(n), '--split-mode', '0', '--max-seqs', '30', '-k', '6', *PREF)
    assert 'Target split mode. Searching through %d splits' % n in p.stdout
    got = read_db(str(out))
    assert sorted(got) == list(range(5898))
    cut = longer = 0
    for q in range(5898):
        lists = [rows_of(d[q]) for d in per_split]
        want = merge(lists)
        assert rows_of(got[q]) == want, q
        cut += any(len(l) == list_len for l in lists)
        longer += len(want) > 30
    assert cut > 0 and longer > 0      # the per-split cut and the uncut merge are both exercised


def pinned(work, db):
    sdgpu('prefixid', work / db, work / (db + '.flat'), '--tsv', '--threads', '1')
    lines = open(work / (db + '.flat')).readlines()
    return len(lines), sorted_md5(lines)


def test_one_split_is_the_pinned_prefilter_db(work):
    g = work / 'genome'
    sdgpu('prefilter', g, g, work / 'one', '--split', '1', '--split-mode', '0', '--max-seqs', '300', *PREF)
    assert pinned(work, 'one') == (98957, '8109a70bdea70ee10e0dbd27ba6b7e37')


def test_query_split_is_the_pinned_prefilter_db(work):
    g = work / 'genome'
    p = sdgpu('prefilter', g, g, work / 'qsplit', '--split', '3', '--split-mode', '1', '--max-seqs', '300', *PREF)
    assert 'Query split mode. Searching through 3 splits' in p.stdout
    assert re.search(r'at k-mer size (\d+)', p.stdout).group(1) == '6'       # residues / 3 is far below the k = 7 threshold
    assert pinned(work, 'qsplit') == (98957, '8109a70bdea70ee10e0dbd27ba6b7e37')


def test_profile_queries(work, genome):
    """a profile DB (result2profile on the module chain's alignments of 300 queries) against a 2-way target split"""
    db, lengths = genome
    g = work / 'genome'
    write_db(str(work / 'q300'), [(k, db[k]) for k in range(0, 5898, 19)][:300], 0)
    sdgpu('prefilter', work / 'q300', g, work / 'q300_pref', '--max-seqs', '300', '--add-self-matches', '1', *PREF)
    sdgpu('align', work / 'q300', g, work / 'q300_pref', work / 'q300_aln', '-a', '1', '--alignment-mode', '2', '-e', '0.001', '-c', '0.8',
          '--cov-mode', '2', '--add-self-matches', '1', '--threads', '8', '-v', '3')
    sdgpu('result2profile', work / 'q300', g, work / 'q300_aln', work / 'q300_prof', '--threads', '8', '-v', '0')
    assert open(work / 'q300_prof.dbtype', 'rb').read()[0] == 2
    paths, list_len = sub_dbs(work, genome, 2, 30)
    per_split = []
    for s, path in enumerate(paths):
        out = work / ('prof_phys_%d' % s)
        sdgpu('prefilter', work / 'q300_prof', path, out, '-k', '6', '--max-seqs', str(list_len), '--add-self-matches', '1', *PREF)
        per_split.append(read_db(str(out)))
    p = sdgpu('prefilter', work / 'q300_prof', g, work / 'prof_split', '--split', '2', '--split-mode', '0', '--max-seqs', '30', '-k', '6',
              '--add-self-matches', '1', *PREF)
    assert 'Query database size: 300 type: Profile' in p.stdout and 'Target split mode. Searching through 2 splits' in p.stdout
    got = read_db(str(work / 'prof_split'))
    assert len(got) == 300
    total = 0
    for q in got:
        want = merge([rows_of(d[q]) for d in per_split])
        assert rows_of(got[q]) == want, q
        total += len(want)
    assert total > 300


def test_automatic_mode(work, genome):
    from spacedust_amd.api import target_footprint
    db, lengths = genome
    g = work / 'genome'
    whole = target_footprint(6, 5898, sum(lengths) - 2 * 5898)
    p = sdgpu('prefilter', g, g, work / 'auto', '--split', '0', '--split-memory-limit', '%dB' % (whole - 1), '--max-seqs', '30', *PREF)
    n = int(re.search(r'Target split mode\. Searching through (\d+) splits', p.stdout).group(1))
    assert n >= 2
    sdgpu('prefilter', g, g, work / 'auto_explicit', '--split', str(n), '--split-mode', '0', '--max-seqs', '30', *PREF)
    assert read_db(str(work / 'auto')) == read_db(str(work / 'auto_explicit'))
    # a limit the whole target fits: one split, no split line
    p = sdgpu('prefilter', g, g, work / 'auto_fits', '--split', '0', '--split-memory-limit', '%dB' % whole, '--max-seqs', '30', *PREF)
    assert 'split mode' not in p.stdout
    # below the footprint of a one-sequence split nothing fits
    p = sdgpu('prefilter', g, g, work / 'auto_none', '--split', '0', '--split-memory-limit', '%dB' % (target_footprint(6, 1, 1) - 1),
              '--max-seqs', '30', *PREF, check=False)
    assert p.returncode != 0 and 'Cannot fit databases into' in p.stderr
    assert not os.path.exists(work / 'auto_none') and not os.path.exists(work / 'auto_none.index')
    p = sdgpu('prefilter', g, g, work / 'auto_many', '--split', '5899', '--split-mode', '0', *PREF, check=False)
    assert p.returncode != 0 and 'the db to split has only 5898 sequences' in p.stderr
    assert not os.path.exists(work / 'auto_many.index')
    # --split N --split-mode 2 with a target that fits: query-split semantics (the rows of the unsplit run)
    p = sdgpu('prefilter', g, g, work / 'detect', '--split', '3', '--split-mode', '2', '--max-seqs', '300', *PREF)
    assert 'Query split mode. Searching through 3 splits' in p.stdout
    assert pinned(work, 'detect') == (98957, '8109a70bdea70ee10e0dbd27ba6b7e37')


def test_footprint_is_an_upper_bound(genome):
    """sd_target_footprint against what sd_target_build held at the fullest point of its phases (hipMemGetInfo inside the build)"""
    from spacedust_amd import api
    db, lengths = genome
    host, gpu = api.Host(), api.Context(0)
    thr = host.kmer_threshold(5.7, 6)
    for name, keys in (('one genome', range(4319, 5898)), ('both genomes', range(5898))):
        res, off = host.map_sequences([db[k][:-1].decode() for k in keys])
        for what, kmer_thr in (('sequence index', thr), ('profile index (threshold 0)', 0)):
            t = api.Target.build_on_device(gpu, host, res, off, k=6, kmer_thr=kmer_thr)
            peak, est = t.build_peak(), api.target_footprint(6, len(off) - 1, int(off[-1]))
            print('%s, %s: estimate %d B, observed peak %d B, estimate / observed %.3f' % (name, what, est, peak, est / max(peak, 1)))
            assert peak > 2 * 8000 * 8000 * 2          # the measurement saw at least the resident 3-mer matrices
            assert est >= peak
            del t


def test_search_workflow_runs_the_module_chain(work):
    g = work / 'genome'
    flags = ['--split', '3', '--split-mode', '0', '--max-seqs', '30', '-s', '5.7']
    p = sdgpu('search', g, g, work / 'wf_res', work / 'wf_tmp', *flags, *ALIGN)
    assert BANNER not in p.stdout and 'Target split mode. Searching through 3 splits' in p.stdout
    sdgpu('prefilter', g, g, work / 'wf_pref', *flags, '-c', '0.8', '--cov-mode', '2', '--threads', '8', '-v', '3')
    sdgpu('align', g, g, work / 'wf_pref', work / 'wf_aln', *ALIGN)
    want = read_db(str(work / 'wf_aln'))
    assert read_db(str(work / 'wf_res')) == want and sum(len(v) for v in want.values()) > 100000
    assert read_db(str(work / 'wf_tmp' / 'pref_0')) == read_db(str(work / 'wf_pref'))


def test_clustersearch_workflow_runs_the_module_chain(work):
    g = work / 'genome'
    flags = ['--split', '3', '--split-mode', '0', '--max-seqs', '30']
    p = sdgpu('clustersearch', g, g, work / 'cs.tsv', work / 'cs_tmp', *flags, '--filter-self-match', '--threads', '8')
    assert BANNER not in p.stdout and 'Target split mode. Searching through 3 splits' in p.stdout
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
    sdgpu('combinehits', g, g, c / 'aggregate_merged', c / 'matches', c, '--alpha', '1', '--aggregation-mode', '0', '--filter-self-match', '1', *common)
    sdgpu('clusterhits', g, g, c / 'matches', c / 'clusters', '--multihit-pval', '0.01', '--cluster-pval', '0.01', '--max-gene-gap', '3',
          '--cluster-size', '2', '--db-output', '1', '--alpha', '1', *common)
    sdgpu('summarizeresults', g, g, c / 'clusters', c / 'result.tsv', *common)
    tsv = open(work / 'cs.tsv').read()
    assert tsv == open(c / 'result.tsv').read() and tsv.count('\n#') + tsv.startswith('#') > 10


def test_iterative_clustersearch_keeps_the_split_prefilter_dbs(work):
    """`clustersearch --num-iterations 2` over a 2-way target split: the module chain's DBs (--keep-tmp 1) are what the split
    prefilter writes for the sequence queries and for the profiles of iteration 1"""
    g = work / 'genome'
    flags = ['--split', '2', '--split-mode', '0', '--max-seqs', '30']
    p = sdgpu('clustersearch', g, g, work / 'it.tsv', work / 'it_tmp', *flags, '--num-iterations', '2', '--keep-tmp', '1', '--filter-self-match',
              '--threads', '8')
    assert BANNER not in p.stdout and p.stdout.count('Target split mode. Searching through 2 splits') == 2
    s = work / 'it_tmp' / 'search'
    pref = ['-s', '5.7', '-k', '0', '-c', '0.8', '--cov-mode', '2', '--threads', '8', '-v', '3']
    sdgpu('prefilter', g, g, work / 'it_pref_0', *flags, *pref)
    assert read_db(str(s / 'pref_0')) == read_db(str(work / 'it_pref_0'))
    assert open(s / 'profile_0.dbtype', 'rb').read()[0] == 2
    sdgpu('prefilter', s / 'profile_0', g, work / 'it_pref_1', *flags, *pref)
    got = read_db(str(s / 'pref_tmp_1'))
    assert got == read_db(str(work / 'it_pref_1')) and max(len(rows_of(v)) for v in got.values()) > 30
    # and without --keep-tmp the same chain runs (the in-memory iterations hold one index of the whole target): the same TSV
    p = sdgpu('clustersearch', g, g, work / 'it2.tsv', work / 'it2_tmp', *flags, '--num-iterations', '2', '--filter-self-match', '--threads', '8')
    assert BANNER not in p.stdout and 'the modules run one after the other in this process' in p.stdout
    tsv = open(work / 'it.tsv').read()
    assert tsv == open(work / 'it2.tsv').read() and tsv.count('\n#') > 10
