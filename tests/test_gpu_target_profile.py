"""GPU: the prefilter against a profile target DB -- the similar-k-mer index sd_target_build_profile builds and the exact-k-mer
query mode of sd_prefilter_batch -- against the reference's own IndexTable::addSimilarSequence and QueryMatcher (takeOnlyBestKmer),
recorded by tools/make_golden_target_profile.py; through the C ABI, the Python binding and `sdgpu prefilter`."""
import numpy as np
import pytest

import tpref
from dbutil import read_db, sdgpu, write_db
from spacedust_amd import api

pytestmark = pytest.mark.gpu

ROW_SETS = ((110, 1), (95, 1), (110, 0))


def _prof(host, name):
    g = tpref.golden()
    data = g[name + '_profiles'].tobytes()
    poff = g[name + '_poff'] if name + '_poff' in g else np.array([0, len(data)], np.uint64)
    return host.map_profiles(data, poff)


@pytest.fixture(scope='module')
def g_prof(host):
    data, poff = tpref.g_profiles()
    return host.map_profiles(data, poff)


@pytest.fixture(scope='module')
def g_targets(gpu, host, g_prof):
    """set G at both thresholds, built once"""
    return {thr: api.Target.build_profile_on_device(gpu, host, g_prof, k=6, kmer_thr=thr) for thr in (110, 95)}


@pytest.fixture(scope='module')
def g_queries(host):
    letters, off = tpref.queries()
    seqs = [letters[int(off[i]):int(off[i + 1])].decode() for i in range(len(off) - 1)]
    res, off2 = host.map_sequences(seqs)
    assert (off2 == off).all()
    return seqs, res, off


@pytest.mark.parametrize('name', ['S', 'R'])
def test_full_index_equals_reference(gpu, host, name):
    g = tpref.golden()
    prof = _prof(host, name)
    t = api.Target.build_profile_on_device(gpu, host, prof, k=6, kmer_thr=int(g[name + '_thr']))
    d = t.download()
    exp = g[name + '_triples'].astype(np.int64)
    assert t.build_stats['entries'] == d['n_entries'] == len(exp)
    assert t.build_stats['records'] == int(g[name + '_records']) and t.build_stats['masked_residues'] == 0
    assert np.array_equal(tpref.triples_of_download(d), exp)
    assert int(d['starts'][-1]) == len(exp) and len(d['starts']) == 64000001
    assert np.array_equal(d['masked'], g[name + '_lookup']) and np.array_equal(d['masked'], prof['consensus'])


@pytest.mark.parametrize('thr', [110, 95])
def test_g_index_counts_and_digest(g_targets, thr):
    g = tpref.golden()
    t = g_targets[thr]
    tag = 'G%d' % thr
    assert t.build_stats['entries'] == int(g[tag + '_entries']) and t.build_stats['records'] == int(g[tag + '_records'])
    assert t.build_stats['passes'] == 1
    d = t.download()
    assert np.array_equal(np.bincount(d['entry_seq'], minlength=18), g[tag + '_per_target'])
    assert int((np.diff(d['starts'].astype(np.int64)) > 0).sum()) == int(g[tag + '_lists'])
    assert tpref.digest_of_download(d) == str(g[tag + '_digest'])
    assert t.build_peak() > 0


def test_g_index_in_many_passes(gpu, host, g_prof, monkeypatch):
    """SD_INDEX_PASS bounds the records of a pass: the generator recounts and rewrites per k-mer range, the index is the same"""
    g = tpref.golden()
    monkeypatch.setenv('SD_INDEX_PASS', '50000')
    t = api.Target.build_profile_on_device(gpu, host, g_prof, k=6, kmer_thr=110)
    assert t.build_stats['passes'] > 1 and t.build_stats['entries'] == int(g['G110_entries'])
    assert tpref.digest_of_download(t.download()) == str(g['G110_digest'])


def test_big_tier_window(gpu, host):
    """set B: window lists beyond PROFILE_PARTIAL_CAP (65 536) partial k-mers run in the second scratch tier (two tiers are kept,
    as for profile queries)"""
    g = tpref.golden()
    t = api.Target.build_profile_on_device(gpu, host, _prof(host, 'B'), k=6, kmer_thr=int(g['B_thr']))
    assert t.build_stats['records'] == int(g['B_records']) == int(g['B_window_len'].sum())
    assert t.build_stats['entries'] == int(g['B_entries'])
    assert tpref.digest_of_download(t.download()) == str(g['B_digest'])


@pytest.mark.parametrize('path', ['join', 'lookup'])
@pytest.mark.parametrize('thr,bias', ROW_SETS)
def test_rows_equal_reference(gpu, host, g_targets, g_queries, monkeypatch, thr, bias, path):
    g = tpref.golden()
    seqs, res, off = g_queries
    if path == 'lookup':
        monkeypatch.setenv('SD_PF_JOIN', '0')
    else:
        monkeypatch.delenv('SD_PF_JOIN', raising=False)
    _, dg_b, km_b = host.comp_bias(res, off)
    if not bias:
        dg_b = np.zeros_like(dg_b)
    ident = np.full(len(seqs), 0xFFFFFFFF, np.uint32)
    rows = g['rows_%d_bias%d' % (thr, bias)].astype(np.int64)
    windows = np.array([tpref.windows_without_x(s.encode()) for s in seqs], np.int64)
    assert np.array_equal(windows, g['rows_%d_bias%d_kmers' % (thr, bias)])   # the reference's kmerListLen
    got = {}
    for kmer_thr in (0, 200):   # ignored: the mode belongs to the target
        par = api.prefilter_params(host, 18, kmer_thr=kmer_thr, max_hits=300, min_diag=15, cov_mode=0, cov_thr=0.0, k=6)
        hits, cnt, st = api.prefilter(gpu, g_targets[thr], par, res, off, km_b, dg_b, ident, want_stats=True)
        out = []
        for q in range(len(cnt)):
            for h in hits[q, :int(cnt[q])]:
                out.append((q, int(h['seqId']), int(h['score']), int(h['diagonal'])))
        got[kmer_thr] = np.array(out, np.int64).reshape(-1, 4)
        assert np.array_equal(st[:, 0].astype(np.int64), windows)
        exp = rows.copy()
        exp[:, 3] &= 0xFFFF
        assert np.array_equal(got[kmer_thr], exp), (thr, bias, path, kmer_thr)
    assert len(got[0]) >= (60 if thr == 110 else 140)


def test_refusals(gpu, host, g_prof, g_targets):
    par = api.prefilter_params(host, 18, kmer_thr=110, max_hits=300, cov_thr=0.0, k=6)
    with pytest.raises(api.SdError) as e:
        api.prefilter_profile(gpu, g_targets[110], par, g_prof)
    assert '(-5)' in str(e.value) and 'profile queries cannot be searched against a profile target' in str(e.value)
    # 65 536 positions: index positions are 16 bit (Host.map_profiles cuts at 65 535 as the reference does, so the arrays are made here)
    n = 65536
    long_prof = dict(letters=np.zeros(n, np.uint8), consensus=np.zeros(n, np.uint8), sorted_score=np.zeros((n, 20), np.int16),
                     sorted_index=np.tile(np.arange(20, dtype=np.uint8), (n, 1)), offsets=np.array([0, n], np.uint64))
    with pytest.raises(api.SdError) as e:
        api.Target.build_profile_on_device(gpu, host, long_prof, k=6, kmer_thr=110)
    assert '(-3)' in str(e.value) and '65535' in str(e.value)
    with pytest.raises(api.SdError) as e:
        api.Target.build_profile_on_device(gpu, host, g_prof, k=7, kmer_thr=110)
    assert '(-5)' in str(e.value) and 'k=7' in str(e.value) and 'k=6 only' in str(e.value)


def test_cli_prefilter_against_profile_db(tmp_path, g_queries):
    g = tpref.golden()
    seqs, _, _ = g_queries
    data, poff = tpref.g_profiles()
    seq_db, prof_db = str(tmp_path / 'seq'), str(tmp_path / 'prof')
    write_db(seq_db, [(i, s.encode() + b'\n') for i, s in enumerate(seqs)], 0)
    write_db(prof_db, [(i, data[int(poff[i]):int(poff[i + 1])]) for i in range(len(poff) - 1)], 2)
    common = ['--k-score', 'seq:2147483647,prof:110', '--max-seqs', '300', '--min-ungapped-score', '15', '-c', '0', '--comp-bias-corr', '1',
              '-v', '0']
    sdgpu('prefilter', seq_db, prof_db, tmp_path / 'out', *common)
    db = read_db(str(tmp_path / 'out'))
    rows = g['rows_110_bias1'].astype(np.int64)
    assert sorted(db) == list(range(len(seqs)))
    for q in range(len(seqs)):
        exp = ''.join('%d\t%d\t%d\n' % (t, s, int(np.int16(np.uint16(d & 0xFFFF)))) for _, t, s, d in rows[rows[:, 0] == q])
        assert db[q].decode() == exp, q
    # --mask is ignored for a profile target
    sdgpu('prefilter', seq_db, prof_db, tmp_path / 'out_mask0', '--mask', '0', *common)
    assert read_db(str(tmp_path / 'out_mask0')) == db
    p = sdgpu('prefilter', seq_db, prof_db, tmp_path / 'out2', '--split', '2', *common, check=False)
    assert p.returncode != 0 and 'a profile target database is searched unsplit' in p.stderr
    p = sdgpu('prefilter', prof_db, prof_db, tmp_path / 'out3', *common, check=False)
    assert p.returncode != 0 and 'Query-profiles cannot be searched against a target-profile database' in p.stderr
    write_db(str(tmp_path / 'prof2'), [(i, data[int(poff[i]):int(poff[i + 1])]) for i in range(3)], 2)
    p = sdgpu('prefilter', tmp_path / 'prof2', prof_db, tmp_path / 'out4', *common, check=False)
    assert p.returncode != 0 and 'Query-profiles cannot be searched against a target-profile database' in p.stderr
    p = sdgpu('prefilter', seq_db, prof_db, tmp_path / 'out5', '-k', '7', *common, check=False)
    assert p.returncode != 0 and 'k=6 only' in p.stderr
    p = sdgpu('ungappedprefilter', seq_db, prof_db, tmp_path / 'out6', check=False)
    assert p.returncode != 0 and 'profile target databases are not supported' in p.stderr
