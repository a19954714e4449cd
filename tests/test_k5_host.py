"""k = 5 without a GPU: the golden file's own conditions (tools/make_golden_k5.py asserts them where it writes), the two k-mer
thresholds, the host index and the host k-mer generator against the reference's, `createindex -k 5`, and what `-k` refuses before a
device is asked for."""
import numpy as np
import pytest

import k5gold
from dbutil import sdgpu, write_db


@pytest.fixture(scope='module')
def db(host):
    seqs, n_small = k5gold.sequences()
    res, off = host.map_sequences(seqs)
    return seqs, n_small, res, off


def test_golden_conditions():
    g = k5gold.golden()
    seqs, n_small = k5gold.sequences()
    assert all(len(g[k]) > 0 for k in ('lists', 'plists', 'index_triples', 'pf_rows_88', 'pf_rows_75', 'prof_rows_82', 'prof_rows_70',
                                       'PT82_rows', 'PT75_rows'))
    assert len(g['windows']) == 12 and g['window_thr'].min() >= 70 and g['window_thr'].max() <= 110 and (np.diff(g['list_off']) > 0).all()
    assert len(g['pwindows']) == 6 and (np.diff(g['plist_off']) > 0).all()
    assert [len(seqs[int(g['special_len%d' % n])]) for n in (11, 12, 13)] == [11, 12, 13]
    for p in k5gold.SEED:   # an X in seed position p of window 20
        assert seqs[int(g['special_x%d' % p])][20 + p] == 'X'
    assert int(g['index_masked_residues']) > 0   # the tantan-masked stretch
    base = n_small   # the family's base: copy 0
    assert seqs[base] == g['fam_base'].tobytes().decode() and len(seqs[base]) == 300
    queries = [int(q) for q in g['queries']]
    assert set(range(0, n_small, 3)) <= set(queries) and base in queries
    for thr in (88, 75):
        rows = g['pf_rows_%d' % thr]
        # the family base has more index hits than the reference's (and the device's first) hit buffer holds
        assert int(g['index_hits_%d' % thr][queries.index(base)]) > k5gold.HIT_BUFFER
        assert not (rows[:, 0] == int(g['special_len11'])).any()
        assert (rows[:, 0] == int(g['special_len12'])).sum() == 1 and (rows[:, 0] == int(g['special_len13'])).sum() == 1
        assert max(len(set(rows[rows[:, 0] == q, 3] & 0xFFFF)) for q in queries) > 1   # hits on more than one diagonal
    assert len(set(g['prof_rows_82'][:, 0])) > 1 and len(g['PT75_rows']) > len(g['PT82_rows'])


def test_thresholds(host):
    """Prefiltering.cpp:1019-1052 at -s 5.7: int(160.75 - 12.75 s) and, for profiles without context pseudo-counts, int(108.8 - 4.7 s)"""
    assert host.kmer_threshold(5.7, 5) == 88
    assert host.profile_kmer_threshold(5.7, 5) == 82
    assert host.auto_kmer_size(10 ** 6) == 6 and host.auto_kmer_size(4 * 10 ** 9) == 7   # the automatic choice never gives 5


def test_host_index_equals_reference(host, db):
    g = k5gold.golden()
    seqs, n_small, res, off = db
    idx = host.build_index(res[:int(off[n_small])], off[:n_small + 1], k=5, kmer_thr=88)
    assert len(idx.kmer_offsets) == k5gold.TABLE + 1 and idx.block_base is None
    assert idx.masked_residues == int(g['index_masked_residues'])
    got = k5gold.index_triples(idx.kmer_offsets, idx.entry_seq, idx.entry_pos)
    assert np.array_equal(got, g['index_triples'].astype(np.int64))
    assert np.array_equal(idx.masked, g['index_lookup'])


def test_host_kmer_generator_equals_reference(oracle):
    """the 2 + 3 generator of the host stage (what oracle/sd_oracle.cpp restates the prefilter with), in the reference's order"""
    g = k5gold.golden()
    lo = g['list_off'].astype(np.int64)
    for i, (w, thr) in enumerate(zip(g['windows'], g['window_thr'])):
        assert np.array_equal(oracle.kmer_list(w, int(thr), k=5), g['lists'][lo[i]:lo[i + 1]]), i


def test_host_profile_kmer_generator_equals_reference(host, oracle):
    """the one-residue-per-step generator over the five seed positions of a profile window"""
    g = k5gold.golden()
    profiles, _ = k5gold.profile_inputs()
    prof = host.map_profiles(b''.join(profiles), k5gold.offsets_of(profiles))
    lo = g['plist_off'].astype(np.int64)
    for i, (pi, pos, thr) in enumerate(g['pwindows']):
        at = int(prof['offsets'][pi]) + int(pos) + np.array(k5gold.SEED)
        got = oracle.profile_kmer_list(prof['sorted_score'][at], prof['sorted_index'][at], int(thr))
        assert np.array_equal(got, g['plists'][lo[i]:lo[i + 1]]), i


def test_restated_prefilter_equals_reference(oracle, host, db):
    """the scalar restatement at k = 5 on the small queries (the overflowing one is the device's to show, tests/test_gpu_k5.py)"""
    g = k5gold.golden()
    seqs, n_small, res, off = db
    ot = oracle.target(res, off, k=5, kmer_thr=88)
    rows = k5gold.expected_rows(g['pf_rows_88'])
    for q, qid in list(zip(g['queries'], g['query_identity']))[:12]:
        ids, sc, dg, _ = ot.prefilter(res[int(off[q]):int(off[q + 1])], identity_id=int(qid), kmer_thr=88, max_hits=300)
        exp = rows[rows[:, 0] == q]
        assert np.array_equal(ids, exp[:, 1]) and np.array_equal(sc, exp[:, 2]) and np.array_equal(dg, exp[:, 3]), q


def _idx_keys(path):
    index = {int(l.split()[0]): (int(l.split()[1]), int(l.split()[2])) for l in open(path + '.index')}
    data = open(path, 'rb').read()
    return {k: data[o:o + n] for k, (o, n) in index.items()}


def test_createindex_k5_file_holds_the_host_index(tmp_path, host, db):
    """`createindex -k 5`: META names k = 5 and the threshold, ENTRIESOFFSETS has 20^5 + 1 list starts and ENTRIES the 6-byte records --
    read back, they are the arrays sd_host_index_build gives (PrefilteringIndexReader's keys: META 1, ENTRIES 9, ENTRIESOFFSETS 10,
    ENTRIESNUM 12, SEQINDEXDATA 14)"""
    seqs, n_small, res, off = db
    t = str(tmp_path / 'target')
    write_db(t, [(i, s.encode() + b'\n') for i, s in enumerate(seqs[:n_small])], 0)
    sdgpu('createindex', t, tmp_path / 'tmp', '-k', '5', '--k-score', 'seq:88,prof:2147483647', '-v', '0')
    keys = _idx_keys(t + '.idx')
    meta = np.frombuffer(keys[1][:48], np.int32)
    assert meta[1] == 5 and meta[6] == 88 and meta[4] == 1
    idx = host.build_index(res[:int(off[n_small])], off[:n_small + 1], k=5, kmer_thr=88)
    n = int(np.frombuffer(keys[12][:8], np.uint64)[0])
    assert n == idx.n_entries
    starts = np.frombuffer(keys[10][:(k5gold.TABLE + 1) * 8], np.uint64)
    assert np.array_equal(starts, idx.kmer_offsets.astype(np.uint64))
    ent = np.frombuffer(keys[9][:n * 6], np.uint8).reshape(n, 6)
    assert np.array_equal(ent[:, :4].copy().view(np.uint32).reshape(-1), idx.entry_seq)
    assert np.array_equal(ent[:, 4:6].copy().view(np.uint16).reshape(-1), idx.entry_pos)
    assert np.array_equal(np.frombuffer(keys[14][:len(idx.masked)], np.uint8), idx.masked)


def test_refusals_by_their_words(tmp_path):
    profiles, pseqs = k5gold.profile_inputs()
    seq_db, prof_db = str(tmp_path / 'seq'), str(tmp_path / 'prof')
    write_db(seq_db, [(i, s.encode() + b'\n') for i, s in enumerate(pseqs[:8])], 0)
    write_db(prof_db, [(i, p) for i, p in enumerate(profiles[:2])], 2)
    for args, words in ((('-k', '4'), '-k 4: k-mer sizes 5, 6 and 7 are implemented'),
                        (('--target-search-mode', '1', '-k', '5'), 'the similar-k-mer index of --target-search-mode 1 is built at k=6 only'),
                        (('--split', '2', '-k', '5'), '--split 2: a k=5 target index is searched unsplit')):
        p = sdgpu('prefilter', seq_db, seq_db, tmp_path / 'out', '-v', '0', *args, check=False)
        assert p.returncode != 0 and words in p.stderr, (args, p.stderr)
    p = sdgpu('prefilter', seq_db, prof_db, tmp_path / 'out', '-v', '0', '-k', '7', check=False)
    assert p.returncode != 0 and 'k=6 only' in p.stderr and 'k=5 and k=6 only' in p.stderr, p.stderr
    p = sdgpu('createindex', seq_db, tmp_path / 'tmp', '-k', '4', '-v', '0', check=False)
    assert p.returncode != 0 and 'k-mer sizes 5, 6 and 7 are implemented' in p.stderr


def test_footprint_does_not_model_k5():
    """a k = 5 target is searched unsplit: the footprint model stays at 6 and 7"""
    from spacedust_amd.api import target_footprint
    assert target_footprint(5, 10, 10) == 0
