"""Rescoring on the diagonal on the GPU (sd_rescore.hip, `sdgpu rescorediagonal`, `--alignment-mode 4`) against
tests/golden/rescore_diag_vectors.npz (written from the reference's DistanceCalculator::computeUngappedAlignment) and the
restatement of tests/rescore_ref.py."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rescore_ref as rr
from dbutil import sorted_md5, sdgpu, example_fasta, read_db, SDGPU

pytestmark = pytest.mark.gpu
FIELDS = rr.FIELDS + ('idCnt',)


@pytest.fixture(scope='module')
def gold():
    g = np.load(rr.GOLDEN)
    letters, off = g['letters'].tobytes(), g['off']
    return dict(M=g['M'].astype(np.int64), seqs=[letters[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)],
                cls=[str(c) for c in g['cls']], q=g['q'], t=g['t'], diag=g['diag'], ref={0: g['ref0'], 1: g['ref1'], 2: g['ref2']})


def table(out):
    return np.stack([out[f].astype(np.int64) for f in FIELDS], axis=1)


def test_c_abi_equals_every_golden_case(gold, host, gpu):
    g = gold
    assert {'len', 'enc', 'long32767', 'long32768', 'long65535', 'tie_max', 'tie_zero', 'negative', 'letters'} <= set(g['cls'])
    assert {1, 2, 63, 64, 65, 255, 256, 257, 1025, 32767, 32768, 65535} <= {len(s) for s in g['seqs']}
    assert np.array_equal(host.matrix(0)[0].reshape(21, 21), g['M'])
    seqs = gpu.letterset(host, g['seqs'])
    for mode in (0, 1, 2):
        got = table(gpu.rescore_diagonal(host, seqs, seqs, g['q'], g['t'], g['diag'], mode=mode))
        # the six fields are the reference's; the identity count is the restatement's over the reference's [start, end]
        want = np.array([rr.compute(g['M'], g['seqs'][q], g['seqs'][t], d, mode) for q, t, d in zip(g['q'], g['t'], g['diag'])], np.int64)
        assert np.array_equal(want[:, :6], g['ref'][mode])
        bad = np.nonzero((got != want).any(axis=1))[0]
        print('mode %d: %d cases, %d mismatches' % (mode, len(want), len(bad)))
        assert len(bad) == 0, [(int(i), g['cls'][i], got[i].tolist(), want[i].tolist()) for i in bad[:8]]


def test_large_ragged_batch_equals_restatement(gold, host, gpu):
    """more than 2^16 hits over 300 short sequences: several hits per workgroup, the last partial workgroup, the grid stride"""
    rng = np.random.default_rng(11)
    aa = np.array(list('ACDEFGHIKLMNPQRSTVWYXBZ'))
    base = ''.join(rng.choice(aa[:20], 700))
    seqs = []
    for i in range(300):
        n = int(rng.integers(1, 520))
        s = np.array(list(base[int(rng.integers(0, 150)):][:n]))
        hit = rng.random(len(s)) < 0.25
        s[hit] = rng.choice(aa, int(hit.sum()))
        s = ''.join(s)
        seqs.append(s.lower() if i % 17 == 0 else s)
    n = 65536 + 4099
    hq, ht = rng.integers(0, 300, n), rng.integers(0, 300, n)
    lens = np.array([len(s) for s in seqs])
    hd = rng.integers(-(lens[ht] + 2), lens[hq] + 3)   # from beside the target to beside the query
    dev = gpu.letterset(host, seqs)
    for mode in (2, 1, 0):
        got = table(gpu.rescore_diagonal(host, dev, dev, hq, ht, hd, mode=mode))
        want = rr.rescore_batch(gold['M'], seqs, seqs, hq, ht, hd, mode)
        bad = np.nonzero((got != want).any(axis=1))[0]
        print('mode %d: %d hits, %d default records, %d mismatches' % (mode, n, int((want[:, 0] == 0).sum()), len(bad)))
        assert len(bad) == 0, [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:8]]


def test_profile_sets_and_sets_without_letters_are_refused(host, gpu):
    from spacedust_amd.api import SdError
    res, off = host.map_sequences(['MKVLAAGIVG', 'MKVLA'])
    plain = gpu.seqset(res, off)
    with pytest.raises(SdError, match='letters'):
        gpu.rescore_diagonal(host, plain, plain, [0], [1], [0])
    prof = gpu.profileset(res, off, np.zeros((len(res), 21), np.int8))
    with pytest.raises(SdError, match=r'\(-5\)'):
        gpu.rescore_diagonal(host, prof, plain, [0], [1], [0])
    lett = gpu.letterset(host, ['MKVLAAGIVG', 'MKVLA'])
    with pytest.raises(SdError, match=r'\(-3\)'):
        gpu.rescore_diagonal(host, lett, lett, [2], [1], [0])


# ---- the module and the workflows on the example genomes -----------------------------------------------------------------------

PREF_PAR = '-s 5.7 --max-seqs 300 -c 0.8 --cov-mode 2 --threads 8'.split()
RESCORE_PAR = '--rescore-mode 2 -a 1 -e 10 -c 0.8 --cov-mode 2 --min-aln-len 30 --threads 8'.split()


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('rescore')
    fa = example_fasta(tmp)
    sdgpu('createsetdb', fa[0], fa[1], tmp / 'genome', tmp / 'tmp', '-v', '0')
    sdgpu('prefilter', tmp / 'genome', tmp / 'genome', tmp / 'pref', *PREF_PAR)
    return tmp


@pytest.fixture(scope='module')
def dbs(work, host):
    seqs = {k: v.rstrip(b'\n') for k, v in read_db(str(work / 'genome')).items()}
    pref = {k: [tuple(int(x) for x in l.split('\t')) for l in v.decode().splitlines()] for k, v in read_db(str(work / 'pref')).items()}
    total = sum(len(s) for s in seqs.values())
    return dict(seqs=seqs, pref=pref, M=host.matrix(0)[0].reshape(21, 21).astype(np.int64), evalue=lambda s, n: host.evalue(total, s, n),
                bitscore=host.bitscore)


def flat(work, db):
    sdgpu('prefixid', work / db, work / (os.path.basename(str(db)) + '.flat'), '--tsv', '--threads', '1')
    return open(work / (os.path.basename(str(db)) + '.flat')).readlines()


_FIELDS = {}


def restated(dbs, **kw):
    """every entry of the prefilter DB through rescore_ref.rows; the per-hit values of a mode come from one vectorised
    rescore_batch over all hits (tests/test_rescore_restatement.py holds it against the per-hit form)"""
    mode = kw['mode']
    keys = sorted(dbs['pref'])
    if mode not in _FIELDS:
        order = sorted(dbs['seqs'])
        at = {k: i for i, k in enumerate(order)}
        hq = [at[k] for k in keys for _ in dbs['pref'][k]]
        ht = [at[r[0]] for k in keys for r in dbs['pref'][k]]
        hd = [r[2] for k in keys for r in dbs['pref'][k]]
        seqs = [dbs['seqs'][k] for k in order]
        _FIELDS[mode] = rr.rescore_batch(dbs['M'], seqs, seqs, hq, ht, hd, mode)
    out, x = {}, 0
    for k in keys:
        n = len(dbs['pref'][k])
        out[k] = rr.rows(dbs['M'], dbs['seqs'][k], dbs['seqs'].__getitem__, k, dbs['pref'][k], dbs['evalue'], dbs['bitscore'],
                         fields=_FIELDS[mode][x:x + n], **kw)
        x += n
    return out


def test_module_mode_2_equals_restated_rows(work, dbs):
    g = work / 'genome'
    sdgpu('rescorediagonal', g, g, work / 'pref', work / 'resc2', *RESCORE_PAR)
    assert open(str(work / 'resc2') + '.dbtype', 'rb').read()[:1] == b'\x05'   # alignment result type
    got = read_db(str(work / 'resc2'))
    assert set(got) == set(dbs['pref'])
    want = restated(dbs, mode=2, e=10.0, c=0.8, cov_mode=2, a=True, min_aln_len=30)
    assert sum(v.count('\n') for v in want.values()) > 5000
    for k in want:   # every entry, line for line, in input order
        assert got[k].decode() == want[k], k
    sdgpu('rescorediagonal', g, g, work / 'pref', work / 'resc2s', *RESCORE_PAR, '--sort-results', '1')
    got_s = read_db(str(work / 'resc2s'))
    want_s = restated(dbs, mode=2, e=10.0, c=0.8, cov_mode=2, a=True, min_aln_len=30, sort=True)
    assert any(want_s[k] != want[k] for k in want)
    for k in want_s:
        assert got_s[k].decode() == want_s[k], k


@pytest.mark.parametrize('mode', [1, 0])
def test_module_modes_0_and_1_equal_restated_rows(work, dbs, mode):
    g = work / 'genome'
    par = ['--rescore-mode', str(mode), '-e', '10', '-c', '0.8', '--cov-mode', '2', '--min-seq-id', '0.3' if mode == 0 else '0', '--threads', '8']
    out = work / ('resc%d' % mode)
    sdgpu('rescorediagonal', g, g, work / 'pref', out, *par, '--sort-results', '1')
    assert open(str(out) + '.dbtype', 'rb').read()[:1] == b'\x07'   # the input's type
    got = read_db(str(out))
    assert set(got) == set(dbs['pref'])
    want = restated(dbs, mode=mode, e=10.0, c=0.8, cov_mode=2, min_seq_id=0.3 if mode == 0 else 0.0, sort=True)
    assert sum(v.count('\n') for v in want.values()) > 500
    for k in want:
        assert got[k].decode() == want[k], k


@pytest.mark.parametrize('pmode', [0, 1])
def test_search_alignment_mode_4_equals_module_chain(work, pmode):
    g = work / 'genome'
    if pmode == 0:
        pref = work / 'pref'
    else:
        pref = work / 'upref'
        sdgpu('ungappedprefilter', g, g, pref, '--max-seqs', '300', '-c', '0.8', '--cov-mode', '2', '--threads', '8')
    chain_db = work / ('chain%d' % pmode)
    sdgpu('rescorediagonal', g, g, pref, chain_db, *RESCORE_PAR)
    fused_db = work / ('fused%d' % pmode)
    sdgpu('search', g, g, fused_db, work / ('tmps%d' % pmode), '--alignment-mode', '4', '--prefilter-mode', str(pmode), '-s', '5.7', '--max-seqs',
          '300', '-a', '1', '-e', '10', '-c', '0.8', '--cov-mode', '2', '--min-aln-len', '30', '--threads', '8')
    chain, fused = flat(work, chain_db), flat(work, fused_db)
    assert len(chain) > 5000 and fused == chain
    assert sorted_md5(flat(work, 'tmps%d/pref_0' % pmode)) == sorted_md5(flat(work, pref))


def test_clustersearch_alignment_mode_4_equals_module_chain(work):
    g = work / 'genome'
    sdgpu('clustersearch', g, g, work / 'fused4.tsv', work / 'tmpc4', '--alignment-mode', '4', '--filter-self-match', '--threads', '8')
    sdgpu('rescorediagonal', g, g, work / 'pref', work / 'caln', *RESCORE_PAR)
    common = ['--threads', '8', '-v', '3']
    sdgpu('prefixid', work / 'caln', work / 'c_prefixed', *common)
    sdgpu('besthitbyset', g, g, work / 'c_prefixed', work / 'c_aggregate', '--simple-best-hit', '1', '--suboptimal-hits', '0', *common)
    sdgpu('mergeresultsbyset', str(g) + '_set_to_member', work / 'c_aggregate', work / 'c_merged', *common)
    sdgpu('combinehits', g, g, work / 'c_merged', work / 'c_matches', work / 'tmp', '--alpha', '1', '--aggregation-mode', '0',
          '--filter-self-match', '1', *common)
    sdgpu('clusterhits', g, g, work / 'c_matches', work / 'c_clusters', '--multihit-pval', '0.01', '--cluster-pval', '0.01', '--max-gene-gap', '3',
          '--cluster-size', '2', '--db-output', '1', '--alpha', '1', *common)
    sdgpu('summarizeresults', g, g, work / 'c_clusters', work / 'chain4.tsv', *common)
    fused, chain = open(work / 'fused4.tsv').readlines(), open(work / 'chain4.tsv').readlines()
    assert sum(1 for l in chain if l.startswith('#')) >= 1   # the comparison is over clusters, not over two empty files
    assert sorted_md5(fused, drop_first_column=True) == sorted_md5(chain, drop_first_column=True)
    # not the Smith-Waterman result
    sdgpu('clustersearch', g, g, work / 'fused2.tsv', work / 'tmpc2', '--filter-self-match', '--threads', '8')
    assert sorted_md5(open(work / 'fused2.tsv').readlines(), drop_first_column=True) != sorted_md5(fused, drop_first_column=True)


def test_refusals(work):
    g, pref = work / 'genome', work / 'pref'

    def refused(*args):
        p = subprocess.run([SDGPU] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode != 0, args
        return p.stderr
    assert '--rescore-mode 3' in refused('rescorediagonal', g, g, pref, work / 'r1', '--rescore-mode', '3')
    assert '--rescore-mode 4' in refused('rescorediagonal', g, g, pref, work / 'r1', '--rescore-mode', '4')
    assert '--filter-hits' in refused('rescorediagonal', g, g, pref, work / 'r1', '--rescore-mode', '2', '--filter-hits', '1')
    assert '--wrapped-scoring' in refused('rescorediagonal', g, g, pref, work / 'r1', '--rescore-mode', '2', '--wrapped-scoring', '1')
    assert '--compressed' in refused('rescorediagonal', g, g, pref, work / 'r1', '--rescore-mode', '2', '--compressed', '1')
    assert '--num-iterations' in refused('search', g, g, work / 'r1', work / 'tmpr', '--alignment-mode', '4', '--num-iterations', '2')
    assert '--num-iterations' in refused('clustersearch', g, g, work / 'r1.tsv', work / 'tmpr', '--alignment-mode', '4', '--num-iterations', '3')
    for name, dbtype in (('nucl', 1), ('prof', 2)):
        for ext in ('', '.index'):
            shutil.copy(str(g) + ext, str(work / name) + ext)
        open(str(work / name) + '.dbtype', 'wb').write(struct.pack('<i', dbtype))
    assert 'nucleotide' in refused('rescorediagonal', work / 'nucl', g, pref, work / 'r2', '--rescore-mode', '2')
    assert 'nucleotide' in refused('rescorediagonal', g, work / 'nucl', pref, work / 'r2', '--rescore-mode', '2')
    assert 'profile' in refused('rescorediagonal', work / 'prof', g, pref, work / 'r2', '--rescore-mode', '2')
    assert 'profile' in refused('rescorediagonal', g, work / 'prof', pref, work / 'r2', '--rescore-mode', '2')
    for ext in ('', '.index'):
        shutil.copy(str(pref) + ext, str(work / 'revpref') + ext)
    open(str(work / 'revpref') + '.dbtype', 'wb').write(struct.pack('<i', 14))
    assert 'reverse' in refused('rescorediagonal', g, g, work / 'revpref', work / 'r3', '--rescore-mode', '2')
    for name in ('r1', 'r2', 'r3'):
        assert not os.path.exists(str(work / name) + '.index'), name
