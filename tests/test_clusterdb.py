"""CPU: `sdgpu profile2consensus` and sd_host_profile_consensus against the reference's profile2consensus on the reference's own profile
DBs (tests/golden/clusterdb_vectors.npz), what the two new modules refuse, and the parameter strings `sdgpu makeclusterdb` derives for its five
steps against tests/clusterdb_ref.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cdbgold
import clusterdb_ref as ref
from dbutil import SDGPU, sdgpu, write_db

ANCILLARY = ('_h', '_h.index', '_h.dbtype', '.lookup', '.source')


def _profile_db(tmp, run):
    path = os.path.join(str(tmp), run + '_profile')
    write_db(path, cdbgold.profile_db(run), 2)
    return path


@pytest.mark.parametrize('run', cdbgold.RUNS)
def test_profile2consensus_module(tmp_path, run):
    prof = _profile_db(tmp_path, run)
    for suffix in ANCILLARY[:4]:   # (no .source: a file the profile DB lacks is not linked)
        open(prof + suffix, 'w').write('x' + suffix)
    out = str(tmp_path / 'cons')
    os.symlink(prof + '_h', out + '.source')   # a stale link is replaced, and removed where the source has no such file
    sdgpu('profile2consensus', prof, out, '--threads', 3, '-v', 0)
    assert cdbgold.read_files(out) == cdbgold.db_files(cdbgold.consensus_db(run), 0)
    for suffix in ANCILLARY[:4]:
        assert os.path.islink(out + suffix) and os.path.realpath(out + suffix) == os.path.realpath(prof + suffix), suffix
    assert not os.path.lexists(out + '.source')
    assert len(cdbgold.consensus_db(run)) == len(cdbgold.profile_db(run)) > 0


def test_profile_consensus_api_and_the_max_seq_len_cut():
    from spacedust_amd import api
    host = api.Host(2)
    entries = cdbgold.profile_db('K_r0')
    off = np.zeros(len(entries) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for _, p in entries])
    blob = b''.join(p for _, p in entries)
    want = [t for _, t in cdbgold.consensus_db('K_r0')]
    assert api.profile_consensus(host, blob, off) == want
    # Sequence::mapProfile reads `while (l < maxLen && l < seqLen)`: the first --max-seq-len positions, then the newline
    assert api.profile_consensus(host, blob, off, max_seq_len=70) == [t[:min(70, len(t) - 1)] + b'\n' for t in want]
    assert min(len(t) for t in want) > 71
    # a consensus code outside the alphabet is an error, not a letter
    bad = bytearray(blob)
    bad[21] = 21
    with pytest.raises(api.SdError):
        api.profile_consensus(host, bytes(bad), off)


def test_max_seq_len_reaches_the_module(tmp_path):
    prof = _profile_db(tmp_path, 'K_r1')
    sdgpu('profile2consensus', prof, tmp_path / 'cut', '--max-seq-len', 50, '-v', 0)
    (key, text), = cdbgold.consensus_db('K_r1')
    assert cdbgold.read_files(str(tmp_path / 'cut')) == cdbgold.db_files([(key, text[:50] + b'\n')], 0)


def _refused(*args, env=None):
    p = subprocess.run([SDGPU] + [str(a) for a in args], env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    assert p.returncode != 0, p.stdout
    return p.stderr + p.stdout


def test_profile2consensus_refusals(tmp_path):
    prof = _profile_db(tmp_path, 'K_r1')
    out = str(tmp_path / 'cons')
    assert '--compressed' in _refused('profile2consensus', prof, out, '--compressed', 1)
    assert 'blosum62' in _refused('profile2consensus', prof, out, '--sub-mat', 'VTML80.out')
    assert 'usage' in _refused('profile2consensus', prof)
    seq = str(tmp_path / 'seq')
    write_db(seq, [(0, b'MKVLAAGIVGLLLAQ\n')], 0)
    assert 'not a profile database' in _refused('profile2consensus', seq, out)
    assert '.dbtype not found' in _refused('profile2consensus', tmp_path / 'nothing', out)
    assert not os.path.exists(out) and not os.path.exists(out + '.index')


def test_clusterdb_refusals(tmp_path):
    seq = str(tmp_path / 'seq')
    write_db(seq, [(0, b'MKVLAAGIVGLLLAQ\n')], 0)
    tmp = tmp_path / 'tmp'
    said = _refused('makeclusterdb', seq, tmp)
    assert '--filter-hits' in said and 'linclust' in said            # the cluster module's message
    assert 'foldseek' in _refused('makeclusterdb', seq, tmp, '--single-step-clustering', 1, '--search-mode', 1)
    assert '--compressed' in _refused('makeclusterdb', seq, tmp, '--single-step-clustering', 1, '--compressed', 1)
    assert 'one rank' in _refused('makeclusterdb', seq, tmp, '--single-step-clustering', 1, env={'WORLD_SIZE': '2', 'RANK': '0'})
    assert 'usage: makeclusterdb' in _refused('makeclusterdb', seq, '--single-step-clustering', 1)
    assert 'makeclusterdb ' in sdgpu('--help').stdout
    said = _refused('clusterdb', seq, tmp)   # the reference's name stays unknown (tests/test_clust.py), and says where the workflow is
    assert 'unknown module' in said and 'makeclusterdb' in said
    for dbtype, named in ((1, 'nucleotide'), (2, 'profile')):
        other = str(tmp_path / ('db%d' % dbtype))
        write_db(other, [(0, b'ACGTACGTACGT\n')], dbtype)
        assert named in _refused('makeclusterdb', other, tmp, '--single-step-clustering', 1)
    assert '.dbtype not found' in _refused('makeclusterdb', tmp_path / 'nothing', tmp, '--single-step-clustering', 1)
    for suffix in ('_clu', '_clu_aln', '_clu_rep_profile'):
        assert not os.path.exists(seq + suffix + '.dbtype')


def _plan(tmp_path, user, threads=3, device=None, done=()):
    """the plan `makeclusterdb -v 3` prints; every step's output is marked as there (a .dbtype file), so nothing runs"""
    seq = str(tmp_path / 'seq')
    write_db(seq, [(0, b'MKVLAAGIVGLLLAQ\n')], 0)
    tmp = str(tmp_path / 'tmp')
    os.makedirs(tmp, exist_ok=True)
    outputs = {'cluster': tmp + '/cluster_mmseqs', 'createsubdb': tmp + '/db_clu', 'result2profile': seq + '_clu_rep_profile',
               'profile2consensus': seq + '_clu', 'align': seq + '_clu_aln'}
    for path in outputs.values():
        open(path + '.dbtype', 'wb').write(struct.pack('<i', 0))
    flags = [x for k, v in user.items() for x in (k, v)] + ['--threads', str(threads)] + (['--device', str(device)] if device is not None else [])
    p = sdgpu('makeclusterdb', seq, tmp, *flags)
    got = [l for l in p.stdout.splitlines() if l.startswith('makeclusterdb skips: ') or l.startswith('makeclusterdb runs: ')]
    want = ref.plan_lines(ref.step_args(seq, tmp, threads, user=user, device=device), skipped=set(outputs))
    return got, want


@pytest.mark.parametrize('user,device', [
    ({'--single-step-clustering': '1'}, None),
    ({'--single-step-clustering': '1', '-e': '1e-5', '-c': '0.5', '--cov-mode': '1', '--min-seq-id': '0.3', '-s': '6', '--max-seqs': '50'}, 0),
    ({'--single-step-clustering': '1', '--max-seq-len': '1000', '--sub-mat': 'blosum62.out', '--remove-tmp-files': '0', '--search-mode': '0'}, None),
])
def test_clusterdb_hands_each_step_its_flags(tmp_path, user, device):
    got, want = _plan(tmp_path, user, device=device)
    assert got == want and len(got) == 5
    # the user's -e, -c, ... reach `cluster` alone
    r2p, aln = got[2], got[4]
    for flag in ('-e', '-c', '--cov-mode', '--min-seq-id', '-s', '--max-seqs', '--single-step-clustering'):
        assert (' %s ' % flag) not in r2p and (' %s ' % flag) not in aln
    assert ' --min-seq-id %s ' % user.get('--min-seq-id', '0.7') in got[0] + ' ' and ' -c %s ' % user.get('-c', '0.8') in got[0]
    assert '--search-mode' not in got[0]


def rows(run, key):
    return [l.split(b'\t') for l in dict(cdbgold.cluster_db(run))[key].splitlines()]


def test_what_the_classes_of_the_vectors_hold():
    """the properties the generator asserted, read back from the file: the vectors exercise what they are named for"""
    g = cdbgold.golden()
    want = cdbgold.pairs('K_r0')
    k = cdbgold.class_key('singleton')
    assert rows('K_r0', k) == [[b'%d' % k]] and set(want[(k, k)][2]) == {'M'}
    bts = [want[(cdbgold.class_key('indels'), int(r[0]))][2] for r in rows('K_r0', cdbgold.class_key('indels'))]
    assert any('IIIII' in b for b in bts) and any('DDDDD' in b for b in bts)
    k = cdbgold.class_key('local')
    assert all(want[(k, int(r[0]))][0] > 0 and want[(k, int(r[0]))][1] > 0 for r in rows('K_r0', k)[1:])
    assert len(g['K_bias_pairs']) > 0 and len(g['K_comp_bias_pairs']) > 0
    for suffix, listed in (('_b0', 'K_bias_pairs'), ('_nb', 'K_comp_bias_pairs')):   # the two settings matter: other starts or backtraces
        off, other = g['K_r0_pair_bt_off' + suffix].astype(np.int64), g['K_r0_pair_bt' + suffix].tobytes()
        differ = {(int(q), int(t)) for i, (q, t) in enumerate(zip(g['K_r0_pair_q'], g['K_r0_pair_t']))
                  if (int(g['K_r0_pair_qstart' + suffix][i]), int(g['K_r0_pair_tstart' + suffix][i]), other[off[i]:off[i + 1]].decode()) != want[(int(q), int(t))]}
        assert differ == {(int(q), int(t)) for q, t in g[listed]}
    msa = {int(k): (int(n), int(kept)) for k, n, kept in g['K_r0_msa']}
    assert 2 < msa[cdbgold.class_key('diversity')][1] < msa[cdbgold.class_key('diversity')][0] == 32
    assert sorted({len(r) for r in rows('K_r1', cdbgold.class_key('mixed'))}) == [1, 11]
    assert cdbgold.class_key('missing_query') not in cdbgold.q_keys()
