"""GPU: sd_r2p_realign -- result2profile's own alignment of the rows that carry none -- against the reference's Matcher per pair, and
`sdgpu result2profile` on a cluster DB against the reference's result2profile, byte for byte (tests/golden/clusterdb_vectors.npz)."""
import functools
import os

import numpy as np
import pytest

import cdbgold
from dbutil import sdgpu, write_db

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def device():
    from spacedust_amd import api
    host, ctx = api.Host(4), api.Context(0)
    aa2num = np.asarray(host.matrix(0)[2], np.uint8)
    seqs = cdbgold.sequences()
    t_off = np.zeros(len(seqs) + 1, np.uint64)
    t_off[1:] = np.cumsum([len(s) for _, s in seqs])
    t_res = aa2num[np.frombuffer(b''.join(s for _, s in seqs), np.uint8)]
    id_of = {k: i for i, (k, _) in enumerate(seqs)}
    return api, host, ctx, t_res, t_off, id_of


def layout(entries):
    """entries: [(centre key, [member key ...])] -> the arrays of api.r2p_realign and the (centre, member) key of every edge"""
    _, _, _, t_res, t_off, id_of = device()
    q_let, q_off, edge_off, edge_t, edge_keys = [], [0], [0], [], []
    for centre, members in entries:
        c = id_of[centre]
        q_let.append(t_res[int(t_off[c]):int(t_off[c + 1])])
        q_off.append(q_off[-1] + len(q_let[-1]))
        edge_t += [id_of[m] for m in members]
        edge_keys += [(centre, m) for m in members]
        edge_off.append(len(edge_t))
    return np.concatenate(q_let), np.array(q_off, np.uint64), np.array(edge_off, np.uint64), np.array(edge_t, np.uint32), edge_keys


def rows(run, key):
    return [l.split(b'\t') for l in dict(cdbgold.cluster_db(run))[key].splitlines()]


def check(got, edge_keys, run='K_r0'):
    qs, ts, bts = got
    want = cdbgold.pairs(run)
    for e, pair in enumerate(edge_keys):
        assert (int(qs[e]), int(ts[e]), bts[e]) == want[pair], pair


@pytest.mark.parametrize('cls', [c for c in cdbgold.classes() if c != 'missing_query'])
def test_realign_per_class(cls):
    api, host, ctx, t_res, t_off, _ = device()
    key = cdbgold.class_key(cls)
    q_let, q_off, edge_off, edge_t, edge_keys = layout([(key, [int(r[0]) for r in rows('K_r0', key)])])
    check(api.r2p_realign(ctx, host, q_let, q_off, edge_off, edge_t, t_res, t_off), edge_keys)
    assert len(edge_keys) >= 1


def all_entries():
    return [(k, [int(r[0]) for r in rows('K_r0', k)]) for k, _ in cdbgold.cluster_db('K_r0') if k in set(cdbgold.q_keys())]


def test_all_pairs_shuffled_into_one_call():
    api, host, ctx, t_res, t_off, _ = device()
    rng = np.random.default_rng(5)
    entries = all_entries()
    entries = [(k, [m[i] for i in rng.permutation(len(m))]) for k, m in (entries[i] for i in rng.permutation(len(entries)))]
    q_let, q_off, edge_off, edge_t, edge_keys = layout(entries)
    targets = ctx.seqset(t_res, t_off)   # resident target sequences, as the workflow provides them
    check(api.r2p_realign(ctx, host, q_let, q_off, edge_off, edge_t, t_res, t_off, targets=targets), edge_keys)
    assert len(edge_keys) == len(cdbgold.pairs('K_r0'))


def test_small_pool_is_retried_with_the_bound_the_stage_names():
    api, host, ctx, t_res, t_off, _ = device()
    q_let, q_off, edge_off, edge_t, edge_keys = layout(all_entries()[:6])
    got = api.r2p_realign(ctx, host, q_let, q_off, edge_off, edge_t, t_res, t_off, pool_cap=100, want_stats=True)
    assert got[3] == 2
    check(got[:3], edge_keys)
    with pytest.raises(api.SdError, match=r'\(-4\)'):   # SD_ENOMEM, nothing written
        api.r2p_realign(ctx, host, q_let, q_off, edge_off, edge_t, t_res, t_off, pool_cap=100, retry=False)
    assert api.r2p_realign(ctx, host, q_let, q_off, edge_off, edge_t, t_res, t_off, want_stats=True)[3] == 1


def test_mixed_edges_keep_what_they_carry():
    """edges with a backtrace of their own stay as they are, in place, among the realigned ones"""
    api, host, ctx, t_res, t_off, _ = device()
    key = cdbgold.class_key('mixed')
    r = rows('K_r1', key)
    q_let, q_off, edge_off, edge_t, edge_keys = layout([(key, [int(x[0]) for x in r])])
    flags = [len(x) < 11 for x in r]
    qs = [0 if f else int(x[4]) for f, x in zip(flags, r)]
    ts = [0 if f else int(x[7]) for f, x in zip(flags, r)]
    held = ['' if f else api.uncompress_cigar(x[10].decode()) for f, x in zip(flags, r)]
    got = api.r2p_realign(ctx, host, q_let, q_off, edge_off, edge_t, t_res, t_off, realign=flags, edge_qstart=qs, edge_tstart=ts, backtraces=held)
    want = cdbgold.pairs('K_r1')
    for e, pair in enumerate(edge_keys):
        if flags[e]:
            assert (int(got[0][e]), int(got[1][e]), got[2][e]) == want[pair], pair
        else:
            assert (int(got[0][e]), int(got[1][e]), got[2][e]) == (qs[e], ts[e], held[e]), pair
    assert 0 < sum(flags) < len(flags)


@pytest.mark.parametrize('run', cdbgold.RUNS)
def test_result2profile_on_a_cluster_db(tmp_path, run):
    """the cluster DB's rows realigned inside the module; an entry whose key db_clu lacks is skipped (K_r0 holds one)"""
    t, q, r = cdbgold.write_inputs(tmp_path, run)
    out = str(tmp_path / 'profile')
    said = sdgpu('result2profile', q, t, r, out, '--threads', 4).stdout
    assert cdbgold.read_files(out) == cdbgold.db_files(cdbgold.profile_db(run), 2)
    assert 'pairs realigned' in said
    if run == 'K_r0':
        assert len(cdbgold.cluster_db(run)) == len(cdbgold.profile_db(run)) + 1


def test_result2profile_retries_a_small_pool(tmp_path):
    t, q, r = cdbgold.write_inputs(tmp_path)
    out = str(tmp_path / 'profile')
    env = dict(os.environ, SD_R2P_REALIGN_POOL='64')
    import subprocess
    from dbutil import SDGPU
    subprocess.run([SDGPU, 'result2profile', q, t, r, out, '--threads', '4', '-v', '0'], env=env, check=True)
    assert cdbgold.read_files(out) == cdbgold.db_files(cdbgold.profile_db('K_r0'), 2)


def test_run_length_pools_are_refused():
    """a context that returns run-length text (sd_sw_set_cigar_pool) cannot serve the stage: refused, nothing copied as letters"""
    api, host, ctx, t_res, t_off, _ = device()
    q_let, q_off, edge_off, edge_t, edge_keys = layout(all_entries()[:2])
    ctx.set_cigar_pool(True)
    try:
        with pytest.raises(api.SdError, match=r'\(-5\)'):   # SD_EUNSUPPORTED
            api.r2p_realign(ctx, host, q_let, q_off, edge_off, edge_t, t_res, t_off)
    finally:
        ctx.set_cigar_pool(False)
    check(api.r2p_realign(ctx, host, q_let, q_off, edge_off, edge_t, t_res, t_off), edge_keys)


@pytest.mark.parametrize('flags,words', [(['--gap-open', '10'], '--gap-open 11'), (['--gap-extend', '2'], '--gap-open 11'),
                                         (['--comp-bias-corr-scale', '0.5'], '--comp-bias-corr-scale 1')])
def test_matcher_parameters_the_stage_lacks_are_refused(tmp_path, flags, words):
    """the reference builds the realigning Matcher from these flags; on rows to realign other values are refused, not ignored"""
    t, q, r = cdbgold.write_inputs(tmp_path)
    p = sdgpu('result2profile', q, t, r, tmp_path / 'profile', *flags, check=False)
    assert p.returncode != 0 and words in p.stderr and 'without a backtrace' in p.stderr


def test_rows_without_a_backtrace_need_the_device(tmp_path):
    t, q, r = cdbgold.write_inputs(tmp_path)
    p = sdgpu('result2profile', q, t, r, tmp_path / 'profile', '--profile-weights-host', 1, check=False)
    assert p.returncode != 0 and '--profile-weights-host 1' in p.stderr and 'without a backtrace' in p.stderr
