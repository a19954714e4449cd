"""Alternative alignments on the GPU (sd_sw_alt.hip, sd_sw_align_alt_batch, `align --alt-ali`, `search --alt-ali`) against
tests/golden/altali_vectors.npz (the reference's matcher driven through Alignment::computeAlternativeAlignment's loop) and the
restatement of tests/altali_ref.py around the scalar oracle.  Every comparison is exact."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import altali_ref as ar
from dbutil import sdgpu, write_db, read_db, example_fasta, entries_by_first_column, flat_lines_from_gz, SDGPU, GOLD
from spacedust_amd._lib import ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return ar.load()


@pytest.fixture(scope='module')
def sets(gold, host, gpu):
    """the golden sequences as one device set with the Smith-Waterman composition bias (queries and targets alike)"""
    res, off = host.map_sequences([s.decode() for s in gold['seqs']])
    bias = host.comp_bias(res, off)[0]
    return dict(res=res, off=off, q=gpu.seqset(res, off, bias), t=gpu.seqset(res, off))


def run_group(gpu, host, gold, sets, pi, idx, cigar):
    """the cases idx (all with parameter set pi) in ONE call -> per case the list of records as dicts"""
    p = gold['params'][pi]
    par = gpu.sw_params(host.matrix(0)[0], gold['db_residues'], sw_mode=p['sw_mode'], eval_thr=p['eval_thr'], cov_mode=p['cov_mode'],
                        cov_thr=p['cov_thr'])
    cases = [gold['cases'][i] for i in idx]
    n_max = max(c[3] for c in cases)
    out = []
    # the call takes one N: cases are grouped by N as well
    for n in sorted({c[3] for c in cases}):
        sel = [x for x, c in enumerate(cases) if c[3] == n]
        res, cnt, pool = gpu.sw_align_alt(par, sets['q'], sets['t'], [cases[x][0] for x in sel], [cases[x][1] for x in sel],
                                          [gold['seeds'][idx[x]][0] for x in sel], [gold['seeds'][idx[x]][1] for x in sel], n,
                                          identity=[cases[x][4] for x in sel], seq_id_thr=p['seq_id_thr'], aln_len_thr=p['aln_len_thr'],
                                          seq_id_mode=p['seq_id_mode'])
        pool = pool.tobytes()
        for y, x in enumerate(sel):
            rows = []
            for r in res[y, :cnt[y]]:
                d = {f: int(r[f]) for f in ar.REC_FIELDS}
                d['evalue'] = float(r['evalue'])
                d['word'] = int(r['flags']) & 1
                if p['sw_mode'] == 2:
                    n_txt = int(r['flags']) >> 8 if cigar else d['btLen']
                    d['backtrace'] = pool[int(r['btOffset']):int(r['btOffset']) + n_txt].decode()
                else:
                    d['backtrace'] = ''
                    d['identical'] = 0
                rows.append(d)
            out.append((idx[x], rows))
    assert n_max <= 10
    return dict(out)


def compress(bt):
    """Matcher::compressAlignment: run-length text, "0M" first when the backtrace does not begin with a match"""
    if not bt:
        return ''
    out = '' if bt[0] == 'M' else '0M'
    return out + ''.join('%d%s' % (len(m.group(0)), m.group(0)[0]) for m in re.finditer(r'M+|I+|D+', bt))


@pytest.mark.parametrize('cigar', [False, True])
def test_c_abi_equals_every_golden_case(gold, sets, host, gpu, cigar):
    g = gold
    gpu.set_cigar_pool(cigar)
    try:
        got = {}
        for pi in range(len(g['params'])):
            idx = [i for i, c in enumerate(g['cases']) if c[2] == pi]
            got.update(run_group(gpu, host, g, sets, pi, idx, cigar))
    finally:
        gpu.set_cigar_pool(False)
    assert len(got) == len(g['cases'])
    bad, word = [], 0
    for i, want in enumerate(g['want']):
        rows = got[i]
        sw2 = g['params'][g['cases'][i][2]]['sw_mode'] == 2
        ok = len(rows) == len(want)
        for a, b in zip(rows, want):
            bt = b['backtrace'] if sw2 else ''
            ok = ok and all(a[f] == b[f] for f in ar.REC_FIELDS) and a['evalue'] == b['evalue'] and a['backtrace'] == (compress(bt) if cigar else bt)
            word += a['word']
        if not ok:
            bad.append((i, g['cls'][i], len(rows), len(want)))
    print('cigar pool %s: %d cases, %d alternatives (%d on the word kernel), %d mismatches' % (cigar, len(got), sum(len(w) for w in g['want']), word, len(bad)))
    assert word >= 1   # a masked round that saturated the byte kernel
    assert not bad, bad[:8]


def test_five_thousand_seeds_in_several_groups_equal_the_restatement(gold, sets, host, gpu, oracle):
    """every golden case of one parameter set many times over, shuffled with random pairs that share no domain, in ONE call whose
    workspace budget holds about a fifth of the copies: several seed groups, each with dead and live seeds in every round"""
    g = gold
    pi = 0
    p = g['params'][pi]
    n = 3
    rng = np.random.default_rng(5)
    # (a case generated for N >= 3 has the same first three rounds; one that ended before its own N ends there for any N)
    base = [i for i, c in enumerate(g['cases']) if c[2] == pi and (c[3] >= n or len(g['want'][i]) < c[3])]
    lens = np.array([len(s) for s in g['seqs']])
    rand_pairs = [(int(a), int(b)) for a, b in rng.integers(0, len(g['seqs']), (120, 2)) if a // 2 != b // 2 and a != b]
    want_rand = []
    for a, b in rand_pairs:   # a seed on unrelated sequences: an interval in the middle of the target
        q, t = sets['res'][int(sets['off'][a]):int(sets['off'][a + 1])], sets['res'][int(sets['off'][b]):int(sets['off'][b + 1])]
        s0, s1 = int(lens[b]) // 3, int(lens[b]) // 2

        def align(num, q=q):
            r = oracle.sw_align(q, num, g['db_residues'], sw_mode=p['sw_mode'], eval_thr=p['eval_thr'], cov_mode=p['cov_mode'], cov_thr=p['cov_thr'])
            return r
        want_rand.append(((a, b, s0, s1), ar.alternatives(align, t, s0, s1, n, len(q), p)))
    seeds, want = [], []
    reps = (5000 - len(want_rand)) // len(base) + 1
    for _ in range(reps):
        for i in base:
            c = g['cases'][i]
            seeds.append((c[0], c[1], g['seeds'][i][0], g['seeds'][i][1], c[4]))
            want.append(g['want'][i][:n])
    for (a, b, s0, s1), w in want_rand:
        seeds.append((a, b, s0, s1, 0))
        want.append(w)
    order = rng.permutation(len(seeds))
    seeds, want = [seeds[i] for i in order], [want[i] for i in order]
    assert len(seeds) >= 5000
    copies = int(sum((lens[s[1]] + 3) // 4 * 4 for s in seeds))
    par = gpu.sw_params(host.matrix(0)[0], g['db_residues'], sw_mode=p['sw_mode'], eval_thr=p['eval_thr'], cov_mode=p['cov_mode'], cov_thr=p['cov_thr'])
    os.environ['SD_ALT_BUDGET'] = str(copies // 5)
    try:
        res, cnt, pool = gpu.sw_align_alt(par, sets['q'], sets['t'], [s[0] for s in seeds], [s[1] for s in seeds], [s[2] for s in seeds],
                                          [s[3] for s in seeds], n, identity=[s[4] for s in seeds])
    finally:
        del os.environ['SD_ALT_BUDGET']
    groups, seed_rounds, copied = gpu.sw_alt_stats()
    ws = dict(gpu.workspace_report(top=4096)[2])
    alt_ws = sum(v for k, v in ws.items() if k.startswith('alt.'))
    print('%d seeds, %d groups, %d alignments, %d bytes masked and copied; alt.* workspace %d bytes for a budget of %d'
          % (len(seeds), groups, seed_rounds, copied, alt_ws, copies // 5))
    assert groups >= 3
    # the budget covers a group's copies and per-seed state; the workspace allocator adds a quarter and 256 bytes per entry, and the
    # fifteen alt.* entries carry a few elements of padding and the scan's block sums (64 KiB holds all of that many times over)
    assert ws.get('alt.scratch', 0) > 0 and alt_ws <= (copies // 5) * 5 // 4 + (64 << 10)
    pool = pool.tobytes()
    bad = []
    for x, w in enumerate(want):
        ok = int(cnt[x]) == len(w)
        for r, b in zip(res[x, :cnt[x]], w):
            ok = ok and all(int(r[f]) == b[f] for f in ar.REC_FIELDS) and float(r['evalue']) == b['evalue'] and \
                pool[int(r['btOffset']):int(r['btOffset']) + int(r['btLen'])].decode() == b['backtrace']
        if not ok:
            bad.append((x, seeds[x], int(cnt[x]), len(w)))
    assert not bad, bad[:8]
    assert sum(len(w) for w in want) > 1000 and sum(1 for w in want if not w) > 100


def test_profile_targets_and_score_only_mode_are_refused(gold, sets, host, gpu):
    from spacedust_amd.api import SdError
    par = gpu.sw_params(host.matrix(0)[0], 10 ** 6, sw_mode=0)
    with pytest.raises(SdError, match='swMode'):
        gpu.sw_align_alt(par, sets['q'], sets['t'], [0], [1], [0], [5], 2)
    par = gpu.sw_params(host.matrix(0)[0], 10 ** 6, sw_mode=2)
    prof = gpu.profileset(sets['res'], sets['off'], np.zeros((len(sets['res']), 21), np.int8))
    with pytest.raises(SdError, match=r'\(-5\)'):
        gpu.sw_align_alt(par, sets['q'], prof, [0], [1], [0], [5], 2)
    with pytest.raises(SdError, match=r'\(-3\)'):
        gpu.sw_align_alt(par, sets['q'], sets['t'], [0], [1], [0], [10 ** 6], 2)


def synthetic_profiles(host, seqs_num, rng):
    """profile queries derived from sequences: the matrix row of every residue, scaled, with noise (as test_gpu_profile.py makes them)"""
    m = np.array([host.matrix(0)[0][i] for i in range(441)], np.int32).reshape(21, 21)
    recs, boff = [], [0]
    for s in seqs_num:
        rec = np.zeros((len(s), 25), np.uint8)
        scale = int(rng.integers(2, 5))
        for i, a in enumerate(s):
            row = m[min(int(a), 19), :20] * scale + rng.integers(-3, 4, 20)
            rec[i, :20] = np.clip(row, -128, 127).astype(np.int8).view(np.uint8)
            rec[i, 20] = a
            rec[i, 21] = int(np.argmax(row))
        recs.append(rec.tobytes())
        boff.append(boff[-1] + len(recs[-1]))
    return host.map_profiles(b''.join(recs), np.array(boff, np.uint64))


def test_profile_queries_equal_the_restatement_around_the_profile_oracle(gold, sets, host, gpu, oracle):
    """profile query sets through sd_sw_align_alt_batch (masking is target-side only): the golden cases of one parameter set with
    a profile made from each query, against the restatement around the oracle's profile Smith-Waterman"""
    g = gold
    pi = next(i for i, p in enumerate(g['params']) if p['sw_mode'] == 2)
    p = g['params'][pi]
    idx = [i for i, c in enumerate(g['cases']) if c[2] == pi and not c[4] and c[3] >= 2][:40]
    assert len(idx) >= 20
    n = 3
    qnum = [sets['res'][int(sets['off'][g['cases'][i][0]]):int(sets['off'][g['cases'][i][0] + 1])] for i in idx]
    prof = synthetic_profiles(host, qnum, np.random.default_rng(17))
    po = prof['offsets']
    qs = gpu.profileset(prof['letters'], po, prof['aln'])
    par = gpu.sw_params(host.matrix(0)[0], g['db_residues'], sw_mode=2, eval_thr=p['eval_thr'], cov_mode=p['cov_mode'], cov_thr=p['cov_thr'])
    res, cnt, pool = gpu.sw_align_alt(par, qs, sets['t'], list(range(len(idx))), [g['cases'][i][1] for i in idx],
                                      [g['seeds'][i][0] for i in idx], [g['seeds'][i][1] for i in idx], n,
                                      seq_id_thr=p['seq_id_thr'], aln_len_thr=p['aln_len_thr'], seq_id_mode=p['seq_id_mode'])
    pool = pool.tobytes()
    total = 0
    for x, i in enumerate(idx):
        ti = g['cases'][i][1]
        t = sets['res'][int(sets['off'][ti]):int(sets['off'][ti + 1])]
        a, b = int(po[x]), int(po[x + 1])

        def align(num, a=a, b=b):
            return oracle.sw_align_profile(prof['letters'][a:b], prof['aln'][a:b], num, g['db_residues'], sw_mode=2, eval_thr=p['eval_thr'],
                                           cov_mode=p['cov_mode'], cov_thr=p['cov_thr'])
        want = ar.alternatives(align, t, g['seeds'][i][0], g['seeds'][i][1], n, b - a, p)
        total += len(want)
        assert int(cnt[x]) == len(want), (x, i, int(cnt[x]), len(want))
        for r, w in zip(res[x, :cnt[x]], want):
            assert all(int(r[f]) == w[f] for f in ar.REC_FIELDS) and float(r['evalue']) == w['evalue'], (x, i, r, w)
            assert pool[int(r['btOffset']):int(r['btOffset']) + int(r['btLen'])].decode() == w['backtrace'], (x, i)
    print('%d profile seeds, %d alternatives' % (len(idx), total))
    assert total >= 10


# ---- the module ------------------------------------------------------------------------------------------------------------------

ALN_COMMON = '-a 1 -e 0.001 --threads 8'.split()
# the `align` commands of the module tests; tests/golden/altali_parent_aln0.json holds, per name, what the binary of the commit
# before --alt-ali existed wrote for the command with `--alt-ali 0` (tools/record_altali_parent.py)
MODULE_CASES = {
    'cov': ['-c', '0.5', '--cov-mode', '2'],
    'nocov': ['--min-aln-len', '30'],
    'cov_realign': ['-c', '0.5', '--cov-mode', '2', '--realign', '1'],
    'nocov_realign': ['--min-aln-len', '30', '--realign', '1'],
}
MODULE_CRIT = {'cov': dict(cov_thr=0.5, cov_mode=2, aln_len_thr=0), 'nocov': dict(cov_thr=0.0, cov_mode=0, aln_len_thr=30)}
FLT_MAX = float(np.finfo(np.float32).max)


def genome_work(tmp):
    """the example genomes as a set DB and their prefilter DB (the fixture the reference classes wrote) cut to the first 200 queries"""
    fa = example_fasta(tmp)
    g = tmp / 'genome'
    sdgpu('createsetdb', fa[0], fa[1], g, tmp / 'tmp', '-v', '0')
    pref = entries_by_first_column(flat_lines_from_gz('config1_pref.tsv.gz'), 5898)[:200]
    write_db(str(tmp / 'pref200'), pref, 7)
    return g, tmp / 'pref200'


def db_md5(path):
    return [hashlib.md5(open(str(path) + ext, 'rb').read()).hexdigest() for ext in ('', '.index')]


@pytest.fixture(scope='module')
def work(tmp_path_factory, host):
    tmp = tmp_path_factory.mktemp('altali')
    g, pref = genome_work(tmp)
    seqs = {k: v.decode().strip() for k, v in read_db(str(g)).items()}
    keys = sorted(seqs)
    res, off = host.map_sequences([seqs[k] for k in keys])
    num = {k: res[int(off[i]):int(off[i + 1])] for i, k in enumerate(keys)}
    return dict(tmp=tmp, g=g, pref=pref, num=num, total=int(off[-1]))


def rows_of(db):
    out = {}
    for k, v in read_db(str(db)).items():
        out[k] = [l.split('\t') for l in v.decode().splitlines()]
    return out


def seq_id_text(seq_id):
    """Util::fastSeqIdToBuffer as Matcher::resultToBuffer uses it (M/src/commons/Util.cpp:222-251, Matcher.cpp:286-287): three
    decimals by truncation in float arithmetic; an identity of one is left as "1.00" """
    seq_id = np.float32(seq_id)
    if seq_id == np.float32(1.0):
        return '1.00'
    return '0.' + ('0' if seq_id < 0.10 else '') + ('0' if seq_id < 0.01 else '') + str(int(seq_id * np.float32(1000)))


def tie_classes(rows):
    """rows in order, with every run of equal (E-value text, bit score, target) as a sorted block: the reference's sort leaves
    the order inside such a run open"""
    out, run = [], []
    for r in rows:
        key = (r[3], r[1], r[0])
        if run and key != run[0][0]:
            out.extend(sorted(x[1] for x in run))
            run = []
        run.append((key, tuple(r)))
    out.extend(sorted(x[1] for x in run))
    return out


def check_module(work, host, name, align_many_of, p):
    """`align --alt-ali 0` equals the parent binary's recorded output byte for byte, and every entry of `align --alt-ali 3` equals
    its rows extended by the restatement (align_many_of(query key list of the seeds) -> the batch aligner of alternatives_many)"""
    g, tmp = work['g'], work['tmp']
    par = ALN_COMMON + MODULE_CASES[name]
    sdgpu('align', g, g, work['pref'], tmp / (name + '0'), *par, '--alt-ali', '0')
    sdgpu('align', g, g, work['pref'], tmp / (name + '3'), *par, '--alt-ali', '3')
    primary, got = rows_of(tmp / (name + '0')), rows_of(tmp / (name + '3'))
    recorded = json.load(open(os.path.join(GOLD, 'altali_parent_aln0.json')))[name]
    n_rows = sum(len(r) for r in primary.values())
    print('%s: --alt-ali 0 wrote %d rows, md5 %s; the parent binary wrote %s' % (name, n_rows, db_md5(tmp / (name + '0')), recorded))
    assert [n_rows] + db_md5(tmp / (name + '0')) == recorded
    assert len(primary) == 200 and sorted(got) == sorted(primary)
    # the seeds: every row of a query whose target is not the query itself (same DB on both sides: an identity pair)
    seeds = [(k, x) for k in sorted(primary) for x, r in enumerate(primary[k]) if int(r[0]) != k]
    targets = [work['num'][int(primary[k][x][0])] for k, x in seeds]
    ivl = [(int(primary[k][x][7]), int(primary[k][x][8])) for k, x in seeds]
    qlens = [len(work['num'][k]) for k, _ in seeds]
    alts = ar.alternatives_many(align_many_of([k for k, _ in seeds]), targets, ivl, 3, qlens, p)
    extra = {k: [] for k in primary}
    for (k, x), t, rows in zip(seeds, targets, alts):
        for a in rows:
            sid = seq_id_text(np.float32(a['identical']) / np.float32(a['btLen']))
            extra[k].append((primary[k][x][0], str(int(host.bitscore(a['score']) + 0.5)), sid, '%.3E' % a['evalue'], str(a['qStart']), str(a['qEnd']),
                             str(len(work['num'][k])), str(a['tStart']), str(a['tEnd']), str(len(t)), compress(a['backtrace'])))
    n_alt = sum(len(v) for v in extra.values())
    print('%s: %d queries, %d primary rows, %d seeds, %d alternative rows' % (name, len(primary), n_rows, len(seeds), n_alt))
    bad = []
    for k in sorted(primary):
        allrows = [tuple(r) for r in primary[k]] + extra[k]
        allrows.sort(key=lambda r: (float(r[3]), -int(r[1]), int(r[9]), int(r[0])))   # Matcher::compareHits
        if tie_classes(got[k]) != tie_classes(allrows):
            bad.append((k, len(got[k]), len(allrows)))
    assert not bad, bad[:8]
    assert n_alt > 0 and any(len(primary[k]) > 10 for k in primary) and len({r[0] for k in primary for r in primary[k]}) > 200


@pytest.mark.parametrize('name', ['cov', 'nocov'])
def test_align_module_on_the_example_genomes_equals_restatement_extended_from_the_primary_rows(work, host, oracle, name):
    crit = MODULE_CRIT[name]
    p = dict(sw_mode=2, eval_thr=float(np.float32(0.001)), seq_id_thr=0.0, seq_id_mode=0, **crit)

    def align_many_of(qkeys):
        def align_many(live, masked):
            return [oracle.sw_align(work['num'][qkeys[s]], m, work['total'], sw_mode=2, eval_thr=p['eval_thr'], cov_mode=p['cov_mode'],
                                    cov_thr=p['cov_thr']) for s, m in zip(live, masked)]
        return align_many
    check_module(work, host, name, align_many_of, p)


@pytest.mark.parametrize('name', ['cov_realign', 'nocov_realign'])
def test_align_module_with_realign_equals_restatement_around_the_realigner(work, host, gpu, name):
    """under --realign the alternatives come from the realigner (Alignment.cpp:433-435): the score-biased matrix with the query's
    composition bias against it, the coverage threshold of -c, no E-value gate, the realigner's alignment mode.  The restatement
    runs around sd_sw_align_batch (which this feature leaves as it was) with exactly those parameters."""
    crit = MODULE_CRIT[name.split('_')[0]]
    p = dict(sw_mode=2, eval_thr=FLT_MAX, seq_id_thr=0.0, seq_id_mode=0, **crit)
    par = gpu.sw_params(host.matrix(2)[0], work['total'], sw_mode=2, eval_thr=FLT_MAX, cov_mode=p['cov_mode'], cov_thr=p['cov_thr'])

    def align_many_of(qkeys):
        uq = sorted(set(qkeys))
        pos = {k: i for i, k in enumerate(uq)}
        qres = np.concatenate([work['num'][k] for k in uq])
        qoff = np.zeros(len(uq) + 1, np.uint64)
        np.cumsum([len(work['num'][k]) for k in uq], out=qoff[1:])
        bias = np.zeros(len(qres), np.int8)
        assert host.L.sd_host_sw_comp_bias(host.h, 2, ptr(qres), ptr(qoff), len(uq), ptr(bias)) == 0
        qs = gpu.seqset(qres, qoff, bias)

        def align_many(live, masked):
            toff = np.zeros(len(masked) + 1, np.uint64)
            np.cumsum([len(m) for m in masked], out=toff[1:])
            ts = gpu.seqset(np.concatenate(masked), toff)
            res, pool = gpu.sw_align(par, qs, ts, [pos[qkeys[s]] for s in live], list(range(len(live))))
            pool = pool.tobytes()
            out = []
            for r in res:
                d = {f: int(r[f]) for f in ar.REC_FIELDS}
                d['evalue'] = float(r['evalue'])
                d['backtrace'] = pool[int(r['btOffset']):int(r['btOffset']) + d['btLen']].decode() if d['btLen'] > 0 else ''
                out.append(d)
            return out
        return align_many
    check_module(work, host, name, align_many_of, p)


def test_search_alt_ali_equals_its_module_chain_and_refusals(tmp_path):
    fa = example_fasta(tmp_path)
    g = tmp_path / 'genome'
    sdgpu('createsetdb', fa[0], fa[1], g, tmp_path / 'tmp', '-v', '0')
    # the first 200 queries
    idx = open(str(g) + '.index').readlines()[:200]
    for ext in ('', '.dbtype', '.lookup', '.source', '_h', '_h.index', '_h.dbtype'):
        if os.path.exists(str(g) + ext):
            os.symlink(str(g) + ext, str(tmp_path / 'q200') + ext)
    open(str(tmp_path / 'q200') + '.index', 'w').writelines(idx)
    q = tmp_path / 'q200'
    sdgpu('search', q, g, tmp_path / 'fused', tmp_path / 'tmps', '--alt-ali', '2', '-a', '1', '-s', '5.7', '-e', '0.001', '--threads', '8')
    sdgpu('prefilter', q, g, tmp_path / 'pref', '-s', '5.7', '--max-seqs', '300', '--threads', '8')
    sdgpu('align', q, g, tmp_path / 'pref', tmp_path / 'chain', '--alt-ali', '2', '--alignment-mode', '2', '-a', '1', '-e', '0.001', '--threads', '8')
    sdgpu('align', q, g, tmp_path / 'pref', tmp_path / 'chain0', '--alignment-mode', '2', '-a', '1', '-e', '0.001', '--threads', '8')
    fused, chain, chain0 = read_db(str(tmp_path / 'fused')), read_db(str(tmp_path / 'chain')), read_db(str(tmp_path / 'chain0'))
    assert fused == chain and len(chain) == 200
    n2, n0 = sum(v.count(b'\n') for v in chain.values()), sum(v.count(b'\n') for v in chain0.values())
    print('200 queries: %d rows, %d with --alt-ali 2' % (n0, n2))
    assert n2 > n0 > 200

    def refused(*args):
        p = subprocess.run([SDGPU] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode != 0, args
        return p.stderr
    assert '--num-iterations' in refused('search', q, g, tmp_path / 'r1', tmp_path / 'tmpr', '--alt-ali', '2', '--num-iterations', '2')
    assert 'clustersearch --alt-ali' in refused('clustersearch', g, g, tmp_path / 'r1.tsv', tmp_path / 'tmpr', '--alt-ali', '2')
    assert '--alignment-mode 4' in refused('search', q, g, tmp_path / 'r1', tmp_path / 'tmpr', '--alt-ali', '2', '--alignment-mode', '4')
    assert not os.path.exists(tmp_path / 'r1') and not os.path.exists(tmp_path / 'r1.tsv')
