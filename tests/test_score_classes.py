"""CPU: the constructed score-class pairs (tests/scgen.py) against the rows that the REAL reference produced for them in
alignment modes 0, 1 and 2 (tests/golden/score_classes.npz, tools/make_golden_score_classes.py): the oracle equals every
row, every pair has the shape it was built for, and the restated class table puts the tasks that follow from the
reference's rows into every one of the 63 score kernels that the SCORE_CLASSES table of sd_sw.hip instantiates, and
the library's table (sd_selftest_score_class) equals the restatement for every row count.
tests/test_gpu_sw_score_classes.py runs the same pairs through the kernels."""
from collections import Counter

import numpy as np
import pytest

import scgen

CMP = ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'btLen')


@pytest.fixture(scope='module')
def gold():
    return scgen.golden()


@pytest.fixture(scope='module')
def built():
    return scgen.build()


@pytest.fixture(scope='module')
def rows(gold):
    return scgen.Rows(gold)


def test_generator_reproduces_the_golden_letters(gold, built):
    seqs, pairs = built
    assert 200 <= len(pairs) <= 400 and max(len(s) for s in seqs) == scgen.WRL_LEN
    assert sorted(len(s) for s in seqs)[-4] <= 2300      # (only the three sequences of the wideRowLimit switch are longer)
    assert scgen.digest(seqs) == str(gold['digest']) and len(seqs) == int(gold['n_seqs'])
    assert [p['name'] for p in pairs] == [str(s) for s in gold['name']] and len(set(p['name'] for p in pairs)) == len(pairs)
    assert [p['kind'] for p in pairs] == [str(s) for s in gold['kind']]
    assert [p['q'] for p in pairs] == list(gold['q']) and [p['t'] for p in pairs] == list(gold['t'])
    assert [len(seqs[p['q']]) for p in pairs] == list(gold['qlen']) and [len(seqs[p['t']]) for p in pairs] == list(gold['tlen'])
    # the target lengths below, at and above the lane counts, and one beyond 1024
    assert set((1, 5, 31, 32, 33, 63, 64, 65)) <= set(int(v) for v in gold['tlen']) and sum(1024 < v <= 2300 for v in gold['tlen']) >= 5


def test_oracle_equals_every_golden_row(oracle, host, gold, built):
    seqs, pairs = built
    db = int(gold['db_residues'])
    num = [oracle.map_sequence(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    sw_bias, _, _ = host.comp_bias(np.concatenate(num), off)
    mat, _, _ = host.matrix(0)
    mat = np.array([mat[i] for i in range(441)], np.int32)
    # the largest composition bias any residue reaches is 3 (wrl_bias3 has it), so int16 cells are safe up to 2340 rows
    assert int(sw_bias.max()) == 3 and int(gold['wide_row_limit']) == 32767 // (int(mat.max()) + 3) == 2340
    twins = {int(x): k for k, x in enumerate(gold['p_twin'])}
    assert [pairs[x]['name'] for x in twins] == list(scgen.PROFILE_TWINS)
    for x, p in enumerate(pairs):
        q, t = p['q'], p['t']
        bias = 4 + abs(min(0, int(sw_bias[int(off[q]):int(off[q + 1])].min())))
        assert bias == int(gold['qbias'][x])
        todo = [('', x, lambda **kw: oracle.sw_align(num[q], num[t], db, **kw))]
        if x in twins:
            prof = host.map_profiles(scgen.profile_record(num[q], mat, 1000 + x), np.array([0, 25 * len(num[q])], np.uint64))
            assert int(gold['p_qbias'][twins[x]]) == -int(prof['aln'][:, :20].min())
            assert int(gold['p_wide_row_limit']) <= 32767 // int(prof['aln'].max())
            todo.append(('p_', twins[x], lambda **kw: oracle.sw_align_profile(prof['letters'], prof['aln'], num[t], db, **kw)))
        for pre, k, align in todo:
            bts = str(gold[pre + 'bt']).split('\n')
            for mode in scgen.MODES:
                o = align(sw_mode=mode)
                r = dict(zip(scgen.FIELDS, (int(v) for v in gold[pre + 'res'][mode][k])))
                assert tuple(o[f] for f in CMP) == tuple(r[f] for f in CMP), (pre, p['name'], mode, o, r)
                assert o['evalue'] == float(gold[pre + 'evalue'][mode][k]), (pre, p['name'], mode)
                assert (o['flags'] & 1) == int(gold[pre + 'word'][k]), (pre, p['name'], mode)
                if mode == 2:
                    assert o['backtrace'] == bts[k] and (o['btLen'] == 0 or o['identical'] == r['identical']), (pre, p['name'])
            o = align(sw_mode=2, cov_thr=0.0)
            assert o['backtrace'] == str(gold[pre + 'bt_nocov']).split('\n')[k] and o['qStart'] == int(gold[pre + 'start_nocov'][k]), (pre, p['name'])


def test_pairs_have_the_shape_they_were_built_for(gold, built, rows):
    """from the reference's rows alone: saturation (the reference reruns a pair whose byte score reaches 255 - bias, and then
    reports the word kernel's score), qEnd + 1, the gap runs of the backtrace, the gates"""
    seqs, pairs = built
    res, ev = gold['res'], gold['evalue']
    n_evalue_gate = 0
    for x, p in enumerate(pairs):
        r0, r1, r2 = (dict(zip(scgen.FIELDS, (int(v) for v in res[m][x]))) for m in scgen.MODES)
        assert r0['score'] == r1['score'] == r2['score'] and r0['qEnd'] == r1['qEnd'] == r2['qEnd'] and r0['tEnd'] == r2['tEnd'], p['name']
        assert (r0['qStart'], r0['tStart'], r0['btLen'], r1['btLen']) == (-1, -1, 0, 0) and (r1['qStart'], r1['tStart']) == (r2['qStart'], r2['tStart'])
        sat = r2['score'] + int(gold['qbias'][x]) >= 255
        assert sat == bool(gold['word'][x])
        if p['sat'] is not None:
            assert sat == p['sat'], (p['name'], r2['score'])
            if p['kind'] == 'edge':      # 255 is the first byte score + bias that saturates, 254 the last that does not
                assert r2['score'] + int(gold['qbias'][x]) == int(p['name'][5:])
            else:                        # (and no other pair sits there by accident)
                assert r2['score'] + int(gold['qbias'][x]) not in (254, 255, 256)
        if p['rows'] is not None:
            assert r2['qEnd'] + 1 == p['rows'], (p['name'], r2)
        gaps = scgen.gap_runs(rows.bt_nocov[x], int(rows.start_nocov[x]))
        if p['igap']:
            _, g, lanes = p['igap']
            n = len(seqs[p['q']])
            seg = (n + lanes - 1) // lanes
            assert g == 2 * seg + 1
            hit = [(row, k) for a, row, k in gaps if a == 'I' and k >= g and row // seg + 2 <= (row + k - 1) // seg]
            assert hit, (p['name'], gaps)
            if p['kind'] == 'lastseg':    # the run's last row lies in the last used segment
                assert any((row + k - 1) // seg == (n - 1) // seg for row, k in hit), (p['name'], gaps, seg)
            if p['kind'] in ('hom', 'lastseg') and p['sat']:   # a full-length pair: the same path in the gated mode-2 row
                assert rows.bt[x] == rows.bt_nocov[x] and r2['btLen'] > 0
        if p['dgap']:
            assert any(a == 'D' and k >= 40 for a, _, k in gaps), (p['name'], gaps)
        if p['gate'] == 'evalue' or p['kind'] == 'unrel':
            stopped = ev[1][x] > 10.0
            assert stopped == (r1['qStart'] == -1) or r2['score'] == 0, p['name']
            assert stopped or p['gate'] is None, p['name']
            n_evalue_gate += stopped
        if p['gate'] == 'coverage':
            assert ev[1][x] <= 10.0 and (r2['qEnd'] + 1) / len(seqs[p['q']]) < 0.8 and r1['qStart'] == r2['qStart'] == -1, p['name']
    assert n_evalue_gate >= 60
    by = {p['name']: x for x, p in enumerate(pairs)}
    assert bool(gold['word'][by['cov_hom']]) and not gold['word'][by['cov_core']]
    # every forward class has a pair whose final result comes from the narrow kernel with a run through two lanes (coregap,
    # lastseg) and a saturating one with such a run and 41 target residues against a gap (hom)
    for kind, want_sat in (('coregap', False), ('hom', True)):
        seen = set(scgen.scope('fwd', len(seqs[p['q']]), True, rows.wrl) for p in pairs if p['kind'] == kind and p['igap'] and p['sat'] == want_sat)
        assert seen == set(scgen.scope('fwd', n, True, rows.wrl) for n in scgen.LENGTHS if n >= 77), kind
    assert set(p['name'][8:] for p in pairs if p['kind'] == 'lastseg') == set(k[0] for k in scgen.LASTSEG)
    # start positions on both sides of the limits of the unshared table, narrow and wide, in queries with an unrelated tail
    for n in scgen.TAIL_ROWS:
        for kind, word in (('core', False), ('hom', True)):
            x = by['tail_%s_%d' % (kind, n)]
            assert int(res[1][x][2]) + 1 == n and bool(gold['word'][x]) == word and int(res[1][x][1]) >= 0
            assert int(gold['qlen'][x]) == n + n // 8


def test_row_ties_of_the_periodic_query(oracle, host, gold, built):
    """tie_rows_*: a plain recurrence (Gotoh, gap open 11, extend 1, matrix + composition bias) has its maximum in the last column
    only, in every seventh row; the reference reports the first of them, and the second lies in the same 12-row lane of the wide
    kernel (w_rt12x32) for the saturating pair, in the next lane of the aligned kernel (a_seg12) for the other"""
    seqs, pairs = built
    mat, _, _ = host.matrix(0)
    m = np.array([mat[i] for i in range(441)], np.int64).reshape(21, 21)
    by = {p['name']: x for x, p in enumerate(pairs)}
    for name, rows_want, same_lane in (('tie_rows_w', (85, 92), True), ('tie_rows_n', (43, 50), False)):
        p = pairs[by[name]]
        q, t = oracle.map_sequence(seqs[p['q']]), oracle.map_sequence(seqs[p['t']])
        bias = host.comp_bias(q, np.array([0, len(q)], np.uint64))[0].astype(np.int64)
        prev_h, best = np.zeros(len(q) + 1, np.int64), {}
        e = np.zeros(len(q) + 1, np.int64)
        for j in range(len(t)):
            h = np.zeros(len(q) + 1, np.int64)
            e = np.maximum(np.maximum(e - 1, prev_h - 11), 0)
            f = 0
            for i in range(1, len(q) + 1):
                f = max(f - 1, h[i - 1] - 11, 0)
                h[i] = max(0, prev_h[i - 1] + m[t[j], q[i - 1]] + bias[i - 1], e[i], f)
            best[j] = (int(h.max()), [int(i) - 1 for i in np.flatnonzero(h == h.max())])
            prev_h = h
        top = max(v for v, _ in best.values())
        assert [j for j in best if best[j][0] == top] == [len(t) - 1] and tuple(best[len(t) - 1][1][:2]) == rows_want, (name, best[len(t) - 1])
        r = gold['res'][0][by[name]]
        assert (int(r[0]), int(r[2]), int(r[4])) == (top, rows_want[0], len(t) - 1)
        assert (rows_want[0] // 12 == rows_want[1] // 12) == same_lane and scgen.scope('fwd', len(q), True, 2340) == 'sw_score_pk.a_seg12'


def test_reach_every_instantiation(gold, rows):
    """the calls of the GPU tests (grouped: modes 0, 1, 2 on the packed kernels and mode 1 on the int32 kernel, odd and even; the
    query set of 2^17 sequences: modes 0 and 1) put tasks into all 63 instantiations, each with at least three tasks, two of a
    positive score, an odd count in one grouped call and an even one in another"""
    tasks, positive, parity, seen_scopes = Counter(), Counter(), {}, set()
    configs = [(m, True, True, True) for m in scgen.MODES] + [(1, True, False, True), (0, False, True, False), (1, False, True, False)]
    for mode, shared, packed, grouped in configs:
        per_pair = [rows.tasks(x, mode, shared, packed) for x in range(rows.n)]
        for x, ts in enumerate(per_pair):
            for p, c, s, inst in ts:
                tasks[inst] += 1
                positive[inst] += int(rows.res[mode][x][0]) > 0
                seen_scopes.add(s)
        if grouped:
            for key, members in rows.groups(mode, shared, packed).items():
                for odd in (True, False):
                    idx = scgen.padded(members, odd)
                    assert len(idx) % 2 == odd and (not odd or len(idx) >= 3)
                    for p, c, s in key:
                        parity.setdefault(scgen.instantiation(s, shared and p < 2), set()).add(len(idx) % 2)
    want = scgen.instantiations()
    assert set(tasks) == set(want), (set(want) - set(tasks), set(tasks) - set(want))
    for inst in want:
        assert tasks[inst] >= 3 and positive[inst] >= 2, (inst, tasks[inst], positive[inst])
        assert parity[inst] == {0, 1}, inst
    # the full list of scopes, shared and unshared
    assert seen_scopes == set(['sw_score_pk.a_seg%d' % rt for rt in range(5, 25)] + ['sw_score_pk.' + k for k in scgen.PK_NAMES[:1] + scgen.PK_NAMES[8:]] +
                              ['sw_score_pk.w_' + k for k in scgen.PK_NAMES] + ['sw_score.' + k for k in scgen.I32_NAMES])
    # the wideRowLimit switch: both pairs saturate, the square one leaves the packed kernels, the flat one stays
    by = {str(s): x for x, s in enumerate(gold['name'])}
    sq, fl = rows.tasks(by['wrl_square'], 1), rows.tasks(by['wrl_flat'], 1)
    assert [s for _, _, s, _ in sq] == ['sw_score_pk.rt8x64sN', 'sw_score.rt32', 'sw_score.rt32']
    assert [s for _, _, s, _ in fl] == ['sw_score_pk.rt8x64sN', 'sw_score_pk.w_rt8x64sN', 'sw_score_pk.w_rt8x64sN']
    assert min(int(gold['qlen'][by['wrl_square']]), int(gold['tlen'][by['wrl_square']])) > rows.wrl >= 2300
    # runs of one to five tasks of one query in a forward class, one and two in a rerun class (all pairs in one call)
    fwd, rerun = Counter(int(q) for q in gold['q']), Counter(int(q) for q, w in zip(gold['q'], gold['word']) if w)
    assert set(fwd.values()) >= {1, 2, 3, 4, 5} and set(rerun.values()) >= {1, 2}
    # a pair of tasks with the longer target first, second, and with equal ones, as the pairing sort leaves them
    order = scgen.shuffled(rows.n)
    key = lambda x: (rows.tasks(x, 0)[0][1], int(gold['q'][x]), (1023 - min(int(gold['tlen'][x]) >> 4, 1023)) >> 1)   # (k_pair_keys)
    srt = sorted(order, key=key)
    rel = set()
    pos = 0
    while pos < len(srt):
        run = [x for x in srt[pos:] if key(x)[:2] == key(srt[pos])[:2]][:fwd[int(gold['q'][srt[pos]])]]
        for a, b in zip(run[0::2], run[1::2]):
            rel.add(int(np.sign(int(gold['tlen'][a]) - int(gold['tlen'][b]))))
        pos += len(run)
    assert rel == {-1, 0, 1}
    # the profile twins run in the scopes of their plain twins, one pair of each kernel family
    prow = scgen.Rows(gold, 'p_')
    fam = set()
    for k, x in enumerate(gold['p_twin']):
        for mode in scgen.MODES:
            assert prow.tasks(k, mode) == rows.tasks(int(x), mode), (gold['name'][x], mode)
        fam |= set(t[3] for t in prow.tasks(k, 2))
    assert fam >= {('a_seg10', True), ('a_seg10', False), ('rt4x32', True), ('rt8x64', False), ('rt8x64multi', True), ('rt8x64multi', False),
                   ('w_rt10x32', True), ('w_rt8x64', False), ('w_rt8x64multi', True)}


def test_library_table_equals_the_restatement(host):
    """sd_selftest_score_class reads the table and the index function that the gate kernels and devRunScore use: for every pass,
    both pairings, the packed and the int32 kernels, every row count up to 2 600 and one far beyond, the column counts around
    wideRowLimit and around 65 535, the library's (class, scope) is klass()'s"""
    checked = 0
    for W in (258, 2340):
        for pass_, word in (('fwd', False), ('word', False), ('start', False), ('start', True)):
            wide = pass_ == 'word' or word
            for packed in (True, False):
                kernel = 2 if not packed else 1 if wide else 0
                for shared in (True, False):
                    lib_shared = shared and pass_ != 'start'      # (start-position tasks are never paired: alignBatchImpl)
                    for tl in (1, W, W + 1, 65535, 65536):
                        for n in list(range(1, 2601)) + [60000]:
                            want = scgen.klass(pass_, n, shared, W, packed=packed, word=word, tl=tl)
                            got = host.score_class(kernel, n, tl, lib_shared, W)
                            if got != want:
                                raise AssertionError((pass_, word, packed, shared, W, tl, n, got, want))
                            checked += 1
    assert checked == 2 * 4 * 2 * 2 * 5 * 2601


def test_scope_restates_the_class_limits():
    s = lambda *a, **k: scgen.scope(*a, **k).split('.')[1]
    W = 2340
    assert s('fwd', 128, True, W) == 'rt4x32' and s('fwd', 129, True, W) == 'a_seg5' and s('fwd', 1, False, W) == 'rt4x32'
    assert [s('fwd', n, True, W) for n in (160, 161, 384, 385, 768)] == ['a_seg5', 'a_seg6', 'a_seg12', 'a_seg13', 'a_seg24']
    assert [s('fwd', n, False, W) for n in (129, 384, 385, 512, 513, 640, 641, 768)] == \
           ['a_seg5', 'a_seg12', 'rt8x64', 'rt8x64', 'rt10x64', 'rt10x64', 'rt12x64', 'rt12x64']
    assert [s('start', n, True, W) for n in (128, 129, 384, 385, 769)] == ['rt4x32', 'a_seg5', 'a_seg12', 'rt8x64', 'rt8x64s2']
    for shared in (True, False):
        assert [s('fwd', n, shared, W) for n in (769, 1024, 1025, 1536, 1537, 2048, 2049, 60000)] == \
               ['rt8x64s2', 'rt8x64s2', 'rt8x64s3', 'rt8x64s3', 'rt8x64sN', 'rt8x64sN', 'rt8x64sN', 'rt8x64sN']
        assert [s('word', n, shared, W) for n in (1, 128, 129, 192, 193, 224, 225, 256, 257, 288, 289, 320, 321, 352, 353, 384, 385)] == \
               ['w_rt4x32', 'w_rt4x32', 'w_rt6x32', 'w_rt6x32', 'w_rt7x32', 'w_rt7x32', 'w_rt8x32', 'w_rt8x32', 'w_rt9x32', 'w_rt9x32',
                'w_rt10x32', 'w_rt10x32', 'w_rt11x32', 'w_rt11x32', 'w_rt12x32', 'w_rt12x32', 'w_rt8x64']
        assert [s('word', n, shared, W) for n in (512, 513, 640, 641, 768, 769, 1024, 1025, 1536, 1537)] == \
               ['w_rt8x64', 'w_rt10x64', 'w_rt10x64', 'w_rt12x64', 'w_rt12x64', 'w_rt8x64s2', 'w_rt8x64s2', 'w_rt8x64s3', 'w_rt8x64s3', 'w_rt8x64sN']
    assert s('start', 300, False, W, word=True) == 'w_rt10x32' and s('start', 300, False, W) == 'a_seg10'
    # beyond wideRowLimit in both dimensions the word structure runs on the int32 kernel; the narrow form never does
    assert s('word', 3000, True, W, tl=W) == 'w_rt8x64sN' and s('word', W, True, W, tl=3000) == 'w_rt8x64sN'
    assert s('word', W + 1, True, W, tl=W + 1) == 'rt32' and s('start', W + 1, False, W, word=True, tl=W + 1) == 'rt32'
    assert s('start', W + 1, False, W, tl=W + 1) == 'rt8x64sN' and s('fwd', 3000, True, W) == 'rt8x64sN'
    assert s('word', 300, True, 258, tl=259) == 'rt16' and s('word', 300, True, 258, tl=258) == 'w_rt10x32'
    assert [s('fwd', n, True, W, packed=False) for n in (128, 129, 256, 257, 512, 513)] == ['rt4', 'rt8', 'rt8', 'rt16', 'rt16', 'rt32']
    assert [scgen.klass('fwd', n, False, W) for n in (416, 417)] == [(9, 'sw_score_pk.rt8x64'), (10, 'sw_score_pk.rt8x64')]   # two classes, one scope
    assert scgen.klass('word', 385, True, W)[0] == 32 and scgen.klass('fwd', 3000, True, W)[0] == 23 and scgen.klass('fwd', 9, True, W, packed=False)[0] == 38
    assert scgen.scope('fwd', 300, True, W) == 'sw_score_pk.a_seg10' and scgen.scope('fwd', 300, True, W, packed=False) == 'sw_score.rt16'
    assert scgen.instantiation('sw_score_pk.rt8x64s3', True) == ('rt8x64multi', True) == scgen.instantiation('sw_score_pk.rt8x64sN', True)
    assert scgen.instantiation('sw_score_pk.w_rt8x64s2', False) == ('w_rt8x64multi', False) and scgen.instantiation('sw_score.rt8', True) == ('i32_rt8', False)
    assert scgen.gap_runs('MMIIIMMDDM', 10) == [('I', 12, 3), ('D', 17, 2)]
