"""CPU: the constructed traceback pairs (tests/tbgen.py) against the rows that the REAL reference produced for them
(tests/golden/tb_classes.npz, tools/make_golden_tb_classes.py): the oracle equals every row, every pair has the shape it
was built for, and the band history that follows from the reference's record reaches the traceback class the pair is
meant for.  tests/test_gpu_sw_traceback.py runs the same pairs through the kernels."""
import numpy as np
import pytest

import tbgen

FIELDS = ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'identical', 'btLen')


@pytest.fixture(scope='module')
def gold():
    return tbgen.golden()


def test_generator_reproduces_the_golden_letters(gold):
    ps = tbgen.pairs()
    assert 60 <= len(ps) <= 85 and max(max(len(p['q']), len(p['t'])) for p in ps) <= 2000
    assert [p['name'] for p in ps] == [str(s) for s in gold['name']]
    assert [p['q'] for p in ps] == [str(s) for s in gold['q']] and [p['t'] for p in ps] == [str(s) for s in gold['t']]
    assert [p['kind'] for p in ps] == [str(s) for s in gold['kind']]


def test_oracle_equals_every_golden_row(oracle, gold):
    db = int(gold['db_residues'])
    for x in range(len(gold['name'])):
        o = oracle.sw_align(oracle.map_sequence(str(gold['q'][x])), oracle.map_sequence(str(gold['t'][x])), db, cov_thr=0.0)
        assert tuple(o[k] for k in FIELDS) == tuple(int(v) for v in gold['res'][x]), (gold['name'][x], o)
        assert o['backtrace'] == str(gold['bt'][x]), gold['name'][x]
        assert o['evalue'] == float(gold['evalue'][x]), gold['name'][x]


def test_pairs_have_the_shape_they_were_built_for(gold):
    """doubling pairs: one run of exactly g I and one of exactly g D, end to end; boundary pairs: a single run"""
    for p, r, bt in zip(tbgen.pairs(), gold['res'], gold['bt']):
        gaps = [(a, n) for a, n in tbgen.runs(str(bt)) if a != 'M']
        whole = (int(r[1]), int(r[3]), int(r[2]), int(r[4])) == (0, 0, len(p['q']) - 1, len(p['t']) - 1)
        if p['kind'] == 'doubling':
            assert whole and gaps == ([('I', p['gap']), ('D', p['gap'])] if p['gap'] else []), (p['name'], gaps)
        elif p['kind'] == 'skew':
            assert whole and gaps == [('I', p['gap'][0]), ('D', p['gap'][1])], (p['name'], gaps)
        elif p['kind'] in ('boundary', 'tcap'):
            assert whole and gaps == [('D' if len(p['t']) > len(p['q']) else 'I', p['gap'])], (p['name'], gaps)
        elif p['kind'] == 'rowcap':
            assert whole and gaps == ([('D', p['gap'])] if p['gap'] else []), (p['name'], gaps)
            assert int(r[2] - r[1] + 1) in [c + d for c in tbgen.NARROW_Q for d in (0, 1)]
        else:
            assert p['kind'] == 'tie' and len(gaps) >= 3


def test_pairs_reach_their_class(gold):
    """the class a pair is built to end in (from its construction: lengths and the distance its path leaves the diagonal) is the
    class that the reference's record leads to; every class is reached, each boundary from both sides"""
    ps = tbgen.pairs()
    n = len(ps)
    hit = 0
    for x, p in enumerate(ps):
        got = tbgen.golden_history(gold, x)
        assert got[-1] == str(gold['label'][x]), (p['name'], got)
        if p['dev'] is None:
            hit += 1
            continue
        hit += got == tbgen.history(len(p['q']), len(p['t']), p['dev'])
        assert tbgen.deviation(str(gold['bt'][x])) == p['dev']
    assert hit >= 0.95 * n, (hit, n)
    by_name = {p['name']: tbgen.golden_history(gold, x) for x, p in enumerate(ps)}
    # doubling: the last g a band reaches and the first that needs the next one, through every class and two global rounds
    want = {0: 'narrow128', 2: 'narrow192', 4: 'narrow320', 8: 'narrow384', 9: 'lds128', 16: 'lds128', 17: 'lds128', 32: 'lds128',
            33: 'lds512', 64: 'lds512', 65: 'lds512', 128: 'lds512', 129: 'lds2048', 256: 'lds2048', 512: 'lds2048', 513: 'global',
            1024: 'global', 1025: 'global'}
    for g_, c in want.items():
        h = by_name['double_g%d' % g_]
        assert h[-1] == c and (h[0].startswith('narrow') if g_ <= 513 else h[0] == 'lds128'), (g_, h)
    assert by_name['double_g1024'].count('global') == 1 and by_name['double_g1025'].count('global') == 2
    assert by_name['double_g513'] == ('narrow1024', 'lds128', 'lds512', 'lds2048', 'global')   # every hand-off in one task
    assert [tbgen.final_band(r[2] - r[1] + 1, r[4] - r[3] + 1, tbgen.deviation(str(b))) for r, b in zip(gold['res'][:18], gold['bt'][:18])] == \
           [1, 2, 4, 8, 16, 16, 32, 32, 64, 64, 128, 128, 256, 256, 512, 1024, 1024, 2048]
    # skew: first bands 2, 3, 6, 11; band 12 fails for skew_20_15 (lds128 at band 24), band 11 fails for skew_14_4
    for name, last in (('skew_3_2', 'narrow192'), ('skew_12_10', 'narrow384'), ('skew_10_5', 'narrow192'), ('skew_11_1', 'narrow320'),
                       ('skew_20_15', 'lds128'), ('skew_14_4', 'lds128'), ('skew_15_20', 'lds128')):
        assert by_name[name][-1] == last and by_name[name][0].startswith('narrow'), (name, by_name[name])
    # boundary: first bands 14 | 15, 62 | 63, 254 | 255, 1022 | 1023 enter each class at its first band, both orientations
    for d, c in ((13, 'narrow256'), (14, 'lds128'), (61, 'lds128'), (62, 'lds512'), (253, 'lds512'), (254, 'lds2048'), (1021, 'lds2048'),
                 (1022, 'global')):
        assert by_name['bound_t%d' % d] == (c,) and by_name['bound_q%d' % d] == (c,), d
    # row caps: c stays, c + 1 moves to the next class; 1025 rows, 1038 columns and band 15 leave the narrow classes
    caps = tbgen.NARROW_Q
    for i, c in enumerate(caps):
        nxt = 'narrow%d' % caps[i + 1] if i + 1 < len(caps) else 'lds128'
        assert by_name['rows_%d' % c] == ('narrow%d' % c,) and by_name['rows_%d' % (c + 1)] == (nxt,), c
    assert by_name['tcap_1024_1037'] == ('narrow1024',) and by_name['tcap_1025_1038'] == ('lds128',) and by_name['tcap_1024_1038'] == ('lds128',)
    # every class with an odd count of at least three and with an even count (tbgen.padded), device and host orchestration
    for hostpath, classes in ((False, tbgen.CLASSES), (True, tbgen.CLASSES[9:])):
        seen = set()
        for h, idx in tbgen.groups(gold, hostpath).items():
            seen |= set(h)
            assert len(tbgen.padded(idx, True)) % 2 == 1 and len(tbgen.padded(idx, True)) >= 3 and len(tbgen.padded(idx, False)) % 2 == 0
        assert seen == set(classes)
    first = tbgen.round_counts(gold, tbgen.shuffled(gold))
    assert all(first[(0, c)] >= 3 and first[(0, c)] % 2 == 1 for c in tbgen.CLASSES)


def test_history_restates_the_class_limits():
    h = tbgen.history
    assert h(100, 100, 8) == ('narrow128',) and h(100, 100, 9) == ('narrow128', 'lds128')
    assert h(100, 113, 0) == ('narrow128',) and h(100, 114, 0) == ('lds128',)
    assert h(1024, 1037, 0) == ('narrow1024',) and h(1025, 1038, 0) == ('lds128',)
    assert h(300, 361, 0) == ('lds128',) and h(300, 362, 0) == ('lds512',)       # w = 127 | 129
    assert h(300, 553, 0) == ('lds512',) and h(300, 554, 0) == ('lds2048',)      # w = 511 | 513
    assert h(300, 1321, 0) == ('lds2048',) and h(300, 1322, 0) == ('global',)    # w = 2047 | 2049
    assert h(2000, 2000, 2048) == ('lds128', 'lds512', 'lds2048', 'global', 'global')
    assert h(100, 100, 9, hostpath=True) == ('lds128',) * 5 and h(300, 362, 0, hostpath=True) == ('lds512',)
    assert tbgen.deviation('MMIIIMMDDDDDM') == 3 and tbgen.runs('MMIID') == [('M', 2), ('I', 2), ('D', 1)]
    assert np.array_equal(tbgen.padded([4, 5], True), [4, 5, 4]) and tbgen.padded([4], False) == [4, 4]
