"""Constructed inputs of `expandaln` (tools/make_golden_expand.py records what the reference makes of them in
tests/golden/expand_vectors.npz; tests/test_expandaln.py asserts every class's defining condition on the file, tests/test_gpu_expandaln.py
runs the kernels and the module on them).

Set K: one query per named class, expanded at the module's defaults.  Set P: one query whose rows lie on either side of every
criterion's threshold, expanded under several parameter sets."""
import numpy as np

import exp_ref


def line(key, score, seqid, ev, q_start, q_len, db_start, db_len, cigar):
    """an alignment row with a run-length backtrace; the ends follow from the backtrace (query: M and I, target: M and D)"""
    bt = exp_ref.uncompress(cigar)
    q_end = q_start + sum(c in 'MI' for c in bt) - 1
    db_end = db_start + sum(c in 'MD' for c in bt) - 1
    return ('%d\t%d\t%s\t%.3E\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n' % (key, score, seqid, ev, q_start, q_end, max(q_len, q_end + 1), db_start, db_end,
                                                         max(db_len, db_end + 1), cigar)).encode()


def random_cigar(rng, n_runs, lo=1, hi=20, first='M'):
    out, st = [], first
    for _ in range(n_runs):
        out.append('%d%s' % (int(rng.integers(lo, hi + 1)), st))
        if st == 'M':
            st = 'ID'[int(rng.integers(0, 2))]
        elif rng.random() < 0.15:   # a gap run of the other kind straight behind this one
            st = 'D' if st == 'I' else 'I'
        else:
            st = 'M'
    return ''.join(out)


# class name -> query key of set K
K_CLASSES = ['ab_earlier', 'bc_earlier', 'same_start', 'skip_exhausts_ab', 'skip_exhausts_bc', 'id_di_middle', 'only_id_di',
             'gap_after_last_m', 'no_m', 'one_column', 'long_runs', 'single_3000m', 'cluster_1', 'cluster_300', 'two_b_first_kept',
             'two_b_first_fails_e', 'two_b_nonoverlap_dropped', 'b_absent', 'empty_ab']
K_QUERY = {name: i for i, name in enumerate(K_CLASSES)}


def set_k():
    """returns (ab_db, bc_db): dict key -> bytes"""
    rng = np.random.default_rng(20261020)
    ab, bc = {}, {}
    q = K_QUERY
    ab[q['ab_earlier']] = line(100, 80, '0.412', 1e-20, 2, 60, 3, 70, '20M2I10M3D15M')
    bc[100] = line(1000, 90, '0.800', 1e-25, 10, 70, 4, 60, '30M1D12M')
    ab[q['bc_earlier']] = line(101, 75, '0.350', 1e-18, 0, 50, 15, 80, '8M2I10M2D20M')
    bc[101] = line(1001, 95, '0.900', 1e-28, 5, 80, 1, 90, '12M3I25M2D10M')
    ab[q['same_start']] = line(102, 60, '0.300', 1e-12, 4, 40, 7, 50, '10M1D10M1I10M')
    bc[102] = line(1002, 88, '0.700', 1e-22, 7, 50, 0, 45, '15M2D14M')
    # the distance in B is larger than the columns the earlier backtrace has: the skip loop ends at its end, nothing is left to translate
    ab[q['skip_exhausts_ab']] = line(103, 40, '0.250', 1e-8, 1, 30, 0, 90, '3M4I2M')
    bc[103] = line(1003, 70, '0.600', 1e-15, 50, 90, 2, 60, '30M')
    ab[q['skip_exhausts_bc']] = line(104, 40, '0.250', 1e-8, 1, 90, 60, 90, '25M')
    bc[104] = line(1004, 70, '0.600', 1e-15, 0, 90, 2, 60, '4M5D3M')
    ab[q['id_di_middle']] = line(105, 66, '0.333', 1e-14, 0, 40, 5, 40, '10M3I10M3D10M')
    bc[105] = line(1005, 77, '0.650', 1e-17, 5, 40, 0, 40, '10M3D10M3I10M')
    ab[q['only_id_di']] = line(106, 30, '0.200', 1e-6, 0, 10, 0, 10, '4I4D')
    bc[106] = line(1006, 30, '0.200', 1e-6, 0, 10, 0, 10, '4D4I')
    # gap columns behind the last M: the ends count them, the printed backtrace does not
    ab[q['gap_after_last_m']] = line(107, 55, '0.400', 1e-11, 3, 40, 0, 40, '10M5D') + line(108, 54, '0.390', 1e-10, 3, 40, 0, 40, '12M4I2D')
    bc[107] = line(1007, 66, '0.500', 1e-13, 0, 40, 6, 40, '15M')
    bc[108] = line(1008, 66, '0.500', 1e-13, 0, 40, 6, 40, '18M')
    ab[q['no_m']] = line(109, 20, '0.100', 1e-5, 0, 10, 0, 10, '6I')
    bc[109] = line(1009, 20, '0.100', 1e-5, 0, 10, 0, 10, '6M')
    ab[q['one_column']] = line(110, 10, '1.00', 1e-4, 5, 10, 5, 10, '1M')
    bc[110] = line(1010, 10, '1.00', 1e-4, 5, 10, 5, 10, '1M')
    ab[q['long_runs']] = line(111, 900, '0.444', 1e-200, 11, 9000, 40, 9000, random_cigar(rng, 640, 1, 18))
    bc[111] = line(1011, 950, '0.555', 1e-210, 3, 9000, 9, 9000, random_cigar(rng, 700, 1, 16))
    ab[q['single_3000m']] = line(112, 2000, '0.990', 1e-300, 0, 3000, 0, 3000, '3000M')
    bc[112] = line(1012, 2000, '0.990', 1e-300, 7, 3000, 0, 3000, '2990M')
    ab[q['cluster_1']] = line(113, 70, '0.420', 1e-15, 0, 50, 0, 50, '20M1I20M')
    bc[113] = line(1013, 99, '1.00', 1e-30, 0, 50, 0, 50, '50M')
    ab[q['cluster_300']] = line(114, 120, '0.470', 1e-30, 2, 120, 5, 130, '30M2D30M3I40M')
    bc[114] = b''.join(line(2000 + m, 100 + m % 7, '0.6%02d' % (m % 100), 1e-20, int(rng.integers(0, 12)), 130, int(rng.integers(0, 9)), 140,
                            random_cigar(rng, int(rng.integers(1, 12)), 3, 30)) for m in range(300))
    # one C (key 1500) behind two B's
    ab[q['two_b_first_kept']] = line(120, 80, '0.410', 1e-20, 0, 60, 0, 60, '40M') + line(121, 70, '0.400', 1e-18, 5, 60, 0, 60, '30M')
    bc[120] = line(1500, 90, '0.800', 1e-25, 0, 60, 0, 60, '40M')
    bc[121] = line(1500, 85, '0.790', 1e-24, 0, 60, 3, 60, '30M') + line(1501, 85, '0.790', 1e-24, 0, 60, 0, 60, '30M')
    ab[q['two_b_first_fails_e']] = line(120, 20, '0.410', 1.0, 0, 60, 0, 60, '40M') + line(121, 70, '0.400', 1e-18, 5, 60, 0, 60, '30M')
    # the second candidate covers A 100 .. 119, the first A 0 .. 19: no overlap, and still one row
    ab[q['two_b_nonoverlap_dropped']] = line(122, 80, '0.410', 1e-20, 0, 200, 0, 60, '20M') + line(123, 70, '0.400', 1e-18, 100, 200, 0, 60, '20M')
    bc[122] = line(1502, 90, '0.800', 1e-25, 0, 60, 0, 60, '20M')
    bc[123] = line(1502, 85, '0.790', 1e-24, 0, 60, 30, 60, '20M')
    ab[q['b_absent']] = line(999, 80, '0.410', 1e-20, 0, 60, 0, 60, '40M') + line(113, 70, '0.420', 1e-15, 0, 50, 0, 50, '20M1I20M')
    ab[q['empty_ab']] = b''
    return ab, bc


# parameter sets of set P (exp_ref.DEFAULTS for what is not named), and per set the criterion it moves
P_PARAMS = [dict(), dict(c=0.5, cov_mode=0), dict(c=0.5, cov_mode=1), dict(c=0.5, cov_mode=2), dict(min_seq_id=0.3), dict(min_aln_len=30),
            dict(e=1e-5)]


def set_p():
    ab, bc = {}, {}
    rows = [(200, '0.299', 1e-10, '100M'), (201, '0.300', 1e-10, '100M'), (202, '0.500', 9.99e-4, '100M'), (203, '0.500', 1.01e-3, '100M'),
            (204, '0.500', 1e-5, '100M'), (205, '0.500', 1.001e-5, '100M'), (206, '0.500', 1e-10, '49M'), (207, '0.500', 1e-10, '50M'),
            (208, '0.500', 1e-10, '50M'), (209, '0.500', 1e-10, '49M'), (210, '0.500', 1e-10, '29M'), (211, '0.500', 1e-10, '30M')]
    ab[0] = b''.join(line(b, 50 + i, sid, ev, 0, 100, 0, 300, cig) for i, (b, sid, ev, cig) in enumerate(rows))
    c_len = {206: 49, 207: 50, 208: 200, 209: 60}
    for b, _, _, cig in rows:
        bc[b] = line(3000 + b, 60, '0.700', 1e-12, 0, 300, 0, c_len.get(b, 100), cig)
    return ab, bc


def pair_facts(ab_row, bc_row):
    """what happens to one (AB row, BC row) pair, on expanded columns (rows as exp_ref.parse_row gives them)"""
    a, b = exp_ref.uncompress(ab_row['cigar']), exp_ref.uncompress(bc_row['cigar'])
    dist = abs(ab_row['db_start'] - bc_row['q_start'])
    off_a = off_b = moved = 0
    if ab_row['db_start'] < bc_row['q_start']:
        while moved < dist and off_a < len(a):
            moved += a[off_a] in 'MD'
            off_a += 1
    elif ab_row['db_start'] > bc_row['q_start']:
        while moved < dist and off_b < len(b):
            moved += b[off_b] in 'MI'
            off_b += 1
    cols = [exp_ref.TABLE[(x, y)] for x, y in zip(a[off_a:], b[off_b:])]
    emitted = [c for c in cols if c is not None]
    last_m = max([i + 1 for i, c in enumerate(emitted) if c == 'M'], default=0)
    return dict(ab_start_b=ab_row['db_start'], bc_start_b=bc_row['q_start'], dist=dist, skip_short=moved < dist,
                none_columns=sum(c is None for c in cols), lockstep_columns=len(cols), emitted=len(emitted), last_m=last_m,
                none_in_middle=any(c is None for c in cols) and cols and cols[0] is not None and cols[-1] is not None,
                ab_columns=len(a), bc_columns=len(b), ab_runs=len(exp_ref.runs_of(ab_row['cigar'])), bc_runs=len(exp_ref.runs_of(bc_row['cigar'])))
