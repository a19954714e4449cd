"""Writes tests/golden/rescore_diag_vectors.npz from the LIVE reference: sequences, 16-bit diagonals and what
DistanceCalculator::computeUngappedAlignment (M/src/alignment/DistanceCalculator.h:94-201) returns for them in rescore modes 0, 1
and 2, plus the entries doRescorediagonal's row logic gives for the short cases taken as a prefilter DB (ROW_SETS, sorted and unsorted):
the six fields of every row are the driver's, the E-values and bit scores the reference library's.  Results only.

The reference's function is a header template: DRIVER below (ours, a few lines) includes DistanceCalculator.h where it lies and is
compiled into a temporary directory, so nothing compiled is kept.  E-values and bit scores come from the reference library
(oracle/_ref/libsdref.so through oracle.pyoracle.RefSW).

    python tools/make_golden_rescore_diag.py [reference root]      (needs `make -C oracle _ref/libsdref.so`; no GPU)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import rescore_ref as rr   # noqa: E402

DRIVER = r'''
#include "DistanceCalculator.h"
#include <cstdio>
#include <string>
#include <vector>
// stdin: the 21 x 21 matrix, then "mode diagonal query target" lines; stdout: the six LocalAlignment fields per line
int main() {
    int M[21][21];
    for (auto &r : M) for (int &v : r) if (scanf("%d", &v) != 1) return 1;
    const char *alph = "ACDEFGHIKLMNPQRSTVWYX";
    int a2n[128];
    for (int c = 0; c < 128; c++) {
        int up = (c >= 'a' && c <= 'z') ? c - 32 : c;
        if (up == 'J') up = 'L';
        if (up == 'Z') up = 'E';
        if (up == 'B') up = 'D';
        const char *p = up ? strchr(alph, up) : NULL;
        a2n[c] = p ? (int) (p - alph) : 20;
    }
    const int range = 'z' + 1;   // SubstitutionMatrix::createAsciiSubMat's layout
    std::vector<char> data((size_t) range * range);
    std::vector<const char *> rows(range);
    for (int i = 0; i < range; i++) {
        rows[i] = data.data() + (size_t) i * range;
        for (int j = 0; j < range; j++) data[(size_t) i * range + j] = (char) M[a2n[i]][a2n[j]];
    }
    static char q[70000], t[70000];
    int mode, diag;
    while (scanf("%d %d %69999s %69999s", &mode, &diag, q, t) == 4) {
        std::string qs(q), ts(t);
        qs.append(64, '\0');   // computeInverseHammingDistance reads whole vectors
        ts.append(64, '\0');
        DistanceCalculator::LocalAlignment r = DistanceCalculator::computeUngappedAlignment(
            qs.c_str(), (unsigned) strlen(q), ts.c_str(), (unsigned) strlen(t), (unsigned short) diag, rows.data(), mode);
        printf("%u %d %d %u %u %d\n", r.score, r.startPos, r.endPos, r.diagonalLen, r.distToDiagonal, r.diagonal);
    }
    return 0;
}
'''


def build_driver(ref_root, tmp):
    """compiles DRIVER against the reference's headers into tmp; returns the program's path"""
    m = os.path.join(ref_root, 'lib', 'mmseqs')
    src, exe = os.path.join(tmp, 'driver.cpp'), os.path.join(tmp, 'driver')
    open(src, 'w').write(DRIVER)
    inc = [os.path.join(m, 'src', 'commons'), os.path.join(m, 'src', 'alignment'), os.path.join(m, 'lib'), os.path.join(m, 'lib', 'simd'),
           os.path.join(m, 'lib', 'simde'), os.path.join(m, 'lib', 'fmt')]
    subprocess.check_call(['g++', '-std=c++14', '-O1', '-mavx2', '-DAVX2=1', '-w'] + ['-I' + d for d in inc] + [src, '-o', exe])
    return exe


def run_driver(exe, M, cases):
    """cases: (mode, d16, query, target) -> int64 [n, 6]"""
    text = ' '.join(str(int(v)) for v in np.asarray(M).reshape(-1)) + '\n'
    text += ''.join('%d %d %s %s\n' % (m, int(d) & 0xFFFF, q, t) for m, d, q, t in cases)
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split('\n')
    rows = [[int(v) for v in line.split()] for line in out if line.strip()]
    assert len(rows) == len(cases)
    return np.array(rows, np.int64).reshape(len(cases), 6)


LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1025]
# parameter sets of the row logic (rescore_ref.rows keywords)
ROW_SETS = {
    'aln': dict(mode=2, e=1000.0, c=0.0, cov_mode=0, a=True),
    'alnstrict': dict(mode=2, e=0.001, c=0.5, cov_mode=2, a=False, min_aln_len=30, seq_id_mode=1, min_seq_id=0.3),
    'sub': dict(mode=1, e=10.0, c=0.3, cov_mode=0),
    'ham': dict(mode=0, c=0.0, min_seq_id=0.3),
}


def make_cases(rng, M):
    """(class, query, target, diagonal as given) -- the classes are what tests/test_gpu_rescore.py asserts to be present"""
    aa = np.array(list('ACDEFGHIKLMNPQRSTVWY'))
    rand = lambda n: ''.join(rng.choice(aa, n))

    def mutate(s, rate):
        s = np.array(list(s))
        hit = rng.random(len(s)) < rate
        s[hit] = rng.choice(aa, int(hit.sum()))
        return ''.join(s)

    master = rand(65535)
    cases = []
    for a in LENGTHS:
        for b in LENGTHS:
            q, t = master[:a], mutate(master[:b], 0.3)
            for d in sorted({0, 1, -1, 3, -3, a - 1, -(b - 1), a, -b, a + 5, -(b + 5)}):
                cases.append(('len', q, t, d))
    # negative diagonals in both encodings
    q, t = master[100:400], mutate(master[95:420], 0.2)
    for d in (-5, 65531, -1, 65535, -300, 65236):
        cases.append(('enc', q, t, d))
    # shifted homologs: the true diagonal, off the dword alignment
    for sh in (1, 2, 3, 5, 7, 130):
        cases.append(('len', master[sh:sh + 300], mutate(master[:280], 0.25), -sh))
        cases.append(('len', master[:280], mutate(master[sh:sh + 300], 0.25), sh))
    # long targets: at 32 767 one negative candidate, from 32 768 on a second one; one pair of the longest sequences
    for n in (32767, 32768):
        t = mutate(master[:n], 0.3)
        for d in (0, 5, -5, -200, 32000, -32000, 40000):
            cases.append(('long%d' % n, master[200:900], t, d))
        cases.append(('long%d' % n, t[:40000], master[:3000], 2000))
    cases.append(('long65535', master, mutate(master, 0.35), 0))
    cases.append(('long65535', master, mutate(master, 0.35)[7:], 7))
    cases.append(('long65535', master[9:], mutate(master, 0.35), -9))
    # ties, built from the matrix itself: two equal maxima with a reset between them (the earliest wins), a prefix that returns to
    # exactly 0 (the start moves behind it), an all-negative diagonal
    L = rr.ALPHABET[:20]
    sc = lambda x, y: int(M[L.index(x), L.index(y)])
    neg = min(((sc('W', y), y) for y in L))[1]
    assert sc('W', 'W') + 4 * sc('W', neg) <= 0
    cases.append(('tie_max', 'W' * 6, 'W' + neg * 4 + 'W', 0))
    cases.append(('tie_max', 'AW' + 'W' * 4 + 'WA', 'CW' + neg * 4 + 'WC', 0))
    zero = [(x, y) for x in L for y in L if sc(x, x) + sc(x, y) == 0]
    assert len(zero) >= 3
    for x, y in zero[:3]:
        cases.append(('tie_zero', x + x + 'WW', x + y + 'WW', 0))
    cases.append(('negative', 'W' * 8, neg * 8, 0))
    cases.append(('negative', 'W' * 4, neg * 8, -4))
    # letters: identity is not matrix code, mode 0 compares bytes as they are
    cases.append(('letters', 'MKBBZZLLXX**ACDEF', 'MKDDEEJJXX**ACDEF', 0))
    cases.append(('letters', 'MKDDEEJJUUOOACDEF', 'MKBBZZLLCCKKACDEF', 0))
    cases.append(('letters', 'mkvlaagivgLSACDEFwwhh', 'MKVLAAGIVGlsacdefWWHH', 0))
    cases.append(('letters', 'xACDEFGHIKLMNPQRSTVWYx', 'XACDEFGHIKLMNPQRSTVWYX', 0))
    cases.append(('letters', 'ACDEF*GHIKL*', 'ACDEFXGHIKLX', 0))
    # identity hits (the query against itself on the main diagonal: a positive score)
    for n in (1, 2, 65, 257):
        cases.append(('self', master[:n], master[:n], 0))
    low = master[500:800].lower()
    cases.append(('letters', low, mutate(master[500:800], 0.2), 0))
    cases.append(('letters', low[3:], mutate(master[500:800], 0.2), -3))
    return cases


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    from spacedust_amd.api import Host
    from oracle.pyoracle import Ref, RefSW
    host = Host()
    M = host.matrix(0)[0].reshape(21, 21).astype(np.int8)
    assert (host.matrix(0)[2][:123] == rr.A2N[:123]).all()
    rng = np.random.default_rng(20261017)
    cases = make_cases(rng, M)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        ref = {mode: run_driver(exe, M, [(mode, d, q, t) for _, q, t, d in cases]) for mode in (0, 1, 2)}
    # keep identity-like hits with score 0 out (the reference reads querySeq[-1] there): nothing here is an identity hit
    pool, index = [], {}
    for _, q, t, _ in cases:
        for s in (q, t):
            if s not in index:
                index[s] = len(pool)
                pool.append(s)
    off = np.zeros(len(pool) + 1, np.int64)
    np.cumsum([len(s) for s in pool], out=off[1:])
    # the row logic: the short cases as one prefilter DB over the pool (key = pool index, an entry per query, rows in case order), run
    # through ROW_SETS.  Fields from the driver, the identity count over the driver's [start, end], E-values from the reference.
    db_res = 1350000
    sw = RefSW(Ref(), 70000, db_res)
    entries = {}
    for x, (_, q, t, d) in enumerate(cases):
        # (identity hits with score 0 stay out: the reference reads querySeq[-1] there)
        if max(len(q), len(t)) <= 1100 and not (index[q] == index[t] and min(int(ref[m][x][0]) for m in (0, 1, 2)) == 0):
            entries.setdefault(index[q], []).append(x)
    row_q = np.array(sorted(entries), np.int32)
    texts = {}
    for name, kw in ROW_SETS.items():
        mode = kw['mode']
        for srt in (0, 1):
            out = []
            for qk in row_q:
                xs = entries[int(qk)]
                fields = []
                for x in xs:
                    own = rr.compute(M, cases[x][1], cases[x][2], cases[x][3], mode)
                    assert own[:6] == tuple(int(v) for v in ref[mode][x])
                    fields.append(tuple(int(v) for v in ref[mode][x]) + (own[6],))
                pref = [(index[cases[x][2]], 0, cases[x][3]) for x in xs]
                out.append(rr.rows(M, pool[int(qk)], pool.__getitem__, int(qk), pref, sw.evalue, sw.bitscore, sort=bool(srt), fields=fields, **kw))
            texts['rows_%s_%d' % (name, srt)] = np.array(out)
            print(name, srt, sum(t.count('\n') for t in out), 'rows')
    np.savez_compressed(rr.GOLDEN, M=M, letters=np.frombuffer(''.join(pool).encode(), np.uint8), off=off,
                        cls=np.array([c for c, _, _, _ in cases]), q=np.array([index[q] for _, q, _, _ in cases], np.int32),
                        t=np.array([index[t] for _, _, t, _ in cases], np.int32), diag=np.array([d for _, _, _, d in cases], np.int32),
                        ref0=ref[0].astype(np.int32), ref1=ref[1].astype(np.int32), ref2=ref[2].astype(np.int32),
                        db_res=np.int64(db_res), row_q=row_q, **texts)
    print('%d cases, %d sequences; wrote %s (%d bytes)' % (len(cases), len(pool), rr.GOLDEN, os.path.getsize(rr.GOLDEN)))


if __name__ == '__main__':
    main()
