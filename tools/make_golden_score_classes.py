#!/usr/bin/env python3
"""Golden rows for the constructed score-class pairs of tests/scgen.py: every pair through the REAL reference classes
(oracle/_ref/libsdref.so) in alignment modes 0, 1 and 2 with the default gates (E-value 10, query coverage 0.8) into
tests/golden/score_classes.npz: score, coordinates, identities, backtrace length, E-value and the mode-2 backtrace, the
pair's name and kind, the classes it is meant for, a digest of the letters (the generator supplies them), and the same for
the profile twins (set_query_profile).  The reference keeps to itself whether it reran a pair with the word kernel; it does
so when the byte score saturates, score + bias >= 255, which is what the rows say, and the oracle's flag agrees.
Writes the archive with fixed time stamps: it regenerates byte for byte.  Dev container only:
python tools/make_golden_score_classes.py"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.pyoracle import Oracle, Ref, RefSW  # noqa: E402
from spacedust_amd.api import Host  # noqa: E402
import scgen  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
DB_RESIDUES = 10 ** 7


def save(path, arrays):
    with zipfile.ZipFile(path, 'w') as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED, 9)


def rows_of(sw, orc_align, targets, bias):
    """([mode][pair] rows, E-values, mode-2 backtraces, word flags) of the pairs whose query is loaded into sw"""
    res, evs, bts, word, nocov = [[] for _ in scgen.MODES], [[] for _ in scgen.MODES], [], [], []
    for t in targets:
        o = orc_align(t)
        for mode in scgen.MODES:
            r = sw.align(t, sw_mode=mode)
            res[mode].append([r[k] if k != 'identical' or r['btLen'] > 0 else 0 for k in scgen.FIELDS])
            evs[mode].append(r['evalue'])
        bts.append(r['backtrace'])
        r0 = sw.align(t, sw_mode=2, cov_thr=0.0)
        nocov.append((r0['backtrace'], r0['qStart']))
        same = all(o[k] == r[k] for k in ('score', 'qStart', 'qEnd', 'tStart', 'tEnd', 'btLen', 'backtrace', 'evalue'))
        word.append(int(r['score'] + bias >= 255))
        assert word[-1] == (o['flags'] & 1), (t, r, o)
        if not same:
            print('   ORACLE DIFFERS', r, o)
    return res, evs, bts, word, nocov


def main():
    ref, orc, host = Ref(6), Oracle(4), Host()
    seqs, pairs = scgen.build()
    num = [orc.map_sequence(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    sw_bias, _, _ = host.comp_bias(np.concatenate(num), off)
    mat, _, _ = host.matrix(0)
    mat = np.array([mat[i] for i in range(441)], np.int32)
    wrl = 32767 // (int(mat.max()) + max(0, int(sw_bias.max())))
    sw = RefSW(ref, max(len(s) for s in seqs), DB_RESIDUES)
    out = {k: [[] for _ in scgen.MODES] for k in ('res', 'evalue', 'p_res', 'p_evalue')}
    out.update({k: [] for k in ('bt', 'word', 'qbias', 'p_bt', 'p_word', 'p_qbias', 'p_twin', 'bt_nocov', 'start_nocov', 'p_bt_nocov', 'p_start_nocov')})
    p_wrl = 1 << 30
    for x, p in enumerate(pairs):
        q, t = p['q'], p['t']
        bias = abs(int(mat.min())) + abs(min(0, int(sw_bias[int(off[q]):int(off[q + 1])].min())))
        sw.set_query(seqs[q])
        res, evs, bts, word, nocov = rows_of(sw, lambda t_: orc.sw_align(num[q], orc.map_sequence(t_), DB_RESIDUES), [seqs[t]], bias)
        for m in scgen.MODES:
            out['res'][m] += res[m]
            out['evalue'][m] += evs[m]
        out['bt'] += bts
        out['bt_nocov'].append(nocov[0][0])
        out['start_nocov'].append(nocov[0][1])
        out['word'] += word
        out['qbias'].append(bias)
        r = res[2][0]
        gaps = scgen.gap_runs(nocov[0][0], nocov[0][1])
        print('%-18s %4d x %4d score %5d word %d qEnd+1 %4d start %5d E %.2g gaps %s' % (p['name'], len(seqs[q]), len(seqs[t]), r[0], word[0],
                                                                                     r[2] + 1, r[1], evs[2][0], gaps[:4]))
        if p['name'] in scgen.PROFILE_TWINS:
            rec = scgen.profile_record(num[q], mat, 1000 + x)
            prof = host.map_profiles(rec, np.array([0, len(rec)], np.uint64))
            pbias = -min(0, int(prof['aln'][:, :20].min()))
            p_wrl = min(p_wrl, 32767 // max(1, int(prof['aln'].max())))
            sw.set_query_profile(rec)
            res, evs, bts, word, nocov = rows_of(sw, lambda t_: orc.sw_align_profile(prof['letters'], prof['aln'], orc.map_sequence(t_), DB_RESIDUES),
                                          [seqs[t]], pbias)
            for m in scgen.MODES:
                out['p_res'][m] += res[m]
                out['p_evalue'][m] += evs[m]
            out['p_bt'] += bts
            out['p_bt_nocov'].append(nocov[0][0])
            out['p_start_nocov'].append(nocov[0][1])
            out['p_word'] += word
            out['p_qbias'].append(pbias)
            out['p_twin'].append(x)
            print('   as a profile: score %5d word %d qEnd+1 %4d start %5d' % (res[2][0][0], word[0], res[2][0][2] + 1, res[2][0][1]))
    tw = out['p_twin']
    arrays = dict(name=np.array([p['name'] for p in pairs]), kind=np.array([p['kind'] for p in pairs]),
                  q=np.array([p['q'] for p in pairs], np.int32), t=np.array([p['t'] for p in pairs], np.int32),
                  qlen=np.array([len(seqs[p['q']]) for p in pairs], np.int32), tlen=np.array([len(seqs[p['t']]) for p in pairs], np.int32),
                  digest=np.array(scgen.digest(seqs)), n_seqs=np.int64(len(seqs)), db_residues=np.int64(DB_RESIDUES),
                  res=np.array(out['res'], np.int32), evalue=np.array(out['evalue'], np.float64), bt=np.array('\n'.join(out['bt'])),
                  bt_nocov=np.array('\n'.join(out['bt_nocov'])), start_nocov=np.array(out['start_nocov'], np.int32),
                  p_bt_nocov=np.array('\n'.join(out['p_bt_nocov'])), p_start_nocov=np.array(out['p_start_nocov'], np.int32),
                  word=np.array(out['word'], np.uint8), qbias=np.array(out['qbias'], np.int32), wide_row_limit=np.int64(wrl),
                  p_twin=np.array(tw, np.int32), p_res=np.array(out['p_res'], np.int32), p_evalue=np.array(out['p_evalue'], np.float64),
                  p_bt=np.array('\n'.join(out['p_bt'])), p_word=np.array(out['p_word'], np.uint8), p_qbias=np.array(out['p_qbias'], np.int32),
                  p_qlen=np.array([len(seqs[pairs[x]['q']]) for x in tw], np.int32),
                  p_tlen=np.array([len(seqs[pairs[x]['t']]) for x in tw], np.int32), p_wide_row_limit=np.int64(p_wrl))
    save(os.path.join(GOLD, 'score_classes.npz'), arrays)
    print(len(pairs), 'pairs', len(seqs), 'sequences', 'wideRowLimit', wrl, 'profiles', p_wrl,
          os.path.getsize(os.path.join(GOLD, 'score_classes.npz')), 'bytes')


if __name__ == '__main__':
    main()
