#!/usr/bin/env python3
"""Golden vectors for k = 5, the reference's k-mer size for a sequence query DB against a profile target DB (Search.cpp:251-257):
spaced seed 110010000101 (span 12, Sequence.h:21), k-mer generator split 2 + 3 (KmerGenerator.cpp:69-85), a table of 20^5 k-mers.
Everything is produced by the REAL reference classes (oracle/_ref/libsdref.so: Sequence, KmerGenerator, IndexTable / IndexBuilder,
QueryMatcher, UngappedAlignment); the profile-target index by the driver of tools/make_golden_target_profile.py compiled at k = 5
into a temporary directory (nothing compiled is kept).  Dev container only:  python tools/make_golden_k5.py

Writes tests/golden/k5_vectors.npz (tests/k5gold.py reads it; tests/test_k5_host.py checks the conditions asserted here):
  windows / lists        similar-k-mer lists of 12 random windows at thresholds 70 ... 110
  pwindows / plists      profile k-mer lists of 6 profile positions (profiles of profile_vectors.npz)
  blob / off             the small part of the crafted DB: the k7 DB, sequences of 11, 12 and 13 residues, an X in each of the five
                         seed positions of one window, a tantan-masked stretch (sequence 10)
  fam_base / fam_mut     the family behind it: near-copies of one 300-mer, so many that the base's index hits overflow the
                         reference's hit buffer (2 * 10^6 entries, QueryMatcher.cpp:43-47) -- see FAMILY below
  index_triples          the reference's index entries (k-mer, sequence, position) of the small part at threshold 88
  pf_rows_88 / _75       prefilter rows (query, target, score, diagonal) of `queries` against the whole DB; index_hits_*: dbMatches
  prof_rows_82 / _70     rows of 8 profile queries against the sequences of profile_vectors.npz (index threshold 0)
  PT*                    the index of the 18 profiles as a profile target at k = 5, thresholds 82 and 75: counts, digest, rows
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import k5gold  # noqa: E402
import make_golden_k7 as k7  # noqa: E402
import make_golden_target_profile as tp  # noqa: E402
from oracle.pyoracle import Ref  # noqa: E402

AA = k7.AA
# The family.  Every near-copy adds about one index hit per window of the base (a k-mer's list holds a sequence once), so the base's
# index hits are about copies x 289: 200 copies give 6 * 10^4, and the buffer of 2 * 10^6 overflows from about 7 000 copies on.
# They are stored as the base and the substitutions, not as sequences.
FAMILY, FAMILY_LEN, FAMILY_RATE = 7600, 300, 0.01


def crafted():
    rng = np.random.default_rng(55)
    seqs = k7.crafted()
    special = {}
    for n in (11, 12, 13):   # no window, one window, two windows
        special['len%d' % n] = len(seqs)
        seqs.append(''.join(rng.choice(list(AA), n)))
    for p in k5gold.SEED:    # window 20 of a 60-mer holds an X in seed position p
        s = list(seqs[0][:60])
        s[20 + p] = 'X'
        special['x%d' % p] = len(seqs)
        seqs.append(''.join(s))
    base = ''.join(rng.choice(list(AA), FAMILY_LEN))
    mut = []
    for c in range(1, FAMILY):   # copy 0 is the base itself
        for p in np.nonzero(rng.random(FAMILY_LEN) < FAMILY_RATE)[0]:
            mut.append((c, int(p), ord(AA[rng.integers(20)])))
    mut.append((FAMILY - 1, 0, ord(base[0])))   # (the last copy has a row, so that the number of copies can be read from the rows)
    return seqs, special, base.encode(), np.array(mut, np.int64)


def main():
    ref = Ref(5)
    rng = np.random.default_rng(5)
    out = {}
    # ---- similar k-mers of sequence windows
    windows = rng.integers(0, 20, (12, 5)).astype(np.uint8)
    thrs = rng.integers(70, 111, 12)
    lists = [np.asarray(ref.kmer_list(w, int(t)), np.uint32) for w, t in zip(windows, thrs)]
    assert all(len(x) > 0 for x in lists)
    out.update(windows=windows, window_thr=thrs, list_off=np.cumsum([0] + [len(x) for x in lists]).astype(np.uint64), lists=np.concatenate(lists))
    print('window lists', [len(x) for x in lists])
    # ---- profile k-mers
    profiles, pseqs = k5gold.profile_inputs()
    pw, pl = [], []
    for pi, pos, want in [(0, 3, 2000), (1, 10, 100), (2, 0, 20000), (5, 20, 10), (7, 40, 5000), (9, 11, 500)]:
        # the highest threshold at which the window's list holds `want` k-mers or more
        thr = next(t for t in range(120, -200, -1) if len(ref.profile_kmer_list(profiles[pi], pos, t)) >= want)
        kl = ref.profile_kmer_list(profiles[pi], pos, thr).astype(np.uint32)
        assert len(kl) > 0
        pw.append((pi, pos, thr))
        pl.append(kl)
    out.update(pwindows=np.array(pw), plist_off=np.cumsum([0] + [len(x) for x in pl]).astype(np.uint64), plists=np.concatenate(pl))
    print('profile lists', [len(x) for x in pl])
    # ---- the crafted DB
    small, special, base, mut = crafted()
    out.update(blob=np.frombuffer(''.join(small).encode(), np.uint8), off=k5gold.offsets_of(small), fam_base=np.frombuffer(base, np.uint8),
               fam_mut=np.stack([mut[:, 0].astype(np.uint16), mut[:, 1].astype(np.uint16), mut[:, 2].astype(np.uint16)], axis=1))
    out.update({'special_' + k: np.int64(v) for k, v in special.items()})
    seqs, n_small = k5gold.sequences(out)
    assert n_small == len(small) and len(seqs) == n_small + FAMILY and seqs[n_small] == base.decode()
    lens = np.array([len(s) for s in seqs])
    off = k5gold.offsets_of(seqs)
    blob = ''.join(seqs).encode()
    # the reference's index of the small part, entry for entry
    six = ref.index(''.join(small).encode(), k5gold.offsets_of(small), kmer_thr=88)
    soff, ses, sep, slk = six.dump()
    assert six.table_size == k5gold.TABLE and six.masked_residues > 0, 'no tantan-masked residue'
    t = k5gold.index_triples(soff, ses, sep)
    assert len(t) == six.n_entries > 0
    for n, want in ((11, 0), (12, 1), (13, 2)):
        assert int((t[:, 1] == special['len%d' % n]).sum()) == want, n
    for p in k5gold.SEED:   # 60 - 12 + 1 windows, five of them hold the X
        assert 30 < int((t[:, 1] == special["x%d" % p]).sum()) <= 49 - 5, p
    out['index_triples'] = np.stack([t[:, 0].astype(np.uint32), t[:, 1].astype(np.uint32), t[:, 2].astype(np.uint32)], axis=1)
    out['index_masked_residues'] = np.int64(six.masked_residues)
    out['index_lookup'] = slk
    print('small index: %d entries, %d masked residues' % (six.n_entries, six.masked_residues))
    # prefilter rows: every third sequence of the small part, the special ones, the family's base (the overflowing query) and a copy
    queries = sorted(set(range(0, n_small, 3)) | set(special.values()) | {n_small, n_small + 7})
    out['queries'] = np.array(queries, np.int64)
    # the identity id of a query that is in the DB is its own id -- QueryMatcher then adds the self hit whatever the k-mers find, so the
    # three short sequences go without one (0xFFFFFFFF): the 11-residue one, which has no window, must come back empty
    no_id = {special['len%d' % n] for n in (11, 12, 13)}
    ident = np.array([0xFFFFFFFF if q in no_id else q for q in queries], np.int64)
    out['query_identity'] = ident
    for thr in (88, 75):
        rix = ref.index(blob, off, kmer_thr=thr)
        rpf = rix.prefilter(int(lens.max()), max_hits=300)
        rows, hits = [], []
        for q, qid in zip(queries, ident):
            ids, sc, dg, st = rpf.query(seqs[q], int(qid))
            rows += [(int(q), int(t_), int(s), int(d)) for t_, s, d in zip(ids, sc, dg)]
            hits.append(int(st[1]))
        rows = np.array(rows, np.int64)
        out['pf_rows_%d' % thr] = rows
        out['index_hits_%d' % thr] = np.array(hits, np.int64)
        over = hits[queries.index(n_small)]
        print('thr', thr, 'rows', len(rows), 'index hits of the family base', over)
        assert len(rows) > 0 and over > k5gold.HIT_BUFFER, 'the family base does not overflow the hit buffer'
        assert not (rows[:, 0] == special['len11']).any(), 'the 11-residue sequence has a row'
        assert (rows[:, 0] == special['len12']).sum() == 1 and (rows[:, 0] == special['len13']).sum() == 1   # their own k-mers find them
        diags = [len(set(rows[(rows[:, 0] == q), 3] & 0xFFFF)) for q in queries]
        assert max(diags) > 1, 'no query with hits on more than one diagonal'
    # ---- profile queries against the sequences of profile_vectors.npz
    plens = np.array([len(s) for s in pseqs])
    pix = ref.index(''.join(pseqs).encode(), k5gold.offsets_of(pseqs), kmer_thr=0)
    for thr in (82, 70):
        rpf = pix.prefilter_profile(int(max(plens.max(), 450)) + 10, thr, max_hits=300)
        rows = []
        for qi in range(8):
            ids, sc, dg, _ = rpf.query(profiles[qi], identity_id=4 * qi if qi % 2 == 0 else 0xFFFFFFFF)
            rows += [(qi, int(t_), int(s), int(d)) for t_, s, d in zip(ids, sc, dg)]
        assert rows
        out['prof_rows_%d' % thr] = np.array(rows, np.int64)
        print('profile queries thr', thr, 'rows', len(rows))
    # ---- the profile-target index at k = 5 (the driver of make_golden_target_profile.py with its k-mer size replaced)
    assert tp.DRIVER.count('kmerSize = 6;') == 1
    tp.DRIVER = tp.DRIVER.replace('kmerSize = 6;', 'kmerSize = 5;')
    with tempfile.TemporaryDirectory() as tmp:
        exe = tp.build_driver('/root/reference', tmp)
        for thr in (82, 75):
            r = tp.run_driver(exe, tmp, profiles, pseqs, thr, comp_bias=True, want_rows=True)
            tag = 'PT%d' % thr
            out[tag + '_entries'] = np.int64(r['n_entries'])
            out[tag + '_records'] = np.int64(r['n_records'])
            out[tag + '_per_target'] = np.bincount(r['entry_seq'], minlength=len(profiles)).astype(np.int64)
            out[tag + '_digest'] = np.array(tp.digest(r['list_kmer'], r['list_start'], r['entry_seq'], r['entry_pos']))
            out[tag + '_rows'] = r['rows']
            out[tag + '_kmers'] = r['kmer_list_len']
            assert r['n_entries'] > 0 and len(r['rows']) > 0
            print('profile target thr %d: %d records, %d entries, longest window list %d, %d rows'
                  % (thr, r['n_records'], r['n_entries'], r['window_len'].max(), len(r['rows'])))
    np.savez_compressed(k5gold.GOLDEN, **out)
    size = os.path.getsize(k5gold.GOLDEN)
    print('wrote %s (%d bytes)' % (k5gold.GOLDEN, size))
    assert size < (1 << 20)


if __name__ == '__main__':
    main()
