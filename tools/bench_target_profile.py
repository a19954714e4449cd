#!/usr/bin/env python3
"""What the prefilter against a profile target costs on the device: set G of tests/golden/profile_vectors.npz (18 crafted profiles,
5 084 positions) repeated to about 10^6 positions, indexed by sd_target_build_profile at the default profile threshold
(Host.profile_kmer_threshold(4.0, k); -k 6 unless given, -k 5 is the reference's k for this search), then 8 192 sequence queries (the golden sequences, repeated) through sd_prefilter_batch.
Every timed call ends in a device synchronise inside the library; the first build and the first query pass are warm-up.

    python tools/bench_target_profile.py [-k 6] [--positions 1000000] [--queries 8192] [--runs 3] [--out profiles/target_profile.txt]
    python tools/bench_target_profile.py --search      (adds: the same input as DBs through `sdgpu prefilter | swapresults | align |
                                                        swapresults` one by one and through `sdgpu search`, wall time of each process)

The reference's build of the same input on a CPU: python tools/make_golden_target_profile.py --time-build REPS THR (dev container)."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden', 'profile_vectors.npz')


def write_db(path, payloads, dbtype):
    """entry i = payloads[i] with key i, in the reference's DB layout (data, .index, .dbtype)"""
    off = 0
    with open(path, 'wb') as f, open(path + '.index', 'w') as ix:
        for key, p in enumerate(payloads):
            f.write(p + b'\0')
            ix.write('%d\t%d\t%d\n' % (key, off, len(p) + 1))
            off += len(p) + 1
    with open(path + '.dbtype', 'wb') as f:
        f.write(struct.pack('<i', dbtype))


def search_leg(log, data, poff, seqs, sensitivity, runs, k):
    """the target-profile search on DBs: the four modules one by one, then `sdgpu search` (which runs them in one process with the
    target resident); every time is the wall time of one process, DB loads and writes included"""
    sdgpu = os.path.join(ROOT, 'spacedust_amd', 'sdgpu')
    threads = str(min(16, os.cpu_count() or 1))
    with tempfile.TemporaryDirectory() as tmp:
        q, t = os.path.join(tmp, 'seq'), os.path.join(tmp, 'prof')
        write_db(q, [s.encode() + b'\n' for s in seqs], 0)
        write_db(t, [data[int(poff[i]):int(poff[i + 1])] for i in range(len(poff) - 1)], 2)
        common = ['--threads', threads, '-v', '0']
        pref = ['-k', str(k), '-s', str(sensitivity), '--max-seqs', '300', '-c', '0', '--cov-mode', '0', '--comp-bias-corr', '1', '--min-ungapped-score', '15']
        aln = ['-a', '1', '-e', '0.001', '--max-seqs', '2147483647', '-c', '0', '--cov-mode', '0']
        steps = (('prefilter', [q, t, tmp + '/pref'] + pref), ('swapresults (prefilter rows)', [q, t, tmp + '/pref', tmp + '/pref_swapped', '-e', '0.001']),
                 ('align', [t, q, tmp + '/pref_swapped', tmp + '/aln_swapped'] + aln),
                 ('swapresults (alignments)', [t, q, tmp + '/aln_swapped', tmp + '/result', '-e', '0.001']))

        def rows(db):
            with open(db, 'rb') as f:
                return f.read().count(b'\n')
        for r in range(runs):
            total = 0.0
            for name, args in steps:
                t0 = time.time()
                subprocess.check_call([sdgpu, name.split()[0]] + args + common)
                dt = time.time() - t0
                total += dt
                log('search run %d: %-28s %.3f s' % (r + 1, name, dt))
            log('search run %d: the four steps                 %.3f s (%d prefilter rows, %d aligned, %d after the second swap)'
                % (r + 1, total, rows(tmp + '/pref'), rows(tmp + '/aln_swapped'), rows(tmp + '/result')))
            t0 = time.time()
            subprocess.check_call([sdgpu, 'search', q, t, tmp + '/result_search', tmp + '/tmp', '-e', '0.001'] + pref + common)
            log('search run %d: sdgpu search                   %.3f s' % (r + 1, time.time() - t0))
            same = all(open(tmp + '/result' + x, 'rb').read() == open(tmp + '/result_search' + x, 'rb').read() for x in ('', '.index'))
            log('search run %d: `search` wrote the bytes of the four steps: %s' % (r + 1, same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('-k', type=int, default=6, help='k-mer size of the index and of the search: 5 or 6')
    ap.add_argument('--positions', type=int, default=1000000)
    ap.add_argument('--queries', type=int, default=8192)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--sensitivity', type=float, default=4.0)
    ap.add_argument('--out', default=None)
    ap.add_argument('--search', action='store_true', help='also time the target-profile search on DBs (four modules, then `search`)')
    a = ap.parse_args()
    from spacedust_amd import api
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    host, gpu = api.Host(), api.Context(0)
    d = np.load(GOLD)
    reps = max(1, round(a.positions / (int(d['poff'][-1]) // 25)))
    data = d['profiles'].tobytes() * reps
    one = d['poff'].astype(np.uint64)
    poff = np.concatenate([[0], (one[1:][None, :] + (np.arange(reps, dtype=np.uint64) * one[-1])[:, None]).reshape(-1)]).astype(np.uint64)
    prof = host.map_profiles(data, poff)
    thr = host.profile_kmer_threshold(a.sensitivity, a.k)
    n_prof, n_pos = len(poff) - 1, int(prof['offsets'][-1])
    log('device: %s' % gpu.device_name())
    log('target: set G x %d = %d profiles, %d positions; k = %d, profile threshold %d (-s %.1f)' % (reps, n_prof, n_pos, a.k, thr, a.sensitivity))
    times, t = [], None
    for r in range(a.runs + 1):
        del t
        t0 = time.time()
        t = api.Target.build_profile_on_device(gpu, host, prof, k=a.k, kmer_thr=thr)
        dt = time.time() - t0
        if r:
            times.append(dt)
        log('build %s: %.3f s' % ('warm-up' if r == 0 else 'run %d' % r, dt))
    st, med = t.build_stats, float(np.median(times))
    log('sd_target_build_profile (upload of the mapped profiles included): median %.3f s of %d runs; %d records, %d entries, %d pass(es); '
        '%.3g records/s, %.3g entries/s; sd_target_build_peak %d B (%.2f GiB)'
        % (med, len(times), st['records'], st['entries'], st['passes'], st['records'] / med, st['entries'] / med, t.build_peak(), t.build_peak() / 2.0 ** 30))
    off = d['off'].astype(np.int64)
    blob = d['blob'].tobytes().decode()
    base = [blob[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    seqs = [base[i % len(base)] for i in range(a.queries)]
    res, qoff = host.map_sequences(seqs)
    _, dg_b, km_b = host.comp_bias(res, qoff, a.k)
    par = api.prefilter_params(host, n_prof, kmer_thr=thr, max_hits=300, cov_mode=0, cov_thr=0.0, k=a.k)
    ident = np.full(len(seqs), 0xFFFFFFFF, np.uint32)
    times = []
    for r in range(a.runs + 1):
        t0 = time.time()
        hits, cnt, stats = api.prefilter(gpu, t, par, res, qoff, km_b, dg_b, ident, want_stats=True)
        dt = time.time() - t0
        if r:
            times.append(dt)
        log('prefilter %s: %.3f s' % ('warm-up' if r == 0 else 'run %d' % r, dt))
    med = float(np.median(times))
    log('sd_prefilter_batch, %d sequence queries (%d residues) against it: median %.3f s of %d runs; %d exact k-mers looked up, %d index hits, '
        '%d rows; %.3g queries/s'
        % (len(seqs), int(qoff[-1]), med, len(times), int(stats[:, 0].sum()), int(stats[:, 1].sum()), int(cnt.sum()), len(seqs) / med))
    if a.search:
        del t
        search_leg(log, data, poff, seqs, a.sensitivity, a.runs, a.k)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
