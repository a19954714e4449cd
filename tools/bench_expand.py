#!/usr/bin/env python3
"""What `expandaln` costs, on the input of tools/bench_target_profile.py --search: set G of tests/golden/profile_vectors.npz repeated to
about 10^6 positions (3 546 profiles) and 8 192 sequence queries.  `sdgpu search` of the sequences against the profiles gives the
A -> B alignment DB; the B -> C DB is cut from the search's own profile -> sequence alignments (<tmp>/aln_swapped, rows with backtrace):
the first --cluster-size rows of every profile are its cluster's members.  Then `sdgpu expandaln` runs --runs + 1 times (the first is
warm-up) with SD_DEBUG_TIMING=1, which makes the module report its wall time by stage and the two kernels' times from sd_profile_get.

    python tools/bench_expand.py [--positions 1000000] [--queries 8192] [--cluster-size 8] [--runs 3] [--out profiles/expandaln.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_target_profile import GOLD, write_db  # noqa: E402


def read_db(path):
    data = open(path, 'rb').read()
    out = {}
    for line in open(path + '.index'):
        k, o, l = line.split()
        out[int(k)] = data[int(o):int(o) + int(l) - 1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--positions', type=int, default=1000000)
    ap.add_argument('--queries', type=int, default=8192)
    ap.add_argument('--cluster-size', type=int, default=8)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--sensitivity', type=float, default=4.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    sdgpu = os.path.join(ROOT, 'spacedust_amd', 'sdgpu')
    threads = str(min(16, os.cpu_count() or 1))
    d = np.load(GOLD)
    reps = max(1, round(a.positions / (int(d['poff'][-1]) // 25)))
    one = d['poff'].astype(np.int64)
    profiles = [d['profiles'].tobytes()[one[i]:one[i + 1]] for i in range(len(one) - 1)] * reps
    off = d['off'].astype(np.int64)
    blob = d['blob'].tobytes().decode()
    base = [blob[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    seqs = [base[i % len(base)] for i in range(a.queries)]
    common = ['--threads', threads, '-v', '0']
    pref = ['-s', str(a.sensitivity), '--max-seqs', '300', '-c', '0', '--cov-mode', '0', '--comp-bias-corr', '1', '--min-ungapped-score', '15']
    with tempfile.TemporaryDirectory() as tmp:
        q, t = os.path.join(tmp, 'seq'), os.path.join(tmp, 'prof')
        write_db(q, [s.encode() + b'\n' for s in seqs], 0)
        write_db(t, profiles, 2)
        log('input: %d profiles (set G x %d), %d sequence queries; %s threads' % (len(profiles), reps, len(seqs), threads))
        t_search = []
        for r in range(a.runs + 1):
            t0 = time.time()
            subprocess.check_call([sdgpu, 'search', q, t, tmp + '/result', tmp + '/tmp', '-e', '0.001', '--keep-tmp', '1'] + pref + common)
            dt = time.time() - t0
            if r:
                t_search.append(dt)
            log('sdgpu search %s: %.3f s' % ('warm-up' if r == 0 else 'run %d' % r, dt))
        listed = read_db(tmp + '/tmp/aln_swapped')
        bc = {k: b''.join(text.splitlines(keepends=True)[:a.cluster_size]) for k, text in listed.items()}
        members = sum(x.count(b'\n') for x in bc.values())
        bc_file = tmp + '/clu_aln'
        with open(bc_file, 'wb') as f, open(bc_file + '.index', 'w') as ix:
            at = 0
            for k in sorted(bc):
                f.write(bc[k] + b'\0')
                ix.write('%d\t%d\t%d\n' % (k, at, len(bc[k]) + 1))
                at += len(bc[k]) + 1
        open(bc_file + '.dbtype', 'wb').write(b'\x05\x00\x00\x00')
        ab_rows = open(tmp + '/result', 'rb').read().count(b'\n')
        log('A -> B: %d rows in %d entries; B -> C: %d clusters, %d members (mean cluster size %.2f, at most %d)'
            % (ab_rows, len(seqs), len(bc), members, members / max(1, len(bc)), a.cluster_size))
        stats = []
        for r in range(a.runs + 1):
            t0 = time.time()
            p = subprocess.run([sdgpu, 'expandaln', q, q, tmp + '/result', bc_file, tmp + '/expanded'] + common, env=dict(os.environ, SD_DEBUG_TIMING='1'),
                               stderr=subprocess.PIPE, text=True, check=True)
            dt = time.time() - t0
            m1 = re.search(r'parse ([\d.]+) s, device ([\d.]+) s, select ([\d.]+) s, print ([\d.]+) s', p.stderr)
            m2 = re.search(r'(\d+) calls, (\d+) pairs, (\d+) kept; kernels: expand_records ([\d.]+) ms, expand_text ([\d.]+) ms; (\d+) runs read, (\d+) bytes written',
                           p.stderr)
            row = [dt] + [float(x) for x in m1.groups()] + [float(x) for x in m2.groups()]
            if r:
                stats.append(row)
            log('sdgpu expandaln %s: %.3f s wall; parse %.3f, device (copies + kernels) %.3f, select %.3f, print + write %.3f s; kernels: pass 1 %.3f ms, '
                'pass 2 %.3f ms' % (('warm-up' if r == 0 else 'run %d' % r,) + tuple(row[:5]) + (row[8], row[9])))
        med = np.median(np.array(stats), axis=0)
        calls, pairs, kept, ms1, ms2, runs_read, written = med[5:12]
        out_rows = open(tmp + '/expanded', 'rb').read().count(b'\n')
        log('medians of %d runs: expandaln %.3f s wall (parse %.3f, device %.3f, select %.3f, print + write %.3f)' % ((len(stats),) + tuple(med[:5])))
        log('%d pairs in %d device calls, %d rows kept (%d rows in the output DB)' % (pairs, calls, kept, out_rows))
        rec_bytes = 48.0
        log('pass 1 (expand_records): %.3f ms = %.2f ns per pair; run lists of %.1f words = %.0f B per pair (counted on the host, not measured traffic: the lanes of '
            'a cluster share their AB row), %.0f B of record written per pair: %.1f GB/s of runs named, %.1f GB/s of records written'
            % (ms1, ms1 * 1e6 / pairs, runs_read / pairs, 4.0 * runs_read / pairs, rec_bytes, 4.0 * runs_read / ms1 / 1e6, rec_bytes * pairs / ms1 / 1e6))
        text_bytes = written - rec_bytes * pairs
        log('pass 2 (expand_text): %.3f ms = %.2f ns per kept pair; %.1f B of text per kept pair' % (ms2, ms2 * 1e6 / max(1, kept), text_bytes / max(1, kept)))
        log('kernels are %.2f %% of the module\'s wall time; the host stages (parse + select + print) %.0f %%'
            % (100.0 * (ms1 + ms2) / 1e3 / med[0], 100.0 * (med[1] + med[3] + med[4]) / med[0]))
        ts = float(np.median(t_search))
        log('sdgpu search alone: median %.3f s; search + expandaln: %.3f s (x %.2f)' % (ts, ts + med[0], (ts + med[0]) / ts))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
