#!/usr/bin/env python3
"""What `--target-search-mode 1` costs and saves on the device, on one input: N synthetic proteomes (spacedust_amd.synth) as the
target, indexed by sd_target_build_similar at the default sequence threshold (Host.kmer_threshold(5.7, 6)), then 8 192 of their
proteins as queries through sd_prefilter_batch -- against the regular index (sd_target_build, mode 0) and its similar-k-mer queries on
the same input.  Every timed call ends in a device synchronise inside the library; the first build and the first query pass of
either mode are warm-up, the figures are medians of the runs after it.

    python tools/bench_target_similar.py [--proteomes 2] [--queries 8192] [--runs 3] [--mode both|0|1] [--out FILE]
    python tools/bench_target_similar.py --package-root DIR --mode 0     (the mode-0 legs with the package of another checkout, e.g.
                                                                          the parent commit built in DIR)
    python tools/bench_target_similar.py --build-only --proteomes 1 --runs 1      (one build after the warm-up: the profiler's input)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--proteomes', type=int, default=2)
    ap.add_argument('--genes', type=int, default=3000)
    ap.add_argument('--queries', type=int, default=8192)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--sensitivity', type=float, default=5.7)
    ap.add_argument('--mode', default='both', choices=['both', '0', '1'])
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--package-root', default=ROOT)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from spacedust_amd import api
    from spacedust_amd.synth import make_proteomes
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    host, gpu = api.Host(), api.Context(0)
    ps = make_proteomes(a.proteomes, genes_per_proteome=a.genes, n_families=2 * a.genes, seed=7)
    res, off = np.ascontiguousarray(ps.residues, np.uint8), np.ascontiguousarray(ps.offsets, np.uint64)
    n_t, n_res = len(off) - 1, int(off[-1])
    thr = host.kmer_threshold(a.sensitivity, 6)
    log('device: %s; package: %s' % (gpu.device_name(), os.path.abspath(a.package_root)))
    log('target: %d synthetic proteomes = %d proteins, %d residues; k = 6, sequence threshold %d (-s %.1f)' % (a.proteomes, n_t, n_res, thr, a.sensitivity))
    nq = min(a.queries, n_t)
    q_res, q_off = res[:int(off[nq])], off[:nq + 1]
    _, dg_b, km_b = host.comp_bias(q_res, q_off)
    ident = np.full(nq, 0xFFFFFFFF, np.uint32)
    par = api.prefilter_params(host, n_t, kmer_thr=thr, max_hits=300, cov_mode=0, cov_thr=0.0, k=6)
    for mode in ('1', '0'):
        if a.mode not in ('both', mode):
            continue
        name = 'sd_target_build_similar (mode 1)' if mode == '1' else 'sd_target_build (mode 0, tantan masking included)'
        times, t = [], None
        for r in range(a.runs + 1):
            del t
            t0 = time.time()
            if mode == '1':
                t = api.Target.build_similar_on_device(gpu, host, res, off, k=6, kmer_thr=thr)
            else:
                t = api.Target.build_on_device(gpu, host, res, off, k=6, kmer_thr=thr, mask=True, mask_prob=0.9)
            dt = time.time() - t0
            if r:
                times.append(dt)
            log('mode %s build %s: %.3f s' % (mode, 'warm-up' if r == 0 else 'run %d' % r, dt))
        st, med = t.build_stats, float(np.median(times))
        log('%s, upload included: median %.3f s of %d runs; %d records, %d entries, %d pass(es); %.1f records and %.1f entries per residue; '
            '%.3g records/s; sd_target_build_peak %d B (%.2f GiB)'
            % (name, med, len(times), st['records'], st['entries'], st['passes'], st['records'] / float(n_res), st['entries'] / float(n_res),
               st['records'] / med, t.build_peak(), t.build_peak() / 2.0 ** 30))
        if a.build_only:
            continue
        times = []
        for r in range(a.runs + 1):
            t0 = time.time()
            hits, cnt, stats = api.prefilter(gpu, t, par, q_res, q_off, km_b, dg_b, ident, want_stats=True)
            dt = time.time() - t0
            if r:
                times.append(dt)
            log('mode %s prefilter %s: %.3f s' % (mode, 'warm-up' if r == 0 else 'run %d' % r, dt))
        med = float(np.median(times))
        log('sd_prefilter_batch mode %s, %d queries (%d residues): median %.3f s of %d runs; %d k-mers looked up, %d index hits, %d rows; %.3g queries/s'
            % (mode, nq, int(q_off[-1]), med, len(times), int(stats[:, 0].sum()), int(stats[:, 1].sum()), int(cnt.sum()), nq / med))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
