"""Micro-benchmark of the alternative alignments (sd_sw_alt.hip, sd_sw_align_alt_batch) on the accepted alignments of a prefilter
hit list, next to the primary alignment pass of the same list; bench.py is the judged entry point.

    python tools/bench_altali.py [--proteomes 100] [--queries 12000] [--reps 3] [--out profiles/alt_ali.txt]

The hit list is the one tools/bench_rescore.py uses (clustersearch parameters).  The primary pass is
sd_sw_align_batch_compact_diag; its accepted, non-identity records (E-value, query coverage 0.8) are the seeds.  One warm-up call,
then --reps timed calls of each leg: device time (HIP events around every launch) and wall time of the call, and of the device
time the share of the kernels between the rounds (mask / copy, accept / compaction) with the bytes they wrote.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spacedust_amd.synth import make_proteomes   # noqa: E402


def main(a):
    from spacedust_amd import api
    from spacedust_amd.api import Host, Context
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ps = make_proteomes(a.proteomes, genes_per_proteome=3000, seed=21)
    host, gpu = Host(), Context(0)
    say(gpu.device_name())
    nq = min(a.queries, ps.n)
    k = host.auto_kmer_size(int(ps.offsets[-1]))
    thr = host.kmer_threshold(5.7, k)
    target = api.Target.build_on_device(gpu, host, ps.residues, ps.offsets, k=k, kmer_thr=thr)
    q_off = ps.offsets[:nq + 1].copy()
    q_res = ps.residues[:int(q_off[-1])]
    sw_b, dg_b, km_b = host.comp_bias(q_res, q_off, k)
    par = api.prefilter_params(host, ps.n, kmer_thr=thr, max_hits=300, k=k)
    hits, cnt, _ = api.prefilter(gpu, target, par, q_res, q_off, km_b, dg_b, np.arange(nq, dtype=np.uint32))
    del target
    gpu.L.sd_workspace_release(gpu.h)
    hq = np.repeat(np.arange(nq, dtype=np.uint32), cnt)
    row = np.concatenate([np.arange(c) for c in cnt]) if len(hq) else np.zeros(0, np.int64)
    ht, hd = hits[hq, row]['seqId'].astype(np.uint32), hits[hq, row]['diagonal'].astype(np.uint16)
    lens = ps.lengths().astype(np.int64)
    t_set = gpu.seqset(ps.residues, ps.offsets, None)
    q_set = gpu.seqset(q_res, q_off, sw_b)
    sw_par = gpu.sw_params(host.matrix(0)[0], int(ps.offsets[-1]))   # swMode 2, -e 10, -c 0.8 --cov-mode 2
    ident = (hq == ht).astype(np.uint8)
    say('%d proteomes, %d targets (%d residues), %d queries, %d prefilter hits' % (a.proteomes, ps.n, int(ps.offsets[-1]), nq, len(hq)))

    def timed(fn):
        fn()   # warm-up
        rows = []
        for _ in range(a.reps):
            gpu.L.sd_profile_reset(gpu.h)
            gpu.profile(True)
            t0 = time.time()
            fn()
            wall = time.time() - t0
            rep = gpu.profile_report()
            dev = sum(v[0] for key, v in rep.items() if not key.startswith('host:')) / 1e3
            alt = sum(v[0] for key, v in rep.items() if key.startswith('alt_')) / 1e3
            rows.append((dev, wall, alt))
        gpu.profile(False)
        return np.array(rows)
    primary = {}

    def run_primary():
        primary['out'] = gpu.sw_align(sw_par, q_set, t_set, hq, ht, identity=ident, compact=True, diag=hd)
    p = timed(run_primary)
    idx, rec, _ = primary['out']
    keep = (ident[idx] == 0) & (rec['btLen'] > 0) & (rec['evalue'] <= 10.0)
    sq, st = hq[idx][keep], ht[idx][keep]
    tb, te = rec['tStart'][keep], rec['tEnd'][keep]
    say('primary  %d pairs: device median %.1f ms (min %.1f, max %.1f), wall median %.1f ms; %.3f us of device time per pair' % (
        len(hq), np.median(p[:, 0]) * 1e3, p[:, 0].min() * 1e3, p[:, 0].max() * 1e3, np.median(p[:, 1]) * 1e3, np.median(p[:, 0]) * 1e6 / len(hq)))
    say('seeds    %d accepted non-identity alignments, %.0f target residues per seed' % (len(sq), lens[st].mean() if len(sq) else 0))
    for n in (1, 3):
        r = timed(lambda: gpu.sw_align_alt(sw_par, q_set, t_set, sq, st, tb, te, n))
        groups, seed_rounds, copied = gpu.sw_alt_stats()
        dev, wall, alt = np.median(r[:, 0]), np.median(r[:, 1]), np.median(r[:, 2])
        say('alt N=%d  device median %.1f ms (min %.1f, max %.1f), wall median %.1f ms; %d groups, %d alignments: %.3f us of device time each' % (
            n, dev * 1e3, r[:, 0].min() * 1e3, r[:, 0].max() * 1e3, wall * 1e3, groups, seed_rounds, dev * 1e6 / max(seed_rounds, 1)))
        say('         mask / accept / compaction kernels %.2f ms = %.1f %% of the device time; %d bytes written into the scratch set' % (
            alt * 1e3, 100.0 * alt / max(dev, 1e-12), copied))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('tools/bench_altali.py --proteomes %d --queries %d --reps %d\n' % (a.proteomes, a.queries, a.reps) + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--proteomes', type=int, default=100)
    ap.add_argument('--queries', type=int, default=12000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default='')
    main(ap.parse_args())
