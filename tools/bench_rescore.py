"""Micro-benchmark of the rescoring on the diagonal (sd_rescore.hip) on a prefilter hit list, next to the Smith-Waterman alignment
of the same list; bench.py is the judged entry point.

    python tools/bench_rescore.py [--proteomes 1000] [--queries 12000] [--reps 5] [--mem-gbs 0] [--out profiles/rescore_diagonal.txt]

The hit list is the k-mer prefilter's (clustersearch parameters: -s 5.7, --max-seqs 300, -c 0.8 --cov-mode 2) for the first
--queries proteins of the synthetic proteomes bench.py searches.  One warm-up call, then --reps timed calls of each leg: median and
spread of the kernel time (HIP events around the launches) and of the wall time of the whole call.  Bytes at the memory side, as
DESIGN 4.9 counts them: per hit 10 bytes of hit, four u64 offsets and 32 bytes of result (74), and per overlapping candidate
diagonal the letters of both sides plus the 7 bytes a side's last aligned dword pair can reach past them.
--mem-gbs: the sequential-read figure of tools/fetch_calib.py on the same box, for the fraction.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from spacedust_amd.synth import make_proteomes   # noqa: E402


def main(a):
    from spacedust_amd import api
    from spacedust_amd.api import Host, Context
    import rescore_ref as rr
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
    n = len(hq)
    lens = ps.lengths().astype(np.int64)
    say('%d proteomes, %d targets (%d residues), %d queries, %d prefilter hits' % (a.proteomes, ps.n, int(ps.offsets[-1]), nq, n))
    # positions and bytes of the overlapping candidates (sequences here are below 32 768 residues: d16 - 65536 and d16)
    d = hd.astype(np.int64)
    ql, tl = lens[hq], lens[ht]
    pos, cands = np.zeros(n, np.int64), 0
    for diag in (d - 65536, d):
        dist = np.abs(diag)
        ln = np.where((diag >= 0) & (dist < ql), np.minimum(tl, ql - dist), np.where((diag < 0) & (dist < tl), np.minimum(tl - dist, ql), 0))
        pos += ln
        cands += int((ln > 0).sum())
    byts = 2 * pos.sum() + 14 * cands + 74 * n
    alphabet = np.frombuffer(rr.ALPHABET.encode(), np.uint8)
    t_set = gpu.seqset(ps.residues, ps.offsets, None)
    t_set.set_letters(alphabet[ps.residues])
    q_set = gpu.seqset(q_res, q_off, sw_b)
    q_set.set_letters(alphabet[q_res])

    def timed(fn, names):
        fn()   # warm-up
        kern, wall = [], []
        for _ in range(a.reps):
            gpu.L.sd_profile_reset(gpu.h)
            gpu.profile(True)
            t0 = time.time()
            fn()
            wall.append(time.time() - t0)
            rep = gpu.profile_report()
            kern.append(sum(v[0] for key, v in rep.items() if not key.startswith('host:') and (names is None or key in names)) / 1e3)
        gpu.profile(False)
        return np.array(kern), np.array(wall)
    rk, rw = timed(lambda: gpu.rescore_diagonal(host, q_set, t_set, hq, ht, hd, mode=2), ('rescore_diagonal',))
    med = float(np.median(rk))
    say('rescore  kernel median %.2f ms (min %.2f, max %.2f, n=%d); whole call median %.1f ms (min %.1f, max %.1f)' % (
        med * 1e3, rk.min() * 1e3, rk.max() * 1e3, len(rk), np.median(rw) * 1e3, rw.min() * 1e3, rw.max() * 1e3))
    say('         %.1f Mhits/s, %.2f Gpositions/s, %.1f GB/s at the memory side (%.0f positions and %.0f bytes per hit)' % (
        n / med / 1e6, pos.sum() / med / 1e9, byts / med / 1e9, pos.sum() / max(n, 1), byts / max(n, 1)))
    if a.mem_gbs > 0:
        say('         %.1f %% of the sequential-read figure of %.0f GB/s' % (100.0 * byts / med / 1e9 / a.mem_gbs, a.mem_gbs))
    sw_par = gpu.sw_params(host.matrix(0)[0], int(ps.offsets[-1]))
    ident = (hq == ht).astype(np.uint8)
    ak, aw = timed(lambda: gpu.sw_align(sw_par, q_set, t_set, hq, ht, identity=ident), None)
    say('align    kernels median %.1f ms (min %.1f, max %.1f); whole call median %.1f ms (min %.1f, max %.1f)' % (
        np.median(ak) * 1e3, ak.min() * 1e3, ak.max() * 1e3, np.median(aw) * 1e3, aw.min() * 1e3, aw.max() * 1e3))
    say('align / rescore: %.1f x in device time, %.1f x in wall time of the call' % (np.median(ak) / med, np.median(aw) / np.median(rw)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('tools/bench_rescore.py --proteomes %d --queries %d --reps %d\n' % (a.proteomes, a.queries, a.reps) + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--proteomes', type=int, default=1000)
    ap.add_argument('--queries', type=int, default=12000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--mem-gbs', type=float, default=0.0)
    ap.add_argument('--out', default='')
    main(ap.parse_args())
