#!/usr/bin/env python3
"""What `sdgpu clust` costs, stage by stage, on the all-vs-all alignment DB of bench.py's synthetic proteomes (100 by default: 300 000
proteins): `sdgpu createsetdb` and `sdgpu search` of the set against itself make the result DB; `sdgpu clust` then runs --runs + 1 times
(the first is warm-up) with SD_DEBUG_TIMING=1, which makes the module report its wall time by stage and the device call's copy-in, kernel
and copy-out times.  --dump-graph FILE also writes the parsed graph (lengths, rows, identity column) for tools/make_golden_clust.py
--time-graph FILE, which times the reference's own readInClusterData / execute on the same lists where the reference tree is.

    python tools/bench_clust.py [--proteomes 100] [--runs 3] [--out profiles/clust.txt] [--dump-graph clust_graph.npz]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--proteomes', type=int, default=100)
    ap.add_argument('--genes', type=int, default=3000)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dump-graph', default=None)
    a = ap.parse_args()
    from iter3_scale import _write_fasta
    from spacedust_amd.synth import ALPHABET, make_proteomes
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    sdgpu = os.path.join(ROOT, 'spacedust_amd', 'sdgpu')
    threads = str(min(16, os.cpu_count() or 1))
    common = ['--threads', threads, '-v', '0']
    ps = make_proteomes(a.proteomes, genes_per_proteome=a.genes, seed=0x5ED0 + 2, workers=1)
    lut = np.frombuffer(ALPHABET.encode(), np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(tmp + '/fa')
        files = [_write_fasta(ps, s, tmp + '/fa', lut) for s in range(a.proteomes)]
        t = tmp + '/t'
        subprocess.check_call([sdgpu, 'createsetdb'] + files + [t, tmp + '/tmp', '-v', '0'])
        t0 = time.time()
        subprocess.check_call([sdgpu, 'search', t, t, tmp + '/aln', tmp + '/search', '-s', '5.7', '--max-seqs', '300', '-e', '0.001', '-c', '0.8',
                               '--cov-mode', '0', '--alignment-mode', '3'] + common)
        rows = 0
        with open(tmp + '/aln', 'rb') as f:
            for block in iter(lambda: f.read(1 << 24), b''):
                rows += block.count(b'\n')
        log('input: %d proteomes, %d proteins; all-vs-all `sdgpu search` (-s 5.7 --max-seqs 300 -e 0.001 -c 0.8): %d alignment rows, %.1f MB, in %.1f s; %s threads'
            % (a.proteomes, ps.n, rows, os.path.getsize(tmp + '/aln') / 1e6, time.time() - t0, threads))
        pat = re.compile(r'\[clust\] (.+?) ([\d.]+) s$', re.M)
        dev = re.compile(r'copy in ([\d.]+) ms, kernels ([\d.]+) ms, copy out ([\d.]+) ms; (\d+) entries in, (\d+) added, largest row (\d+)')
        for mode in (0, 1, 2):
            stats = []
            for r in range(a.runs + 1 if mode == 0 else 2):
                t0 = time.time()
                p = subprocess.run([sdgpu, 'clust', t, tmp + '/aln', tmp + '/clu', '--cluster-mode', str(mode)] + common,
                                   env=dict(os.environ, SD_DEBUG_TIMING='1'), stderr=subprocess.PIPE, text=True, check=True)
                wall = time.time() - t0
                st = {k: float(v) for k, v in pat.findall(p.stderr)}
                m = dev.search(p.stderr)
                d = [float(x) for x in m.groups()] if m else [0.0] * 6
                if r:
                    stats.append([wall, st.get('open DBs', 0), st.get('parse', 0), st.get('context', 0), st.get('symmetric graph', 0), st.get('algorithm', 0),
                                  st.get('write', 0)] + d)
                if mode == 0:
                    log('sdgpu clust --cluster-mode 0 %s: %.3f s wall; open %.3f, parse %.3f, context %.3f, symmetric graph %.3f (copy in %.1f ms, kernels %.1f ms, '
                        'copy out %.1f ms), algorithm %.3f, write %.3f s'
                        % ('warm-up' if r == 0 else 'run %d' % r, wall, st.get('open DBs', 0), st.get('parse', 0), st.get('context', 0),
                           st.get('symmetric graph', 0), d[0], d[1], d[2], st.get('algorithm', 0), st.get('write', 0)))
            med = np.median(np.array(stats), axis=0)
            clusters = sum(1 for _ in open(tmp + '/clu.index'))
            log('--cluster-mode %d, median of %d: %.3f s wall; open %.3f, parse %.3f, context %.3f, symmetric graph %.3f, algorithm %.3f, write %.3f s; %d clusters'
                % ((mode, len(stats)) + tuple(med[:7]) + (clusters,)))
            if mode == 0:
                e_in, added, largest = int(med[10]), int(med[11]), int(med[12])
                log('device stage: %d entries in, %d added, largest row %d; copy in %.2f ms, kernels %.2f ms, copy out %.2f ms: %.0f M entries/s through the '
                    'kernels, %.0f M entries/s with the copies' % (e_in, added, largest, med[7], med[8], med[9], e_in / med[8] / 1e3, e_in / (med[7] + med[8] + med[9]) / 1e3))
                log('the device stage (copies + kernels) is %.1f %% of the module\'s wall time, parse %.1f %%, the set cover %.1f %%'
                    % (100 * (med[7] + med[8] + med[9]) / 1e3 / med[0], 100 * med[2] / med[0], 100 * med[5] / med[0]))
        if a.dump_graph:
            from spacedust_amd import api
            index = np.loadtxt(t + '.index', dtype=np.int64).reshape(-1, 3)
            keys, lens = index[:, 0].astype(np.uint32), index[:, 2].astype(np.uint64)
            data = open(tmp + '/aln', 'rb').read()
            aidx = np.loadtxt(tmp + '/aln.index', dtype=np.int64).reshape(-1, 3)
            entry = {int(k): data[int(o):int(o) + int(l) - 1] for k, o, l in aidx}
            order = api.clust_order(lens)
            off, elem, score = api.clust_parse(keys[order], [entry[int(k)] for k in keys[order]], 5, 2)
            os.makedirs(os.path.dirname(os.path.abspath(a.dump_graph)), exist_ok=True)
            np.savez_compressed(a.dump_graph, keys=keys, lens=lens.astype(np.uint32), order=order, off=off, elem=elem, score=score)
            log('graph written to %s (%.1f MB)' % (a.dump_graph, os.path.getsize(a.dump_graph) / 1e6))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
