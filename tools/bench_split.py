#!/usr/bin/env python3
"""What a target split costs (`sdgpu prefilter --split N --split-mode 0`): a synthetic target set that fits in one split (default
1 000 proteomes of spacedust_amd/synth.py, 3 * 10^6 proteins), the first Q proteomes as queries, the module run at --split 1, 2
and 4, three runs each.  Per run the wall time of the process and its split into index builds, query passes and merge, from the
module's own Lap marks (SD_DEBUG_TIMING=1).  A split run's result differs from the unsplit one by definition (shorter per-split
lists, uncut merge), so only times are compared; tests/test_gpu_split.py checks the rows.  Also prints sd_target_footprint against
the peak sd_target_build observed for the whole target.

    python tools/bench_split.py [--proteomes 1000] [--queries 20] [--splits 1,2,4] [--runs 3] [--out profiles/split_prefilter.txt]"""
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
SDGPU = os.path.join(ROOT, 'spacedust_amd', 'sdgpu')


def write_seq_db(path, ps, first_set, last_set):
    """the proteins of proteomes [first_set, last_set) as an amino-acid DB: key = index, entries 'SEQUENCE\\n\\0'"""
    from spacedust_amd.synth import ALPHABET
    lut = np.frombuffer(ALPHABET.encode(), np.uint8)
    a, e = int(ps.set_start[first_set]), int(ps.set_start[last_set])
    lens = ps.lengths()[a:e]
    with open(path, 'wb') as f:
        for s in range(first_set, last_set):          # one proteome at a time: a few MB of index arithmetic each
            p0, p1 = int(ps.set_start[s]), int(ps.set_start[s + 1])
            r0, r1 = int(ps.offsets[p0]), int(ps.offsets[p1])
            l = lens[p0 - a:p1 - a]
            out = np.zeros(r1 - r0 + 2 * len(l), np.uint8)
            dst = np.arange(r1 - r0) + np.repeat(2 * np.arange(len(l)), l)
            out[dst] = lut[ps.residues[r0:r1]]
            ends = np.cumsum(l + 2)
            out[ends - 2] = ord('\n')
            f.write(out.tobytes())
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens + 2, out=off[1:])
    with open(path + '.index', 'w') as f:
        f.write(''.join('%d\t%d\t%d\n' % (i, off[i], lens[i] + 2) for i in range(len(lens))))
    with open(path + '.dbtype', 'wb') as f:
        f.write((0).to_bytes(4, 'little'))


def laps(stderr):
    """'[prefilter] what X s' lines summed by what"""
    out = {}
    for m in re.finditer(r'^\[prefilter\] (.*) ([0-9.]+) s$', stderr, re.M):
        out[m.group(1)] = out.get(m.group(1), 0.0) + float(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--proteomes', type=int, default=1000)
    ap.add_argument('--queries', type=int, default=20, help='query proteomes (the first ones of the target set)')
    ap.add_argument('--splits', default='1,2,4')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--threads', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from spacedust_amd import api
    from spacedust_amd.cpus import effective_cpus
    from spacedust_amd.synth import make_proteomes
    threads = a.threads or effective_cpus()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    work = tempfile.mkdtemp(prefix='sd_split_')
    t0 = time.time()
    ps = make_proteomes(a.proteomes, genes_per_proteome=3000, seed=0x5ED0 + 2)
    print('generated %d proteins in %.0f s' % (ps.n, time.time() - t0), flush=True)
    T, Q = os.path.join(work, 'T'), os.path.join(work, 'Q')
    write_seq_db(T, ps, 0, a.proteomes)
    write_seq_db(Q, ps, 0, a.queries)
    nq = int(ps.set_start[a.queries])
    log('target: %d proteomes, %d proteins, %d residues; queries: %d proteins of the first %d proteomes (generated and written in %.0f s)'
        % (a.proteomes, ps.n, int(ps.offsets[-1]), nq, a.queries, time.time() - t0))
    flags = ['-s', '5.7', '-c', '0.8', '--cov-mode', '2', '--max-seqs', '300', '--threads', str(threads), '-v', '3']
    log('command: sdgpu prefilter Q T out --split N --split-mode 0 ' + ' '.join(flags) + '   (SD_DEBUG_TIMING=1)')
    env = dict(os.environ, SD_DEBUG_TIMING='1')
    base = None
    for n in [int(x) for x in a.splits.split(',')]:
        rows = []
        for r in range(a.runs):
            out = os.path.join(work, 'out_%d_%d' % (n, r))
            t0 = time.time()
            p = subprocess.run([SDGPU, 'prefilter', Q, T, out, '--split', str(n), '--split-mode', '0'] + flags, env=env, capture_output=True, text=True)
            wall = time.time() - t0
            if p.returncode != 0:
                raise RuntimeError('sdgpu prefilter --split %d failed: %s' % (n, p.stderr[-600:]))
            l = laps(p.stderr)
            build = l.get('split: index build', 0.0) + l.get('target index', 0.0)
            query = l.get('split: query passes', 0.0) + l.get('chunk: bias + device', 0.0)
            merge = l.get('merge + write', 0.0) + l.get('chunks: text + write', 0.0) + l.get('close', 0.0)
            hits = int(re.search(r'(\d+) prefilter hits written', p.stdout).group(1))
            rows.append((wall, l.get('load DBs', 0.0), l.get('context', 0.0), build, query, merge, hits))
            log('--split %d run %d: wall %.2f s | load DBs %.2f | context %.2f | index builds %.2f | query passes %.2f | merge + write %.2f | %d hits'
                % ((n, r) + rows[-1]))
            for f in (out, out + '.index', out + '.dbtype'):
                os.remove(f)
        med = [float(np.median([x[i] for x in rows])) for i in range(6)]
        if base is None:
            base = med
        log('--split %d median: wall %.2f s, index builds %.2f s, query passes %.2f s, merge + write %.2f s; against --split %s: wall %+.2f s '
            '(%+.2f s per added split), index builds %+.2f s, query passes %+.2f s'
            % (n, med[0], med[3], med[4], med[5], a.splits.split(',')[0], med[0] - base[0], (med[0] - base[0]) / max(n - 1, 1), med[3] - base[3],
               med[4] - base[4]))
    # the footprint model against the build of the whole target
    host, gpu = api.Host(), api.Context(0)
    t = api.Target.build_on_device(gpu, host, ps.residues, ps.offsets, k=6, kmer_thr=host.kmer_threshold(5.7, 6))
    est, peak = api.target_footprint(6, ps.n, int(ps.offsets[-1])), t.build_peak()
    log('sd_target_footprint(6, %d, %d) = %d B; sd_target_build held %d B at its peak (%d entries); estimate / observed %.3f; device: %s'
        % (ps.n, int(ps.offsets[-1]), est, peak, t.build_stats['entries'], est / max(peak, 1), gpu.device_name()))
    del t
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    os.rmdir(work)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
