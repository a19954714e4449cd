#!/usr/bin/env python3
"""What `sdgpu kmermatcher` costs, stage by stage, on bench.py's synthetic proteomes (100 by default: 300 000 proteins) at the module's
defaults: the sequence DB is written here, then the module runs --runs + 1 times (the first is warm-up) with SD_DEBUG_TIMING=1, which makes
it report its wall time by stage and the device call's times per stage (host preparation, first-use allocations, then copies and kernels each followed by a wait, so they add up to the call).  --dump FILE
also writes the sequences for tools/make_golden_kmermatch.py --time FILE THREADS, which times the reference's own doComputation and
writeKmerMatcherResult on them where the reference tree is.

    python tools/bench_kmermatcher.py [--proteomes 100] [--runs 3] [--out profiles/kmermatcher.txt] [--dump kmm_seqs.npz]
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


def write_seq_db(path, residues, offsets, alphabet):
    """a sequence DB (amino acids, keys 0 .. n - 1) from 21-letter codes"""
    offsets = np.asarray(offsets, np.int64)
    n, total = len(offsets) - 1, int(offsets[-1])
    lens = np.diff(offsets)
    data = np.zeros(total + 2 * n, np.uint8)
    lut = np.frombuffer(alphabet.encode(), np.uint8)
    data[np.arange(total) + 2 * np.repeat(np.arange(n), lens)] = lut[residues]
    data[offsets[1:] + 2 * np.arange(n)] = ord('\n')
    data.tofile(path)
    start = offsets[:-1] + 2 * np.arange(n)
    with open(path + '.index', 'w') as f:
        f.write(''.join('%d\t%d\t%d\n' % (i, s, l + 2) for i, (s, l) in enumerate(zip(start.tolist(), lens.tolist()))))
    with open(path + '.dbtype', 'wb') as f:
        f.write((0).to_bytes(4, 'little'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--proteomes', type=int, default=100)
    ap.add_argument('--genes', type=int, default=3000)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dump', default=None)
    a = ap.parse_args()
    from spacedust_amd.synth import ALPHABET, make_proteomes
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    sdgpu = os.path.join(ROOT, 'spacedust_amd', 'sdgpu')
    threads = str(min(16, os.cpu_count() or 1))
    ps = make_proteomes(a.proteomes, genes_per_proteome=a.genes, seed=0x5ED0 + 2, workers=1)
    if a.dump:
        os.makedirs(os.path.dirname(os.path.abspath(a.dump)), exist_ok=True)
        np.savez_compressed(a.dump, res=ps.residues, off=ps.offsets)
    stages = ['open', 'letter map', 'context', 'device', 'text and write']
    device = ['prepare', 'alloc', 'copy_in', 'records', 'sort1', 'group', 'sort2', 'hits', 'copy_out']
    pat = re.compile(r'\[kmermatcher\] (.+?) ([\d.]+) s$', re.M)
    dev = re.compile(r'\[kmermatcher\] device: (.*); (\d+) records, (\d+) grouped, (\d+) hits, largest group (\d+)')
    with tempfile.TemporaryDirectory() as tmp:
        db = tmp + '/seq'
        write_seq_db(db, ps.residues, ps.offsets, ALPHABET)
        log('input: %d proteomes, %d proteins, %d residues; `sdgpu kmermatcher` at its defaults; %s threads' % (a.proteomes, ps.n, int(ps.offsets[-1]), threads))
        rows = []
        for r in range(a.runs + 1):
            t0 = time.time()
            p = subprocess.run([sdgpu, 'kmermatcher', db, tmp + '/pref', '--threads', threads, '-v', '0'], env=dict(os.environ, SD_DEBUG_TIMING='1'),
                               stderr=subprocess.PIPE, text=True, check=True)
            wall = time.time() - t0
            st = {k: float(v) for k, v in pat.findall(p.stderr)}
            m = dev.search(p.stderr)
            ms = dict((k, float(v)) for k, v in re.findall(r'(\w+) ([\d.]+) ms', m.group(1)))
            counts = [int(x) for x in m.groups()[1:]]
            row = [wall] + [st.get(s, 0.0) for s in stages] + [ms.get(d, 0.0) for d in device]
            if r:
                rows.append(row)
            log('%s: %.3f s wall; %s s; device call: %s ms' % ('warm-up' if r == 0 else 'run %d' % r, wall,
                                                              ', '.join('%s %.3f' % (s, st.get(s, 0.0)) for s in stages),
                                                              ', '.join('%s %.2f' % (d.replace('_', ' '), ms.get(d, 0.0)) for d in device)))
        med = np.median(np.array(rows), axis=0)
        log('median of %d: %.3f s wall; %s s' % (len(rows), med[0], ', '.join('%s %.3f' % (s, v) for s, v in zip(stages, med[1:6]))))
        log('device call, median: %s ms' % ', '.join('%s %.2f' % (d.replace('_', ' '), v) for d, v in zip(device, med[6:])))
        kernels = float(med[9:14].sum())
        with_copies = float(med[8:15].sum())
        log('%d records, %d after grouping, %d hits, largest group %d: %.0f M records/s through the kernels (%.2f ms), %.0f M records/s with the copies (%.2f ms)'
            % (counts[0], counts[1], counts[2], counts[3], counts[0] / kernels / 1e3, kernels, counts[0] / with_copies / 1e3, with_copies))
        log('the device call is %.1f %% of the module\'s wall time, opening the DB %.1f %%, the text and the DB writer %.1f %%'
            % (100 * med[4] / med[0], 100 * med[1] / med[0], 100 * med[5] / med[0]))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
