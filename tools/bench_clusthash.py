#!/usr/bin/env python3
"""What `sdgpu clusthash` costs, stage by stage, on one MI355X at the module's defaults (alphabet 3, --min-seq-id 0.99).  Inputs:

  plain    bench.py's synthetic proteomes (100 by default: 300 000 proteins)
  copies   the same set with copies added behind it: --share of the proteins (default 5 %) get one copy each -- exact, or with 1, 2 or 5
           letters substituted, inside the letter's class of the 3-letter alphabet (same hash: compared) or across classes (other hash:
           never compared), in equal parts -- and one protein is copied 5 000 times
  groups   (--groups) 16 groups each of 8, 32, 64, 128, 512 and 2 048 sequences of one hash and length (a root and copies 0 .. 3 letters
           away, as tests/test_gpu_clusthash.py builds them): what the single-wavefront bound of the group pass is chosen on.  A build
           with another bound (SD_HIP_EXTRA=-DCH_WAVE_BOUND=...) run on this input gives the other side of the comparison.

The module runs --runs + 1 times per input (the first is warm-up) with SD_DEBUG_TIMING=1: its wall time by stage, and the device call's
stages, each followed by a wait, so that they add up to the call.  --trace runs the module once more on `copies` under
`rocprofv3 --kernel-trace --stats` (no counters) and lists the kernels.  --dump FILE writes the letters of `copies` for
tools/make_golden_clusthash.py --time FILE THREADS, which times the reference's own clusthash() where the reference tree is.

    python tools/bench_clusthash.py [--proteomes 100] [--runs 3] [--groups] [--trace] [--only INPUT] [--sdgpu PATH]
                                    [--out profiles/clusthash.txt] [--dump ch_seqs.npz]
"""
import argparse
import glob
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
from bench_kmermatcher import write_seq_db  # noqa: E402

STAGES = ['open', 'letter map', 'context', 'device', 'text and write']
DEVICE = ['prepare', 'alloc', 'copy_in', 'hash', 'sort', 'groups', 'pass', 'copy_out']


def with_copies(residues, offsets, lmap3, share, rng):
    """-> (residues, offsets, description) with the copies behind the set"""
    off = np.asarray(offsets, np.int64)
    n = len(off) - 1
    peers = {c: [d for d in range(20) if d != c and lmap3[d] == lmap3[c]] for c in range(20)}
    others = {c: [d for d in range(20) if lmap3[d] != lmap3[c]] for c in range(20)}
    picked = rng.permutation(n)[:int(n * share)]
    kinds = [(0, True)] + [(k, inside) for k in (1, 2, 5) for inside in (True, False)]
    extra = []
    for x, s in enumerate(picked):
        seq = residues[off[s]:off[s + 1]].copy()
        k, inside = kinds[x % len(kinds)]
        for p in rng.permutation(len(seq))[:k]:
            pool = (peers if inside else others).get(int(seq[p]), [])
            if pool:
                seq[p] = pool[int(rng.integers(0, len(pool)))]
        extra.append(seq)
    hub = residues[off[picked[0]]:off[picked[0] + 1]]
    extra += [hub] * 5000
    lens = np.concatenate([np.diff(off), [len(s) for s in extra]])
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    what = ('%d copies (%.1f %% of %d proteins: a seventh each exact, and 1, 2 and 5 substitutions inside and across the classes of the '
            '3-letter alphabet) and one protein of %d residues 5 000 times' % (len(picked), 100.0 * len(picked) / n, n, len(hub)))
    return np.concatenate([residues] + extra).astype(np.uint8), new_off, what


def group_input(lmap3, rng):
    peers = {c: [d for d in range(20) if d != c and lmap3[d] == lmap3[c]] for c in range(20)}
    seqs = []
    for size in (8, 32, 64, 128, 512, 2048):
        for _ in range(16):
            root = rng.integers(0, 20, 150).astype(np.uint8)
            seqs.append(root)
            for _ in range(size - 1):
                s = root.copy()
                for p in rng.permutation(150)[:int(rng.integers(0, 4))]:
                    s[p] = peers[int(root[p])][int(rng.integers(0, len(peers[int(root[p])])))]
                seqs.append(s)
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return np.concatenate(seqs), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--proteomes', type=int, default=100)
    ap.add_argument('--genes', type=int, default=3000)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--share', type=float, default=0.05)
    ap.add_argument('--groups', action='store_true')
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--only', default=None, help='one input alone: plain, copies or groups')
    ap.add_argument('--sdgpu', default=None, help='another build of the driver (a tuning build of the bound), next to its libsdgpu.so')
    ap.add_argument('--step-timeout', type=float, default=60.0, help='seconds one run of the module may take (the traced run: twice that)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--dump', default=None)
    a = ap.parse_args()
    from spacedust_amd import api
    from spacedust_amd.synth import ALPHABET, make_proteomes
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    sdgpu = a.sdgpu or os.path.join(ROOT, 'spacedust_amd', 'sdgpu')
    threads = str(min(16, os.cpu_count() or 1))
    lmap3 = api.reduced_alphabet(3)[0]
    rng = np.random.default_rng(0xC1A5)
    inputs = []
    if a.only in (None, 'plain', 'copies'):
        ps = make_proteomes(a.proteomes, genes_per_proteome=a.genes, seed=0x5ED0 + 2, workers=1)
        inputs.append(('plain', ps.residues, ps.offsets, '%d proteomes, %d proteins' % (a.proteomes, ps.n)))
        res2, off2, what = with_copies(ps.residues, ps.offsets, lmap3, a.share, rng)
        inputs.append(('copies', res2, off2, 'plain and ' + what))
    if a.groups or a.only == 'groups':
        res3, off3 = group_input(lmap3, rng)
        inputs.append(('groups', res3, off3, '16 groups each of 8, 32, 64, 128, 512 and 2 048 sequences of 150 residues, one hash per group'))
    inputs = [i for i in inputs if a.only in (None, i[0])]
    if a.dump:
        os.makedirs(os.path.dirname(os.path.abspath(a.dump)), exist_ok=True)
        np.savez_compressed(a.dump, letters=np.frombuffer(ALPHABET.encode(), np.uint8)[res2], off=off2)
    pat = re.compile(r'\[clusthash\] (.+?) ([\d.]+) s$', re.M)
    dev = re.compile(r'\[clusthash\] device: (.*); (\d+) groups, (\d+) pairs compared, largest group (\d+)')
    env = dict(os.environ, SD_DEBUG_TIMING='1')
    with tempfile.TemporaryDirectory() as tmp:
        for name, res, off, what in inputs:
            db = '%s/%s' % (tmp, name)
            write_seq_db(db, res, off, ALPHABET)
            log('input `%s`: %s; %d sequences, %d residues; `sdgpu clusthash` at its defaults; %s threads' % (name, what, len(off) - 1, int(off[-1]), threads))
            rows = []
            for r in range(a.runs + 1):
                t0 = time.time()
                p = subprocess.run([sdgpu, 'clusthash', db, db + '_res', '--threads', threads, '-v', '0'], env=env, stderr=subprocess.PIPE, text=True,
                                   check=True, timeout=a.step_timeout)
                wall = time.time() - t0
                st = {k: float(v) for k, v in pat.findall(p.stderr)}
                m = dev.search(p.stderr)
                ms = dict((k, float(v)) for k, v in re.findall(r'(\w+) ([\d.]+) ms', m.group(1)))
                counts = [int(x) for x in m.groups()[1:]]
                if r:
                    rows.append([wall] + [st.get(s, 0.0) for s in STAGES] + [ms.get(d, 0.0) for d in DEVICE])
                log('  %s: %.3f s wall; %s s; device call: %s ms' % ('warm-up' if r == 0 else 'run %d' % r, wall,
                                                                    ', '.join('%s %.3f' % (s, st.get(s, 0.0)) for s in STAGES),
                                                                    ', '.join('%s %.2f' % (d.replace('_', ' '), ms.get(d, 0.0)) for d in DEVICE)))
            med = np.median(np.array(rows), axis=0)
            log('  median of %d: %.3f s wall; %s s' % (len(rows), med[0], ', '.join('%s %.3f' % (s, v) for s, v in zip(STAGES, med[1:6]))))
            log('  device call, median: %s ms' % ', '.join('%s %.2f' % (d.replace('_', ' '), v) for d, v in zip(DEVICE, med[6:])))
            log('  stage sum %.2f ms against the call %.2f ms; %d groups, %d pairs compared, largest group %d' %
                (float(med[6:].sum()), 1e3 * med[4], counts[0], counts[1], counts[2]))
        if a.trace:
            db = '%s/copies' % tmp
            out = '%s/trace' % tmp
            subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '-d', out, '-o', 'clusthash', '--', sdgpu, 'clusthash', db, db + '_res', '--threads',
                            threads, '-v', '0'], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=2 * a.step_timeout)
            found = glob.glob(out + '/**/*results.db', recursive=True)
            log('kernels of one run on `copies` under rocprofv3 --kernel-trace --stats (no counters), by tools/rocprof_summary.py:')
            if found:
                p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rocprof_summary.py'), found[0]], stdout=subprocess.PIPE, text=True, check=True)
                for line in p.stdout.splitlines():
                    log('  ' + line)
            else:
                log('  (no results.db was written)')
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
