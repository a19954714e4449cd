#!/usr/bin/env python3
"""What `sdgpu makeclusterdb --single-step-clustering 1` costs, step by step, on one MI355X at the workflow's defaults (--min-seq-id 0.7 -c 0.8
--cov-mode 0): bench.py's synthetic proteomes (3 000 proteins each) as one sequence DB, the workflow run --runs times on a fresh
directory.  Per run: wall time, the seconds of each of the five steps (the workflow's own `makeclusterdb: <step> took` lines), the clusters
found, and of `result2profile` the pairs realigned, their rate inside the realign stage and the bytes uploaded for it (the module's
own line).  Nothing is asserted; profiles/clusterdb.txt records the lines with date and box.

    python tools/bench_clusterdb.py [--proteomes 100] [--genes 3000] [--runs 2] [--out profiles/clusterdb.txt]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_kmermatcher import write_seq_db  # noqa: E402

STEPS = ['cluster', 'createsubdb', 'result2profile', 'profile2consensus', 'align']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--proteomes', type=int, default=100)
    ap.add_argument('--genes', type=int, default=3000)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from spacedust_amd.synth import ALPHABET, make_proteomes
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    sdgpu = os.path.join(ROOT, 'spacedust_amd', 'sdgpu')
    threads = str(min(16, os.cpu_count() or 1))
    ps = make_proteomes(a.proteomes, genes_per_proteome=a.genes, seed=0x5ED0 + 2)
    took = re.compile(r'^makeclusterdb: (\w+) took ([\d.]+) s$', re.M)
    realigned = re.compile(r'result2profile: (\d+) pairs realigned in ([\d.]+) s \((\d+) pairs/s\), about (\d+) bytes uploaded')
    with tempfile.TemporaryDirectory() as tmp:
        log('input: %d proteomes, %d proteins, %d residues; `sdgpu makeclusterdb --single-step-clustering 1` at its defaults; %s threads'
            % (a.proteomes, ps.n, int(ps.offsets[-1]), threads))
        for r in range(a.runs):
            work = os.path.join(tmp, 'run%d' % r)
            os.makedirs(work)
            db = os.path.join(work, 'seq')
            write_seq_db(db, ps.residues, ps.offsets, ALPHABET)
            t0 = time.time()
            p = subprocess.run([sdgpu, 'makeclusterdb', db, os.path.join(work, 'tmp'), '--single-step-clustering', '1', '--threads', threads],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            wall = time.time() - t0
            if p.returncode != 0:
                log('run %d: failed (%d) after %.1f s: %s' % (r + 1, p.returncode, wall, p.stderr.strip().splitlines()[-1:] or ''))
                break
            sec = dict((k, float(v)) for k, v in took.findall(p.stdout))
            n_clu = sum(1 for _ in open(db + '_clu.index'))
            m = realigned.search(p.stdout)
            log('run %d: %.2f s wall; %s s; %d clusters' % (r + 1, wall, ', '.join('%s %.2f' % (s, sec.get(s, 0.0)) for s in STEPS), n_clu))
            if m:
                log('  result2profile: %s pairs realigned in %s s: %s pairs/s in the realign stage (upload, the three Smith-Waterman passes, '
                    'download, the pool rewritten), about %.1f MB uploaded for it (an estimate: residues, bias and pair lists)'
                    % (m.group(1), m.group(2), m.group(3), int(m.group(4)) / 1e6))
            for l in p.stdout.splitlines():
                if l.startswith('makeclusterdb: sequence set '):
                    log('  ' + l.replace(work, '<run>'))
            shutil.rmtree(work)
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
