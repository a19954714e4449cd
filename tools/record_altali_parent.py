#!/usr/bin/env python3
"""Records tests/golden/altali_parent_aln0.json: per `align` command of tests/test_gpu_altali.py's module tests (MODULE_CASES),
the row count and the md5 of the alignment DB's data and index files that a given sdgpu binary writes with `--alt-ali 0`.
The committed file was written by the binary built from the commit before `--alt-ali` was implemented; the test holds the
current binary's `--alt-ali 0` output against it byte for byte.

    python tools/record_altali_parent.py /path/to/parent/build/spacedust_amd/sdgpu   (needs a GPU)"""
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import dbutil  # noqa: E402
import test_gpu_altali as t  # noqa: E402


def main():
    dbutil.SDGPU = os.path.abspath(sys.argv[1])
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        g, pref = t.genome_work(tmp)
        for name, par in t.MODULE_CASES.items():
            dbutil.sdgpu('align', g, g, pref, tmp / name, *t.ALN_COMMON, *par, '--alt-ali', '0')
            out[name] = [sum(len(r) for r in t.rows_of(tmp / name).values())] + t.db_md5(tmp / name)
            print(name, out[name])
    with open(os.path.join(dbutil.GOLD, 'altali_parent_aln0.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
