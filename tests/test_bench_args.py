"""bench.py's options: a plain run leaves out every leg beside the timed steps, --full keeps them (no GPU: the parser only)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ('no_cpu', 'no_children', 'no_index_check', 'no_p100', 'no_p10000', 'no_iter3')


def parsed(*argv):
    # in a child process: importing bench.py sets the OpenMP environment of the process
    code = 'import json, sys; import bench; sys.argv = ["bench.py"] + sys.argv[1:]; print(json.dumps(vars(bench.parse())))'
    r = subprocess.run([sys.executable, '-c', code] + list(argv), cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


def test_plain_run_is_the_headline_only():
    a = parsed('--gpus', '1', '--steps', '3', '--warmup', '1')
    assert not a['full'] and a['no_cpu'] and a['no_children'] and a['no_index_check']
    assert (a['steps'], a['warmup'], a['proteomes'], a['batch']) == (3, 1, 1000, 4)


def test_full_run_keeps_every_leg_unless_told_otherwise():
    a = parsed('--gpus', '1', '--steps', '3', '--warmup', '1', '--full')
    assert a['full'] and not any(a[k] for k in LEGS)
    a = parsed('--full', '--no-cpu', '--no-iter3')
    assert a['no_cpu'] and a['no_iter3'] and not a['no_children'] and not a['no_index_check'] and not a['no_p100']
