"""CPU: `sdgpu createsubdb` and `sdgpu mergeclusters` (the host glue of `cluster --single-step-clustering 1`) on small DBs, against
the Python restatements tests/cluglue_ref.py."""
import os

import pytest

import cluglue_ref as ref
from dbutil import read_db, sdgpu, write_db

SEQS = [(3, b'MKVLAAGIV\n'), (4, b'MKV\n'), (9, b'\n'), (10, b'GLLLAQWERTY\n'), (17, b'ACDEFGHIKL\n'), (40, b'PQRST\n')]


def source(tmp):
    """a sequence DB with headers, lookup and source -> path"""
    path = str(tmp / 'seq')
    write_db(path, SEQS, 0)
    write_db(path + '_h', [(k, b'name%d\n' % k) for k, _ in SEQS], 12)
    open(path + '.lookup', 'w').write(''.join('%d\tname%d\t0\n' % (k, k) for k, _ in SEQS))
    open(path + '.source', 'w').write('0\tfile.fasta\n')
    return path


def key_file(tmp, keys):
    path = str(tmp / 'keys')
    open(path, 'w').write(''.join('%d\tsomething else\n' % k for k in keys))
    return path


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('keys', [[4, 10, 17], [17, 3, 10, 4], [3, 5, 40, 41], []])
def test_createsubdb_from_a_list_file(tmp_path, mode, keys):
    src = source(tmp_path)
    out = str(tmp_path / 'sub')
    p = sdgpu('createsubdb', key_file(tmp_path, keys), src, out, '--subdb-mode', mode)
    want_index, want_data = ref.createsubdb(keys, ref.read_index(src), open(src, 'rb').read(), mode)
    assert ref.read_index(out) == want_index
    # byte for byte: tab separated, list order (sorted by key only where the list was not ascending)
    assert open(out + '.index').read() == ''.join('%d\t%d\t%d\n' % e for e in want_index)
    if mode == 1:
        assert os.path.islink(out) and os.path.realpath(out) == os.path.realpath(src)
    else:
        assert not os.path.islink(out) and open(out, 'rb').read() == want_data
    assert read_db(out) == {k: v for k, v in dict(SEQS).items() if k in keys}
    assert open(out + '.dbtype', 'rb').read() == open(src + '.dbtype', 'rb').read()
    for suffix in ('_h', '_h.index', '_h.dbtype', '.lookup', '.source'):
        assert os.path.islink(out + suffix) and os.path.realpath(out + suffix) == os.path.realpath(src + suffix)
    for missing in (k for k in keys if k not in dict(SEQS)):
        assert 'Key %d not found in database' % missing in p.stderr


def test_createsubdb_from_a_db(tmp_path):
    """clustering.sh passes a cluster DB: its index names the keys"""
    src = source(tmp_path)
    clu = str(tmp_path / 'clu')
    write_db(clu, [(3, b'3\n4\n'), (10, b'10\n'), (40, b'40\n17\n')], 6)
    out = str(tmp_path / 'sub')
    sdgpu('createsubdb', clu, src, out, '--subdb-mode', 1, '-v', 0)
    index = ref.read_index(src)
    assert ref.read_index(out) == [e for e in index if e[0] in (3, 10, 40)]
    assert read_db(out) == {k: dict(SEQS)[k] for k in (3, 10, 40)}
    # again over the links of the first run, and as a copy where a link was
    sdgpu('createsubdb', clu, src, out, '--subdb-mode', 0, '-v', 0)
    assert not os.path.islink(out) and read_db(out) == {k: dict(SEQS)[k] for k in (3, 10, 40)}
    assert read_db(src) == dict(SEQS)


def test_createsubdb_refuses_names_and_a_missing_list(tmp_path):
    src = source(tmp_path)
    p = sdgpu('createsubdb', key_file(tmp_path, [3]), src, tmp_path / 'sub', '--id-mode', 1, check=False)
    assert p.returncode != 0 and '--id-mode 1' in p.stderr + p.stdout
    p = sdgpu('createsubdb', tmp_path / 'nothing', src, tmp_path / 'sub', check=False)
    assert p.returncode != 0 and 'does not exist' in p.stderr + p.stdout


def clu_entries(step):
    return [(rep, b''.join(b'%d\n' % m for m in members)) for rep, members in step]


STEP1 = [(3, [3, 4]), (9, [9]), (10, [10, 17]), (40, [40])]
STEP2 = [(10, [10, 3]), (9, [9]), (40, [40])]      # 10 takes 3's list behind its own; 9 is a cluster of one
STEP3 = [(40, [40, 9, 10])]                        # 40 takes 9's, then 10's merged list


@pytest.mark.parametrize('steps', [[STEP1, STEP2], [STEP1, STEP2, STEP3], [STEP1]])
def test_mergeclusters(tmp_path, steps):
    src = source(tmp_path)
    paths = []
    for s, step in enumerate(steps):
        paths.append(str(tmp_path / ('clu%d' % s)))
        write_db(paths[-1], clu_entries(step), 6)
    out = str(tmp_path / 'merged')
    sdgpu('mergeclusters', src, out, *paths, '-v', 0)
    want = ref.mergeclusters([k for k, _ in SEQS], steps)
    assert read_db(out) == {rep: b''.join(b'%d\n' % m for m in members) for rep, members in want.items()}
    assert open(out + '.dbtype', 'rb').read() == b'\x06\x00\x00\x00'
    assert [e[0] for e in ref.read_index(out)] == sorted(want)
    if len(steps) == 2:    # member order after the splice: the representative's list, then the spliced one
        assert want == {9: [9], 10: [10, 17, 3, 4], 40: [40]}
    if len(steps) == 3:
        assert want == {40: [40, 9, 10, 17, 3, 4]}


def test_mergeclusters_names_a_missing_key(tmp_path):
    src = source(tmp_path)
    write_db(str(tmp_path / 'clu0'), clu_entries([(3, [3, 5])]), 6)
    p = sdgpu('mergeclusters', src, tmp_path / 'merged', tmp_path / 'clu0', check=False)
    assert p.returncode != 0 and 'key 5 ' in p.stderr + p.stdout
    with pytest.raises(KeyError):
        ref.mergeclusters([k for k, _ in SEQS], [[(3, [3, 5])]])
    write_db(str(tmp_path / 'clu1'), clu_entries([(3, [3])]), 6)
    write_db(str(tmp_path / 'clu2'), clu_entries([(77, [77])]), 6)
    p = sdgpu('mergeclusters', src, tmp_path / 'merged2', tmp_path / 'clu1', tmp_path / 'clu2', check=False)
    assert p.returncode != 0 and 'key 77 ' in p.stderr + p.stdout


def test_help_lists_the_modules():
    text = sdgpu('--help').stdout
    assert all(m in text for m in ('createsubdb', 'mergeclusters', 'cluster '))
