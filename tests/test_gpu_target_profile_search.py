"""GPU: sequence queries searched against a profile target DB -- `prefilter`, `swapresults`, `align` with the profile as the query,
`swapresults` (M/data/workflow/searchtargetprofile.sh) -- module by module, through `sdgpu search` and through a workflow script with
MMSEQS=sdgpu, against the reference's rows as tools/make_golden_swap.py recorded them for the 18 profiles x 152 sequences of set G."""
import os
import subprocess

import numpy as np
import pytest

import swapgold
import tpref
from dbutil import SDGPU, read_db, sdgpu, write_db

pytestmark = pytest.mark.gpu

THRESHOLDS = {'G110': 110, 'G95': 95}
# the parameter strings Search.cpp:453-475 hands to the script (Parameters::createParameterString of the prefilter, align and swapresult
# sets): the align step lists every hit (--max-seqs INT_MAX) with the swapped coverage mode (0 stays 0)
PREFILTER_PAR = ("--sub-mat aa:blosum62.out,nucl:nucleotide.out --seed-sub-mat aa:VTML80.out,nucl:nucleotide.out -k 0 "
                 "--target-search-mode 0 --k-score seq:2147483647,prof:%d --alph-size aa:21,nucl:5 --max-seq-len 65535 "
                 "--max-seqs 300 --split 0 --split-mode 2 --split-memory-limit 0 -c 0 --cov-mode 0 --comp-bias-corr 1 "
                 "--comp-bias-corr-scale 1 --diag-score 1 --exact-kmer-matching 0 --mask 1 --mask-prob 0.9 --mask-lower-case 0 "
                 "--mask-n-repeat 0 --min-ungapped-score 15 --add-self-matches 0 --spaced-kmer-mode 1 --db-load-mode 0 "
                 "--pca substitution:1.100,context:1.400 --pcb substitution:4.100,context:5.800 --threads 8 --compressed 0 -v 3 -s 5.7")
ALIGN_PAR = ("--sub-mat aa:blosum62.out,nucl:nucleotide.out -a 1 --alignment-mode 2 --alignment-output-mode 0 --wrapped-scoring 0 "
             "-e %s --min-seq-id 0 --min-aln-len 0 --seq-id-mode 0 --alt-ali 0 -c 0 --cov-mode 0 --max-seq-len 65535 "
             "--comp-bias-corr 1 --comp-bias-corr-scale 1 --max-rejected 2147483647 --max-accept 2147483647 --add-self-matches 0 "
             "--db-load-mode 0 --pca substitution:1.100,context:1.400 --pcb substitution:4.100,context:5.800 --score-bias 0 "
             "--realign 0 --realign-score-bias -0.2 --realign-max-seqs 2147483647 --corr-score-weight 0 --gap-open aa:11,nucl:5 "
             "--gap-extend aa:1,nucl:2 --zdrop 40 --max-seqs 2147483647 --threads 8 --compressed 0 -v 3")
SWAP_PAR = ("--sub-mat aa:blosum62.out,nucl:nucleotide.out -e %s --split-memory-limit 0 --gap-open aa:11,nucl:5 --gap-extend aa:1,nucl:2 "
            "--threads 8 --compressed 0 --db-load-mode 0 -v 3")
# the four module calls of searchtargetprofile.sh ($1 query, $2 target, $3 result, $4 tmp), written here
SCRIPT = '''#!/bin/sh -e
$RUNNER "$MMSEQS" prefilter "$1" "$2" "$4/pref" ${PREFILTER_PAR}
"$MMSEQS" swapresults "$1" "$2" "$4/pref" "$4/pref_swapped" ${SWAP_PAR}
$RUNNER "$MMSEQS" "${ALIGN_MODULE}" "$2" "$1" "$4/pref_swapped" "$4/aln_swapped" ${ALIGNMENT_PAR}
"$MMSEQS" swapresults "$2" "$1" "$4/aln_swapped" "$3" ${SWAP_PAR}
'''


def e_text(tag, which):
    return '%.3E' % float(swapgold.golden()[tag + '_E'][which])


def aln_swapped_at(tag, which):
    """what `align` leaves at -e E[which]: the recorded entries (aligned at E[0]) without the lines above it (E[1] lies in a gap of the
    E-values, tests/test_swapresults.py)"""
    e = float(swapgold.golden()[tag + '_E'][which])
    return {k: b''.join(l + b'\n' for l in t.splitlines() if float(l.split(b'\t')[3]) <= e) for k, t in swapgold.db(tag + '_aln_swapped').items()}


@pytest.fixture(scope='module')
def dbs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('tpsearch')
    seq_db, prof_db = swapgold.write_set_g(tmp)
    return tmp, seq_db, prof_db


@pytest.mark.parametrize('tag', swapgold.SETS)
def test_the_four_modules_one_by_one(dbs, tag):
    tmp, seq_db, prof_db = dbs
    w = str(tmp / (tag + '_mod_'))
    sdgpu('prefilter', seq_db, prof_db, w + 'pref', *(PREFILTER_PAR % THRESHOLDS[tag]).split())
    assert read_db(w + 'pref') == swapgold.db(tag + '_pref')
    sdgpu('swapresults', seq_db, prof_db, w + 'pref', w + 'pref_swapped', *(SWAP_PAR % e_text(tag, 0)).split())
    assert read_db(w + 'pref_swapped') == swapgold.db(tag + '_pref_swapped')
    sdgpu('align', prof_db, seq_db, w + 'pref_swapped', w + 'aln_swapped', *(ALIGN_PAR % e_text(tag, 0)).split())
    assert read_db(w + 'aln_swapped') == swapgold.db(tag + '_aln_swapped')
    for which in (0, 1):
        sdgpu('swapresults', prof_db, seq_db, w + 'aln_swapped', w + 'final_%d' % which, *(SWAP_PAR % e_text(tag, which)).split())
        assert read_db(w + 'final_%d' % which) == swapgold.db(tag + '_final_%d' % which), which


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('tag', swapgold.SETS)
def test_search_routes_through_the_swapped_chain(dbs, tag, which):
    tmp, seq_db, prof_db = dbs
    res, work = str(tmp / ('%s_search_%d' % (tag, which))), str(tmp / ('%s_tmp_%d' % (tag, which)))
    sdgpu('search', seq_db, prof_db, res, work, '--k-score', 'seq:2147483647,prof:%d' % THRESHOLDS[tag], '-e', e_text(tag, which),
          '--keep-tmp', '1', '--threads', '8', '-v', '0')
    assert read_db(res) == swapgold.db(tag + '_final_%d' % which)
    assert read_db(work + '/pref') == swapgold.db(tag + '_pref')
    assert read_db(work + '/pref_swapped') == swapgold.db(tag + '_pref_swapped')
    assert read_db(work + '/aln_swapped') == aln_swapped_at(tag, which)
    assert open(res + '.dbtype', 'rb').read() == b'\x05\x00\x00\x00'


def test_search_removes_its_intermediates(dbs):
    tmp, seq_db, prof_db = dbs
    res, work = str(tmp / 'search_clean'), str(tmp / 'tmp_clean')
    sdgpu('search', seq_db, prof_db, res, work, '--k-score', 'seq:2147483647,prof:110', '--threads', '8', '-v', '0')
    assert read_db(res) == swapgold.db('G110_final_0')           # -e 0.001, the workflow's default, is E[0]
    for name in ('pref', 'pref_swapped', 'aln_swapped'):
        for suffix in ('', '.index', '.dbtype'):
            assert not os.path.exists(os.path.join(work, name + suffix)), name + suffix


def _seqid_text(identical, aln_len):
    """Util::fastSeqIdToBuffer as Matcher::resultToBuffer leaves it"""
    s = np.float32(identical) / np.float32(aln_len)
    if s == np.float32(1.0):
        return '1.00'
    return '0.' + ('0' if s < np.float32(0.10) else '') + ('0' if s < np.float32(0.01) else '') + str(int(np.float32(s * np.float32(1000))))


def _compress(bt):
    out, state, n = [], 'M', 0
    for ch in bt:
        if ch != state:
            out.append('%d%s' % (n, state))
            state, n = ch, 1
        else:
            n += 1
    out.append('%d%s' % (n, state))
    return ''.join(out)


def test_align_lists_every_sequence_of_the_query_db(dbs, host, oracle):
    """an entry of pref_swapped may list every sequence of the user's DB (--max-seqs INT_MAX): one profile against all 152, next to
    empty entries; every row is the oracle's"""
    tmp, seq_db, prof_db = dbs
    p = 4
    seqs = swapgold.sequences()
    entries = [(k, b''.join(b'%d\t20\t0\n' % s for s in range(len(seqs))) if k == p else b'') for k in range(swapgold.N_PROF)]
    write_db(str(tmp / 'all_pref_swapped'), entries, 7)
    out = str(tmp / 'all_aln_swapped')
    sdgpu('align', prof_db, seq_db, tmp / 'all_pref_swapped', out, *(ALIGN_PAR % '10').split())
    got = read_db(out)
    assert sorted(got) == list(range(swapgold.N_PROF)) and all(got[k] == b'' for k in got if k != p)
    data, poff = tpref.g_profiles()
    prof = host.map_profiles(data[int(poff[p]):int(poff[p + 1])], np.array([0, int(poff[p + 1] - poff[p])], np.uint64))
    res, off = host.map_sequences([s.decode() for s in seqs])
    db_residues = int(off[-1])
    want = []
    for s in range(len(seqs)):
        r = oracle.sw_align_profile(prof['letters'], prof['aln'], res[int(off[s]):int(off[s + 1])], db_residues, sw_mode=2, eval_thr=10.0,
                                    cov_mode=0, cov_thr=0.0)
        if r['qStart'] < 0 or r['tStart'] < 0 or r['btLen'] <= 0 or not r['evalue'] <= 10.0:
            continue
        bits = int(oracle.bitscore(r['score']) + 0.5)
        line = '%d\t%d\t%s\t%.3E\t%d\t%d\t%d\t%d\t%d\t%d\t%s' % (s, bits, _seqid_text(r['identical'], r['btLen']), r['evalue'], r['qStart'], r['qEnd'],
                                                             len(prof['letters']), r['tStart'], r['tEnd'], len(seqs[s]), _compress(r['backtrace']))
        want.append(((r['evalue'], -bits, len(seqs[s]), s), line.encode()))
    want.sort(key=lambda x: x[0])
    lines = got[p].splitlines()
    assert len(lines) >= 4                                             # the four descendants of the profile's base at least
    assert set(lines) <= set(l for _, l in want)
    assert lines == [l for _, l in want]


def test_workflow_script_with_sdgpu_as_mmseqs(dbs):
    tmp, seq_db, prof_db = dbs
    script = str(tmp / 'searchtargetprofile.sh')
    open(script, 'w').write(SCRIPT)
    work = str(tmp / 'script_tmp')
    os.makedirs(work)
    res = str(tmp / 'script_result')
    env = dict(os.environ, MMSEQS=SDGPU, RUNNER='', ALIGN_MODULE='align', PREFILTER_PAR=PREFILTER_PAR % 95, ALIGNMENT_PAR=ALIGN_PAR % e_text('G95', 1),
               SWAP_PAR=SWAP_PAR % e_text('G95', 1))
    p = subprocess.run(['sh', '-e', script, seq_db, prof_db, res, work], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert read_db(res) == swapgold.db('G95_final_1')
    assert read_db(work + '/pref_swapped') == swapgold.db('G95_pref_swapped')
    assert read_db(work + '/aln_swapped') == aln_swapped_at('G95', 1)


@pytest.mark.parametrize('flags,env,words', [
    (['--num-iterations', '2'], {}, 'profile target databases are not supported'),
    (['--alignment-mode', '4'], {}, 'profile target databases are not supported'),
    (['--alt-ali', '2'], {}, '--alt-ali with a profile target database'),
    ([], {'WORLD_SIZE': '2', 'RANK': '0'}, 'profile target databases are not supported'),
])
def test_what_stays_refused(dbs, flags, env, words):
    tmp, seq_db, prof_db = dbs
    res = str(tmp / ('refused' + ''.join(flags).replace('-', '_') + '_'.join(sorted(env))))
    p = subprocess.run([SDGPU, 'search', seq_db, prof_db, res, str(tmp / 'refused_tmp'), '--k-score', 'seq:2147483647,prof:110'] + flags,
                       env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode != 0 and words in p.stderr, p.stderr
    for suffix in ('', '.index', '.dbtype'):
        assert not os.path.exists(res + suffix), suffix
