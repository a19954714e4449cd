"""sd_host_split_plan (the target split of `prefilter --split N --split-mode 0`) against a restatement of the reference written
here from M/src/commons/DBReader.cpp:1216-1257 (decomposeDomainByAminoAcid) and M/src/prefiltering/Prefiltering.cpp:351-361
(k-mer size and list length after setupSplit), not from the product's code.  Every case asserts on its own input that it takes
the branch it is named after."""
import math

import numpy as np
import pytest

from spacedust_amd.api import Host
from spacedust_amd._lib import SdError
from dbutil import sdgpu, example_fasta


@pytest.fixture(scope='module')
def host():
    return Host(1)


def ref_decompose(lengths, world_rank, world_size):
    """DBReader::decomposeDomainByAminoAcid: (startEntry, numEntries) of one rank; lengths = DBReader::index[i].length"""
    data_size = sum(lengths)            # DBReader::getDataSize(): readIndex sums the length column
    db_entries = len(lengths)
    assert world_size <= data_size      # the reference exits otherwise
    if world_size == 1:
        return 0, db_entries
    if db_entries <= world_size:
        return (world_rank, 1) if world_rank < db_entries else (0, 0)
    chunk_size = int(math.ceil(float(data_size) / float(world_size)))
    entries_per_worker = [0] * world_size
    current_rank, assigned = 0, 0
    for i in range(db_entries):
        if assigned >= chunk_size:
            assigned = 0
            current_rank += 1
        assigned += lengths[i]
        entries_per_worker[current_rank] += 1
    return sum(entries_per_worker[:world_rank]), entries_per_worker[world_rank]


def ref_list_len(max_seqs, db_size, n):
    """Prefiltering.cpp:169 then :358-361"""
    L = min(db_size, max_seqs)
    if n > 1:
        four_times_std_deviation = int(4 * math.sqrt(float(L) / float(n)))   # size_t = 4 * sqrt(double / double)
        L = max(1, L // n + four_times_std_deviation)
    return L


def ref_kmer_size(aa_size):
    """IndexTable::computeKmerSize (IndexTable.h:439-449)"""
    return 6 if aa_size < 3350000000 else 7


def check(host, lengths, n, max_seqs=300, k=0, residues=None):
    lengths = [int(x) for x in lengths]
    if residues is None:
        residues = sum(lengths) - 2 * len(lengths)    # DBReader::getAminoAcidDBSize
    p = host.split_plan(lengths, n, max_seqs=max_seqs, k=k, residues=residues)
    want = [ref_decompose(lengths, r, n) for r in range(n)]
    assert [(int(f), int(s)) for f, s in zip(p['db_from'], p['db_size'])] == want
    assert p['list_len'] == ref_list_len(max_seqs, len(lengths), n)
    assert p['k'] == (k if k else ref_kmer_size(residues // max(n, 1)))
    return p, want


def test_one_split(host):
    p, want = check(host, [12, 7, 300, 41], 1)
    assert want == [(0, 4)] and p['list_len'] == 4          # the worldSize == 1 branch; L = min(--max-seqs, 4)


def test_entries_not_more_than_splits(host):
    _, want = check(host, [50, 60, 70], 3)                  # dbEntries == worldSize
    assert want == [(0, 1), (1, 1), (2, 1)]
    _, want = check(host, [50, 60], 5)                      # dbEntries < worldSize: ranks past the entries get (0, 0)
    assert want == [(0, 1), (1, 1), (0, 0), (0, 0), (0, 0)]


def test_chunk_closed_exactly_at_chunk_size_and_one_entry_past_it(host):
    # dataSize 60, 2 splits: chunkSize 30.  10 + 20 reaches 30 exactly: the chunk closes before the third entry
    lengths = [10, 20, 10, 10, 10]
    assert math.ceil(sum(lengths) / 2) == 30 and lengths[0] + lengths[1] == 30
    _, want = check(host, lengths, 2)
    assert want == [(0, 2), (2, 3)]
    # 10 + 19 = 29 < 30: the entry that crosses the size (to 39) still belongs to the first chunk
    lengths = [10, 19, 10, 11, 10]
    assert math.ceil(sum(lengths) / 2) == 30 and lengths[0] + lengths[1] < 30 < sum(lengths[:3])
    _, want = check(host, lengths, 2)
    assert want == [(0, 3), (3, 2)]


def test_long_first_entry_leaves_trailing_splits_empty(host):
    lengths = [1000, 5, 5, 5, 5]
    assert len(lengths) > 4 and math.ceil(sum(lengths) / 4) < lengths[0]
    _, want = check(host, lengths, 4)
    assert want == [(0, 1), (1, 4), (5, 0), (5, 0)]          # runSplit skips the splits of size 0


@pytest.fixture(scope='module')
def genome_lengths(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('splitplan')
    fa = example_fasta(tmp)
    sdgpu('createsetdb', fa[0], fa[1], tmp / 'genome', tmp / 'tmp', '-v', '0')
    rows = sorted((int(l.split()[0]), int(l.split()[2])) for l in open(tmp / 'genome.index'))
    return [l for _, l in rows]


@pytest.mark.parametrize('n', [2, 3, 7])
def test_example_genomes(host, genome_lengths, n):
    assert len(genome_lengths) == 5898
    p, want = check(host, genome_lengths, n)
    assert len(genome_lengths) > n                           # the chunk branch
    start = 0
    for f, s in want:                                        # contiguous, nothing empty at this size, sizes sum to the DB size
        assert f == start and s > 0
        start += s
    assert start == len(genome_lengths)
    assert p['list_len'] == {2: 198, 3: 140, 7: 68}[n] and p['k'] == 6


def test_list_lengths(host):
    lengths = [100] * 1000
    for n, want in ((2, 198), (3, 140), (7, 68)):
        p, _ = check(host, lengths, n, max_seqs=300)
        assert p['list_len'] == want
    p, _ = check(host, lengths, 3, max_seqs=1)               # L = 1: 1 / 3 + size_t(4 sqrt(1 / 3)) = 0 + 2
    assert p['list_len'] == 2
    p, _ = check(host, [100], 1, max_seqs=300)               # L = min(--max-seqs, DB size) = 1, one split: unchanged
    assert p['list_len'] == 1
    p, _ = check(host, lengths, 1000, max_seqs=1)            # 1 / 1000 + size_t(4 sqrt(0.001)) = 0: max(1, .) holds the floor
    assert int(4 * math.sqrt(1 / 1000)) == 0 and p['list_len'] == 1


def test_kmer_size_follows_the_split(host):
    lengths = [100] * 10
    thr = 3350000000
    for n in (1, 2, 3):
        p, _ = check(host, lengths, n, residues=thr * n - 1)     # (thr n - 1) / n < thr
        assert (thr * n - 1) // n < thr and p['k'] == 6
        p, _ = check(host, lengths, n, residues=thr * n)         # thr n / n = thr: not below
        assert (thr * n) // n >= thr and p['k'] == 7
    # a target that is k = 7 whole becomes k = 6 in three splits
    assert check(host, lengths, 1, residues=2 * thr)[0]['k'] == 7 and check(host, lengths, 3, residues=2 * thr)[0]['k'] == 6
    assert check(host, lengths, 3, k=7, residues=10)[0]['k'] == 7    # -k given: kept


def test_refusals(host):
    with pytest.raises(SdError):
        host.split_plan([3, 3], 0)
    with pytest.raises(SdError):
        host.split_plan([1, 1], 3)        # more splits than bytes of data: the reference exits (DBReader.cpp:1219-1223)


def test_footprint_is_monotone_and_covers_the_resident_tables():
    from spacedust_amd.api import target_footprint
    tables6 = 2 * 8000 * 8000 * 2 + 64000001 * 4       # the 3-mer matrices and the list starts of k = 6 stay resident
    tables7 = 2 * 8000 * 8000 * 2 + 1280000001 * 4
    assert target_footprint(6, 1, 1) > tables6 and target_footprint(7, 1, 1) > tables7
    a, b, c = target_footprint(6, 1000, 300000), target_footprint(6, 2000, 600000), target_footprint(6, 2000, 10 ** 9)
    assert a <= b < c
    assert c >= 10 ** 9 * (1 + 8)                        # masked residues and 8-byte entries of up to one record per residue
    assert target_footprint(5, 10, 10) == 0
