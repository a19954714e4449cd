#!/usr/bin/env python3
"""Golden rows of the target split (`prefilter --split 3 --split-mode 0`): tests/golden/split_vectors.npz.

The two example genomes as one DB (createsetdb's key order = FASTA order), N = 3 splits, the parameters of the regression
command line (-s 5.7 -k 6, -c 0.8 --cov-mode 2) with --max-seqs MAX_SEQS.  Only the reference's classes compute
(oracle/_ref/libsdref.so): per split a RefIndex over the split's sequences and a RefPrefilter with the per-split list length
(QueryMatcher sees the split's own dbSize), the identity id handed over in the query's home split only and relative to dbFrom
(Prefiltering.cpp:824-837).  Restated here: the split itself (DBReader::decomposeDomainByAminoAcid, DBReader.cpp:1216-1257, and
the list length of Prefiltering.cpp:358-361), the writer's coverage filter (Prefiltering.cpp:856-863), the id offset
(:848-850) and the merge (mergeTargetSplits, :379-479: the per-split lists one after the other, sorted by
hit_t::compareHitsByScoreAndId, QueryMatcher.h:38-48, nothing cut).

Three conditions are asserted on the reference's output before anything is written (tests/test_gpu_split.py asserts them again
on the file): a sampled (query, split) list is cut at the per-split length, a merged list is longer than --max-seqs, and a
merged list differs from the first --max-seqs rows of the unsplit reference list."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.pyoracle import Ref, read_fasta  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
EX = '/root/reference/examples/'
N_SPLITS = 3
MAX_SEQS = 30          # per split 30 / 3 + int(4 sqrt(30 / 3)) = 22, up to 66 merged: all three conditions hold on the sample
SAMPLE = range(7, 5898, 127)   # 47 queries of both genomes
COV_THR = np.float32(0.8)      # -c 0.8 --cov-mode 2: targetLength / queryLength >= 0.8 (Util::canBeCovered)


def decompose(lengths, n):
    """entries per rank, DBReader.cpp:1237-1250 (more entries than ranks)"""
    chunk = int(math.ceil(float(sum(lengths)) / float(n)))
    per, rank, acc = [0] * n, 0, 0
    for l in lengths:
        if acc >= chunk:
            acc = 0
            rank += 1
        acc += l
        per[rank] += 1
    return per


def main():
    ref = Ref(6)
    seqs = read_fasta(EX + 'NC_000913.faa')[1] + read_fasta(EX + 'NC_000915.faa')[1]
    lens = np.array([len(s) for s in seqs])
    n = len(seqs)
    size = decompose([int(l) + 2 for l in lens], N_SPLITS)     # the index's length column counts "\n\0"
    frm = [sum(size[:s]) for s in range(N_SPLITS)]
    L = min(MAX_SEQS, n)
    list_len = max(1, L // N_SPLITS + int(4 * math.sqrt(float(L) / float(N_SPLITS))))

    def index(sub):
        off = np.zeros(len(sub) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in sub])
        return ref.index(''.join(sub).encode(), off)          # k-mer threshold 112 = -s 5.7 at k = 6, masking on

    splits = []
    for s in range(N_SPLITS):
        ix = index(seqs[frm[s]:frm[s] + size[s]])
        splits.append((ix, ix.prefilter(int(lens.max()), max_hits=list_len)))
    whole_ix = index(seqs)
    whole = whole_ix.prefilter(int(lens.max()), max_hits=MAX_SEQS)

    def covered(q, t):
        return np.float32(lens[t]) / np.float32(lens[q]) >= COV_THR

    queries, raw_counts = [], []
    m_off, m_key, m_score, m_diag = [0], [], [], []
    u_off, u_key, u_score, u_diag = [0], [], [], []
    for q in SAMPLE:
        rows, raw = [], []
        for s in range(N_SPLITS):
            home = frm[s] <= q < frm[s] + size[s]
            ids, sc, dg, _ = splits[s][1].query(seqs[q], q - frm[s] if home else 0xFFFFFFFF)
            raw.append(len(ids))
            for t, score, d in zip(ids, sc, dg):
                t = int(t) + frm[s]                              # back to an id of the whole DB; key = id in this DB
                if covered(q, t):
                    rows.append((t, int(score), int(np.int16(np.uint16(d)))))
        rows.sort(key=lambda r: (-abs(r[1]), r[0]))              # compareHitsByScoreAndId
        queries.append(q)
        raw_counts.append(raw)
        m_key += [r[0] for r in rows]
        m_score += [r[1] for r in rows]
        m_diag += [r[2] for r in rows]
        m_off.append(len(m_key))
        ids, sc, dg, _ = whole.query(seqs[q], q)
        keep = [i for i, t in enumerate(ids) if covered(q, int(t))]
        u_key += [int(ids[i]) for i in keep]
        u_score += [int(sc[i]) for i in keep]
        u_diag += [int(np.int16(np.uint16(dg[i]))) for i in keep]
        u_off.append(len(u_key))

    raw_counts = np.array(raw_counts, np.uint32)
    m_off, u_off = np.array(m_off, np.uint64), np.array(u_off, np.uint64)
    merged_len = np.diff(m_off.astype(np.int64))
    differs = 0
    for i in range(len(queries)):
        a, b = int(m_off[i]), int(m_off[i + 1])
        c, d = int(u_off[i]), int(u_off[i + 1])
        if (m_key[a:b], m_score[a:b], m_diag[a:b]) != (u_key[c:d], u_score[c:d], u_diag[c:d]):
            differs += 1
    assert (raw_counts >= list_len).any(), 'no sampled (query, split) list is cut at the per-split length: change MAX_SEQS'
    assert (merged_len > MAX_SEQS).any(), 'no merged list is longer than --max-seqs: change MAX_SEQS'
    assert differs > 0, 'every merged list equals the unsplit list: change MAX_SEQS'
    np.savez_compressed(os.path.join(GOLD, 'split_vectors.npz'), n_splits=N_SPLITS, max_seqs=MAX_SEQS, list_len=list_len,
                        db_from=np.array(frm, np.uint64), db_size=np.array(size, np.uint64), queries=np.array(queries, np.uint32),
                        split_raw_count=raw_counts, merged_off=m_off, merged_key=np.array(m_key, np.uint32),
                        merged_score=np.array(m_score, np.int32), merged_diag=np.array(m_diag, np.int16), unsplit_off=u_off,
                        unsplit_key=np.array(u_key, np.uint32), unsplit_score=np.array(u_score, np.int32),
                        unsplit_diag=np.array(u_diag, np.int16))
    print('split', list(zip(frm, size)), 'list length', list_len, '|', len(queries), 'queries,', int((raw_counts >= list_len).sum()),
          'cut lists,', int((merged_len > MAX_SEQS).sum()), 'merged lists above --max-seqs,', differs, 'differ from the unsplit list,',
          int(merged_len.sum()), 'rows')


if __name__ == '__main__':
    main()
