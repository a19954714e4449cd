"""The graph half of the reference's `clust` module restated in Python (ClusteringAlgorithms::readInClusterData with
AlignmentSymmetry::findMissingLinks / addMissingLinks, M/src/clustering): what sd_clust_symmetrize computes on the GPU.  Checked against the
reference's own graphs in tests/test_clust.py; the GPU tests compare the kernel with it on graphs the golden file does not hold."""
import numpy as np


def symmetrize(row_off, elem, score):
    """CSR graph (row_off [n + 1], elem, score; rows in file order) -> (row_off, elem, score) of the symmetric graph: every row keeps its
    entries in input order, then gains one entry s for every input edge s -> c at position p of row s for which s is not among the INPUT
    entries of row c, in (s, p) order with score[s][p].  A row listing c twice appends twice; a self edge is never missing."""
    row_off = np.asarray(row_off, np.int64)
    elem = np.asarray(elem, np.int64)
    score = np.asarray(score, np.uint16)
    n = len(row_off) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_off))
    # (c, s) is an input edge iff c lists s
    have = np.unique(src * n + elem) if n else np.zeros(0, np.int64)
    rev = elem * n + src
    at = np.searchsorted(have, rev)
    at[at >= len(have)] = 0
    missing = have[at] != rev if len(have) else np.zeros(0, bool)
    m_src, m_dst, m_score = src[missing], elem[missing], score[missing]
    order = np.argsort(m_dst, kind='stable')   # the stream is in (s, p) order: a stable sort by destination keeps it per row
    m_src, m_dst, m_score = m_src[order], m_dst[order], m_score[order]
    add = np.bincount(m_dst, minlength=n) if n else np.zeros(0, np.int64)
    out_len = np.diff(row_off) + add
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(out_len, out=out_off[1:])
    out_elem = np.zeros(int(out_off[-1]), np.uint32)
    out_score = np.zeros(int(out_off[-1]), np.uint16)
    keep_at = out_off[src] + (np.arange(len(elem)) - row_off[src])
    out_elem[keep_at] = elem
    out_score[keep_at] = score
    add_off = np.zeros(n + 1, np.int64)
    np.cumsum(add, out=add_off[1:])
    add_at = out_off[m_dst] + np.diff(row_off)[m_dst] + (np.arange(len(m_dst)) - add_off[m_dst])
    out_elem[add_at] = m_src
    out_score[add_at] = m_score
    return out_off.astype(np.uint64), out_elem, out_score


def random_graph(n, n_edges, seed, self_edges=True):
    """a seeded graph of n rows and about n_edges one-way entries (rows of very different lengths with one hub, repeated targets, some rows empty)"""
    rng = np.random.default_rng(seed)
    weight = rng.random(n) ** 4
    weight[n // 3] = 0.08 * weight.sum()   # a hub
    src = np.sort(rng.choice(n, n_edges, p=weight / weight.sum()))
    dst = rng.integers(0, n, n_edges)
    if self_edges:
        first = np.flatnonzero(np.diff(np.concatenate([[-1], src])) != 0)
        dst[first] = src[first]
    row_off = np.zeros(n + 1, np.uint64)
    row_off[1:] = np.cumsum(np.bincount(src, minlength=n))
    return row_off, dst.astype(np.uint32), rng.integers(0, 65536, n_edges).astype(np.uint16)
