"""Thin Python mirror of the C ABI (include/spacedust_gpu.h): Host (CPU stages), Context (one GPU),
SeqSet / Target (data resident in HBM) and the three hot-path calls.  All compute happens in
libsdgpu.so; numpy only carries buffers."""
import ctypes as C

import numpy as np

from . import _lib
from .cpus import effective_cpus
from ._lib import SdError, ptr


def _check(ctx, rc, what):
    if rc != 0:
        msg = ''
        if ctx is not None:
            msg = _lib.load().sd_last_error(ctx).decode(errors='replace')
        raise SdError('%s failed (%d): %s' % (what, rc, msg))


class Host:
    """Host-side stages (sd_host_*): matrices, composition bias, target masking + index, E-values."""

    def __init__(self, threads=0):
        import os
        self.L = _lib.load()
        self.threads = threads or effective_cpus()
        h = C.c_void_p()
        _check(None, self.L.sd_host_create(self.threads, C.byref(h)), 'sd_host_create')
        self.h = h

    def matrix(self, which):
        m = np.zeros(441, np.int8)
        pb = np.zeros(21, np.float64)
        a2n = np.zeros(256, np.uint8)
        self.L.sd_host_matrix(self.h, which, ptr(m), ptr(pb), ptr(a2n))
        return m, pb, a2n

    def map_sequences(self, seqs):
        """list of ASCII protein strings -> (residues uint8, offsets uint64)"""
        lens = np.fromiter((len(s) for s in seqs), np.uint64, len(seqs))
        off = np.zeros(len(seqs) + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        blob = ''.join(seqs).encode()
        out = np.zeros(len(blob), np.uint8)
        self.L.sd_host_map_sequence(self.h, blob, len(blob), ptr(out))
        return out, off

    def comp_bias(self, residues, offsets, k=6):
        n = len(offsets) - 1
        sw = np.zeros(len(residues), np.int8)
        dg = np.zeros(len(residues), np.int8)
        km = np.zeros(len(residues), np.int16)
        self.L.sd_host_comp_bias(self.h, ptr(residues), ptr(offsets), n, k, ptr(sw), ptr(dg), ptr(km))
        return sw, dg, km

    def build_index(self, residues, offsets, k=6, kmer_thr=112, mask=True, mask_prob=0.9):
        return HostIndex(self, residues, offsets, k, kmer_thr, mask, mask_prob)

    def ext_matrix(self, word_len):
        sp = C.c_void_p()
        ip = C.c_void_p()
        n = C.c_uint32()
        _check(None, self.L.sd_host_ext_matrix(self.h, word_len, C.byref(sp), C.byref(ip), C.byref(n)), 'sd_host_ext_matrix')
        size = n.value
        sc = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_int16)), shape=(size * size,))
        ix = np.ctypeslib.as_array(C.cast(ip, C.POINTER(C.c_uint16)), shape=(size * size,))
        return sc, ix, size

    def kmer_threshold(self, sensitivity, k):
        return self.L.sd_host_kmer_threshold(sensitivity, k)

    def map_profiles(self, data, byte_offsets):
        """sd_host_map_profiles: profile DB entries (25 bytes per position) -> dict(letters, consensus, aln [P,21],
        sorted_score [P,20], sorted_index [P,20], offsets [n+1] in positions)"""
        data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        bo = np.ascontiguousarray(byte_offsets, np.uint64)
        n = len(bo) - 1
        total = int(bo[-1]) // 25
        out = dict(letters=np.zeros(total, np.uint8), consensus=np.zeros(total, np.uint8), aln=np.zeros((total, 21), np.int8),
                   sorted_score=np.zeros((total, 20), np.int16), sorted_index=np.zeros((total, 20), np.uint8),
                   offsets=np.zeros(n + 1, np.uint64))
        _check(None, self.L.sd_host_map_profiles(ptr(data), ptr(bo), n, ptr(out['letters']), ptr(out['consensus']),
                                                 ptr(out['aln']), ptr(out['sorted_score']), ptr(out['sorted_index']),
                                                 ptr(out['offsets'])), 'sd_host_map_profiles')
        used = int(out['offsets'][-1])   # profiles beyond --max-seq-len positions are cut (Sequence::mapProfile): trim the arrays
        if used < total:
            for k_ in ('letters', 'consensus', 'aln', 'sorted_score', 'sorted_index'):
                out[k_] = np.ascontiguousarray(out[k_][:used])
        return out

    def profile_kmer_threshold(self, sensitivity, k):
        return self.L.sd_host_profile_kmer_threshold(sensitivity, k)

    def auto_kmer_size(self, target_residues):
        return self.L.sd_host_auto_kmer_size(int(target_residues))

    def bin_size(self, db_size, l2=0):
        return self.L.sd_host_bin_size(db_size, l2)

    def split_plan(self, entry_lengths, n_splits, max_seqs=300, k=0, residues=None):
        """sd_host_split_plan: the target split of `prefilter --split N --split-mode 0`.  entry_lengths: the length column of the
        target DB's index (sequence length + 2) in key order; residues defaults to sum(entry_lengths - 2).
        Returns dict(db_from, db_size [n_splits], list_len, k)."""
        lens = np.ascontiguousarray(entry_lengths, np.uint64)
        if residues is None:
            residues = int(lens.sum()) - 2 * len(lens)
        db_from, db_size = np.zeros(max(n_splits, 1), np.uint64), np.zeros(max(n_splits, 1), np.uint64)
        list_len, k_out = C.c_uint64(), C.c_int()
        _check(None, self.L.sd_host_split_plan(ptr(lens), len(lens), n_splits, int(max_seqs), int(k), int(residues), ptr(db_from), ptr(db_size),
                                               C.byref(list_len), C.byref(k_out)), 'sd_host_split_plan')
        return dict(db_from=db_from, db_size=db_size, list_len=int(list_len.value), k=int(k_out.value))

    def lgamma_table(self, n):
        out = np.zeros(n, np.float64)
        self.L.sd_host_lgamma_table(ptr(out), n)
        return out

    def evalue(self, db_residues, score, qlen):
        return self.L.sd_host_evalue(db_residues, float(score), float(qlen))

    def bitscore(self, score):
        return self.L.sd_host_bitscore(float(score))

    def score_class(self, kernel, n, tl, shared, wide_row_limit):
        """sd_selftest_score_class: (class, profile scope) of a Smith-Waterman score task of n rows and tl columns on kernel
        0 (packed), 1 (packed, wide row code) or 2 (int32), from the library's class table; needs no GPU"""
        klass = C.c_uint32()
        if not hasattr(self, '_scope_buf'):
            self._scope_buf = C.create_string_buffer(48)
        _check(None, self.L.sd_selftest_score_class(kernel, n, tl, int(shared), wide_row_limit, C.byref(klass), self._scope_buf, 48),
               'sd_selftest_score_class')
        return klass.value, self._scope_buf.value.decode()


def uncompress_cigar(c):
    """Matcher::uncompressAlignment (Matcher.cpp:187-201)"""
    out, n = [], 0
    for ch in c:
        if '0' <= ch <= '9':
            n = n * 10 + ord(ch) - 48
        else:
            out.append(ch * (n if n else 1))
            n = 0
    return ''.join(out)


def swapresults(entries, first_db_residues, second_db_keys, eval_thr=0.001, gap_open=11, gap_extend=1, want_counts=False):
    """sd_host_swapresults: a result DB keyed by query re-keyed by target (the `swapresults` module without the DB files).
    entries: dict key -> entry text (bytes) or a list of (key, bytes); first_db_residues: the amino-acid size of the module's first DB
    argument; second_db_keys: the keys of its second.  Returns dict key -> bytes (empty entries included) and, with want_counts, the
    rows read and written."""
    L = _lib.load()
    items = sorted(entries.items()) if isinstance(entries, dict) else list(entries)
    keys = np.array([k for k, _ in items], np.uint32)
    off = np.zeros(len(items) + 1, np.uint64)
    if items:
        np.cumsum([len(t) for _, t in items], out=off[1:])
    blob = b''.join(bytes(t) for _, t in items) + b'\0'
    tkeys = np.ascontiguousarray(second_db_keys, np.uint32)
    h = C.c_void_p()
    rc = L.sd_host_swapresults(len(items), ptr(keys), ptr(off), blob, int(first_db_residues), ptr(tkeys), len(tkeys), float(eval_thr),
                               gap_open, gap_extend, C.byref(h))
    _check(None, rc, 'sd_host_swapresults')
    try:
        n, rows_in, rows_out = C.c_uint32(), C.c_uint64(), C.c_uint64()
        k_p, o_p, t_p = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(None, L.sd_swap_get(h, C.byref(n), C.byref(k_p), C.byref(o_p), C.byref(t_p), C.byref(rows_in), C.byref(rows_out)), 'sd_swap_get')
        out = {}
        if n.value:
            k = np.ctypeslib.as_array(C.cast(k_p, C.POINTER(C.c_uint32)), (n.value,))
            o = np.ctypeslib.as_array(C.cast(o_p, C.POINTER(C.c_uint64)), (n.value + 1,))
            text = C.string_at(t_p, int(o[-1])) if int(o[-1]) else b''
            for i in range(n.value):
                out[int(k[i])] = text[int(o[i]):int(o[i + 1])]
    finally:
        L.sd_swap_destroy(h)
    return (out, rows_in.value, rows_out.value) if want_counts else out


def result2profile(q_letters, q_off, edge_off, edge_t, edge_qstart, edge_tstart, backtraces, t_residues, t_off, **kw):
    """sd_r2p_batch: profiles (25 bytes per position, bytes object) of nQ centre sequences from their alignments"""
    L = _lib.load()
    h = C.c_void_p()
    _check(None, L.sd_r2p_create(C.byref(h)), 'sd_r2p_create')
    p = _lib.R2pParams()
    p.filterMsa, p.filterMinEnable, p.filterMaxSeqId = kw.get('filter_msa', 1), kw.get('filter_min_enable', 0), kw.get('max_seq_id', 0.9)
    p.qid, p.qsc, p.covMSAThr, p.Ndiff = kw.get('qid', '0.0').encode(), kw.get('qsc', -20.0), kw.get('cov', 0.0), kw.get('ndiff', 1000)
    p.pcMode, p.pca, p.pcb, p.wg = 0, kw.get('pca', 1.1), kw.get('pcb', 4.1), kw.get('wg', 0)
    p.compBiasCorr, p.maskProfile, p.maskProb = kw.get('comp_bias', 1), kw.get('mask_profile', 1), kw.get('mask_prob', 0.9)
    q_letters = np.ascontiguousarray(q_letters, np.uint8)
    q_off = np.ascontiguousarray(q_off, np.uint64)
    edge_off = np.ascontiguousarray(edge_off, np.uint64)
    edge_t = np.ascontiguousarray(edge_t, np.uint32)
    qs = np.ascontiguousarray(edge_qstart, np.int32)
    ts = np.ascontiguousarray(edge_tstart, np.int32)
    bt_off = np.zeros(len(backtraces) + 1, np.uint64)
    np.cumsum([len(b) for b in backtraces], out=bt_off[1:])
    pool = np.frombuffer((''.join(backtraces) + ' ').encode(), np.uint8).copy()
    t_residues = np.ascontiguousarray(t_residues, np.uint8)
    t_off = np.ascontiguousarray(t_off, np.uint64)
    out = np.zeros(int(q_off[-1]) * 25 + 1, np.uint8)
    ctx = kw.get('ctx')   # a Context: sd_r2p_batch_device (sequence weights on the GPU); None: the host implementation
    if ctx is not None:
        rc = L.sd_r2p_batch_device(ctx.h, h, C.byref(p), len(q_off) - 1, ptr(q_letters), ptr(q_off), ptr(edge_off), ptr(edge_t), ptr(qs),
                                   ptr(ts), ptr(pool), ptr(bt_off), ptr(t_residues), ptr(t_off), ptr(out), None)
    else:
        rc = L.sd_r2p_batch(h, C.byref(p), len(q_off) - 1, ptr(q_letters), ptr(q_off), ptr(edge_off), ptr(edge_t), ptr(qs), ptr(ts), ptr(pool),
                            ptr(bt_off), ptr(t_residues), ptr(t_off), ptr(out), None)
    L.sd_r2p_destroy(h)
    _check(ctx.h if ctx is not None else None, rc, 'sd_r2p_batch')
    return out[:-1].tobytes()


def r2p_realign(ctx, host, q_letters, q_off, edge_off, edge_t, t_residues, t_off, realign=None, edge_qstart=None, edge_tstart=None,
                backtraces=None, comp_bias=1, targets=None, pool_cap=None, retry=True, want_stats=False):
    """sd_r2p_realign: result2profile's alignment of the edges that carry none (matrix with score bias -0.2, the centre's composition
    bias against it, no gates), in the layout of `result2profile` above.  realign: per edge, nonzero = realign (None: every edge); the
    others keep edge_qstart / edge_tstart / backtraces (a list of strings, '' for the marked ones).  targets: a SeqSet of t_residues on
    ctx (None: uploaded by the call).  pool_cap: the first guess of the backtrace pool (None: the library's bound); with retry, a call
    that reports SD_ENOMEM is repeated once with the capacity it names.  Returns (qstart int32, tstart int32, backtraces list of str)
    and, with want_stats, the number of calls made."""
    L = _lib.load()
    q_letters = np.ascontiguousarray(np.concatenate([np.asarray(q_letters, np.uint8), np.zeros(1, np.uint8)]))
    q_off = np.ascontiguousarray(q_off, np.uint64)
    edge_off = np.ascontiguousarray(edge_off, np.uint64)
    n_e = int(edge_off[-1])
    edge_t = np.ascontiguousarray(np.concatenate([np.asarray(edge_t, np.uint32), np.zeros(1, np.uint32)]))
    t_residues = np.ascontiguousarray(t_residues, np.uint8)
    t_off = np.ascontiguousarray(t_off, np.uint64)
    flags = None if realign is None else np.ascontiguousarray(np.concatenate([np.asarray(realign, np.uint8), np.zeros(1, np.uint8)]))
    qs = np.zeros(n_e + 1, np.int32)
    ts = np.zeros(n_e + 1, np.int32)
    if edge_qstart is not None:
        qs[:n_e] = edge_qstart
        ts[:n_e] = edge_tstart
    held = list(backtraces) if backtraces is not None else [''] * n_e
    bt_off0 = np.zeros(n_e + 1, np.uint64)
    if n_e:
        np.cumsum([len(b) for b in held], out=bt_off0[1:])
    text = ''.join(held).encode()
    need, bad = C.c_uint64(), C.c_uint64()
    cap = pool_cap
    calls = 0
    while True:
        if cap is None:   # the bound itself, formed as the library forms *btNeed: held backtraces + sum(qLen + tLen) of the marked pairs
            bound_cap = len(text) + 1
            for q in range(len(q_off) - 1):
                for e in range(int(edge_off[q]), int(edge_off[q + 1])):
                    if flags is None or flags[e]:
                        t = int(edge_t[e])
                        bound_cap += int(q_off[q + 1] - q_off[q]) + int(t_off[t + 1] - t_off[t])
            cap = bound_cap + 64
        cap = max(int(cap), len(text) + 1)
        pool = np.zeros(cap + 1, np.uint8)
        pool[:len(text)] = np.frombuffer(text, np.uint8)
        bt_off = bt_off0.copy()
        calls += 1
        rc = L.sd_r2p_realign(ctx.h, host.h, len(q_off) - 1, ptr(q_letters), ptr(q_off), ptr(edge_off), ptr(edge_t), ptr(flags), int(comp_bias),
                              targets.h if targets is not None else None, ptr(t_residues), ptr(t_off), len(t_off) - 1, ptr(qs), ptr(ts),
                              ptr(pool), cap, ptr(bt_off), C.byref(need), C.byref(bad))
        if rc == _lib.SD_ENOMEM and retry and calls == 1:
            cap = need.value
            continue
        if rc == _lib.SD_EINVAL and bad.value != 2 ** 64 - 1:
            raise SdError('sd_r2p_realign: the alignment of edge %d scores 0 (the reference leaves its start positions unset)' % bad.value)
        _check(ctx.h, rc, 'sd_r2p_realign')
        break
    raw = pool.tobytes()
    bts = [raw[int(bt_off[e]):int(bt_off[e + 1])].decode() for e in range(n_e)]
    out = (qs[:n_e].copy(), ts[:n_e].copy(), bts)
    return out + (calls,) if want_stats else out


def profile_consensus(host, data, byte_offsets, max_seq_len=65535):
    """sd_host_profile_consensus: profile DB entries (25 bytes per position, byte_offsets[n+1]) -> list of bytes, one per entry: the
    consensus letters and a newline (profile2consensus' entries)"""
    data = np.ascontiguousarray(np.frombuffer(bytes(data) + b'\0', np.uint8))
    bo = np.ascontiguousarray(byte_offsets, np.uint64)
    n = len(bo) - 1
    lens = np.minimum((bo[1:] - bo[:-1]) // 25, np.uint64(max_seq_len)).astype(np.int64)
    text = np.zeros(int(lens.sum()) + n + 1, np.uint8)
    off = np.zeros(n + 1, np.uint64)
    _check(None, host.L.sd_host_profile_consensus(host.h, ptr(data), ptr(bo), n, int(max_seq_len), ptr(text), ptr(off)), 'sd_host_profile_consensus')
    raw = text.tobytes()
    return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]


def r2p_weights(tasks, ctx=None):
    """sd_selftest_r2p_weights: the weights stage of result2profile alone on alignments given as uint8 cell matrices [nRows, L]
    (row 0 the centre; 0..19 residue, 20 any, 21 gap) -- on the device through sd_r2p_batch_device's staging with a Context, by
    the host implementation without.  Returns [(freq float32 [L, 20], eff float32 [L])] per task"""
    L = _lib.load()
    mats = [np.ascontiguousarray(m, np.uint8) for m in tasks]
    assert all(m.ndim == 2 for m in mats)
    n_rows = np.array([m.shape[0] for m in mats], np.uint32)
    cols = np.array([m.shape[1] for m in mats], np.uint32)
    cells = np.concatenate([m.ravel() for m in mats] + [np.zeros(1, np.uint8)])
    total = int(cols.astype(np.int64).sum())
    freq = np.zeros((total + 1, 20), np.float32)
    eff = np.zeros(total + 1, np.float32)
    h = ctx.h if ctx is not None else None
    _check(h, L.sd_selftest_r2p_weights(h, len(mats), ptr(n_rows), ptr(cols), ptr(cells), ptr(freq), ptr(eff)), 'sd_selftest_r2p_weights')
    at = np.concatenate([[0], np.cumsum(cols.astype(np.int64))])
    return [(freq[at[k]:at[k + 1]].copy(), eff[at[k]:at[k + 1]].copy()) for k in range(len(mats))]


def mask_on_device(ctx, host, residues, offsets, mask_prob=0.9):
    """sd_selftest_mask: the masking phase of sd_target_build alone (no index) -> (masked residues uint8, masked count)"""
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    assert len(residues) == int(offsets[-1])
    out = np.zeros(len(residues) + 1, np.uint8)
    n = C.c_uint64()
    _check(ctx.h, ctx.L.sd_selftest_mask(ctx.h, host.h, ptr(residues) if len(residues) else ptr(out), ptr(offsets), len(offsets) - 1,
                                         float(mask_prob), ptr(out), C.byref(n)), 'sd_selftest_mask')
    return out[:len(residues)], int(n.value)


class HostIndex:
    def __init__(self, host, residues, offsets, k, kmer_thr, mask, mask_prob):
        self.host = host
        self.k = k
        self.kmer_thr = kmer_thr
        self.n = len(offsets) - 1
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        residues = np.ascontiguousarray(residues, np.uint8)
        h = C.c_void_p()
        _check(None, host.L.sd_host_index_build(host.h, ptr(residues), ptr(self.offsets), self.n, k, kmer_thr,
                                                1 if mask else 0, mask_prob, C.byref(h)), 'sd_host_index_build')
        self.h = h
        ts, ne, mk = C.c_uint64(), C.c_uint64(), C.c_uint64()
        host.L.sd_host_index_info(h, C.byref(ts), C.byref(ne), C.byref(mk))
        self.table_size, self.n_entries, self.masked_residues = ts.value, ne.value, mk.value
        po, ps, pp, pm = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        host.L.sd_host_index_arrays(h, C.byref(po), C.byref(ps), C.byref(pp), C.byref(pm))
        self.kmer_offsets = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint32)), shape=(self.table_size + 1,))
        # wide index (>= 2^32 entries): kmer_offsets[i] is relative to block_base[i >> 16]; None otherwise
        pb, nb = C.c_void_p(), C.c_uint64()
        host.L.sd_host_index_block_base(h, C.byref(pb), C.byref(nb))
        self.block_base = np.ctypeslib.as_array(C.cast(pb, C.POINTER(C.c_uint64)), shape=(nb.value,)) if pb.value else None
        ne1 = max(self.n_entries, 1)
        self.entry_seq = np.ctypeslib.as_array(C.cast(ps, C.POINTER(C.c_uint32)), shape=(ne1,))[:self.n_entries]
        self.entry_pos = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_uint16)), shape=(ne1,))[:self.n_entries]
        tot = max(int(self.offsets[-1]), 1)
        self.masked = np.ctypeslib.as_array(C.cast(pm, C.POINTER(C.c_uint8)), shape=(tot,))[:int(self.offsets[-1])]

    def __del__(self):
        try:
            self.host.L.sd_host_index_destroy(self.h)
        except Exception:
            pass


class DeviceArray:
    """a device-resident array (a torch tensor) where the C ABI takes a pointer that may live on the device: ptr(x) yields
    its data pointer, the tensor is kept alive"""

    class _P:
        def __init__(self, t):
            self.t = t

        def data_as(self, _):
            return C.c_void_p(self.t.data_ptr())

    def __init__(self, tensor, n_elements):
        self.tensor, self.n = tensor, int(n_elements)
        self.ctypes = DeviceArray._P(tensor)
        self.nbytes = int(tensor.numel() * tensor.element_size())

    def __len__(self):
        return self.n


class IndexArrays:
    """A target index that exists already as arrays (received from another rank, read from an index file): the attributes
    of HostIndex that Target and ClusterSearch(index=...) read"""

    def __init__(self, k, kmer_thr, seq_offsets, kmer_offsets, entry_seq, entry_pos, masked, masked_residues=0, block_base=None):
        self.k, self.kmer_thr = int(k), int(kmer_thr)
        host = lambda a, dt: a if isinstance(a, DeviceArray) else np.ascontiguousarray(a, dt)   # device arrays pass through
        self.block_base = None if block_base is None else host(block_base, np.uint64)
        self.offsets = np.ascontiguousarray(seq_offsets, np.uint64)
        self.n = len(self.offsets) - 1
        self.kmer_offsets = host(kmer_offsets, np.uint32)
        self.entry_seq = host(entry_seq, np.uint32)
        self.entry_pos = host(entry_pos, np.uint16)
        self.masked = host(masked, np.uint8)
        self.table_size, self.n_entries, self.masked_residues = len(self.kmer_offsets) - 1, len(self.entry_seq), int(masked_residues)


class Context:
    """One GPU (sd_ctx).  Raises SdError when no HIP device is visible -- there is no CPU fallback."""

    def __init__(self, device=0, priority=0):
        self.L = _lib.load()
        h = C.c_void_p()
        rc = self.L.sd_ctx_create_prio(device, priority, C.byref(h))
        if rc != 0:
            raise SdError('sd_ctx_create(%d) failed (%d): no usable HIP device; the HIP path has no CPU fallback'
                          % (device, rc))
        self.h = h
        self.device_index = device

    def device_name(self):
        b = C.create_string_buffer(256)
        self.L.sd_device_name(self.h, b, 256)
        return b.value.decode()

    def synchronize(self):
        _check(self.h, self.L.sd_synchronize(self.h), 'sd_synchronize')

    def last_error(self):
        return self.L.sd_last_error(self.h).decode(errors='replace')

    def device_memory(self):
        """(free, total) bytes of this context's device"""
        f, t = C.c_uint64(), C.c_uint64()
        _check(self.h, self.L.sd_device_memory(self.h, C.byref(f), C.byref(t)), 'sd_device_memory')
        return f.value, t.value

    def workspace_report(self, top=8):
        """(device bytes, pinned host bytes, [(key, bytes)] of the largest device workspaces) of this context"""
        d, p = C.c_uint64(), C.c_uint64()
        buf = C.create_string_buffer(1 << 16)
        _check(self.h, self.L.sd_workspace_report(self.h, C.byref(d), C.byref(p), buf, len(buf)), 'sd_workspace_report')
        rows = [ln.rsplit(' ', 1) for ln in buf.value.decode().splitlines() if ln]
        return d.value, p.value, [(k, int(v)) for k, v in rows[:top]]

    def profile(self, on=True):
        self.L.sd_profile_enable(self.h, 1 if on else 0)
        self.L.sd_profile_reset(self.h)

    def profile_report(self):
        b = C.create_string_buffer(4096)
        self.L.sd_profile_names(self.h, b, 4096)
        out = {}
        for name in filter(None, b.value.decode().split(',')):
            ms, cnt = C.c_double(), C.c_uint64()
            self.L.sd_profile_get(self.h, name.encode(), C.byref(ms), C.byref(cnt))
            out[name] = (ms.value, cnt.value)
        return out

    def seqset(self, residues, offsets, sw_bias=None):
        return SeqSet(self, residues, offsets, sw_bias)

    def comp_bias(self, host, residues, offsets, k=6):
        """sd_comp_bias_batch: the (sw int8, diag int8, kmer int16) bias arrays of Host.comp_bias, formed on the device"""
        residues = np.ascontiguousarray(residues, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sw = np.zeros(len(residues), np.int8)
        dg = np.zeros(len(residues), np.int8)
        km = np.zeros(len(residues), np.int16)
        _check(self.h, self.L.sd_comp_bias_batch(self.h, host.h, ptr(residues), ptr(offsets), len(offsets) - 1, k, ptr(sw), ptr(dg),
                                                 ptr(km)), 'sd_comp_bias_batch')
        return sw, dg, km

    def profileset(self, letters, offsets, aln):
        """profile queries for sw_align (sd_profileset_create): query letters + int8 alignment profile [P, 21]"""
        return SeqSet(self, letters, offsets, None, aln=aln)

    def sw_params(self, matrix, db_residues, sw_mode=2, eval_thr=10.0, cov_mode=2, cov_thr=0.8, gap_open=11,
                  gap_extend=1):
        p = _lib.SwParams()
        p.gapOpen, p.gapExtend = gap_open, gap_extend
        for i in range(441):
            p.matrix[i] = int(matrix[i])
        p.covMode, p.covThr, p.evalThr, p.swMode, p.dbResidues = cov_mode, cov_thr, eval_thr, sw_mode, db_residues
        return p

    def sw_score(self, par, queries, targets, pair_q, pair_t, lanes=32, reverse=False, q_end=None, t_end=None):
        pq = np.ascontiguousarray(pair_q, np.uint32)
        pt = np.ascontiguousarray(pair_t, np.uint32)
        out = np.zeros((len(pq), 3), np.int32)
        qe = np.ascontiguousarray(q_end, np.int32) if q_end is not None else None
        te = np.ascontiguousarray(t_end, np.int32) if t_end is not None else None
        _check(self.h, self.L.sd_sw_score_batch(self.h, C.byref(par), queries.h, targets.h, len(pq), ptr(pq), ptr(pt),
                                                lanes, 1 if reverse else 0, ptr(qe), ptr(te), ptr(out)),
               'sd_sw_score_batch')
        return out

    def sw_align(self, par, queries, targets, pair_q, pair_t, identity=None, bt_cap=None, hostpath=False, reuse=False,
                 compact=False, diag=None):
        """sd_sw_align_batch.  bt_cap: capacity of the backtrace pool (default: a generous guess, grown to the exact
        bound sum(qLen + tLen) if the library reports SD_ENOMEM).  reuse=True hands out views of two alternating
        context-owned buffers instead of fresh arrays (valid until the next-but-one call).  compact=True
        (sd_sw_align_batch_compact) returns (pair indices, their records, pool) for the reportable pairs only."""
        pq = np.ascontiguousarray(pair_q, np.uint32)
        pt = np.ascontiguousarray(pair_t, np.uint32)
        n = len(pq)
        idt = np.ascontiguousarray(identity, np.uint8) if identity is not None else np.zeros(n, np.uint8)
        fn = self.L.sd_sw_align_batch_hostpath if hostpath else self.L.sd_sw_align_batch
        exact_cap = None
        if bt_cap is None:
            bt_cap = max(1 << 20, 96 * n)
        if reuse:
            # one flip per call: a retry after SD_ENOMEM must stay on this call's slot -- the other one still holds the
            # previous call's records and backtraces, which the caller may be reading (pipeline.py aggregates them
            # asynchronously)
            self._flip = 1 - getattr(self, '_flip', 0)
        while True:
            if reuse:
                bufs = self.__dict__.setdefault('_align_bufs', [None, None])
                b = bufs[self._flip]
                if b is None or len(b[0]) < n or len(b[1]) < bt_cap:
                    b = (np.empty(max(n, int(1.25 * (len(b[0]) if b else 0))), _lib.SW_RESULT_DTYPE),
                         np.empty(max(bt_cap, int(1.25 * (len(b[1]) if b else 0))), np.uint8))
                    bufs[self._flip] = b
                res, pool = b[0][:n], b[1]
            else:
                res = np.zeros(n, _lib.SW_RESULT_DTYPE)
                pool = np.zeros(bt_cap, np.uint8)
            used = C.c_uint64()
            if compact:
                if not hasattr(self, '_cidx') or len(self._cidx[0]) < n:
                    self._cidx = [np.empty(int(1.25 * n) + 1, np.uint32), np.empty(int(1.25 * n) + 1, np.uint32)]
                cidx = self._cidx[getattr(self, '_flip', 0)] if reuse else np.empty(n, np.uint32)
                n_out = C.c_uint32()
                if diag is not None:   # the prefilter's diagonals: sd_sw_align_batch_compact_diag (same results)
                    dg = np.ascontiguousarray(diag, np.uint16)
                    rc = self.L.sd_sw_align_batch_compact_diag(self.h, C.byref(par), queries.h, targets.h, n, ptr(pq), ptr(pt), ptr(dg),
                                                               ptr(idt), ptr(cidx), ptr(res), C.byref(n_out), ptr(pool), len(pool),
                                                               C.byref(used))
                else:
                    rc = self.L.sd_sw_align_batch_compact(self.h, C.byref(par), queries.h, targets.h, n, ptr(pq), ptr(pt), ptr(idt),
                                                          ptr(cidx), ptr(res), C.byref(n_out), ptr(pool), len(pool), C.byref(used))
            else:
                rc = fn(self.h, C.byref(par), queries.h, targets.h, n, ptr(pq), ptr(pt), ptr(idt), ptr(res), ptr(pool),
                        len(pool), C.byref(used))
            if rc == _lib.SD_ENOMEM and exact_cap is None:
                ql = (queries.offsets[pq + 1] - queries.offsets[pq]).astype(np.int64)
                tl = (targets.offsets[pt + 1] - targets.offsets[pt]).astype(np.int64)
                exact_cap = bt_cap = (2 if getattr(self, '_cigar_pool', False) else 1) * int((ql + tl).sum()) + 64
                continue
            _check(self.h, rc, 'sd_sw_align_batch')
            if compact:
                return cidx[:n_out.value], res[:n_out.value], pool[:used.value]
            return res, pool[:used.value]

    def sw_align_alt(self, par, queries, targets, seed_q, seed_t, t_start, t_end, max_alt, identity=None, seq_id_thr=0.0,
                     aln_len_thr=0, seq_id_mode=0, bt_cap=None):
        """sd_sw_align_alt_batch: the alternative alignments of `align --alt-ali max_alt` for seeds (query, target, accepted
        target interval [t_start, t_end]).  Returns (records [n_seeds, max_alt], counts [n_seeds], pool): records[s, :counts[s]]
        are seed s's alternatives in round order."""
        sq = np.ascontiguousarray(seed_q, np.uint32)
        st = np.ascontiguousarray(seed_t, np.uint32)
        tb = np.ascontiguousarray(t_start, np.int32)
        te = np.ascontiguousarray(t_end, np.int32)
        n = len(sq)
        assert len(st) == len(tb) == len(te) == n
        idt = np.ascontiguousarray(identity, np.uint8) if identity is not None else None
        ql = (queries.offsets[sq.astype(np.int64) + 1] - queries.offsets[sq]).astype(np.int64)
        tl = (targets.offsets[st.astype(np.int64) + 1] - targets.offsets[st]).astype(np.int64)
        exact = (2 if getattr(self, '_cigar_pool', False) else 1) * int(max_alt) * int((ql + tl).sum()) + 64
        if bt_cap is None:
            bt_cap = min(exact, max(1 << 20, 2 * int((ql + tl).sum()) + 64))
        res = np.zeros((n, int(max_alt)), _lib.SW_RESULT_DTYPE)
        cnt = np.zeros(n, np.uint32)
        while True:
            pool = np.zeros(bt_cap, np.uint8)
            used = C.c_uint64()
            rc = self.L.sd_sw_align_alt_batch(self.h, C.byref(par), queries.h, targets.h, n, ptr(sq), ptr(st), ptr(tb), ptr(te), ptr(idt),
                                              int(max_alt), float(seq_id_thr), int(aln_len_thr), int(seq_id_mode), ptr(res), ptr(cnt),
                                              ptr(pool), len(pool), C.byref(used))
            if rc == _lib.SD_ENOMEM and bt_cap < exact:
                bt_cap = exact
                continue
            _check(self.h, rc, 'sd_sw_align_alt_batch')
            return res, cnt, pool[:used.value]

    def sw_alt_stats(self):
        """(seed groups, alignments run, bytes the mask kernel wrote) of the last sw_align_alt"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.L.sd_sw_alt_last_stats(self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def letterset(self, host, seqs):
        """a SeqSet of ASCII sequences (str or bytes) that also carries their letters (sd_seqset_set_letters): what
        rescore_diagonal takes"""
        blobs = [x.encode() if isinstance(x, str) else bytes(x) for x in seqs]
        off = np.zeros(len(blobs) + 1, np.uint64)
        np.cumsum(np.fromiter((len(b) for b in blobs), np.uint64, len(blobs)), out=off[1:])
        blob = b''.join(blobs)
        res = np.zeros(len(blob), np.uint8)
        host.L.sd_host_map_sequence(host.h, blob, len(blob), ptr(res))
        s = SeqSet(self, res, off, None)
        s.set_letters(blob)
        return s

    def rescore_diagonal(self, host, queries, targets, hit_q, hit_t, hit_diag, mode=2):
        """sd_rescore_diagonal_batch: DistanceCalculator::computeUngappedAlignment for every (query, target, 16-bit diagonal) hit.
        queries / targets: SeqSets with letters (letterset / SeqSet.set_letters); hit_diag: the prefilter row's diagonal (negative
        values are taken through an unsigned short, as the reference does).  Returns a RESCORE_DTYPE record per hit."""
        m, _, a2n = host.matrix(0)
        par = _lib.RescoreParams()
        par.mode = int(mode)
        C.memmove(par.matrix, m.ctypes.data, 441)
        C.memmove(par.aa2num, a2n.ctypes.data, 256)
        hq = np.ascontiguousarray(hit_q, np.uint32)
        ht = np.ascontiguousarray(hit_t, np.uint32)
        hd = np.ascontiguousarray(np.asarray(hit_diag, np.int64) & 0xFFFF, np.uint16)
        assert len(hq) == len(ht) == len(hd)
        out = np.zeros(len(hq), _lib.RESCORE_DTYPE)
        _check(self.h, self.L.sd_rescore_diagonal_batch(self.h, C.byref(par), queries.h, targets.h, len(hq), ptr(hq), ptr(ht), ptr(hd),
                                                        ptr(out)), 'sd_rescore_diagonal_batch')
        return out

    def set_cigar_pool(self, on=True):
        """sd_sw_set_cigar_pool: the alignment calls return run-length text (Matcher::compressAlignment's output) in the pool;
        a record's text is pool[btOffset : btOffset + (flags >> 8)]"""
        _check(self.h, self.L.sd_sw_set_cigar_pool(self.h, 1 if on else 0), 'sd_sw_set_cigar_pool')
        self._cigar_pool = bool(on)

    def set_narrow_final(self, on=True):
        """sd_sw_set_narrow_final: a pair whose byte score saturates is rerun on the wide kernels only when the narrow forward
        pass reports 1023 (or the pair skipped that pass); same records, fewer launches and cells"""
        _check(self.h, self.L.sd_sw_set_narrow_final(self.h, 1 if on else 0), 'sd_sw_set_narrow_final')

    def set_shared_start(self, on=True):
        """sd_sw_set_shared_start: the narrow start-position tasks of a query of 129 .. 768 residues run as suffixes of one profile
        of the whole reversed query (scopes sw_score_pk.s_seg*); same records"""
        _check(self.h, self.L.sd_sw_set_shared_start(self.h, 1 if on else 0), 'sd_sw_set_shared_start')

    def set_group16(self, on=True):
        """sd_sw_set_group16: the paired forward score tasks of 129 .. 448 query rows run on 16-lane groups, four task pairs of one
        query per wavefront (same records, scopes and launch counts; off by default)"""
        _check(self.h, self.L.sd_sw_set_group16(self.h, 1 if on else 0), 'sd_sw_set_group16')

    def sw_download_bytes(self):
        a, b = C.c_uint64(), C.c_uint64()
        self.L.sd_sw_download_bytes(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def sw_cells(self):
        f, r, t = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.L.sd_sw_last_cells(self.h, C.byref(f), C.byref(r), C.byref(t))
        return f.value, r.value, t.value

    def __del__(self):
        try:
            h, self.h = self.h, None   # (sets and targets that the collector finalises after their context see it gone)
            if h:
                self.L.sd_ctx_destroy(h)
        except Exception:
            pass


class SeqSet:
    def __init__(self, ctx, residues, offsets, sw_bias, aln=None):
        self.ctx = ctx
        self.residues = np.ascontiguousarray(residues, np.uint8)
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        self.n = len(self.offsets) - 1
        b = np.ascontiguousarray(sw_bias, np.int8) if sw_bias is not None else None
        h = C.c_void_p()
        if aln is not None:
            a = np.ascontiguousarray(aln, np.int8)
            assert a.size == len(self.residues) * 21
            _check(ctx.h, ctx.L.sd_profileset_create(ctx.h, ptr(self.residues), ptr(self.offsets), self.n, ptr(a), C.byref(h)),
                   'sd_profileset_create')
        else:
            _check(ctx.h, ctx.L.sd_seqset_create(ctx.h, ptr(self.residues), ptr(self.offsets), self.n, ptr(b), C.byref(h)),
                   'sd_seqset_create')
        self.h = h

    def set_letters(self, letters):
        """sd_seqset_set_letters: the DB's bytes of the same sequences, laid out like the residues"""
        b = np.frombuffer(bytes(letters), np.uint8) if not isinstance(letters, np.ndarray) else np.ascontiguousarray(letters, np.uint8)
        assert len(b) == len(self.residues)
        _check(self.ctx.h, self.ctx.L.sd_seqset_set_letters(self.h, ptr(b) if len(b) else ptr(np.zeros(1, np.uint8))), 'sd_seqset_set_letters')

    def __del__(self):
        # a set is destroyed before its context (include/spacedust_gpu.h): its buffers go back to the context's pool.  The
        # cycle collector may finalise the context first (both held by the traceback of a failed test): nothing to return to then
        try:
            if self.ctx.h:
                self.ctx.L.sd_seqset_destroy(self.h)
        except Exception:
            pass


class Target:
    """Target side of the prefilter resident in HBM (sd_target): k-mer index, masked lookup, 3-mer tables."""

    def __init__(self, ctx, host, index):
        self.ctx, self.host, self.index = ctx, host, index
        s2, i2, _ = host.ext_matrix(2)
        s3, i3, _ = host.ext_matrix(3)
        h = C.c_void_p()
        bb = getattr(index, 'block_base', None)
        _check(ctx.h, ctx.L.sd_target_create_wide(ctx.h, index.k, ptr(index.kmer_offsets), ptr(bb) if bb is not None else None,
                                                  ptr(index.entry_seq), ptr(index.entry_pos), index.n_entries, ptr(index.masked),
                                                  ptr(index.offsets), index.n, ptr(s2), ptr(i2), ptr(s3), ptr(i3),
                                                  C.byref(h)), 'sd_target_create')
        self.h = h
        self.n = index.n

    @classmethod
    def build_on_device(cls, ctx, host, residues, offsets, k=6, kmer_thr=112, mask=True, mask_prob=0.9):
        """sd_target_build: masking, k-mer collection and list construction on the GPU (no host index); k = 5, 6 or 7"""
        self = cls.__new__(cls)
        self.ctx, self.host, self.index = ctx, host, None
        residues = np.ascontiguousarray(residues, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        s2, i2, _ = host.ext_matrix(2)
        s3, i3, _ = host.ext_matrix(3)
        lr = np.zeros(441, np.float64)
        self_score = np.zeros(21, np.int8)
        _check(None, host.L.sd_host_index_tables(host.h, ptr(lr), ptr(self_score)), 'sd_host_index_tables')
        h = C.c_void_p()
        stats = np.zeros(4, np.uint64)
        _check(ctx.h, ctx.L.sd_target_build(ctx.h, k, kmer_thr, 1 if mask else 0, mask_prob, ptr(residues), ptr(offsets), len(offsets) - 1,
                                            ptr(lr), ptr(self_score), ptr(s2), ptr(i2), ptr(s3), ptr(i3), C.byref(h), ptr(stats)),
               'sd_target_build')
        self.h = h
        self.n = len(offsets) - 1
        self.k = k
        self.total = int(offsets[-1])
        self.build_stats = dict(entries=int(stats[0]), masked_residues=int(stats[1]), passes=int(stats[2]), records=int(stats[3]))
        return self

    @classmethod
    def build_profile_on_device(cls, ctx, host, prof, k=6, kmer_thr=None):
        """sd_target_build_profile: the similar-k-mer index of a profile target DB, built on the GPU (k = 5 or 6).  prof: the dict
        Host.map_profiles returns; kmer_thr: the profile threshold (default: Host.profile_kmer_threshold(4.0, k)).  Sequence
        queries (api.prefilter) look up their own k-mers only against it; api.prefilter_profile refuses it."""
        self = cls.__new__(cls)
        self.ctx, self.host, self.index = ctx, host, None
        if kmer_thr is None:
            kmer_thr = host.profile_kmer_threshold(4.0, k)
        letters = np.ascontiguousarray(prof['letters'], np.uint8)
        consensus = np.ascontiguousarray(prof['consensus'], np.uint8)
        score = np.ascontiguousarray(prof['sorted_score'], np.int16)
        index = np.ascontiguousarray(prof['sorted_index'], np.uint8)
        offsets = np.ascontiguousarray(prof['offsets'], np.uint64)
        h = C.c_void_p()
        stats = np.zeros(4, np.uint64)
        _check(ctx.h, ctx.L.sd_target_build_profile(ctx.h, k, kmer_thr, ptr(letters), ptr(consensus), ptr(score), ptr(index), ptr(offsets),
                                                    len(offsets) - 1, C.byref(h), ptr(stats)), 'sd_target_build_profile')
        self.h = h
        self.n = len(offsets) - 1
        self.k = k
        self.total = int(offsets[-1])
        self.build_stats = dict(entries=int(stats[0]), masked_residues=int(stats[1]), passes=int(stats[2]), records=int(stats[3]))
        return self

    @classmethod
    def build_similar_on_device(cls, ctx, host, residues, offsets, k=6, kmer_thr=112):
        """sd_target_build_similar: the similar-k-mer index of a sequence target DB (--target-search-mode 1), built on the GPU from
        the unmasked residues at the sequence threshold.  Sequence queries (api.prefilter) look up their own k-mers only against
        it; api.prefilter_profile refuses it."""
        self = cls.__new__(cls)
        self.ctx, self.host, self.index = ctx, host, None
        residues = np.ascontiguousarray(residues, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        s3, i3, _ = host.ext_matrix(3)
        h = C.c_void_p()
        stats = np.zeros(4, np.uint64)
        _check(ctx.h, ctx.L.sd_target_build_similar(ctx.h, k, kmer_thr, ptr(residues), ptr(offsets), len(offsets) - 1, ptr(s3), ptr(i3),
                                                    C.byref(h), ptr(stats)), 'sd_target_build_similar')
        self.h = h
        self.n = len(offsets) - 1
        self.k = k
        self.total = int(offsets[-1])
        self.build_stats = dict(entries=int(stats[0]), masked_residues=int(stats[1]), passes=int(stats[2]), records=int(stats[3]))
        return self

    def build_peak(self):
        """sd_target_build_peak: the device bytes sd_target_build held at the fullest point of its phases"""
        b = C.c_uint64()
        _check(self.ctx.h, self.ctx.L.sd_target_build_peak(self.h, C.byref(b)), 'sd_target_build_peak')
        return int(b.value)

    def sample_check(self, host, residues, offsets, kmer_thr, runs=24, run_len=400, seed=3, mask=True, mask_prob=0.9):
        """an index too large to download against the host builder on a sample: `runs` runs of `run_len` consecutive sequences are
        masked and indexed on the host (sd_host_index_build of the sample alone: masking and k-mer collection are per sequence);
        every host entry must be in the device index, the device index must hold nothing else for these sequences, and their
        masked residues must agree.  Returns dict(sequences, entries, missing, extra, masked_mismatch)"""
        n = len(offsets) - 1
        rng = np.random.default_rng(seed)
        run_len = min(run_len, n)
        starts = np.unique(rng.integers(0, max(1, n - run_len + 1), runs))
        ids = np.unique(np.concatenate([np.arange(s, s + run_len) for s in starts])).astype(np.uint32)
        lens = (offsets[1:] - offsets[:-1]).astype(np.int64)[ids]
        sub_off = np.zeros(len(ids) + 1, np.uint64)
        np.cumsum(lens, out=sub_off[1:])
        sub_res = np.concatenate([residues[int(offsets[i]):int(offsets[i + 1])] for i in ids])
        h = host.build_index(sub_res, sub_off, k=self.k, kmer_thr=kmer_thr, mask=mask, mask_prob=mask_prob)
        list_start = h.kmer_offsets.astype(np.uint64) if h.block_base is None else None
        assert list_start is not None
        ent = np.arange(h.n_entries, dtype=np.uint64)
        kmer = (np.searchsorted(h.kmer_offsets[:-1], ent, side='right') - 1).astype(np.uint32)
        # (empty lists share their start with the next one: side='right' lands on the last list starting at or before the entry,
        #  which is the one that holds it)
        seq = ids[h.entry_seq].astype(np.uint32)
        pos = h.entry_pos.astype(np.uint32)
        missing, in_sample = C.c_uint64(), C.c_uint64()
        _check(self.ctx.h, self.ctx.L.sd_target_sample_check(self.ctx.h, self.h, ptr(kmer), ptr(seq), ptr(pos), len(kmer), ptr(ids), len(ids),
                                                             C.byref(missing), C.byref(in_sample), 0, 0, None), 'sd_target_sample_check')
        bad = 0
        z = np.zeros(1, np.uint32)
        for s in starts:   # (runs may overlap: compare run by run against the host's masked bytes of the same sequences)
            a, b = int(offsets[s]), int(offsets[min(n, s + run_len)])
            buf = np.zeros(b - a, np.uint8)
            m2, i2 = C.c_uint64(), C.c_uint64()
            _check(self.ctx.h, self.ctx.L.sd_target_sample_check(self.ctx.h, self.h, ptr(z), ptr(z), ptr(z), 0, ptr(z), 0, C.byref(m2), C.byref(i2),
                                                                 a, b, ptr(buf)), 'sd_target_sample_check')
            first = int(np.searchsorted(ids, s))
            ha, hb = int(sub_off[first]), int(sub_off[first + min(run_len, n - int(s))])
            bad += int((buf != h.masked[ha:hb]).sum())
        return dict(sequences=int(len(ids)), entries=int(h.n_entries), missing=int(missing.value),
                    extra=int(in_sample.value) - int(h.n_entries) + int(missing.value), masked_mismatch=bad,
                    masked_residues_in_sample=int(h.masked_residues))

    def download(self, entries=True):
        """the device's copy of the index: dict(n_entries, masked, starts [tableSize + 1], entry_seq, entry_pos)"""
        ne, ts = C.c_uint64(), C.c_uint64()
        _check(self.ctx.h, self.ctx.L.sd_target_download(self.ctx.h, self.h, C.byref(ne), C.byref(ts), None, None, None, None), 'sd_target_download')
        total = self.total if getattr(self, 'total', None) is not None else int(self.index.offsets[-1])
        out = dict(n_entries=ne.value, masked=np.zeros(total, np.uint8), starts=np.zeros(ts.value + 1, np.uint64))
        es = np.zeros(ne.value if entries else 0, np.uint32)
        ep = np.zeros(ne.value if entries else 0, np.uint16)
        _check(self.ctx.h, self.ctx.L.sd_target_download(self.ctx.h, self.h, None, None, ptr(out['masked']), ptr(out['starts']),
                                                         ptr(es) if entries else None, ptr(ep) if entries else None), 'sd_target_download')
        out['entry_seq'], out['entry_pos'] = es, ep
        return out

    def __del__(self):
        try:
            if self.ctx.h:   # (as SeqSet.__del__)
                self.ctx.L.sd_target_destroy(self.h)
        except Exception:
            pass


def target_footprint(k, n_seq, n_residues):
    """sd_target_footprint: upper bound, in bytes, of the device memory building and holding a target of that size takes"""
    return int(_lib.load().sd_target_footprint(int(k), int(n_seq), int(n_residues)))


def prefilter_params(host, n_targets, kmer_thr=112, max_hits=300, min_diag=15, bin_size=None, cov_mode=2,
                     cov_thr=0.8, k=6):
    p = _lib.PrefilterParams()
    p.kmerSize, p.kmerThr, p.maxHitsPerQuery, p.minDiagScore = k, kmer_thr, max_hits, min_diag
    p.binSize = bin_size if bin_size is not None else host.bin_size(n_targets)
    p.covMode, p.covThr = cov_mode, cov_thr
    m, _, _ = host.matrix(2)
    for i in range(441):
        p.ungappedMatrix[i] = int(m[i])
    return p


def prefilter(ctx, target, par, residues, offsets, kmer_bias, diag_bias, identity_id, want_stats=False):
    """sd_prefilter_batch: returns (hits[nQ, maxHits] structured array, counts[nQ], stats[nQ,4] or None)"""
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    kb = np.ascontiguousarray(kmer_bias, np.int16)
    db = np.ascontiguousarray(diag_bias, np.int8)
    ident = np.ascontiguousarray(identity_id, np.uint32)
    nq = len(offsets) - 1
    hits = np.zeros((nq, par.maxHitsPerQuery), _lib.HIT_DTYPE)
    counts = np.zeros(nq, np.uint32)
    stats = np.zeros((nq, 4), np.uint64) if want_stats else None
    _check(ctx.h, ctx.L.sd_prefilter_batch(ctx.h, target.h, C.byref(par), nq, ptr(residues), ptr(offsets), ptr(kb),
                                           ptr(db), ptr(ident), ptr(hits), ptr(counts), ptr(stats)),
           'sd_prefilter_batch')
    return hits, counts, stats


def ungapped_params(host, max_hits=300, min_score=15, cov_mode=0, cov_thr=0.0):
    """sd_ungapped_params with the Smith-Waterman matrix (blosum62 at bit factor 2, score bias 0)"""
    p = _lib.UngappedParams()
    m, _, _ = host.matrix(0)
    for i in range(441):
        p.matrix[i] = int(m[i])
    p.minScore, p.maxHitsPerQuery, p.covMode, p.covThr = min_score, max_hits, cov_mode, cov_thr
    return p


def ungapped_prefilter(ctx, par, queries, targets, target_keys=None, identity_id=None):
    """sd_ungapped_prefilter_batch: every query of the SeqSet `queries` against every target of `targets`.
    Returns (hits[nQ, maxHits] structured array, counts[nQ])."""
    keys = np.ascontiguousarray(target_keys, np.uint32) if target_keys is not None else None
    ident = np.ascontiguousarray(identity_id, np.uint32) if identity_id is not None else None
    hits = np.zeros((queries.n, par.maxHitsPerQuery), _lib.HIT_DTYPE)
    counts = np.zeros(queries.n, np.uint32)
    _check(ctx.h, ctx.L.sd_ungapped_prefilter_batch(ctx.h, C.byref(par), queries.h, targets.h, ptr(keys), ptr(ident), ptr(hits),
                                                    ptr(counts)), 'sd_ungapped_prefilter_batch')
    return hits, counts


def ungapped_scores(ctx, matrix, queries, targets):
    """sd_ungapped_score_matrix: the uint8 score of every (query, target) pair, [nQ, nT]"""
    m = np.ascontiguousarray(matrix, np.int8)
    out = np.zeros((queries.n, targets.n), np.uint8)
    _check(ctx.h, ctx.L.sd_ungapped_score_matrix(ctx.h, ptr(m), queries.h, targets.h, ptr(out)), 'sd_ungapped_score_matrix')
    return out


def ungapped_last_cells(ctx):
    c = C.c_uint64()
    _check(ctx.h, ctx.L.sd_ungapped_last_cells(ctx.h, C.byref(c)), 'sd_ungapped_last_cells')
    return c.value


def prefilter_profile(ctx, target, par, prof, identity_id=None, want_stats=False):
    """sd_prefilter_profile_batch for the profiles of Host.map_profiles (the target index built with kmer_thr=0)"""
    nq = len(prof['offsets']) - 1
    ident = np.ascontiguousarray(identity_id, np.uint32) if identity_id is not None else None
    hits = np.zeros((nq, par.maxHitsPerQuery), _lib.HIT_DTYPE)
    counts = np.zeros(nq, np.uint32)
    stats = np.zeros((nq, 4), np.uint64) if want_stats else None
    _check(ctx.h, ctx.L.sd_prefilter_profile_batch(ctx.h, target.h, C.byref(par), nq, ptr(prof['letters']), ptr(prof['offsets']),
                                                   ptr(prof['sorted_score']), ptr(prof['sorted_index']), ptr(prof['aln']),
                                                   ptr(ident), ptr(hits), ptr(counts), ptr(stats)), 'sd_prefilter_profile_batch')
    return hits, counts, stats


def clusterhits(ctx, host, hit_off, q_pos, t_pos, strands, pval, nq, max_gene_gap=3, cluster_size=2, alpha=1.0,
                p_clu_thr=0.01, p_mh_thr=0.01, lgamma=None):
    """sd_clusterhits_batch over entries [hit_off[p], hit_off[p+1]).  Returns dict of output arrays."""
    hit_off = np.ascontiguousarray(hit_off, np.uint64)
    q_pos = np.ascontiguousarray(q_pos, np.uint32)
    t_pos = np.ascontiguousarray(t_pos, np.uint32)
    strands = np.ascontiguousarray(strands, np.uint8)
    pval = np.ascontiguousarray(pval, np.float64)
    nq = np.ascontiguousarray(nq, np.uint32)
    n_pairs = len(hit_off) - 1
    total = int(hit_off[-1])
    if lgamma is None:
        need = int(max(int(q_pos.max(initial=0)), int(t_pos.max(initial=0)), int(nq.max(initial=0)), total)) + 8
        lgamma = host.lgamma_table(need)
    par = _lib.ChParams(max_gene_gap, cluster_size, alpha, p_clu_thr, p_mh_thr)
    out = dict(cluster_of=np.full(total, 0xFFFFFFFF, np.uint32), rank=np.zeros(total, np.uint32),
               n_clusters=np.zeros(n_pairs, np.uint32), pCO=np.zeros(total, np.float64),
               pMH=np.zeros(total, np.float64), size=np.zeros(total, np.uint32))
    _check(ctx.h, ctx.L.sd_clusterhits_batch(ctx.h, C.byref(par), n_pairs, ptr(hit_off), ptr(q_pos), ptr(t_pos),
                                             ptr(strands), ptr(pval), ptr(nq), ptr(lgamma), len(lgamma),
                                             ptr(out['cluster_of']), ptr(out['rank']), ptr(out['n_clusters']),
                                             ptr(out['pCO']), ptr(out['pMH']), ptr(out['size'])),
           'sd_clusterhits_batch')
    return out


EXPAND_STATES = 'MID'


def cigar_runs(cigar):
    """run-length backtrace text -> the uint32 runs sd_expand_batch takes, (length << 2) | state with M = 0, I = 1, D = 2; a count of
    0 is one column (Matcher::uncompressAlignment)"""
    runs, n = [], 0
    for ch in cigar:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            runs.append((max(n, 1) << 2) | EXPAND_STATES.index(ch))
            n = 0
    return runs


def expand(ctx, ab_start_a, ab_start_b, ab_runs, ab_cluster, bc_rows, mode=0, want_text=None, queries=None, targets=None, ab_query=None,
           bc_target=None, matrix=None, gap_open=11, gap_extend=1):
    """sd_expand_batch (+ sd_expand_backtraces): BacktraceTranslator::translateResult for every (AB row, BC row of its cluster) pair.
    ab_runs: one run list per AB row (cigar_runs); ab_cluster[i]: index into bc_rows or -1 (the B key has no BC entry);
    bc_rows: per cluster a list of (startB, startC, runs).  Returns EXPAND_DTYPE records, pair p = the p-th (AB row, member) in row order.
    mode 1 (the walk of rescoreResultByBacktrace: rawScore, identities, EXPAND_LEAVES_SEQUENCE): queries / targets are SeqSets (the
    queries' set carries the composition bias), ab_query[i] / bc_target[flat BC row] the sequences of the rows, matrix the 21 x 21 int8 one.
    want_text: None, True (every pair with a printed backtrace) or an array of pair indices -> also (pool bytes, offsets[len + 1])."""
    L = ctx.L
    n_ab = len(ab_runs)
    ab_off = np.zeros(n_ab + 1, np.uint64)
    ab_off[1:] = np.cumsum([len(r) for r in ab_runs], dtype=np.uint64)
    ab_flat = np.ascontiguousarray(np.concatenate([np.asarray(r, np.uint32) for r in ab_runs] + [np.zeros(0, np.uint32)]), np.uint32)
    row_off = np.zeros(len(bc_rows) + 1, np.uint64)
    row_off[1:] = np.cumsum([len(c) for c in bc_rows], dtype=np.uint64)
    rows = [r for c in bc_rows for r in c]
    bc_sb = np.array([r[0] for r in rows], np.int32)
    bc_sc = np.array([r[1] for r in rows], np.int32)
    bc_off = np.zeros(len(rows) + 1, np.uint64)
    bc_off[1:] = np.cumsum([len(r[2]) for r in rows], dtype=np.uint64)
    bc_flat = np.ascontiguousarray(np.concatenate([np.asarray(r[2], np.uint32) for r in rows] + [np.zeros(0, np.uint32)]), np.uint32)
    sa = np.ascontiguousarray(ab_start_a, np.int32)
    sb = np.ascontiguousarray(ab_start_b, np.int32)
    clu = np.ascontiguousarray(np.asarray(ab_cluster, np.int64) & 0xFFFFFFFF, np.uint32)
    assert len(sa) == len(sb) == len(clu) == n_ab
    n_pairs = int(sum(len(bc_rows[c]) for c in np.asarray(ab_cluster, np.int64) if 0 <= c < len(bc_rows)))
    par = _lib.ExpandParams()
    par.mode, par.gapOpen, par.gapExtend = int(mode), int(gap_open), int(gap_extend)
    if matrix is not None:
        C.memmove(par.matrix, np.ascontiguousarray(matrix, np.int8).ctypes.data, 441)
    abq = np.ascontiguousarray(ab_query, np.uint32) if ab_query is not None else None
    bct = np.ascontiguousarray(bc_target, np.uint32) if bc_target is not None else None
    assert abq is None or len(abq) == n_ab
    assert bct is None or len(bct) == len(rows)
    res = np.zeros(n_pairs, _lib.EXPAND_DTYPE)
    got = C.c_uint64()
    _check(ctx.h, L.sd_expand_batch(ctx.h, C.byref(par), n_ab, ptr(sa), ptr(sb), ptr(ab_off), ptr(ab_flat), ptr(clu), len(bc_rows),
                                    ptr(row_off), ptr(bc_sb), ptr(bc_sc), ptr(bc_off), ptr(bc_flat), queries.h if queries is not None else None,
                                    targets.h if targets is not None else None, ptr(abq), ptr(bct), n_pairs, ptr(res), C.byref(got)),
           'sd_expand_batch')
    assert got.value == n_pairs
    if want_text is None:
        return res
    kept = np.flatnonzero(res['btLen'] > 0).astype(np.uint64) if want_text is True else np.ascontiguousarray(want_text, np.uint64)
    pool = np.zeros(int(res['textLen'][kept.astype(np.int64)].sum()) + 1, np.uint8)
    off = np.zeros(len(kept) + 1, np.uint64)
    _check(ctx.h, L.sd_expand_backtraces(ctx.h, len(kept), ptr(kept), ptr(pool), len(pool), ptr(off)), 'sd_expand_backtraces')
    return res, pool[:int(off[-1])], off


def expand_last_stats(ctx):
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(ctx.h, ctx.L.sd_expand_last_stats(ctx.h, C.byref(a), C.byref(b), C.byref(c)), 'sd_expand_last_stats')
    return dict(pairs=a.value, runs_read=b.value, bytes_written=c.value)


# ---- clust: the symmetric graph on the GPU, everything else on the host

def clust_symmetrize(ctx, row_off, elem, score, cap=None):
    """sd_clust_symmetrize: CSR graph over local ids -> (row_off uint64 [n + 1], elem uint32, score uint16, stats) with every missing back
    edge appended to its row; stats = dict(entries_in, added, largest_row).  cap: room of the output in entries (default: exactly enough,
    learned from a count-only call first)."""
    L = _lib.load()
    row_off = np.ascontiguousarray(row_off, np.uint64)
    elem = np.ascontiguousarray(elem, np.uint32)
    score = np.ascontiguousarray(score, np.uint16)
    n = len(row_off) - 1
    assert len(elem) == len(score) == int(row_off[-1])
    stats = np.zeros(3, np.uint64)
    if cap is None:
        rc = L.sd_clust_symmetrize(ctx.h, n, ptr(row_off), ptr(elem), ptr(score), 0, None, None, None, ptr(stats))
        if rc != _lib.SD_ENOMEM:
            _check(ctx.h, rc, 'sd_clust_symmetrize')
        cap = int(stats[0] + stats[1])
    out_off = np.zeros(n + 1, np.uint64)
    out_elem = np.zeros(max(cap, 1), np.uint32)
    out_score = np.zeros(max(cap, 1), np.uint16)
    _check(ctx.h, L.sd_clust_symmetrize(ctx.h, n, ptr(row_off), ptr(elem), ptr(score), cap, ptr(out_off), ptr(out_elem), ptr(out_score), ptr(stats)),
           'sd_clust_symmetrize')
    total = int(out_off[-1])
    return out_off, out_elem[:total], out_score[:total], dict(entries_in=int(stats[0]), added=int(stats[1]), largest_row=int(stats[2]))


def clust_order(index_lengths):
    """sd_host_clust_order: local id -> position in key order (index length descending, then key order)"""
    lens = np.ascontiguousarray(index_lengths, np.uint64)
    out = np.zeros(len(lens), np.uint32)
    _check(None, _lib.load().sd_host_clust_order(len(lens), ptr(lens), ptr(out)), 'sd_host_clust_order')
    return out


def clust_parse(local_keys, entries, dbtype, similarity_type=2):
    """sd_host_clust_parse: entries[i] (bytes) is the result entry of local id i -> (row_off, elem, score)"""
    L = _lib.load()
    keys = np.ascontiguousarray(local_keys, np.uint32)
    n = len(keys)
    assert len(entries) == n
    bufs = [C.create_string_buffer(bytes(e)) for e in entries]   # ('\0'-terminated)
    arr = (C.c_char_p * max(n, 1))(*[C.cast(b, C.c_char_p) for b in bufs])
    row_off = np.zeros(n + 1, np.uint64)
    bad = C.c_uint32()
    _check(None, L.sd_host_clust_parse(n, ptr(keys), arr, dbtype, similarity_type, ptr(row_off), 0, None, None, C.byref(bad)), 'sd_host_clust_parse')
    total = int(row_off[-1])
    elem, score = np.zeros(max(total, 1), np.uint32), np.zeros(max(total, 1), np.uint16)
    rc = L.sd_host_clust_parse(n, ptr(keys), arr, dbtype, similarity_type, ptr(row_off), total, ptr(elem), ptr(score), C.byref(bad))
    if rc == _lib.SD_EINVAL:
        raise SdError('Element %d contained in some alignment list, but not contained in the sequence database!' % bad.value)
    _check(None, rc, 'sd_host_clust_parse')
    return row_off, elem[:total], score[:total]


def clust_assign(mode, row_off, elem, score=None, max_iterations=1000):
    """the host algorithms: mode 0 set cover and 1 connected component on the symmetric graph, 2 / 3 greedy on the parsed rows.
    Returns assigned uint32 [n] (local id of the representative)."""
    L = _lib.load()
    row_off = np.ascontiguousarray(row_off, np.uint64)
    elem = np.ascontiguousarray(elem, np.uint32)
    n = len(row_off) - 1
    out = np.zeros(max(n, 1), np.uint32)
    if mode == 0:
        score = np.ascontiguousarray(score, np.uint16)
        rc = L.sd_host_clust_setcover(n, ptr(row_off), ptr(elem), ptr(score), ptr(out))
    elif mode == 1:
        rc = L.sd_host_clust_connected(n, ptr(row_off), ptr(elem), int(max_iterations), ptr(out))
    elif mode in (2, 3):
        rc = L.sd_host_clust_greedy(n, ptr(row_off), ptr(elem), ptr(out))
    else:
        raise SdError('Wrong clustering mode!')
    _check(None, rc, 'sd_host_clust_* (mode %d)' % mode)
    return out[:n]


def clust_format(local_keys, assigned):
    """sd_host_clust_format: (pairs uint32 [n, 2] sorted, cluster DB as dict key -> bytes)"""
    L = _lib.load()
    keys = np.ascontiguousarray(local_keys, np.uint32)
    assigned = np.ascontiguousarray(assigned, np.uint32)
    n = len(keys)
    rep, mem = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    ekey, eoff, text = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint64), np.zeros(22 * n + 1, np.uint8)
    ne = C.c_uint64()
    _check(None, L.sd_host_clust_format(n, ptr(keys), ptr(assigned), ptr(rep), ptr(mem), C.byref(ne), ptr(ekey), ptr(eoff), ptr(text)),
           'sd_host_clust_format')
    raw = text.tobytes()
    db = {int(ekey[e]): raw[int(eoff[e]):int(eoff[e + 1])] for e in range(ne.value)}
    return np.stack([rep[:n], mem[:n]], axis=1), db


def reduced_alphabet(alphabet_size=13, which=0):
    """sd_host_reduced_alphabet: (letter_map uint8 [21], reduced size) -- ReducedMatrix's merging of the 21 letters of matrix `which` down
    to alphabet_size codes (X the last one); 21 is the identity."""
    out = np.zeros(21, np.uint8)
    size = C.c_int()
    _check(None, _lib.load().sd_host_reduced_alphabet(int(which), int(alphabet_size), ptr(out), C.byref(size)), 'sd_host_reduced_alphabet')
    return out, size.value


def kmermatch_auto_k(min_seq_id, residues):
    """sd_host_kmermatch_auto_k: (k, alphabet size) of `kmermatcher -k 0`"""
    k, a = C.c_int(), C.c_int()
    _check(None, _lib.load().sd_host_kmermatch_auto_k(float(min_seq_id), int(residues), C.byref(k), C.byref(a)), 'sd_host_kmermatch_auto_k')
    return k.value, a.value


def kmermatch_params(k=0, alph_size=13, kmer_per_seq=0, kmer_per_seq_scale=0.0, hash_shift=67, cov_mode=0, c=0.8,
                     include_only_extendable=False, min_seq_id=0.0, residues=0):
    """the kmermatcher module's parameters after its defaults (setLinearFilterDefault, setKmerLengthAndAlphabet): k = 0 chooses k and the
    alphabet from min_seq_id and the residue count, kmer_per_seq = 0 is 20"""
    if k == 0:
        k, alph_size = kmermatch_auto_k(min_seq_id, residues)
    return _lib.KmParams(int(k), int(alph_size), int(kmer_per_seq) if kmer_per_seq else 20, float(kmer_per_seq_scale), int(hash_shift),
                         int(cov_mode), float(c), 1 if include_only_extendable else 0)


def kmermatch(ctx, par, residues, offsets, keys, letter_map=None, cap=None):
    """sd_kmermatch_batch: the hits of linclust's kmermatcher as (rep, member, score uint32, diagonal int32, stats), sorted by (rep, member);
    stats = dict(records, grouped, hits, largest_group).  letter_map: default reduced_alphabet(par.alphabetSize).  cap: room of the output
    in hits (default: exactly enough, learned from a count-only call first)."""
    L = _lib.load()
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    keys = np.ascontiguousarray(keys, np.uint32)
    n = len(offsets) - 1
    assert len(keys) == n and len(residues) == int(offsets[-1])
    if letter_map is None:
        letter_map = reduced_alphabet(par.alphabetSize)[0]
    letter_map = np.ascontiguousarray(letter_map, np.uint8)
    stats = np.zeros(4, np.uint64)
    named = lambda: dict(records=int(stats[0]), grouped=int(stats[1]), hits=int(stats[2]), largest_group=int(stats[3]))
    if cap is None:
        rc = L.sd_kmermatch_batch(ctx.h, C.byref(par), n, ptr(residues), ptr(offsets), ptr(keys), ptr(letter_map), 0, None, None, None, None,
                                  ptr(stats))
        if rc != _lib.SD_ENOMEM or int(stats[2]) == 0:
            _check(ctx.h, rc, 'sd_kmermatch_batch')
        cap = int(stats[2])
    rep, mem, score = (np.zeros(max(cap, 1), np.uint32) for _ in range(3))
    diag = np.zeros(max(cap, 1), np.int32)
    _check(ctx.h, L.sd_kmermatch_batch(ctx.h, C.byref(par), n, ptr(residues), ptr(offsets), ptr(keys), ptr(letter_map), cap, ptr(rep), ptr(mem),
                                       ptr(score), ptr(diag), ptr(stats)), 'sd_kmermatch_batch')
    h = int(stats[2])
    return rep[:h], mem[:h], score[:h], diag[:h], named()


def kmermatch_records(ctx, par, residues, offsets, keys, letter_map=None, cap=None):
    """sd_selftest_kmermatch_records: the records stage of sd_kmermatch_batch alone -> dict(considered, threshold, excess uint32 [n],
    rec_off uint64 [n + 1], key uint64, id, len, pos uint32 [records]), sequences in input order, records in emission order.  cap: room in
    records (default: exactly enough, learned from a count-only call first)."""
    L = _lib.load()
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    keys = np.ascontiguousarray(keys, np.uint32)
    n = len(offsets) - 1
    assert len(keys) == n and len(residues) == int(offsets[-1])
    if letter_map is None:
        letter_map = reduced_alphabet(par.alphabetSize)[0]
    letter_map = np.ascontiguousarray(letter_map, np.uint8)
    stats = np.zeros(1, np.uint64)
    call = lambda room, *out: L.sd_selftest_kmermatch_records(ctx.h, C.byref(par), n, ptr(residues), ptr(offsets), ptr(keys), ptr(letter_map),
                                                              room, *out, ptr(stats))
    if cap is None:
        rc = call(0, *[None] * 8)
        if rc != _lib.SD_ENOMEM or int(stats[0]) == 0:
            _check(ctx.h, rc, 'sd_selftest_kmermatch_records')
        cap = int(stats[0])
    cons, thr, exc = (np.zeros(max(n, 1), np.uint32) for _ in range(3))
    rec_off = np.zeros(n + 1, np.uint64)
    key = np.zeros(max(cap, 1), np.uint64)
    rid, rlen, rpos = (np.zeros(max(cap, 1), np.uint32) for _ in range(3))
    _check(ctx.h, call(cap, ptr(cons), ptr(thr), ptr(exc), ptr(rec_off), ptr(key), ptr(rid), ptr(rlen), ptr(rpos)),
           'sd_selftest_kmermatch_records')
    r = int(stats[0])
    return dict(considered=cons[:n], threshold=thr[:n], excess=exc[:n], rec_off=rec_off, key=key[:r], id=rid[:r], len=rlen[:r], pos=rpos[:r])


def kmermatch_format(keys, rep, member, score, diag):
    """sd_host_kmermatch_format: the prefilter DB of the hits as dict key -> bytes (every sequence key has an entry)"""
    L = _lib.load()
    keys = np.ascontiguousarray(keys, np.uint32)
    rep, member, score = (np.ascontiguousarray(x, np.uint32) for x in (rep, member, score))
    diag = np.ascontiguousarray(diag, np.int32)
    n, h = len(keys), len(rep)
    nbytes = C.c_uint64()
    _check(None, L.sd_host_kmermatch_format(n, ptr(keys), h, ptr(rep), ptr(member), ptr(score), ptr(diag), None, None, 0, None, C.byref(nbytes)),
           'sd_host_kmermatch_format')
    ekey, eoff, text = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint64), np.zeros(nbytes.value + 1, np.uint8)
    _check(None, L.sd_host_kmermatch_format(n, ptr(keys), h, ptr(rep), ptr(member), ptr(score), ptr(diag), ptr(ekey), ptr(eoff), nbytes.value,
                                            ptr(text), C.byref(nbytes)), 'sd_host_kmermatch_format')
    raw = text.tobytes()
    return {int(ekey[e]): raw[int(eoff[e]):int(eoff[e + 1])] for e in range(n)}


def clusthash_min_identical(min_seq_id, length):
    """sd_host_clusthash_min_identical: the smallest d with float32(d) / float32(length) >= min_seq_id, length + 1 when there is none"""
    return int(_lib.load().sd_host_clusthash_min_identical(float(min_seq_id), int(length)))


def clusthash(ctx, residues, offsets, letters, alph_size=3, min_seq_id=0.99, letter_map=None, want_hash=True):
    """sd_clusthash_batch: (found_by uint32 [n] (UINT32_MAX: not found), identical uint32 [n], hash uint64 [n] or None, stats) of the
    sequences in input order = id order; stats = dict(unique_hashes, groups, pairs, largest_group).  letters: the DB's own bytes, laid out
    like residues.  letter_map: default reduced_alphabet(alph_size)."""
    L = _lib.load()
    residues = np.ascontiguousarray(residues, np.uint8)
    letters = np.ascontiguousarray(letters, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    assert len(residues) == int(offsets[-1]) and len(letters) == len(residues)
    if letter_map is None:
        letter_map = reduced_alphabet(alph_size)[0]
    letter_map = np.ascontiguousarray(letter_map, np.uint8)
    par = _lib.ClusthashParams(int(alph_size), float(min_seq_id))
    found_by, identical = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    hashes = np.zeros(max(n, 1), np.uint64) if want_hash else None
    stats = np.zeros(4, np.uint64)
    _check(ctx.h, L.sd_clusthash_batch(ctx.h, C.byref(par), n, ptr(residues), ptr(offsets), ptr(letters), ptr(letter_map), ptr(found_by),
                                       ptr(identical), ptr(hashes), ptr(stats)), 'sd_clusthash_batch')
    named = dict(unique_hashes=int(stats[0]), groups=int(stats[1]), pairs=int(stats[2]), largest_group=int(stats[3]))
    return found_by[:n], identical[:n], (hashes[:n] if want_hash else None), named


def clusthash_format(keys, offsets, found_by, identical):
    """sd_host_clusthash_format: the alignment DB of clusthash as dict key -> bytes (one entry per sequence)"""
    L = _lib.load()
    keys, found_by, identical = (np.ascontiguousarray(x, np.uint32) for x in (keys, found_by, identical))
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(keys)
    assert len(offsets) == n + 1 and len(found_by) == n and len(identical) == n
    nbytes = C.c_uint64()
    _check(None, L.sd_host_clusthash_format(n, ptr(keys), ptr(offsets), ptr(found_by), ptr(identical), None, 0, None, C.byref(nbytes)),
           'sd_host_clusthash_format')
    eoff, text = np.zeros(n + 1, np.uint64), np.zeros(nbytes.value + 1, np.uint8)
    _check(None, L.sd_host_clusthash_format(n, ptr(keys), ptr(offsets), ptr(found_by), ptr(identical), ptr(eoff), nbytes.value, ptr(text),
                                            C.byref(nbytes)), 'sd_host_clusthash_format')
    raw = text.tobytes()
    return {int(keys[e]): raw[int(eoff[e]):int(eoff[e + 1])] for e in range(n)}
