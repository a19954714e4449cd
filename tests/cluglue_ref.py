"""Python restatements of the host glue of `cluster --single-step-clustering 1`, for tests/test_glue_cluster.py and
tests/test_gpu_cluster_workflow.py: createsubdb (M/src/util/createsubdb.cpp:10-101) and mergeclusters (M/src/util/mergeclusters.cpp:13-153),
and the parameter strings of the chain's steps (M/src/workflow/Cluster.cpp:14-20,63-104,244-262)."""


def read_index(path):
    """-> list of (key, offset, length) in file order"""
    return [tuple(int(x) for x in line.split()) for line in open(path + '.index') if line.strip()]


def createsubdb(keys, source_index, source_data, mode):
    """keys: the list, in its order; source_index: (key, offset, length) lines of the source; -> (index lines of the sub DB, data bytes of
    the sub DB or None when it is a link).  A key the source lacks is skipped; the index is in list order, sorted by key (stably) only when
    the list was not ascending"""
    by_key = {k: (o, l) for k, o, l in source_index}
    index, data, at = [], b'', 0
    for key in keys:
        if key not in by_key:
            continue
        o, l = by_key[key]
        if mode == 1:
            index.append((key, o, l))
        else:
            payload = source_data[o:o + max(l, 1) - 1]
            data += payload + b'\0'
            index.append((key, at, l))
            at += len(payload) + 1
    if any(a > b for a, b in zip(keys, keys[1:])):
        index.sort(key=lambda e: e[0])
    return index, (None if mode == 1 else data)


def mergeclusters(seq_keys, steps):
    """seq_keys: the sequence DB's keys, ascending; steps: list of cluster DBs, each a list of (representative key, [member keys]) in data
    order -> dict representative key -> member keys.  KeyError(key) for a key the sequence DB lacks"""
    known = set(seq_keys)
    lists = {k: [] for k in seq_keys}

    def check(k):
        if k not in known:
            raise KeyError(k)
        return k

    for s, step in enumerate(steps):
        for rep, members in step:
            check(rep)
            for m in members:
                check(m)
                if s == 0:
                    lists[rep].append(m)
                elif m != rep:
                    lists[rep] += lists[m]
                    lists[m] = []
    return {k: v for k, v in lists.items() if v}


def automatic_sensitivity(seq_id):
    """setAutomaticThreshold, in the reference's mixed float / double arithmetic, printed with %g"""
    import numpy as np
    s = np.float32(seq_id)
    if s <= 0.3:
        v = np.float32(6)
    elif s > 0.8:
        v = np.float32(1.0)
    else:
        v = np.float32(1.0 + (1.0 * (0.7 - float(s)) * 10))
    return '%g' % float(v)


def step_flags(threads, min_seq_id=0.0, cov_mode=0, alignment_mode=3, c=0.8, e=0.001, max_seqs=20):
    """the flags of clusthash, clust, createsubdb, prefilter, the alignment step (module name and flags) and mergeclusters, as `sdgpu
    cluster --single-step-clustering 1` derives them from its own (no -s, --cluster-mode, --comp-bias-corr or --min-ungapped-score given)"""
    common = ['--threads', str(threads), '-v', '0']
    high = float(min_seq_id) >= 0.7
    comp_bias = '0' if high else '1'
    hits = ['-e', str(e), '-c', str(c), '--cov-mode', str(cov_mode), '--min-seq-id', str(min_seq_id)]
    if alignment_mode == 4:
        aln = ('rescorediagonal', common + hits + ['--rescore-mode', '2'])
    else:
        aln = ('align', common + hits + ['--alignment-mode', str(alignment_mode), '--comp-bias-corr', comp_bias])
    return dict(clusthash=common + ['--alph-size', '3', '--min-seq-id', '0.99'],
                clust=common + ['--cluster-mode', '2' if cov_mode in (1, 2) else '0'],
                createsubdb=['-v', '0', '--subdb-mode', '1'],
                prefilter=common + ['-s', automatic_sensitivity(min_seq_id), '--max-seqs', str(max_seqs), '-c', str(c), '--cov-mode', str(cov_mode),
                                    '--min-ungapped-score', '60' if high else '15', '--comp-bias-corr', comp_bias],
                align=aln, mergeclusters=common)
