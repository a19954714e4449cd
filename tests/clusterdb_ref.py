"""Python restatement of the parameter strings `sdgpu makeclusterdb` hands to its five steps (R/src/workflow/clusterdb.cpp:9-13,62-66 and the
non-foldseek branch of R/data/clusterdb.sh:97-126), for tests/test_clusterdb.py and tests/test_gpu_clusterdb.py."""


def step_args(t, tmp, threads, v='3', user=None, device=None):
    """user: the flags given to clusterdb besides --threads, -v and --device, as {flag: value} (booleans '1' / '0').  Returns the steps in
    order as (module, positional arguments, flags)."""
    user = dict(user or {})
    given = dict(user, **{'--threads': str(threads), '-v': str(v)})
    if device is not None:
        given['--device'] = str(device)
    # CLUSTER_PAR: what the user gave over setclusterDbDefaults, without the two flags only clusterdb has; in flag order
    cluster = {k: x for k, x in given.items() if k not in ('--search-mode', '--foldseek-path')}
    for flag, default in (('--min-seq-id', '0.7'), ('-c', '0.8'), ('--cov-mode', '0')):
        cluster.setdefault(flag, default)
    cluster_flags = [x for k in sorted(cluster) for x in (k, cluster[k])]
    threads_par = ['--threads', str(threads), '-v', str(v)]      # THREADS_PAR: nothing else of the user's reaches result2profile and align
    consensus = list(threads_par)
    if device is not None:
        threads_par += ['--device', str(device)]
    for flag in ('--sub-mat', '--max-seq-len'):
        if flag in user:
            consensus += [flag, user[flag]]
    clu, db_clu = tmp + '/cluster_mmseqs', tmp + '/db_clu'
    return [('cluster', [t, clu, tmp + '/cluster'], cluster_flags),
            ('createsubdb', [clu, t, db_clu], ['-v', str(v)]),
            ('result2profile', [db_clu, t, clu, t + '_clu_rep_profile'], threads_par),
            ('profile2consensus', [t + '_clu_rep_profile', t + '_clu'], consensus),
            ('align', [t, t, clu, t + '_clu_aln'], ['-a', '1'] + threads_par)]


def plan_lines(steps, skipped=()):
    """the lines clusterdb prints at -v 3 before its first step"""
    return ['makeclusterdb %s: %s' % ('skips' if m in skipped else 'runs', ' '.join([m] + pos + flags)) for m, pos, flags in steps]
