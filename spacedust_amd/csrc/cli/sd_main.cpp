// sdgpu -- multi-call host driver of the MI355X-native clustersearch hot path.  `sdgpu <module> <args>` accepts the
// command lines the reference's workflow scripts issue as `$MMSEQS <module> <args>` (R/src/spacedust.cpp:26-114 is
// the reference's command table; R/data/clustersearch.sh and M/data/workflow/blastp.sh / blastpgp.sh are the callers), so a
// wrapper that forwards the hot modules here and everything else to the reference binary runs those scripts unchanged.
#include "sd_cli.h"
#include <omp.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>

using namespace sdcli;

namespace {
struct Module {
    const char *name;
    int (*fn)(const Args &);
    const char *what;
};
const Module kModules[] = {
    {"prefilter", prefilterModule, "k-mer prefilter on the GPU: <queryDB> <targetDB> <prefilterDB>"},
    {"ungappedprefilter", ungappedprefilterModule, "exhaustive ungapped prefilter on the GPU (--prefilter-mode 1): <queryDB> <targetDB> <prefilterDB>"},
    {"align", alignModule, "Smith-Waterman alignments on the GPU: <queryDB> <targetDB> <prefilterDB> <alignmentDB>"},
    {"rescorediagonal", rescorediagonalModule, "ungapped alignment on each hit's diagonal on the GPU (--alignment-mode 4): <queryDB> <targetDB> <prefilterDB> <resultDB>"},
    {"clusterhits", clusterhitsModule, "agglomerative hit clustering on the GPU: <querySetDB> <targetSetDB> <matchesDB> <clustersDB>"},
    {"search", searchModule, "prefilter + align (the --num-iterations profile loop; a profile target DB through swapresults): <queryDB> <targetDB> <alignmentDB> <tmpDir>"},
    {"clustersearch", clustersearchModule, "the whole --search-mode 0 workflow in one process (--profile-cluster-search 1: through the cluster representatives' profiles and expandaln): <querySetDB> <targetSetDB> <out.tsv> <tmpDir>"},
    {"prefixid", prefixidModule, "host glue: prefix every line of a result DB with its entry key"},
    {"besthitbyset", besthitbysetModule, "host glue: best hit per (query protein, target set)"},
    {"mergeresultsbyset", mergeresultsbysetModule, "host glue: concatenate the entries of a set's members"},
    {"combinehits", combinehitsModule, "host glue: per (query set, target set) hit lists + multihit E-value"},
    {"summarizeresults", summarizeresultsModule, "host glue: clusters DB -> final TSV"},
    {"result2profile", result2profileModule, "host: alignment DB -> profile DB (between search iterations)"},
    {"subtractdbs", subtractdbsModule, "host glue: remove from result DB A the targets listed in result DB B"},
    {"mergedbs", mergedbsModule, "host glue: merge the entries of several DBs by key"},
    {"swapresults", swapresultsModule, "host glue: re-key a prefilter / alignment DB by its targets: <queryDB> <targetDB> <resultDB> <outDB>"},
    {"expandaln", expandalnModule, "A->B alignments carried over to the C's each B is aligned with, backtraces translated on the GPU: <queryDB> <targetDB> <resultDB_AB> <resultDB_BC> <outDB>"},
    {"clust", clustModule, "result DB of a set against itself -> cluster DB; the symmetric graph of --cluster-mode 0 / 1 is built on the GPU: <sequenceDB> <resultDB> <clusterDB>"},
    {"kmermatcher", kmermatcherModule, "linclust's first stage: sequences sharing a selected k-mer grouped under the longest, records sorted and grouped on the GPU: <sequenceDB> <prefDB>"},
    {"clusthash", clusthashModule, "sequences of equal reduced-alphabet hash and length compared byte for byte, hashed, sorted and compared on the GPU: <sequenceDB> <resultDB>"},
    {"createsubdb", createsubdbModule, "host glue: the entries of a DB that a key list or another DB's index names, copied (--subdb-mode 0) or soft-linked (1): <subsetFile|DB> <DB> <DB>"},
    {"mergeclusters", mergeclustersModule, "host glue: the cluster DBs of successive steps merged into one: <sequenceDB> <clusterDB> <clusterDB1> [<clusterDB2> ...]"},
    {"cluster", clusterModule, "--single-step-clustering 1: clusthash, clust, createsubdb, prefilter, align (or rescorediagonal), clust, mergeclusters in one process: <sequenceDB> <clusterDB> <tmpDir>"},
    {"profile2consensus", profile2consensusModule, "host: the consensus residue of every profile position as an amino-acid DB: <profileDB> <sequenceDB>"},
    {"makeclusterdb", clusterdbModule, "the reference's clusterdb workflow with --single-step-clustering 1: cluster, createsubdb, result2profile (members realigned on the GPU), profile2consensus, align -a in one process; writes <setDB>_clu_rep_profile, <setDB>_clu, <setDB>_clu_aln: <setDB> <tmpDir>"},
    {"createindex", createindexModule, "target k-mer index built once, in the reference's createindex file layout: <sequenceDB> <tmpDir>"},
    {"createsetdb", createsetdbModule, "FASTA files (Prodigal headers) -> setDB in the createsetdb layout"},
};
}  // namespace

int main(int argc, const char **argv) {
    // The host stages' OpenMP teams wait between parallel regions while a kernel runs or another stage has the CPUs; libgomp's default
    // is to spin there (round 6, `clustersearch --num-iterations 3` on 4 query proteomes: 98 CPU-seconds inside 6.6 s of the alignment
    // stage, 89 inside 5.8 s of result2profile -- sixteen threads spinning).  The policy is read when libgomp is loaded, i.e. before
    // main: when the caller has not chosen one, choose the passive one and start over (spacedust_amd/cpus.py does the same for Python).
    if (!getenv("OMP_WAIT_POLICY") && !getenv("GOMP_SPINCOUNT") && !getenv("SD_NO_REEXEC")) {
        setenv("OMP_WAIT_POLICY", "passive", 1);
        setenv("GOMP_SPINCOUNT", "0", 1);
        setenv("SD_NO_REEXEC", "1", 1);
        execv("/proc/self/exe", (char *const *) argv);
        // (exec failed: go on with the default policy)
    }
    if (argc < 2 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) {
        printf("sdgpu: MI355X-native hot path of spacedust clustersearch --search-mode 0\n\nusage: sdgpu <module> <args>\n\n");
        for (const Module &m : kModules) printf("  %-18s %s\n", m.name, m.what);
        return argc < 2 ? 1 : 0;
    }
    for (const Module &m : kModules) {
        if (strcmp(argv[1], m.name) != 0) continue;
        Args a;
        a.module = m.name;
        std::string err;
        if (!a.parse(argc - 2, argv + 2, &err)) {
            fprintf(stderr, "sdgpu %s: %s\n", m.name, err.c_str());
            return 1;
        }
        info(a, "");
        // OpenMP teams of the host stages: --threads, else the cgroup CPU quota (a 256-thread default team on a 16-CPU quota
        // spends its time being descheduled)
        omp_set_num_threads(threadsOf(a));
        return m.fn(a);
    }
    if (!strcmp(argv[1], "clusterdb"))
        fprintf(stderr, "sdgpu: unknown module \"clusterdb\" (the reference's clusterdb workflow is the module makeclusterdb here)\n");
    else
        fprintf(stderr, "sdgpu: unknown module \"%s\" (sdgpu --help lists the modules)\n", argv[1]);
    return 1;
}
