// The workflow modules: what the reference runs as shell scripts over several processes, here one process around the
// C++ pipeline object of libsdgpu.so (sd_search_*):
//   search         <queryDB> <targetDB> <alignmentDB> <tmpDir>   = prefilter + align (M/data/workflow/blastp.sh:59-90),
//                                                                   the DBs written from the pipeline's sinks
//   clustersearch  <querySetDB> <targetSetDB> <out.tsv> <tmpDir> = search -> prefixid -> besthitbyset -> mergeresultsbyset ->
//                                                                   combinehits -> clusterhits -> summarizeresults
//                                                                   (R/data/clustersearch.sh:110-152), fused in-process
// Several ranks (RANK / WORLD_SIZE / LOCAL_RANK in the environment, one process per GPU): whole query sets are dealt to
// the ranks, every rank's cluster records are gathered on rank 0 (RCCL: sd_gather_results), which writes the TSV (the
// reference's MPI mode merges per-rank result files on the master instead, M/src/prefiltering/Prefiltering.cpp:619-650).
#include "sd_cli.h"
#include "sd_align_core.h"
#include "sd_pref_core.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <fstream>
#include <map>
#include <memory>
#include <omp.h>
#include <sys/stat.h>
#include <unistd.h>
#include <thread>

namespace sdcli {

namespace {

struct SearchH {
    sd_search *s = nullptr;
    ~SearchH() { if (s) sd_search_destroy(s); }
};

int envInt(const char *name, int def) {
    const char *e = getenv(name);
    return e ? atoi(e) : def;
}

// search parameters from the command line over the workflow's defaults
void fillParams(const Args &a, sd_search_params &p, bool clustersearchDefaults) {
    sd_search_default_params(&p);
    if (!clustersearchDefaults) {   // plain `search` defaults (M/src/commons/Parameters.cpp:2351-2611)
        p.sensitivity = 5.7f;       // search workflow default (Parameters: sensitivity 5.7 for search)
        p.evalThr = 0.001;
        p.covMode = 0;
        p.covThr = 0.0f;
        p.alnLenThr = 0;
    }
    p.sensitivity = (float) a.real("-s", p.sensitivity);
    p.kmerSize = (int32_t) a.integer("-k", 0);
    p.maxSeqs = (int32_t) a.integer("--max-seqs", 300);
    p.minDiagScore = (int32_t) a.integer("--min-ungapped-score", 15);
    p.binSize = (uint32_t) a.integer("--bin-size", 0);
    p.mask = (int32_t) a.integer("--mask", 1);
    p.maskProb = a.real("--mask-prob", 0.9);
    p.compBiasCorr = (int32_t) a.integer("--comp-bias-corr", 1);
    p.evalThr = a.real("-e", p.evalThr);
    p.covMode = (int32_t) a.integer("--cov-mode", p.covMode);
    p.covThr = (float) a.real("-c", p.covThr);
    p.alnLenThr = (int32_t) a.integer("--min-aln-len", p.alnLenThr);
    p.maxGeneGap = (uint32_t) a.integer("--max-gene-gap", 3);
    p.clusterSize = (uint32_t) a.integer("--cluster-size", 2);
    p.alpha = a.real("--alpha", 1.0);
    p.pCluThr = (float) a.real("--cluster-pval", 0.01);
    p.pMHThr = (float) a.real("--multihit-pval", 0.01);
    p.filterSelfMatch = a.flag("--filter-self-match", false) ? 1 : 0;
    p.chunkQueries = (int32_t) a.integer("--chunk-queries", 0);   // 0: sd_search_stream chooses by the size of the target set
    p.threads = threadsOf(a);
}

int checkWorkflowFlags(const Args &a) {
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    if (a.integer("--search-mode", 0) != 0) return fail("--search-mode 1/2 (Foldseek) are outside this path; only --search-mode 0");
    if (a.integer("--gpu", 0) != 0) return fail("--gpu 1 selects the reference's CUDA ungapped prefilter (a different algorithm); run without it");
    if (a.multi("--sub-mat", "aa", "blosum62.out") != "blosum62.out") return fail("--sub-mat: only blosum62.out is built into this path");
    if (a.multi("--seed-sub-mat", "aa", "VTML80.out") != "VTML80.out") return fail("--seed-sub-mat: only VTML80.out is built into this path");
    if (a.integer("--exact-kmer-matching", 0) != 0 || a.integer("--spaced-kmer-mode", 1) != 1 || !a.flag("--diag-score", true))
        return fail("--exact-kmer-matching 1 / --spaced-kmer-mode 0 / --diag-score 0 are not supported");
    if (a.flag("--realign", false)) return fail("--alt-ali / --realign: use the `align` module");
    if (a.real("--min-seq-id", 0.0) != 0.0) return fail("--min-seq-id > 0: use the module-by-module path");
    if (a.integer("--max-accept", INT_MAX) != INT_MAX || a.integer("--max-rejected", INT_MAX) != INT_MAX)
        return fail("--max-accept / --max-rejected: use the `align` module");
    if (!a.flag("--simple-best-hit", true) || a.integer("--suboptimal-hits", 0) != 0 || a.integer("--aggregation-mode", 0) != 0)
        return fail("the fused aggregation implements --simple-best-hit 1 --suboptimal-hits 0 --aggregation-mode 0; use the glue modules otherwise");
    return 0;
}

// --prefilter-mode (M/src/workflow/Search.cpp:337-350): 0 the k-mer prefilter, 1 the exhaustive ungapped scan; what is not
// implemented is refused by value
int checkPrefilterMode(const Args &a) {
    if (int rc = ungappedPrefilterModeCheck(a)) return rc;
    if (a.integer("--prefilter-mode", 0) == 1 && a.integer("--num-iterations", 1) > 1)
        return fail("--prefilter-mode 1 with --num-iterations > 1 is not implemented (profile queries in the ungapped prefilter)");
    return 0;
}

// DB writers fed by the pipeline's sinks
struct Sinks {
    const SeqDb *qdb = nullptr, *tdb = nullptr;
    sddb::Writer pref, aln;
    bool wantPref = false, wantAln = false, failed = false;
    sd_aln_criteria crit;
    sd_alntext *text = nullptr;
    std::string buf;
    std::vector<uint32_t> order, counts;
    std::vector<int32_t> qlen;
    ~Sinks() { if (text) sd_alntext_destroy(text); }

    static void onPref(void *u, uint32_t first, uint32_t nQ, const sd_hit *rows, const uint32_t *counts, uint32_t W) {
        Sinks *s = (Sinks *) u;
        if (!s->wantPref || s->failed) return;
        std::string &b = s->buf;
        for (uint32_t i = 0; i < nQ; i++) {
            b.clear();
            const sd_hit *row = rows + (size_t) i * W;
            for (uint32_t x = 0; x < counts[i]; x++) {
                appendPrefRow(b, s->tdb->keys[row[x].seqId], row[x].score, row[x].diagonal);
            }
            if (!s->pref.write(s->qdb->keys[first + i], b.data(), b.size())) s->failed = true;
        }
    }
    static void onAln(void *u, uint32_t first, uint32_t nQ, uint32_t nRes, const uint32_t *resQ, const uint32_t *resT,
                      const sd_sw_result *res, const uint8_t *ident, const char *pool) {
        Sinks *s = (Sinks *) u;
        if (!s->wantAln || s->failed) return;
        s->qlen.resize(nQ);
        for (uint32_t i = 0; i < nQ; i++) s->qlen[i] = s->qdb->lens[first + i];
        s->order.resize(std::max<uint32_t>(nRes, 1));
        s->counts.assign(std::max<uint32_t>(nQ, 1), 0);
        if (sd_host_accept_sort(&s->crit, nQ, nRes, resQ, resT, res, ident, s->qlen.data(), s->tdb->lens.data(), s->tdb->keys.data(),
                                s->order.data(), s->counts.data()) != SD_OK ||
            sd_alntext_format(s->text, &s->crit, nQ, s->counts.data(), s->order.data(), resT, res, ident, pool, s->qlen.data(),
                              s->tdb->lens.data(), s->tdb->keys.data()) != SD_OK) {
            s->failed = true;
            return;
        }
        const char *txt;
        const uint64_t *eoff;
        sd_alntext_get(s->text, &txt, &eoff);
        for (uint32_t i = 0; i < nQ; i++)
            if (!s->aln.write(s->qdb->keys[first + i], txt + eoff[i], (size_t) (eoff[i + 1] - eoff[i]))) s->failed = true;
    }
};

// Several ranks leave NAME.<rank> + NAME.<rank>.index each; rank 0 turns them into one DB with split data files -- NAME.0 ..
// NAME.<world-1> and one NAME.index whose offsets run through their concatenation, the layout the reference's multi-threaded
// DBWriter leaves and every reader here understands (M/src/commons/DBWriter.cpp:540-600)
bool mergeRankDbs(const std::string &name, int world, int dbtype, std::string *err) {
    struct Row {
        uint32_t key;
        uint64_t off, len;
    };
    std::vector<Row> rows;
    uint64_t base = 0;
    for (int r = 0; r < world; r++) {
        const std::string part = name + "." + std::to_string(r);
        std::ifstream in(part + ".index");
        if (!in) {
            *err = "cannot read " + part + ".index";
            return false;
        }
        unsigned long long k, o, l;
        while (in >> k >> o >> l) rows.push_back({(uint32_t) k, base + o, l});
        struct stat st;
        if (stat(part.c_str(), &st) != 0) {
            *err = "cannot stat " + part;
            return false;
        }
        base += (uint64_t) st.st_size;
        remove((part + ".index").c_str());
        remove((part + ".dbtype").c_str());
    }
    std::sort(rows.begin(), rows.end(), [](const Row &x, const Row &y) { return x.key < y.key; });
    FILE *f = fopen((name + ".index").c_str(), "wb");
    if (!f) {
        *err = "cannot write " + name + ".index";
        return false;
    }
    for (const Row &w : rows) fprintf(f, "%u\t%llu\t%llu\n", w.key, (unsigned long long) w.off, (unsigned long long) w.len);
    fclose(f);
    f = fopen((name + ".dbtype").c_str(), "wb");
    if (!f) {
        *err = "cannot write " + name + ".dbtype";
        return false;
    }
    const int32_t t = dbtype;
    fwrite(&t, sizeof(t), 1, f);
    fclose(f);
    return true;
}

int runSearch(const Args &a, bool withClusters) {
    if (a.pos.size() != 4)
        return fail(withClusters ? "usage: clustersearch <querySetDB> <targetSetDB> <out.tsv> <tmpDir> [options]"
                                 : "usage: search <queryDB> <targetDB> <alignmentDB> <tmpDir> [options]");
    if (int rc = checkWorkflowFlags(a)) return rc;
    if (int rc = checkPrefilterMode(a)) return rc;
    const bool ungapped = a.integer("--prefilter-mode", 0) == 1;
    if (a.integer("--num-iterations", 1) > 1) return fail("--num-iterations > 1: run the iterations with the modules (prefilter, align, result2profile)");
    const int rank = (int) a.integer("--rank", envInt("RANK", 0)), world = (int) a.integer("--world-size", envInt("WORLD_SIZE", 1));
    const int device = a.has("--device") ? (int) a.integer("--device", 0) : envInt("LOCAL_RANK", 0);
    sd_search_params par;
    fillParams(a, par, withClusters);
    const std::string tmpDir = a.pos[3];
    mkdir(tmpDir.c_str(), 0777);

    HostH host;
    if (sd_host_create(par.threads, &host.h) != SD_OK) return fail("sd_host_create failed");
    std::string err;
    DbPair db;   // (loaded for this run alone: not a workflow's resident DB)
    if (!db.open(a.pos[0], a.pos[1], host.h, false, true, &err)) return fail(err);
    const bool sameDb = db.sameDb;
    const SeqDb *const qdb = db.qdb, *const tdb = db.tdb.get();
    SetInfo qs, tsOwn;
    const SetInfo *qsP = nullptr, *tsP = nullptr;
    if (withClusters) {
        if (!qs.load(a.pos[0], true, &err)) return fail(err);
        if (!sameDb && !tsOwn.load(a.pos[1], true, &err)) return fail(err);
        qsP = &qs;
        tsP = sameDb ? &qs : &tsOwn;
    }
    par.profileQueries = qdb->profile ? 1 : 0;
    if (ungapped && qdb->profile) return fail("profile query databases are not implemented in the ungapped prefilter (--prefilter-mode 1)");
    SetDbArrays tv, qv;
    tv.fill(*tdb, tsP);
    qv.fill(*qdb, qsP);
    info(a, "Query database size: %u type: %s\nTarget database size: %u type: Aminoacid\n", qdb->n, qdb->profile ? "Profile" : "Aminoacid", tdb->n);

    SearchH S;
    int rc;
    if (ungapped) {
        // --prefilter-mode 1: the scan as the prefilter stage; no k-mer index is read, built or held
        rc = sd_search_create_ungapped(device, &par, &tv.view, &S.s);
    } else {
        // TARGET.idx (createindex layout) instead of a rebuild when its parameters match this run
        const int k = par.kmerSize ? par.kmerSize : sd_host_auto_kmer_size(tdb->totalResidues());
        const int thr = par.profileQueries ? 0 : sd_host_kmer_threshold(par.sensitivity, k);
        LoadedIndex loaded;
        std::string why;
        const int got = loadTargetIndex(a.pos[1], k, thr, par.mask ? 1 : 0, tdb->n, tdb->totalResidues(), loaded, &why);
        if (got < 0) return fail(why);
        if (got == 0) {
            sd_index_view v;
            v.kmerSize = k;
            v.kmerThr = thr;
            v.kmerOffsets = loaded.offsets.data();
            v.kmerBlockBase = loaded.blockBase.empty() ? nullptr : loaded.blockBase.data();
            v.entrySeq = loaded.entrySeq.data();
            v.entryPos = loaded.entryPos.data();
            v.nEntries = loaded.nEntries;
            v.maskedResidues = loaded.masked.data();
            v.nMaskedResidues = 0;
            info(a, "Use index %s.idx\n", a.pos[1].c_str());
            rc = sd_search_create_indexed(device, &par, &tv.view, &v, &S.s);
        } else {
            if (sddb::fileExists(a.pos[1] + ".idx.index")) info(a, "Index file not used: %s\n", why.c_str());
            rc = sd_search_create(device, &par, &tv.view, &S.s);
        }
    }
    if (rc == SD_ENODEVICE) return failNoDevice(rc, "sd_search_create");
    if (rc != SD_OK) return fail("sd_search_create failed (" + std::to_string(rc) + ")");
    uint64_t st[16];
    double tm[16];
    sd_search_stats(S.s, st, tm);
    if (ungapped) info(a, "Prefilter mode 1: exhaustive ungapped scan, no index table\n");
    else info(a, "Index table: k-mer size %llu, k-mer threshold %llu, %llu entries, %llu masked residues (%.2f s host, %.2f s upload)\n",
         (unsigned long long) st[11], (unsigned long long) st[12], (unsigned long long) st[9], (unsigned long long) st[10], tm[0], tm[1]);

    // query ranges of this rank: whole query sets (contiguous id ranges), dealt greedily by residue count; a plain search
    // deals contiguous blocks of queries
    std::vector<uint32_t> rb, re;
    if (world <= 1) {
        rb.push_back(0);
        re.push_back(qdb->n);
    } else if (withClusters) {
        std::vector<uint32_t> first(qs.nSets, UINT32_MAX), last(qs.nSets, 0);
        std::vector<uint64_t> resOfSet(qs.nSets, 0);
        for (uint32_t i = 0; i < qdb->n; i++) {
            const uint32_t sId = qv.setId[i];
            first[sId] = std::min(first[sId], i);
            last[sId] = std::max(last[sId], i + 1);
            resOfSet[sId] += (uint64_t) qdb->lens[i];
        }
        for (uint32_t sId = 0; sId < qs.nSets; sId++)
            if (first[sId] != UINT32_MAX) {
                uint64_t members = 0;
                for (uint32_t i = first[sId]; i < last[sId]; i++) members += qv.setId[i] == sId;
                if (members != last[sId] - first[sId]) return fail("the members of a query set are not contiguous in the DB; multi-rank sharding needs createsetdb's layout");
            }
        std::vector<uint32_t> mine(std::max<uint32_t>(qs.nSets, 1));
        uint32_t nMine = 0;
        sd_shard_query_sets(resOfSet.data(), qs.nSets, (uint32_t) world, (uint32_t) rank, mine.data(), &nMine);
        for (uint32_t x = 0; x < nMine; x++)
            if (first[mine[x]] != UINT32_MAX) {
                // neighbouring sets of this rank merge into one range
                if (!re.empty() && re.back() == first[mine[x]]) re.back() = last[mine[x]];
                else {
                    rb.push_back(first[mine[x]]);
                    re.push_back(last[mine[x]]);
                }
            }
    } else {
        const uint64_t per = ((uint64_t) qdb->n + world - 1) / world;
        rb.push_back((uint32_t) std::min<uint64_t>(qdb->n, per * rank));
        re.push_back((uint32_t) std::min<uint64_t>(qdb->n, per * (rank + 1)));
    }

    // DB outputs: `search` always writes the alignment DB (and pref_0 under <tmpDir>); clustersearch only with --keep-dbs 1
    Sinks sinks;
    sinks.qdb = qdb;
    sinks.tdb = tdb;
    const bool dbs = !withClusters || a.integer("--keep-dbs", 0) != 0;
    const std::string rankSuffix = world > 1 ? "." + std::to_string(rank) : "";
    if (dbs) {
        memset(&sinks.crit, 0, sizeof(sinks.crit));
        sinks.crit.evalThr = par.evalThr;
        sinks.crit.alnLenThr = par.alnLenThr;
        sinks.crit.covMode = par.covMode;
        sinks.crit.covThr = par.covThr;
        sinks.crit.swMode = 2;
        sinks.crit.addBacktrace = 1;
        sinks.crit.realignMaxSeqs = INT_MAX;
        sinks.crit.maxAccept = (uint32_t) INT_MAX;
        sinks.crit.maxRejected = (uint32_t) INT_MAX;
        sd_alntext_create(&sinks.text);
        const std::string alnPath = (withClusters ? tmpDir + "/result" : a.pos[2]) + rankSuffix;
        if (!sinks.pref.open(tmpDir + "/pref_0" + rankSuffix, sddb::DBTYPE_PREFILTER_RES, &err)) return fail(err);
        if (!sinks.aln.open(alnPath, sddb::DBTYPE_ALIGNMENT_RES, &err)) return fail(err);
        sinks.wantPref = sinks.wantAln = true;
        sd_search_set_sinks(S.s, Sinks::onPref, Sinks::onAln, &sinks);
    }
    // the ranks meet over TCP at MASTER_ADDR:MASTER_PORT+1: the RCCL unique id (clustersearch), the merge of the per-rank DBs
    sd_tcp *tcp = nullptr;
    struct TcpClose {
        sd_tcp *&t;
        ~TcpClose() { if (t) sd_tcp_close(t); }
    } tcpClose{tcp};
    // The one exchange of the path: every rank's cluster records to rank 0, which writes the TSV from the gathered buffer -- round by
    // round behind the running search (sd_gather_stream_*: a rank's ranges in eight rounds; the records of a range leave through the
    // stream's records sink when the range is finalised).  Over RCCL (sd_gather_results per round); ranks that share a device -- RCCL
    // refuses that, a one-GPU test rig -- hand their records over the TCP rendezvous instead.
    sd_comm *comm = nullptr;
    sd_gather_stream *gstream = nullptr;
    struct GatherClose {   // (declared behind tcpClose: destroyed first -- the worker thread uses the socket / the communicator)
        sd_gather_stream *&g;
        sd_comm *&c;
        ~GatherClose() {
            if (g) sd_gather_stream_destroy(g);
            if (c) sd_comm_destroy(c);
        }
    } gatherClose{gstream, comm};
    bool sharedDevice = false;
    if (world > 1) {
        const char *addrEnv = getenv("MASTER_ADDR");
        const std::string addr = addrEnv && *addrEnv ? addrEnv : "127.0.0.1";
        const int port = (int) a.integer("--comm-port", envInt("MASTER_PORT", 29500) + 1);
        if (sd_tcp_connect(addr.c_str(), port, world, rank, &tcp) != SD_OK)
            return fail("rendezvous of the ranks at " + addr + ":" + std::to_string(port) + " failed");
    }
    if (world > 1 && withClusters) {
        // the physical GPU of every rank (host name + PCI bus id, not the local ordinal: ranks on different nodes, or ranks that
        // each see their GPU as device 0 through HIP_VISIBLE_DEVICES, are not sharing) -> does each rank have a GPU of its own?
        uint64_t gpuId = 0;
        if (sd_device_identity(device, &gpuId) != SD_OK) return fail("sd_device_identity failed");
        int32_t devs[2] = {(int32_t) (uint32_t) gpuId, (int32_t) (uint32_t) (gpuId >> 32)};
        std::vector<int32_t> allDevs((size_t) world * 2, 0);
        uint64_t got = 0;
        if (sd_tcp_gather(tcp, devs, sizeof(devs), nullptr, allDevs.data(), allDevs.size() * sizeof(int32_t), &got) != SD_OK)
            return fail("rendezvous of the ranks failed (devices)");
        int32_t shared = 0;
        if (rank == 0)
            for (int x = 0; x < world; x++)
                for (int y = 0; y < x; y++)
                    if (allDevs[(size_t) x * 2] == allDevs[(size_t) y * 2] && allDevs[(size_t) x * 2 + 1] == allDevs[(size_t) y * 2 + 1]) shared = 1;
        if (sd_tcp_bcast(tcp, &shared, sizeof(shared)) != SD_OK) return fail("rendezvous of the ranks failed");
        sharedDevice = shared != 0;
        constexpr uint32_t GATHER_ROUNDS = 8;
        std::vector<uint32_t> roundOfRange(rb.size());
        for (size_t i = 0; i < rb.size(); i++) roundOfRange[i] = (uint32_t) (i * GATHER_ROUNDS / rb.size());
        if (!sharedDevice) {
            char uid[128];
            if (rank == 0 && sd_comm_unique_id(uid) != SD_OK) return fail("sd_comm_unique_id failed (librccl not loadable?)");
            if (sd_tcp_bcast(tcp, uid, sizeof(uid)) != SD_OK) return fail("broadcast of the RCCL unique id failed");
            if (sd_comm_init(device, world, rank, uid, &comm) != SD_OK) return fail("sd_comm_init failed");
            rc = sd_gather_stream_begin(comm, 0, (uint32_t) rb.size(), roundOfRange.data(), GATHER_ROUNDS, nullptr, 0, 1, &gstream);
        } else {
            rc = sd_gather_stream_begin_tcp(tcp, world, rank, (uint32_t) rb.size(), roundOfRange.data(), GATHER_ROUNDS, nullptr, 0, 1, &gstream);
        }
        if (rc != SD_OK) return fail("sd_gather_stream_begin failed (" + std::to_string(rc) + ")");
        sd_search_set_records_sink(S.s, sd_gather_stream_sink, gstream);
    }
    std::vector<sd_search_result *> results(std::max<size_t>(rb.size(), 1), nullptr);
    if (!rb.empty()) {
        // the TSV (this rank's, or rank 0's from the gathered buffers) is written from the cluster records: the stream builds them range by
        // range while its lanes work (sd_search_result_records below is then a copy, not a second pass over every entry's hits)
        if (withClusters) sd_search_set_want_records(S.s, 1);
        rc = sd_search_stream(S.s, &qv.view, sameDb ? 1 : 0, (uint32_t) rb.size(), rb.data(), re.data(), results.data());
        sd_search_set_records_sink(S.s, nullptr, nullptr);
        if (rc != SD_OK) return fail(std::string("sd_search_stream: ") + sd_search_last_error(S.s));
    }
    struct Free {
        std::vector<sd_search_result *> &v;
        ~Free() { for (sd_search_result *r : v) if (r) sd_search_result_destroy(r); }
    } freeResults{results};
    if (dbs) {
        if (sinks.failed) return fail("writing the prefilter / alignment DB failed");
        if (!sinks.pref.close(&err) || !sinks.aln.close(&err)) return fail(err);
    }
    // (the gather's last rounds: the socket / the communicator are the worker thread's until then)
    const void *gathered = nullptr;
    uint64_t gatheredBytes = 0;
    if (gstream) {
        rc = sd_gather_stream_wait(gstream, nullptr, nullptr, &gatheredBytes, &gathered);
        if (rc == SD_EMISMATCH) return fail("a rank closed its gather before all its query sets had arrived (its search failed): no result is written");
        if (rc != SD_OK) return fail("the gather of the cluster records failed (" + std::to_string(rc) + ")" + (comm ? std::string(": ") + sd_comm_last_error(comm) : std::string()));
        info(a, "records gathered %s: %llu bytes from %d ranks\n", sharedDevice ? "over TCP (ranks share a device)" : "over RCCL", (unsigned long long) gatheredBytes, world);
    }
    if (world > 1) {
        if (dbs) {   // every rank's DB parts are closed: rank 0 makes them one DB (split data files, one index)
            uint8_t done = 1;
            std::vector<uint8_t> allDone((size_t) world, 0);
            uint64_t got = 0;
            if (sd_tcp_gather(tcp, &done, 1, nullptr, allDone.data(), allDone.size(), &got) != SD_OK) return fail("rendezvous of the ranks failed (DB parts)");
            if (rank == 0) {
                const std::string alnPath = withClusters ? tmpDir + "/result" : a.pos[2];
                if (!mergeRankDbs(tmpDir + "/pref_0", world, sddb::DBTYPE_PREFILTER_RES, &err)) return fail(err);
                if (!mergeRankDbs(alnPath, world, sddb::DBTYPE_ALIGNMENT_RES, &err)) return fail(err);
            }
        }
    }
    sd_search_stats(S.s, st, tm);
    info(a, "%llu prefilter hits, %llu pairs aligned; prefilter %.2f s | align %.2f s | aggregate %.2f s | clusterhits %.2f s | total %.2f s\n",
         (unsigned long long) st[4], (unsigned long long) st[5], tm[3], tm[6], tm[8], tm[9], tm[11]);
    const uint64_t notComputed = st[14];
    if (notComputed) fprintf(stderr, "sdgpu %s: %s\n", a.module.c_str(), sd_search_last_error(S.s));
    if (!withClusters) return notComputed ? 1 : 0;

    // summarizeresults: this rank's part, then rank 0 concatenates in rank order
    std::string qn, tn, qsrc, tsrc;
    std::vector<uint64_t> qno, tno, qso, tso;
    {
        std::vector<std::string> names(qdb->n);
        for (uint32_t i = 0; i < qdb->n; i++) names[i] = qdb->keys[i] < qs.nameOfKey.size() ? qs.nameOfKey[qdb->keys[i]] : std::string();
        packNames(names, qn, qno);
        names.assign(tdb->n, std::string());
        for (uint32_t i = 0; i < tdb->n; i++) names[i] = tdb->keys[i] < tsP->nameOfKey.size() ? tsP->nameOfKey[tdb->keys[i]] : std::string();
        packNames(names, tn, tno);
        packNames(qs.sourceOfSet, qsrc, qso);
        packNames(tsP->sourceOfSet, tsrc, tso);
    }
    // one rank: its cluster records (every range's clusters, in range order); several: what the gather brought to rank 0
    std::vector<char> rec;
    const char *toWrite = nullptr;
    uint64_t toWriteBytes = 0;
    if (world == 1) {
        for (size_t r = 0; r < rb.size(); r++) {
            uint64_t need = 0;
            rc = sd_search_result_records(results[r], nullptr, 0, &need);
            if (rc != SD_OK) return fail("sd_search_result_records failed (" + std::to_string(rc) + ")");
            const size_t at = rec.size();
            rec.resize(at + need);
            rc = sd_search_result_records(results[r], rec.data() + at, need, &need);
            if (rc != SD_OK) return fail("sd_search_result_records failed (" + std::to_string(rc) + ")");
        }
        toWrite = rec.data();
        toWriteBytes = rec.size();
    } else {
        toWrite = (const char *) gathered;
        toWriteBytes = gatheredBytes;
    }
    uint64_t nClu = 0, nHit = 0;
    if (rank == 0) {
        // (gathered records came over the wire: indices are checked against the tables they will index)
        rc = sd_records_check(toWrite, toWriteBytes, (uint32_t) (qso.size() - 1), (uint32_t) (tso.size() - 1), (uint32_t) (qno.size() - 1),
                              (uint32_t) (tno.size() - 1), nullptr, nullptr);
        if (rc != SD_OK) return fail("the gathered cluster records are truncated or index outside the name tables");
        rc = sd_records_write_tsv(toWrite, toWriteBytes, a.pos[2].c_str(), 0, 0, qn.data(), qno.data(), tn.data(), tno.data(),
                                  qsrc.data(), qso.data(), tsrc.data(), tso.data(), 0, &nClu, &nHit);
        if (rc != SD_OK) return fail("sd_records_write_tsv failed (" + std::to_string(rc) + ")");
        info(a, "%llu clusters with %llu hits written\n", (unsigned long long) nClu, (unsigned long long) nHit);
    }
    return notComputed ? 1 : 0;
}

}  // namespace

// the ancillary files a DB derived from a sequence DB shares with it (DBReader::softlinkDb(..., SEQUENCE_ANCILLARY))
static void softlinkSequenceAncillary(const std::string &from, const std::string &to) {
    for (const char *suffix : {"_h", "_h.index", "_h.dbtype", ".lookup", ".source"}) {
        const std::string src = from + suffix, dst = to + suffix;
        ::remove(dst.c_str());
        if (sddb::fileExists(src)) {
            char *real = realpath(src.c_str(), nullptr);
            if (real) {
                if (symlink(real, dst.c_str()) != 0) { /* best effort, as the reference */ }
                free(real);
            }
        }
    }
}

int r2pSetupFromArgs(const Args &a, R2pSetup &s) {
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    if (a.integer("--profile-output-mode", 0) != 0) return fail("--profile-output-mode 0 only");
    if (a.integer("--pseudo-cnt-mode", 0) != 0) return fail("--pseudo-cnt-mode 1 needs the context library (not built in)");
    if (a.flag("--allow-deletion", false)) return fail("--allow-deletion 1 is not supported");
    if (a.multi("--sub-mat", "aa", "blosum62.out") != "blosum62.out") return fail("--sub-mat: only blosum62.out is built into this path");
    s.qid = a.str("--qid", "0.0");
    sd_r2p_params &p = s.par;
    memset(&p, 0, sizeof(p));
    p.filterMsa = (int32_t) a.integer("--filter-msa", 1);
    p.filterMinEnable = (int32_t) a.integer("--filter-min-enable", 0);
    p.filterMaxSeqId = (float) a.real("--max-seq-id", 0.9);
    p.qid = s.qid.c_str();
    p.qsc = (float) a.real("--qsc", -20.0);
    p.covMSAThr = (float) a.real("--cov", 0.0);
    p.Ndiff = (int32_t) a.integer("--diff", 1000);
    p.pcMode = 0;
    p.pca = (float) strtod(a.multi("--pca", "substitution", "1.1").c_str(), nullptr);
    p.pcb = (float) strtod(a.multi("--pcb", "substitution", "4.1").c_str(), nullptr);
    p.wg = a.flag("--wg", false) ? 1 : 0;
    p.compBiasCorr = (int32_t) a.integer("--comp-bias-corr", 1);
    p.maskProfile = (int32_t) a.integer("--mask-profile", 1);
    p.maskProb = a.real("--mask-prob", 0.9);
    double evalThr = a.real("-e", 0.001), evalProfile = a.real("--e-profile", 0.001);
    s.evalProfile = (evalThr < evalProfile) ? evalThr : evalProfile;   // result2profile.cpp:33
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// result2profile <queryDB> <targetDB> <alignmentDB> <profileDB>   (M/src/util/result2profile.cpp:16-322): the host step
// between search iterations.  The arithmetic is sd_r2p_batch of the C ABI; this is the DB side.
int result2profileModule(const Args &a) {
    if (a.pos.size() != 4) return fail("usage: result2profile <queryDB> <targetDB> <alignmentDB> <profileDB> [options]");
    R2pSetup RS;
    if (int rcS = r2pSetupFromArgs(a, RS)) return rcS;
    const sd_r2p_params &p = RS.par;
    const double evalProfile = RS.evalProfile;
    const int threads = threadsOf(a);
    Lap lap("result2profile");
    HostH host;
    if (host.open(threads) != SD_OK) return fail("sd_host_create failed");
    std::string err;
    DbPair db;
    if (!db.open(a.pos[0], a.pos[1], host.h, true, false, &err)) return fail(err);
    const bool sameDb = db.sameDb;
    const SeqDb *const qdb = db.qdb, *const tdb = db.tdb.get();
    if (tdb->profile) return fail("Only the query OR the target database can be a profile database");
    lap.mark("load DBs");
    sddb::Reader aln;
    if (!aln.open(a.pos[2], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    sd_r2p *r2p = nullptr;
    if (sd_r2p_create(&r2p) != SD_OK) return fail("sd_r2p_create failed");
    std::unique_ptr<sd_r2p, void (*)(sd_r2p *)> guard(r2p, sd_r2p_destroy);
    // the position-specific weights -- the O(columns^2 x rows) part -- run on the GPU (sd_r2p_batch_device); --profile-weights-host 1
    // asks for the host implementation explicitly (a box without a GPU, the CPU-side tests).  No silent fallback.
    const bool hostWeights = a.integer("--profile-weights-host", 0) != 0;
    sd_ctx *r2pCtx = nullptr;
    bool ownCtx = true;
    const int device = a.has("--device") ? (int) a.integer("--device", 0) : envInt("LOCAL_RANK", 0);
    if (!hostWeights) {
        int rcCtx = SD_OK;
        if (resident().enabled) {
            r2pCtx = resident().ctx(device, &rcCtx);
            ownCtx = false;
        } else {
            rcCtx = sd_ctx_create(device, &r2pCtx);
        }
        if (rcCtx != SD_OK)
            return failNoDevice(rcCtx, "sd_ctx_create", "result2profile computes the sequence weights on the GPU (--profile-weights-host 1 selects the "
                                                        "host implementation)");
    }
    std::unique_ptr<sd_ctx, void (*)(sd_ctx *)> ctxGuard(ownCtx ? r2pCtx : nullptr, sd_ctx_destroy);
    lap.mark("r2p object + context");
    sddb::Writer out;
    if (!out.open(a.pos[3], sddb::DBTYPE_HMM_PROFILE, &err)) return fail(err);
    const size_t n = aln.size();
    const size_t chunk = 4096;
    double tParse = 0, tCompute = 0, tWrite = 0;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tLoaded = now();
    std::vector<uint8_t> qLetters;
    std::vector<uint64_t> qOff, edgeOff, btOff;
    std::vector<uint32_t> edgeT, keys;
    std::vector<int32_t> eQ, eT;
    std::vector<uint8_t> eRealign;
    std::string pool;
    std::vector<char> profiles;
    // rows without a backtrace (a cluster DB's one-column rows) are aligned to their centre here (:224-233), by sd_r2p_realign; the
    // target sequences go to the device once per run, or are the workflow's resident set
    SeqSetH realignTargets;
    uint64_t pairsRealigned = 0, realignUploaded = 0;
    double tRealign = 0;
    struct ParsedEntry {
        bool valid = false;
        size_t qId = 0;
        std::vector<uint32_t> edgeT;
        std::vector<uint8_t> realign;
        std::vector<int32_t> eQ, eT;
        std::vector<uint64_t> btEnd;
        std::string pool, error;
    };
    std::vector<ParsedEntry> parsed;
    for (size_t c0 = 0; c0 < n; c0 += chunk) {
        const size_t c1 = std::min(n, c0 + chunk);
        const double t0 = now();
        qLetters.clear();
        qOff.assign(1, 0);
        edgeOff.assign(1, 0);
        btOff.assign(1, 0);
        edgeT.clear();
        eQ.clear();
        eT.clear();
        eRealign.clear();
        keys.clear();
        pool.clear();
        // the entries of the chunk parsed on all threads, each into lists of its own, then laid out back to back in entry order
        parsed.resize(c1 - c0);
#pragma omp parallel for schedule(dynamic, 16)
        for (size_t id = c0; id < c1; id++) {
            ParsedEntry &pe = parsed[id - c0];
            pe.valid = false;
            pe.error.clear();
            pe.edgeT.clear();
            pe.eQ.clear();
            pe.eT.clear();
            pe.realign.clear();
            pe.btEnd.clear();
            pe.pool.clear();
            const uint32_t qKey = aln.key(id);
            pe.qId = qdb->rd.idOfKey(qKey);
            if (pe.qId == SIZE_MAX) continue;   // "Invalid query sequence": skipped (result2profile.cpp:173-176)
            pe.valid = true;
            const char *d = aln.data(id);
            while (*d != '\0') {
                const char *ls = d;
                while (*d != '\n' && *d != '\0') d++;
                const char *le = d;
                if (*d == '\n') d++;
                // columns: tKey bits seqId eval qStart qEnd qLen tStart tEnd tLen [cigar]
                const char *col[12];
                int nc = 0;
                col[nc++] = ls;
                for (const char *c = ls; c < le && nc < 12; c++)
                    if (*c == '\t') col[nc++] = c + 1;
                const uint32_t tKey = (uint32_t) strtoul(ls, nullptr, 10);
                if (tKey == qKey && sameDb) continue;   // the query repeated in the same database case (:186-195)
                double evalue = 0.0;
                if (nc >= 4) evalue = strtod(col[3], nullptr);
                if (!(evalue < evalProfile)) continue;
                const size_t tId = tdb->rd.idOfKey(tKey);
                if (tId == SIZE_MAX) {
                    pe.error = "Sequence " + std::to_string(tKey) + " does not exist in target sequence database";
                    break;
                }
                pe.edgeT.push_back((uint32_t) tId);
                if (nc < 11) {   // at most Matcher::ALN_RES_WITHOUT_BT_COL_CNT columns: no backtrace to parse (:224-233)
                    pe.realign.push_back(1);
                    pe.eQ.push_back(0);
                    pe.eT.push_back(0);
                    pe.btEnd.push_back(pe.pool.size());
                    continue;
                }
                pe.realign.push_back(0);
                pe.eQ.push_back((int32_t) strtol(col[4], nullptr, 10));
                pe.eT.push_back((int32_t) strtol(col[7], nullptr, 10));
                // Matcher::uncompressAlignment (Matcher.cpp:187-201)
                size_t count = 0;
                for (const char *c = col[10]; c < le; c++) {
                    if (*c >= '0' && *c <= '9') count = count * 10 + (size_t) (*c - '0');
                    else {
                        pe.pool.append(count == 0 ? 1 : count, *c);
                        count = 0;
                    }
                }
                pe.btEnd.push_back(pe.pool.size());
            }
        }
        for (size_t id = c0; id < c1; id++) {
            const ParsedEntry &pe = parsed[id - c0];
            if (!pe.error.empty()) return fail(pe.error);
            if (!pe.valid) continue;
            keys.push_back(aln.key(id));
            qLetters.insert(qLetters.end(), qdb->residues.begin() + qdb->offsets[pe.qId], qdb->residues.begin() + qdb->offsets[pe.qId + 1]);
            qOff.push_back(qLetters.size());
            edgeT.insert(edgeT.end(), pe.edgeT.begin(), pe.edgeT.end());
            eQ.insert(eQ.end(), pe.eQ.begin(), pe.eQ.end());
            eT.insert(eT.end(), pe.eT.begin(), pe.eT.end());
            eRealign.insert(eRealign.end(), pe.realign.begin(), pe.realign.end());
            const uint64_t base = pool.size();
            pool.append(pe.pool);
            for (uint64_t e : pe.btEnd) btOff.push_back(base + e);
            edgeOff.push_back(edgeT.size());
        }
        const uint32_t nQ = (uint32_t) keys.size();
        profiles.assign(qOff.back() * 25 + 1, 0);
        uint64_t nRealign = 0;
        for (uint8_t f : eRealign) nRealign += f;
        if (nRealign) {
            if (qdb->profile) return fail("rows without a backtrace next to a profile query DB are not supported");
            // the reference builds this Matcher from --gap-open, --gap-extend and --comp-bias-corr-scale; the stage has the presets only
            if (a.multi("--gap-open", "aa", "11") != "11" || a.multi("--gap-extend", "aa", "1") != "1")
                return fail("rows without a backtrace are aligned with --gap-open 11 --gap-extend 1 only (other gap costs need other E-value "
                            "parameters than the built-in preset)");
            if (a.real("--comp-bias-corr-scale", 1.0) != 1.0) return fail("rows without a backtrace are aligned with --comp-bias-corr-scale 1 only");
            if (!r2pCtx)
                return fail("the result DB has rows without a backtrace: result2profile aligns them on the GPU, and --profile-weights-host 1 "
                            "runs without a device (align them first: align -a)");
            const double tr0 = now();
            if (!realignTargets.s) {
                const bool had = resident().enabled && resident().seqSets.count(a.pos[1] + "|" + std::to_string(device));
                const int rcT = residentSeqSet(r2pCtx, a.pos[1], device, *tdb, realignTargets);
                if (rcT != SD_OK) return failCtx(r2pCtx, rcT, "sd_seqset_create(targets)");
                if (!had) realignUploaded += tdb->totalResidues();
            }
            // the pool's first guess, as the align module's: about min(qLen, tLen) columns per pair; sd_r2p_realign names what suffices
            uint64_t cap = pool.size() + (1u << 20), est = 0;
            for (uint32_t q = 0; q < nQ; q++)
                for (uint64_t e = edgeOff[q]; e < edgeOff[q + 1]; e++)
                    if (eRealign[e]) est += std::min<uint64_t>(qOff[q + 1] - qOff[q], (uint64_t) tdb->lens[edgeT[e]]) + 16;
            cap += est + est / 4;
            // (test-only: tests/test_gpu_r2p_realign.py sets it to a few bytes so that the retry below runs; no tuning value)
            if (const char *forced = getenv("SD_R2P_REALIGN_POOL")) cap = std::max<uint64_t>(pool.size(), strtoull(forced, nullptr, 10));
            for (bool exact = false;;) {
                const uint64_t heldBytes = pool.size();
                pool.resize(cap);
                uint64_t need = 0, bad = UINT64_MAX;
                const int rcR = sd_r2p_realign(r2pCtx, host.h, nQ, qLetters.data(), qOff.data(), edgeOff.data(), edgeT.data(), eRealign.data(),
                                               p.compBiasCorr, realignTargets.s, tdb->residues.data(), tdb->offsets.data(), tdb->n, eQ.data(),
                                               eT.data(), &pool[0], cap, btOff.data(), &need, &bad);
                if (rcR == SD_ENOMEM && !exact) {
                    pool.resize(heldBytes);
                    cap = need;
                    exact = true;
                    continue;
                }
                if (rcR == SD_EINVAL && bad != UINT64_MAX) {
                    uint32_t q = 0;
                    while (edgeOff[q + 1] <= bad) q++;
                    return fail("the alignment of member " + std::to_string(tdb->keys[edgeT[bad]]) + " with its centre " + std::to_string(keys[q]) +
                                " scores 0: the reference leaves its start positions unset");
                }
                if (rcR != SD_OK) return failCtx(r2pCtx, rcR, "sd_r2p_realign");
                break;
            }
            pool.resize(btOff.back());
            pairsRealigned += nRealign;
            realignUploaded += qOff.back() * 2 + nRealign * 8;
            tRealign += now() - tr0;
        }
        pool.push_back(' ');
        qLetters.push_back(0);
        edgeT.push_back(0);
        eQ.push_back(0);
        eT.push_back(0);
        const double t1 = now();
        const int rc = r2pCtx ? sd_r2p_batch_device(r2pCtx, r2p, &p, nQ, qLetters.data(), qOff.data(), edgeOff.data(), edgeT.data(), eQ.data(),
                                                    eT.data(), pool.data(), btOff.data(), tdb->residues.data(), tdb->offsets.data(),
                                                    profiles.data(), nullptr)
                              : sd_r2p_batch(r2p, &p, nQ, qLetters.data(), qOff.data(), edgeOff.data(), edgeT.data(), eQ.data(), eT.data(),
                                             pool.data(), btOff.data(), tdb->residues.data(), tdb->offsets.data(), profiles.data(), nullptr);
        if (rc != SD_OK) return fail("sd_r2p_batch failed (" + std::to_string(rc) + ")" + (r2pCtx ? std::string(": ") + sd_last_error(r2pCtx) : std::string()));
        const double t2 = now();
        for (uint32_t q = 0; q < nQ; q++)
            if (!out.write(keys[q], profiles.data() + qOff[q] * 25, (size_t) (qOff[q + 1] - qOff[q]) * 25)) return fail("cannot write " + a.pos[3]);
        tParse += t1 - t0;
        tCompute += t2 - t1;
        tWrite += now() - t2;
    }
    lap.mark("chunks");
    info(a, "result2profile: parse %.2f s, profiles %.2f s (%d threads, weights on the %s), write %.2f s\n", tParse, tCompute, threads,
         r2pCtx ? "GPU" : "host", tWrite);
    if (pairsRealigned)
        // (the bytes are an estimate: residues, bias and pair lists; the offset arrays and the batch's own staging are not counted)
        info(a, "result2profile: %llu pairs realigned in %.2f s (%.0f pairs/s), about %llu bytes uploaded for them\n", (unsigned long long) pairsRealigned,
             tRealign, tRealign > 0 ? pairsRealigned / tRealign : 0.0, (unsigned long long) realignUploaded);
    (void) tLoaded;
    if (!out.close(&err)) return fail(err);
    // the profile DB shares the query DB's ancillary files (DBReader::softlinkDb(..., SEQUENCE_ANCILLARY), :318-320)
    softlinkSequenceAncillary(a.pos[0], a.pos[3]);
    lap.mark("close + links");
    info(a, "%zu profiles written\n", n);
    return 0;
}

// profile2consensus <profileDB> <sequenceDB>  (M/src/util/profile2seq.cpp:13-58): the consensus residue of every profile position as
// an amino-acid DB.  One byte per position: a host module (sd_host_profile_consensus).
int profile2consensusModule(const Args &a) {
    if (a.pos.size() != 2) return fail("usage: profile2consensus <profileDB> <sequenceDB> [options]");
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    if (a.multi("--sub-mat", "aa", "blosum62.out") != "blosum62.out") return fail("--sub-mat: only blosum62.out is built into this path");
    const long long maxSeqLen = a.integer("--max-seq-len", 65535);
    if (maxSeqLen < 1 || maxSeqLen > UINT32_MAX) return fail("--max-seq-len " + a.str("--max-seq-len", "") + " is out of range");
    if (sddb::readDbType(a.pos[0]) == -1) return fail(a.pos[0] + ".dbtype not found");
    if (sddb::baseType(sddb::readDbType(a.pos[0])) != sddb::DBTYPE_HMM_PROFILE) return fail(a.pos[0] + " is not a profile database");
    if (sddb::isCompressed(sddb::readDbType(a.pos[0]))) return fail("compressed databases are not supported (" + a.pos[0] + ")");
    HostH host;
    if (host.open(threadsOf(a)) != SD_OK) return fail("sd_host_create failed");
    std::string err;
    sddb::Reader rd;
    if (!rd.open(a.pos[0], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    sddb::Writer out;
    if (!out.open(a.pos[1], sddb::DBTYPE_AMINO_ACIDS, &err)) return fail(err);
    const size_t n = rd.size(), chunk = 65536;
    std::vector<char> raw, text;
    std::vector<uint64_t> byteOff, textOff;
    for (size_t c0 = 0; c0 < n; c0 += chunk) {
        const size_t c1 = std::min(n, c0 + chunk);
        byteOff.assign(1, 0);
        for (size_t id = c0; id < c1; id++) byteOff.push_back(byteOff.back() + (std::max<size_t>(rd.entryLength(id), 1) - 1) / 25 * 25);
        raw.resize(byteOff.back() + 1);
        uint64_t positions = 0;
        for (size_t id = c0; id < c1; id++) {
            memcpy(raw.data() + byteOff[id - c0], rd.data(id), (size_t) (byteOff[id - c0 + 1] - byteOff[id - c0]));
            positions += std::min<uint64_t>((byteOff[id - c0 + 1] - byteOff[id - c0]) / 25, (uint64_t) maxSeqLen) + 1;
        }
        text.resize(positions + 1);
        textOff.resize(c1 - c0 + 1);
        const int rc = sd_host_profile_consensus(host.h, raw.data(), byteOff.data(), (uint32_t) (c1 - c0), (uint32_t) maxSeqLen, text.data(), textOff.data());
        if (rc != SD_OK) return fail("sd_host_profile_consensus failed (" + std::to_string(rc) + "): " + a.pos[0] + " holds a consensus code outside the alphabet");
        for (size_t id = c0; id < c1; id++)
            if (!out.write(rd.key(id), text.data() + textOff[id - c0], (size_t) (textOff[id - c0 + 1] - textOff[id - c0]))) return fail("cannot write " + a.pos[1]);
    }
    if (!out.close(&err)) return fail(err);
    softlinkSequenceAncillary(a.pos[0], a.pos[1]);
    info(a, "%zu consensus sequences written\n", n);
    return 0;
}

// subtractdbs <resultDB A> <resultDB B> <outDB>  (M/src/util/subtractdbs.cpp:13-118): lines of A whose target is not listed
// (with E <= threshold) in B
int subtractdbsModule(const Args &a) {
    if (a.pos.size() != 3) return fail("usage: subtractdbs <resultDB> <resultDB> <outDB>");
    double evalThr = a.real("-e", 0.001), evalProfile = a.real("--e-profile", 0.001);
    evalProfile = (evalThr < evalProfile) ? evalThr : evalProfile;
    std::string err;
    sddb::Reader left, right;
    if (!left.open(a.pos[0], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    if (!right.open(a.pos[1], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::NOSORT, &err)) return fail(err);
    sddb::Writer out;
    if (!out.open(a.pos[2], left.dbtype(), &err)) return fail(err);
    auto evalOf = [](const char *ls, const char *le) {
        int tabs = 0;
        const char *c3 = nullptr;
        for (const char *c = ls; c < le; c++)
            if (*c == '\t' && ++tabs == 3) c3 = c + 1;
        // an alignment record has at least ten columns; anything shorter (prefilter lines) counts as E = 0
        int cols = 1;
        for (const char *c = ls; c < le; c++) cols += (*c == '\t');
        return (cols >= 10 && c3) ? strtod(c3, nullptr) : 0.0;
    };
    // a block of entries on all threads (every thread its own lookup), written in order
    std::vector<std::string> results;
    const size_t block = 8192;
    for (size_t b0 = 0; b0 < left.size(); b0 += block) {
        const size_t b1 = std::min(left.size(), b0 + block);
        results.resize(b1 - b0);
#pragma omp parallel
        {
            std::map<unsigned, bool> lookup;
#pragma omp for schedule(dynamic, 16)
            for (size_t id = b0; id < b1; id++) {
                lookup.clear();
                const char *leftData = left.data(id);
                for (const char *d = leftData; *d != '\0';) {
                    const char *ls = d;
                    while (*d != '\n' && *d != '\0') d++;
                    if (evalOf(ls, d) <= evalProfile) lookup[(unsigned) strtoul(ls, nullptr, 10)] = true;
                    if (*d == '\n') d++;
                }
                const size_t rid = right.idOfKey(left.key(id));
                if (rid != SIZE_MAX) {
                    for (const char *d = right.data(rid); *d != '\0';) {
                        const char *ls = d;
                        while (*d != '\n' && *d != '\0') d++;
                        if (evalOf(ls, d) <= evalProfile) lookup[(unsigned) strtoul(ls, nullptr, 10)] = false;
                        if (*d == '\n') d++;
                    }
                }
                std::string &result = results[id - b0];
                result.clear();
                for (const char *d = leftData; *d != '\0';) {
                    const char *ls = d;
                    while (*d != '\n' && *d != '\0') d++;
                    if (*d == '\n') d++;
                    if (lookup[(unsigned) strtoul(ls, nullptr, 10)]) result.append(ls, d - ls);
                }
            }
        }
        for (size_t id = b0; id < b1; id++)
            if (!out.write(left.key(id), results[id - b0].data(), results[id - b0].size())) return fail("cannot write " + a.pos[2]);
    }
    if (!out.close(&err)) return fail(err);
    return 0;
}

// mergedbs <keyDB> <outDB> <DB1> <DB2> ...  (M/src/util/mergedbs.cpp:8-78): per key of keyDB the concatenation of its entries
int mergedbsModule(const Args &a) {
    if (a.pos.size() < 4) return fail("usage: mergedbs <sequenceDB> <outDB> <resultDB1> <resultDB2> [...]");
    if (a.has("--prefixes") && !a.str("--prefixes", "").empty()) return fail("--prefixes is not supported");
    std::string err;
    sddb::Reader keysDb;
    if (!keysDb.open(a.pos[0], sddb::Reader::USE_INDEX, sddb::Reader::NOSORT, &err)) return fail(err);
    std::vector<std::unique_ptr<sddb::Reader> > in;
    for (size_t i = 2; i < a.pos.size(); i++) {
        in.emplace_back(new sddb::Reader());
        if (!in.back()->open(a.pos[i], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::NOSORT, &err)) return fail(err);
    }
    sddb::Writer out;
    if (!out.open(a.pos[1], in[0]->dbtype(), &err)) return fail(err);
    std::string buf;
    for (size_t id = 0; id < keysDb.size(); id++) {
        const uint32_t key = keysDb.key(id);
        buf.clear();
        for (size_t i = 0; i < in.size(); i++) {
            const size_t e = in[i]->idOfKey(key);
            if (e == SIZE_MAX) continue;
            buf.append(in[i]->data(e), in[i]->entryLength(e) - 1);
        }
        if (!out.write(key, buf.data(), buf.size())) return fail("cannot write " + a.pos[1]);
    }
    if (!out.close(&err)) return fail(err);
    return 0;
}

namespace {

int runModule(int (*fn)(const Args &), const char *name, const std::vector<std::string> &pos, const std::vector<std::string> &flags) {
    std::vector<const char *> argv;
    for (const std::string &s : pos) argv.push_back(s.c_str());
    for (const std::string &s : flags) argv.push_back(s.c_str());
    Args sub;
    sub.module = name;
    std::string err;
    if (!sub.parse((int) argv.size(), argv.data(), &err)) return fail(std::string(name) + ": " + err);
    info(sub, "");
    omp_set_num_threads(threadsOf(sub));
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = fn(sub);
    // the reference prints "Time for processing" after every module of a workflow (M/src/commons/CommandCaller / Timer)
    info(sub, "%s: time for processing %.2f s\n", name, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return rc;
}

std::vector<std::string> with(std::vector<std::string> v, std::initializer_list<std::string> more) {
    v.insert(v.end(), more.begin(), more.end());
    return v;
}

// --split / --split-mode / --split-memory-limit of a workflow (none given: nothing is read or decided, `s` stays as it is).
// The plan is resolved once, here (resolveSplit, sd_mod_prefilter.cpp), and `s` carries its outcome to the steps:
//   a target split with N > 1: --split N --split-mode 0 for the prefilter step; targetSplit = true tells the workflow to run the module
//     chain in this process (the streaming pipeline and the in-memory iterations hold ONE index of the whole target);
//   otherwise (one split, or query-split semantics: the rows of the unsplit run with k taken from residues / N) the split flags are
//     dropped and -k carries the k-mer size, so every path runs as it does today.
int workflowSplit(const Args &a, Args &s, bool &targetSplit) {
    targetSplit = false;
    if (!a.has("--split") && !a.has("--split-mode") && !a.has("--split-memory-limit")) return 0;
    if (a.integer("--prefilter-mode", 0) == 1) return 0;   // the ungapped prefilter has no index to split
    if (a.pos.size() != 4) return 0;                         // the workflow prints its usage line
    std::string err;
    sddb::Reader trd, qrd;
    if (!trd.open(a.pos[1], sddb::Reader::USE_INDEX, sddb::Reader::NOSORT, &err)) return fail(err);
    uint64_t nQ = trd.size();
    if (a.pos[0] != a.pos[1]) {
        if (!qrd.open(a.pos[0], sddb::Reader::USE_INDEX, sddb::Reader::NOSORT, &err)) return fail(err);
        nQ = qrd.size();
    }
    SplitPlan plan;
    Args quiet = a;   // the prefilter step prints the split lines
    quiet.opt["-v"] = "0";
    if (int rc = resolveSplit(quiet, trd, trd.aminoAcidDbSize(), nQ, nullptr, false, plan)) return rc;
    s.opt.erase("--split");
    s.opt.erase("--split-mode");
    if (plan.target) {
        if (envInt("WORLD_SIZE", 1) > 1 || a.integer("--world-size", 1) > 1)
            return fail("a target split (--split " + std::to_string(plan.n) + ") runs on one rank; several ranks shard the query sets against one resident index");
        s.opt["--split"] = std::to_string(plan.n);
        s.opt["--split-mode"] = "0";
        targetSplit = true;
        info(a, "Target split into %d splits: the modules run one after the other in this process; the streaming pipeline and the in-memory "
                "iterations need the whole target index resident and are not used\n", plan.n);
    } else {
        s.opt.erase("--split-memory-limit");
        if (plan.n > 1) s.opt["-k"] = std::to_string(plan.k);
    }
    return 0;
}

// the split flags of a resolved target split for the prefilter step (workflowSplit left them in `a`, or nothing)
std::vector<std::string> withSplit(const Args &a, std::vector<std::string> pref) {
    for (const char *f : {"--split", "--split-mode", "--split-memory-limit"})
        if (a.has(f)) pref = with(pref, {f, a.str(f, "")});
    return pref;
}

// The chains below run `prefilter` in this process.  That module takes a profile target DB on its own (the similar-k-mer index,
// sd_target_build_profile); the modules behind it in these chains do not, so the workflows keep refusing such a target up front, with
// the words DbPair::open uses.
int refuseProfileTarget(const std::string &T) {
    if (sddb::baseType(sddb::readDbType(T)) == sddb::DBTYPE_HMM_PROFILE) return fail("profile target databases are not supported on this path");
    return 0;
}

// `search --num-iterations N` (M/src/workflow/Search.cpp:476-518 builds the per-step parameter strings,
// M/data/workflow/blastpgp.sh:52-140 runs them): iteration 0 with --realign and the profile E-value, prefilter results of
// later iterations minus what is aligned already, the last alignment with the user's -e, merged into the result DB
int iterativeSearch(const Args &a, const std::string &Q, const std::string &T, const std::string &result, const std::string &tmp,
                    const std::string *inMemoryTsv = nullptr) {
    const int numIt = (int) a.integer("--num-iterations", 1);
    if (int rc = refuseProfileTarget(T)) return rc;
    if (!inMemoryTsv) mkdir(tmp.c_str(), 0777);
    const std::string eUser = a.str("-e", "0.001"), eProfile = a.str("--e-profile", "0.001");
    const std::vector<std::string> common = {"--threads", std::to_string(threadsOf(a)), "-v", a.str("-v", "3")};
    std::vector<std::string> pref = with(common, {"-s", a.str("-s", "5.7"), "-k", a.str("-k", "0"), "--max-seqs", a.str("--max-seqs", "300"), "-c",
                                                  a.str("-c", "0"), "--cov-mode", a.str("--cov-mode", "0"), "--min-ungapped-score",
                                                  a.str("--min-ungapped-score", "15"), "--mask", a.str("--mask", "1"), "--mask-prob",
                                                  a.str("--mask-prob", "0.9"), "--comp-bias-corr", a.str("--comp-bias-corr", "1")});
    for (const char *f : {"--device", "--bin-size", "--l2-cache-size", "--chunk-queries"})
        if (a.has(f)) pref = with(pref, {f, a.str(f, "")});
    pref = withSplit(a, pref);
    std::vector<std::string> aln = with(common, {"-a", "1", "--alignment-mode", a.str("--alignment-mode", "2"), "--min-aln-len", a.str("--min-aln-len", "0"),
                                                 "-c", a.str("-c", "0"), "--cov-mode", a.str("--cov-mode", "0"), "--min-seq-id",
                                                 a.str("--min-seq-id", "0"), "--comp-bias-corr", a.str("--comp-bias-corr", "1"),
                                                 "--realign-score-bias", a.str("--realign-score-bias", "-0.2")});
    if (a.has("--device")) aln = with(aln, {"--device", a.str("--device", "0")});
    std::vector<std::string> prof = with(common, {"-e", eProfile, "--e-profile", eProfile, "--mask-profile", a.str("--mask-profile", "1"),
                                                        "--comp-bias-corr", a.str("--comp-bias-corr", "1"), "--filter-msa", a.str("--filter-msa", "1"),
                                                        "--filter-min-enable", a.str("--filter-min-enable", "0"), "--max-seq-id",
                                                        a.str("--max-seq-id", "0.9"), "--qid", a.str("--qid", "0.0"), "--qsc", a.str("--qsc", "-20"),
                                                        "--cov", a.str("--cov", "0"), "--diff", a.str("--diff", "1000"), "--pca",
                                                        a.str("--pca", "substitution:1.100,context:1.400"), "--pcb",
                                                        a.str("--pcb", "substitution:4.100,context:5.800")});
    // result2profile's sequence weights run on the GPU and the module fails without one unless the user asked for the host form:
    // the workflow hands both choices on (device and --profile-weights-host) instead of deciding for the module
    if (a.has("--profile-weights-host")) prof = with(prof, {"--profile-weights-host", a.str("--profile-weights-host", "0")});
    if (a.has("--device")) prof = with(prof, {"--device", a.str("--device", "0")});
    const bool keep = a.integer("--keep-tmp", 0) != 0;   // keep the per-iteration DBs (parity checks at size read them)
    if (inMemoryTsv) {
        // clustersearch without DB files between the modules (sd_mod_iter.cpp): chunks of queries through all iterations in memory,
        // several at a time, into one aggregation.  --keep-tmp 1 wants the per-iteration DBs: the module chain below writes them
        return iterativeClusterSearchInMemory(a, Q, T, *inMemoryTsv, pref, aln, prof, eUser, eProfile);
    }
    // the modules below run in this process: the target DB, its index on the device and its sequence set stay resident between them
    // (sd_cli.h: Resident) instead of being reloaded / rebuilt by every module
    ResidentScope residentScope;
    std::string query = Q;
    for (int step = 0; step < numIt; step++) {
        const std::string s = std::to_string(step), s1 = std::to_string(step - 1);
        const bool last = step == numIt - 1;
        const std::string prefDb = tmp + (step == 0 ? "/pref_0" : "/pref_tmp_" + s);
        if (int rc = runModule(prefilterModule, "prefilter", {query, T, prefDb}, pref)) return rc;
        std::string prefForAln = prefDb;
        if (step >= 1) {
            prefForAln = tmp + "/pref_" + s;
            if (int rc = runModule(subtractdbsModule, "subtractdbs", {prefDb, tmp + "/aln_" + s1, prefForAln},
                                   with(common, {"--e-profile", eProfile, "-e", eUser})))
                return rc;
            if (!keep) sddb::removeDb(prefDb);
        }
        // the realign pass belongs to iteration 0 only; every iteration but the last aligns with the profile E-value
        // (Search.cpp:484-486,497-505)
        std::vector<std::string> alnPar = with(aln, {"-e", last ? eUser : eProfile, "--realign", step == 0 ? "1" : "0"});
        const std::string alnDb = tmp + (step == 0 ? "/aln_0" : "/aln_tmp_" + s);
        if (int rc = runModule(alignModule, "align", {query, T, prefForAln, alnDb}, alnPar)) return rc;
        std::string merged = alnDb;
        if (step > 0) {
            merged = last ? result : tmp + "/aln_" + s;
            if (int rc = runModule(mergedbsModule, "mergedbs", {query, merged, tmp + "/aln_" + s1, alnDb}, {})) return rc;
            if (!keep) {
                sddb::removeDb(tmp + "/aln_" + s1);
                sddb::removeDb(alnDb);
            }
        }
        if (!last) {
            const std::string profDb = tmp + "/profile_" + s;
            if (int rc = runModule(result2profileModule, "result2profile", {query, T, merged, profDb}, prof)) return rc;
            query = profDb;
        }
    }
    return 0;
}

// the module chain of R/data/clustersearch.sh:121-151 on the alignment DB <tmp>/result
int clusterChain(const Args &a, const std::string &Q, const std::string &T, const std::string &tmp) {
    const std::vector<std::string> common = {"--threads", std::to_string(threadsOf(a)), "-v", a.str("-v", "3")};
    if (int rc = runModule(prefixidModule, "prefixid", {tmp + "/result", tmp + "/result_prefixed"}, common)) return rc;
    if (int rc = runModule(besthitbysetModule, "besthitbyset", {Q, T, tmp + "/result_prefixed", tmp + "/aggregate"},
                           with(common, {"--simple-best-hit", "1", "--suboptimal-hits", "0"})))
        return rc;
    if (int rc = runModule(mergeresultsbysetModule, "mergeresultsbyset", {Q + "_set_to_member", tmp + "/aggregate", tmp + "/aggregate_merged"}, common))
        return rc;
    if (int rc = runModule(combinehitsModule, "combinehits", {Q, T, tmp + "/aggregate_merged", tmp + "/matches", tmp},
                           with(common, {"--alpha", a.str("--alpha", "1"), "--aggregation-mode", "0", "--filter-self-match",
                                         a.flag("--filter-self-match", false) ? "1" : "0"})))
        return rc;
    std::vector<std::string> ch = with(common, {"--multihit-pval", a.str("--multihit-pval", "0.01"), "--cluster-pval", a.str("--cluster-pval", "0.01"),
                                                "--max-gene-gap", a.str("--max-gene-gap", "3"), "--cluster-size", a.str("--cluster-size", "2"),
                                                "--db-output", "1", "--alpha", a.str("--alpha", "1")});
    if (a.has("--device")) ch = with(ch, {"--device", a.str("--device", "0")});
    if (int rc = runModule(clusterhitsModule, "clusterhits", {Q, T, tmp + "/matches", tmp + "/clusters"}, ch)) return rc;
    return runModule(summarizeresultsModule, "summarizeresults", {Q, T, tmp + "/clusters", a.pos[2]}, common);
}

// `search --alignment-mode 4` (M/src/workflow/Search.cpp:261-319,386-388; M/data/workflow/blastp.sh): the prefilter -- the k-mer one, or
// the ungapped one under --prefilter-mode 1 -- followed by `rescorediagonal --rescore-mode 2` with the rescorediagonal parameter set
// (Parameters.cpp:506-523) instead of `align`.  The modules run in this process, the target resident between them.
int checkUngappedAlign(const Args &a) {
    if (a.integer("--num-iterations", 1) > 1)
        return fail("--alignment-mode 4 with --num-iterations > 1: cannot use the ungapped alignment mode with profile databases");
    if (envInt("WORLD_SIZE", 1) > 1 || a.integer("--world-size", 1) > 1) return fail("--alignment-mode 4 runs on one rank");
    return 0;
}

int ungappedAlignSearch(const Args &a, const std::string &Q, const std::string &T, const std::string &result, const std::string &tmp) {
    if (int rc = checkUngappedAlign(a)) return rc;
    if (int rc = refuseProfileTarget(T)) return rc;
    mkdir(tmp.c_str(), 0777);
    const std::vector<std::string> common = {"--threads", std::to_string(threadsOf(a)), "-v", a.str("-v", "3")};
    const bool ungapped = a.integer("--prefilter-mode", 0) == 1;
    std::vector<std::string> pref = with(common, {"--max-seqs", a.str("--max-seqs", "300"), "-c", a.str("-c", "0"), "--cov-mode", a.str("--cov-mode", "0"),
                                                  "--min-ungapped-score", a.str("--min-ungapped-score", "15"), "--comp-bias-corr",
                                                  a.str("--comp-bias-corr", "1")});
    if (!ungapped)
        pref = with(pref, {"-s", a.str("-s", "5.7"), "-k", a.str("-k", "0"), "--mask", a.str("--mask", "1"), "--mask-prob", a.str("--mask-prob", "0.9")});
    // what each prefilter kind takes beyond that (ungappedprefilter has no index, bins or --add-self-matches)
    const std::vector<const char *> kmerOnly = {"--device", "--bin-size", "--l2-cache-size", "--chunk-queries", "--add-self-matches", "--target-search-mode"};
    const std::vector<const char *> ungappedOnly = {"--device", "--chunk-queries"};
    for (const char *f : ungapped ? ungappedOnly : kmerOnly)
        if (a.has(f)) pref = with(pref, {f, a.str(f, "")});
    if (!ungapped) pref = withSplit(a, pref);
    std::vector<std::string> rescore = with(common, {"--rescore-mode", "2", "-e", a.str("-e", "0.001"), "-c", a.str("-c", "0"), "--cov-mode",
                                                     a.str("--cov-mode", "0"), "-a", a.str("-a", "0"),
                                                     "--min-aln-len", a.str("--min-aln-len", "0"), "--seq-id-mode", a.str("--seq-id-mode", "0"),
                                                     "--sort-results", a.str("--sort-results", "0")});
    for (const char *f : {"--device", "--add-self-matches", "--filter-hits", "--wrapped-scoring"})
        if (a.has(f)) rescore = with(rescore, {f, a.str(f, "")});
    ResidentScope residentScope;
    const std::string prefDb = tmp + "/pref_0";
    if (ungapped) {
        if (int rc = runModule(ungappedprefilterModule, "ungappedprefilter", {Q, T, prefDb}, pref)) return rc;
    } else {
        if (int rc = runModule(prefilterModule, "prefilter", {Q, T, prefDb}, pref)) return rc;
    }
    return runModule(rescorediagonalModule, "rescorediagonal", {Q, T, prefDb, result}, rescore);
}

// `search --alt-ali N` (M/src/workflow/Search.cpp hands --alt-ali to the align step of blastp.sh): the prefilter -- the k-mer one,
// or the ungapped one under --prefilter-mode 1 -- followed by the `align` module with the alternative alignments, in this process
// with the target resident between them.  The streaming pipeline hands one record per pair from stage to stage and is not used.
int checkAltAli(const Args &a, bool withClusters) {
    if (withClusters)
        return fail("clustersearch --alt-ali: the fused best-hit aggregation is defined on one alignment per (query, target) pair; run "
                    "`search --alt-ali` or the `align` module");
    if (a.integer("--alignment-mode", 0) == 4) return fail("--alt-ali with --alignment-mode 4: the ungapped alignment mode has no alternative alignments");
    if (a.integer("--num-iterations", 1) > 1) return fail("--alt-ali with --num-iterations > 1 is not implemented; run the iterations with the modules");
    if (envInt("WORLD_SIZE", 1) > 1 || a.integer("--world-size", 1) > 1) return fail("--alt-ali runs on one rank");
    return 0;
}

int altAliSearch(const Args &a, const std::string &Q, const std::string &T, const std::string &result, const std::string &tmp) {
    if (int rc = refuseProfileTarget(T)) return rc;
    mkdir(tmp.c_str(), 0777);
    const std::vector<std::string> common = {"--threads", std::to_string(threadsOf(a)), "-v", a.str("-v", "3")};
    const bool ungapped = a.integer("--prefilter-mode", 0) == 1;
    std::vector<std::string> pref = with(common, {"--max-seqs", a.str("--max-seqs", "300"), "-c", a.str("-c", "0"), "--cov-mode", a.str("--cov-mode", "0"),
                                                  "--min-ungapped-score", a.str("--min-ungapped-score", "15"), "--comp-bias-corr",
                                                  a.str("--comp-bias-corr", "1")});
    if (!ungapped)
        pref = with(pref, {"-s", a.str("-s", "5.7"), "-k", a.str("-k", "0"), "--mask", a.str("--mask", "1"), "--mask-prob", a.str("--mask-prob", "0.9")});
    const std::vector<const char *> kmerOnly = {"--device", "--bin-size", "--l2-cache-size", "--chunk-queries", "--add-self-matches", "--target-search-mode"};
    const std::vector<const char *> ungappedOnly = {"--device", "--chunk-queries"};
    for (const char *f : ungapped ? ungappedOnly : kmerOnly)
        if (a.has(f)) pref = with(pref, {f, a.str(f, "")});
    if (!ungapped) pref = withSplit(a, pref);
    // the search workflow's alignment mode is 2 (score and coverage, Search.cpp:23)
    std::vector<std::string> aln = with(common, {"--alt-ali", a.str("--alt-ali", "0"), "--alignment-mode", a.str("--alignment-mode", "2"), "-e",
                                                 a.str("-e", "0.001"), "-c", a.str("-c", "0"), "--cov-mode", a.str("--cov-mode", "0"), "-a", a.str("-a", "0"),
                                                 "--min-aln-len", a.str("--min-aln-len", "0"), "--seq-id-mode", a.str("--seq-id-mode", "0"),
                                                 "--comp-bias-corr", a.str("--comp-bias-corr", "1")});
    for (const char *f : {"--device", "--add-self-matches"})
        if (a.has(f)) aln = with(aln, {f, a.str(f, "")});
    ResidentScope residentScope;
    const std::string prefDb = tmp + "/pref_0";
    if (ungapped) {
        if (int rc = runModule(ungappedprefilterModule, "ungappedprefilter", {Q, T, prefDb}, pref)) return rc;
    } else {
        if (int rc = runModule(prefilterModule, "prefilter", {Q, T, prefDb}, pref)) return rc;
    }
    return runModule(alignModule, "align", {Q, T, prefDb, result}, aln);
}

// `search <sequenceDB> <profileDB>` (M/src/workflow/Search.cpp:453-475 builds the parameter strings, M/data/workflow/searchtargetprofile.sh
// runs them): the prefilter against the profile DB's similar-k-mer index, its result swapped so that every profile lists the sequences
// that hit it, `align` with the profile as the Smith-Waterman query -- every listed sequence (--max-seqs INT_MAX), the coverage mode
// swapped with the sides -- and that result swapped back, which recomputes the E-values for the search the user asked for.  The
// intermediate DBs carry the script's names under <tmp>.
bool isProfileDb(const std::string &db) { return sddb::baseType(sddb::readDbType(db)) == sddb::DBTYPE_HMM_PROFILE; }

int swapCoverageMode(int covMode) {   // Util::swapCoverageMode (M/src/commons/Util.cpp:513-530)
    switch (covMode) {
        case 1: return 2;
        case 2: return 1;
        case 3: return 4;
        case 4: return 3;
        default: return covMode;
    }
}

int targetProfileSearch(const Args &a, const std::string &Q, const std::string &T, const std::string &result, const std::string &tmp) {
    // an entry of the swapped alignment DB is ordered by Matcher::compareHits, which ends at the key: two alignments of one pair
    // (one key twice in an entry) have no order there
    if (a.integer("--alt-ali", 0) != 0) return fail("--alt-ali with a profile target database: swapresults has no order for the alignments of one pair; run without --alt-ali");
    mkdir(tmp.c_str(), 0777);
    const std::vector<std::string> common = {"--threads", std::to_string(threadsOf(a)), "-v", a.str("-v", "3")};
    std::vector<std::string> pref = with(common, {"-s", a.str("-s", "5.7"), "-k", a.str("-k", "0"), "--max-seqs", a.str("--max-seqs", "300"), "-c",
                                                  a.str("-c", "0"), "--cov-mode", a.str("--cov-mode", "0"), "--min-ungapped-score",
                                                  a.str("--min-ungapped-score", "15"), "--comp-bias-corr", a.str("--comp-bias-corr", "1")});
    for (const char *f : {"--k-score", "--device", "--bin-size", "--l2-cache-size", "--chunk-queries", "--split", "--split-mode", "--split-memory-limit"})
        if (a.has(f)) pref = with(pref, {f, a.str(f, "")});
    std::vector<std::string> aln = with(common, {"-a", "1", "--alignment-mode", a.str("--alignment-mode", "2"), "-e", a.str("-e", "0.001"), "--max-seqs",
                                                 std::to_string(INT_MAX), "-c", a.str("-c", "0"), "--cov-mode",
                                                 std::to_string(swapCoverageMode((int) a.integer("--cov-mode", 0))), "--min-aln-len",
                                                 a.str("--min-aln-len", "0"), "--min-seq-id", a.str("--min-seq-id", "0"), "--seq-id-mode",
                                                 a.str("--seq-id-mode", "0"), "--comp-bias-corr", a.str("--comp-bias-corr", "1")});
    if (a.has("--device")) aln = with(aln, {"--device", a.str("--device", "0")});
    const std::vector<std::string> swap = with(common, {"-e", a.str("-e", "0.001")});
    // Two targets are resident in turn: the profile DB with its index for `prefilter`, the sequence DB with its sequence set for
    // `align` (Resident keys both by DB path, so they are entries of their own).  The index has no reader after the prefilter and is
    // freed before `align` uploads.
    ResidentScope residentScope;
    const std::string prefDb = tmp + "/pref", prefSwapped = tmp + "/pref_swapped", alnSwapped = tmp + "/aln_swapped";
    const bool keep = a.integer("--keep-tmp", 0) != 0;
    struct RemoveTmp {
        bool on;
        std::vector<std::string> dbs;
        ~RemoveTmp() { if (on) for (const std::string &d : dbs) sddb::removeDb(d); }
    } removeTmp{!keep, {prefDb, prefSwapped, alnSwapped}};
    if (int rc = runModule(prefilterModule, "prefilter", {Q, T, prefDb}, pref)) return rc;
    residentTargetOf(T, deviceOf(a), true);
    if (int rc = runModule(swapresultsModule, "swapresults", {Q, T, prefDb, prefSwapped}, swap)) return rc;
    if (int rc = runModule(alignModule, "align", {T, Q, prefSwapped, alnSwapped}, aln)) return rc;
    return runModule(swapresultsModule, "swapresults", {T, Q, alnSwapped, result}, swap);
}

// `clustersearch --profile-cluster-search 1` (R/src/workflow/clustersearch.cpp:60-75, R/data/clustersearch.sh:69-80): the queries are
// searched against the profiles of the target's cluster representatives (<T>_clu_rep_profile), every hit on a representative is carried
// over to the members of its cluster by `expandaln` along <T>_clu_aln, and the module chain runs on the expanded alignment DB.  The
// reference's default --exhaustive-search 1 sends its `search` down searchslicedtargetprofile.sh, which is not built: this path is
// searchtargetprofile.sh (targetProfileSearch above) and wants --exhaustive-search 0 said.
int profileClusterSearch(const Args &a) {
    if (a.pos.size() != 4) return fail("usage: clustersearch <querySetDB> <targetSetDB> <out.tsv> <tmpDir> [options]");
    if (int rc = checkWorkflowFlags(a)) return rc;
    if (a.integer("--num-iterations", 1) > 1) return fail("Profile-profile cluster searches are currently not supported. Please use only 1 iteration.");
    if (!a.has("--exhaustive-search") || a.has("--exhaustive-search#toggled") || a.str("--exhaustive-search", "1") != "0")
        return fail("--profile-cluster-search 1 runs with --exhaustive-search 1 by default, which searches through searchslicedtargetprofile "
                    "(not implemented); pass --exhaustive-search 0 for the searchtargetprofile chain");
    if (envInt("WORLD_SIZE", 1) > 1 || a.integer("--world-size", 1) > 1) return fail("--profile-cluster-search 1 runs on one rank");
    if (a.integer("--prefilter-mode", 0) != 0) return fail("--profile-cluster-search 1 with --prefilter-mode " + a.str("--prefilter-mode", "0") + " is not implemented");
    if (a.integer("--alignment-mode", 2) == 4) return fail("--profile-cluster-search 1 with --alignment-mode 4: cannot use the ungapped alignment mode with profile databases");
    const std::string Q = a.pos[0], T = a.pos[1], tmp = a.pos[3];
    const std::string repProfile = T + "_clu_rep_profile", cluAln = T + "_clu_aln";
    if (sddb::readDbType(repProfile) < 0 || !sddb::fileExists(repProfile + ".index"))
        return fail("--profile-cluster-search 1 needs " + repProfile + " (clusterdb writes it)");
    if (sddb::readDbType(cluAln) < 0 || !sddb::fileExists(cluAln + ".index")) return fail("--profile-cluster-search 1 needs " + cluAln + " (clusterdb writes it)");
    if (!isProfileDb(repProfile)) return fail(repProfile + " is not a profile database");
    mkdir(tmp.c_str(), 0777);
    Args s = a;   // the workflow's defaults for this mode (R/src/workflow/clustersearch.cpp:9-37,60-66)
    auto def = [&](const char *f, const char *v) { if (!s.has(f)) s.opt[f] = v; };
    def("-s", "5.7");
    def("--cov-mode", "2");
    def("-c", "0.8");
    def("-e", "0.001");
    def("--max-seqs", "100");
    def("--min-aln-len", "30");
    def("--alignment-mode", "2");
    def("-a", "1");
    for (const char *db : {"/result_clu", "/result", "/result_prefixed", "/aggregate", "/aggregate_merged", "/matches", "/matches_h", "/clusters", "/clusters_h"})
        sddb::removeDb(tmp + db);
    const std::string resultClu = tmp + "/result_clu";
    struct RemoveTmp {
        bool on;
        std::string db;
        ~RemoveTmp() { if (on) sddb::removeDb(db); }
    } removeTmp{a.integer("--keep-tmp", 0) == 0, resultClu};
    if (int rc = targetProfileSearch(s, Q, repProfile, resultClu, tmp + "/search")) return rc;
    // clustersearch.sh:77-79 passes the threads parameter only: expandaln runs at its own defaults
    std::vector<std::string> ex = {"--threads", std::to_string(threadsOf(a)), "-v", a.str("-v", "3")};
    if (a.has("--device")) ex = with(ex, {"--device", a.str("--device", "0")});
    if (int rc = runModule(expandalnModule, "expandaln", {Q, repProfile, resultClu, cluAln, tmp + "/result"}, ex)) return rc;
    return clusterChain(a, Q, T, tmp);
}

// --target-search-mode 1 (the similar-k-mer index of a sequence target, `prefilter --target-search-mode 1`): the workflows run the module
// chain with it, as for a target split -- the streaming pipeline builds the regular index.  What the chain does not cover is refused
// by name.  similar: the flag is 1 (a profile target makes it moot: the caller looks at the DB).
int checkTargetSearchMode(const Args &a, bool &similar) {
    const long long tsm = a.integer("--target-search-mode", 0);
    similar = false;
    if (tsm == 0) return 0;
    if (tsm != 1) return fail("--target-search-mode " + std::to_string(tsm) + ": 0 (regular k-mer index) or 1 (similar k-mer index)");
    if (a.flag("--profile-cluster-search", false))
        return fail("--target-search-mode 1 with --profile-cluster-search 1: a profile target is a similar-k-mer index already; run without the flag");
    if (a.integer("--num-iterations", 1) > 1)
        return fail("--target-search-mode 1 with --num-iterations > 1 is not implemented (profile queries against the similar-k-mer index)");
    if (a.integer("--prefilter-mode", 0) == 1) return fail("--target-search-mode 1 with --prefilter-mode 1: the ungapped prefilter has no k-mer index");
    if (envInt("WORLD_SIZE", 1) > 1 || a.integer("--world-size", 1) > 1) return fail("--target-search-mode 1 runs on one rank");
    similar = true;
    return 0;
}

}  // namespace

int searchModule(const Args &a0) {
    if (a0.flag("--profile-cluster-search", false)) return fail("--profile-cluster-search is a flag of clustersearch");
    bool similarTarget = false;
    if (int rc = checkTargetSearchMode(a0, similarTarget)) return rc;
    if (similarTarget && a0.pos.size() == 4 && isProfileDb(a0.pos[1])) similarTarget = false;   // isProfile || targetSearchMode (IndexBuilder.cpp:62)
    if (int rc = checkPrefilterMode(a0)) return rc;
    // a profile target DB on the one path that takes it: sequence queries, the k-mer prefilter, one pass, one rank, gapped alignments.
    // Every other combination goes on to its own path below and is refused there
    if (a0.pos.size() == 4 && isProfileDb(a0.pos[1]) && !isProfileDb(a0.pos[0]) && a0.integer("--prefilter-mode", 0) == 0 && a0.integer("--num-iterations", 1) <= 1 &&
        a0.integer("--alignment-mode", 0) != 4 && envInt("WORLD_SIZE", 1) <= 1 && a0.integer("--world-size", 1) <= 1) {
        if (int rc = checkWorkflowFlags(a0)) return rc;
        return targetProfileSearch(a0, a0.pos[0], a0.pos[1], a0.pos[2], a0.pos[3]);
    }
    Args a = a0;
    bool targetSplit = false;
    if (int rc = workflowSplit(a0, a, targetSplit)) return rc;
    if (a.integer("--alt-ali", 0) != 0) {
        if (a.pos.size() != 4) return fail("usage: search <queryDB> <targetDB> <alignmentDB> <tmpDir> [options]");
        if (int rc = checkAltAli(a, false)) return rc;
        if (int rc = checkWorkflowFlags(a)) return rc;
        return altAliSearch(a, a.pos[0], a.pos[1], a.pos[2], a.pos[3]);
    }
    if (a.integer("--alignment-mode", 0) == 4) {
        if (a.pos.size() != 4) return fail("usage: search <queryDB> <targetDB> <alignmentDB> <tmpDir> [options]");
        if (int rc = checkWorkflowFlags(a)) return rc;
        return ungappedAlignSearch(a, a.pos[0], a.pos[1], a.pos[2], a.pos[3]);
    }
    if (a.integer("--num-iterations", 1) > 1) {
        if (a.pos.size() != 4) return fail("usage: search <queryDB> <targetDB> <alignmentDB> <tmpDir> [options]");
        if (int rc = checkWorkflowFlags(a)) return rc;
        return iterativeSearch(a, a.pos[0], a.pos[1], a.pos[2], a.pos[3]);
    }
    if (targetSplit || similarTarget) {
        // one pass over a split target, or over the similar-k-mer index: `prefilter --split N` / `prefilter --target-search-mode 1` then
        // `align`, the chain altAliSearch runs (with --alt-ali 0)
        if (a.pos.size() != 4) return fail("usage: search <queryDB> <targetDB> <alignmentDB> <tmpDir> [options]");
        if (int rc = checkWorkflowFlags(a)) return rc;
        return altAliSearch(a, a.pos[0], a.pos[1], a.pos[2], a.pos[3]);
    }
    return runSearch(a, false);
}

int clustersearchModule(const Args &a0) {
    bool similarTarget = false;
    if (int rc = checkTargetSearchMode(a0, similarTarget)) return rc;
    if (a0.flag("--profile-cluster-search", false)) return profileClusterSearch(a0);
    if (int rc = checkPrefilterMode(a0)) return rc;
    if (a0.integer("--alt-ali", 0) != 0) return checkAltAli(a0, true);
    Args a = a0;
    bool targetSplit = false;
    if (int rc = workflowSplit(a0, a, targetSplit)) return rc;
    if (a.integer("--alignment-mode", 2) == 4) {
        // the ungapped alignment mode through the modules, then the module chain on its alignment DB
        if (a.pos.size() != 4) return fail("usage: clustersearch <querySetDB> <targetSetDB> <out.tsv> <tmpDir> [options]");
        if (int rc = checkWorkflowFlags(a)) return rc;
        if (int rc = checkUngappedAlign(a)) return rc;   // before anything under <tmpDir> is touched
        const std::string Q = a.pos[0], T = a.pos[1], tmp = a.pos[3];
        mkdir(tmp.c_str(), 0777);
        Args s = a;   // the clustersearch workflow's defaults (R/src/workflow/clustersearch.cpp:9-37)
        auto def = [&](const char *f, const char *v) { if (!s.has(f)) s.opt[f] = v; };
        def("-s", "5.7");
        def("--cov-mode", "2");
        def("-c", "0.8");
        def("-e", "10");
        def("--min-aln-len", "30");
        def("-a", "1");
        for (const char *db : {"/result", "/result_prefixed", "/aggregate", "/aggregate_merged", "/matches", "/matches_h", "/clusters", "/clusters_h"})
            sddb::removeDb(tmp + db);
        if (int rc = ungappedAlignSearch(s, Q, T, tmp + "/result", tmp + "/search")) return rc;
        return clusterChain(a, Q, T, tmp);
    }
    if (a.integer("--num-iterations", 1) <= 1 && (targetSplit || similarTarget)) {
        // one pass over a split target, or over the similar-k-mer index, through the modules (prefilter --split N / --target-search-mode 1,
        // align), then the module chain on its alignment DB
        if (a.pos.size() != 4) return fail("usage: clustersearch <querySetDB> <targetSetDB> <out.tsv> <tmpDir> [options]");
        if (int rc = checkWorkflowFlags(a)) return rc;
        const std::string Q = a.pos[0], T = a.pos[1], tmp = a.pos[3];
        mkdir(tmp.c_str(), 0777);
        Args s = a;   // the clustersearch workflow's defaults (R/src/workflow/clustersearch.cpp:9-37)
        auto def = [&](const char *f, const char *v) { if (!s.has(f)) s.opt[f] = v; };
        def("-s", "5.7");
        def("--cov-mode", "2");
        def("-c", "0.8");
        def("-e", "10");
        def("--min-aln-len", "30");
        def("--alignment-mode", "2");
        def("-a", "1");
        for (const char *db : {"/result", "/result_prefixed", "/aggregate", "/aggregate_merged", "/matches", "/matches_h", "/clusters", "/clusters_h"})
            sddb::removeDb(tmp + db);
        if (int rc = altAliSearch(s, Q, T, tmp + "/result", tmp + "/search")) return rc;
        return clusterChain(a, Q, T, tmp);
    }
    if (a.integer("--num-iterations", 1) <= 1) return runSearch(a, true);
    // iterative profile search (BASELINE config 4): the iterations through the modules, then the module chain of
    // R/data/clustersearch.sh:121-151 on the merged alignment DB
    if (a.pos.size() != 4) return fail("usage: clustersearch <querySetDB> <targetSetDB> <out.tsv> <tmpDir> [options]");
    if (int rc = checkWorkflowFlags(a)) return rc;
    const std::string Q = a.pos[0], T = a.pos[1], tmp = a.pos[3];
    mkdir(tmp.c_str(), 0777);
    Args s = a;   // the search step runs with the clustersearch workflow's defaults (R/src/workflow/clustersearch.cpp:9-37)
    auto def = [&](const char *f, const char *v) { if (!s.has(f)) s.opt[f] = v; };
    def("-s", "5.7");
    def("--cov-mode", "2");
    def("-c", "0.8");
    def("-e", "10");
    def("--min-aln-len", "30");
    def("--alignment-mode", "2");
    for (const char *db : {"/result", "/result_prefixed", "/aggregate", "/aggregate_merged", "/matches", "/matches_h", "/clusters", "/clusters_h"})
        sddb::removeDb(tmp + db);
    // default: in memory (no DB between the modules of an iteration, no text chain behind them).  The module chain runs when its DBs
    // are wanted (--keep-tmp 1), with SD_ITER_FILES=1, and for several ranks (they shard whole query sets over the module chain's DBs)
    const bool files = a.integer("--keep-tmp", 0) != 0 || (getenv("SD_ITER_FILES") && atoi(getenv("SD_ITER_FILES")) != 0) ||
                       envInt("WORLD_SIZE", 1) > 1 || a.integer("--world-size", 1) > 1 || targetSplit;
    if (!files) return iterativeSearch(s, Q, T, tmp + "/result", tmp + "/search", &a.pos[2]);
    if (int rc = iterativeSearch(s, Q, T, tmp + "/result", tmp + "/search")) return rc;
    return clusterChain(a, Q, T, tmp);
}

// cluster <sequenceDB> <clusterDB> <tmpDir> --single-step-clustering 1  (M/src/workflow/Cluster.cpp:14-20,63-104,244-262 set the
// parameters, M/data/workflow/clustering.sh is the chain): clusthash, clust, createsubdb --subdb-mode 1, prefilter of the sub DB against
// itself, align (rescorediagonal --rescore-mode 2 under --alignment-mode 4), clust, mergeclusters, in this process; the DBs between them
// lie under <tmpDir> with the reference's names.  DESIGN.md 4.18
int clusterModule(const Args &a) {
    if (a.pos.size() != 3) return fail("usage: cluster <sequenceDB> <clusterDB> <tmpDir> --single-step-clustering 1 [options]");
    if (int rc = checkCommon(a)) return rc;
    if (!a.flag("--single-step-clustering", false))
        return fail("only --single-step-clustering 1 is implemented: the cascaded workflow starts with linclust, whose ungapped filter "
                    "(rescorediagonal --filter-hits 1) needs the reference's --filter-hits threshold table");
    if (a.flag("--cluster-reassign", false)) return fail("--cluster-reassign is not part of the single-step chain");
    if (envInt("WORLD_SIZE", 1) > 1 || a.integer("--world-size", 1) > 1) return fail("cluster runs on one rank");
    const std::string in = a.pos[0], out = a.pos[1], tmp = a.pos[2];
    {
        const int bt = sddb::baseType(sddb::readDbType(in));
        if (sddb::readDbType(in) == -1) return fail(in + ".dbtype not found");
        if (bt == sddb::DBTYPE_NUCLEOTIDES) return fail("nucleotide DBs are not implemented (" + in + ")");
        if (bt == sddb::DBTYPE_HMM_PROFILE) return fail("profile DBs are not implemented (" + in + ")");
    }
    if (sddb::fileExists(out + ".dbtype")) return fail(out + ".dbtype exists already");
    mkdir(tmp.c_str(), 0777);
    // setWorkflowDefaults and setClusterAutomagicParameters
    const float seqId = (float) a.real("--min-seq-id", 0.0);
    const bool ungapped = a.integer("--alignment-mode", 3) == 4;
    const int covMode = (int) a.integer("--cov-mode", 0);
    const std::string clusterMode = a.str("--cluster-mode", (covMode == 1 || covMode == 2) ? "2" : "0");
    const std::string compBias = a.str("--comp-bias-corr", seqId >= 0.7f ? "0" : "1");
    const std::string minUngapped = a.str("--min-ungapped-score", seqId >= 0.7f ? "60" : "15");
    std::string sens = a.str("-s", "");
    if (sens.empty()) {
        const float s = seqId <= 0.3 ? 6.0f : seqId > 0.8 ? 1.0f : (float) (1.0 + (1.0 * (0.7 - seqId) * 10));   // setAutomaticThreshold
        char buf[32];
        snprintf(buf, sizeof(buf), "%g", s);
        sens = buf;
        info(a, "Set cluster sensitivity to -s %s\n", buf);
    }
    std::vector<std::string> common = {"--threads", std::to_string(threadsOf(a)), "-v", a.str("-v", "3")};
    const std::vector<std::string> hostOnly = common;
    if (a.has("--device")) common = with(common, {"--device", a.str("--device", "")});
    auto passed = [&](std::vector<std::string> v, std::initializer_list<const char *> flags) {
        for (const char *f : flags)
            if (a.has(f)) v = with(v, {f, a.str(f, "")});
        return v;
    };
    const std::vector<std::string> hashPar = with(common, {"--alph-size", "3", "--min-seq-id", "0.99"});   // whatever the user gave
    const std::vector<std::string> clustPar = passed(with(hostOnly, {"--cluster-mode", clusterMode}), {"--max-iterations", "--similarity-type"});
    const std::vector<std::string> pref =
        passed(with(common, {"-s", sens, "--max-seqs", a.str("--max-seqs", "20"), "-c", a.str("-c", "0.8"), "--cov-mode", std::to_string(covMode),
                             "--min-ungapped-score", minUngapped, "--comp-bias-corr", compBias}),
               {"-k", "--mask", "--mask-prob", "--spaced-kmer-mode", "--bin-size", "--chunk-queries", "--add-self-matches"});
    const std::vector<std::string> hits = {"-e", a.str("-e", "0.001"), "-c", a.str("-c", "0.8"), "--cov-mode", std::to_string(covMode), "--min-seq-id",
                                           a.str("--min-seq-id", "0")};
    std::vector<std::string> aln = common;
    aln.insert(aln.end(), hits.begin(), hits.end());
    aln = ungapped ? with(aln, {"--rescore-mode", "2"}) : with(aln, {"--alignment-mode", a.str("--alignment-mode", "3"), "--comp-bias-corr", compBias});
    aln = passed(aln, {"-a", "--min-aln-len", "--seq-id-mode", "--add-self-matches"});
    ResidentScope residentScope;
    const std::string alnRed = tmp + "/aln_redundancy", cluRed = tmp + "/clu_redundancy", sub = tmp + "/input_step_redundancy",
                      prefDb = tmp + "/pref", alnDb = tmp + "/aln", clu0 = tmp + "/clu_step0";
    for (const std::string &db : {alnRed, cluRed, sub, prefDb, alnDb, clu0}) sddb::removeDb(db);
    if (int rc = runModule(clusthashModule, "clusthash", {in, alnRed}, hashPar)) return rc;
    if (int rc = runModule(clustModule, "clust", {in, alnRed, cluRed}, clustPar)) return rc;
    if (int rc = runModule(createsubdbModule, "createsubdb", {cluRed, in, sub}, {"-v", a.str("-v", "3"), "--subdb-mode", "1"})) return rc;
    if (int rc = runModule(prefilterModule, "prefilter", {sub, sub, prefDb}, pref)) return rc;
    if (ungapped) {
        if (int rc = runModule(rescorediagonalModule, "rescorediagonal", {sub, sub, prefDb, alnDb}, aln)) return rc;
    } else {
        if (int rc = runModule(alignModule, "align", {sub, sub, prefDb, alnDb}, aln)) return rc;
    }
    if (int rc = runModule(clustModule, "clust", {sub, alnDb, clu0}, clustPar)) return rc;
    if (int rc = runModule(mergeclustersModule, "mergeclusters", {in, out, cluRed, clu0}, hostOnly)) return rc;
    if (a.flag("--remove-tmp-files", false)) {
        for (const std::string &db : {prefDb, alnDb, clu0, cluRed, alnRed}) sddb::removeDb(db);
        for (const char *suffix : {"", ".index", ".dbtype", "_h", "_h.index", "_h.dbtype", ".lookup", ".source"}) unlink((sub + suffix).c_str());
    }
    return 0;
}

// clusterdb <setDB> <tmpDir>  (R/src/workflow/clusterdb.cpp:9-85 sets the parameters, the non-foldseek branch of R/data/clusterdb.sh:97-143
// is the chain): cluster, createsubdb, result2profile on the cluster DB (its one-column rows realigned by sd_r2p_realign), profile2consensus,
// align -a on the cluster DB, in this process under one resident scope.  It leaves <T>_clu_rep_profile, <T>_clu and <T>_clu_aln, what
// `clustersearch --profile-cluster-search 1` reads.  DESIGN.md 4.19
int clusterdbModule(const Args &a) {
    if (a.pos.size() != 2) return fail("usage: makeclusterdb <setDB> <tmpDir> --single-step-clustering 1 [options]");
    if (int rc = checkCommon(a)) return rc;
    if (a.integer("--search-mode", 0) != 0)
        return fail("--search-mode " + a.str("--search-mode", "") + " clusters structures with foldseek, which is not part of this build");
    const std::string T = a.pos[0], tmp = a.pos[1];
    {
        const int dbtype = sddb::readDbType(T);
        if (dbtype == -1) return fail(T + ".dbtype not found");
        if (sddb::baseType(dbtype) == sddb::DBTYPE_NUCLEOTIDES) return fail("nucleotide DBs are not implemented (" + T + ")");
        if (sddb::baseType(dbtype) == sddb::DBTYPE_HMM_PROFILE) return fail("profile DBs are not implemented (" + T + ")");
    }
    if (!a.flag("--single-step-clustering", false))
        return fail("only --single-step-clustering 1 is implemented: the cascaded workflow starts with linclust, whose ungapped filter "
                    "(rescorediagonal --filter-hits 1) needs the reference's --filter-hits threshold table");
    if (envInt("WORLD_SIZE", 1) > 1 || a.integer("--world-size", 1) > 1) return fail("makeclusterdb runs on one rank");
    mkdir(tmp.c_str(), 0777);
    // CLUSTER_PAR: the cluster workflow's flags as the user gave them over setclusterDbDefaults; THREADS_PAR for result2profile and align
    // (the user's -e, -c, ... do not reach them); CONSENSUS_PAR; VERBOSITY
    std::vector<std::string> cluPar;
    {
        Args c = a;
        for (const char *f : {"--search-mode", "--foldseek-path"}) c.opt.erase(f);
        auto def = [&](const char *f, const char *v) { if (!c.has(f)) c.opt[f] = v; };
        def("--min-seq-id", "0.7");
        def("-c", "0.8");
        def("--cov-mode", "0");
        c.opt["--threads"] = std::to_string(threadsOf(a));
        c.opt["-v"] = a.str("-v", "3");
        cluPar = c.flagsAsArgv();
    }
    const std::vector<std::string> verbosity = {"-v", a.str("-v", "3")};
    std::vector<std::string> threadsPar = {"--threads", std::to_string(threadsOf(a)), "-v", a.str("-v", "3")};
    std::vector<std::string> consPar = threadsPar;
    if (a.has("--device")) threadsPar = with(threadsPar, {"--device", a.str("--device", "")});
    for (const char *f : {"--sub-mat", "--max-seq-len"})
        if (a.has(f)) consPar = with(consPar, {f, a.str(f, "")});
    const std::string clu = tmp + "/cluster_mmseqs", dbClu = tmp + "/db_clu", prof = T + "_clu_rep_profile", cons = T + "_clu", aln = T + "_clu_aln";
    struct Step {
        int (*fn)(const Args &);
        const char *name;
        std::string out;
        std::vector<std::string> pos, flags;
        bool skip = false;
    };
    std::vector<std::string> alnPar = {"-a", "1"};
    alnPar.insert(alnPar.end(), threadsPar.begin(), threadsPar.end());
    std::vector<Step> steps = {
        {clusterModule, "cluster", clu, {T, clu, tmp + "/cluster"}, cluPar},
        {createsubdbModule, "createsubdb", dbClu, {clu, T, dbClu}, verbosity},
        {result2profileModule, "result2profile", prof, {dbClu, T, clu, prof}, threadsPar},
        {profile2consensusModule, "profile2consensus", cons, {prof, cons}, consPar},
        {alignModule, "align", aln, {T, T, clu, aln}, alnPar},
    };
    // a step whose output exists is not run again (notExists "<out>.dbtype" in the script); the plan is printed before the first step
    for (Step &s : steps) {
        s.skip = sddb::fileExists(s.out + ".dbtype");
        std::string line = s.name;
        for (const std::string &x : s.pos) line += " " + x;
        for (const std::string &x : s.flags) line += " " + x;
        info(a, "makeclusterdb %s: %s\n", s.skip ? "skips" : "runs", line.c_str());
    }
    ResidentScope residentScope;
    for (const Step &s : steps) {
        if (s.skip) continue;
        const double t0 = omp_get_wtime();
        if (int rc = runModule(s.fn, s.name, s.pos, s.flags)) return rc;
        info(a, "makeclusterdb: %s took %.2f s\n", s.name, omp_get_wtime() - t0);
    }
    // what became of the target sequence sets the steps asked for (the set result2profile uploads is the one `align` finds resident)
    for (const std::string &l : resident().seqSetLog) info(a, "makeclusterdb: sequence set %s\n", l.c_str());
    if (a.flag("--remove-tmp-files", false)) {
        // what the script removes: the cluster DB and the cluster workflow's directory (db_clu stays, as it does there)
        info(a, "Remove temporary files\n");
        sddb::removeDb(clu);
        const std::string dir = tmp + "/cluster";
        if (DIR *d = opendir(dir.c_str())) {
            while (struct dirent *e = readdir(d))
                if (strcmp(e->d_name, ".") != 0 && strcmp(e->d_name, "..") != 0) unlink((dir + "/" + e->d_name).c_str());
            closedir(d);
            rmdir(dir.c_str());
        }
    }
    return 0;
}

}  // namespace sdcli
