#!/usr/bin/env python3
"""Writes tests/golden/clusterdb_vectors.npz from the LIVE reference: what `result2profile` makes of a cluster DB (rows without a
backtrace, which the module aligns itself), what `profile2consensus` makes of those profiles, and what `align -a` writes for the same
cluster DB -- the three DBs `clusterdb` (R/data/clusterdb.sh:97-126) leaves beside a set DB.  Inputs and recorded outputs only.

The modules cannot be linked as they stand (Parameters.cpp needs generated headers; DBReader / DBWriter are files), so DRIVER below includes
result2profile.cpp, profile2seq.cpp and Matcher.cpp where they lie, links oracle/_ref/libsdref.so (Sequence, SubstitutionMatrix,
SmithWaterman, Masker, Util, Debug) and the objects of oracle/_ref/libsdref_r2p.so (MultipleAlignment, MsaFilter, PSSMCalculator), and
runs result2profile() and profile2consensus() themselves.  Function by function:

  the reference's own object code
    result2profile()                 the whole function: the per-row decision "more than 10 columns: parse, else Matcher::getSWResult", the
                                     E-value cut, computeMSA, MsaFilter::filter, computePSSMFromMSA, the bias correction, maskPssm, toBuffer
    profile2consensus()              the whole function
    Matcher                          called by the driver once more per row, with the module's arguments and with two variations of them
                                     (score bias 0; no composition bias), to record qStart / tStart / backtrace per pair and to show that
                                     the two settings matter
    MultipleAlignment, MsaFilter     called by the driver per entry on those alignments: rows before and after the filter
  restated in the driver (no module function reachable: Alignment::run is bound to Parameters and files)
    the row loop of `align -a`       M/src/alignment/Alignment.cpp:339-510 for one-column rows: Matcher over the bias-0 matrix with composition
                                     bias, scoreIdentical for the row whose key is the entry's (both DBs are one), Alignment::checkCriteria's
                                     expression with the module's defaults (-e 0.001, no coverage / identity / length threshold), SORT_SERIAL
                                     with Matcher::compareHits, Matcher::resultToBuffer with the backtrace
  reader / writer plumbing defined in the driver (no algorithm)
    DBReader<unsigned int>           over tables in memory by DB name; ids in the order given (the linear order), getId by key
    DBWriter                         into a list key -> bytes per DB name, in write order (one thread)
    Parameters                       zeroed storage; parseParameters sets the members the functions read to the reference's defaults
    IndexReader, MMseqsMPI, FileUtil, BandedNucleotideAligner, ContextLibrary, CSProfile: what the untaken branches name; they abort when reached

    python tools/make_golden_clusterdb.py [reference root]      (needs `make -C oracle _ref/libsdref.so _ref/libsdref_r2p.so`; no GPU)

Set K: <T> = K_let / K_off / K_keys (the sequence DB), K_q_keys (the keys of db_clu: the representatives, one left out), and two runs:
K_r0 the cluster DB as `cluster` writes it (one column), K_r1 one entry that mixes 11-column rows and one-column rows.  Per run <R>:
<R>_clu_{keys,off,text} (the input rows), <R>_profile_*, <R>_consensus_* (the DBs written, in write order), <R>_pair_{q,t,qstart,tstart,
bt_off,bt} (every row's realignment as the module computes it; _b0 / _nb: with score bias 0 / without composition bias), <R>_msa
(key, rows, rows kept).  K_r0_aln_*: the rows of `align -a`.  K_class_names / K_class_key name the representative of each class.
main() asserts every class on the recorded output before the file is written.
"""
import gzip
import io
import os
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLD, 'clusterdb_vectors.npz')
AA = b'ACDEFGHIKLMNPQRSTVWY'

DRIVER = r'''
#include <algorithm>
#include <chrono>
#include <climits>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <queue>
#include <set>
#include <sstream>
#include <fstream>
#include <iostream>
#include <iomanip>
#include <memory>
#include <limits>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <atomic>
#include <stdexcept>
#include <utility>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>
#include <sys/stat.h>
#include <sys/mman.h>
#include <fcntl.h>
#include <omp.h>
#define private public
#define protected public
#include "DBReader.h"
#include "DBWriter.h"
#include "Parameters.h"
#undef private
#undef protected
#include "MMseqsMPI.h"
#include "FileUtil.h"
#include "Matcher.h"
#include "MultipleAlignment.h"
#include "MsaFilter.h"
#include "FastSort.h"
#include "CSProfile.h"

static void unreachable(const char *what) {
    fprintf(stderr, "driver: %s reached\n", what);
    abort();
}

// ---- DBs in memory ------------------------------------------------------------------------------------------------------------------
struct Table {
    int dbtype = 0;
    std::vector<unsigned int> keyOfId;
    std::vector<std::string> dataOfId;                       // payload without the terminating null byte
    std::vector<std::pair<unsigned int, size_t> > byKey;     // (key, id), ascending
};
static std::map<std::string, Table> g_tables;
static std::map<std::string, std::vector<std::pair<unsigned int, std::string> > > g_written;
static std::map<std::string, int> g_writtenType;
static int g_threads = 1;
static std::string g_matrix;

static Table *tableOf(const DBReader<unsigned int> *r) { return (Table *) r->dataFiles; }

template <> DBReader<unsigned int>::DBReader(const char *name, const char *, int threads_, int mode) {
    memset((void *) &threads, 0, (char *) &magicBytes - (char *) &threads);
    new (&dataFileNames) std::vector<std::string>();
    if (!g_tables.count(name)) unreachable((std::string("a reader of the unknown DB ") + name).c_str());
    Table *t = &g_tables[name];
    threads = threads_;
    dataMode = mode;
    indexFileName = (char *) "memory";
    dataFileName = (char *) "memory";
    dataFiles = (char **) t;
    size = t->keyOfId.size();
    dbtype = t->dbtype;
    index = (Index *) calloc(size + 1, sizeof(Index));
    for (size_t i = 0; i < size; i++) {
        index[i].id = t->keyOfId[i];
        index[i].length = t->dataOfId[i].size() + 1;
        maxSeqLen = std::max<unsigned int>(maxSeqLen, (unsigned int) index[i].length);
        dataSize += index[i].length;
    }
    closed = 0;
}
template <> DBReader<unsigned int>::~DBReader() { free(index); }
template <> bool DBReader<unsigned int>::open(int) { return true; }
template <> void DBReader<unsigned int>::close() {}
template <> void DBReader<unsigned int>::readMmapedDataInMemory() {}
template <> char *DBReader<unsigned int>::getData(size_t id, int) { return &tableOf(this)->dataOfId[id][0]; }
template <> unsigned int DBReader<unsigned int>::getDbKey(size_t id) { return tableOf(this)->keyOfId[id]; }
template <> size_t DBReader<unsigned int>::getSize() const { return size; }
template <> size_t DBReader<unsigned int>::getId(unsigned int key) {
    const std::vector<std::pair<unsigned int, size_t> > &v = tableOf(this)->byKey;
    std::vector<std::pair<unsigned int, size_t> >::const_iterator it = std::lower_bound(v.begin(), v.end(), std::make_pair(key, (size_t) 0));
    return (it != v.end() && it->first == key) ? it->second : UINT_MAX;
}
template <> size_t DBReader<unsigned int>::getAminoAcidDBSize() {
    if (Parameters::isEqualDbtype(dbtype, Parameters::DBTYPE_HMM_PROFILE)) return (dataSize - size) / Sequence::PROFILE_READIN_SIZE;
    return dataSize - 2 * size;
}
template <> size_t DBReader<unsigned int>::maxCount(char c) {
    size_t best = 0;
    for (size_t i = 0; i < size; i++) {
        const std::string &d = tableOf(this)->dataOfId[i];
        best = std::max<size_t>(best, (size_t) std::count(d.begin(), d.end(), c));
    }
    return best;
}
template <> void DBReader<unsigned int>::softlinkDb(const std::string &, const std::string &, DBFiles::Files) {}

DBWriter::DBWriter(const char *name, const char *, unsigned int threads_, size_t mode_, int dbtype_) : threads(threads_), mode(mode_), dbtype(dbtype_) {
    dataFileName = strdup(name);
    g_written[name].clear();
    g_writtenType[name] = dbtype_;
}
DBWriter::~DBWriter() { free(dataFileName); }
void DBWriter::open(size_t) {}
void DBWriter::close(bool, bool) {}
void DBWriter::writeData(const char *data, size_t dataSize, unsigned int key, unsigned int, bool, bool) {
#pragma omp critical
    g_written[dataFileName].push_back(std::make_pair(key, std::string(data, dataSize)));
}

static void registerWritten(const std::string &name) {
    Table &t = g_tables[name];
    t = Table();
    t.dbtype = g_writtenType[name];
    const std::vector<std::pair<unsigned int, std::string> > &w = g_written[name];
    for (size_t i = 0; i < w.size(); i++) {
        t.keyOfId.push_back(w[i].first);
        t.dataOfId.push_back(w[i].second);
        t.byKey.push_back(std::make_pair(w[i].first, i));
    }
    std::sort(t.byKey.begin(), t.byKey.end());
}

// ---- what the functions name beside the DBs --------------------------------------------------------------------------------------------
Parameters *Parameters::instance = NULL;
void initParameterSingleton(void) { unreachable("initParameterSingleton"); }
void Parameters::parseParameters(int, const char **, const Command &, bool, int, int) {
    threads = g_threads;
    compressed = 0;
    maxSeqLen = 65535;
    preloadMode = Parameters::PRELOAD_MODE_MMAP;
    evalThr = 0.001;
    evalProfile = evalThr;
    maskProfile = 1;
    filterMaxSeqId = 0.9;
    qsc = -20.0f;
    covMSAThr = 0.0;
    Ndiff = 1000;
    filterMinEnable = 0;
    wg = false;
    pcmode = Parameters::PCMODE_SUBSTITUTION_SCORE;
    profileOutputMode = 0;
    compBiasCorrection = 1;
    compBiasCorrectionScale = 1.0;
    maskProb = 0.9;
    zdrop = 40;
    includeIdentity = false;
}
void Parameters::printParameters(const std::string &, int, const char **, const std::vector<MMseqsParameter *> &) {}
bool MMseqsMPI::active = false;
int MMseqsMPI::rank = 0;
int MMseqsMPI::numProc = 1;
void MMseqsMPI::init(int, const char **) {}
int FileUtil::parseDbType(const char *name) { return g_tables.count(name) ? g_tables[name].dbtype : -1; }
void FileUtil::remove(const char *) {}
// the context-specific pseudo counts (--pseudo-cnt-mode 1) need a library blob that is not part of the tree; mode 0 never reaches them
ContextLibrary *ContextLibrary::contextLibrary = NULL;
ContextLibrary::ContextLibrary() { unreachable("ContextLibrary"); }
float *CSProfile::computeProfileCs(int, float *, float *, float, float) {
    unreachable("CSProfile::computeProfileCs");
    return NULL;
}
BandedNucleotideAligner::BandedNucleotideAligner(BaseMatrix *, size_t, int, int, int) : fastMatrix(NULL, NULL, 0) { unreachable("BandedNucleotideAligner"); }
BandedNucleotideAligner::~BandedNucleotideAligner() {}
void BandedNucleotideAligner::initQuery(Sequence *) { unreachable("BandedNucleotideAligner::initQuery"); }
s_align BandedNucleotideAligner::align(Sequence *, int, bool, std::string &, EvalueComputation *, bool) {
    unreachable("BandedNucleotideAligner::align");
    return s_align();
}
// result2profile.cpp reads a target index through this class when the target DB is one; it is not
#define MMSEQS_INDEXREADER_H
class IndexReader {
public:
    static const int SEQUENCES = 1, SRC_SEQUENCES = 2, PRELOAD_INDEX = 1, PRELOAD_DATA = 2;
    IndexReader(const std::string &, int, int, int) : sequenceReader(NULL) { unreachable("IndexReader"); }
    DBReader<unsigned int> *sequenceReader;
};

#include "Matcher.cpp"
#include "result2profile.cpp"
#include "profile2seq.cpp"

// ---- job / result files ----------------------------------------------------------------------------------------------------------------
static bool readAll(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static std::string readString(FILE *f) {
    uint32_t n = 0;
    if (!readAll(f, &n, 4)) exit(2);
    std::string s(n, '\0');
    if (!readAll(f, &s[0], n)) exit(2);
    return s;
}
static void put32(FILE *f, uint32_t v) { fwrite(&v, 4, 1, f); }
static void puti(FILE *f, int32_t v) { fwrite(&v, 4, 1, f); }
static void put64(FILE *f, uint64_t v) { fwrite(&v, 8, 1, f); }
static void putDb(FILE *f, const std::vector<std::pair<unsigned int, std::string> > &db) {
    put32(f, (uint32_t) db.size());
    for (size_t i = 0; i < db.size(); i++) {
        put32(f, db[i].first);
        put64(f, db[i].second.size());
        fwrite(db[i].second.data(), 1, db[i].second.size(), f);
    }
}
static void putResult(FILE *f, const Matcher::result_t &r) {
    puti(f, r.score);
    puti(f, r.qStartPos);
    puti(f, r.qEndPos);
    puti(f, r.dbStartPos);
    puti(f, r.dbEndPos);
    put32(f, (uint32_t) r.backtrace.size());
    fwrite(r.backtrace.data(), 1, r.backtrace.size(), f);
}

// job: i32 threads; u32 nDbs; per DB: name, i32 dbtype, u32 n, per entry u32 key + string; then the names of <Q> <T> <R>
int main(int argc, char **argv) {
    if (argc != 4) return 1;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 1;
    g_matrix = argv[3];
    int32_t threads = 1;
    uint32_t nDbs = 0;
    if (!readAll(in, &threads, 4) || !readAll(in, &nDbs, 4)) return 2;
    g_threads = threads;
    omp_set_num_threads(threads);
    for (uint32_t d = 0; d < nDbs; d++) {
        const std::string name = readString(in);
        Table &t = g_tables[name];
        int32_t type = 0;
        uint32_t n = 0;
        if (!readAll(in, &type, 4) || !readAll(in, &n, 4)) return 2;
        t.dbtype = type;
        for (uint32_t i = 0; i < n; i++) {
            uint32_t key = 0;
            if (!readAll(in, &key, 4)) return 2;
            t.keyOfId.push_back(key);
            t.dataOfId.push_back(readString(in));
            t.byKey.push_back(std::make_pair(key, (size_t) i));
        }
        std::sort(t.byKey.begin(), t.byKey.end());
    }
    const std::string Q = readString(in), T = readString(in), R = readString(in);
    fclose(in);

    Parameters *par = (Parameters *) calloc(1, sizeof(Parameters));
    new (&par->db1) std::string(Q);
    new (&par->db1Index) std::string(Q + ".index");
    new (&par->db2) std::string(T);
    new (&par->db2Index) std::string(T + ".index");
    new (&par->db3) std::string(R);
    new (&par->db3Index) std::string(R + ".index");
    new (&par->db4) std::string("P");
    new (&par->db4Index) std::string("P.index");
    new (&par->qid) std::string("0.0");
    new (&par->scoringMatrixFile) MultiParam<NuclAA<std::string>>(NuclAA<std::string>(g_matrix, "nucleotide.out"));
    new (&par->gapOpen) MultiParam<NuclAA<int>>(NuclAA<int>(11, 5));
    new (&par->gapExtend) MultiParam<NuclAA<int>>(NuclAA<int>(1, 2));
    new (&par->pca) MultiParam<PseudoCounts>(PseudoCounts(1.1, 1.4));
    new (&par->pcb) MultiParam<PseudoCounts>(PseudoCounts(4.1, 5.8));
    Parameters::instance = par;
    Debug::setDebugLevel(1);
    Command *command = (Command *) calloc(1, sizeof(Command));
    std::vector<MMseqsParameter *> noParams;
    command->params = &noParams;
    command->cmd = "driver";

    if (result2profile(0, NULL, *command) != EXIT_SUCCESS) return 3;
    registerWritten("P");
    par->db1 = "P";
    par->db1Index = "P.index";
    par->db2 = "C";
    par->db2Index = "C.index";
    if (profile2consensus(0, NULL, *command) != EXIT_SUCCESS) return 3;

    FILE *out = fopen(argv[2], "wb");
    if (!out) return 1;
    putDb(out, g_written["P"]);
    putDb(out, g_written["C"]);

    // every row's realignment as the module computes it, and with one argument changed at a time
    const Table &q = g_tables[Q], &t = g_tables[T], &r = g_tables[R];
    unsigned int maxLen = 2;
    size_t aaSize = 0;
    for (size_t i = 0; i < t.dataOfId.size(); i++) {
        maxLen = std::max<unsigned int>(maxLen, (unsigned int) t.dataOfId[i].size() + 2);
        aaSize += t.dataOfId[i].size() - 1;
    }
    for (size_t i = 0; i < q.dataOfId.size(); i++) maxLen = std::max<unsigned int>(maxLen, (unsigned int) q.dataOfId[i].size() + 2);
    SubstitutionMatrix biased(g_matrix.c_str(), 2.0f, -0.2f), plain(g_matrix.c_str(), 2.0f, 0.0f);
    EvalueComputation evBiased(aaSize, &biased, 11, 1), evPlain(aaSize, &plain, 11, 1);
    const int AAT = Parameters::DBTYPE_AMINO_ACIDS;
    struct Variant {
        SubstitutionMatrix *m;
        EvalueComputation *ev;
        bool bias;
    } variants[3] = {{&biased, &evBiased, true}, {&plain, &evPlain, true}, {&biased, &evBiased, false}};
    size_t maxRows = r.dataOfId.empty() ? 1 : 1;
    for (size_t i = 0; i < r.dataOfId.size(); i++) maxRows = std::max<size_t>(maxRows, (size_t) std::count(r.dataOfId[i].begin(), r.dataOfId[i].end(), '\n') + 1);
    std::vector<std::pair<unsigned int, unsigned int> > pairKeys;
    std::vector<std::vector<Matcher::result_t> > pairRes(3);
    std::vector<unsigned int> msaKey, msaRows, msaKept;
    for (int v = 0; v < 3; v++) {
        Matcher matcher(AAT, AAT, maxLen, variants[v].m, variants[v].ev, variants[v].bias, 1.0f, 11, 1, 0.0, 40);
        Sequence centre(maxLen, AAT, variants[v].m, 0, false, variants[v].bias);
        Sequence edge(maxLen, AAT, variants[v].m, 0, false, false);
        MultipleAlignment aligner(maxLen, variants[v].m);
        MsaFilter filter(maxLen, maxRows, variants[v].m, 11, 1);
        std::vector<int> qidVec(1, 0);
        for (size_t e = 0; e < r.keyOfId.size(); e++) {
            const unsigned int qKey = r.keyOfId[e];
            std::vector<std::pair<unsigned int, size_t> >::const_iterator qi = std::lower_bound(q.byKey.begin(), q.byKey.end(), std::make_pair(qKey, (size_t) 0));
            if (qi == q.byKey.end() || qi->first != qKey) continue;
            const std::string &qd = q.dataOfId[qi->second];
            centre.mapSequence(qi->second, qKey, qd.c_str(), qd.size() - 1);
            matcher.initQuery(&centre);
            std::vector<Matcher::result_t> results;
            std::vector<std::vector<unsigned char> > seqSet;
            const char *data = r.dataOfId[e].c_str();
            while (*data != '\0') {
                const unsigned int tKey = (unsigned int) strtoul(data, NULL, 10);
                std::vector<std::pair<unsigned int, size_t> >::const_iterator ti = std::lower_bound(t.byKey.begin(), t.byKey.end(), std::make_pair(tKey, (size_t) 0));
                if (ti == t.byKey.end() || ti->first != tKey) unreachable("a row whose key the target DB lacks");
                const std::string &td = t.dataOfId[ti->second];
                edge.mapSequence(ti->second, tKey, td.c_str(), td.size() - 1);
                seqSet.emplace_back(std::vector<unsigned char>(edge.numSequence, edge.numSequence + edge.L));
                results.push_back(matcher.getSWResult(&edge, INT_MAX, false, 0, 0.0, FLT_MAX, Matcher::SCORE_COV_SEQID, 0, false));
                if (v == 0) pairKeys.push_back(std::make_pair(qKey, tKey));
                data = Util::skipLine((char *) data);
            }
            pairRes[v].insert(pairRes[v].end(), results.begin(), results.end());
            if (v == 0) {
                MultipleAlignment::MSAResult res = aligner.computeMSA(&centre, seqSet, results, true);
                const size_t kept = filter.filter(res, results, 0, qidVec, -20.0f, 90, 1000, 0);
                msaKey.push_back(qKey);
                msaRows.push_back((unsigned int) res.setSize);
                msaKept.push_back((unsigned int) kept);
                MultipleAlignment::deleteMSA(&res);
            }
        }
    }
    put64(out, pairKeys.size());
    for (size_t p = 0; p < pairKeys.size(); p++) {
        put32(out, pairKeys[p].first);
        put32(out, pairKeys[p].second);
        for (int v = 0; v < 3; v++) putResult(out, pairRes[v][p]);
    }
    put32(out, (uint32_t) msaKey.size());
    for (size_t i = 0; i < msaKey.size(); i++) {
        put32(out, msaKey[i]);
        put32(out, msaRows[i]);
        put32(out, msaKept[i]);
    }

    // align <T> <T> <R> -a: Alignment::run's row loop (see the header of the generator)
    std::vector<std::pair<unsigned int, std::string> > alnDb;
    {
        Matcher matcher(AAT, AAT, maxLen, &plain, &evPlain, true, 1.0f, 11, 1, 0.0, 40);
        Sequence qSeq(maxLen, AAT, &plain, 0, false, true);
        Sequence dbSeq(maxLen, AAT, &plain, 0, false, true);
        char buffer[1024 + 32768 * 4];
        for (size_t e = 0; e < r.keyOfId.size(); e++) {
            const unsigned int qKey = r.keyOfId[e];
            std::vector<std::pair<unsigned int, size_t> >::const_iterator qi = std::lower_bound(t.byKey.begin(), t.byKey.end(), std::make_pair(qKey, (size_t) 0));
            if (qi == t.byKey.end() || qi->first != qKey) unreachable("a cluster whose representative the sequence DB lacks");
            const std::string &qd = t.dataOfId[qi->second];
            qSeq.mapSequence(qi->second, qKey, qd.c_str(), qd.size() - 1);
            matcher.initQuery(&qSeq);
            std::vector<Matcher::result_t> accepted;
            const char *data = r.dataOfId[e].c_str();
            while (*data != '\0') {
                const unsigned int tKey = (unsigned int) strtoul(data, NULL, 10);
                std::vector<std::pair<unsigned int, size_t> >::const_iterator ti = std::lower_bound(t.byKey.begin(), t.byKey.end(), std::make_pair(tKey, (size_t) 0));
                const std::string &td = t.dataOfId[ti->second];
                dbSeq.mapSequence(ti->second, tKey, td.c_str(), td.size() - 1);
                const bool isIdentity = qKey == tKey;   // the same DB twice
                Matcher::result_t res = matcher.getSWResult(&dbSeq, INT_MAX, false, 0, 0.0f, 0.001, Matcher::SCORE_COV_SEQID, 0, isIdentity);
                const bool ok = res.eval <= 0.001 && res.seqId >= 0.0 && Util::hasCoverage(0.0f, 0, res.qcov, res.dbcov) &&
                                Util::hasAlignmentLength(0, res.alnLength);
                if (isIdentity || ok) accepted.push_back(res);
                data = Util::skipLine((char *) data);
            }
            if (accepted.size() > 1) SORT_SERIAL(accepted.begin(), accepted.end(), Matcher::compareHits);
            std::string text;
            for (size_t i = 0; i < accepted.size(); i++) text.append(buffer, Matcher::resultToBuffer(buffer, accepted[i], true));
            alnDb.push_back(std::make_pair(qKey, text));
        }
    }
    putDb(out, alnDb);
    fclose(out);
    return 0;
}
'''


def build_driver(ref_root, tmp):
    m = os.path.join(ref_root, 'lib', 'mmseqs')
    src, exe = os.path.join(tmp, 'driver.cpp'), os.path.join(tmp, 'driver')
    open(src, 'w').write(DRIVER)
    inc = [os.path.join(m, *p) for p in (('src', 'commons'), ('src', 'alignment'), ('src', 'prefiltering'), ('src', 'clustering'), ('src', 'linclust'),
                                          ('src', 'util'), ('lib',), ('lib', 'simd'), ('lib', 'alp'), ('lib', 'tantan'), ('lib', 'fmt'), ('lib', 'simde'),
                                          ('lib', 'zstd', 'lib'), ('lib', 'xxhash'), ('lib', 'omptl'), ('lib', 'ips4o'), ('lib', 'kerasify'))]
    inc = [d for d in inc if os.path.isdir(d)]
    refdir = os.path.join(ROOT, 'oracle', '_ref')
    r2p_objs = [os.path.join(refdir, 'obj', 'r2p_%s.o' % n) for n in ('PSSMCalculator', 'MsaFilter', 'MultipleAlignment')]
    subprocess.check_call(['g++', '-std=c++14', '-O3', '-mavx2', '-mfma', '-mcx16', '-DAVX2=1', '-DOPENMP=1', '-fopenmp', '-w', '-fvisibility=hidden',
                           '-ffunction-sections', '-fdata-sections'] + ['-I' + d for d in inc] +
                          [src] + r2p_objs + ['-L' + refdir, '-lsdref', '-Wl,-rpath,' + refdir, '-Wl,--gc-sections', '-Wl,--allow-shlib-undefined',
                                              '-o', exe])
    return exe


def _string(b):
    return struct.pack('<I', len(b)) + b


def run_driver(exe, tmp, matrix, t_db, q_keys, clu, threads=1):
    """t_db: list of (key, letters bytes) in id order; q_keys: the keys of db_clu; clu: list of (key, text).  -> dict"""
    by = dict(t_db)
    dbs = [(b'T', 0, [(k, s + b'\n') for k, s in t_db]), (b'Q', 0, [(k, by[k] + b'\n') for k in q_keys]), (b'R', 6, clu)]
    job, res = os.path.join(tmp, 'job.bin'), os.path.join(tmp, 'res.bin')
    with open(job, 'wb') as f:
        f.write(struct.pack('<iI', threads, len(dbs)))
        for name, dbtype, entries in dbs:
            f.write(_string(name) + struct.pack('<iI', dbtype, len(entries)))
            for k, payload in entries:
                f.write(struct.pack('<I', k) + _string(payload))
        f.write(_string(b'Q') + _string(b'T') + _string(b'R'))
    subprocess.run([exe, job, res, matrix], check=True)
    raw = open(res, 'rb').read()
    at = [0]

    def take(fmt):
        v = struct.unpack_from(fmt, raw, at[0])
        at[0] += struct.calcsize(fmt)
        return v if len(v) > 1 else v[0]

    def take_db():
        db = []
        for _ in range(take('<I')):
            k, ln = take('<IQ')
            db.append((k, raw[at[0]:at[0] + ln]))
            at[0] += ln
        return db

    out = dict(profile=take_db(), consensus=take_db(), pairs=[])
    for _ in range(take('<Q')):
        qk, tk = take('<II')
        variants = []
        for _v in range(3):
            score, qs, qe, ts, te, n = take('<iiiiiI')
            variants.append(dict(score=score, qstart=qs, qend=qe, tstart=ts, tend=te, bt=raw[at[0]:at[0] + n]))
            at[0] += n
        out['pairs'].append((qk, tk, variants))
    out['msa'] = [take('<III') for _ in range(take('<I'))]
    out['aln'] = take_db()
    assert at[0] == len(raw)
    return out


def save(path, arrays):
    """an .npz with fixed time stamps: it regenerates byte for byte"""
    with zipfile.ZipFile(path, 'w') as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED, 9)


def pack_db(out, name, db):
    """db: list of (key, bytes) in its own order"""
    off = np.zeros(len(db) + 1, np.uint64)
    if db:
        off[1:] = np.cumsum([len(t) for _, t in db])
    out[name + '_keys'] = np.array([k for k, _ in db], np.uint32)
    out[name + '_off'] = off
    out[name + '_text'] = np.frombuffer(b''.join(t for _, t in db), np.uint8)


# ---- the set -------------------------------------------------------------------------------------------------------------------------
def example_proteins():
    seqs = []
    for f in ('NC_000913.faa', 'NC_000915.faa'):
        cur = None
        for line in gzip.open(os.path.join(GOLD, 'examples', f + '.gz'), 'rt'):
            if line.startswith('>'):
                if cur is not None:
                    seqs.append(cur)
                cur = ''
            else:
                cur += line.strip()
        seqs.append(cur)
    return [np.frombuffer(s.rstrip('*').encode(), np.uint8) for s in seqs]


def rnd(rng, n):
    return np.frombuffer(AA, np.uint8)[rng.integers(0, 20, n)].copy()


def mutate(rng, s, lo, hi):
    """the mutation scheme of tests/test_gpu_cluster_workflow.py: a share of the letters substituted"""
    s = s.copy()
    pos = rng.permutation(len(s))[:max(1, int(len(s) * rng.uniform(lo, hi)))]
    s[pos] = rnd(rng, len(pos))
    return s


def build_set():
    """-> (sequences [(key, bytes)] in id order, clusters [(class name, [member index ...])] with the representative first)"""
    rng = np.random.default_rng(67)
    roots = [s for s in example_proteins() if 120 <= len(s) <= 330 and set(s.tobytes()) <= set(AA)]
    roots = [roots[i] for i in range(0, len(roots), 41)]
    take = iter(roots)
    seqs, clusters = [], []

    def cluster(name, members):
        first = len(seqs)
        seqs.extend(members)
        clusters.append((name, list(range(first, len(seqs)))))

    cluster('singleton', [next(take)])
    a = next(take)
    cluster('exact_copy', [a, a.copy()])
    a = next(take)
    ins = mutate(rng, a, 0.02, 0.04)
    ins = np.concatenate([ins[:len(a) // 3], rnd(rng, 7), ins[len(a) // 3:]])
    dele = mutate(rng, a, 0.02, 0.04)
    dele = np.concatenate([dele[:len(a) // 2], dele[len(a) // 2 + 9:]])
    cluster('indels', [a, ins, dele])
    a = next(take)
    cluster('local', [a, np.concatenate([rnd(rng, 40), mutate(rng, a[70:len(a) - 60], 0.08, 0.12), rnd(rng, 55)])])
    for c in range(6):   # diverged members with ragged ends: where the score bias of the matrix moves an alignment's ends
        a = next(take)
        members = [a]
        for _ in range(3):
            lo, hi = int(rng.integers(0, 25)), int(rng.integers(0, 25))
            members.append(np.concatenate([rnd(rng, int(rng.integers(0, 20))), mutate(rng, a[lo:len(a) - hi], 0.3, 0.5), rnd(rng, int(rng.integers(0, 20)))]))
        cluster('far_%d' % c, members)
    for c, rich in enumerate((b'SSGSSSGSSSSGSS', b'KEKKEEKKEKEEKK', b'QQPQQQPQQPQQQQ')):   # a low-complexity stretch: the composition bias of the centre
        a = next(take)
        stretch = np.frombuffer(rich * 3, np.uint8)
        a = np.concatenate([a[:len(a) // 2], stretch, a[len(a) // 2:]])
        cluster('low_complexity_%d' % c, [a] + [mutate(rng, a, 0.3, 0.45) for _ in range(3)])
    a = next(take)
    cluster('diversity', [a] + [mutate(rng, a, 0.01, 0.25) for _ in range(30)])   # near copies at a range of distances: the filter keeps some
    a = next(take)
    cluster('mixed', [a] + [mutate(rng, a, 0.05, 0.25) for _ in range(4)])
    a = next(take)
    cluster('missing_query', [a, mutate(rng, a, 0.05, 0.1)])
    order = rng.permutation(len(seqs))
    key_of = {int(x): 5 + 3 * n for n, x in enumerate(order)}
    t_db = [(key_of[int(x)], seqs[int(x)].tobytes()) for x in order]
    return t_db, [(name, [key_of[m] for m in members]) for name, members in clusters]


def compress(bt):
    """Matcher::compressAlignment"""
    out, i = [], 0
    while i < len(bt):
        j = i
        while j < len(bt) and bt[j] == bt[i]:
            j += 1
        out.append(b'%d%c' % (j - i, bt[i]))
        i = j
    return b''.join(out)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    matrix = os.path.join(ref_root, 'lib', 'mmseqs', 'data', 'blosum62.out')
    t_db, clusters = build_set()
    assert len(t_db) <= 150 and all(60 <= len(s) <= 450 for _, s in t_db)
    rep = {name: members[0] for name, members in clusters}
    q_keys = sorted(members[0] for name, members in clusters if name != 'missing_query')
    clu0 = sorted((members[0], b''.join(b'%d\n' % m for m in members)) for _, members in clusters)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        r0 = run_driver(exe, tmp, matrix, t_db, q_keys, clu0)
        # the mixed entry: two members' rows as `align -a` wrote them (11 columns), the others as the cluster DB has them
        aln = dict(r0['aln'])
        rows = {int(l.split(b'\t')[0]): l for l in aln[rep['mixed']].splitlines(True)}
        members = dict(clusters)['mixed']
        assert all(m in rows and rows[m].count(b'\t') == 10 for m in members)
        mixed = b''.join(rows[m] if i in (1, 3) else b'%d\n' % m for i, m in enumerate(members))
        r1 = run_driver(exe, tmp, matrix, t_db, q_keys, [(rep['mixed'], mixed)])
    by_len = dict(t_db)

    # ---- the classes, on the reference's own output ----
    pairs = {(q, t): v for q, t, v in r0['pairs']}
    assert len(pairs) == len(r0['pairs']) == sum(len(m) for n, m in clusters if n != 'missing_query')
    assert all(len(v[0]['bt']) > 0 and v[0]['score'] > 0 for v in pairs.values()), 'a zero-score pair'
    profiles, consensus = dict(r0['profile']), dict(r0['consensus'])
    assert sorted(profiles) == q_keys == sorted(consensus) and rep['missing_query'] not in profiles              # missing query key: skipped
    assert all(len(profiles[k]) == 25 * len(by_len[k]) and len(consensus[k]) == len(by_len[k]) + 1 for k in q_keys)
    k = rep['singleton']
    assert dict(clu0)[k] == b'%d\n' % k and pairs[(k, k)][0]['bt'] == b'M' * len(by_len[k])
    from spacedust_amd.api import Host
    m2, _, a2n = Host().matrix(2)
    codes = a2n[np.frombuffer(by_len[k], np.uint8)]
    assert int(m2.reshape(21, 21)[codes, codes].astype(np.int64).sum()) > 255, 'the self alignment does not saturate the byte kernel'
    members = dict(clusters)['exact_copy']
    assert by_len[members[0]] == by_len[members[1]] and pairs[(members[0], members[1])][0]['bt'] == b'M' * len(by_len[members[0]])
    members = dict(clusters)['indels']
    bts = [pairs[(members[0], m)][0]['bt'] for m in members[1:]]
    assert any(b'I' * 5 in b for b in bts) and any(b'D' * 5 in b for b in bts), bts
    members = dict(clusters)['local']
    v = pairs[(members[0], members[1])][0]
    assert v['qstart'] > 0 and v['tstart'] > 0 and v['qend'] < len(by_len[members[0]]) - 1 and v['tend'] < len(by_len[members[1]]) - 1, v
    differs = lambda a, b: (a['qstart'], a['tstart'], a['bt']) != (b['qstart'], b['tstart'], b['bt'])
    bias_pairs = [p for p, v in pairs.items() if differs(v[0], v[1])]
    comp_pairs = [p for p, v in pairs.items() if differs(v[0], v[2])]
    assert bias_pairs, 'no pair differs between the -0.2 and the bias-0 matrix'
    assert comp_pairs, 'no pair differs with and without the composition bias'
    msa = {k: (rows_, kept) for k, rows_, kept in r0['msa']}
    assert msa[rep['diversity']][0] == 32 and 2 < msa[rep['diversity']][1] < 32, msa[rep['diversity']]   # (the centre, its own row, 30 copies)
    assert len(r1['profile']) == 1 and r1['profile'][0][0] == rep['mixed']
    n_cols = [l.count(b'\t') + 1 for l in mixed.splitlines()]
    assert sorted(set(n_cols)) == [1, 11]
    print('set K: %d sequences, %d clusters, %d pairs; %d pairs differ by the score bias, %d by the composition bias; the filter keeps %d of %d '
          'rows of the diversity cluster' % (len(t_db), len(clusters), len(pairs), len(bias_pairs), len(comp_pairs), msa[rep['diversity']][1],
                                             msa[rep['diversity']][0]))

    # ---- the file ----
    off = np.zeros(len(t_db) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for _, s in t_db])
    out['K_let'] = np.frombuffer(b''.join(s for _, s in t_db), np.uint8)
    out['K_off'] = off
    out['K_keys'] = np.array([k for k, _ in t_db], np.uint32)
    out['K_q_keys'] = np.array(q_keys, np.uint32)
    out['K_class_names'] = np.array([n for n, _ in clusters], dtype='U40')
    out['K_class_key'] = np.array([m[0] for _, m in clusters], np.uint32)
    out['K_bias_pairs'] = np.array(sorted(bias_pairs), np.uint32).reshape(-1, 2)
    out['K_comp_bias_pairs'] = np.array(sorted(comp_pairs), np.uint32).reshape(-1, 2)
    for tag, clu, run in (('K_r0', clu0, r0), ('K_r1', [(rep['mixed'], mixed)], r1)):
        pack_db(out, tag + '_clu', clu)
        pack_db(out, tag + '_profile', run['profile'])
        pack_db(out, tag + '_consensus', run['consensus'])
        out[tag + '_pair_q'] = np.array([q for q, _, _ in run['pairs']], np.uint32)
        out[tag + '_pair_t'] = np.array([t for _, t, _ in run['pairs']], np.uint32)
        for v, suffix in enumerate(('', '_b0', '_nb')):
            out[tag + '_pair_qstart' + suffix] = np.array([p[2][v]['qstart'] for p in run['pairs']], np.int32)
            out[tag + '_pair_tstart' + suffix] = np.array([p[2][v]['tstart'] for p in run['pairs']], np.int32)
            bt_off = np.zeros(len(run['pairs']) + 1, np.uint64)
            bt_off[1:] = np.cumsum([len(p[2][v]['bt']) for p in run['pairs']])
            out[tag + '_pair_bt_off' + suffix] = bt_off
            out[tag + '_pair_bt' + suffix] = np.frombuffer(b''.join(p[2][v]['bt'] for p in run['pairs']), np.uint8)
        out[tag + '_msa'] = np.array(run['msa'], np.uint32).reshape(-1, 3)
    pack_db(out, 'K_r0_aln', r0['aln'])
    save(OUT, out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 1000000


if __name__ == '__main__':
    main()
