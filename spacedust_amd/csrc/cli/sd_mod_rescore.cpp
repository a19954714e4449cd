// rescorediagonal <queryDB> <targetDB> <prefilterDB> <resultDB> (M/src/alignment/rescorediagonal.cpp:45-434 with the parameters of
// Parameters.cpp:506-523): the best ungapped local alignment on every prefilter hit's own diagonal -- what blastp.sh calls instead of
// `align` under --alignment-mode 4.  The per-hit arithmetic runs on the device (sd_rescore_diagonal_batch); the row logic of
// doRescorediagonal (:194-363) is the host side here.
#include "sd_pref_core.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace sdcli {

namespace {

// SmithWaterman::computeCov (StripedSmithWaterman.cpp:1671-1673)
inline float rescoreCov(unsigned start, unsigned end, unsigned len) {
    return (std::min(len, std::max(start, end)) - std::min(start, end) + 1) / (float) len;
}
// Util::hasCoverage (Util.cpp:496-511)
inline bool rescoreHasCov(float thr, int mode, float qCov, float tCov) {
    switch (mode) {
        case 0: return qCov >= thr && tCov >= thr;
        case 1: return qCov >= thr;
        case 2: return tCov >= thr;
        default: return true;
    }
}
// Util::computeSeqId (Util.cpp:532-542)
inline float rescoreSeqId(int mode, int ids, int qLen, int tLen, int alnLen) {
    switch (mode) {
        case 1: return static_cast<float>(ids) / static_cast<float>(std::min(qLen, tLen));
        case 2: return static_cast<float>(ids) / static_cast<float>(std::max(qLen, tLen));
        case 0: return static_cast<float>(ids) / static_cast<float>(alnLen);
    }
    return 0.0f;
}

// the DB's bytes of every sequence, laid out like SeqDb::residues
void gatherLetters(const SeqDb &db, std::vector<char> &out) {
    out.resize(db.totalResidues() + 1);
#pragma omp parallel for schedule(static)
    for (uint32_t i = 0; i < db.n; i++) memcpy(out.data() + db.offsets[i], db.rd.data(i), (size_t) db.lens[i]);
}

}  // namespace

int rescorediagonalModule(const Args &a) {
    if (a.pos.size() != 4) return fail("usage: rescorediagonal <queryDB> <targetDB> <prefilterDB> <resultDB> [options]");
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    const std::string sm = a.multi("--sub-mat", "aa", "blosum62.out");
    if (sm != "blosum62.out") return fail("--sub-mat " + sm + ": only blosum62.out is built into this path");
    const int mode = (int) a.integer("--rescore-mode", 0);
    if (mode == 3) return fail("--rescore-mode 3 (global alignment) is not implemented");
    if (mode == 4) return fail("--rescore-mode 4 (window quality alignment) is not implemented");
    if (mode < 0 || mode > 4) return fail("--rescore-mode " + std::to_string(mode) + ": 0 (Hamming), 1 (substitution) and 2 (alignment) are implemented");
    if (a.flag("--filter-hits", false)) return fail("--filter-hits 1 is not implemented (its score-per-column thresholds are a table of the reference)");
    if (a.flag("--wrapped-scoring", false)) return fail("--wrapped-scoring 1 is a nucleotide mode and is not implemented");
    const double evalThr = a.real("-e", 0.001);
    const float covThr = (float) a.real("-c", 0.0), seqIdThr = (float) a.real("--min-seq-id", 0.0);
    const int covMode = (int) a.integer("--cov-mode", 0), alnLenThr = (int) a.integer("--min-aln-len", 0);
    const int seqIdMode = (int) a.integer("--seq-id-mode", 0);
    const bool addBacktrace = a.flag("-a", false), includeIdentity = a.flag("--add-self-matches", false);
    const bool sortResults = a.integer("--sort-results", 0) > 0;
    const int threads = threadsOf(a);

    Lap lap("rescorediagonal");
    HostH host;
    if (host.open(threads) != SD_OK) return fail("sd_host_create failed");
    std::string err;
    {   // (SeqDb::load names amino acid and profile DBs only; say what this module was given)
        const int qt = sddb::baseType(sddb::readDbType(a.pos[0])), tt = sddb::baseType(sddb::readDbType(a.pos[1]));
        if (qt == sddb::DBTYPE_NUCLEOTIDES || tt == sddb::DBTYPE_NUCLEOTIDES) return fail("nucleotide databases are not implemented in rescorediagonal");
        if (qt == sddb::DBTYPE_HMM_PROFILE || tt == sddb::DBTYPE_HMM_PROFILE) return fail("profile databases are not implemented in rescorediagonal");
    }
    DbPair db;
    if (!db.open(a.pos[0], a.pos[1], host.h, true, false, &err)) return fail(err);
    const bool sameDb = db.sameDb;
    const SeqDb *const qdb = db.qdb, *const tdb = db.tdb.get();
    sddb::Reader pref;
    if (!pref.open(a.pos[2], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    if (sddb::baseType(pref.dbtype()) == 14)   // Parameters::DBTYPE_PREFILTER_REV_RES
        return fail("reverse (bi-directional) prefilter results are a nucleotide mode and are not implemented");
    lap.mark("load DBs");
    info(a, "Rescore mode %d\nQuery database size: %u type: Aminoacid\nTarget database size: %u type: Aminoacid\n", mode, qdb->n, tdb->n);

    CtxH ctx;
    int rc = ctx.open(deviceOf(a));
    if (rc != SD_OK) return failNoDevice(rc);
    // both sides as sets that carry the DB's letters; the target set of a workflow is the resident one
    SeqSetH tset, qsetOwn;
    std::vector<char> letters;
    rc = residentSeqSet(ctx.c, a.pos[1], deviceOf(a), *tdb, tset);
    if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create(targets)");
    // a resident set that carries its letters already (an earlier rescorediagonal of the workflow) is taken as it is
    const std::string lettersKey = a.pos[1] + "|" + std::to_string(deviceOf(a)) + "|letters";
    if (tset.own || !resident().seqSets.count(lettersKey)) {
        gatherLetters(*tdb, letters);
        rc = sd_seqset_set_letters(tset.s, letters.data());
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_set_letters(targets)");
        if (!tset.own) resident().seqSets[lettersKey] = nullptr;   // a mark only: Resident::clear and the stale-DB sweep skip null entries
    }
    sd_seqset *qset = tset.s;
    if (!sameDb) {
        rc = sd_seqset_create(ctx.c, qdb->residues.data(), qdb->offsets.data(), qdb->n, nullptr, &qsetOwn.s);
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_create(queries)");
        gatherLetters(*qdb, letters);
        rc = sd_seqset_set_letters(qsetOwn.s, letters.data());
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_seqset_set_letters(queries)");
        qset = qsetOwn.s;
    }
    letters.clear();
    letters.shrink_to_fit();
    lap.mark("context + sequences on the device");

    sd_rescore_params par;
    memset(&par, 0, sizeof(par));
    sd_host_matrix(host.h, 0, par.matrix, nullptr, par.aa2num);
    par.mode = mode;
    sd_aln_criteria crit;
    memset(&crit, 0, sizeof(crit));
    crit.evalThr = evalThr;
    crit.seqIdMode = seqIdMode;
    crit.swMode = 2;
    crit.addBacktrace = addBacktrace ? 1 : 0;
    const uint64_t dbResidues = tdb->totalResidues();   // tdbr->getAminoAcidDBSize() (rescorediagonal.cpp:107)

    sddb::Writer out;
    // rescorediagonal.cpp:396-401: an alignment DB in mode 2, else the input's type
    if (!out.open(a.pos[3], mode == 2 ? (int) sddb::DBTYPE_ALIGNMENT_RES : pref.dbtype(), &err)) return fail(err);
    sd_alntext *text = nullptr;
    sd_alntext_create(&text);
    std::unique_ptr<sd_alntext, void (*)(sd_alntext *)> textGuard(text, sd_alntext_destroy);
    const std::string mPool(65536, 'M');   // the backtrace of an ungapped alignment: alnLen matches

    const size_t nEntries = pref.size();
    const uint64_t maxHits = 4000000;
    uint64_t rescored = 0, passed = 0;
    std::vector<uint32_t> hq, ht, entryQ, order, counts, recT;
    std::vector<uint16_t> hd;
    std::vector<uint64_t> hitOff;
    std::vector<sd_rescore_result> res;
    std::vector<sd_sw_result> rec;
    std::vector<int32_t> qlen;
    std::vector<std::string> shortText;
    struct Short {
        int score;
        uint32_t key;
        int diagonal;
    };
    for (size_t e0 = 0; e0 < nEntries;) {
        // a chunk of entries bounded by hits; the pairs that cannot be covered never reach the device (rescorediagonal.cpp:211-213)
        size_t e1 = e0;
        hq.clear();
        ht.clear();
        hd.clear();
        entryQ.clear();
        hitOff.assign(1, 0);
        while (e1 < nEntries && (hq.size() < maxHits || e1 == e0)) {
            const char *d = pref.data(e1);
            uint32_t qId = UINT32_MAX;
            if (*d != '\0') {
                const size_t id = qdb->rd.idOfKey(pref.key(e1));
                if (id == SIZE_MAX)
                    return fail("Query sequence " + std::to_string(pref.key(e1)) + " is required in the prefiltering, but is not contained in the query sequence database.");
                qId = (uint32_t) id;
            }
            while (*d != '\0') {
                char *end;
                const uint32_t tKey = (uint32_t) strtoul(d, &end, 10);
                (void) strtol(end, &end, 10);
                const long diag = strtol(end, &end, 10);
                while (*d != '\n' && *d != '\0') d++;
                if (*d == '\n') d++;
                const size_t tId = tdb->rd.idOfKey(tKey);
                if (tId == SIZE_MAX)
                    return fail("Sequence " + std::to_string(tKey) + " is required in the prefiltering, but is not contained in the target sequence database!");
                if (!sd_host_can_be_covered(covThr, covMode, (float) qdb->lens[qId], (float) tdb->lens[tId])) continue;
                hq.push_back(qId);
                ht.push_back((uint32_t) tId);
                hd.push_back((uint16_t) (short) diag);   // QueryMatcher::parsePrefilterHit: a short, kept as an unsigned short
            }
            entryQ.push_back(qId);
            hitOff.push_back(hq.size());
            e1++;
        }
        const uint32_t nHits = (uint32_t) hq.size(), nE = (uint32_t) (e1 - e0);
        res.resize(std::max<uint32_t>(nHits, 1));
        rc = sd_rescore_diagonal_batch(ctx.c, &par, qset, tset.s, nHits, hq.data(), ht.data(), hd.data(), res.data());
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_rescore_diagonal_batch");
        rescored += nHits;
        lap.mark("chunk: parse + device");
        // the row logic per entry (rescorediagonal.cpp:239-341), the accepted rows of an entry in input order or sorted
        rec.resize(std::max<uint32_t>(nHits, 1));
        recT = ht;
        order.assign(std::max<uint32_t>(nHits, 1), 0);
        counts.assign(std::max<uint32_t>(nE, 1), 0);
        qlen.assign(std::max<uint32_t>(nE, 1), 0);
        shortText.assign(nE, std::string());
#pragma omp parallel
        {
            std::vector<uint32_t> acc;
            std::vector<Short> shorts;
#pragma omp for schedule(dynamic, 64)
            for (uint32_t e = 0; e < nE; e++) {
                acc.clear();
                shorts.clear();
                const uint32_t qId = entryQ[e];
                const int qLen = qId == UINT32_MAX ? 0 : qdb->lens[qId];
                qlen[e] = qLen;
                for (uint64_t x = hitOff[e]; x < hitOff[e + 1]; x++) {
                    const sd_rescore_result &r = res[x];
                    const uint32_t tId = ht[x];
                    const int tLen = tdb->lens[tId];
                    const bool isIdentity = qId == tId && (includeIdentity || sameDb);
                    double seqId = 0, evalue = 0.0;
                    int bitScore = 0, alnLen = 0, idCnt = 0;
                    float targetCov = static_cast<float>(r.diagonalLen) / static_cast<float>(tLen);
                    float queryCov = static_cast<float>(r.diagonalLen) / static_cast<float>(qLen);
                    sd_sw_result &o = rec[x];
                    memset(&o, 0, sizeof(o));
                    if (mode == 0) {
                        seqId = rescoreSeqId(seqIdMode, r.score, qLen, tLen, r.diagonalLen);
                        alnLen = r.diagonalLen;
                    } else {
                        evalue = sd_host_evalue(dbResidues, (double) r.score, (double) qLen);
                        bitScore = static_cast<int>(sd_host_bitscore((double) r.score) + 0.5);
                        if (mode == 2) {
                            alnLen = (r.endPos - r.startPos) + 1;
                            int qS, qE, tS, tE;
                            if (r.diagonal >= 0) {
                                qS = r.startPos + r.distToDiagonal;
                                qE = r.endPos + r.distToDiagonal;
                                tS = r.startPos;
                                tE = r.endPos;
                            } else {
                                qS = r.startPos;
                                qE = r.endPos;
                                tS = r.startPos + r.distToDiagonal;
                                tE = r.endPos + r.distToDiagonal;
                            }
                            if (evalue <= evalThr || isIdentity) {   // the identity count is used only here (:284-292)
                                idCnt = r.idCnt;
                                seqId = rescoreSeqId(seqIdMode, idCnt, qLen, tLen, alnLen);
                            }
                            queryCov = rescoreCov((unsigned) qS, (unsigned) qE, (unsigned) qLen);
                            targetCov = rescoreCov((unsigned) tS, (unsigned) tE, (unsigned) tLen);
                            o.score = r.score;
                            o.qStart = qS;
                            o.qEnd = qE;
                            o.tStart = tS;
                            o.tEnd = tE;
                            o.identical = idCnt;
                            o.btLen = alnLen;
                            o.evalue = evalue;
                        }
                    }
                    const bool hasCov = rescoreHasCov(covThr, covMode, queryCov, targetCov);
                    const bool hasSeqId = seqId >= (seqIdThr - std::numeric_limits<float>::epsilon());
                    const bool hasEvalue = evalue <= evalThr;
                    const bool hasAlnLen = alnLen >= alnLenThr;
                    if (!(isIdentity || (hasAlnLen && hasCov && hasSeqId && hasEvalue))) continue;
                    if (mode == 2) acc.push_back((uint32_t) x);
                    else shorts.push_back({mode == 1 ? bitScore : (int) (100 * seqId), tdb->keys[tId], r.diagonal});
                }
                if (mode == 2) {
                    if (sortResults && acc.size() > 1)   // Matcher::compareHits (Matcher.h:157-168)
                        std::sort(acc.begin(), acc.end(), [&](uint32_t x, uint32_t y) {
                            const sd_sw_result &p = rec[x], &q = rec[y];
                            if (p.evalue != q.evalue) return p.evalue < q.evalue;
                            const int bp = static_cast<int>(sd_host_bitscore((double) p.score) + 0.5), bq = static_cast<int>(sd_host_bitscore((double) q.score) + 0.5);
                            if (bp != bq) return bp > bq;
                            if (tdb->lens[ht[x]] != tdb->lens[ht[y]]) return tdb->lens[ht[x]] < tdb->lens[ht[y]];
                            return tdb->keys[ht[x]] < tdb->keys[ht[y]];
                        });
                    counts[e] = (uint32_t) acc.size();
                    for (size_t i = 0; i < acc.size(); i++) order[hitOff[e] + i] = acc[i];   // compacted below
                } else {
                    if (sortResults && shorts.size() > 1)   // hit_t::compareHitsByScoreAndId (QueryMatcher.h:38-48)
                        std::sort(shorts.begin(), shorts.end(), [](const Short &p, const Short &q) {
                            if (abs(p.score) != abs(q.score)) return abs(p.score) > abs(q.score);
                            return p.key < q.key;
                        });
                    for (const Short &h : shorts) appendPrefRow(shortText[e], h.key, h.score, h.diagonal);
                    counts[e] = (uint32_t) shorts.size();
                }
            }
        }
        for (uint32_t e = 0; e < nE; e++) passed += counts[e];
        if (mode == 2) {
            uint64_t w = 0;
            for (uint32_t e = 0; e < nE; e++)
                for (uint32_t i = 0; i < counts[e]; i++) order[w++] = order[hitOff[e] + i];
            rc = sd_alntext_format(text, &crit, nE, counts.data(), order.data(), recT.data(), rec.data(), nullptr, mPool.data(), qlen.data(),
                                   tdb->lens.data(), tdb->keys.data());
            if (rc != SD_OK) return fail("sd_alntext_format failed (" + std::to_string(rc) + ")");
            const char *txt;
            const uint64_t *eoff;
            sd_alntext_get(text, &txt, &eoff);
            for (uint32_t e = 0; e < nE; e++)
                if (!out.write(pref.key(e0 + e), txt + eoff[e], (size_t) (eoff[e + 1] - eoff[e]))) return fail("cannot write " + a.pos[3]);
        } else {
            for (uint32_t e = 0; e < nE; e++)
                if (!out.write(pref.key(e0 + e), shortText[e].data(), shortText[e].size())) return fail("cannot write " + a.pos[3]);
        }
        lap.mark("chunk: rows + write");
        e0 = e1;
    }
    if (!out.close(&err)) return fail(err);
    info(a, "%llu hits rescored\n%llu sequence pairs passed the thresholds\n", (unsigned long long) rescored, (unsigned long long) passed);
    return 0;
}

}  // namespace sdcli
