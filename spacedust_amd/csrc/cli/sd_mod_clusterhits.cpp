// clusterhits <querySetDB> <targetSetDB> <matches> <out>   (R/src/util/ClusterHits.cpp:215-511): DB in, sd_clusterhits_batch in the
// middle, DB out.  No compute here, no CPU fallback.
#include "sd_cli.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace sdcli {

int clusterhitsModule(const Args &a) {
    if (a.pos.size() != 4) return fail("usage: clusterhits <querySetDB> <targetSetDB> <matchesDB> <clustersDB> [options]");
    if (a.integer("--compressed", 0) != 0) return fail("--compressed 1 is not supported");
    if (a.flag("--cluster-use-weight", false)) return fail("--cluster-use-weight 1 is not supported");
    std::string err;
    Lap lap("clusterhits");
    const std::shared_ptr<const SetInfo> qsP = loadSetInfo(a.pos[0], false, &err);
    if (!qsP) return fail(err);
    const bool sameDb = a.pos[0] == a.pos[1];
    const std::shared_ptr<const SetInfo> tsP = sameDb ? qsP : loadSetInfo(a.pos[1], false, &err);
    if (!tsP) return fail(err);
    const SetInfo &qs = *qsP, &ts = *tsP;
    lap.mark("set info");
    sddb::Reader res, hdr;
    if (!res.open(a.pos[2], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    if (!hdr.open(a.pos[2] + "_h", sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, &err)) return fail(err);
    if (hdr.size() != res.size()) return fail("matches and matches_h differ in size");
    const bool dbOut = a.flag("--db-output", false);

    sd_ch_params par;
    par.maxGeneGap = (uint32_t) a.integer("--max-gene-gap", 3);
    par.clusterSize = (uint32_t) a.integer("--cluster-size", 2);
    par.alpha = a.real("--alpha", 1.0);
    par.pCluThr = (float) a.real("--cluster-pval", 0.01);
    par.pMHThr = (float) a.real("--multihit-pval", 0.01);

    // entries -> flat arrays (R/src/util/ClusterHits.cpp:300-353)
    std::vector<uint64_t> hitOff(1, 0);
    std::vector<uint32_t> qPos, tPos, Nq, entryQSet, entryTSet;
    std::vector<uint8_t> strands;
    std::vector<double> pval;
    std::vector<std::pair<const char *, uint32_t> > lines;   // hit line (with its '\n')
    uint32_t maxOrf = 0;
    for (uint32_t s : qs.setSize) maxOrf = std::max(maxOrf, s);
    for (uint32_t s : ts.setSize) maxOrf = std::max(maxOrf, s);
    uint32_t maxPos = 0;
    // the matches parsed on all threads, each into lists of its own, then laid out back to back in entry order
    struct ParsedMatch {
        std::vector<std::pair<const char *, uint32_t> > lines;
        std::vector<uint32_t> qPos, tPos;
        std::vector<uint8_t> strands;
        std::vector<double> pval;
        unsigned long qSet = 0, tSet = 0, nq = 0;
        uint32_t maxPos = 0;
        std::string error;
    };
    std::vector<ParsedMatch> parsed;
    const size_t parseBlock = 8192;
    for (size_t b0 = 0; b0 < res.size(); b0 += parseBlock) {
        const size_t b1 = std::min(res.size(), b0 + parseBlock);
        parsed.resize(b1 - b0);
#pragma omp parallel for schedule(dynamic, 8)
        for (size_t i = b0; i < b1; i++) {
            ParsedMatch &pm = parsed[i - b0];
            pm.lines.clear();
            pm.qPos.clear();
            pm.tPos.clear();
            pm.strands.clear();
            pm.pval.clear();
            pm.error.clear();
            pm.maxPos = 0;
            const char *h = hdr.data(i);
            char *end;
            pm.qSet = strtoul(h, &end, 10);
            pm.tSet = strtoul(end, &end, 10);
            pm.nq = strtoul(end, &end, 10);
            // six tab separated columns are required (ClusterHits.cpp:303-307)
            int cols = 0;
            for (const char *c = h; *c && *c != '\n'; c++) cols += (*c == '\t');
            if (cols < 5) {
                pm.error = "Invalid header record";
                continue;
            }
            const char *d = res.data(i);
            while (*d != '\0') {
                const char *ls = d;
                char *e2;
                const unsigned long qid = strtoul(d, &e2, 10);
                const unsigned long tid = strtoul(e2, &e2, 10);
                const double p = strtod(e2, nullptr);
                while (*d != '\n' && *d != '\0') d++;
                if (*d == '\n') d++;
                if (qid >= qs.nameOfKey.size() || qs.nameOfKey[qid].empty()) {
                    pm.error = "Invalid query lookup record";
                    break;
                }
                if (tid >= ts.nameOfKey.size() || ts.nameOfKey[tid].empty()) {
                    pm.error = "Invalid target lookup record";
                    break;
                }
                pm.lines.push_back(std::make_pair(ls, (uint32_t) (d - ls)));
                pm.qPos.push_back(qs.posOfKey[qid]);
                pm.tPos.push_back(ts.posOfKey[tid]);
                pm.maxPos = std::max(pm.maxPos, std::max(qs.posOfKey[qid], ts.posOfKey[tid]));
                pm.strands.push_back((uint8_t) (qs.strandOfKey[qid] | (ts.strandOfKey[tid] << 1)));
                pm.pval.push_back(p);
            }
        }
        for (size_t i = b0; i < b1; i++) {
            const ParsedMatch &pm = parsed[i - b0];
            if (!pm.error.empty()) return fail(pm.error);
            const size_t K = pm.lines.size();
            if (K <= 1) continue;   // a single hit is no cluster (ClusterHits.cpp:359-361)
            lines.insert(lines.end(), pm.lines.begin(), pm.lines.end());
            qPos.insert(qPos.end(), pm.qPos.begin(), pm.qPos.end());
            tPos.insert(tPos.end(), pm.tPos.begin(), pm.tPos.end());
            strands.insert(strands.end(), pm.strands.begin(), pm.strands.end());
            pval.insert(pval.end(), pm.pval.begin(), pm.pval.end());
            maxPos = std::max(maxPos, pm.maxPos);
            hitOff.push_back(lines.size());
            Nq.push_back((uint32_t) pm.nq);
            entryQSet.push_back((uint32_t) pm.qSet);
            entryTSet.push_back((uint32_t) pm.tSet);
        }
    }
    parsed.clear();
    parsed.shrink_to_fit();
    lap.mark("parse matches");
    const uint32_t nPairs = (uint32_t) Nq.size();
    const uint64_t total = hitOff.back();
    std::vector<uint32_t> clusterOf(std::max<uint64_t>(total, 1), UINT32_MAX), rank(std::max<uint64_t>(total, 1), 0),
        nClusters(std::max<uint32_t>(nPairs, 1), 0), cSize(std::max<uint64_t>(total, 1), 0);
    std::vector<double> pCO(std::max<uint64_t>(total, 1), 0.0), pMH(std::max<uint64_t>(total, 1), 0.0);
    if (nPairs > 0) {
        CtxH ctx;
        int rc = sd_ctx_create(deviceOf(a), &ctx.c);
        if (rc != SD_OK) return failNoDevice(rc);
        const uint32_t lgN = std::max(maxOrf, maxPos) + 8;
        std::vector<double> lg(lgN);
        sd_host_lgamma_table(lg.data(), lgN);
        rc = sd_clusterhits_batch(ctx.c, &par, nPairs, hitOff.data(), qPos.data(), tPos.data(), strands.data(), pval.data(), Nq.data(),
                                  lg.data(), lgN, clusterOf.data(), rank.data(), nClusters.data(), pCO.data(), pMH.data(), cSize.data());
        if (rc != SD_OK) return failCtx(ctx.c, rc, "sd_clusterhits_batch");
    }
    lap.mark("device");
    sddb::Writer out, outH;
    if (!out.open(a.pos[3], dbOut ? res.dbtype() : (int) sddb::DBTYPE_OMIT_FILE, &err)) return fail(err);
    if (!outH.open(a.pos[3] + "_h", sddb::DBTYPE_GENERIC_DB, &err)) return fail(err);
    uint32_t key = 0;
    // the clusters of a block of set pairs formatted on all threads (members in their rank order), written in order
    struct PairText {
        std::string body, head;
        std::vector<uint32_t> bodyEnd, headEnd;   // per cluster
    };
    std::vector<PairText> texts;
    const uint32_t writeBlock = 4096;
    for (uint32_t e0 = 0; e0 < nPairs; e0 += writeBlock) {
        const uint32_t e1 = std::min(nPairs, e0 + writeBlock);
        texts.resize(e1 - e0);
#pragma omp parallel
        {
            std::vector<uint32_t> member, start;
            char co[32], mh[32];
#pragma omp for schedule(dynamic, 8)
            for (uint32_t e = e0; e < e1; e++) {
                PairText &pt = texts[e - e0];
                pt.body.clear();
                pt.head.clear();
                pt.bodyEnd.clear();
                pt.headEnd.clear();
                const uint64_t off = hitOff[e], end = hitOff[e + 1];
                const uint32_t nC = nClusters[e];
                start.assign((size_t) nC + 1, 0);
                for (uint32_t c = 0; c < nC; c++) start[c + 1] = start[c] + cSize[off + c];
                member.assign(start[nC], 0);
                for (uint64_t h = off; h < end; h++)
                    if (clusterOf[h] < nC) member[start[clusterOf[h]] + rank[h]] = (uint32_t) (h - off);
                for (uint32_t c = 0; c < nC; c++) {
                    for (uint32_t x = start[c]; x < start[c + 1]; x++) pt.body.append(lines[off + member[x]].first, lines[off + member[x]].second);
                    snprintf(co, sizeof(co), "%.3E", pCO[off + c]);
                    snprintf(mh, sizeof(mh), "%.3E", pMH[off + c]);
                    pt.head += std::to_string(entryQSet[e]) + "\t" + std::to_string(entryTSet[e]) + "\t" + co + "\t" + mh + "\t" +
                               std::to_string(cSize[off + c]) + "\n";
                    pt.bodyEnd.push_back((uint32_t) pt.body.size());
                    pt.headEnd.push_back((uint32_t) pt.head.size());
                }
            }
        }
        for (uint32_t e = e0; e < e1; e++) {
            const PairText &pt = texts[e - e0];
            uint32_t b0 = 0, h0 = 0;
            for (size_t c = 0; c < pt.bodyEnd.size(); c++) {
                if (!out.write(key, pt.body.data() + b0, pt.bodyEnd[c] - b0) || !outH.write(key, pt.head.data() + h0, pt.headEnd[c] - h0))
                    return fail("cannot write " + a.pos[3]);
                b0 = pt.bodyEnd[c];
                h0 = pt.headEnd[c];
                key++;
            }
        }
    }
    lap.mark("write clusters");
    if (!out.close(&err) || !outH.close(&err)) return fail(err);
    if (!dbOut) ::remove((a.pos[3] + ".index").c_str());
    lap.mark("close");
    info(a, "%u clusters from %u set pairs\n", key, nPairs);
    return 0;
}

}  // namespace sdcli
