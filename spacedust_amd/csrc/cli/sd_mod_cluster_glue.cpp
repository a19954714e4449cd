// Host glue of `cluster --single-step-clustering 1` (M/data/workflow/clustering.sh); no device.
//
// createsubdb <subsetFile|DB> <DB> <DB>  (M/src/util/createsubdb.cpp:10-101, DBReader::softlinkDb): the entries of the second DB whose keys
//   the first argument lists -- its .index when it has one (clustering.sh passes a cluster DB), else the file itself, first column of every
//   line.  --subdb-mode 0 copies the entries; --subdb-mode 1 writes index entries that keep the source's offsets and links the data file(s).
//   Both link the ancillary files (_h, .lookup, .source, taxonomy) and copy the dbtype.  The index stays in list order and is sorted by key
//   only when the list was not ascending.  A key that the source lacks: a warning, skipped.  --id-mode 1 (names through the lookup) is refused.
// mergeclusters <sequenceDB> <clusterDB> <clu1> <clu2> [...]  (M/src/util/mergeclusters.cpp:13-153): the member lists of step 1 by
//   representative; for every later step and every cluster of it, the lists of the members other than the representative spliced behind the
//   representative's list, in the order the entry names them; one DBTYPE_CLUSTER_RES entry per non-empty list, in sequence-DB order.  A key
//   that the sequence DB lacks is an error that names it (the reference indexes out of bounds there).
#include "sd_cli.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits.h>
#include <list>
#include <unistd.h>

namespace sdcli {

namespace {

// FileUtil::symlinkAbs: link -> the real path of target; an existing link is replaced
bool symlinkAbs(const std::string &target, const std::string &link, std::string *err) {
    char real[PATH_MAX];
    if (!realpath(target.c_str(), real)) {
        *err = "cannot resolve " + target;
        return false;
    }
    unlink(link.c_str());
    if (symlink(real, link.c_str()) != 0) {
        *err = "cannot link " + link + " to " + real;
        return false;
    }
    return true;
}

bool linkIfThere(const std::string &from, const std::string &to, std::string *err) {
    return !sddb::fileExists(from) || symlinkAbs(from, to, err);
}

// DBFiles::SEQUENCE_ANCILLARY: everything of a sequence DB but data, index and dbtype
bool linkAncillary(const std::string &from, const std::string &to, std::string *err) {
    for (const char *suffix : {"_h", "_h.index", "_h.dbtype", ".lookup", ".source", "_mapping", "_names.dmp", "_nodes.dmp", "_merged.dmp", "_taxonomy"})
        if (!linkIfThere(from + suffix, to + suffix, err)) return false;
    return true;
}

// DBFiles::DATA: NAME, or NAME.0 .. NAME.N-1
bool linkData(const std::string &from, const std::string &to, std::string *err) {
    if (sddb::fileExists(from + ".0")) {
        for (size_t i = 0; sddb::fileExists(from + "." + std::to_string(i)); i++)
            if (!symlinkAbs(from + "." + std::to_string(i), to + "." + std::to_string(i), err)) return false;
        return true;
    }
    return symlinkAbs(from, to, err);
}

struct IndexLine {
    uint32_t key;
    uint64_t offset, length;
};

bool writeIndex(const std::string &path, std::vector<IndexLine> &index, bool sortByKey, std::string *err) {
    if (sortByKey) std::stable_sort(index.begin(), index.end(), [](const IndexLine &a, const IndexLine &b) { return a.key < b.key; });
    FILE *f = fopen(path.c_str(), "w");
    if (!f) {
        *err = "cannot write " + path;
        return false;
    }
    for (const IndexLine &e : index) fprintf(f, "%u\t%llu\t%llu\n", e.key, (unsigned long long) e.offset, (unsigned long long) e.length);
    return fclose(f) == 0;
}

}  // namespace

// the keys a list names, in its order: the first column of every line (Util::parseKey + fast_atoi: the digits the line starts with)
bool readKeyList(const std::string &path, std::vector<uint32_t> &keys, std::string *err) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) {
        *err = "File " + path + " does not exist.";
        return false;
    }
    char *line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, f) != -1) {
        uint64_t v = 0;
        for (const char *c = line; *c >= '0' && *c <= '9'; c++) v = v * 10 + (uint64_t) (*c - '0');
        keys.push_back((uint32_t) v);
    }
    free(line);
    fclose(f);
    return true;
}

int createsubdbModule(const Args &a) {
    if (a.pos.size() != 3) return fail("usage: createsubdb <subsetFile|DB> <DB> <DB> [--subdb-mode 0|1]");
    if (int rc = checkCommon(a)) return rc;
    if (a.integer("--id-mode", 0) != 0) return fail("--id-mode 1 (a list of names, through the lookup) is not implemented");
    const int mode = (int) a.integer("--subdb-mode", 0);
    if (mode != 0 && mode != 1) return fail("--subdb-mode " + std::to_string(mode) + ": 0 (copy) and 1 (soft link) exist");
    std::string err;
    std::vector<uint32_t> keys;
    const std::string list = sddb::fileExists(a.pos[0] + ".index") ? a.pos[0] + ".index" : a.pos[0];
    if (!readKeyList(list, keys, &err)) return fail(err);
    sddb::Reader src;
    if (!src.open(a.pos[1], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::NOSORT, &err)) return fail(err);
    const std::string &out = a.pos[2];
    std::vector<IndexLine> index;
    bool ordered = true;
    uint32_t prev = 0;
    FILE *data = nullptr;
    if (mode == 0) {
        unlink(out.c_str());   // (a link left by an earlier soft-linked DB of this name must not be written through)
        data = fopen(out.c_str(), "wb");
        if (!data) return fail("cannot write " + out);
    }
    uint64_t at = 0;
    for (const uint32_t key : keys) {
        ordered = ordered && prev <= key;
        prev = key;
        const size_t id = src.idOfKey(key);
        if (id == SIZE_MAX) {
            if (a.integer("-v", 3) >= 2) fprintf(stderr, "Key %u not found in database\n", key);   // (a warning: -v 2 and above)
            continue;
        }
        const uint64_t len = src.entryLength(id);
        if (mode == 1) {
            index.push_back({key, src.entryOffset(id), len});
        } else {
            // the payload and a terminator of its own; the index keeps the source's length
            const uint64_t payload = std::max<uint64_t>(len, 1) - 1;
            if ((payload && fwrite(src.data(id), 1, (size_t) payload, data) != payload) || fputc('\0', data) == EOF) {
                fclose(data);
                return fail("cannot write " + out);
            }
            index.push_back({key, at, len});
            at += payload + 1;
        }
    }
    if (data && fclose(data) != 0) return fail("cannot write " + out);
    if (!writeIndex(out + ".index", index, !ordered, &err)) return fail(err);
    if (mode == 1 && !linkData(a.pos[1], out, &err)) return fail(err);
    {
        FILE *f = fopen((out + ".dbtype").c_str(), "wb");
        const int32_t t = src.dbtype();
        if (!f || fwrite(&t, 4, 1, f) != 1 || fclose(f) != 0) return fail("cannot write " + out + ".dbtype");
    }
    if (!linkAncillary(a.pos[1], out, &err)) return fail(err);
    return 0;
}

// the merged lists as entries of the cluster DB: (representative key, text), in sequence-DB order.  false with the key in *err when a
// cluster DB names a key that the sequence DB lacks
bool mergeClusterLists(const sddb::Reader &seqs, const std::vector<std::string> &steps, std::vector<std::pair<uint32_t, std::string> > &out,
                       std::string *err) {
    std::vector<std::list<uint32_t> > merged(seqs.size());
    bool ok = true;
    auto idOf = [&](uint32_t key, const std::string &where) -> size_t {
        const size_t id = seqs.idOfKey(key);
        if (id == SIZE_MAX && ok) {
            ok = false;
            *err = "key " + std::to_string(key) + " of " + where + " is not in the sequence DB " + seqs.name();
        }
        return id;
    };
    for (size_t s = 0; s < steps.size() && ok; s++) {
        sddb::Reader clu;
        if (!clu.open(steps[s], sddb::Reader::USE_INDEX | sddb::Reader::USE_DATA, sddb::Reader::LINEAR_ACCESS, err)) return false;
        for (size_t i = 0; i < clu.size() && ok; i++) {
            const size_t cluId = idOf(clu.key(i), steps[s]);
            if (!ok) break;
            for (const char *c = clu.data(i); *c != '\0';) {
                uint64_t v = 0;
                for (const char *d = c; *d >= '0' && *d <= '9'; d++) v = v * 10 + (uint64_t) (*d - '0');
                const size_t seqId = idOf((uint32_t) v, steps[s]);
                if (!ok) break;
                if (s == 0) {
                    merged[cluId].push_back((uint32_t) seqId);
                } else if (seqId != cluId) {   // (the representative's own list stays where it is)
                    merged[cluId].splice(merged[cluId].end(), merged[seqId]);
                }
                while (*c != '\0' && *c != '\n') c++;
                if (*c == '\n') c++;
            }
        }
    }
    if (!ok) return false;
    for (size_t i = 0; i < seqs.size(); i++) {
        if (merged[i].empty()) continue;
        std::string text;
        for (const uint32_t id : merged[i]) text += std::to_string(seqs.key(id)) + "\n";
        out.emplace_back(seqs.key(i), std::move(text));
    }
    return true;
}

int mergeclustersModule(const Args &a) {
    if (a.pos.size() < 3) return fail("usage: mergeclusters <sequenceDB> <clusterDB> <clusterDB1> [<clusterDB2> ...]");
    if (int rc = checkCommon(a)) return rc;
    std::string err;
    sddb::Reader seqs;
    if (!seqs.open(a.pos[0], sddb::Reader::USE_INDEX, sddb::Reader::NOSORT, &err)) return fail(err);
    std::vector<std::pair<uint32_t, std::string> > entries;
    if (!mergeClusterLists(seqs, std::vector<std::string>(a.pos.begin() + 2, a.pos.end()), entries, &err)) return fail(err);
    sddb::Writer out;
    if (!out.open(a.pos[1], sddb::DBTYPE_CLUSTER_RES, &err)) return fail(err);
    for (const auto &e : entries)
        if (!out.write(e.first, e.second.data(), e.second.size())) return fail("cannot write " + a.pos[1]);
    if (!out.close(&err)) return fail(err);
    return 0;
}

}  // namespace sdcli
