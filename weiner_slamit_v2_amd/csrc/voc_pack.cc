// voc_pack.cc — see voc_pack.h.  Reference: Thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1345-1440 (loadFromTextFile).
#include "voc_pack.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static bool refuse(std::string& why, const std::string& msg) { why = msg; return false; }

// The header's bounds (:1377) and the combinations that are built: the others take different accumulate and normalise branches
// (:1180-1198, ScoringObject.cpp).
static bool check_header(int k, int L, int scoring, int weighting, std::string& why) {
    if (k < 0 || k > SLAMIT_VOC_MAX_K || L < 1 || L > SLAMIT_VOC_MAX_L || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3)
        return refuse(why, "vocabulary header out of bounds (k 0..20, L 1..10, scoring 0..5, weighting 0..3)");
    if (weighting != 0 && weighting != 1) return refuse(why, "vocabulary weighting is not TF_IDF (0) or TF (1): not built");
    if (scoring != 0) return refuse(why, "vocabulary scoring is not L1_NORM (0): not built");
    return true;
}

// Line format: "k L scoring weighting", then per node "parent is_leaf b0 .. b31 weight".  Node ids count the node lines from 1.
// Departure from the reference: its loop is while(!f.eof()) (:1396), so the empty string getline returns after a final newline
// becomes one more node, parent 0 by an unset `pid`: a phantom child of the root.  Empty lines are skipped here.
bool voc_load_text(const char* path, VocArrays& out, std::string& why) {
    FILE* f = path ? fopen(path, "rb") : nullptr;
    if (!f) return refuse(why, std::string("cannot open vocabulary file ") + (path ? path : "(null)"));
    std::vector<char> buf;
    {
        char chunk[1 << 16];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
        fclose(f);
    }
    buf.push_back('\n');
    buf.push_back(0);
    out = VocArrays();
    char* p = buf.data();
    char* const end = buf.data() + buf.size() - 1;
    long line_no = 0;
    bool have_header = false;
    while (p < end) {
        char* nl = (char*)memchr(p, '\n', (size_t)(end - p));
        *nl = 0;
        ++line_no;
        char* s = p;
        p = nl + 1;
        while (*s == ' ' || *s == '\t' || *s == '\r') ++s;
        if (!*s) {
            if (!have_header) return refuse(why, "vocabulary file: empty header line");
            continue;
        }
        char* e = nullptr;
        if (!have_header) {
            long v[4];
            for (int i = 0; i < 4; ++i) { v[i] = strtol(s, &e, 10); if (e == s) return refuse(why, "vocabulary file: header is not 'k L scoring weighting'"); s = e; }
            if (!check_header((int)v[0], (int)v[1], (int)v[2], (int)v[3], why)) return false;
            out.k = (int32_t)v[0]; out.L = (int32_t)v[1]; out.scoring = (int32_t)v[2]; out.weighting = (int32_t)v[3];
            have_header = true;
            continue;
        }
        long head[2];
        uint8_t d[SLAMIT_DESC_BYTES];
        bool ok = true;
        for (int i = 0; i < 2 && ok; ++i) { head[i] = strtol(s, &e, 10); ok = e != s; s = e; }
        for (int i = 0; i < SLAMIT_DESC_BYTES && ok; ++i) { const long b = strtol(s, &e, 10); ok = e != s; s = e; d[i] = (uint8_t)b; }   // FORB::fromString: (unsigned char)n
        double w = 0;
        if (ok) { w = strtod(s, &e); ok = e != s; }
        if (!ok) return refuse(why, "vocabulary file: line " + std::to_string(line_no) + " is not 'parent is_leaf 32 bytes weight'");
        if (head[0] < 0 || head[0] > 0x7fffffffL) return refuse(why, "vocabulary file: line " + std::to_string(line_no) + " has a bad parent id");
        out.parent.push_back((int32_t)head[0]);
        out.is_leaf.push_back(head[1] > 0 ? 1 : 0);
        out.desc.insert(out.desc.end(), d, d + SLAMIT_DESC_BYTES);
        out.weight.push_back(w);
    }
    if (!have_header) return refuse(why, "vocabulary file is empty");
    return true;
}

bool voc_pack(const slamit_voc_desc& d, VocPacked& out, std::string& why) {
    if (!check_header(d.k, d.L, d.scoring, d.weighting, why)) return false;
    const int n = d.n_nodes;
    if (n < 1) return refuse(why, "vocabulary has no nodes");
    if (!d.parent || !d.is_leaf || !d.desc || !d.weight) return refuse(why, "vocabulary arrays are null");
    // reference ids: 0 = root, i + 1 = entry i.  Children in ascending id = the order of the reference's push_back.
    std::vector<int32_t> count((size_t)n + 1, 0), level((size_t)n + 1, 0);
    int depth = 0, fan = 0;
    for (int i = 0; i < n; ++i) {
        const int id = i + 1, par = d.parent[i];
        if (par < 0 || par >= id) return refuse(why, "vocabulary node " + std::to_string(id) + ": parent id " + std::to_string(par) + " is not smaller than its own");
        if (++count[par] > SLAMIT_VOC_MAX_K) return refuse(why, "vocabulary node " + std::to_string(par) + " has more than SLAMIT_VOC_MAX_K children");
        level[id] = level[par] + 1;
        if (level[id] > SLAMIT_VOC_MAX_L) return refuse(why, "vocabulary node " + std::to_string(id) + " lies deeper than SLAMIT_VOC_MAX_L");
        if (level[id] > depth) depth = level[id];
        if (count[par] > fan) fan = count[par];
    }
    for (int i = 0; i < n; ++i)
        if ((d.is_leaf[i] != 0) != (count[i + 1] == 0))
            return refuse(why, "vocabulary node " + std::to_string(i + 1) + ": is_leaf disagrees with its children");
    // children lists as CSR over reference ids
    std::vector<int32_t> start((size_t)n + 2, 0), kids((size_t)n);
    for (int id = 0; id <= n; ++id) start[id + 1] = start[id] + count[id];
    {
        std::vector<int32_t> fill(start.begin(), start.end() - 1);
        for (int i = 0; i < n; ++i) kids[fill[d.parent[i]]++] = i + 1;
    }
    // word ids: leaves in file order
    std::vector<int32_t> word((size_t)n + 1, -1);
    int nw = 0;
    for (int i = 0; i < n; ++i) if (d.is_leaf[i]) word[i + 1] = nw++;
    // breadth-first renumbering: dev_to_orig is its own queue
    const size_t N = (size_t)n + 1;
    out = VocPacked();
    out.k = d.k; out.L = d.L; out.n_nodes = n; out.n_words = nw; out.max_fanout = fan; out.depth = depth;
    out.child_first.assign(N, 0); out.child_count.assign(N, 0); out.orig_id.assign(N, 0); out.word_id.assign(N, -1);
    out.weight.assign(N, 0.0); out.desc.assign(N * SLAMIT_DESC_BYTES, 0);
    size_t next = 1;
    for (size_t dev = 0; dev < next; ++dev) {
        const int id = out.orig_id[dev];
        out.child_count[dev] = count[id];
        out.child_first[dev] = count[id] ? (int32_t)next : 0;
        for (int c = start[id]; c < start[id + 1]; ++c) out.orig_id[next++] = kids[c];
        if (id > 0) {
            out.word_id[dev] = word[id];
            out.weight[dev] = d.weight[id - 1];
            memcpy(&out.desc[dev * SLAMIT_DESC_BYTES], d.desc + (size_t)(id - 1) * SLAMIT_DESC_BYTES, SLAMIT_DESC_BYTES);
        }
    }
    if (next != N) return refuse(why, "vocabulary tree is not connected");   // cannot happen with parent < id; kept as a bound on `next`
    return true;
}
