// dbow_ref_harness.cc — drives the REFERENCE's own DBoW2 (compiled by oracle/Makefile.ref from /root/reference against the stand-in
// headers of oracle/cvstub, outputs in oracle/_ref/) from POD inputs.  TEST INFRASTRUCTURE ONLY: used in the authoring container to
// generate tests/golden/bow_*.npz (tools/gen_bow_golden.py) and by the live test of tests/test_bow_golden.py.
//
// Calls into Thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h ("T") over FORB, i.e. include/ORBVocabulary.h's ORBVocabulary:
//   loadFromTextFile                                  T:1345-1440
//   transform(feature) -> WordId                      T:1057   public
//   transform(feature, id, weight, &nid, levelsup)    T:1225   protected: reached through a derived class
//   transform(features, v)                            T:1073
//   transform(features, v, fv, levelsup)              T:1134
//   score(a, b)                                       T:1206 -> the scoring object of the text file's header (L1Scoring::score)
// Nothing is restated here: every number that goes out was computed by the reference's code.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "TemplatedVocabulary.h"
#include "FORB.h"

namespace {

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> OrbVocabulary;

struct Voc : public OrbVocabulary {
    // The protected per-feature overload.  *nid comes in as (NodeId)-1: the reference writes it only when the descent passes level
    // L - levelsup (T:1234, :1258), so "never written" goes out as -1.
    void feature(const cv::Mat& d, int levelsup, DBoW2::WordId& id, DBoW2::WordValue& w, DBoW2::NodeId& nid) const {
        nid = (DBoW2::NodeId)-1;
        OrbVocabulary::transform(d, id, w, &nid, levelsup);
    }
    int nodes() const { return (int)m_nodes.size() - 1; }
    int words() const { return (int)m_words.size(); }
};

std::vector<cv::Mat> features(const uint8_t* desc, int n) {
    std::vector<cv::Mat> f((size_t)n);
    for (int i = 0; i < n; ++i) {
        f[i].create(1, 32, CV_8U);
        std::memcpy(f[i].ptr<unsigned char>(), desc + 32 * (size_t)i, 32);
    }
    return f;
}

void put(const DBoW2::BowVector& v, int32_t* bow_n, int32_t* bow_word, double* bow_value) {
    int j = 0;
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it, ++j) {   // std::map: ascending word id
        bow_word[j] = (int32_t)it->first;
        bow_value[j] = it->second;
    }
    *bow_n = j;
}

DBoW2::BowVector take(int n, const int32_t* word, const double* value) {
    DBoW2::BowVector v;
    for (int i = 0; i < n; ++i) v.insert(v.end(), DBoW2::BowVector::value_type((DBoW2::WordId)word[i], value[i]));
    return v;
}

}  // namespace

extern "C" {

void* dbow_ref_load(const char* path) {
    Voc* v = new Voc();
    if (!v->loadFromTextFile(path) || v->empty()) {
        delete v;
        return 0;
    }
    return v;
}

void dbow_ref_free(void* h) { delete static_cast<Voc*>(h); }

// head = k L scoring weighting n_nodes (without the root) n_words
void dbow_ref_info(const void* h, int32_t* head) {
    const Voc* v = static_cast<const Voc*>(h);
    head[0] = v->getBranchingFactor();
    head[1] = v->getDepthLevels();
    head[2] = (int32_t)v->getScoringType();
    head[3] = (int32_t)v->getWeightingType();
    head[4] = v->nodes();
    head[5] = v->words();
}

// Per feature: word_pub from the public transform(feature); word_id, weight, node_id (-1 = not written) from the protected overload.
void dbow_ref_features(const void* h, const uint8_t* desc, int n, int levelsup, int32_t* word_pub, int32_t* word_id, double* weight,
                       int32_t* node_id) {
    const Voc* v = static_cast<const Voc*>(h);
    std::vector<cv::Mat> f = features(desc, n);
    for (int i = 0; i < n; ++i) {
        word_pub[i] = (int32_t)static_cast<const OrbVocabulary*>(v)->transform(f[i]);
        DBoW2::WordId id;
        DBoW2::WordValue w;
        DBoW2::NodeId nid;
        v->feature(f[i], levelsup, id, w, nid);
        word_id[i] = (int32_t)id;
        weight[i] = w;
        node_id[i] = (int32_t)nid;
    }
}

// transform(features, v): outputs sized n.
void dbow_ref_transform_bow(const void* h, const uint8_t* desc, int n, int32_t* bow_n, int32_t* bow_word, double* bow_value) {
    DBoW2::BowVector bv;
    static_cast<const OrbVocabulary*>(static_cast<const Voc*>(h))->transform(features(desc, n), bv);
    put(bv, bow_n, bow_word, bow_value);
}

// transform(features, v, fv, levelsup): outputs sized n (fv_ptr n + 1); the FeatureVector as CSR in ascending node id.
void dbow_ref_transform(const void* h, const uint8_t* desc, int n, int levelsup, int32_t* bow_n, int32_t* bow_word, double* bow_value,
                        int32_t* fv_n, int32_t* fv_node, int32_t* fv_ptr, int32_t* fv_items) {
    DBoW2::BowVector bv;
    DBoW2::FeatureVector fv;
    static_cast<const OrbVocabulary*>(static_cast<const Voc*>(h))->transform(features(desc, n), bv, fv, levelsup);
    put(bv, bow_n, bow_word, bow_value);
    int j = 0, m = 0;
    fv_ptr[0] = 0;
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it, ++j) {
        fv_node[j] = (int32_t)it->first;
        for (size_t i = 0; i < it->second.size(); ++i) fv_items[m++] = (int32_t)it->second[i];
        fv_ptr[j + 1] = m;
    }
    *fv_n = j;
}

// score(a, b) of two BowVectors handed back as (word ids ascending, values).
double dbow_ref_score(const void* h, int n1, const int32_t* w1, const double* v1, int n2, const int32_t* w2, const double* v2) {
    return static_cast<const Voc*>(h)->score(take(n1, w1, v1), take(n2, w2, v2));
}

}  // extern "C"
