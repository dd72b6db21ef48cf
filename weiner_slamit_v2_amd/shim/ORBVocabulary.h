// ORBVocabulary.h — ORB_SLAM2::ORBVocabulary (include/ORBVocabulary.h: DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) above the
// C-ABI: the part of the class that Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:520-527, src/KeyFrame.cc:63-72) and
// System's start-up (loadFromTextFile) use.  transform() runs on the device (slamit_voc_transform); the two maps it fills have the
// shapes shim/ORBmatcher.h accepts as DBoW2::BowVector / DBoW2::FeatureVector.  score() is L1Scoring::score restated on the host, for
// the dozen calls of LoopClosing.cc:149; the keyframe database is shim/KeyFrameDatabase.h.  Not here: vocabulary creation.
// A loaded vocabulary may be used by several threads at once, as the reference's is: transform() is const and
// the call's state lives in the calling thread.
#ifndef SLAMIT_SHIM_ORBVOCABULARY_H
#define SLAMIT_SHIM_ORBVOCABULARY_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#ifdef SLAMIT_USE_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvlite.h"
#endif

#include "../../include/slamit.h"

namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
typedef unsigned int NodeId;
typedef std::map<WordId, WordValue> BowVector;                           // the reference's derive from these maps
typedef std::map<NodeId, std::vector<unsigned int> > FeatureVector;
}  // namespace DBoW2

namespace ORB_SLAM2 {

class ORBVocabulary {
public:
    explicit ORBVocabulary(int device = 0) : mDevice(device), mVoc(nullptr), mWords(0) {}
    ~ORBVocabulary() { slamit_voc_destroy(mVoc); }
    ORBVocabulary(const ORBVocabulary&) = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;

    // TemplatedVocabulary::loadFromTextFile: false when the file is missing or not a vocabulary (slamit_last_error() says why)
    bool loadFromTextFile(const std::string& filename) {
        slamit_voc* v = nullptr;
        if (slamit_voc_load_text(filename.c_str(), mDevice, &v) != SLAMIT_OK) return false;
        slamit_voc_destroy(mVoc);
        mVoc = v;
        int32_t nw = 0;
        slamit_voc_info(mVoc, nullptr, nullptr, nullptr, &nw);
        mWords = (unsigned int)nw;
        return true;
    }

    // the same vocabulary from arrays (slamit_voc_desc), for callers that keep it in another format
    bool create(const slamit_voc_desc& desc) {
        slamit_voc* v = nullptr;
        if (slamit_voc_create(&desc, mDevice, &v) != SLAMIT_OK) return false;
        slamit_voc_destroy(mVoc);
        mVoc = v;
        int32_t nw = 0;
        slamit_voc_info(mVoc, nullptr, nullptr, nullptr, &nw);
        mWords = (unsigned int)nw;
        return true;
    }

    unsigned int size() const { return mWords; }   // number of words
    bool empty() const { return mWords == 0; }

    // TemplatedVocabulary::transform(features, v, fv, levelsup): features are 1 x 32 CV_8U rows (Converter::toDescriptorVector)
    void transform(const std::vector<cv::Mat>& features, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const {
        v.clear();
        fv.clear();
        if (empty()) return;
        const int n = (int)features.size();
        std::vector<uint8_t> desc((size_t)n * SLAMIT_DESC_BYTES);
        for (int i = 0; i < n; ++i) memcpy(&desc[(size_t)i * SLAMIT_DESC_BYTES], features[i].ptr(0), SLAMIT_DESC_BYTES);
        const size_t m = n > 0 ? n : 1;
        std::vector<int32_t> word(m), node(m), bw(m), fnode(m), fptr(m + 1), fitems(m);
        std::vector<double> bv(m);
        int32_t bn = 0, fn = 0;
        if (slamit_voc_transform(mVoc, desc.data(), n, levelsup, word.data(), node.data(), &bn, bw.data(), bv.data(), &fn, fnode.data(),
                                 fptr.data(), fitems.data()) != SLAMIT_OK)
            return;   // the reference's transform cannot fail; slamit_last_error() keeps the reason
        DBoW2::BowVector::iterator vit = v.end();
        for (int j = 0; j < bn; ++j) vit = v.insert(vit, std::make_pair((DBoW2::WordId)bw[j], bv[j]));   // ascending: appended in O(1)
        DBoW2::FeatureVector::iterator fit = fv.end();
        for (int j = 0; j < fn; ++j) {
            fit = fv.insert(fit, std::make_pair((DBoW2::NodeId)fnode[j], std::vector<unsigned int>()));
            fit->second.assign(fitems.begin() + fptr[j], fitems.begin() + fptr[j + 1]);
        }
    }

    // TemplatedVocabulary::score for L1_NORM (Thirdparty/DBoW2/src/ScoringObject.cpp:23-68), the only scoring slamit_voc_create
    // accepts: one term per shared word in ascending word id, added from 0.0, then -sum / 2.  Both maps ascend, so stepping the one
    // with the smaller id visits the same words in the same order as the reference's lower_bound walk: the same double, bit for bit
    // (slamit_kfdb_query returns it for a whole database at once).
    double score(const DBoW2::BowVector& v1, const DBoW2::BowVector& v2) const {
        DBoW2::BowVector::const_iterator a = v1.begin(), b = v2.begin();
        double sum = 0.0;
        while (a != v1.end() && b != v2.end()) {
            if (a->first < b->first) ++a;
            else if (b->first < a->first) ++b;
            else {
                const double vi = a->second, wi = b->second;
                sum += fabs(vi - wi) - fabs(vi) - fabs(wi);
                ++a;
                ++b;
            }
        }
        return -sum / 2.0;
    }

    int device() const { return mDevice; }   // the GPU this vocabulary lives on (shim/KeyFrameDatabase.h puts its handle there too)

private:
    int mDevice;
    slamit_voc* mVoc;
    unsigned int mWords;
};

}  // namespace ORB_SLAM2

#endif
