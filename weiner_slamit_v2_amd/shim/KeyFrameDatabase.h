// KeyFrameDatabase.h — ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) above the C-ABI, as a
// template over the caller's KeyFrame and Frame types.  The inverted file is gone: the handle (slamit_kfdb_*) keeps every keyframe's
// BowVector on the device and one dense query gives, per keyframe, the number of shared words, the smallest shared word and the L1
// score.  Everything after it is the reference's host logic in the reference's order, on the members the reference keeps in the
// keyframes themselves: mnLoopQuery / mnLoopWords / mLoopScore and mnRelocQuery / mnRelocWords / mRelocScore are written exactly
// where KeyFrameDatabase.cc writes them -- :103 included, which zeroes the words of a connected keyframe without claiming it -- so
// a relocalisation still adds the mRelocScore an EARLIER query left in a neighbour that shares a word but missed minCommonWords
// (:292-295).  Initialise the two scores in your KeyFrame (the reference does not; 0.0f is what api.KeyFrameDatabase uses).
//
// KeyFrameT needs mnId, mBowVec, the six members, GetConnectedKeyFrames() -> std::set<KeyFrameT*> and
// GetBestCovisibilityKeyFrames(int) -> std::vector<KeyFrameT*>; FrameT needs mnId and mBowVec.
#ifndef SLAMIT_SHIM_KEYFRAMEDATABASE_H
#define SLAMIT_SHIM_KEYFRAMEDATABASE_H

#include <stdint.h>

#include <algorithm>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "ORBVocabulary.h"

namespace ORB_SLAM2 {

template <class KeyFrameT, class FrameT>
class KeyFrameDatabase {
public:
    // slots / maxWords size the first handle; a full one is replaced by one of twice the slots (and a keyframe with more words than
    // maxWords by one that holds them), refilled from the keyframes' own mBowVec in the order they were added
    KeyFrameDatabase(const ORBVocabulary& voc, int slots = 256, int maxWords = 2048)
        : mpVoc(&voc), mDb(nullptr), mSlots(slots < 1 ? 1 : slots), mMaxWords(std::min(std::max(maxWords, 1), SLAMIT_VOC_MAX_FEATURES)), mNextOrder(0) {}
    ~KeyFrameDatabase() { slamit_kfdb_destroy(mDb); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    void add(KeyFrameT* pKF) {                                             // :45-54
        std::unique_lock<std::mutex> lock(mMutex);
        if (mSlotOf.count(pKF)) return;                                    // (one entry per keyframe; the reference's callers add once)
        const int n = (int)pKF->mBowVec.size();
        if (n > SLAMIT_VOC_MAX_FEATURES) return;                           // cannot be a BowVector of slamit_voc_transform
        if (!mDb || n > mMaxWords || (int)mSlotOf.size() >= mSlots) {
            int slots = mSlots, words = mMaxWords;
            if (mDb && (int)mSlotOf.size() >= mSlots) slots *= 2;
            while (words < n) words = std::min(2 * words, SLAMIT_VOC_MAX_FEATURES);
            if (!rebuild(slots, words)) return;
        }
        const int slot = put(pKF);
        if (slot < 0) return;
        mSlotOf[pKF] = slot;
        mKFOfSlot[slot] = pKF;
        mOrderOfSlot[slot] = mNextOrder++;
    }

    void erase(KeyFrameT* pKF) {                                           // :56-75; an absent keyframe: nothing happens
        std::unique_lock<std::mutex> lock(mMutex);
        typename std::map<KeyFrameT*, int>::iterator it = mSlotOf.find(pKF);
        if (it == mSlotOf.end()) return;
        slamit_kfdb_erase(mDb, it->second);
        mKFOfSlot[it->second] = nullptr;
        mSlotOf.erase(it);
    }

    void clear() {                                                         // :77-81
        std::unique_lock<std::mutex> lock(mMutex);
        if (mDb) slamit_kfdb_clear(mDb);
        mSlotOf.clear();
        std::fill(mKFOfSlot.begin(), mKFOfSlot.end(), (KeyFrameT*)nullptr);
    }

    // Loop Detection (:84-206)
    std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore) {
        std::set<KeyFrameT*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
        std::vector<std::pair<KeyFrameT*, float> > lKFsSharingWords;       // with the keyframe's score as a float (:142)
        {
            std::unique_lock<std::mutex> lock(mMutex);
            Dense d;
            if (!dense(pKF->mBowVec, d)) return std::vector<KeyFrameT*>();
            for (size_t k = 0; k < d.order.size(); ++k) {                  // :94-112, a keyframe at a time instead of a word at a time
                const int s = d.order[k];
                KeyFrameT* pKFi = mKFOfSlot[s];
                if (pKFi->mnLoopQuery != pKF->mnId) {
                    if (!spConnectedKeyFrames.count(pKFi)) {
                        pKFi->mnLoopQuery = pKF->mnId;
                        pKFi->mnLoopWords = d.common[s];
                        lKFsSharingWords.push_back(std::make_pair(pKFi, (float)d.score[s]));
                    } else {
                        pKFi->mnLoopWords = 1;                             // :103 at every shared word, :110 after the last one
                    }
                } else {
                    pKFi->mnLoopWords += d.common[s];                      // already claimed by this id: :110 alone
                }
            }
        }
        if (lKFsSharingWords.empty()) return std::vector<KeyFrameT*>();
        int maxCommonWords = 0;
        for (size_t k = 0; k < lKFsSharingWords.size(); ++k)
            if (lKFsSharingWords[k].first->mnLoopWords > maxCommonWords) maxCommonWords = lKFsSharingWords[k].first->mnLoopWords;
        const int minCommonWords = maxCommonWords * 0.8f;                  // :129
        std::list<std::pair<float, KeyFrameT*> > lScoreAndMatch;
        for (size_t k = 0; k < lKFsSharingWords.size(); ++k) {             // :134-148
            KeyFrameT* pKFi = lKFsSharingWords[k].first;
            if (pKFi->mnLoopWords > minCommonWords) {
                const float si = lKFsSharingWords[k].second;
                pKFi->mLoopScore = si;
                if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, pKFi));
            }
        }
        if (lScoreAndMatch.empty()) return std::vector<KeyFrameT*>();
        std::list<std::pair<float, KeyFrameT*> > lAccScoreAndMatch;
        float bestAccScore = minScore;                                     // :154
        for (typename std::list<std::pair<float, KeyFrameT*> >::iterator it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); ++it) {   // :157-182
            KeyFrameT* pKFi = it->second;
            std::vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
            float bestScore = it->first, accScore = it->first;
            KeyFrameT* pBestKF = pKFi;
            for (size_t j = 0; j < vpNeighs.size(); ++j) {
                KeyFrameT* pKF2 = vpNeighs[j];
                if (pKF2->mnLoopQuery == pKF->mnId && pKF2->mnLoopWords > minCommonWords) {
                    accScore += pKF2->mLoopScore;
                    if (pKF2->mLoopScore > bestScore) { pBestKF = pKF2; bestScore = pKF2->mLoopScore; }
                }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        return retain(lAccScoreAndMatch, 0.75f * bestAccScore);            // :185-205
    }

    // Relocalization (:208-328)
    std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F) {
        std::vector<std::pair<KeyFrameT*, float> > lKFsSharingWords;
        {
            std::unique_lock<std::mutex> lock(mMutex);
            Dense d;
            if (!dense(F->mBowVec, d)) return std::vector<KeyFrameT*>();
            for (size_t k = 0; k < d.order.size(); ++k) {                  // :219-237
                const int s = d.order[k];
                KeyFrameT* pKFi = mKFOfSlot[s];
                if (pKFi->mnRelocQuery != F->mnId) {
                    pKFi->mnRelocWords = d.common[s];
                    pKFi->mnRelocQuery = F->mnId;
                    lKFsSharingWords.push_back(std::make_pair(pKFi, (float)d.score[s]));
                } else {
                    pKFi->mnRelocWords += d.common[s];
                }
            }
        }
        if (lKFsSharingWords.empty()) return std::vector<KeyFrameT*>();
        int maxCommonWords = 0;
        for (size_t k = 0; k < lKFsSharingWords.size(); ++k)
            if (lKFsSharingWords[k].first->mnRelocWords > maxCommonWords) maxCommonWords = lKFsSharingWords[k].first->mnRelocWords;
        const int minCommonWords = maxCommonWords * 0.8f;                  // :254
        std::list<std::pair<float, KeyFrameT*> > lScoreAndMatch;
        for (size_t k = 0; k < lKFsSharingWords.size(); ++k) {             // :261-272
            KeyFrameT* pKFi = lKFsSharingWords[k].first;
            if (pKFi->mnRelocWords > minCommonWords) {
                const float si = lKFsSharingWords[k].second;
                pKFi->mRelocScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, pKFi));
            }
        }
        if (lScoreAndMatch.empty()) return std::vector<KeyFrameT*>();
        std::list<std::pair<float, KeyFrameT*> > lAccScoreAndMatch;
        float bestAccScore = 0;                                            // :278
        for (typename std::list<std::pair<float, KeyFrameT*> >::iterator it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); ++it) {   // :281-306
            KeyFrameT* pKFi = it->second;
            std::vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
            float bestScore = it->first, accScore = bestScore;
            KeyFrameT* pBestKF = pKFi;
            for (size_t j = 0; j < vpNeighs.size(); ++j) {
                KeyFrameT* pKF2 = vpNeighs[j];
                if (pKF2->mnRelocQuery != F->mnId) continue;               // :292: shares any word with F
                accScore += pKF2->mRelocScore;                             // this query's, or what an earlier one left
                if (pKF2->mRelocScore > bestScore) { pBestKF = pKF2; bestScore = pKF2->mRelocScore; }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        return retain(lAccScoreAndMatch, 0.75f * bestAccScore);            // :309-327
    }

    int slots() const { return mDb ? mSlots : 0; }                         // of the current handle (0: none yet)

protected:
    struct Dense {
        std::vector<int32_t> common, first;
        std::vector<int64_t> seq;
        std::vector<double> score;
        std::vector<int> order;          // the slots that share a word, as the reference's walk first meets their keyframes
    };
    struct ByFirstWordThenSeq {
        const Dense* d;
        bool operator()(int a, int b) const { return d->first[a] != d->first[b] ? d->first[a] < d->first[b] : d->seq[a] < d->seq[b]; }
    };

    static void flatten(const DBoW2::BowVector& v, std::vector<int32_t>& w, std::vector<double>& x) {
        w.clear(); x.clear();
        for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) { w.push_back((int32_t)it->first); x.push_back(it->second); }
    }

    bool dense(const DBoW2::BowVector& v, Dense& d) {                      // mMutex held
        if (!mDb || mSlotOf.empty()) return false;
        std::vector<int32_t> w;
        std::vector<double> x;
        flatten(v, w, x);
        d.common.resize(mSlots); d.first.resize(mSlots); d.seq.resize(mSlots); d.score.resize(mSlots);
        if (slamit_kfdb_query(mDb, w.data(), x.data(), (int)w.size(), d.common.data(), d.first.data(), d.seq.data(), d.score.data()) != SLAMIT_OK)
            return false;                                                  // slamit_last_error() keeps the reason
        for (int s = 0; s < mSlots; ++s)
            if (d.common[s] >= 1 && mKFOfSlot[s]) d.order.push_back(s);
        ByFirstWordThenSeq cmp = {&d};
        std::sort(d.order.begin(), d.order.end(), cmp);
        return true;
    }

    int put(KeyFrameT* pKF) {
        std::vector<int32_t> w;
        std::vector<double> x;
        flatten(pKF->mBowVec, w, x);
        int32_t slot = -1;
        return slamit_kfdb_add(mDb, w.data(), x.data(), (int)w.size(), &slot) == SLAMIT_OK ? (int)slot : -1;
    }

    // a new handle of `slots` x `words`, refilled in the order the keyframes were added: their places in the lists stay
    bool rebuild(int slots, int words) {
        slamit_kfdb* db = nullptr;
        if (slamit_kfdb_create(slots, words, mpVoc->device(), &db) != SLAMIT_OK) return false;
        std::vector<std::pair<int64_t, KeyFrameT*> > live;
        for (size_t s = 0; s < mKFOfSlot.size(); ++s)
            if (mKFOfSlot[s]) live.push_back(std::make_pair(mOrderOfSlot[s], mKFOfSlot[s]));
        std::sort(live.begin(), live.end());
        slamit_kfdb_destroy(mDb);
        mDb = db; mSlots = slots; mMaxWords = words;
        mSlotOf.clear();
        mKFOfSlot.assign(slots, (KeyFrameT*)nullptr);
        mOrderOfSlot.assign(slots, -1);
        for (size_t k = 0; k < live.size(); ++k) {
            const int slot = put(live[k].second);
            if (slot < 0) return false;
            mSlotOf[live[k].second] = slot;
            mKFOfSlot[slot] = live[k].second;
            mOrderOfSlot[slot] = live[k].first;
        }
        return true;
    }

    static std::vector<KeyFrameT*> retain(const std::list<std::pair<float, KeyFrameT*> >& lAccScoreAndMatch, float minScoreToRetain) {
        std::set<KeyFrameT*> spAlreadyAddedKF;
        std::vector<KeyFrameT*> vpCandidates;
        vpCandidates.reserve(lAccScoreAndMatch.size());
        for (typename std::list<std::pair<float, KeyFrameT*> >::const_iterator it = lAccScoreAndMatch.begin(); it != lAccScoreAndMatch.end(); ++it)
            if (it->first > minScoreToRetain && !spAlreadyAddedKF.count(it->second)) {
                vpCandidates.push_back(it->second);
                spAlreadyAddedKF.insert(it->second);
            }
        return vpCandidates;
    }

    const ORBVocabulary* mpVoc;          // Associated vocabulary: its device is the database's
    slamit_kfdb* mDb;                    // created by the first add
    int mSlots, mMaxWords;
    std::map<KeyFrameT*, int> mSlotOf;
    std::vector<KeyFrameT*> mKFOfSlot;
    std::vector<int64_t> mOrderOfSlot;
    int64_t mNextOrder;
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2

#endif
