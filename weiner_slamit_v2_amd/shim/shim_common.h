// shim_common.h — what the class headers of the shim share: the per-thread LastStatus() cell with its report / refuse
// step, the RandomInt hook of the two RANSAC classes, the rotation-consistency histogram of the matcher's searches and the cv::Mat loads.  Header only; a program that
// never reports needs no library (the reporting functions are templates: uninstantiated, they reference no slamit_* symbol).
#ifndef SLAMIT_SHIM_COMMON_H
#define SLAMIT_SHIM_COMMON_H

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/slamit.h"

namespace ORB_SLAM2 {
namespace shim {

// The cell behind a class's LastStatus(): one per class (the tag) and per calling thread -- Tracking, LocalMapping and
// LoopClosing run concurrently, and all three use the matcher.
template <class Tag>
inline int& status() { static thread_local int s = SLAMIT_OK; return s; }

// A device call failed: "<where> failed (<rc>): <slamit_last_error()>" on stderr, rc in the cell.  Returns 0.
template <class Tag>
inline int report(const char* where, int rc) {
    status<Tag>() = rc;
    fprintf(stderr, "%s failed (%d): %s\n", where, rc, slamit_last_error());
    return 0;
}

// A call refused before the device: the caller's line on stderr, rc in the cell.  Returns 0.
template <class Tag>
inline int refuse(const char* why, int rc = SLAMIT_ERR_ARG) {
    status<Tag>() = rc;
    fprintf(stderr, "%s\n", why);
    return 0;
}

// DUtils::Random::RandomInt(min, max) over rand(); RandomInt() lets a caller (or a test) put its own source in.  One hook for the
// process: PnPsolver and Initializer both draw from it, as both draw from DUtils::Random in the reference.
inline int DefaultRandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}
typedef int (*RandomIntFn)(int, int);
inline RandomIntFn& RandomInt() { static RandomIntFn fn = DefaultRandomInt; return fn; }

// Loads of a CV_32F cv::Mat, and nothing else: out[stride * r + c] = m(r, c) of the top-left 3 x 3, out[stride * r] = m(r, col).
template <class MatT>
inline void load3x3(const MatT& m, float* out, int stride = 3) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[stride * r + c] = m.template at<float>(r, c);
}
template <class MatT>
inline void load3(const MatT& m, float* out, int col = 0, int stride = 1) {
    for (int r = 0; r < 3; ++r) out[stride * r] = m.template at<float>(r, col);
}

// Does the caller's type have a data member of this name?  C++11 member detection: has_member_<name><T>::value, and
// member_or_<name>(obj, fallback) reads it where it exists.  The stereo paths of the guided searches are chosen by it at compile time
// (mTrackProjXR on the map point, mbf on the frame or keyframe): a type without the member keeps the monocular code and its refusal
// of stereo frames, and never names the member.  LocalMapping::CreateNewMapPoints takes its stereo path for a keyframe type with all
// of mb, mbf, mvDepth and mvKeys.
template <bool B> struct bool_tag {};
#define SLAMIT_SHIM_HAS_MEMBER(name)                                                                                   \
    template <class T>                                                                                                 \
    struct has_member_##name {                                                                                         \
        template <class U> static char test(decltype(&U::name));                                                       \
        template <class U> static long test(...);                                                                      \
        static const bool value = sizeof(test<T>(0)) == sizeof(char);                                                  \
    };                                                                                                                 \
    template <class T> inline float member_or_##name(const T& o, float, bool_tag<true>) { return o.name; }             \
    template <class T> inline float member_or_##name(const T&, float fallback, bool_tag<false>) { return fallback; }   \
    template <class T> inline float member_or_##name(const T& o, float fallback) {                                     \
        return member_or_##name(o, fallback, bool_tag<has_member_##name<T>::value>());                                 \
    }
SLAMIT_SHIM_HAS_MEMBER(mTrackProjXR)
SLAMIT_SHIM_HAS_MEMBER(mbf)
SLAMIT_SHIM_HAS_MEMBER(mb)
SLAMIT_SHIM_HAS_MEMBER(mvDepth)
SLAMIT_SHIM_HAS_MEMBER(mvKeys)

// The rotation-consistency filter of the reference's searches (ORBmatcher.cc:240-250 with :271-289, and its copies): matches
// are binned by the difference of their keypoint angles, and those outside the three most populated bins are undone.
class RotationHistogram {
public:
    static const int LENGTH = 30;   // ORBmatcher::HISTO_LENGTH

    void add(float angle1, float angle2, int payload) {
        float rot = angle1 - angle2;
        if (rot < 0.0) rot += 360.0f;
        int bin = (int)roundf(rot * (1.0f / LENGTH));
        if (bin == LENGTH) bin = 0;
        if (bin >= 0 && bin < LENGTH) bins[bin].push_back(payload);
    }

    // fn(payload) for every entry outside the three maxima: bins in ascending order, entries in insertion order
    template <class Fn>
    void reject(Fn fn) const {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        ThreeMaxima(bins, LENGTH, ind1, ind2, ind3);
        for (int i = 0; i < LENGTH; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (size_t j = 0, jend = bins[i].size(); j < jend; j++) fn(bins[i][j]);
        }
    }

    // three most populated bins, the first on ties; the 2nd/3rd are dropped when below 10 % of the first (ORBmatcher.cc:1605-1646)
    static void ThreeMaxima(const std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3) {
        int top[3] = {0, 0, 0};
        int at[3] = {-1, -1, -1};
        for (int i = 0; i < L; ++i) {
            const int s = (int)histo[i].size();
            int pos = s > top[0] ? 0 : s > top[1] ? 1 : s > top[2] ? 2 : 3;
            for (int k = 2; k > pos; --k) { top[k] = top[k - 1]; at[k] = at[k - 1]; }
            if (pos < 3) { top[pos] = s; at[pos] = i; }
        }
        if (top[1] < 0.1f * (float)top[0]) { at[1] = -1; at[2] = -1; }
        else if (top[2] < 0.1f * (float)top[0]) at[2] = -1;
        ind1 = at[0]; ind2 = at[1]; ind3 = at[2];
    }

private:
    std::vector<int> bins[LENGTH];
};

}  // namespace shim
}  // namespace ORB_SLAM2

#endif
