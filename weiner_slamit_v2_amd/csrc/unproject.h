// unproject.h — what a stereo or RGB-D frame does between its depths and its new map points: Frame::ComputeStereoFromRGBD
// (ORB_SLAM2/src/Frame.cc:766-787), Frame::UnprojectStereo (:789-803), what the two MapPoint constructors and UpdateNormalAndDepth
// store for a point with one observer (src/MapPoint.cc:52-77, :336-377), and the closest-point walk of Tracking::UpdateLastFrame
// (src/Tracking.cc:1039-1091), CreateNewKeyFrame (:1334-1396) and StereoInitialization (:712-727).  Plain C++ over IEEE +,-,*,/ and
// sqrt, float and double exactly where the reference has them; it must be compiled with -ffp-contract=off.  unproject.hip runs it
// one lane per keypoint; the CPU test of the restatement, the shim's test driver and tools/bench_unproject.py build the same text
// with g++ for the host.
//
// The arithmetic, line by line (where the reference goes through OpenCV the order below is the statement of it,
// PARITY UNPINNED as in frustum.h and triangulate.h):
//   row, column       (int)kp.pt.y, (int)kp.pt.x of the RAW keypoint: Mat::at<float>(float, float) converts     Frame.cc:776-779
//                     its arguments to int, which truncates toward zero
//   d                 imDepth.at<float>(row, column) of the plane Tracking::GrabImageRGBD converted:             Tracking.cc:267-268
//                     convertTo(CV_32F, mDepthMapFactor) ALWAYS runs (the `if` in front of it ends in `;`), so
//                     d = (float)raw * factor in float for a uint16 AND for a float plane.  PARITY UNPINNED:
//                     cvtScale's own evaluation (a float product, no double intermediate) is read, not run
//   d > 0             a NaN and -0 are not; mvDepth = d                                                          Frame.cc:781-783
//   mvuRight          kpU.pt.x - (mbf / d) in float, two roundings, from the UNDISTORTED keypoint                :784
//   x, y              ((u - cx) * z) * invfx, ((v - cy) * z) * invfy in float from the undistorted keypoint      :796-797
//   Pos               mRwc * x3Dc + mOw: per row ((r0 x + r1 y) + r2 z) in float, then                           :799, cv::gemm
//                     (float)((double)row + (double)Ow): fru_gemm_row3 of frustum.h
//   PC = Pos - Ow     float                                                                                      MapPoint.cc:60, :63, :360, :365
//   norm              sqrt(double sum of double squares, in order): cv::norm returns double                      :61, :64, :361, :366
//   dist              (float)norm                                                                                :64, :366
//   normal            PC * (float)(1.0 / norm): Mat / double is a convertTo with scale 1./s                      :61, :361
//   max_dist          dist * scale_factors[octave] in float                                                      :69, :373
//   min_dist          max_dist / scale_factors[n_levels - 1] in float                                            :70, :374
//
// TWO CONSTRUCTORS, ONE DIFFERENCE.  MapPoint(Pos, pMap, pFrame, idxF) (UpdateLastFrame) stores PC / norm as it is.
// MapPoint(Pos, pKF, pMap) followed by UpdateNormalAndDepth with the single observer (CreateNewKeyFrame, StereoInitialization)
// stores (zeros + PC / norm) / n with n = 1 (:354-375): 0.0f + x and then x * (float)(1.0 / 1) in float.  Both steps are exact for
// every x but one: -0 becomes +0.  So the forms differ only in the sign of a zero normal component: a negative PC component whose
// product with 1 / norm underflows (PC itself is never -0, because Pos = fl(row + Ow) is -0 only for Ow = -0).  The call says which
// form it wants (ctor: UNP_CTOR_FRAME / UNP_CTOR_KEYFRAME).  Positions and distances are
// one form.  PARITY UNPINNED: that cv::add and the scaled convertTo do round -0 this way is read, not run.
//
// THE WALK.  Candidates are the keypoints with z > 0: NaN is none, +inf is one, a denormal is one whatever the float mode, because
// the test is made on the bits (unp_candidate).  They are sorted as pair<float, int>: by depth, by index on equal depths.  A
// positive float's bit pattern is monotone as an unsigned integer, so the 64-bit key (bits << 32) | index orders exactly as the
// pair does and no two keys are equal: a keypoint's walk position is a pure function of the input.  The loop visits position j,
// counts it whether it creates a point or not, and leaves after the first j with depth_j > th_depth && j + 1 > min_points.
// CLOSED FORM: with M candidates of which c have !(z > th_depth), the loop visits the first
//     n_visited = min(M, max(c, min_points) + 1)
// positions (the c close ones sort first; position j is the first far one past min_points when j >= c and j >= min_points, so the
// last visited j is max(c, min_points), if there is one).  One far point beyond the close set is always taken when there is one:
// the reference's behaviour, kept.  tests/test_unproject_ref.py holds the literal loop against this form on every fixture and on
// random cases.  Mode ALL (StereoInitialization) visits every candidate in index order, without a cut and without looking at the
// frame's map points.
//
// ONE STATED DEPARTURE.  The reference reads mvScaleFactors[octave] unchecked.  Here a visited keypoint that needs a point but whose
// octave lies outside [0, n_levels) is UNP_OCTAVE (4): it counts in the walk like any other and nothing is created for it.  In
// ComputeStereoFromRGBD a truncated row or column outside the plane (or a coordinate that is not finite) is RGBD_OUTSIDE (2) with
// uR = depth = -1, where the reference reads out of bounds.
#ifndef SLAMIT_UNPROJECT_H
#define SLAMIT_UNPROJECT_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define UNP_HD __host__ __device__ __forceinline__
#else
#define UNP_HD static inline
#endif

#define UNP_MAX_LEVELS 16          // = SLAMIT_MAX_LEVELS; a power of two: the table index is masked with UNP_MAX_LEVELS - 1

enum { UNP_NO_DEPTH = 0, UNP_BEYOND = 1, UNP_TRACKED = 2, UNP_CREATED = 3, UNP_OCTAVE = 4 };
enum { UNP_MODE_CLOSEST = 0, UNP_MODE_ALL = 1 };
enum { UNP_CTOR_FRAME = 0, UNP_CTOR_KEYFRAME = 1 };
enum { RGBD_NONE = 0, RGBD_DEPTH = 1, RGBD_OUTSIDE = 2 };
enum { UNP_DEPTH_F32 = 0, UNP_DEPTH_U16 = 1 };

// What the frame contributes (fx .. invfy, mRwc, mOw, mvScaleFactors) and what the caller passes (mThDepth, the 100 of both
// walks, the mode, the constructor).  Layout of slamit_unproject_frame.
struct UnprojectFrame {
    float fx, fy, cx, cy, invfx, invfy;
    float Rwc[9], Ow[3];
    float th_depth;
    int min_points, mode, ctor, n_levels;
    float scale_factors[UNP_MAX_LEVELS];
};

struct UnprojectPoint {
    float pos[3], normal[3], max_dist, min_dist;
};

UNP_HD unsigned unp_bits(float z) {
    unsigned b;
    __builtin_memcpy(&b, &z, 4);
    return b;
}

// z > 0 on the bits: sign clear, not zero, not a NaN; +inf and the denormals are candidates
UNP_HD bool unp_candidate(float z) {
    const unsigned b = unp_bits(z);
    return b != 0u && b <= 0x7f800000u;
}

// z > th for a candidate z, on the bits where th is a positive number (so that a denormal z compares as its value in any float
// mode); a th that is negative or -0 lies below every candidate, +0 below every candidate too, a NaN th is above none
UNP_HD bool unp_far(float z, float th) {
    const unsigned t = unp_bits(th);
    if (t > 0x7f800000u) return (t & 0x80000000u) != 0u && t <= 0xff800000u;   // negative (or -0, -inf): far; NaN: not
    return unp_bits(z) > t;
}
// z < th for a candidate z (NeedNewKeyFrame's strict test)
UNP_HD bool unp_below(float z, float th) {
    const unsigned t = unp_bits(th);
    if (t > 0x7f800000u) return false;   // negative, -0 or NaN: no candidate lies below it
    return unp_bits(z) < t;
}

UNP_HD unsigned long long unp_key(float z, int i) { return ((unsigned long long)unp_bits(z) << 32) | (unsigned)i; }

// positions the walk visits: M candidates, c of them not far
UNP_HD int unp_n_visited(int M, int c, int min_points, int mode) {
    if (mode == UNP_MODE_ALL) return M;
    const long long cut = (long long)(c > min_points ? c : min_points) + 1;
    return (long long)M < cut ? M : (int)cut;
}

// cv::norm of a 3 x 1 float Mat: the square root of the double sum of double squares, in order (MapPoint.cc:61, :64, :361, :366)
UNP_HD double unp_norm3(const float v[3]) { return sqrt(((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1]) + (double)v[2] * (double)v[2]); }
// Mat / s: a convertTo with scale 1. / s, so every element is multiplied by this float (:61, :361, :375)
UNP_HD float unp_mat_div(double s) { return (float)(1.0 / s); }

// Frame::UnprojectStereo and what the new point's constructor stores; false = the octave lies outside the table (UNP_OCTAVE)
UNP_HD bool unp_point(const UnprojectFrame& F, float u, float v, float z, int octave, UnprojectPoint& o) {
    const float x = (u - F.cx) * z * F.invfx;
    const float y = (v - F.cy) * z * F.invfy;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float t0 = F.Rwc[3 * r] * x + F.Rwc[3 * r + 1] * y + F.Rwc[3 * r + 2] * z;
        o.pos[r] = (float)((double)t0 + (double)F.Ow[r]);
    }
    const float PC[3] = {o.pos[0] - F.Ow[0], o.pos[1] - F.Ow[1], o.pos[2] - F.Ow[2]};
    const double norm = unp_norm3(PC);
    const float dist = (float)norm;
    const float inv = unp_mat_div(norm);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float nr = PC[r] * inv;
        if (F.ctor == UNP_CTOR_KEYFRAME) nr = (0.0f + nr) * 1.0f;
        o.normal[r] = nr;
    }
    o.max_dist = 0.f; o.min_dist = 0.f;
    if (octave < 0 || octave >= F.n_levels || octave >= UNP_MAX_LEVELS) return false;
    o.max_dist = dist * F.scale_factors[octave & (UNP_MAX_LEVELS - 1)];
    o.min_dist = o.max_dist / F.scale_factors[(F.n_levels - 1) & (UNP_MAX_LEVELS - 1)];
    return true;
}

// One keypoint of Frame::ComputeStereoFromRGBD.  `data` is the plane's first byte, `pitch` the bytes between rows.
UNP_HD int unp_rgbd(const void* data, size_t pitch, int width, int height, int type, float factor, float mbf, float raw_x, float raw_y,
                    float un_x, float& u_right, float& depth) {
    u_right = -1.0f; depth = -1.0f;
    // the conversion to int is made only on a value an int holds; (-1, 0) truncates to 0
    if (!(raw_x > -1.0f && raw_x < 2147483648.0f && raw_y > -1.0f && raw_y < 2147483648.0f)) return RGBD_OUTSIDE;
    const int col = (int)raw_x, row = (int)raw_y;
    if (col >= width || row >= height) return RGBD_OUTSIDE;
    const unsigned char* p = (const unsigned char*)data + (size_t)row * pitch;
    float raw;
    if (type == UNP_DEPTH_U16) raw = (float)((const unsigned short*)p)[col];
    else raw = ((const float*)p)[col];
    const float d = raw * factor;
    if (!(d > 0.0f)) return RGBD_NONE;
    depth = d;
    u_right = un_x - mbf / d;
    return RGBD_DEPTH;
}

#if !defined(__HIPCC__)
// The whole walk of one frame on the host, through the functions above: what unproject.hip's workgroup computes, for the CPU test of
// the restatement, the shim's test driver and the one-core baseline of tools/bench_unproject.py.  kp is the keypoints' x, y
// (float) and octave (int) at a stride of kp_stride bytes (28 for slamit_kp / cv::KeyPoint); tracked may be null in mode ALL.
// pos / normal are n x 3; counts: n_candidates, n_close, n_visited, n_created, n_total, n_map.
#include <algorithm>
#include <vector>
static inline void unp_walk_host(const UnprojectFrame& F, int n, const unsigned char* kp, size_t kp_stride, size_t octave_offset, const float* depth,
                                 const unsigned char* tracked, unsigned char* status, int* order, float* pos, float* normal, float* max_dist,
                                 float* min_dist, int counts[6]) {
    std::vector<unsigned long long> keys;
    keys.reserve((size_t)n);
    int c = 0, n_total = 0, n_map = 0, n_created = 0;
    for (int i = 0; i < n; ++i) {
        status[i] = UNP_NO_DEPTH; order[i] = -1;
        for (int r = 0; r < 3; ++r) { pos[3 * (size_t)i + r] = 0.f; normal[3 * (size_t)i + r] = 0.f; }
        max_dist[i] = 0.f; min_dist[i] = 0.f;
        if (!unp_candidate(depth[i])) continue;
        keys.push_back(unp_key(depth[i], i));
        if (!unp_far(depth[i], F.th_depth)) ++c;
        if (unp_below(depth[i], F.th_depth)) { ++n_total; if (tracked && tracked[i]) ++n_map; }
    }
    const int M = (int)keys.size();
    if (F.mode != UNP_MODE_ALL) std::sort(keys.begin(), keys.end());
    const int n_visit = unp_n_visited(M, c, F.min_points, F.mode);
    for (int j = 0; j < M; ++j) {
        const int i = (int)(unsigned)(keys[(size_t)j] & 0xffffffffull);
        if (j >= n_visit) { status[i] = UNP_BEYOND; continue; }
        order[j] = i;
        if (F.mode != UNP_MODE_ALL && tracked && tracked[i]) { status[i] = UNP_TRACKED; continue; }
        const unsigned char* k = kp + (size_t)i * kp_stride;
        float u, v;
        int octave;
        __builtin_memcpy(&u, k, 4); __builtin_memcpy(&v, k + 4, 4); __builtin_memcpy(&octave, k + octave_offset, 4);
        UnprojectPoint o;
        if (!unp_point(F, u, v, depth[i], octave, o)) { status[i] = UNP_OCTAVE; continue; }
        status[i] = UNP_CREATED; ++n_created;
        for (int r = 0; r < 3; ++r) { pos[3 * (size_t)i + r] = o.pos[r]; normal[3 * (size_t)i + r] = o.normal[r]; }
        max_dist[i] = o.max_dist; min_dist[i] = o.min_dist;
    }
    counts[0] = M; counts[1] = c; counts[2] = n_visit; counts[3] = n_created; counts[4] = n_total; counts[5] = n_map;
}
#endif

#endif
