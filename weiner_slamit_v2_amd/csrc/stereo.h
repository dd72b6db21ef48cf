// stereo.h — one left keypoint of Frame::ComputeStereoMatches (ORB_SLAM2/src/Frame.cc:591-763): the row band of a right keypoint, the
// candidate gate, the coordinates at the keypoint's level, the two window tests, the parabola with disparity and depth, and the
// median threshold.  Plain C++ over IEEE +,-,*,/ with float and double exactly where the reference has them; it must be compiled
// with -ffp-contract=off.  stereo.hip runs it one wavefront per left keypoint; the CPU tests, the shim's test driver and
// tools/bench_stereo.py build the same text with g++ (stereo_frame_host below is the whole walk on one host core).
//
// The walk, line by line:
//   band            r = 2.0f * scale[octave]; rows (int)floorf(y - r) .. (int)ceilf(y + r), sums in float                    :610-612
//   row             (int)vL; no candidates in it, or uL + 3 < 0 in float: status 1                                          :634-643
//   gate            octave within +-1 of the left one, uR >= uL - maxD && uR <= uL + 3, maxD = mbf / mb in float            :619-621, :656-661
//   selection       least Hamming distance strictly below TH_HIGH = 100, the first (smallest right index) on ties: 2        :645-675
//   coordinates     roundf(x * inv_scale[octave]) as floats, for uL, vL and the chosen uR0                                  :679-682
//   right window    scaleduR0 < 0 || scaleduR0 + 11 >= cols, in float: status 3                                             :696-699
//   SAD             11 x 11 bytes minus the centre byte against 11 shifts of the right strip, each minus its centre: exact
//                   integers <= 121 * 510; the least one, the first on ties; at shift -5 or +5: status 4                    :701-718
//   parabola        deltaR = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2)) in float; < -1 or > 1: status 5 (a NaN passes)     :721-728
//   bestuR          scale[octave] * ((scaleduR0 + (float)bestinc) + deltaR) in float                                        :731
//   disparity       uL - bestuR; outside [0, maxD) (or NaN): status 6; == 0: 0.01f, bestuR = (float)((double)uL - 0.01)     :733-741
//   depth           mbf / disparity in float                                                                                :742
//   median          of the matched SADs sorted ascending, entry size / 2; thDist = 1.5f * 1.4f * median in float; an entry
//                   with (float)sad >= thDist: status 7, uRight = depth = -1                                                :749-762
//
// DEPARTURES, where the reference reads out of bounds, throws or has undefined behaviour (none of them is reachable from the
// extractor's own keypoints).  A LEFT keypoint gets STEREO_DEPARTURE (8), no match and uRight = depth = -1 when
//   - its octave is outside [0, nlevels) (mvInvScaleFactors[octave], mvImagePyramid[octave])                  tested on entry
//   - uL or vL is not finite, or (int)vL is outside [0, rows) (vRowIndices[vL])                               tested on entry
//   - the right keypoint the selection chose has an octave outside [0, nlevels) (possible at -1 and nlevels: the gate is +-1)
//   - the left 11 x 11 window leaves the left plane of its level (rowRange / colRange throw)                  tested before the :698 test
//   - the right 11 x 21 strip, columns scaleduR0 - 10 .. scaleduR0 + 10 and rows scaledvL +- 5, leaves the right plane: the
//     reference's test at :698 admits scaleduR0 in [0, 10), where its first colRange starts left of the image  tested after the :698 test
// A RIGHT keypoint's band is clamped to [0, rows); one with a coordinate that is not finite has no band and is never a candidate
// (its NaN fails the gate in the reference too); one whose octave is outside the table takes the band of the nearest level.
// An empty match list skips the median step (the reference indexes an empty vector).  Every test is written so that a NaN fails
// into the departure, and every float is compared against its bounds BEFORE it is converted to an integer.
//
// Outputs of a keypoint without a match: uRight = depth = -1; best_r and ham_dist are written once a right keypoint was chosen
// (statuses 0, 3 .. 7 and the last three departures), sad_dist once the shifts ran (0, 4 .. 7); -1 otherwise.
#ifndef SLAMIT_STEREO_H
#define SLAMIT_STEREO_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define STEREO_HD __host__ __device__ __forceinline__
#else
#define STEREO_HD static inline
#endif

#define STEREO_MAX_LEVELS 16       // = SLAMIT_MAX_LEVELS
#define STEREO_TH_HIGH 100         // ORBmatcher::TH_HIGH
#define STEREO_W 5                 // half size of the patch
#define STEREO_L 5                 // shifts -L .. +L
#define STEREO_SHIFTS (2 * STEREO_L + 1)
#define STEREO_PATCH (2 * STEREO_W + 1)

enum { STEREO_MATCHED = 0, STEREO_NO_CANDIDATE = 1, STEREO_NO_DESCRIPTOR = 2, STEREO_RIGHT_WINDOW = 3, STEREO_EDGE_SHIFT = 4,
       STEREO_DELTA = 5, STEREO_DISPARITY = 6, STEREO_MEDIAN = 7, STEREO_DEPARTURE = 8 };

STEREO_HD bool stereo_finite(float x) { return x >= -3.402823466e+38f && x <= 3.402823466e+38f; }

// Rows of the table a right keypoint enters, clamped to [0, rows): false = none.
STEREO_HD bool stereo_band(float y, float x, int octave, int nlevels, const float* scale, int rows, int& minr, int& maxr) {
    minr = 0; maxr = -1;
    if (!stereo_finite(y) || !stereo_finite(x) || rows < 1 || nlevels < 1) return false;
    const int o = octave < 0 ? 0 : (octave >= nlevels ? nlevels - 1 : octave);
    const float r = 2.0f * scale[o];
    const float hi = ceilf(y + r), lo = floorf(y - r);
    if (!(hi >= 0.0f) || !(lo <= (float)(rows - 1))) return false;       // a NaN (r not finite) has no band
    minr = lo < 0.0f ? 0 : (int)lo;
    maxr = hi > (float)(rows - 1) ? rows - 1 : (int)hi;
    return true;
}

// What the left keypoint brings to the walk: -1 = go on, else the status it ends with.
STEREO_HD int stereo_entry(float uL, float vL, int octave, int nlevels, int rows, float mb, float mbf, int& row, float& minU, float& maxU,
                           float& maxD) {
    row = 0;
    maxD = mbf / mb;
    minU = uL - maxD;
    maxU = uL - (-3.0f);
    if (octave < 0 || octave >= nlevels || octave >= STEREO_MAX_LEVELS) return STEREO_DEPARTURE;
    if (!stereo_finite(uL) || !stereo_finite(vL)) return STEREO_DEPARTURE;
    if (!(vL > -1.0f && vL < (float)rows)) return STEREO_DEPARTURE;
    row = (int)vL;
    if (row < 0 || row >= rows) return STEREO_DEPARTURE;
    if (maxU < 0.0f) return STEREO_NO_CANDIDATE;
    return -1;
}

STEREO_HD bool stereo_gate(int octR, int levelL, float uR, float minU, float maxU) {
    if (octR < levelL - 1 || octR > levelL + 1) return false;
    return uR >= minU && uR <= maxU;
}

STEREO_HD float stereo_scaled(float x, float inv_scale) { return roundf(x * inv_scale); }

// the 11 x 11 window round (su, sv) lies in a w x h plane
STEREO_HD bool stereo_left_window_inside(float su, float sv, int w, int h) {
    return su - (float)STEREO_W >= 0.0f && su + (float)STEREO_W <= (float)(w - 1) && sv - (float)STEREO_W >= 0.0f && sv + (float)STEREO_W <= (float)(h - 1);
}
// the reference's own test (:696-699): true = it goes on to the shifts
STEREO_HD bool stereo_right_window_ref(float suR0, int cols) {
    const float iniu = suR0 + (float)STEREO_L - (float)STEREO_W;
    const float endu = suR0 + (float)STEREO_L + (float)STEREO_W + 1.0f;
    return !(iniu < 0.0f || endu >= (float)cols);
}
// the strip every shift reads lies in the right plane
STEREO_HD bool stereo_right_strip_inside(float suR0, float sv, int w, int h) {
    const float k = (float)(STEREO_L + STEREO_W);
    return suR0 - k >= 0.0f && suR0 + k <= (float)(w - 1) && sv - (float)STEREO_W >= 0.0f && sv + (float)STEREO_W <= (float)(h - 1);
}

// the least of the 11 sums, the first on ties (:708 compares the float against the int: both exact)
STEREO_HD void stereo_best_shift(const int* d, int& bestinc, int& bestsad) {
    bestsad = d[0]; bestinc = -STEREO_L;
    for (int k = 1; k < STEREO_SHIFTS; ++k)
        if (d[k] < bestsad) { bestsad = d[k]; bestinc = k - STEREO_L; }
}

// from the sums to uRight and depth: 0, or the status 4 / 5 / 6 the keypoint ends with (uR = depth = -1 then)
STEREO_HD int stereo_subpixel(const int* d, int bestinc, float scale, float suR0, float uL, float maxD, float mbf, float& uR, float& depth) {
    uR = -1.0f; depth = -1.0f;
    if (bestinc == -STEREO_L || bestinc == STEREO_L) return STEREO_EDGE_SHIFT;
    const float dist1 = (float)d[STEREO_L + bestinc - 1], dist2 = (float)d[STEREO_L + bestinc], dist3 = (float)d[STEREO_L + bestinc + 1];
    const float deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2));
    if (deltaR < -1.0f || deltaR > 1.0f) return STEREO_DELTA;
    float bestuR = scale * (suR0 + (float)bestinc + deltaR);
    float disparity = uL - bestuR;
    if (!(disparity >= 0.0f && disparity < maxD)) return STEREO_DISPARITY;
    if (disparity <= 0.0f) {
        disparity = 0.01f;
        bestuR = (float)((double)uL - 0.01);
    }
    depth = mbf / disparity;
    uR = bestuR;
    return STEREO_MATCHED;
}

STEREO_HD float stereo_th_dist(int median) { return 1.5f * 1.4f * (float)median; }
STEREO_HD bool stereo_removed(int sad, float th_dist) { return !((float)sad < th_dist); }

// ---- the whole walk on the host ---------------------------------------------------------------------------------------------------
#if !defined(__HIPCC__)
#include <algorithm>
#include <vector>

struct StereoPlaneHost { const uint8_t* p; int w, h; long stride; };

struct StereoFrameHost {
    int nlevels;
    StereoPlaneHost left[STEREO_MAX_LEVELS], right[STEREO_MAX_LEVELS];
    int n_left, n_right;
    const float* xy_left; const int32_t* oct_left; const uint8_t* desc_left;      // n x 2, n, n x 32
    const float* xy_right; const int32_t* oct_right; const uint8_t* desc_right;
    float mb, mbf;
    const float* scale; const float* inv_scale;                                   // [STEREO_MAX_LEVELS]
    float* u_right; float* depth; uint8_t* status; int32_t* best_r; int32_t* ham_dist; int32_t* sad_dist;
};

static inline int stereo_hamming_host(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; k += 8) {
        unsigned long long x, y;
        __builtin_memcpy(&x, a + k, 8); __builtin_memcpy(&y, b + k, 8);
        d += __builtin_popcountll(x ^ y);
    }
    return d;
}

// -> the number of matches that survive the median filter
static inline int stereo_frame_host(const StereoFrameHost& F) {
    const int rows = F.nlevels >= 1 ? F.left[0].h : 0;
    // vRowIndices as one array: count, scan, fill in ascending right index (the order the reference's push_back gives a row)
    std::vector<int32_t> band(2 * (size_t)F.n_right + 2), row_start((size_t)(rows > 0 ? rows : 0) + 2, 0);
    for (int i = 0; i < F.n_right; ++i)
        if (stereo_band(F.xy_right[2 * i + 1], F.xy_right[2 * i], F.oct_right[i], F.nlevels, F.scale, rows, band[2 * i], band[2 * i + 1]))
            for (int y = band[2 * i]; y <= band[2 * i + 1]; ++y) ++row_start[y + 1];
    for (int y = 0; y < rows; ++y) row_start[y + 1] += row_start[y];
    std::vector<int32_t> row_items((size_t)row_start[rows > 0 ? rows : 0] + 1), fill(row_start.begin(), row_start.end());
    for (int i = 0; i < F.n_right; ++i)
        for (int y = band[2 * i]; y <= band[2 * i + 1]; ++y) row_items[fill[y]++] = i;
    for (int iL = 0; iL < F.n_left; ++iL) {
        F.u_right[iL] = -1.0f; F.depth[iL] = -1.0f; F.best_r[iL] = -1; F.ham_dist[iL] = -1; F.sad_dist[iL] = -1;
        const float uL = F.xy_left[2 * iL], vL = F.xy_left[2 * iL + 1];
        const int levelL = F.oct_left[iL];
        int row;
        float minU, maxU, maxD;
        int st = stereo_entry(uL, vL, levelL, F.nlevels, rows, F.mb, F.mbf, row, minU, maxU, maxD);
        if (st >= 0) { F.status[iL] = (uint8_t)st; continue; }
        if (row_start[row] == row_start[row + 1]) { F.status[iL] = STEREO_NO_CANDIDATE; continue; }
        int best = 256 + 1, bestR = -1;
        for (int c = row_start[row]; c < row_start[row + 1]; ++c) {
            const int iR = row_items[c];
            if (!stereo_gate(F.oct_right[iR], levelL, F.xy_right[2 * iR], minU, maxU)) continue;
            const int dist = stereo_hamming_host(F.desc_left + 32 * (long)iL, F.desc_right + 32 * (long)iR);
            if (dist < best) { best = dist; bestR = iR; }
        }
        if (best >= STEREO_TH_HIGH) { F.status[iL] = STEREO_NO_DESCRIPTOR; continue; }
        F.best_r[iL] = bestR; F.ham_dist[iL] = best;
        const int octR = F.oct_right[bestR];
        if (octR < 0 || octR >= F.nlevels) { F.status[iL] = STEREO_DEPARTURE; continue; }
        const float inv = F.inv_scale[levelL];
        const float su = stereo_scaled(uL, inv), sv = stereo_scaled(vL, inv), suR0 = stereo_scaled(F.xy_right[2 * bestR], inv);
        const StereoPlaneHost& PL = F.left[levelL];
        const StereoPlaneHost& PR = F.right[levelL];
        if (!stereo_left_window_inside(su, sv, PL.w, PL.h)) { F.status[iL] = STEREO_DEPARTURE; continue; }
        if (!stereo_right_window_ref(suR0, PR.w)) { F.status[iL] = STEREO_RIGHT_WINDOW; continue; }
        if (!stereo_right_strip_inside(suR0, sv, PR.w, PR.h)) { F.status[iL] = STEREO_DEPARTURE; continue; }
        const int x0 = (int)su - STEREO_W, y0 = (int)sv - STEREO_W, xr = (int)suR0 - STEREO_L - STEREO_W;
        int d[STEREO_SHIFTS];
        const int lc = PL.p[(long)(y0 + STEREO_W) * PL.stride + x0 + STEREO_W];
        for (int k = 0; k < STEREO_SHIFTS; ++k) {
            const int rc = PR.p[(long)(y0 + STEREO_W) * PR.stride + xr + k + STEREO_W];
            int s = 0;
            for (int i = 0; i < STEREO_PATCH; ++i) {
                const uint8_t* a = PL.p + (long)(y0 + i) * PL.stride + x0;
                const uint8_t* b = PR.p + (long)(y0 + i) * PR.stride + xr + k;
                for (int j = 0; j < STEREO_PATCH; ++j) {
                    const int v = ((int)a[j] - lc) - ((int)b[j] - rc);
                    s += v < 0 ? -v : v;
                }
            }
            d[k] = s;
        }
        int bestinc, bestsad;
        stereo_best_shift(d, bestinc, bestsad);
        F.sad_dist[iL] = bestsad;
        F.status[iL] = (uint8_t)stereo_subpixel(d, bestinc, F.scale[levelL], suR0, uL, maxD, F.mbf, F.u_right[iL], F.depth[iL]);
    }
    // the size / 2-th smallest SAD (the reference sorts pairs; the first member alone decides)
    std::vector<int32_t> sads;
    for (int iL = 0; iL < F.n_left; ++iL)
        if (F.status[iL] == STEREO_MATCHED) sads.push_back(F.sad_dist[iL]);
    if (sads.empty()) return 0;
    std::nth_element(sads.begin(), sads.begin() + sads.size() / 2, sads.end());
    const int median = sads[sads.size() / 2];
    const float th = stereo_th_dist(median);
    int kept = 0;
    for (int iL = 0; iL < F.n_left; ++iL) {
        if (F.status[iL] != STEREO_MATCHED) continue;
        if (stereo_removed(F.sad_dist[iL], th)) { F.status[iL] = STEREO_MEDIAN; F.u_right[iL] = -1.0f; F.depth[iL] = -1.0f; }
        else ++kept;
    }
    return kept;
}
#endif

#endif
