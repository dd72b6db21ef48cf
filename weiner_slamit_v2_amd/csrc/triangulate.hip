// triangulate.hip — the per-pair body of LocalMapping::CreateNewMapPoints on the GPU (include/slamit.h, slamit_triangulate*).
//
// Reference: ORB_SLAM2/src/LocalMapping.cc:323-503.  After SearchForTriangulation every matched pair of the (current keyframe,
// neighbour) pair is independent: ONE LANE takes one pair and runs triangulate.h on it -- rays and parallax, the 4x4 one-sided
// Jacobi with both matrices in registers, the depth, reprojection and scale gates.  The poses, intrinsics and camera centres of
// the problem are the same for every lane (scalar loads of the problem record); the level tables sit in the record and are
// indexed by the lane's octave.  No LDS, no atomics: the accepted pairs of a wavefront are a ballot's popcount, written to one
// slot per wavefront and summed on the host.  A batch of keyframe pairs is one launch (grid.y).
//
// Stereo keypoints (slamit_triangulate_stereo*) are the STEREO instantiation of the same kernel: six more coalesced
// per-pair arrays and three scalars of the record feed tri_pair_stereo, and a wavefront may hold triangulated, unprojected and
// skipped lanes side by side.  A batch without a stereo record launches the monocular instantiation, which is the kernel it was.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "triangulate.h"

static_assert((SLAMIT_MAX_LEVELS & (SLAMIT_MAX_LEVELS - 1)) == 0, "the kernel masks octaves with SLAMIT_MAX_LEVELS - 1");

struct TriProb {
    TriView c1, c2;
    float ratio_factor;
    int32_t n;
    float sf1[SLAMIT_MAX_LEVELS], s1[SLAMIT_MAX_LEVELS], sf2[SLAMIT_MAX_LEVELS], s2[SLAMIT_MAX_LEVELS];   // entries past n_levels are zero
    const SLAMIT_GLOBAL float* kp1; const SLAMIT_GLOBAL float* kp2;
    const SLAMIT_GLOBAL int32_t* o1; const SLAMIT_GLOBAL int32_t* o2;
    SLAMIT_GLOBAL uint8_t* status; SLAMIT_GLOBAL float* x3d; SLAMIT_GLOBAL int32_t* wave_counts;   // n, 3 n, (n + 63) / 64
    // the STEREO instantiation only; ur1 == null: this problem of the batch is monocular
    const SLAMIT_GLOBAL float* ur1; const SLAMIT_GLOBAL float* ur2; const SLAMIT_GLOBAL float* depth1; const SLAMIT_GLOBAL float* depth2;
    const SLAMIT_GLOBAL float* raw1; const SLAMIT_GLOBAL float* raw2;
    SLAMIT_GLOBAL uint8_t* source;   // n
    float mb1, mb2, bf;
};

// grid (ceil(max n / 256), problems), 256 threads: lane t of block b takes pair 256 b + t of problem blockIdx.y.  The host has
// checked every octave against [0, n_levels); the mask keeps the table index inside the record whatever it holds.
template <bool STEREO>
__global__ __launch_bounds__(256) void triangulate_kernel(const TriProb* __restrict__ probs) {
    const TriProb& P = probs[blockIdx.y];
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P.n) return;
    const float p1[2] = {P.kp1[2 * i], P.kp1[2 * i + 1]}, p2[2] = {P.kp2[2 * i], P.kp2[2 * i + 1]};
    const int o1 = P.o1[i] & (SLAMIT_MAX_LEVELS - 1), o2 = P.o2[i] & (SLAMIT_MAX_LEVELS - 1);
    float X[3];
    int st;
    if constexpr (STEREO) {
        int src;
        if (P.ur1) {   // uniform over the block
            const TriStereoPair s = {P.ur1[i], P.ur2[i], P.depth1[i], P.depth2[i], {P.raw1[2 * i], P.raw1[2 * i + 1]}, {P.raw2[2 * i], P.raw2[2 * i + 1]}};
            st = tri_pair_stereo(P.c1, P.c2, p1, p2, s, P.mb1, P.mb2, P.bf, P.s1[o1], P.s2[o2], P.sf1[o1], P.sf2[o2], P.ratio_factor, X, src);
        } else {
            st = tri_pair(P.c1, P.c2, p1, p2, P.s1[o1], P.s2[o2], P.sf1[o1], P.sf2[o2], P.ratio_factor, X);
            src = st == TRI_PARALLAX || st == TRI_W_ZERO ? TRI_SRC_NONE : TRI_SRC_TRIANGULATED;
        }
        P.source[i] = (uint8_t)src;
    } else {
        st = tri_pair(P.c1, P.c2, p1, p2, P.s1[o1], P.s2[o2], P.sf1[o1], P.sf2[o2], P.ratio_factor, X);
    }
    P.status[i] = (uint8_t)st;
    P.x3d[3 * (size_t)i] = X[0]; P.x3d[3 * (size_t)i + 1] = X[1]; P.x3d[3 * (size_t)i + 2] = X[2];
    const unsigned long long m = __ballot(st == TRI_OK);   // the lanes past n have left: they count as 0
    if ((threadIdx.x & 63) == 0) P.wave_counts[i >> 6] = __popcll(m);
}

extern "C" {

int slamit_triangulate_stereo_batch(int device, int nprob, const slamit_triangulate_problem* probs, const struct slamit_triangulate_stereo* const* stereo,
                                    slamit_triangulate_result* results, uint8_t* const* source) {
    const char* const where = "slamit_triangulate_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_triangulate_batch: bad argument");
    if (nprob == 0) return SLAMIT_OK;
    int max_n = 0;
    bool any_stereo = false;   // a problem with pairs and a stereo record: the STEREO instantiation runs the batch
    for (int f = 0; f < nprob; ++f) {
        const slamit_triangulate_problem& P = probs[f];
        if (P.n < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_triangulate_batch: negative count");
        if (P.n > SLAMIT_TRIANGULATE_MAX_N) return slamit_fail(SLAMIT_ERR_ARG, "slamit_triangulate_batch: more than SLAMIT_TRIANGULATE_MAX_N pairs");
        if (P.n == 0) continue;   // nothing to triangulate, nothing read
        if (P.n_levels < 1 || P.n_levels > SLAMIT_MAX_LEVELS) return slamit_fail(SLAMIT_ERR_ARG, "slamit_triangulate_batch: n_levels outside [1, SLAMIT_MAX_LEVELS]");
        if (!P.kp1_xy || !P.kp2_xy || !P.octave1 || !P.octave2 || !P.scale_factors1 || !P.level_sigma2_1 || !P.scale_factors2 || !P.level_sigma2_2 ||
            !results[f].status || !results[f].x3d)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_triangulate_batch: null array");
        for (int k = 0; k < P.n; ++k)
            if (P.octave1[k] < 0 || P.octave1[k] >= P.n_levels || P.octave2[k] < 0 || P.octave2[k] >= P.n_levels)
                return slamit_fail(SLAMIT_ERR_ARG, "slamit_triangulate_batch: octave outside [0, n_levels)");
        if (stereo && stereo[f]) {
            const struct slamit_triangulate_stereo& T = *stereo[f];
            if (!T.ur1 || !T.ur2 || !T.depth1 || !T.depth2 || !T.raw1_xy || !T.raw2_xy)
                return slamit_fail(SLAMIT_ERR_ARG, "slamit_triangulate_stereo_batch: null array in a stereo record");
            any_stereo = true;
        }
        max_n = std::max(max_n, (int)P.n);
    }
    for (int f = 0; f < nprob; ++f) results[f].n_accepted = 0;
    if (max_n == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // [records | per problem: kp1 kp2 octave1 octave2, with a stereo record its six arrays] go up; [per problem: status x3d wave counts, in
    // a stereo launch the source the caller asked for] come down; a source nobody asked for stays on the device
    std::vector<StageView<int32_t>> waves(nprob);
    static thread_local SlamitScratch S;
    const int rc = slamit_staged_batch<TriProb>(
        where, S, device, nprob,
        [&](StageBinder& b, int f, TriProb& Q) {
            const slamit_triangulate_problem& P = probs[f];
            const size_t n = (size_t)P.n;
            Q.n = P.n;
            if (n) {
                memcpy(Q.c1.T, P.Tcw1, sizeof(Q.c1.T)); memcpy(Q.c2.T, P.Tcw2, sizeof(Q.c2.T));
                Q.c1.fx = P.intr1[0]; Q.c1.fy = P.intr1[1]; Q.c1.cx = P.intr1[2]; Q.c1.cy = P.intr1[3]; Q.c1.invfx = P.intr1[4]; Q.c1.invfy = P.intr1[5];
                Q.c2.fx = P.intr2[0]; Q.c2.fy = P.intr2[1]; Q.c2.cx = P.intr2[2]; Q.c2.cy = P.intr2[3]; Q.c2.invfx = P.intr2[4]; Q.c2.invfy = P.intr2[5];
                tri_centre(Q.c1); tri_centre(Q.c2);
                Q.ratio_factor = P.ratio_factor;
                memcpy(Q.sf1, P.scale_factors1, sizeof(float) * P.n_levels); memcpy(Q.s1, P.level_sigma2_1, sizeof(float) * P.n_levels);
                memcpy(Q.sf2, P.scale_factors2, sizeof(float) * P.n_levels); memcpy(Q.s2, P.level_sigma2_2, sizeof(float) * P.n_levels);
            }
            Q.kp1 = slamit_global(b.in(P.kp1_xy, 2 * n)); Q.kp2 = slamit_global(b.in(P.kp2_xy, 2 * n));
            Q.o1 = slamit_global(b.in(P.octave1, n)); Q.o2 = slamit_global(b.in(P.octave2, n));
            if (n && stereo && stereo[f]) {
                const struct slamit_triangulate_stereo& T = *stereo[f];
                Q.mb1 = T.mb1; Q.mb2 = T.mb2; Q.bf = T.bf;
                Q.ur1 = slamit_global(b.in(T.ur1, n)); Q.ur2 = slamit_global(b.in(T.ur2, n));
                Q.depth1 = slamit_global(b.in(T.depth1, n)); Q.depth2 = slamit_global(b.in(T.depth2, n));
                Q.raw1 = slamit_global(b.in(T.raw1_xy, 2 * n)); Q.raw2 = slamit_global(b.in(T.raw2_xy, 2 * n));
            }
            Q.status = slamit_global(b.out(results[f].status, n)); Q.x3d = slamit_global(b.out(results[f].x3d, 3 * n));
            Q.wave_counts = slamit_global(b.out_view((n + 63) / 64, &waves[f]));
            if (any_stereo) Q.source = slamit_global(source && source[f] ? b.out(source[f], n) : b.scratch<uint8_t>(n));
        },
        [&](const TriProb* d_recs) {
            if (any_stereo) hipLaunchKernelGGL(triangulate_kernel<true>, dim3((max_n + 255) / 256, nprob), dim3(256), 0, S.st, d_recs);
            else hipLaunchKernelGGL(triangulate_kernel<false>, dim3((max_n + 255) / 256, nprob), dim3(256), 0, S.st, d_recs);
            return hipGetLastError();
        });
    if (rc != SLAMIT_OK) return rc;
    for (int f = 0; f < nprob; ++f) {
        results[f].n_accepted = stage_sum(waves[f].data, waves[f].count);
        if (!any_stereo && source && source[f])   // a monocular launch writes no source: it follows from the status
            for (int k = 0; k < probs[f].n; ++k) source[f][k] = results[f].status[k] == TRI_PARALLAX || results[f].status[k] == TRI_W_ZERO ? TRI_SRC_NONE : TRI_SRC_TRIANGULATED;
    }
    return SLAMIT_OK;
}

int slamit_triangulate_stereo(int device, const slamit_triangulate_problem* prob, const struct slamit_triangulate_stereo* stereo,
                              slamit_triangulate_result* res, uint8_t* source) {
    return slamit_triangulate_stereo_batch(device, 1, prob, &stereo, res, &source);
}

int slamit_triangulate_batch(int device, int nprob, const slamit_triangulate_problem* probs, slamit_triangulate_result* results) {
    return slamit_triangulate_stereo_batch(device, nprob, probs, nullptr, results, nullptr);
}

int slamit_triangulate(int device, const slamit_triangulate_problem* prob, slamit_triangulate_result* res) {
    return slamit_triangulate_stereo_batch(device, 1, prob, nullptr, res, nullptr);
}

}  // extern "C"
