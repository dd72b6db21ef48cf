// bow.hip — vocabulary-node search (include/slamit.h, slamit_bow_search, slamit_bow_search_stereo).
//
// Reference: ORB_SLAM2/src/ORBmatcher.cc:161-290 (SearchByBoW KeyFrame/Frame), :526-657 (SearchByBoW KeyFrame/KeyFrame),
// :659-826 (SearchForTriangulation), :141-158 (CheckDistEpipolarLine).
//
// One WAVEFRONT per group (= vocabulary node present on both sides).  A group's queries are walked in order, because in
// mode 0 an accepted query removes its candidate from the ones that follow; lanes hold the group's candidates (lane l:
// list positions l, l + 64, ...; a lane's matched positions are bits of one register).  "best / second best with strict
// '<', first one wins" is "the two smallest keys (distance << 16 | position)"; mode 1's "minimum distance, last one wins"
// is the smallest key (distance << 16 | 0xFFFF - position).  Wave-wide minima are DPP reductions (wave_ops.h).
// Float expressions are written exactly as the reference writes them; compiled with -ffp-contract=off.
//
// Stereo keyframes in mode 1 (:703-713, :734-753) are the STEREO instantiation of the search kernel: bStereo1 is
// one value per query (wave-uniform), bStereo2 one more 4-byte load per candidate lane; the epipole test runs only when neither
// is stereo, and only_stereo skips the queries and candidates that are not.  Without a stereo record the kernel is the one it was.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "wave_ops.h"

struct BowDev {
    int n_groups, n1;
    const int* q_ptr; const int* q_idx; const int* c_ptr; const int* c_idx;
    const uint8_t* desc1; const uint8_t* desc2; const uint8_t* valid1; const uint8_t* valid2;   // valid* may be null
    int mode, th, th_inclusive; float nnratio;
    float F[9]; float ex, ey;
    const float* kp1; const float* kp2; const int* oct2;
    float scale[16], sigma2[16];
    int* match12; int* dist12; int* nmatches;
    const float* ur1; const float* ur2; int only_stereo;   // the STEREO instantiation only
};

__global__ __launch_bounds__(256) void bow_init_kernel(BowDev D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *D.nmatches = 0;
    if (i < D.n1) { D.match12[i] = -1; D.dist12[i] = 256; }
}

template <bool STEREO>
__global__ __launch_bounds__(64) void bow_search_kernel(BowDev D) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int q0 = D.q_ptr[g], q1 = D.q_ptr[g + 1], c0 = D.c_ptr[g], nc = D.c_ptr[g + 1] - c0;
    if (nc <= 0 || q1 <= q0) return;
    const int nj = (nc + 63) >> 6;            // list positions per lane (<= 32: SLAMIT_BOW_MAX_GROUP)
    // positions this lane may not use: past the list, or not allowed by valid2
    unsigned blocked = 0;
    for (int j = 0; j < nj; ++j) {
        const int pos = lane + 64 * j;
        bool off = pos >= nc;
        if (!off && D.valid2) off = D.valid2[D.c_idx[c0 + pos]] == 0;
        blocked |= (unsigned)off << j;
    }
    int accepted = 0;
    for (int qi = q0; qi < q1; ++qi) {
        const int i1 = D.q_idx[qi];
        if (D.valid1 && !D.valid1[i1]) continue;   // wave-uniform
        bool stereo1 = false;
        if constexpr (STEREO) {
            stereo1 = D.ur1[i1] >= 0;               // :703 (wave-uniform)
            if (D.only_stereo && !stereo1) continue;   // :711-713
        }
        const uint4* dq = reinterpret_cast<const uint4*>(D.desc1 + 32 * (size_t)i1);
        const uint4 a0 = dq[0], a1 = dq[1];
        float la = 0.f, lb = 0.f, lc = 0.f;       // epipolar line of the query in image 2 (mode 1)
        if (D.mode == 1) {
            const float x1 = D.kp1[2 * i1], y1 = D.kp1[2 * i1 + 1];
            la = x1 * D.F[0] + y1 * D.F[3] + D.F[6];
            lb = x1 * D.F[1] + y1 * D.F[4] + D.F[7];
            lc = x1 * D.F[2] + y1 * D.F[5] + D.F[8];
        }
        unsigned kb = 0xFFFFFFFFu, ks = 0xFFFFFFFFu;
        for (int j = 0; j < nj; ++j) {
            if ((blocked >> j) & 1u) continue;
            const int pos = lane + 64 * j;
            const int i2 = D.c_idx[c0 + pos];
            const uint4* dt = reinterpret_cast<const uint4*>(D.desc2 + 32 * (size_t)i2);
            const uint4 t0 = dt[0], t1 = dt[1];
            const unsigned d = (unsigned)hamming256(a0, a1, t0, t1);
            if (D.mode == 0) {
                if (d >= 256u) continue;             // 'dist < bestDist1' can never hold against the initial 256
                const unsigned k = (d << 16) | (unsigned)pos;
                ks = min(ks, max(kb, k));
                kb = min(kb, k);
            } else {
                if ((int)d > D.th) continue;          // :731 (bestDist starts at TH_LOW; the running bound is the wave minimum)
                const float x2 = D.kp2[2 * i2], y2 = D.kp2[2 * i2 + 1];
                const int oc = D.oct2[i2] & 15;
                const float distex = D.ex - x2, distey = D.ey - y2;
                if constexpr (STEREO) {
                    const bool stereo2 = D.ur2[i2] >= 0;                               // :732
                    if (D.only_stereo && !stereo2) continue;                           // :734-736
                    if (!stereo1 && !stereo2 && distex * distex + distey * distey < 100 * D.scale[oc]) continue;   // :747-753
                } else {
                    if (distex * distex + distey * distey < 100 * D.scale[oc]) continue;   // :741
                }
                const float num = la * x2 + lb * y2 + lc;
                const float den = la * la + lb * lb;
                if (den == 0) continue;
                const float dsqr = num * num / den;
                if (!((double)dsqr < 3.84 * (double)D.sigma2[oc])) continue;           // :157 (double comparison)
                kb = min(kb, (d << 16) | (0xFFFFu - (unsigned)pos));
            }
        }
        const unsigned best = wave_min_u32(kb);
        if (best == 0xFFFFFFFFu) continue;            // no candidate at all: dist12 stays 256
        const int bd = (int)(best >> 16);
        if (D.mode == 0) {
            const unsigned second = wave_min_u32(kb == best ? ks : kb);   // keys are unique: one lane holds the best
            const int sd = second == 0xFFFFFFFFu ? 256 : (int)(second >> 16);
            const bool ok = (D.th_inclusive ? bd <= D.th : bd < D.th) && (float)bd < D.nnratio * (float)sd;
            const int pos = (int)(best & 0xFFFFu);
            if (ok && lane == (pos & 63)) blocked |= 1u << (pos >> 6);
            if (lane == 0) { D.dist12[i1] = bd; if (ok) D.match12[i1] = D.c_idx[c0 + pos]; }
            accepted += ok;
        } else {
            const int pos = 0xFFFF - (int)(best & 0xFFFFu);
            if (lane == 0) { D.dist12[i1] = bd; D.match12[i1] = D.c_idx[c0 + pos]; }
            ++accepted;
        }
    }
    if (lane == 0 && accepted) atomicAdd(D.nmatches, accepted);
}

extern "C" int slamit_bow_search_stereo(int device, const uint8_t* desc1, int32_t n1, const uint8_t* valid1, const uint8_t* desc2,
                                        int32_t n2, const uint8_t* valid2, const slamit_bow_groups* G, const slamit_bow_rule* rule,
                                        const slamit_bow_stereo* st, int32_t* match12, int32_t* dist12, int32_t* nmatches) {
    if (!G || !rule || !nmatches || n1 < 0 || n2 < 0 || G->n_groups < 0 || (rule->mode != 0 && rule->mode != 1))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search: bad argument");
    if (st && rule->mode != 1) return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search_stereo: a stereo record needs mode 1 (SearchByBoW has no stereo branch)");
    if (st && ((n1 > 0 && !st->ur1) || (n1 > 0 && n2 > 0 && !st->ur2))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search_stereo: null ur1 / ur2");
    *nmatches = 0;
    if (n1 == 0) return SLAMIT_OK;
    if (!match12 || !desc1 || (n2 && !desc2)) return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search: null array");
    for (int i = 0; i < n1; ++i) { match12[i] = -1; if (dist12) dist12[i] = 256; }
    const int ng = G->n_groups;
    if (ng == 0 || n2 == 0) return SLAMIT_OK;
    if (!G->q_ptr || !G->q_idx || !G->c_ptr || !G->c_idx) return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search: null group arrays");
    if (rule->mode == 1 && (!rule->kp1_xy || !rule->kp2_xy || !rule->kp2_octave))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search: mode 1 needs kp1_xy, kp2_xy, kp2_octave");
    const int nq = G->q_ptr[ng], ncand = G->c_ptr[ng];
    if (G->q_ptr[0] != 0 || G->c_ptr[0] != 0 || nq < 0 || ncand < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search: malformed group offsets");
    {   // a feature sits in one vocabulary node: an index may appear once per side (this is what makes groups independent)
        std::vector<uint8_t> seen1((size_t)n1, 0), seen2((size_t)n2, 0);
        for (int g = 0; g < ng; ++g) {
            if (G->q_ptr[g + 1] < G->q_ptr[g] || G->c_ptr[g + 1] < G->c_ptr[g]) return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search: malformed group offsets");
            if (G->c_ptr[g + 1] - G->c_ptr[g] > SLAMIT_BOW_MAX_GROUP) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_bow_search: a group holds more than SLAMIT_BOW_MAX_GROUP candidates");
        }
        for (int k = 0; k < nq; ++k) {
            const int i = G->q_idx[k];
            if (i < 0 || i >= n1 || seen1[i]) return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search: side-1 index out of range or repeated");
            seen1[i] = 1;
        }
        for (int k = 0; k < ncand; ++k) {
            const int i = G->c_idx[k];
            if (i < 0 || i >= n2 || seen2[i]) return slamit_fail(SLAMIT_ERR_ARG, "slamit_bow_search: side-2 index out of range or repeated");
            seen2[i] = 1;
        }
    }
    if (nq == 0 || ncand == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // one pinned staging block and one device slab per host thread, kept between calls (LocalMapping makes this call for
    // every neighbour keyframe of every new keyframe)
    const bool m1 = rule->mode == 1;
    const size_t N1 = n1, N2 = n2;
    StageLayout L;
    const StageSpan<uint8_t> d1 = L.take<uint8_t>(32 * N1), d2 = L.take<uint8_t>(32 * N2), v1 = L.take<uint8_t>(N1), v2 = L.take<uint8_t>(N2);
    const StageSpan<int> qp = L.take<int>((size_t)ng + 1), cp = L.take<int>((size_t)ng + 1), qi = L.take<int>(nq), ci = L.take<int>(ncand);
    const StageSpan<float> k1 = L.take<float>(m1 ? 2 * N1 : 0), k2 = L.take<float>(m1 ? 2 * N2 : 0);
    const StageSpan<int> oc = L.take<int>(m1 ? N2 : 0);
    const StageSpan<float> u1 = L.take<float>(st ? N1 : 0), u2 = L.take<float>(st ? N2 : 0);
    L.end_inputs();
    const StageSpan<int> om = L.take<int>(N1), od = L.take<int>(N1), nm = L.take<int>(1);
    L.end_outputs();
    static thread_local SlamitScratch S;
    HIP_TRY_AT("slamit_bow_search: scratch", slamit_stage_reserve(S, device, L));
    memcpy(d1.at(S.host), desc1, d1.bytes()); memcpy(d2.at(S.host), desc2, d2.bytes());
    if (valid1) memcpy(v1.at(S.host), valid1, v1.bytes());
    if (valid2) memcpy(v2.at(S.host), valid2, v2.bytes());
    memcpy(qp.at(S.host), G->q_ptr, qp.bytes()); memcpy(cp.at(S.host), G->c_ptr, cp.bytes());
    memcpy(qi.at(S.host), G->q_idx, qi.bytes()); memcpy(ci.at(S.host), G->c_idx, ci.bytes());
    if (m1) { memcpy(k1.at(S.host), rule->kp1_xy, k1.bytes()); memcpy(k2.at(S.host), rule->kp2_xy, k2.bytes()); memcpy(oc.at(S.host), rule->kp2_octave, oc.bytes()); }
    if (st) { memcpy(u1.at(S.host), st->ur1, u1.bytes()); memcpy(u2.at(S.host), st->ur2, u2.bytes()); }
    HIP_TRY_AT("slamit_bow_search", slamit_stage_upload(S, L));
    BowDev D;
    D.n_groups = ng; D.n1 = n1;
    D.q_ptr = qp.at(S.dev); D.q_idx = qi.at(S.dev); D.c_ptr = cp.at(S.dev); D.c_idx = ci.at(S.dev);
    D.desc1 = d1.at(S.dev); D.desc2 = d2.at(S.dev); D.valid1 = valid1 ? v1.at(S.dev) : nullptr; D.valid2 = valid2 ? v2.at(S.dev) : nullptr;
    D.mode = rule->mode; D.th = rule->th; D.th_inclusive = rule->th_inclusive; D.nnratio = rule->nnratio;
    memcpy(D.F, rule->F12, sizeof(D.F)); D.ex = rule->ex; D.ey = rule->ey;
    D.kp1 = k1.at(S.dev); D.kp2 = k2.at(S.dev); D.oct2 = oc.at(S.dev);
    memcpy(D.scale, rule->scale_factor, sizeof(D.scale)); memcpy(D.sigma2, rule->level_sigma2, sizeof(D.sigma2));
    D.match12 = om.at(S.dev); D.dist12 = od.at(S.dev); D.nmatches = nm.at(S.dev);
    hipLaunchKernelGGL(bow_init_kernel, dim3((n1 + 255) / 256), dim3(256), 0, S.st, D);
    D.ur1 = u1.at(S.dev); D.ur2 = u2.at(S.dev); D.only_stereo = st ? st->only_stereo : 0;
    if (st) hipLaunchKernelGGL(bow_search_kernel<true>, dim3(ng), dim3(64), 0, S.st, D);
    else hipLaunchKernelGGL(bow_search_kernel<false>, dim3(ng), dim3(64), 0, S.st, D);
    HIP_TRY_AT("slamit_bow_search", slamit_stage_download_and_wait(S, L));
    memcpy(match12, om.at(S.host), om.bytes());
    if (dist12) memcpy(dist12, od.at(S.host), od.bytes());
    *nmatches = *nm.at(S.host);
    return SLAMIT_OK;
}

extern "C" int slamit_bow_search(int device, const uint8_t* desc1, int32_t n1, const uint8_t* valid1, const uint8_t* desc2, int32_t n2,
                                 const uint8_t* valid2, const slamit_bow_groups* G, const slamit_bow_rule* rule, int32_t* match12,
                                 int32_t* dist12, int32_t* nmatches) {
    return slamit_bow_search_stereo(device, desc1, n1, valid1, desc2, n2, valid2, G, rule, nullptr, match12, dist12, nmatches);
}
