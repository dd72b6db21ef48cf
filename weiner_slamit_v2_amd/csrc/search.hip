// search.hip — guided search: Frame::GetFeaturesInArea + Hamming best/second + greedy take
// (include/slamit.h, slamit_guided_search).
//
// Reference: ORB_SLAM2/src/ORBmatcher.cc:47-131 and :1332-1474 (the per-query loop bodies),
// ORB_SLAM2/src/Frame.cc:336-357, 447-517 (grid assignment and window query).
//
// Two steps:
//   search_candidates_kernel  one wavefront per query, all queries in parallel: every keypoint is tested
//       against the window exactly as GetFeaturesInArea does (grid cell range from the reference's float
//       expressions, level range, |dx| < r && |dy| < r); hits are appended to the query's candidate list
//       as one u64 key  (distance << 32) | (cell_x * 48 + cell_y) << 17 | keypoint << 4 | octave  — sorting by
//       that key IS the reference's scan order (cells x-major, then y, then insertion = keypoint index) with the
//       Hamming distance in front, and "best / second best with strict <" equals "two smallest keys".
//   search_resolve_walk       one wavefront walks the queries IN ORDER (the reference commits the winning
//       keypoint before it looks at the next map point): the tentative pair stands unless the per-keypoint state
//       excludes one of the two, otherwise lanes re-scan the candidates and two wave-wide min-reductions (wave_ops.h)
//       give best and second; then the acceptance rule runs and the state is updated in LDS.  The walk is written once;
//       what the state is, whom it excludes and how a query is accepted comes in as a model, the way lm_block.h takes
//       its problems: TakenBits (search_resolve_kernel: SearchByProjection / Fuse) and MatchedDist
//       (search_resolve_init_kernel: SearchForInitialization).
// Float expressions are written exactly as the reference writes them; compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "wave_ops.h"

#define GRID_COLS 64   // FRAME_GRID_COLS, include/Frame.h:41
#define GRID_ROWS 48   // FRAME_GRID_ROWS, include/Frame.h:40

// One frame of a batch: blockIdx.y (candidates) / blockIdx.x (resolve) selects it; all arrays are strided per frame.
struct SearchDev {
    int nframes, kp_cap, q_cap, cand_cap;
    const int* n_arr; int n_fixed;           // keypoints per frame
    const int* m_arr; int m_fixed;           // queries per frame
    const uint8_t* kp; int kp_rec;           // keypoint records: float x, y at byte 0 / 4, int octave at kp_oct_off; kp_rec bytes each
    int kp_oct_off;
    const uint8_t* kp_desc; const uint8_t* kp_taken;
    float min_x, min_y, inv_w, inv_h;
    const float* uvr; const int* lmin; const int* lmax; const uint8_t* qdesc; const uint8_t* valid; const uint8_t* takes;
    unsigned long long* cand;   // [nframes][q_cap][cand_cap]
    int* cand_n;                // [nframes][q_cap] (may exceed cand_cap: overflow)
    unsigned long long* tent;   // [nframes][q_cap][2]: the two smallest keys among the candidates not taken ON ENTRY
    int th_dist, use_ratio; float nnratio;
    float chi2_gate; float inv_sigma2[16];   // Fuse's reprojection gate (chi2_gate <= 0: off)
    int mode;                                 // 0 taken flags, 1 SearchForInitialization's matched-distance state
    int* match_kp; int* out4;   // [nframes][q_cap], [nframes][q_cap][4] (best_dist, best_level, second_dist, second_level) or null
    int* nmatches;              // [nframes]
    // The right-image gate of the three stereo drivers.  Read only by the kernels instantiated for er_mode != 0.
    const float* kp_ur;         // [nframes][kp_cap]: mvuRight of the searched frame
    const float* q_ur; int q_ur_stride;   // query q of frame f: q_ur[(f * q_cap + q) * q_ur_stride]
    int er_mode;                // SLAMIT_SEARCH_ER_*: uniform per launch, and the kernels' template argument
    float chi2_gate_stereo;     // CHI2: the three-term gate (7.8)
};

// key = distance << 32 | cell << 17 | keypoint << 4 | octave: ordered by (distance, cell, keypoint) = the reference's
// scan order; the octave rides along in the low bits so the resolve step never goes back to the keypoint table
#define KEY_KP(k) ((int)(((k) >> 4) & 8191))
#define KEY_OCT(k) ((int)((k) & 15))
#define KEY_NONE (~0ull)

// A query's search window (Frame::GetFeaturesInArea, Frame.cc:452-466) and descriptor; ok = the window meets the grid.
struct QueryWin {
    float x, y, r, ur;   // ur: the query's right-image column, loaded only when the launch has a gate
    int nMinCellX, nMaxCellX, nMinCellY, nMaxCellY, minLevel, maxLevel;
    uint4 a0, a1;
};
template <int ER>
__device__ __forceinline__ bool query_window(const SearchDev& D, size_t qo, QueryWin& W) {
    W.x = D.uvr[3 * qo]; W.y = D.uvr[3 * qo + 1]; W.r = D.uvr[3 * qo + 2];
    W.ur = ER != SLAMIT_SEARCH_ER_NONE ? D.q_ur[qo * (size_t)D.q_ur_stride] : 0.f;
    W.nMinCellX = max(0, (int)floorf((W.x - D.min_x - W.r) * D.inv_w));
    if (W.nMinCellX >= GRID_COLS) return false;
    W.nMaxCellX = min(GRID_COLS - 1, (int)ceilf((W.x - D.min_x + W.r) * D.inv_w));
    if (W.nMaxCellX < 0) return false;
    W.nMinCellY = max(0, (int)floorf((W.y - D.min_y - W.r) * D.inv_h));
    if (W.nMinCellY >= GRID_ROWS) return false;
    W.nMaxCellY = min(GRID_ROWS - 1, (int)ceilf((W.y - D.min_y + W.r) * D.inv_h));
    if (W.nMaxCellY < 0) return false;
    W.minLevel = D.lmin[qo]; W.maxLevel = D.lmax[qo];
    const uint4* Q = reinterpret_cast<const uint4*>(D.qdesc + 32 * qo);
    W.a0 = Q[0]; W.a1 = Q[1];
    return true;
}
// keypoint i against the window: is it a candidate, and its key (distance, cell, keypoint, octave).  ER is the launch's er_mode: the
// monocular instantiation (ER = 0) is the code as it stood, without a load or a branch for the gate.  KUR: the frame's mvuRight.
//   RADIUS (ORBmatcher.cc:93-98, :1411-1417)  a keypoint with uR > 0 is skipped when fabs(q_ur - uR) > r; a NaN passes, 0 is monocular
//   CHI2   (ORBmatcher.cc:918-942)            a keypoint with uR >= 0 takes the three-term e2 against chi2_gate_stereo; 0 is stereo
template <int ER>
__device__ __forceinline__ bool window_key(const SearchDev& D, const QueryWin& W, const uint8_t* KP, const uint8_t* KD, const float* KUR, int i,
                                           unsigned long long& key) {
    const uint8_t* rec = KP + (size_t)i * D.kp_rec;
    const float px = *reinterpret_cast<const float*>(rec), py = *reinterpret_cast<const float*>(rec + 4);
    // Frame::PosInGrid, Frame.cc:505-517 (round = half away from zero)
    const int posX = (int)roundf((px - D.min_x) * D.inv_w), posY = (int)roundf((py - D.min_y) * D.inv_h);
    const bool ingrid = !(posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS);
    const int oct = *reinterpret_cast<const int*>(rec + D.kp_oct_off);
    const bool lev = !(oct < W.minLevel) && !(W.maxLevel >= 0 && oct > W.maxLevel);
    const float distx = px - W.x, disty = py - W.y;
    bool hit = ingrid && posX >= W.nMinCellX && posX <= W.nMaxCellX && posY >= W.nMinCellY && posY <= W.nMaxCellY && lev &&
               fabsf(distx) < W.r && fabsf(disty) < W.r;
    if (ER == SLAMIT_SEARCH_ER_RADIUS && hit) {
        const float kur = KUR[i];
        if (kur > 0) {
            const float er = fabsf(W.ur - kur);
            if (er > W.r) hit = false;
        }
    }
    if (hit && D.chi2_gate > 0.f) {   // ORBmatcher::Fuse, ORBmatcher.cc:918-942
        const float kur = ER == SLAMIT_SEARCH_ER_CHI2 ? KUR[i] : -1.f;
        if (ER == SLAMIT_SEARCH_ER_CHI2 && kur >= 0) {
            const float er = W.ur - kur;
            const float e2 = (distx * distx + disty * disty) + er * er;
            if (e2 * D.inv_sigma2[oct & 15] > D.chi2_gate_stereo) hit = false;
        } else {
            const float e2 = distx * distx + disty * disty;
            if (e2 * D.inv_sigma2[oct & 15] > D.chi2_gate) hit = false;
        }
    }
    if (hit) {
        const uint4* T = reinterpret_cast<const uint4*>(KD + 32 * (size_t)i);
        const uint4 t0 = T[0], t1 = T[1];
        const int d = hamming256(W.a0, W.a1, t0, t1);
        hit = d < 256;   // bestDist starts at 256 and the test is a strict '<': a complement never wins
        key = ((unsigned long long)d << 32) | ((unsigned long long)(posX * GRID_ROWS + posY) << 17) |
              ((unsigned long long)i << 4) | (unsigned long long)(oct & 15);
    }
    return hit;
}

template <int ER>
__global__ __launch_bounds__(256) void search_candidates_kernel(SearchDev D) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.y;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int m = D.m_arr ? min(D.m_arr[f], D.q_cap) : D.m_fixed;
    if (q >= m) return;
    const int n = D.n_arr ? min(D.n_arr[f], D.kp_cap) : D.n_fixed;
    const size_t qo = (size_t)f * D.q_cap + q;
    if (lane == 0) { D.cand_n[qo] = 0; D.tent[2 * qo] = ~0ull; D.tent[2 * qo + 1] = ~0ull; }
    if (!D.valid[qo]) return;
    QueryWin W;
    if (!query_window<ER>(D, qo, W)) return;
    unsigned long long* out = D.cand + qo * D.cand_cap;
    const uint8_t* KP = D.kp + (size_t)f * D.kp_cap * D.kp_rec;
    const uint8_t* KD = D.kp_desc + (size_t)f * D.kp_cap * 32;
    const uint8_t* TK = D.kp_taken + (size_t)f * D.kp_cap;
    const float* KUR = ER != SLAMIT_SEARCH_ER_NONE ? D.kp_ur + (size_t)f * D.kp_cap : nullptr;
    int count = 0;
    unsigned long long k1 = ~0ull, k2 = ~0ull;   // this lane's two smallest keys among keypoints free on entry
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        unsigned long long key = 0;
        const bool hit = i < n && window_key<ER>(D, W, KP, KD, KUR, i, key);
        const unsigned long long mk = __ballot(hit);
        if (hit) {
            const int o = count + __popcll(mk & ((1ull << lane) - 1ull));
            if (o < D.cand_cap) out[o] = key;
            if (D.mode == 1 || !TK[i]) keep2(k1, k2, key);
        }
        count += __popcll(mk);
    }
    // tentative (best, second): exact for the resolve pass unless an EARLIER query of this call takes one of the two
    unsigned long long best, second;
    wave_min2(k1, k2, best, second);
    if (lane == 0) { D.cand_n[qo] = count; D.tent[2 * qo] = best; D.tent[2 * qo + 1] = second; }
}

// One query's answer: the keypoint (or -1) and (best_dist, best_level, second_dist, second_level) as out4 reports them
struct SearchHit { int res = -1, bd = 256, bl = -1, sd = 256, sl = -1; };

// The serial half.  One wavefront per frame walks that frame's queries IN ORDER (the reference commits the winning keypoint before it
// looks at the next map point).  The candidates kernel already found every query's two smallest keys among the keypoints free on
// entry; removing OTHER candidates cannot change the two smallest, so that pair is still the answer unless the state an earlier query
// of this call left behind excludes one of the two.  The walk therefore only asks the state about two keypoints per query (64 queries'
// pairs are loaded at once, lane j holding query j) and re-scans the query's candidates on the rare conflict.
//
// What the per-keypoint state is comes in as `State`, a small struct of force-inlined members over LDS the kernel owns:
//     void      init(D, f, n, lane)      fills the state for frame f's n keypoints and publishes it to the wavefront
//     bool      excluded(key)            may the query this key belongs to not have the key's keypoint?
//     void      decide(D, best, r, takes_q, lane, qb, j, res, nmatches)
//                                        the acceptance rule for query qb + j (r: its distances) and its commit to the state; `res`
//                                        is this lane's pending result of query qb + lane, which a take-over may reset
//     void      end_chunk()              after a chunk's results are stored
// The mode is the type: the loop is serial (about 1 us per query), so nothing in it is decided at run time.
template <int ER, class State>
__device__ __forceinline__ void search_resolve_walk(const SearchDev& D, State& S) {
    const int lane = threadIdx.x, f = blockIdx.x;
    const int n = D.n_arr ? min(D.n_arr[f], D.kp_cap) : D.n_fixed;
    const int m = D.m_arr ? min(D.m_arr[f], D.q_cap) : D.m_fixed;
    S.init(D, f, n, lane);
    const size_t q0 = (size_t)f * D.q_cap;
    int nmatches = 0;
    for (int qb = 0; qb < m; qb += 64) {
        const int qj = qb + lane;
        const bool live = qj < m;
        unsigned long long tb = KEY_NONE, ts = KEY_NONE;
        int ncq = 0, tkq = 0;
        if (live) { tb = D.tent[2 * (q0 + qj)]; ts = D.tent[2 * (q0 + qj) + 1]; ncq = D.cand_n[q0 + qj]; tkq = D.takes[q0 + qj]; }
        SearchHit mine;     // lane j collects query qb + j
        const int jn = min(64, m - qb);
        for (int j = 0; j < jn; ++j) {
            unsigned long long best = readlane_u64(tb, j), second = readlane_u64(ts, j);
            const int takes_q = __builtin_amdgcn_readlane(tkq, j);
            // both tests unconditionally (a lone best stands in for its second): two independent LDS reads, no branch between them
            if (best != KEY_NONE && (S.excluded(best) | S.excluded(second != KEY_NONE ? second : best))) {   // stale: re-scan under the state as it is now
                const size_t qo = q0 + qb + j;
                const int nc_all = __builtin_amdgcn_readlane(ncq, j);
                // The stored list is only read HERE.  The tentative pair was reduced over every hit, so a window that holds
                // more than cand_cap keypoints is exact as long as no re-scan of it is needed; a re-scan of a TRUNCATED list
                // walks the frame's keypoints again instead (the reference has no limit on a window's size, ORBmatcher.cc:85-117).
                unsigned long long k1 = KEY_NONE, k2 = KEY_NONE;
                if (nc_all <= D.cand_cap) {
                    const unsigned long long* C = D.cand + qo * D.cand_cap;
                    for (int c = lane; c < nc_all; c += 64) {
                        const unsigned long long k = C[c];
                        if (!S.excluded(k)) keep2(k1, k2, k);
                    }
                } else {
                    QueryWin W;
                    query_window<ER>(D, qo, W);   // (it met the grid: the query has candidates)
                    const uint8_t* KP = D.kp + (size_t)f * D.kp_cap * D.kp_rec;
                    const uint8_t* KD = D.kp_desc + (size_t)f * D.kp_cap * 32;
                    const float* KUR = ER != SLAMIT_SEARCH_ER_NONE ? D.kp_ur + (size_t)f * D.kp_cap : nullptr;
                    for (int i = lane; i < n; i += 64) {
                        unsigned long long k;
                        if (window_key<ER>(D, W, KP, KD, KUR, i, k) && !S.excluded(k)) keep2(k1, k2, k);
                    }
                }
                wave_min2(k1, k2, best, second);
            }
            SearchHit r;
            if (best != KEY_NONE) {
                r.bd = (int)(best >> 32);
                if (second != KEY_NONE) { r.sd = (int)(second >> 32); r.sl = KEY_OCT(second); }
                S.decide(D, best, r, takes_q, lane, qb, j, mine.res, nmatches);
            }
            if (lane == j) mine = r;
        }
        if (live) {
            const size_t qo = q0 + qj;
            D.match_kp[qo] = mine.res;
            if (D.out4) *reinterpret_cast<int4*>(&D.out4[4 * qo]) = make_int4(mine.bd, mine.bl, mine.sd, mine.sl);
        }
        S.end_chunk();
    }
    if (lane == 0) D.nmatches[f] = nmatches;
}

// publishes lane 0's write to the LDS state before the next query reads it
__device__ __forceinline__ void search_state_publish() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// mode 0 (SearchByProjection, Fuse): a keypoint is free or taken, F.mvpMapPoints[idx] with observations; a query with `takes` set
// takes the keypoint it is matched to.  ORBmatcher.cc:85-128.
struct TakenBits {
    unsigned* taken;   // LDS bit mask, one bit per keypoint
    __device__ __forceinline__ void init(const SearchDev& D, int f, int n, int lane) {
        const uint8_t* TK = D.kp_taken + (size_t)f * D.kp_cap;
        for (int w = lane; w < (n + 31) / 32; w += 64) {
            unsigned bits = 0;
            for (int b = 0; b < 32; ++b) { const int i = 32 * w + b; if (i < n && TK[i]) bits |= 1u << b; }
            taken[w] = bits;
        }
        search_state_publish();
    }
    __device__ __forceinline__ bool excluded(unsigned long long key) const {
        const int i = KEY_KP(key);
        return (taken[i >> 5] >> (i & 31)) & 1u;
    }
    __device__ __forceinline__ void decide(const SearchDev& D, unsigned long long best, SearchHit& r, int takes_q, int lane, int, int, int&, int& nmatches) {
        const int bi = KEY_KP(best);
        r.bl = KEY_OCT(best);
        if (r.bd <= D.th_dist) {   // ORBmatcher.cc:120-128
            const bool reject = D.use_ratio && r.bl == r.sl && (float)r.bd > D.nnratio * (float)r.sd;
            if (!reject) {
                r.res = bi;
                if (takes_q) {
                    if (lane == 0) taken[bi >> 5] |= 1u << (bi & 31);
                    search_state_publish();
                }
                ++nmatches;
            }
        }
    }
    __device__ __forceinline__ void end_chunk() const {}
};

// mode 1 (ORBmatcher::SearchForInitialization, ORBmatcher.cc:409-474): a keypoint carries the distance of its current match and the
// query that holds it.  A candidate is excluded when that distance is <= the query's own (:448); an accepted query takes the keypoint
// over and the previous holder loses it (:466-470).
struct MatchedDist {
    int* md;    // LDS, per keypoint: distance of its current match (INT_MAX: none)
    int* m21;   // LDS, per keypoint: the query holding it, or -1
    __device__ __forceinline__ void init(const SearchDev&, int, int n, int lane) {
        for (int i = lane; i < n; i += 64) { md[i] = 0x7FFFFFFF; m21[i] = -1; }
        search_state_publish();
    }
    __device__ __forceinline__ bool excluded(unsigned long long key) const { return md[KEY_KP(key)] <= (int)(key >> 32); }
    __device__ __forceinline__ void decide(const SearchDev& D, unsigned long long best, SearchHit& r, int, int lane, int qb, int j, int& res, int& nmatches) {
        const int bi = KEY_KP(best);
        const float second_f = r.sl < 0 ? 2147483648.0f /* no second: (float)INT_MAX */ : (float)r.sd;
        if (r.bd <= D.th_dist && (float)r.bd < second_f * D.nnratio) {   // ORBmatcher.cc:462-464
            const int old = m21[bi];
            if (old >= 0) {   // the keypoint changes hands: vnMatches12[vnMatches21[bestIdx2]] = -1
                if (old >= qb) { if (lane == old - qb) res = -1; }   // the holder is of this chunk: its result is still in a lane
                else if (lane == 0) D.match_kp[(size_t)blockIdx.x * D.q_cap + old] = -1;
                --nmatches;
            }
            r.res = bi;
            r.bl = bi;   // mode 1 reports the keypoint accepted AT DECISION TIME in the level slot (levels are all 0
                         // here); unlike match_kp it is not reset by a later take-over -- the rotation histogram bins it
            if (lane == 0) { m21[bi] = qb + j; md[bi] = r.bd; }
            search_state_publish();
            ++nmatches;
        }
    }
    // later chunks may reset entries of this one through global memory
    __device__ __forceinline__ void end_chunk() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent"); }
};

template <int ER>
__global__ __launch_bounds__(64) void search_resolve_kernel(SearchDev D) {
    __shared__ unsigned taken[(SLAMIT_SEARCH_MAX_KP + 32) / 32];
    TakenBits S{taken};
    search_resolve_walk<ER>(D, S);
}

__global__ __launch_bounds__(64) void search_resolve_init_kernel(SearchDev D) {
    extern __shared__ int s_state[];   // md[kp_cap] | m21[kp_cap]
    MatchedDist S{s_state, s_state + D.kp_cap};
    search_resolve_walk<SLAMIT_SEARCH_ER_NONE>(D, S);   // SearchForInitialization has no stereo branch
}

// the two launches of mode 0 for one er_mode
template <int ER>
static void search_launch_taken(hipStream_t st, const SearchDev& D, int max_m) {
    if (max_m > 0)
        hipLaunchKernelGGL(search_candidates_kernel<ER>, dim3((max_m + 3) / 4, D.nframes), dim3(256), 0, st, D);
    hipLaunchKernelGGL(search_resolve_kernel<ER>, dim3(D.nframes), dim3(64), 0, st, D);
}

static void search_launch(hipStream_t st, const SearchDev& D, int max_m) {
    if (D.er_mode == SLAMIT_SEARCH_ER_RADIUS) return search_launch_taken<SLAMIT_SEARCH_ER_RADIUS>(st, D, max_m);
    if (D.er_mode == SLAMIT_SEARCH_ER_CHI2) return search_launch_taken<SLAMIT_SEARCH_ER_CHI2>(st, D, max_m);
    if (D.mode != 1) return search_launch_taken<SLAMIT_SEARCH_ER_NONE>(st, D, max_m);
    if (max_m > 0)
        hipLaunchKernelGGL(search_candidates_kernel<SLAMIT_SEARCH_ER_NONE>, dim3((max_m + 3) / 4, D.nframes), dim3(256), 0, st, D);
    {
        static bool prepared = false;   // 2 x 4 x 8191 bytes of state sit just under the 64 KB default; ask explicitly
        if (!prepared) { hipFuncSetAttribute(reinterpret_cast<const void*>(search_resolve_init_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024); prepared = true; }
        hipLaunchKernelGGL(search_resolve_init_kernel, dim3(D.nframes), dim3(64), 2 * sizeof(int) * (size_t)D.kp_cap, st, D);
    }
}

// the rule half of SearchDev, the same for both entry points
static void search_rule_fill(SearchDev& D, const slamit_search_rule* rule) {
    D.th_dist = rule->th_dist; D.use_ratio = rule->use_ratio; D.nnratio = rule->nnratio;
    D.chi2_gate = rule->mode == 1 ? 0.f : rule->chi2_gate; memcpy(D.inv_sigma2, rule->inv_level_sigma2, sizeof(D.inv_sigma2));
    D.mode = rule->mode;
}

// The stereo record's own checks, the same for both entry points (dev: the message names the batch form); null arrays are each entry
// point's to test, where it knows whether there is work.  0: fine.
static int search_stereo_check(bool dev, const slamit_search_rule* rule, int er_mode, int q_ur_stride) {
    if (er_mode < SLAMIT_SEARCH_ER_NONE || er_mode > SLAMIT_SEARCH_ER_CHI2)
        return slamit_fail(SLAMIT_ERR_ARG, dev ? "slamit_guided_search_stereo_batch_dev: er_mode outside 0..2" : "slamit_guided_search_stereo: er_mode outside 0..2");
    if (er_mode == SLAMIT_SEARCH_ER_NONE) return SLAMIT_OK;
    if (q_ur_stride < 1)
        return slamit_fail(SLAMIT_ERR_ARG, dev ? "slamit_guided_search_stereo_batch_dev: q_ur_stride < 1" : "slamit_guided_search_stereo: q_ur_stride < 1");
    if (rule->mode == 1)
        return slamit_fail(SLAMIT_ERR_ARG, dev ? "slamit_guided_search_stereo_batch_dev: er_mode with rule mode 1 (SearchForInitialization has no stereo branch)"
                                               : "slamit_guided_search_stereo: er_mode with rule mode 1 (SearchForInitialization has no stereo branch)");
    return SLAMIT_OK;
}

extern "C" int slamit_guided_search_stereo(int device, const slamit_frame_view* F, const slamit_search_queries* Q,
                                           const slamit_search_rule* rule, const slamit_search_stereo* st, int32_t* match_kp, int32_t* nmatches,
                                           int32_t* best_dist, int32_t* best_level, int32_t* second_dist, int32_t* second_level) {
    if (!F || !Q || !rule || !nmatches || F->n < 0 || Q->m < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_guided_search: bad argument");
    const int er_mode = st ? st->er_mode : SLAMIT_SEARCH_ER_NONE;
    if (st) {
        const int rc = search_stereo_check(false, rule, er_mode, st->q_ur_stride);
        if (rc != SLAMIT_OK) return rc;
        if (er_mode != SLAMIT_SEARCH_ER_NONE && Q->m && (!st->q_ur || (F->n && !st->kp_ur)))
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_guided_search_stereo: er_mode set with a null kp_ur or q_ur");
    }
    *nmatches = 0;
    if (Q->m == 0) return SLAMIT_OK;
    if (!match_kp || !Q->uvr || !Q->level_min || !Q->level_max || !Q->desc || !Q->valid ||
        (F->n && (!F->kp_xy || !F->kp_octave || !F->desc || !F->kp_taken)))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_guided_search: null array");
    if (F->n > SLAMIT_SEARCH_MAX_KP) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_guided_search: more than SLAMIT_SEARCH_MAX_KP keypoints");
    SLAMIT_USE_DEVICE(device);
    const size_t n = F->n, m = Q->m, cap = std::min(std::max(F->n, 1), SLAMIT_SEARCH_MAX_CAND);
    // One pinned staging block and one device slab per host thread, kept between calls (a Tracking thread makes this
    // call every frame: a fresh hipMalloc + nine pageable copies cost more than the search itself).  The candidate lists
    // and tentative pairs live only on the device.
    StageLayout L;
    const StageSpan<uint8_t> kp = L.take<uint8_t>(12 * n), kd = L.take<uint8_t>(32 * n), tk = L.take<uint8_t>(n);   // kp: {x, y, octave} records
    const StageSpan<float> uvr = L.take<float>(3 * m);
    const StageSpan<int> l0 = L.take<int>(m), l1 = L.take<int>(m);
    const StageSpan<uint8_t> qd = L.take<uint8_t>(32 * m), va = L.take<uint8_t>(m), tq = L.take<uint8_t>(m);
    const StageSpan<float> kur = L.take<float>(er_mode ? n : 0), qur = L.take<float>(er_mode ? m : 0);   // no gate: no room taken
    L.end_inputs();
    const StageSpan<int> mk = L.take<int>(m), o4 = L.take<int>(4 * m), nm = L.take<int>(1);
    L.end_outputs();
    const StageSpan<unsigned long long> cand = L.take<unsigned long long>(m * cap);
    const StageSpan<int> cn = L.take<int>(m);
    const StageSpan<unsigned long long> te = L.take<unsigned long long>(2 * m);
    static thread_local SlamitScratch S;
    HIP_TRY_AT("slamit_guided_search: scratch", slamit_stage_reserve(S, device, L));
    for (size_t i = 0; i < n; ++i) {
        memcpy(kp.at(S.host) + 12 * i, &F->kp_xy[2 * i], 8);
        memcpy(kp.at(S.host) + 12 * i + 8, &F->kp_octave[i], 4);
    }
    memcpy(kd.at(S.host), F->desc, kd.bytes()); memcpy(tk.at(S.host), F->kp_taken, tk.bytes());
    memcpy(uvr.at(S.host), Q->uvr, uvr.bytes()); memcpy(l0.at(S.host), Q->level_min, l0.bytes()); memcpy(l1.at(S.host), Q->level_max, l1.bytes());
    memcpy(qd.at(S.host), Q->desc, qd.bytes()); memcpy(va.at(S.host), Q->valid, va.bytes());
    if (Q->takes) memcpy(tq.at(S.host), Q->takes, tq.bytes()); else memset(tq.at(S.host), 1, tq.bytes());
    if (er_mode) {
        if (n) memcpy(kur.at(S.host), st->kp_ur, kur.bytes());
        float* qu = qur.at(S.host);
        for (size_t q = 0; q < m; ++q) qu[q] = st->q_ur[q * (size_t)st->q_ur_stride];   // packed on the way up: the device reads stride 1
    }
    HIP_TRY_AT("slamit_guided_search", slamit_stage_upload(S, L));
    SearchDev D;
    D.nframes = 1; D.kp_cap = std::max(F->n, 1); D.q_cap = Q->m; D.cand_cap = (int)cap;
    D.n_arr = nullptr; D.n_fixed = F->n; D.m_arr = nullptr; D.m_fixed = Q->m;
    D.kp = kp.at(S.dev); D.kp_rec = 12; D.kp_oct_off = 8; D.kp_desc = kd.at(S.dev); D.kp_taken = tk.at(S.dev);
    D.min_x = F->min_x; D.min_y = F->min_y; D.inv_w = F->inv_w; D.inv_h = F->inv_h;
    D.uvr = uvr.at(S.dev); D.lmin = l0.at(S.dev); D.lmax = l1.at(S.dev); D.qdesc = qd.at(S.dev); D.valid = va.at(S.dev); D.takes = tq.at(S.dev);
    D.cand = cand.at(S.dev); D.cand_n = cn.at(S.dev); D.tent = te.at(S.dev);
    search_rule_fill(D, rule);
    D.er_mode = er_mode; D.chi2_gate_stereo = er_mode ? st->chi2_gate_stereo : 0.f;
    D.kp_ur = er_mode ? kur.at(S.dev) : nullptr; D.q_ur = er_mode ? qur.at(S.dev) : nullptr; D.q_ur_stride = 1;
    D.match_kp = mk.at(S.dev); D.out4 = o4.at(S.dev); D.nmatches = nm.at(S.dev);
    search_launch(S.st, D, Q->m);
    HIP_TRY_AT("slamit_guided_search", slamit_stage_download_and_wait(S, L));
    *nmatches = *nm.at(S.host);
    memcpy(match_kp, mk.at(S.host), mk.bytes());
    const int* r4 = o4.at(S.host);
    for (size_t q = 0; q < m; ++q) {
        if (best_dist) best_dist[q] = r4[4 * q];
        if (best_level) best_level[q] = r4[4 * q + 1];
        if (second_dist) second_dist[q] = r4[4 * q + 2];
        if (second_level) second_level[q] = r4[4 * q + 3];
    }
    return SLAMIT_OK;
}

extern "C" int slamit_guided_search(int device, const slamit_frame_view* F, const slamit_search_queries* Q,
                                    const slamit_search_rule* rule, int32_t* match_kp, int32_t* nmatches, int32_t* best_dist,
                                    int32_t* best_level, int32_t* second_dist, int32_t* second_level) {
    return slamit_guided_search_stereo(device, F, Q, rule, nullptr, match_kp, nmatches, best_dist, best_level, second_dist, second_level);
}

extern "C" size_t slamit_guided_search_workspace(int nframes, int q_cap) {
    if (nframes < 0 || q_cap < 0) return 0;
    return (size_t)nframes * q_cap * (8 * (size_t)SLAMIT_SEARCH_BATCH_CAND + 16 + 4) + 256;
}

extern "C" int slamit_guided_search_stereo_batch_dev(int device, const slamit_search_batch* B, const slamit_search_rule* rule,
                                                     const slamit_search_stereo_dev* st, int32_t* d_match_kp, int32_t* d_nmatches, int32_t* d_out4,
                                                     void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!B || !rule || !d_match_kp || !d_nmatches || B->nframes < 0 || B->kp_cap < 0 || B->q_cap < 0)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_guided_search_batch_dev: bad argument");
    const int er_mode = st ? st->er_mode : SLAMIT_SEARCH_ER_NONE;
    if (st) {
        const int rc = search_stereo_check(true, rule, er_mode, st->q_ur_stride);
        if (rc != SLAMIT_OK) return rc;
        // the host cannot see d_n / d_m: a batch with frames and room for queries has work to do
        if (er_mode != SLAMIT_SEARCH_ER_NONE && B->nframes && B->q_cap && (!st->d_q_ur || (B->kp_cap && !st->d_kp_ur)))
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_guided_search_stereo_batch_dev: er_mode set with a null d_kp_ur or d_q_ur");
    }
    if (B->nframes == 0) return SLAMIT_OK;
    if (!B->d_n || !B->d_kps_un || !B->d_desc || !B->d_kp_taken || !B->d_m || !B->d_uvr || !B->d_level_min || !B->d_level_max ||
        !B->d_qdesc || !B->d_valid || !B->d_takes || !d_workspace)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_guided_search_batch_dev: null array");
    if (B->kp_cap > SLAMIT_SEARCH_MAX_KP) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_guided_search_batch_dev: kp_cap > SLAMIT_SEARCH_MAX_KP");
    if (workspace_bytes < slamit_guided_search_workspace(B->nframes, B->q_cap))
        return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_guided_search_batch_dev: workspace smaller than slamit_guided_search_workspace()");
    SLAMIT_USE_DEVICE(device);
    SearchDev D;
    D.nframes = B->nframes; D.kp_cap = B->kp_cap; D.q_cap = B->q_cap; D.cand_cap = SLAMIT_SEARCH_BATCH_CAND;
    D.n_arr = B->d_n; D.n_fixed = 0; D.m_arr = B->d_m; D.m_fixed = 0;
    D.kp = reinterpret_cast<const uint8_t*>(B->d_kps_un); D.kp_rec = (int)sizeof(slamit_kp); D.kp_oct_off = 20;
    D.kp_desc = B->d_desc; D.kp_taken = B->d_kp_taken;
    D.min_x = B->min_x; D.min_y = B->min_y; D.inv_w = B->inv_w; D.inv_h = B->inv_h;
    D.uvr = B->d_uvr; D.lmin = B->d_level_min; D.lmax = B->d_level_max; D.qdesc = B->d_qdesc; D.valid = B->d_valid; D.takes = B->d_takes;
    const size_t nq = (size_t)B->nframes * B->q_cap;
    D.cand = reinterpret_cast<unsigned long long*>(d_workspace);
    D.tent = D.cand + nq * SLAMIT_SEARCH_BATCH_CAND;
    D.cand_n = reinterpret_cast<int*>(D.tent + 2 * nq);
    search_rule_fill(D, rule);
    D.er_mode = er_mode; D.chi2_gate_stereo = er_mode ? st->chi2_gate_stereo : 0.f;
    D.kp_ur = er_mode ? st->d_kp_ur : nullptr; D.q_ur = er_mode ? st->d_q_ur : nullptr; D.q_ur_stride = er_mode ? st->q_ur_stride : 1;
    D.match_kp = d_match_kp; D.out4 = d_out4; D.nmatches = d_nmatches;
    search_launch((hipStream_t)stream, D, B->q_cap);
    HIP_TRY(hipGetLastError());
    return SLAMIT_OK;
}

extern "C" int slamit_guided_search_batch_dev(int device, const slamit_search_batch* B, const slamit_search_rule* rule,
                                              int32_t* d_match_kp, int32_t* d_nmatches, int32_t* d_out4, void* d_workspace,
                                              size_t workspace_bytes, void* stream) {
    return slamit_guided_search_stereo_batch_dev(device, B, rule, nullptr, d_match_kp, d_nmatches, d_out4, d_workspace, workspace_bytes, stream);
}
