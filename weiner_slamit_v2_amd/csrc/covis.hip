// covis.hip — KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling on the GPU (include/slamit.h, slamit_update_connections*
// and slamit_keyframe_culling*; both walks are stated in covis.h, whose per-element functions the kernels call).
//
// UpdateConnections, a grid over (something, item), one item per map:
//   (a) cv_counts_kernel     local_map.hip's vote pass with keyframe k's row in place of a frame's: one lane per keypoint walks its
//                            point's observers and adds 1 per observer other than k with an integer atomicAdd -- into a histogram in
//                            LDS that the workgroup flushes when the map has at most CV_LDS_KF keyframes, into HBM otherwise.
//   (b) cv_list_kernel       one workgroup per item.  Its first wavefront reads the counts 64 slots at a time: the size of the
//                            counter, the number at or above 15 and the maximum as a wave minimum of (inverted count, slot); then
//                            again, compacting the counter into k's cw row in ascending slot order (ballot + scan) and the listed
//                            keys into LDS.  All four wavefronts then place the keys by rank into k's ord row and kf_best row.
//   (c) cv_neighbour_kernel  one workgroup per (item, listed neighbour j): j's cw row into LDS as keys, the entry of k found or its
//                            place counted, the row updated or opened up by one, and the WHOLE row placed by rank into j's ord row
//                            and kf_best row.  Rows of different j are different memory; k's rows are only read.
// KeyFrameCulling, culls being rare:
//   cv_cull_first_kernel     one workgroup per (problem, candidate) evaluates with nothing culled: exact up to and including the
//                            first cull of the problem.
//   cv_cull_cascade_kernel   one workgroup per problem finds the first cull (atomicMin in LDS) and evaluates only the candidates
//                            behind it again, one after the other, against the culled set as a bitset in LDS; then marks the points
//                            the set turned bad.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "wave_ops.h"
#include "map_check.h"
#include "covis.h"

static_assert(sizeof(CvIndex) == sizeof(slamit_covis_index) && offsetof(CvIndex, mp_nobs) == offsetof(slamit_covis_index, mp_nobs) &&
                  offsetof(CvIndex, kf_not_erase) == offsetof(slamit_covis_index, kf_not_erase) && offsetof(CvIndex, cw_n) == offsetof(slamit_covis_index, cw_n) &&
                  offsetof(CvIndex, ord_n) == offsetof(slamit_covis_index, ord_n) && offsetof(CvIndex, kf_best) == offsetof(slamit_covis_index, kf_best),
              "slamit_covis_index is CvIndex");
static_assert(sizeof(LmMap) == sizeof(slamit_map_index), "slamit_map_index is LmMap");
static_assert(CV_NO_OBSERVER == SLAMIT_COVIS_NO_OBSERVER && CV_ROW_OVERFLOW == SLAMIT_COVIS_ROW_OVERFLOW && CV_BAD_SLOT == SLAMIT_COVIS_BAD_SLOT &&
                  CV_MAX_ROW == SLAMIT_COVIS_MAX_ROW && CV_TH == SLAMIT_COVIS_TH && CV_KEPT == SLAMIT_COVIS_KEPT && CV_CULLED == SLAMIT_COVIS_CULLED &&
                  CV_TO_BE_ERASED == SLAMIT_COVIS_TO_BE_ERASED && CV_ORIGIN == SLAMIT_COVIS_ORIGIN,
              "covis.h restates the C-ABI's constants");

#define CV_LDS_KF 4096                                  // keyframes whose counts fit the workgroup's LDS histogram (16 KiB)
#define CV_COUNT_BLOCKS 4                               // workgroups striding one keyframe's row in (a)
#define CV_SET_WORDS ((LM_MAX_KF + 1 + 31) / 32)        // the culled set, a bit per slot (8 KiB)
#define CV_NT 256

// The batches as the kernels' argument: the maps' records travel with them, the arrays stay where the caller keeps them.
struct CvConnBatch {
    int32_t nitems, count_cap;
    int32_t item_map[SLAMIT_LOCAL_MAP_MAX_MAPS];
    LmMap maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    CvIndex covis[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const int32_t* kf; const int32_t* first;
    int32_t* counts; int32_t* n_counted; int32_t* n_listed; int32_t* parent; int32_t* status;
};
struct CvCullBatch {
    int32_t nprob, n_maps, cand_cap, mp_cap;
    LmMap maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    CvIndex covis[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const int32_t* prob_map; const int32_t* kf; const int32_t* monocular;
    uint8_t* verdict; int32_t* n_mps; int32_t* n_redundant; int32_t* n_cand; uint8_t* mp_turned_bad; int32_t* status;
};

__device__ __forceinline__ int cv_wave_total(int v) { return __builtin_amdgcn_readlane(wave_inclusive_scan_i32(v), 63); }   // every lane active

// the map and columns of item `it`, capacities bounding every index into an item's row
__device__ __forceinline__ void cv_item(const CvConnBatch& B, int it, LmMap& M, CvIndex& X) {
    const int m = B.item_map[it];
    M = B.maps[m]; X = B.covis[m];
    M.n_kf = min(M.n_kf, min(B.count_cap, LM_MAX_KF));
    X.row_cap = cv_clamp(X.row_cap, CV_MAX_ROW);
}

// ---- (a) grid (CV_COUNT_BLOCKS, items), 256 threads -------------------------------------------------------------------------------
__global__ __launch_bounds__(CV_NT) void cv_counts_kernel(CvConnBatch B) {
    __shared__ int hist[CV_LDS_KF];
    const int it = blockIdx.y;
    LmMap M; CvIndex X;
    cv_item(B, it, M, X);
    const int k = __builtin_amdgcn_readfirstlane(B.kf[it]);
    if (!lm_kf_ok(M, k)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&B.status[it], CV_BAD_SLOT);
        return;
    }
    const int e0 = M.kf_mp_ptr[k], e1 = M.kf_mp_ptr[k + 1];
    if (e0 + (int)(blockIdx.x * CV_NT) >= e1) return;   // the whole workgroup
    const bool lds = M.n_kf <= CV_LDS_KF;
    if (lds) {
        for (int j = threadIdx.x; j < M.n_kf; j += CV_NT) hist[j] = 0;
        __syncthreads();
    }
    int32_t* const counts = B.counts + (size_t)it * B.count_cap;
    int st = 0;
    for (int e = e0 + (int)(blockIdx.x * CV_NT + threadIdx.x); e < e1; e += CV_COUNT_BLOCKS * CV_NT) {
        const int p = M.kf_mp[e];
        if (p == -1) continue;
        if (!lm_mp_ok(M, p)) { st = CV_BAD_SLOT; continue; }
        if (M.mp_bad[p]) continue;
        const int o1 = M.obs_ptr[p + 1];
        for (int o = M.obs_ptr[p]; o < o1; ++o) {
            const int j = M.obs_kf[o];
            if (!lm_kf_ok(M, j)) { st = CV_BAD_SLOT; continue; }
            if (j == k) continue;
            if (lds) atomicAdd(&hist[j], 1); else atomicAdd(&counts[j], 1);
        }
    }
    if (st) atomicOr(&B.status[it], st);
    if (lds) {
        __syncthreads();
        for (int j = threadIdx.x; j < M.n_kf; j += CV_NT) {
            const int v = hist[j];
            if (v) atomicAdd(&counts[j], v);
        }
    }
}

// keys[n] in LDS -> the ordered row and the kf_best row of keyframe j, by the whole workgroup (the caller has synchronised)
__device__ __forceinline__ void cv_place_row(const CvIndex& X, int j, const unsigned long long* keys, int n) {
    for (int i = threadIdx.x; i < n; i += CV_NT) cv_place(X, j, keys, n, i);
    if (threadIdx.x < LM_BEST) cv_pad_best(X, j, n, threadIdx.x);
    if (threadIdx.x == 0) X.ord_n[j] = n;
}

// ---- (b) grid (items), 256 threads -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CV_NT) void cv_list_kernel(CvConnBatch B) {
    __shared__ unsigned long long keys[CV_MAX_ROW];
    __shared__ int n_keys;
    const int it = blockIdx.x, lane = threadIdx.x & 63;
    LmMap M; CvIndex X;
    cv_item(B, it, M, X);
    const int k = __builtin_amdgcn_readfirstlane(B.kf[it]);
    if (threadIdx.x == 0) n_keys = 0;
    __syncthreads();
    if (threadIdx.x < 64) {   // the first wavefront, every lane of it
        B.n_listed[it] = 0; B.n_counted[it] = 0;
        const int32_t* const counts = B.counts + (size_t)it * B.count_cap;
        int nc = 0, nl = 0;
        unsigned long long best = ~0ull;   // (0x7fffffff - count, slot): the minimum is the largest count at its lowest slot
        if (lm_kf_ok(M, k))
            for (int j0 = 0; j0 < M.n_kf; j0 += 64) {
                const int j = j0 + lane;
                const int v = j < M.n_kf ? counts[j] : 0;
                nc += __popcll(__ballot(v > 0));
                nl += __popcll(__ballot(v >= CV_TH));
                if (v > 0) {
                    const unsigned long long key = ((unsigned long long)(unsigned)(0x7fffffff - v) << 32) | (unsigned)j;
                    best = key < best ? key : best;
                }
            }
        best = wave_min_u64(best);
        int st = 0;
        if (!lm_kf_ok(M, k)) st = 0;   // (a) reported it
        else if (nc == 0) st = CV_NO_OBSERVER;
        else if (nc > X.row_cap) st = CV_ROW_OVERFLOW;
        if (lane == 0) {
            B.n_counted[it] = nc;
            if (st) atomicOr(&B.status[it], st);
        }
        if (lm_kf_ok(M, k) && nc > 0 && nc <= X.row_cap) {
            int32_t* const ckf = X.cw_kf + (size_t)k * X.row_cap;
            int32_t* const cw = X.cw_w + (size_t)k * X.row_cap;
            int cbase = 0, lbase = 0;
            for (int j0 = 0; j0 < M.n_kf; j0 += 64) {
                const int j = j0 + lane;
                const int v = j < M.n_kf ? counts[j] : 0;
                const bool counted = v > 0, listed = v >= CV_TH;
                const int cr = cbase + wave_inclusive_scan_i32(counted ? 1 : 0) - 1;
                const int lr = lbase + wave_inclusive_scan_i32(listed ? 1 : 0) - 1;
                if (counted) { ckf[cr] = j; cw[cr] = v; }          // cr < nc <= row_cap
                if (listed) keys[lr] = cv_key(v, j);                // lr < nl <= nc <= row_cap <= CV_MAX_ROW
                cbase += __popcll(__ballot(counted));
                lbase += __popcll(__ballot(listed));
            }
            if (lane == 0) {
                X.cw_n[k] = nc;
                if (nl == 0) { keys[0] = cv_key(0x7fffffff - (int)(unsigned)(best >> 32), (int)(unsigned)best); nl = 1; }
                n_keys = nl;
            }
        }
    }
    __syncthreads();
    const int n = n_keys;
    if (n == 0) return;   // the whole workgroup
    cv_place_row(X, k, keys, n);
    __syncthreads();      // the row's front, for the parent
    if (threadIdx.x == 0) {
        B.n_listed[it] = n;
        B.parent[it] = B.first[it] && k != X.origin_kf ? X.ord_kf[(size_t)k * X.row_cap] : -1;
    }
}

// ---- (c) grid (largest row_cap, items), 256 threads -------------------------------------------------------------------------------
__global__ __launch_bounds__(CV_NT) void cv_neighbour_kernel(CvConnBatch B) {
    __shared__ unsigned long long keys[CV_MAX_ROW];
    __shared__ int found, below;
    const int idx = blockIdx.x, it = blockIdx.y;
    if (idx >= B.n_listed[it]) return;   // the whole workgroup; n_listed <= row_cap
    LmMap M; CvIndex X;
    cv_item(B, it, M, X);
    const int k = __builtin_amdgcn_readfirstlane(B.kf[it]);
    const int j = __builtin_amdgcn_readfirstlane(X.ord_kf[(size_t)k * X.row_cap + idx]);   // a slot (b) took from the counts: inside the map, not k
    const int w = __builtin_amdgcn_readfirstlane(X.ord_w[(size_t)k * X.row_cap + idx]);
    int32_t* const ckf = X.cw_kf + (size_t)j * X.row_cap;
    int32_t* const cw = X.cw_w + (size_t)j * X.row_cap;
    int n = cv_clamp(X.cw_n[j], X.row_cap);
    if (threadIdx.x == 0) { found = -1; below = 0; }
    __syncthreads();
    int nb = 0;
    for (int e = threadIdx.x; e < n; e += CV_NT) {
        const int s = ckf[e];
        keys[e] = cv_key(cw[e], s);
        if (s == k) found = e;      // slots of a row are distinct: at most one writer
        nb += s < k;
    }
    if (nb) atomicAdd(&below, nb);
    __syncthreads();
    const int at = found, pos = below;
    if (at >= 0) {
        if ((int)(keys[at] >> 32) == w) return;   // AddConnection's `else return`: nothing of j changes
        __syncthreads();
        if (threadIdx.x == 0) { cw[at] = w; keys[at] = cv_key(w, k); }
    } else {
        if (n == X.row_cap) {
            if (threadIdx.x == 0) atomicOr(&B.status[it], CV_ROW_OVERFLOW);
            return;
        }
        // the row is in LDS: open it up at `pos` from there
        for (int e = pos + threadIdx.x; e < n; e += CV_NT) { ckf[e + 1] = (int32_t)(uint32_t)keys[e]; cw[e + 1] = (int32_t)(keys[e] >> 32); }
        __syncthreads();
        if (threadIdx.x == 0) { ckf[pos] = k; cw[pos] = w; keys[n] = cv_key(w, k); X.cw_n[j] = n + 1; }
        ++n;
    }
    __syncthreads();
    cv_place_row(X, j, keys, n);
}

// ---- KeyFrameCulling ------------------------------------------------------------------------------------------------------------
// the map of problem f, or false for a map index outside the batch's
__device__ __forceinline__ bool cv_prob(const CvCullBatch& B, int f, LmMap& M, CvIndex& X) {
    const int m = __builtin_amdgcn_readfirstlane(B.prob_map[f]);
    if ((unsigned)m >= (unsigned)B.n_maps) return false;
    M = B.maps[m]; X = B.covis[m];
    M.n_kf = min(M.n_kf, LM_MAX_KF); M.n_mp = min(M.n_mp, B.mp_cap);
    X.row_cap = cv_clamp(X.row_cap, min(CV_MAX_ROW, B.cand_cap));
    return true;
}
// ... and its current keyframe c inside the map, with the depth columns there when the problem is not monocular
__device__ __forceinline__ bool cv_prob_ready(const CvCullBatch& B, int f, LmMap& M, CvIndex& X, int& c, bool& monocular) {
    if (!cv_prob(B, f, M, X)) return false;
    c = __builtin_amdgcn_readfirstlane(B.kf[f]);
    monocular = __builtin_amdgcn_readfirstlane(B.monocular[f]) != 0;
    return lm_kf_ok(M, c) && (monocular || (X.kf_depth && X.kf_th_depth));
}

// candidate `cand` against the culled set S (null = empty), by the whole workgroup: acc[0] = nMPs, acc[1] = nRedundant in LDS.
// Every thread returns with the sums readable.
__device__ __forceinline__ void cv_eval_wg(const LmMap& M, const CvIndex& X, int cand, bool monocular, const uint32_t* S, int* acc, int& st) {
    if (threadIdx.x == 0) { acc[0] = 0; acc[1] = 0; }
    __syncthreads();
    const int e0 = M.kf_mp_ptr[cand], e1 = M.kf_mp_ptr[cand + 1];
    int nm = 0, nr = 0;
    for (int e = e0 + (int)threadIdx.x; e < e1; e += CV_NT) {
        const int r = cv_eval_point(M, X, cand, e, monocular, S, st);
        nm += r & CV_COUNTS; nr += (r & CV_REDUNDANT) != 0;
    }
    nm = cv_wave_total(nm); nr = cv_wave_total(nr);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&acc[0], nm); atomicAdd(&acc[1], nr); }
    __syncthreads();
}

// grid (cand_cap, problems), 256 threads
__global__ __launch_bounds__(CV_NT) void cv_cull_first_kernel(CvCullBatch B) {
    __shared__ int acc[2];
    const int t = blockIdx.x, f = blockIdx.y;
    LmMap M; CvIndex X;
    int c;
    bool monocular;
    if (!cv_prob_ready(B, f, M, X, c, monocular)) {
        if (t == 0 && threadIdx.x == 0) { B.n_cand[f] = 0; atomicOr(&B.status[f], CV_BAD_SLOT); }
        return;
    }
    const int n = cv_clamp(X.ord_n[c], X.row_cap);
    if (t == 0 && threadIdx.x == 0) B.n_cand[f] = n;
    if (t >= n) return;
    const int cand = __builtin_amdgcn_readfirstlane(X.ord_kf[(size_t)c * X.row_cap + t]);
    int st = 0, v = CV_KEPT, nm = 0, nr = 0;
    if (!lm_kf_ok(M, cand)) st = CV_BAD_SLOT;
    else if (cand == X.origin_kf) v = CV_ORIGIN;
    else {
        cv_eval_wg(M, X, cand, monocular, nullptr, acc, st);
        nm = acc[0]; nr = acc[1];
        v = cv_verdict(X, cand, nm, nr);
    }
    if (st) atomicOr(&B.status[f], st);
    if (threadIdx.x == 0) {
        const size_t at = (size_t)f * B.cand_cap + t;
        B.verdict[at] = (uint8_t)v; B.n_mps[at] = nm; B.n_redundant[at] = nr;
    }
}

// grid (problems), 256 threads
__global__ __launch_bounds__(CV_NT) void cv_cull_cascade_kernel(CvCullBatch B) {
    __shared__ uint32_t S[CV_SET_WORDS];
    __shared__ int acc[2];
    __shared__ int first;
    const int f = blockIdx.x;
    LmMap M; CvIndex X;
    int c;
    bool monocular;
    if (!cv_prob_ready(B, f, M, X, c, monocular)) return;   // the first pass reported it
    const int n = cv_clamp(X.ord_n[c], X.row_cap);
    if (threadIdx.x == 0) first = n;
    __syncthreads();
    uint8_t* const verdict = B.verdict + (size_t)f * B.cand_cap;
    for (int t = threadIdx.x; t < n; t += CV_NT)
        if (verdict[t] == CV_CULLED) atomicMin(&first, t);
    __syncthreads();
    const int t0 = first;
    if (t0 >= n) return;   // no cull: the first pass was the walk
    for (int w = threadIdx.x; w < (M.n_kf + 31) / 32; w += CV_NT) S[w] = 0;
    __syncthreads();
    const int32_t* const cands = X.ord_kf + (size_t)c * X.row_cap;
    if (threadIdx.x == 0) lm_mark(S, cands[t0]);   // verdict CV_CULLED: the first pass found it inside the map
    __syncthreads();
    int st = 0;
    for (int t = t0 + 1; t < n; ++t) {
        const int cand = __builtin_amdgcn_readfirstlane(cands[t]);
        if (!lm_kf_ok(M, cand) || cand == X.origin_kf) continue;   // the first pass wrote these
        cv_eval_wg(M, X, cand, monocular, S, acc, st);
        const int nm = acc[0], nr = acc[1];
        const int v = cv_verdict(X, cand, nm, nr);
        __syncthreads();   // everyone has read acc and S
        if (threadIdx.x == 0) {
            verdict[t] = (uint8_t)v; B.n_mps[(size_t)f * B.cand_cap + t] = nm; B.n_redundant[(size_t)f * B.cand_cap + t] = nr;
            if (v == CV_CULLED) lm_mark(S, cand);
        }
        __syncthreads();
    }
    if (st) atomicOr(&B.status[f], st);
    uint8_t* const turned = B.mp_turned_bad + (size_t)f * B.mp_cap;
    for (int p = threadIdx.x; p < M.n_mp; p += CV_NT)
        if (cv_turned_bad(M, X, p, S)) turned[p] = 1;
}

static hipError_t cv_launch_connections(const CvConnBatch& B, int max_row_cap, hipStream_t st) {
    hipError_t e = hipMemsetAsync(B.counts, 0, sizeof(int32_t) * (size_t)B.nitems * B.count_cap, st);
    if (e == hipSuccess) e = hipMemsetAsync(B.status, 0, sizeof(int32_t) * (size_t)B.nitems, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cv_counts_kernel, dim3(CV_COUNT_BLOCKS, B.nitems), dim3(CV_NT), 0, st, B);
    hipLaunchKernelGGL(cv_list_kernel, dim3(B.nitems), dim3(CV_NT), 0, st, B);
    hipLaunchKernelGGL(cv_neighbour_kernel, dim3(max_row_cap, B.nitems), dim3(CV_NT), 0, st, B);
    return hipGetLastError();
}

static hipError_t cv_launch_culling(const CvCullBatch& B, hipStream_t st) {
    hipError_t e = hipMemsetAsync(B.status, 0, sizeof(int32_t) * (size_t)B.nprob, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cv_cull_first_kernel, dim3(B.cand_cap, B.nprob), dim3(CV_NT), 0, st, B);
    hipLaunchKernelGGL(cv_cull_cascade_kernel, dim3(B.nprob), dim3(CV_NT), 0, st, B);
    return hipGetLastError();
}

// ---- what the host forms check before anything is launched (map_check.h) -------------------------------------------------------
// the tables both host forms read; null on success, else what is wrong
static const char* cv_host_tables(const slamit_map_index* map, const slamit_covis_index* X, int32_t k) {
    if (!map || !X) return "null table";
    if (const char* bad = map_sizes_error(map)) return bad;
    if (X->row_cap < 1 || X->row_cap > SLAMIT_COVIS_MAX_ROW) return "row_cap outside [1, SLAMIT_COVIS_MAX_ROW]";
    if (!map->obs_ptr || !map->kf_mp_ptr || (map->n_mp && !map->mp_bad)) return "null table";
    if (map->n_kf && (!X->ord_kf || !X->ord_n)) return "null table";
    if (!map_csr_ok(map->obs_ptr, map->n_mp) || !map_csr_ok(map->kf_mp_ptr, map->n_kf)) return "a CSR pointer array does not ascend from 0";
    const size_t n_obs = (size_t)map->obs_ptr[map->n_mp], n_kfmp = (size_t)map->kf_mp_ptr[map->n_kf];
    if ((n_obs && !map->obs_kf) || (n_kfmp && !map->kf_mp)) return "null table";
    if (k < 0 || k >= map->n_kf) return "the keyframe is a slot outside [0, n_kf)";
    if (X->origin_kf < -1 || X->origin_kf >= map->n_kf) return "origin_kf is a slot outside [-1, n_kf)";
    if (const char* bad = map_obs_error(map, nullptr, nullptr)) return bad;
    if (!map_slots_ok(map->kf_mp, n_kfmp, -1, map->n_mp)) return "kf_mp holds a point slot outside [-1, n_mp)";
    return nullptr;
}

extern "C" {

int slamit_update_connections(int device, const slamit_map_index* map, const slamit_covis_index* covis, int32_t k, int32_t first_connection,
                              int32_t* counts, int32_t* n_counted, int32_t* n_listed, int32_t* parent, int32_t* status) {
    const char* const where = "slamit_update_connections";
    if (!counts || !n_counted || !n_listed || !parent || !status) return slamit_refuse(where, "null array");
    if (const char* what = cv_host_tables(map, covis, k)) return slamit_refuse(where, what);
    if (!covis->cw_kf || !covis->cw_w || !covis->cw_n || !covis->ord_w) return slamit_refuse(where, "null table");
    const int n_kf = map->n_kf, n_mp = map->n_mp, row_cap = covis->row_cap;
    const size_t n_obs = (size_t)map->obs_ptr[n_mp], n_kfmp = (size_t)map->kf_mp_ptr[n_kf], rows = (size_t)n_kf * row_cap;
    SLAMIT_USE_DEVICE(device);
    CvConnBatch H;
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<CvConnBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, CvConnBatch& Q) {
            io.clear();
            Q.nitems = 1; Q.count_cap = n_kf; Q.item_map[0] = 0;
            LmMap& M = Q.maps[0];
            M.n_kf = n_kf; M.n_mp = n_mp;
            M.obs_ptr = b.in(map->obs_ptr, (size_t)n_mp + 1); M.obs_kf = b.in(map->obs_kf, n_obs); M.mp_bad = b.in(map->mp_bad, (size_t)n_mp);
            M.kf_mp_ptr = b.in(map->kf_mp_ptr, (size_t)n_kf + 1); M.kf_mp = b.in(map->kf_mp, n_kfmp);
            CvIndex& X = Q.covis[0];
            X.row_cap = row_cap; X.origin_kf = covis->origin_kf;
            X.cw_kf = slamit_inout(b, io, covis->cw_kf, rows); X.cw_w = slamit_inout(b, io, covis->cw_w, rows); X.cw_n = slamit_inout(b, io, covis->cw_n, (size_t)n_kf);
            X.ord_kf = slamit_inout(b, io, covis->ord_kf, rows); X.ord_w = slamit_inout(b, io, covis->ord_w, rows); X.ord_n = slamit_inout(b, io, covis->ord_n, (size_t)n_kf);
            X.kf_best = covis->kf_best ? slamit_inout(b, io, covis->kf_best, (size_t)n_kf * LM_BEST) : nullptr;
            int32_t* h2;
            const int32_t* const d2 = b.in_fill<int32_t>(2, &h2);   // k, first_connection
            if (h2) { h2[0] = k; h2[1] = first_connection != 0; }
            Q.kf = d2; Q.first = d2 ? d2 + 1 : nullptr;
            Q.counts = b.out(counts, (size_t)n_kf); Q.n_counted = b.out(n_counted, 1); Q.n_listed = b.out(n_listed, 1);
            Q.parent = slamit_inout(b, io, parent, 1); Q.status = b.out(status, 1);
            H = Q;
        },
        [&](const CvConnBatch*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            return e != hipSuccess ? e : cv_launch_connections(H, row_cap, S.st);
        });
}

int slamit_update_connections_batch_dev(int device, const slamit_covis_batch_rec* R, void* stream) {
    const char* const where = "slamit_update_connections_batch_dev";
    if (!R || R->nitems < 0 || R->n_maps < 0 || R->count_cap < 0) return slamit_refuse(where, "bad argument");
    if (R->nitems == 0) return SLAMIT_OK;
    if (R->n_maps < 1 || R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !R->maps || !R->covis)
        return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->nitems > R->n_maps || !R->item_map) return slamit_refuse(where, "more items than maps (one item per map) or no item_map");
    if (R->count_cap > SLAMIT_LOCAL_MAP_MAX_KF) return slamit_refuse(where, "count_cap above SLAMIT_LOCAL_MAP_MAX_KF");
    bool used[SLAMIT_LOCAL_MAP_MAX_MAPS] = {};
    int max_row_cap = 1;
    for (int i = 0; i < R->nitems; ++i) {
        const int m = R->item_map[i];
        if (m < 0 || m >= R->n_maps) return slamit_refuse(where, "item_map names a map outside [0, n_maps)");
        if (used[m]) return slamit_refuse(where, "a map is named twice in item_map: a second keyframe of a map is a second call");
        used[m] = true;
        const slamit_map_index& M = R->maps[m];
        const slamit_covis_index& X = R->covis[m];
        if (M.n_kf < 0 || M.n_mp < 0 || M.n_kf > R->count_cap) return slamit_refuse(where, "a map with n_kf above count_cap");
        if (X.row_cap < 1 || X.row_cap > SLAMIT_COVIS_MAX_ROW) return slamit_refuse(where, "row_cap outside [1, SLAMIT_COVIS_MAX_ROW]");
        if (!M.obs_ptr || !M.obs_kf || !M.mp_bad || !M.kf_mp_ptr || !M.kf_mp || !X.cw_kf || !X.cw_w || !X.cw_n || !X.ord_kf || !X.ord_w || !X.ord_n)
            return slamit_refuse(where, "null table");
        max_row_cap = std::max(max_row_cap, (int)X.row_cap);
    }
    if (!R->d_kf || !R->d_first || !R->d_counts || !R->d_n_counted || !R->d_n_listed || !R->d_parent || !R->d_status) return slamit_refuse(where, "null array");
    SLAMIT_USE_DEVICE(device);
    CvConnBatch B;
    memset(&B, 0, sizeof(B));
    B.nitems = R->nitems; B.count_cap = R->count_cap;
    memcpy(B.item_map, R->item_map, sizeof(int32_t) * (size_t)R->nitems);
    memcpy(B.maps, R->maps, sizeof(LmMap) * (size_t)R->n_maps);
    memcpy(B.covis, R->covis, sizeof(CvIndex) * (size_t)R->n_maps);
    B.kf = R->d_kf; B.first = R->d_first; B.counts = R->d_counts; B.n_counted = R->d_n_counted; B.n_listed = R->d_n_listed;
    B.parent = R->d_parent; B.status = R->d_status;
    HIP_TRY_AT(where, cv_launch_connections(B, max_row_cap, (hipStream_t)stream));
    return SLAMIT_OK;
}

int slamit_keyframe_culling(int device, const slamit_map_index* map, const slamit_covis_index* covis, int32_t c, int32_t monocular,
                            uint8_t* verdict, int32_t* n_mps, int32_t* n_redundant, int32_t* n_cand, uint8_t* mp_turned_bad, int32_t* status) {
    const char* const where = "slamit_keyframe_culling";
    if (!verdict || !n_mps || !n_redundant || !n_cand || !status || (map && map->n_mp > 0 && !mp_turned_bad)) return slamit_refuse(where, "null array");
    if (const char* what = cv_host_tables(map, covis, c)) return slamit_refuse(where, what);
    const int n_kf = map->n_kf, n_mp = map->n_mp, row_cap = covis->row_cap;
    const size_t n_obs = (size_t)map->obs_ptr[n_mp], n_kfmp = (size_t)map->kf_mp_ptr[n_kf], rows = (size_t)n_kf * row_cap;
    if (!monocular && (!covis->kf_depth || !covis->kf_th_depth)) return slamit_refuse(where, "kf_depth or kf_th_depth NULL with monocular == 0");
    if (!covis->kf_not_erase || (n_mp && !covis->mp_nobs) || (n_obs && (!covis->obs_octave || !covis->obs_weight)) || (n_kfmp && !covis->kf_octave))
        return slamit_refuse(where, "null table");
    const int n_c = std::min(std::max(covis->ord_n[c], 0), row_cap);
    if (!map_slots_ok(covis->ord_kf + (size_t)c * row_cap, (size_t)n_c, 0, n_kf)) return slamit_refuse(where, "the candidates hold a keyframe slot outside [0, n_kf)");
    SLAMIT_USE_DEVICE(device);
    CvCullBatch H;
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<CvCullBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, CvCullBatch& Q) {
            io.clear();
            Q.nprob = 1; Q.n_maps = 1; Q.cand_cap = row_cap; Q.mp_cap = n_mp;
            LmMap& M = Q.maps[0];
            M.n_kf = n_kf; M.n_mp = n_mp;
            M.obs_ptr = b.in(map->obs_ptr, (size_t)n_mp + 1); M.obs_kf = b.in(map->obs_kf, n_obs); M.mp_bad = b.in(map->mp_bad, (size_t)n_mp);
            M.kf_mp_ptr = b.in(map->kf_mp_ptr, (size_t)n_kf + 1); M.kf_mp = b.in(map->kf_mp, n_kfmp);
            CvIndex& X = Q.covis[0];
            X.row_cap = row_cap; X.origin_kf = covis->origin_kf;
            X.obs_octave = b.in(covis->obs_octave, n_obs); X.obs_weight = b.in(covis->obs_weight, n_obs); X.mp_nobs = b.in(covis->mp_nobs, (size_t)n_mp);
            X.kf_octave = b.in(covis->kf_octave, n_kfmp);
            if (!monocular) { X.kf_depth = b.in(covis->kf_depth, n_kfmp); X.kf_th_depth = b.in(covis->kf_th_depth, (size_t)n_kf); }
            X.kf_not_erase = b.in(covis->kf_not_erase, (size_t)n_kf);
            X.ord_kf = const_cast<int32_t*>(b.in(covis->ord_kf, rows)); X.ord_n = const_cast<int32_t*>(b.in(covis->ord_n, (size_t)n_kf));
            int32_t* h3;
            const int32_t* const d3 = b.in_fill<int32_t>(3, &h3);   // prob_map, c, monocular
            if (h3) { h3[0] = 0; h3[1] = c; h3[2] = monocular != 0; }
            Q.prob_map = d3; Q.kf = d3 ? d3 + 1 : nullptr; Q.monocular = d3 ? d3 + 2 : nullptr;
            Q.verdict = slamit_inout(b, io, verdict, (size_t)row_cap); Q.n_mps = slamit_inout(b, io, n_mps, (size_t)row_cap);
            Q.n_redundant = slamit_inout(b, io, n_redundant, (size_t)row_cap); Q.n_cand = b.out(n_cand, 1);
            Q.mp_turned_bad = slamit_inout(b, io, mp_turned_bad, (size_t)n_mp); Q.status = b.out(status, 1);
            H = Q;
        },
        [&](const CvCullBatch*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            return e != hipSuccess ? e : cv_launch_culling(H, S.st);
        });
}

int slamit_keyframe_culling_batch_dev(int device, const slamit_culling_batch_rec* R, void* stream) {
    const char* const where = "slamit_keyframe_culling_batch_dev";
    if (!R || R->nprob < 0 || R->n_maps < 0 || R->cand_cap < 0 || R->mp_cap < 0) return slamit_refuse(where, "bad argument");
    if (R->nprob == 0) return SLAMIT_OK;
    if (R->nprob > 65535) return slamit_refuse(where, "more than 65535 problems");
    if (R->n_maps < 1 || R->n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !R->maps || !R->covis)
        return slamit_refuse(where, "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps");
    if (R->cand_cap < 1 || R->cand_cap > SLAMIT_COVIS_MAX_ROW) return slamit_refuse(where, "cand_cap outside [1, SLAMIT_COVIS_MAX_ROW]");
    for (int m = 0; m < R->n_maps; ++m) {
        const slamit_map_index& M = R->maps[m];
        const slamit_covis_index& X = R->covis[m];
        if (M.n_kf < 0 || M.n_mp < 0 || M.n_kf > SLAMIT_LOCAL_MAP_MAX_KF || M.n_mp > R->mp_cap) return slamit_refuse(where, "a map with n_kf above SLAMIT_LOCAL_MAP_MAX_KF or n_mp above mp_cap");
        if (X.row_cap < 1 || X.row_cap > R->cand_cap) return slamit_refuse(where, "row_cap outside [1, cand_cap]");
        if (!M.obs_ptr || !M.obs_kf || !M.mp_bad || !M.kf_mp_ptr || !M.kf_mp || !X.obs_octave || !X.obs_weight || !X.mp_nobs || !X.kf_octave ||
            !X.kf_not_erase || !X.ord_kf || !X.ord_n || (!X.kf_depth) != (!X.kf_th_depth))
            return slamit_refuse(where, "null table");
    }
    if (!R->d_prob_map || !R->d_kf || !R->d_monocular || !R->d_verdict || !R->d_n_mps || !R->d_n_redundant || !R->d_n_cand || !R->d_mp_turned_bad || !R->d_status)
        return slamit_refuse(where, "null array");
    SLAMIT_USE_DEVICE(device);
    CvCullBatch B;
    memset(&B, 0, sizeof(B));
    B.nprob = R->nprob; B.n_maps = R->n_maps; B.cand_cap = R->cand_cap; B.mp_cap = R->mp_cap;
    memcpy(B.maps, R->maps, sizeof(LmMap) * (size_t)R->n_maps);
    memcpy(B.covis, R->covis, sizeof(CvIndex) * (size_t)R->n_maps);
    B.prob_map = R->d_prob_map; B.kf = R->d_kf; B.monocular = R->d_monocular; B.verdict = R->d_verdict; B.n_mps = R->d_n_mps;
    B.n_redundant = R->d_n_redundant; B.n_cand = R->d_n_cand; B.mp_turned_bad = R->d_mp_turned_bad; B.status = R->d_status;
    HIP_TRY_AT(where, cv_launch_culling(B, (hipStream_t)stream));
    return SLAMIT_OK;
}

}  // extern "C"
