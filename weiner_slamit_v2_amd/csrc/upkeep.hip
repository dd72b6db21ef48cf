// upkeep.hip — MapPoint::UpdateNormalAndDepth, MapPoint::ComputeDistinctiveDescriptors and LocalMapping::MapPointCulling on the GPU
// (include/slamit.h, slamit_update_points* and slamit_map_point_culling*; the walks are stated in upkeep.h, whose per-point functions
// the kernels call).
//
// up_points_kernel     one wavefront per listed point.  Lanes gather the point's row of obs_kf as keys slot << 10 | position into LDS
//                      and place every key by its rank, so the row stands in ascending slot whatever order it was stored in.  Each
//                      lane computes its observers' contributions to the normal -- they are independent of one another -- and stores
//                      them at the rank; ONE ordered pass then adds them, the float sum being sequential in the reference.  The
//                      descriptors of the non-bad observers go to LDS in the same order (ballot + scan) for distinctive.h's all-pairs
//                      Hamming and median by bisection, shared with distinctive_kernel.
//                      LDS BY CLASS OF n: a typical point has 3-20 observers, and the 36 KiB of the descriptor pass at 128 rows would
//                      cap a CU at four such wavefronts.  The kernel is instantiated for rows of at most UP_SMALL observers (3.7 KiB)
//                      and for the rest up to UP_MAX_OBS (46 KiB); both run over the whole list and a wavefront leaves at once when
//                      its point belongs to the other class.  Against the large class alone (up_points_kernel<UP_MAX_OBS,
//                      UP_MAX_DESC, 0, true> over everything) the two classes took half the time: profiles/r25_upkeep.json,
//                      DESIGN.md section 25.
// up_culling_kernel    one workgroup per recent list: the predicate per lane, the kept entries compacted in list order by the wave scan
//                      of wave_ops.h and the four wave totals through LDS.
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
#include "distinctive.h"
#include "upkeep.h"

static_assert(sizeof(UpIndex) == sizeof(slamit_point_index) && offsetof(UpIndex, scale_factors) == offsetof(slamit_point_index, scale_factors) &&
                  offsetof(UpIndex, obs_idx) == offsetof(slamit_point_index, obs_idx) && offsetof(UpIndex, kf_desc) == offsetof(slamit_point_index, kf_desc) &&
                  offsetof(UpIndex, mp_ref_kf) == offsetof(slamit_point_index, mp_ref_kf) && offsetof(UpIndex, mp_first_kf) == offsetof(slamit_point_index, mp_first_kf) &&
                  offsetof(UpIndex, mp_normal) == offsetof(slamit_point_index, mp_normal) && offsetof(UpIndex, mp_desc) == offsetof(slamit_point_index, mp_desc),
              "slamit_point_index is UpIndex");
static_assert(sizeof(LmMap) == sizeof(slamit_map_index), "slamit_map_index is LmMap");
static_assert(UP_REF_NOT_OBSERVER == SLAMIT_UPKEEP_REF_NOT_OBSERVER && UP_NO_REF == SLAMIT_UPKEEP_NO_REF && UP_REF_NO_KP == SLAMIT_UPKEEP_REF_NO_KP &&
                  UP_OCTAVE == SLAMIT_UPKEEP_OCTAVE && UP_DESC_OVERFLOW == SLAMIT_UPKEEP_DESC_OVERFLOW && UP_OBS_OVERFLOW == SLAMIT_UPKEEP_OBS_OVERFLOW &&
                  UP_BAD_SLOT == SLAMIT_UPKEEP_BAD_SLOT && UP_MAX_OBS == SLAMIT_UPKEEP_MAX_OBS && UP_MAX_DESC == SLAMIT_DISTINCTIVE_MAX &&
                  UP_MAX_POINTS == SLAMIT_UPKEEP_MAX_POINTS && UP_MAX_RECENT == SLAMIT_UPKEEP_MAX_RECENT && UP_NORMAL == SLAMIT_UPKEEP_NORMAL &&
                  UP_DESC == SLAMIT_UPKEEP_DESC && UP_KEPT == SLAMIT_UPKEEP_KEPT && UP_WAS_BAD == SLAMIT_UPKEEP_WAS_BAD && UP_LOW_RATIO == SLAMIT_UPKEEP_LOW_RATIO &&
                  UP_FEW_OBS == SLAMIT_UPKEEP_FEW_OBS && UP_AGED == SLAMIT_UPKEEP_AGED && UNP_MAX_LEVELS == SLAMIT_MAX_LEVELS,
              "upkeep.h restates the C-ABI's constants");
static_assert(UP_MAX_OBS <= (1 << UP_KEY_SHIFT) && LM_MAX_KF < (1 << (32 - UP_KEY_SHIFT)), "an order key holds a slot and a position");

#define UP_SMALL 32           // observers of the small LDS class
#define UP_NT 256             // threads of the culling workgroup

// The batches as the kernels' argument: the maps' records travel with them, the arrays stay where the caller keeps them.
struct UpBatch {
    int32_t nitems, n_maps, cap, reserved;
    LmMap maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    UpIndex pts[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const int32_t* item_map; const int32_t* n; const int32_t* what; const int32_t* points;
    int32_t* status;
};
struct UpCullBatch {
    int32_t nlists, n_maps, cap, reserved;
    LmMap maps[SLAMIT_LOCAL_MAP_MAX_MAPS];
    UpIndex pts[SLAMIT_LOCAL_MAP_MAX_MAPS];
    const int32_t* list_map; const int32_t* cur_id; const int32_t* monocular; const int32_t* n; const int32_t* recent;
    uint8_t* verdict; int32_t* kept; int32_t* n_kept; int32_t* status;
};

// ---- grid (cap, items), 64 threads.  This instantiation takes the points with LO < observers <= ROWS; the one with LO == 0 also
// reports what has no row (a map or a point outside its table), the LAST one the rows above UP_MAX_OBS. --------------------------
template <int ROWS, int DROWS, int LO, bool LAST>
__global__ __launch_bounds__(64) void up_points_kernel(UpBatch B) {
    static_assert(!LAST || ROWS == UP_MAX_OBS, "the last class ends at the ceiling");
    static_assert(DROWS <= UP_MAX_DESC && DROWS <= ROWS, "descriptor rows");
    __shared__ uint32_t keys[ROWS];           // as gathered: slot << 10 | position, ~0 for a slot outside the map
    __shared__ uint32_t skeys[ROWS];          // by rank
    __shared__ float con[3][ROWS];            // the contributions to the normal, by rank
    __shared__ uint4 rowsd[DROWS * 2];
    __shared__ unsigned short D[DROWS * DROWS];
    const int it = blockIdx.y, j = blockIdx.x, lane = threadIdx.x;
    const int cap = min(B.cap, UP_MAX_POINTS);
    if (j >= min(B.n[it], cap)) return;       // the whole wavefront, here and at every return below
    int32_t* const status = B.status + (size_t)it * B.cap + j;
    const int m = __builtin_amdgcn_readfirstlane(B.item_map[it]);
    if ((unsigned)m >= (unsigned)B.n_maps) {
        if (LO == 0 && lane == 0) *status = UP_BAD_SLOT;
        return;
    }
    LmMap M = B.maps[m];
    const UpIndex& X = B.pts[m];             // read where it lies: scale_factors is indexed by the level
    M.n_kf = min(M.n_kf, LM_MAX_KF);
    const int p = __builtin_amdgcn_readfirstlane(B.points[(size_t)it * B.cap + j]);
    if (!lm_mp_ok(M, p)) {
        if (LO == 0 && lane == 0) *status = UP_BAD_SLOT;
        return;
    }
    const int o0 = __builtin_amdgcn_readfirstlane(M.obs_ptr[p]), n_all = __builtin_amdgcn_readfirstlane(M.obs_ptr[p + 1]) - o0;
    if ((LO > 0 && n_all <= LO) || (!LAST && n_all > ROWS)) return;   // the other class's
    if (M.mp_bad[p] || n_all <= 0) {
        if (lane == 0) *status = 0;
        return;
    }
    if (n_all > ROWS) {                       // LAST only: above UP_MAX_OBS
        if (lane == 0) *status = UP_OBS_OVERFLOW;
        return;
    }
    const int what = __builtin_amdgcn_readfirstlane(B.what[it]);
    int st = 0, n = 0;                        // wave-uniform
    int lst = 0;                              // this lane's
    for (int e0 = 0; e0 < n_all; e0 += 64) {
        const int e = e0 + lane;
        uint32_t key = ~0u;
        if (e < n_all) {
            const int k = M.obs_kf[o0 + e];
            if (lm_kf_ok(M, k)) key = up_key(k, e); else lst |= UP_BAD_SLOT;
            keys[e] = key;                    // e < n_all <= ROWS
        }
        n += __popcll(__ballot(key != ~0u));
    }
    wave_mem_sync();
    for (int e = lane; e < n_all; e += 64) {
        const uint32_t key = keys[e];
        if (key == ~0u) continue;
        int r = 0;                            // keys are distinct: r < n is this observation's place in ascending (slot, position)
        for (int f = 0; f < n_all; ++f) r += keys[f] < key;
        skeys[r] = key;
        if (what & UP_NORMAL) {
            float c[3];
            up_contribution(M.mp_pos + 3 * (size_t)p, X.kf_center + 3 * (size_t)up_key_slot(key), c);
            con[0][r] = c[0]; con[1][r] = c[1]; con[2][r] = c[2];
        }
    }
    wave_mem_sync();
    if (n > 0 && (what & UP_NORMAL)) {
        const int ref = __builtin_amdgcn_readfirstlane(X.mp_ref_kf[p]);
        int o_ref = -1;                       // the first observation of the reference keyframe in the order above
        for (int r0 = 0; r0 < n && o_ref < 0; r0 += 64) {
            const int r = r0 + lane;
            const unsigned long long hit = __ballot(r < n && up_key_slot(skeys[min(r, n - 1)]) == ref);
            if (hit) o_ref = o0 + up_key_pos(skeys[r0 + __ffsll((long long)hit) - 1]);
        }
        int level;
        const int rs = up_ref_level(M, X, ref, o_ref, level);
        st |= rs;
        if (!(rs & (UP_NO_REF | UP_REF_NO_KP | UP_OCTAVE | UP_BAD_SLOT))) {
            float sum[3] = {0.f, 0.f, 0.f};   // every lane takes the same ordered sum from LDS
            for (int i = 0; i < n; ++i) { sum[0] = sum[0] + con[0][i]; sum[1] = sum[1] + con[1][i]; sum[2] = sum[2] + con[2][i]; }
            if (lane == 0) up_store_normal(M, X, p, ref, level, sum, n);
        }
    }
    if (n > 0 && (what & UP_DESC)) {
        int N = 0;
        for (int r0 = 0; r0 < n; r0 += 64) {
            const int r = r0 + lane;
            bool good = false;
            int k = 0, o = 0;
            if (r < n) {
                k = up_key_slot(skeys[r]); o = o0 + up_key_pos(skeys[r]);
                good = up_desc_row(M, X, k, o, lst);
            }
            const int g = N + wave_inclusive_scan_i32(good ? 1 : 0) - 1;
            if (good && g < DROWS) {
                const uint4* const src = reinterpret_cast<const uint4*>(up_desc_of(M, X, k, o));
                rowsd[2 * g] = src[0]; rowsd[2 * g + 1] = src[1];
            }
            N += __popcll(__ballot(good));
        }
        if (N > DROWS) st |= UP_DESC_OVERFLOW;   // DROWS == UP_MAX_DESC wherever a row can hold more
        else if (N > 0) {
            wave_mem_sync();
            DISTINCTIVE_SELECT(rowsd, D, N, lane, bestkey)
            const int b = (int)(bestkey & 0xFFFFu);
            if (lane < 2) reinterpret_cast<uint4*>(X.mp_desc + 32 * (size_t)p)[lane] = rowsd[2 * b + lane];
        }
    }
    if (__ballot(lst != 0)) st |= UP_BAD_SLOT;
    if (lane == 0) *status = st;
}

// ---- grid (lists), 256 threads ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UP_NT) void up_culling_kernel(UpCullBatch B) {
    __shared__ int wave_total[UP_NT / 64];
    const int f = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = __builtin_amdgcn_readfirstlane(B.list_map[f]);
    if ((unsigned)m >= (unsigned)B.n_maps) {
        if (threadIdx.x == 0) { B.n_kept[f] = 0; B.status[f] = UP_BAD_SLOT; }
        return;
    }
    const LmMap& M = B.maps[m];
    const UpIndex& X = B.pts[m];
    const int n = min(max(B.n[f], 0), min(B.cap, UP_MAX_RECENT));
    const int cur = B.cur_id[f];
    const bool monocular = B.monocular[f] != 0;
    const int32_t* const recent = B.recent + (size_t)f * B.cap;
    uint8_t* const verdict = B.verdict + (size_t)f * B.cap;
    int32_t* const kept = B.kept + (size_t)f * B.cap;
    int base = 0, bad = 0;
    for (int j0 = 0; j0 < n; j0 += UP_NT) {   // every thread walks the same rounds
        const int j = j0 + (int)threadIdx.x;
        int p = -1, v = -1;
        if (j < n) {
            p = recent[j];
            if (lm_mp_ok(M, p)) { v = up_cull_verdict(M, X, p, cur, monocular); verdict[j] = (uint8_t)v; }
            else bad = 1;
        }
        const bool keep = v == UP_KEPT;
        const int incl = wave_inclusive_scan_i32(keep ? 1 : 0);
        if (lane == 63) wave_total[w] = incl;
        __syncthreads();
        int off = base, total = 0;
        for (int u = 0; u < UP_NT / 64; ++u) { const int t = wave_total[u]; off += u < w ? t : 0; total += t; }
        if (keep) kept[off + incl - 1] = p;   // off + incl <= the entries looked at so far <= n <= cap
        base += total;
        __syncthreads();
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) { B.n_kept[f] = base; B.status[f] = bad ? UP_BAD_SLOT : 0; }
}

static hipError_t up_launch_points(const UpBatch& B, hipStream_t st) {
    const dim3 grid(B.cap, B.nitems);
    hipLaunchKernelGGL((up_points_kernel<UP_SMALL, UP_SMALL, 0, false>), grid, dim3(64), 0, st, B);
    hipLaunchKernelGGL((up_points_kernel<UP_MAX_OBS, UP_MAX_DESC, UP_SMALL, true>), grid, dim3(64), 0, st, B);
    return hipGetLastError();
}
static hipError_t up_launch_culling(const UpCullBatch& B, hipStream_t st) {
    hipLaunchKernelGGL(up_culling_kernel, dim3(B.nlists), dim3(UP_NT), 0, st, B);
    return hipGetLastError();
}

// ---- what the host forms check before anything is launched (map_check.h) -------------------------------------------------------
// the map's sizes and the CSR arrays a host form walks; null on success, else what is wrong
static const char* up_host_map(const slamit_map_index* map, const slamit_point_index* X) {
    if (!map || !X) return "null table";
    if (const char* bad = map_sizes_error(map)) return bad;
    if (map->n_mp && !map->mp_bad) return "null table";
    return nullptr;
}
// what a batch record shows the host
static const char* up_batch_maps(int n_maps, const slamit_map_index* maps, const slamit_point_index* pts, bool culling) {
    if (n_maps < 1 || n_maps > SLAMIT_LOCAL_MAP_MAX_MAPS || !maps || !pts) return "n_maps outside [1, SLAMIT_LOCAL_MAP_MAX_MAPS] or no maps";
    for (int m = 0; m < n_maps; ++m) {
        const slamit_map_index& M = maps[m];
        const slamit_point_index& X = pts[m];
        if (const char* bad = map_batch_sizes_error(&M)) return bad;
        if (culling) {
            if (!M.mp_bad || !X.mp_nobs || !X.mp_found || !X.mp_visible || !X.mp_first_kf) return "null table";
            continue;
        }
        if (X.n_levels < 1 || X.n_levels > SLAMIT_MAX_LEVELS) return "n_levels outside [1, SLAMIT_MAX_LEVELS]";
        if (!M.obs_ptr || !M.obs_kf || !M.mp_bad || !M.kf_bad || !M.kf_mp_ptr || !M.mp_pos || !X.obs_idx || !X.obs_octave || !X.kf_octave || !X.kf_center ||
            !X.kf_desc || !X.mp_ref_kf || !X.mp_normal || !X.mp_max_dist || !X.mp_min_dist || !X.mp_desc)
            return "null table";
        if (((uintptr_t)X.kf_desc | (uintptr_t)X.mp_desc) & 15) return "kf_desc or mp_desc not 16-byte aligned";
    }
    return nullptr;
}

extern "C" {

int slamit_update_points(int device, const slamit_map_index* map, const slamit_point_index* pts, int32_t n, const int32_t* points, int32_t what,
                         int32_t* status) {
    const char* const where = "slamit_update_points";
    if (n < 0 || (n && (!points || !status))) return slamit_refuse(where, "null array or negative n");
    if (what < 1 || what > (UP_NORMAL | UP_DESC)) return slamit_refuse(where, "`what` outside 1..3");
    if (n > SLAMIT_UPKEEP_MAX_POINTS) return slamit_refuse(where, "more than SLAMIT_UPKEEP_MAX_POINTS points", SLAMIT_ERR_CAPACITY);
    if (const char* bad = up_host_map(map, pts)) return slamit_refuse(where, bad);
    if (pts->n_levels < 1 || pts->n_levels > SLAMIT_MAX_LEVELS) return slamit_refuse(where, "n_levels outside [1, SLAMIT_MAX_LEVELS]");
    const int n_kf = map->n_kf, n_mp = map->n_mp;
    if (!map->obs_ptr || !map->kf_mp_ptr) return slamit_refuse(where, "null table");
    if (!map_csr_ok(map->obs_ptr, n_mp) || !map_csr_ok(map->kf_mp_ptr, n_kf)) return slamit_refuse(where, "a CSR pointer array does not ascend from 0");
    const size_t n_obs = (size_t)map->obs_ptr[n_mp], n_kfmp = (size_t)map->kf_mp_ptr[n_kf];
    if (n_obs && !map->obs_kf) return slamit_refuse(where, "null table");
    const bool nrm = (what & UP_NORMAL) != 0, dsc = (what & UP_DESC) != 0;
    if (nrm && ((n_obs && !pts->obs_octave) || (n_kfmp && !pts->kf_octave) || (n_kf && !pts->kf_center) ||
                (n_mp && (!pts->mp_ref_kf || !map->mp_pos || !pts->mp_normal || !pts->mp_max_dist || !pts->mp_min_dist))))
        return slamit_refuse(where, "null table");
    if (dsc && ((n_kf && !map->kf_bad) || (n_obs && !pts->obs_idx) || (n_kfmp && !pts->kf_desc) || (n_mp && !pts->mp_desc))) return slamit_refuse(where, "null table");
    if (!map_slots_ok(points, (size_t)n, 0, n_mp)) return slamit_refuse(where, "points holds a point slot outside [0, n_mp)");
    if (const char* bad = map_obs_error(map, dsc ? pts->obs_idx : nullptr, nullptr)) return slamit_refuse(where, bad);   // no weights here
    if (nrm && !map_slots_ok(pts->mp_ref_kf, (size_t)n_mp, -1, n_kf)) return slamit_refuse(where, "mp_ref_kf holds a keyframe slot outside [-1, n_kf)");
    if (n == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    UpBatch H;
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<UpBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, UpBatch& Q) {
            io.clear();
            Q.nitems = 1; Q.n_maps = 1; Q.cap = n;
            LmMap& M = Q.maps[0];
            M.n_kf = n_kf; M.n_mp = n_mp;
            M.obs_ptr = b.in(map->obs_ptr, (size_t)n_mp + 1); M.obs_kf = b.in(map->obs_kf, n_obs); M.mp_bad = b.in(map->mp_bad, (size_t)n_mp);
            M.kf_mp_ptr = b.in(map->kf_mp_ptr, (size_t)n_kf + 1);
            UpIndex& X = Q.pts[0];
            X.n_levels = pts->n_levels;
            memcpy(X.scale_factors, pts->scale_factors, sizeof(X.scale_factors));
            if (nrm) {
                M.mp_pos = b.in(map->mp_pos, 3 * (size_t)n_mp);
                X.obs_octave = b.in(pts->obs_octave, n_obs); X.kf_octave = b.in(pts->kf_octave, n_kfmp); X.kf_center = b.in(pts->kf_center, 3 * (size_t)n_kf);
                X.mp_ref_kf = b.in(pts->mp_ref_kf, (size_t)n_mp);
                X.mp_normal = slamit_inout(b, io, pts->mp_normal, 3 * (size_t)n_mp); X.mp_max_dist = slamit_inout(b, io, pts->mp_max_dist, (size_t)n_mp);
                X.mp_min_dist = slamit_inout(b, io, pts->mp_min_dist, (size_t)n_mp);
            }
            if (dsc) {
                M.kf_bad = b.in(map->kf_bad, (size_t)n_kf);
                X.obs_idx = b.in(pts->obs_idx, n_obs); X.kf_desc = b.in(pts->kf_desc, 32 * n_kfmp);
                X.mp_desc = slamit_inout(b, io, pts->mp_desc, 32 * (size_t)n_mp);
            }
            int32_t* h3;
            const int32_t* const d3 = b.in_fill<int32_t>(3, &h3);   // item_map, n, what
            if (h3) { h3[0] = 0; h3[1] = n; h3[2] = what; }
            Q.item_map = d3; Q.n = d3 ? d3 + 1 : nullptr; Q.what = d3 ? d3 + 2 : nullptr;
            Q.points = b.in(points, (size_t)n); Q.status = b.out(status, (size_t)n);
            H = Q;
        },
        [&](const UpBatch*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            return e != hipSuccess ? e : up_launch_points(H, S.st);
        });
}

int slamit_update_points_batch_dev(int device, const slamit_points_batch_rec* R, void* stream) {
    const char* const where = "slamit_update_points_batch_dev";
    if (!R || R->nitems < 0 || R->n_maps < 0 || R->cap < 0) return slamit_refuse(where, "bad argument");
    if (R->nitems == 0 || R->cap == 0) return SLAMIT_OK;
    if (R->nitems > 65535) return slamit_refuse(where, "more than 65535 items", SLAMIT_ERR_CAPACITY);
    if (R->cap > SLAMIT_UPKEEP_MAX_POINTS) return slamit_refuse(where, "cap above SLAMIT_UPKEEP_MAX_POINTS", SLAMIT_ERR_CAPACITY);
    if ((size_t)R->cap * (size_t)R->nitems > ((size_t)1 << 25)) return slamit_refuse(where, "more than 2^25 list entries (nitems x cap) in one call", SLAMIT_ERR_CAPACITY);
    if (const char* bad = up_batch_maps(R->n_maps, R->maps, R->pts, false)) return slamit_refuse(where, bad);
    if (!R->d_item_map || !R->d_n || !R->d_what || !R->d_points || !R->d_status) return slamit_refuse(where, "null array");
    SLAMIT_USE_DEVICE(device);
    UpBatch B;
    memset(&B, 0, sizeof(B));
    B.nitems = R->nitems; B.n_maps = R->n_maps; B.cap = R->cap;
    memcpy(B.maps, R->maps, sizeof(LmMap) * (size_t)R->n_maps);
    memcpy(B.pts, R->pts, sizeof(UpIndex) * (size_t)R->n_maps);
    B.item_map = R->d_item_map; B.n = R->d_n; B.what = R->d_what; B.points = R->d_points; B.status = R->d_status;
    HIP_TRY_AT(where, up_launch_points(B, (hipStream_t)stream));
    return SLAMIT_OK;
}

int slamit_map_point_culling(int device, const slamit_map_index* map, const slamit_point_index* pts, int32_t cur_id, int32_t monocular, int32_t n,
                             const int32_t* recent, uint8_t* verdict, int32_t* kept, int32_t* n_kept, int32_t* status) {
    const char* const where = "slamit_map_point_culling";
    if (n < 0 || !n_kept || !status || (n && (!recent || !verdict || !kept))) return slamit_refuse(where, "null array or negative n");
    if (n > SLAMIT_UPKEEP_MAX_RECENT) return slamit_refuse(where, "more than SLAMIT_UPKEEP_MAX_RECENT entries", SLAMIT_ERR_CAPACITY);
    if (const char* bad = up_host_map(map, pts)) return slamit_refuse(where, bad);
    const int n_mp = map->n_mp;
    if (n_mp && (!pts->mp_nobs || !pts->mp_found || !pts->mp_visible || !pts->mp_first_kf)) return slamit_refuse(where, "null table");
    if (!map_slots_ok(recent, (size_t)n, 0, n_mp)) return slamit_refuse(where, "recent holds a point slot outside [0, n_mp)");
    SLAMIT_USE_DEVICE(device);
    UpCullBatch H;
    std::vector<SlamitInOut> io;
    static thread_local SlamitScratch S;
    return slamit_staged_batch<UpCullBatch>(
        where, S, device, 1,
        [&](StageBinder& b, int, UpCullBatch& Q) {
            io.clear();
            Q.nlists = 1; Q.n_maps = 1; Q.cap = n;
            LmMap& M = Q.maps[0];
            M.n_kf = map->n_kf; M.n_mp = n_mp;
            M.mp_bad = b.in(map->mp_bad, (size_t)n_mp);
            UpIndex& X = Q.pts[0];
            X.mp_nobs = b.in(pts->mp_nobs, (size_t)n_mp); X.mp_found = b.in(pts->mp_found, (size_t)n_mp); X.mp_visible = b.in(pts->mp_visible, (size_t)n_mp);
            X.mp_first_kf = b.in(pts->mp_first_kf, (size_t)n_mp);
            int32_t* h4;
            const int32_t* const d4 = b.in_fill<int32_t>(4, &h4);   // list_map, cur_id, monocular, n
            if (h4) { h4[0] = 0; h4[1] = cur_id; h4[2] = monocular != 0; h4[3] = n; }
            Q.list_map = d4; Q.cur_id = d4 ? d4 + 1 : nullptr; Q.monocular = d4 ? d4 + 2 : nullptr; Q.n = d4 ? d4 + 3 : nullptr;
            Q.recent = b.in(recent, (size_t)n);
            Q.verdict = slamit_inout(b, io, verdict, (size_t)n); Q.kept = slamit_inout(b, io, kept, (size_t)n);
            Q.n_kept = b.out(n_kept, 1); Q.status = b.out(status, 1);
            H = Q;
        },
        [&](const UpCullBatch*) {
            const hipError_t e = slamit_copy_inouts(io, S.st);
            return e != hipSuccess ? e : up_launch_culling(H, S.st);
        });
}

int slamit_map_point_culling_batch_dev(int device, const slamit_point_culling_batch_rec* R, void* stream) {
    const char* const where = "slamit_map_point_culling_batch_dev";
    if (!R || R->nlists < 0 || R->n_maps < 0 || R->cap < 0) return slamit_refuse(where, "bad argument");
    if (R->nlists == 0) return SLAMIT_OK;
    if (R->cap > SLAMIT_UPKEEP_MAX_RECENT) return slamit_refuse(where, "cap above SLAMIT_UPKEEP_MAX_RECENT", SLAMIT_ERR_CAPACITY);
    if (const char* bad = up_batch_maps(R->n_maps, R->maps, R->pts, true)) return slamit_refuse(where, bad);
    if (!R->d_list_map || !R->d_cur_id || !R->d_monocular || !R->d_n || !R->d_n_kept || !R->d_status || (R->cap && (!R->d_recent || !R->d_verdict || !R->d_kept)))
        return slamit_refuse(where, "null array");
    SLAMIT_USE_DEVICE(device);
    UpCullBatch B;
    memset(&B, 0, sizeof(B));
    B.nlists = R->nlists; B.n_maps = R->n_maps; B.cap = R->cap;
    memcpy(B.maps, R->maps, sizeof(LmMap) * (size_t)R->n_maps);
    memcpy(B.pts, R->pts, sizeof(UpIndex) * (size_t)R->n_maps);
    B.list_map = R->d_list_map; B.cur_id = R->d_cur_id; B.monocular = R->d_monocular; B.n = R->d_n; B.recent = R->d_recent;
    B.verdict = R->d_verdict; B.kept = R->d_kept; B.n_kept = R->d_n_kept; B.status = R->d_status;
    HIP_TRY_AT(where, up_launch_culling(B, (hipStream_t)stream));
    return SLAMIT_OK;
}

}  // extern "C"
