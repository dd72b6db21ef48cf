// map_check.h — what a valid map table is, for the host forms of the map modules (local_map, covis, upkeep, map_edit, map_replace,
// map_fuse, kf_erase): the one statement between a caller's host pointers and a kernel that dereferences them.  Plain C++11 over
// include/slamit.h, no HIP: tests/test_map_check.py builds it with g++.
//
// Every *_error function returns nullptr, or the text of what is wrong without the "where: " prefix; the entry point hands it to
// slamit_refuse (slamit_internal.h).  What is per entry point stays there: its null tests and the walk over its own op list.  The
// functions read only the arrays they name; the caller has tested those for null wherever their length is not zero.
#ifndef SLAMIT_MAP_CHECK_H
#define SLAMIT_MAP_CHECK_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/slamit.h"

// a CSR pointer array of rows + 1 entries ascends from 0
static inline bool map_csr_ok(const int32_t* ptr, int rows) {
    if (ptr[0] != 0) return false;
    for (int r = 0; r < rows; ++r)
        if (ptr[r + 1] < ptr[r]) return false;
    return true;
}
// every one of v[count] lies in [lo, n)
static inline bool map_slots_ok(const int32_t* v, size_t count, int lo, int n) {
    for (size_t i = 0; i < count; ++i)
        if (v[i] < lo || v[i] >= n) return false;
    return true;
}

static inline bool map_sizes_ok(const slamit_map_index* map) { return map->n_kf >= 0 && map->n_mp >= 0 && map->n_kf <= SLAMIT_LOCAL_MAP_MAX_KF; }
static inline const char* map_sizes_error(const slamit_map_index* map) {
    return map_sizes_ok(map) ? nullptr : "n_kf outside [0, SLAMIT_LOCAL_MAP_MAX_KF] or negative n_mp";
}
// the same for one map of a batch record
static inline const char* map_batch_sizes_error(const slamit_map_index* map) {
    return map_sizes_ok(map) ? nullptr : "a map with n_kf outside [0, SLAMIT_LOCAL_MAP_MAX_KF] or negative n_mp";
}

// The observation table, entry by entry: obs_kf in [0, n_kf), obs_idx inside its keyframe's row, obs_weight 1 or 2.  A null obs_idx
// or obs_weight skips that test.  obs_ptr and kf_mp_ptr have passed map_csr_ok.
static inline const char* map_obs_error(const slamit_map_index* map, const int32_t* obs_idx, const uint8_t* obs_weight) {
    const size_t n_obs = (size_t)map->obs_ptr[map->n_mp];
    for (size_t o = 0; o < n_obs; ++o) {
        const int k = map->obs_kf[o];
        if (k < 0 || k >= map->n_kf) return "obs_kf holds a keyframe slot outside [0, n_kf)";
        if (obs_idx && (obs_idx[o] < 0 || obs_idx[o] >= map->kf_mp_ptr[k + 1] - map->kf_mp_ptr[k])) return "obs_idx holds a keypoint index outside its keyframe's row";
        if (obs_weight && obs_weight[o] != 1 && obs_weight[o] != 2) return "obs_weight holds a weight other than 1 or 2";
    }
    return nullptr;
}

// The pair slamit_map_index + slamit_replace_index of a host form (map_replace, map_fuse), from the two records themselves through
// map_obs_error, in the order the entry points have always tested.  touched: the entry point's own output of n_mp entries, tested
// here because its place lies between the tables' tests.
static inline const char* map_replace_tables_error(const slamit_map_index* map, const slamit_replace_index* X, const int32_t* touched) {
    if (!map || !X) return "null table";
    if (const char* bad = map_sizes_error(map)) return bad;
    const int n_kf = map->n_kf, n_mp = map->n_mp;
    if (n_mp && !touched) return "null array or negative n";
    if (X->obs_cap_out < 0) return "negative obs_cap_out";
    if (!map->obs_ptr || !map->kf_mp_ptr || !X->obs_ptr_out) return "null table";
    if (!map_csr_ok(map->obs_ptr, n_mp) || !map_csr_ok(map->kf_mp_ptr, n_kf)) return "a CSR pointer array does not ascend from 0";
    const size_t n_obs = (size_t)map->obs_ptr[n_mp], n_kfmp = (size_t)map->kf_mp_ptr[n_kf], cap_out = (size_t)X->obs_cap_out;
    if ((n_obs && (!map->obs_kf || !X->obs_idx || !X->obs_octave || !X->obs_weight)) ||
        (n_mp && (!X->mp_bad || !X->mp_nobs || !X->mp_found || !X->mp_visible || !X->mp_replaced)) || (n_kfmp && !X->kf_mp) ||
        (cap_out && (!X->obs_kf_out || !X->obs_idx_out || !X->obs_octave_out || !X->obs_weight_out)))
        return "null table";
    return map_obs_error(map, X->obs_idx, X->obs_weight);
}
// The same pair in a resident form, map by map: the sizes and the pointers, which are the device's and not read here.
static inline const char* map_replace_batch_error(int n_maps, int mp_cap, const slamit_map_index* maps, const slamit_replace_index* index) {
    for (int m = 0; m < n_maps; ++m) {
        const slamit_map_index& M = maps[m];
        const slamit_replace_index& X = index[m];
        if (const char* bad = map_batch_sizes_error(&M)) return bad;
        if (M.n_mp > mp_cap) return "a map with n_mp above mp_cap";
        if (X.obs_cap_out < 0) return "negative obs_cap_out";
        if (!M.obs_ptr || !M.obs_kf || !M.kf_mp_ptr || !X.obs_idx || !X.obs_octave || !X.obs_weight || !X.mp_bad || !X.mp_nobs || !X.mp_found || !X.mp_visible ||
            !X.mp_replaced || !X.kf_mp || !X.obs_ptr_out || !X.obs_kf_out || !X.obs_idx_out || !X.obs_octave_out || !X.obs_weight_out)
            return "null table";
    }
    return nullptr;
}

// The covisibility rows [n_kf][row_cap]: counts in [0, row_cap], cw_kf slots in [0, n_kf) and never the keyframe's own, ord_kf slots
// in [0, n_kf).
static inline const char* map_graph_rows_error(int n_kf, int row_cap, const int32_t* cw_kf, const int32_t* cw_n, const int32_t* ord_kf, const int32_t* ord_n) {
    for (int j = 0; j < n_kf; ++j) {
        if (cw_n[j] < 0 || cw_n[j] > row_cap || ord_n[j] < 0 || ord_n[j] > row_cap) return "a graph row's count outside [0, row_cap]";
        const int32_t* const cw = cw_kf + (size_t)j * row_cap;
        for (int e = 0; e < cw_n[j]; ++e)
            if (cw[e] < 0 || cw[e] >= n_kf || cw[e] == j) return "cw_kf holds a keyframe slot outside [0, n_kf) or a keyframe's own";
        if (!map_slots_ok(ord_kf + (size_t)j * row_cap, (size_t)ord_n[j], 0, n_kf)) return "ord_kf holds a keyframe slot outside [0, n_kf)";
    }
    return nullptr;
}

// The children table: slots in [0, n_kf), every row strictly ascending.  kf_child_ptr has passed map_csr_ok.
static inline const char* map_children_error(const slamit_map_index* map) {
    for (int j = 0; j < map->n_kf; ++j)
        for (int e = map->kf_child_ptr[j]; e < map->kf_child_ptr[j + 1]; ++e) {
            if (map->kf_child[e] < 0 || map->kf_child[e] >= map->n_kf) return "kf_child holds a keyframe slot outside [0, n_kf)";
            if (e > map->kf_child_ptr[j] && map->kf_child[e - 1] >= map->kf_child[e]) return "a children row does not ascend";
        }
    return nullptr;
}

#endif
