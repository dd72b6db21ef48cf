// orb_api.hip — C-ABI of the ORB extractor (include/slamit.h, slamit_orb_*): handle, device memory and the launch
// sequence; the plan (level geometry and every read-only table) is orb_plan.cc's.  Mirrors the interface of ORB_SLAM2::ORBextractor
// (include/ORBextractor.h:45-111, src/ORBextractor.cc:415-482,1064-1168).  No CPU compute path:
// every entry point fails with SLAMIT_ERR_DEVICE when no HIP device is usable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "orb_plan.h"
#include "slamit_internal.h"

// kernels (orb_kernels.hip)
hipError_t orbk_upload_pattern(hipStream_t st);
void orbk_resize(hipStream_t st, const uint8_t* src, int sw, int sh, size_t sstride, size_t sframe,
                 uint8_t* dst, int dw, int dh, size_t dstride, size_t dframe, const int* xofs,
                 const short* ialpha, const int* yofs, const short* ibeta, int nframes);
void orbk_resize_rows4(hipStream_t st, const uint8_t* src, size_t sstride, size_t sframe, int sh, uint8_t* dst, int dw, int dh,
                       size_t dstride, size_t dframe, const uint32_t* d_col, const uint32_t* d_row, int nframes);
void orbk_resize_rows8(hipStream_t st, const uint8_t* src, size_t sstride, size_t sframe, int sh, uint8_t* dst, int dw, int dh,
                       size_t dstride, size_t dframe, const uint32_t* d_col8, const uint32_t* d_row, int nframes);
hipError_t orbk_pyramid_bands_prepare(int smem_bytes);
void orbk_pyramid_bands(hipStream_t st, const BandTab& tab, const uint8_t* d_tables, const BandRows* d_rows, int first, int last, int nbands,
                        const uint8_t* src, size_t sstride, size_t sframe, int sh, uint8_t* pyr, size_t pyr_frame, int tile0, int smem, int nframes);
hipError_t orbk_pyramid_prepare(int smem_bytes);
void orbk_pyramid(hipStream_t st, const OrbLevel* levels, int nlevels, const PyrBox* boxes, const PyrTabs* tabs,
                  int nregions, const uint8_t* img0, size_t img0_stride, size_t img0_frame, uint8_t* pyr, int bufA_bytes,
                  int smem_bytes, int nframes, int l_first, int l_last);
hipError_t orbk_fast_prepare(int max_wcell, int max_hcell);
void orbk_fast(hipStream_t st, const FastTab& tab, int nlevels, const uint32_t* d_cells, int cells_per_frame, const uint8_t* img0,
               size_t img0_stride, size_t img0_frame, const uint8_t* pyr, unsigned long long* cand,
               size_t cand_frame_stride, int* cand_count, int iniTh, int minTh, int max_wcell, int max_hcell, int nframes);
hipError_t orbk_octree_prepare(int node_cap, int key_cap);
void orbk_octree(hipStream_t st, const OrbLevel* levels, int nlevels, const unsigned long long* cand,
                 size_t cand_frame_stride, int* cand_count, uint32_t* ws_xy, uint16_t* ws_node,
                 OrbLevelKp* lkp, size_t kp_frame_stride, int* kp_count, int node_cap, int key_cap, int nframes,
                 int level_override);
void orbk_ic_angle(hipStream_t st, const OrbLevel* levels, int nlevels, const uint8_t* img0, size_t img0_stride,
                   size_t img0_frame, const uint8_t* pyr, OrbLevelKp* lkp, size_t kp_frame_stride,
                   const int* kp_count, const KpBlockTab& tab, int nframes);
void orbk_blur_stream(hipStream_t st, const OrbLevel* levels, const uint32_t* d_inner, int n_inner, const uint32_t* d_edge, int n_edge,
                      const uint8_t* img0, size_t img0_stride, size_t img0_frame, const uint8_t* pyr, uint8_t* blur, int nframes);
void orbk_blur(hipStream_t st, const OrbLevel* levels, const uint32_t* d_tiles, int total_tiles, const uint8_t* img0,
               size_t img0_stride, size_t img0_frame, const uint8_t* pyr, uint8_t* blur, int nframes);
void orbk_describe(hipStream_t st, const OrbLevel* levels, int nlevels, const uint8_t* blur,
                   const OrbLevelKp* lkp, size_t kp_frame_stride, const int* kp_count, slamit_kp* out_kps,
                   uint8_t* out_desc, int out_cap, int* out_n, const KpBlockTab& tab, int nframes);
void orbk_pad(hipStream_t st, const uint8_t* src, int w, int h, size_t sstride, uint8_t* dst);
void orbk_decode_candidates(hipStream_t st, const OrbLevel* levels, int level, const unsigned long long* K, int n,
                            unsigned long long* order_out, int* xys);

namespace {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

// per-level chain: levels 0 .. ORB_BLUR_SPLIT are blurred on the side stream beside the tail of the pyramid chain, the rest after it
// (2 until the pyramid chain got its wide loads: its tail is shorter now); the banded pyramid forks where its first segment ends
#define ORB_BLUR_SPLIT 1

struct slamit_orb {
    slamit_orb_params p;
    int device;
    hipStream_t stream;
    hipStream_t stream_b;     // side stream: the blur of a call runs beside its FAST / octree / orientation launches
    hipEvent_t ev_pyr, ev_mid, ev_blur;
    SlamitSwitches sw;        // the environment switches, read when the handle is created
    int nlevels;
    OrbPlan pl;               // level geometry, sizes and the read-only tables (orb_plan.cc)
    bool blur_stream_on;      // blur through the strip tables split at the level edges (blur_stream_kernel), not the tile kernel
    // device memory: the plan's tables in one block (pl.*_off), then the per-frame buffers
    uint8_t* d_tables;
    const OrbLevel* d_levels;
    uint8_t* d_pyr;
    uint8_t* d_blur;
    unsigned long long* d_cand;
    uint32_t* d_ws_xy;
    uint16_t* d_ws_node;
    int* d_counts;  // cand_count [max_batch][nlevels][ORB_CC_PAD], then kp_count [max_batch][nlevels]
    bool counters_clean;   // every cand_count is zero (left so by the last call's octree pass)
    OrbLevelKp* d_lkp;
    // staging for the host-pointer entry points
    uint8_t* d_in;
    size_t d_in_stride, d_in_frame;
    slamit_kp* d_out_kps;
    uint8_t* d_out_desc;
    int* d_out_n;
    uint8_t* h_out;   // pinned: [n per frame | keypoints | descriptors] of a whole batch, so the readback is one stream op chain + one sync
    uint8_t* d_scratch;  // padded plane / debug scratch
    size_t scratch_bytes;
    // optional per-stage hipEvent timing (slamit_orb_profile)
    int prof_on;
    long prof_call;                       // extract calls since profiling was switched on
    std::vector<hipEvent_t> prof_ev;   // pairs (begin, end)
    std::vector<int> prof_stage;       // stage id of each pair
    // last call (for slamit_orb_level / debug getters)
    const uint8_t* last_img0;
    size_t last_stride, last_frame;
    int last_nframes;
};

// a table of the block at byte offset `off`
template <typename T>
static const T* dtab(const slamit_orb* h, size_t off) { return reinterpret_cast<const T*>(h->d_tables + off); }

static void orb_free(slamit_orb* h) {
    if (!h) return;
    SlamitDeviceGuard guard(h->device);
    hipFree(h->d_tables); hipFree(h->d_pyr); hipFree(h->d_blur); hipFree(h->d_cand); hipFree(h->d_ws_xy);
    hipFree(h->d_ws_node); hipFree(h->d_counts); hipFree(h->d_lkp); hipFree(h->d_in); hipFree(h->d_out_kps);
    hipFree(h->d_out_desc); hipFree(h->d_out_n); if (h->h_out) hipHostFree(h->h_out); hipFree(h->d_scratch);
    for (hipEvent_t e : h->prof_ev) hipEventDestroy(e);
    if (h->ev_pyr) hipEventDestroy(h->ev_pyr);
    if (h->ev_mid) hipEventDestroy(h->ev_mid);
    if (h->ev_blur) hipEventDestroy(h->ev_blur);
    if (h->stream_b) hipStreamDestroy(h->stream_b);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

extern "C" {

int slamit_orb_create(const slamit_orb_params* p, int device, slamit_orb** out) {
    if (!p || !out) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_create: null argument");
    *out = nullptr;
    if (p->nlevels < 1 || p->nlevels > ORB_MAX_LEVELS || p->nfeatures < 1 || !(p->scale_factor > 1.f) ||
        p->ini_th_fast < 1 || p->ini_th_fast > 255 || p->min_th_fast < 1 || p->min_th_fast > 255 ||
        p->width < 0 || p->height < 0 || p->max_batch < 1)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_create: parameter out of range");
    SLAMIT_USE_DEVICE(device);
    slamit_orb* h = new slamit_orb();
    h->p = *p;
    h->device = device;
    h->sw = slamit_read_switches();
    const int nl = h->nlevels = p->nlevels;
    const char* why = "";
    if (!orb_plan(*p, OrbPlanOptions{h->sw.resize_no8}, h->pl, &why)) {
        delete h;
        return slamit_fail(SLAMIT_ERR_ARG, why);
    }
    const OrbPlan& P = h->pl;
    const bool empty = P.levels.empty();
    h->blur_stream_on = !empty && !h->sw.blur_no_stream;

    const size_t B = (size_t)p->max_batch;
    const size_t counts_bytes = sizeof(int) * ((ORB_CC_PAD + 1) * B * nl + 2 * ORB_CC_PAD);
    h->d_in_stride = round_up((size_t)std::max(p->width, 1), 64);
    h->d_in_frame = h->d_in_stride * std::max(p->height, 1);
    h->scratch_bytes = std::max<size_t>((size_t)(p->width + 38) * (p->height + 38),
                                        (sizeof(unsigned long long) + 3 * sizeof(int)) * (P.cand_frame_stride + 64));
    hipError_t e = hipSuccess;
#define ALLOC(ptr, bytes) if (e == hipSuccess) e = hipMalloc((void**)&(ptr), std::max<size_t>((bytes), 256))
    ALLOC(h->d_tables, P.table_bytes);
    ALLOC(h->d_pyr, P.pyr_frame_total * B);
    ALLOC(h->d_blur, P.blur_frame_total * B + 256);   // + slack: the descriptor kernel stages whole dwords up to 6 bytes past a row end
    ALLOC(h->d_cand, sizeof(unsigned long long) * P.cand_frame_stride * B);
    ALLOC(h->d_ws_xy, sizeof(uint32_t) * P.cand_frame_stride * B);
    ALLOC(h->d_ws_node, sizeof(uint16_t) * P.cand_frame_stride * B);
    ALLOC(h->d_counts, counts_bytes);
    ALLOC(h->d_lkp, sizeof(OrbLevelKp) * P.kp_frame_stride * B);
    ALLOC(h->d_in, h->d_in_frame * B);
    ALLOC(h->d_out_kps, sizeof(slamit_kp) * (size_t)P.max_out * B);
    ALLOC(h->d_out_desc, (size_t)SLAMIT_DESC_BYTES * P.max_out * B);
    ALLOC(h->d_out_n, sizeof(int) * B);
    ALLOC(h->d_scratch, h->scratch_bytes);
#undef ALLOC
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_out, 256 + (size_t)B * 256 + (sizeof(slamit_kp) + SLAMIT_DESC_BYTES) * (size_t)P.max_out * B, hipHostMallocDefault);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream_b, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_pyr, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_mid, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_blur, hipEventDisableTiming);
    if (e == hipSuccess && P.table_bytes) {
        std::vector<uint8_t> img;
        orb_plan_image(P, h->d_tables, img);
        e = hipMemcpy(h->d_tables, img.data(), img.size(), hipMemcpyHostToDevice);
    }
    h->d_levels = dtab<OrbLevel>(h, P.levels_off);
    if (e == hipSuccess && P.pyr_regions) e = orbk_pyramid_prepare(P.pyr_smem);
    for (const OrbBandSeg& G : P.bands) if (e == hipSuccess) e = orbk_pyramid_bands_prepare(G.smem);
    if (e == hipSuccess) e = orbk_upload_pattern(h->stream);
    if (e == hipSuccess) e = orbk_octree_prepare(P.node_cap, P.oct_key_cap);
    if (e == hipSuccess && !empty) e = orbk_fast_prepare(P.max_wcell, P.max_hcell);
    if (e == hipSuccess) e = hipMemset(h->d_counts, 0, counts_bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        orb_free(h);
        return slamit_fail_hip(e, "slamit_orb_create");
    }
    *out = h;
    return SLAMIT_OK;
}
void slamit_orb_destroy(slamit_orb* h) { orb_free(h); }

int slamit_orb_tables(const slamit_orb* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                      int32_t* features_per_level) {
    if (!h) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_tables: null handle");
    for (int i = 0; i < h->nlevels; ++i) {
        if (scale) scale[i] = h->pl.scale[i];
        if (inv_scale) inv_scale[i] = h->pl.inv_scale[i];
        if (sigma2) sigma2[i] = h->pl.sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = h->pl.inv_sigma2[i];
        if (features_per_level) features_per_level[i] = h->pl.per_level[i];
    }
    return SLAMIT_OK;
}

int slamit_orb_max_keypoints(const slamit_orb* h) { return h ? h->pl.max_out : 0; }

// stage ids reported by slamit_orb_profile
enum { ST_RESIZE = 0, ST_FAST, ST_OCTREE, ST_ANGLE, ST_BLUR, ST_DESCRIBE, ST_COUNT };

static void prof_mark(slamit_orb* h, hipStream_t st, int stage, bool begin) {
    if (!h->prof_on || h->prof_ev.size() >= 2 * 16384) return;
    if (h->prof_on >= 2 && (stage != ST_FAST || h->prof_call % (h->prof_on - 1) != 0)) return;   // dominant kernel, sampled
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    hipEventRecord(e, st);
    h->prof_ev.push_back(e);
    if (begin) h->prof_stage.push_back(stage);
}

int slamit_orb_extract_batch_dev(slamit_orb* h, const uint8_t* d_gray, size_t stride, size_t frame_stride,
                                 int nframes, slamit_kp* d_kps, uint8_t* d_desc, int cap, int32_t* d_n_out,
                                 void* stream) {
    if (!h || !d_n_out || nframes < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_extract_batch_dev: bad argument");
    if (nframes > h->p.max_batch) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_orb_extract_batch_dev: nframes > max_batch");
    if (nframes == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(h->device);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const int nl = h->nlevels;
    const OrbPlan& P = h->pl;
    if (h->p.width == 0 || h->p.height == 0) {  // ORBextractor.cc:1068: empty image -> nothing
        HIP_TRY(hipMemsetAsync(d_n_out, 0, sizeof(int) * nframes, st));
        h->last_nframes = 0;
        return SLAMIT_OK;
    }
    if (!d_gray || !d_kps || !d_desc) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_extract_batch_dev: null buffer");
    if (cap < P.max_out) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_orb_extract_batch_dev: cap < slamit_orb_max_keypoints()");
    if (stride < (size_t)h->p.width || (nframes > 1 && frame_stride < stride * (size_t)h->p.height))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_extract_batch_dev: stride smaller than the frame");
    if (stride >= ((size_t)1 << 24)) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_extract_batch_dev: row pitch of 16 MiB or more");   // kernels address rows with 24-bit multiplies
    int* cand_count = h->d_counts;
    int* kp_count = h->d_counts + (size_t)h->p.max_batch * nl * ORB_CC_PAD;
    // the candidate counters are zero between calls: the octree pass consumes and re-zeroes them.  Only a call that
    // follows a failed one (or the first) clears them itself.
    if (!h->counters_clean) HIP_TRY(hipMemsetAsync(h->d_counts, 0, sizeof(int) * (size_t)h->p.max_batch * nl * ORB_CC_PAD, st));
    h->counters_clean = false;
    // the blur of levels [l0, l1): every strip streams down its columns (blur_stream_kernel: one launch for the strips inside the
    // level and those at its left / right edge); when the caller's level-0 plane is not 4-byte aligned everything takes the tile kernel
    const bool blur_src_aligned = ((((uintptr_t)d_gray) | stride | frame_stride) & 3) == 0;
    auto launch_blur = [&](hipStream_t bs, int l0, int l1) {
        auto strips = [&](const OrbStrips& S) { return dtab<uint32_t>(h, S.off) + 4 * (size_t)S.base[l0]; };
        auto nstrips = [&](const OrbStrips& S) { return S.base[l1] - S.base[l0]; };
        if (h->blur_stream_on && blur_src_aligned) {
            orbk_blur_stream(bs, h->d_levels, strips(P.blur_str), nstrips(P.blur_str), strips(P.blur_edge), nstrips(P.blur_edge), d_gray, stride, frame_stride,
                             h->d_pyr, h->d_blur, nframes);
        } else {
            orbk_blur(bs, h->d_levels, strips(P.blur_all), nstrips(P.blur_all), d_gray, stride, frame_stride, h->d_pyr, h->d_blur, nframes);
        }
    };
    // K1: pyramid, level l from level l-1
    prof_mark(h, st, ST_RESIZE, true);
    const bool src0_aligned = ((((uintptr_t)d_gray) | stride | frame_stride) & 3) == 0;
    const bool side = h->prof_on != 1;   // while every stage is timed (slamit_orb_profile(h, 1)) everything stays on one stream
    const bool early_blur = side && ORB_BLUR_SPLIT < nl - 1;
    int early_done = -1;   // the last level the early blur launch took
    auto fork_early_blur = [&](int l) -> hipError_t {
        // the blur of the big levels 0 .. l (most of its bytes) runs on the side stream beside the rest of the pyramid: the small
        // levels are a few microseconds of work behind a barrier or a kernel boundary each and leave the chip idle
        hipError_t e = hipEventRecord(h->ev_mid, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->stream_b, h->ev_mid, 0);
        if (e != hipSuccess) return e;
        launch_blur(h->stream_b, 0, l + 1);
        early_done = l;
        return hipSuccess;
    };
    if (!P.bands.empty() && src0_aligned) {
        // one launch per segment: a (frame, band) workgroup walks the segment's levels out of LDS (pyramid_bands_kernel)
        for (const OrbBandSeg& G : P.bands) {
            const OrbLevel& S = P.levels[G.first];
            orbk_pyramid_bands(st, P.band_tab, h->d_tables, dtab<BandRows>(h, G.rows_off), G.first, G.last, G.nbands,
                               G.first == 0 ? d_gray : h->d_pyr + S.plane_off, G.first == 0 ? stride : (size_t)S.stride,
                               G.first == 0 ? frame_stride : P.pyr_frame_total, S.h, h->d_pyr, P.pyr_frame_total, G.tile0, G.smem, nframes);
            if (early_blur && G.last < nl - 1 && early_done < 0) HIP_TRY(fork_early_blur(G.last));   // beside the second segment
        }
    } else if (P.rows4_ok && src0_aligned) {
        for (int l = 1; l < nl; ++l) {
            const OrbLevel& S = P.levels[l - 1];
            const OrbLevel& D = P.levels[l];
            const uint8_t* src = l == 1 ? d_gray : h->d_pyr + S.plane_off;
            const OrbResizeTabs& T = P.rs[l];
            if (!T.col8.empty())
                orbk_resize_rows8(st, src, l == 1 ? stride : (size_t)S.stride, l == 1 ? frame_stride : P.pyr_frame_total, S.h,
                                  h->d_pyr + D.plane_off, D.w, D.h, (size_t)D.stride, P.pyr_frame_total, dtab<uint32_t>(h, T.col8_off),
                                  dtab<uint32_t>(h, T.row4_off), nframes);
            else
                orbk_resize_rows4(st, src, l == 1 ? stride : (size_t)S.stride, l == 1 ? frame_stride : P.pyr_frame_total, S.h,
                                  h->d_pyr + D.plane_off, D.w, D.h, (size_t)D.stride, P.pyr_frame_total, dtab<uint32_t>(h, T.col4_off),
                                  dtab<uint32_t>(h, T.row4_off), nframes);
            if (early_blur && l == ORB_BLUR_SPLIT) HIP_TRY(fork_early_blur(l));
        }
    } else if (P.pyr_regions) {
        orbk_pyramid(st, h->d_levels, nl, dtab<PyrBox>(h, P.boxes_off), dtab<PyrTabs>(h, P.tabs_off), P.pyr_regions, d_gray, stride, frame_stride,
                     h->d_pyr, P.pyr_bufA, P.pyr_smem, nframes, 0, nl - 1);
    } else {
        for (int l = 1; l < nl; ++l) {
            const OrbLevel& S = P.levels[l - 1];
            const OrbLevel& D = P.levels[l];
            const uint8_t* src = l == 1 ? d_gray : h->d_pyr + S.plane_off;
            size_t sstride = l == 1 ? stride : (size_t)S.stride;
            size_t sframe = l == 1 ? frame_stride : P.pyr_frame_total;
            const OrbResizeTabs& T = P.rs[l];
            orbk_resize(st, src, S.w, S.h, sstride, sframe, h->d_pyr + D.plane_off, D.w, D.h, (size_t)D.stride,
                        P.pyr_frame_total, dtab<int>(h, T.xofs_off), dtab<short>(h, T.ialpha_off), dtab<int>(h, T.yofs_off),
                        dtab<short>(h, T.ibeta_off), nframes);
        }
    }
    prof_mark(h, st, ST_RESIZE, false);
    // K2: FAST + NMS + per-cell threshold fallback -> candidate lists
    prof_mark(h, st, ST_FAST, true);
    orbk_fast(st, P.fast, nl, dtab<uint32_t>(h, P.cells_off), (int)(P.cells.size() / 4), d_gray, stride, frame_stride, h->d_pyr, h->d_cand,
              P.cand_frame_stride, cand_count, h->p.ini_th_fast, h->p.min_th_fast, P.max_wcell, P.max_hcell, nframes);
    prof_mark(h, st, ST_FAST, false);
    // K6: blur every level.  Only the descriptor pass reads it, and it only needs the pyramid: it runs on the side stream
    // beside the octree / orientation launches (latency bound: a few hundred workgroups on 256 CUs) and joins before the
    // descriptors.  FAST (issue bound, the kernel the roofline is quoted on) keeps the chip to itself.
    if (side) {
        HIP_TRY(hipEventRecord(h->ev_pyr, st));
        HIP_TRY(hipStreamWaitEvent(h->stream_b, h->ev_pyr, 0));
        launch_blur(h->stream_b, early_done + 1, nl);   // the levels the early launch left
        HIP_TRY(hipEventRecord(h->ev_blur, h->stream_b));
    }
    // K4: octree
    prof_mark(h, st, ST_OCTREE, true);
    orbk_octree(st, h->d_levels, nl, h->d_cand, P.cand_frame_stride, cand_count, h->d_ws_xy, h->d_ws_node, h->d_lkp,
                P.kp_frame_stride, kp_count, P.node_cap, P.oct_key_cap, nframes, -1);
    prof_mark(h, st, ST_OCTREE, false);
    // K5: orientation
    prof_mark(h, st, ST_ANGLE, true);
    orbk_ic_angle(st, h->d_levels, nl, d_gray, stride, frame_stride, h->d_pyr, h->d_lkp, P.kp_frame_stride, kp_count,
                  P.ic_blocks, nframes);
    prof_mark(h, st, ST_ANGLE, false);
    if (side) {
        HIP_TRY(hipStreamWaitEvent(st, h->ev_blur, 0));
    } else {
        prof_mark(h, st, ST_BLUR, true);
        launch_blur(st, 0, nl);
        prof_mark(h, st, ST_BLUR, false);
    }
    // K7: descriptors + output records
    prof_mark(h, st, ST_DESCRIBE, true);
    orbk_describe(st, h->d_levels, nl, h->d_blur, h->d_lkp, P.kp_frame_stride, kp_count, d_kps, d_desc, cap, d_n_out,
                  P.desc_blocks, nframes);
    prof_mark(h, st, ST_DESCRIBE, false);
    ++h->prof_call;
    HIP_TRY(hipGetLastError());
    h->counters_clean = true;
    h->last_img0 = d_gray; h->last_stride = stride; h->last_frame = frame_stride; h->last_nframes = nframes;
    return SLAMIT_OK;
}

int slamit_orb_extract_batch(slamit_orb* h, const uint8_t* gray, size_t stride, size_t frame_stride, int nframes,
                             slamit_kp* kps, uint8_t* desc, int cap, int* n_out) {
    if (!h || !n_out || nframes < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_extract_batch: bad argument");
    if (nframes > h->p.max_batch) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_orb_extract_batch: nframes > max_batch");
    if (nframes == 0) return SLAMIT_OK;
    if (h->p.width == 0 || h->p.height == 0) {
        for (int f = 0; f < nframes; ++f) n_out[f] = 0;
        return SLAMIT_OK;
    }
    if (!gray || !kps || !desc) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_extract_batch: null buffer");
    if (cap < h->pl.max_out) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_orb_extract_batch: cap < slamit_orb_max_keypoints()");
    SLAMIT_USE_DEVICE(h->device);
    const int W = h->p.width, H = h->p.height;
    for (int f = 0; f < nframes; ++f)
        HIP_TRY(hipMemcpy2DAsync(h->d_in + f * h->d_in_frame, h->d_in_stride, gray + (size_t)f * frame_stride, stride, W, H,
                                 hipMemcpyHostToDevice, h->stream));
    int rc = slamit_orb_extract_batch_dev(h, h->d_in, h->d_in_stride, h->d_in_frame, nframes, h->d_out_kps, h->d_out_desc,
                                          h->pl.max_out, h->d_out_n, h->stream);
    if (rc != SLAMIT_OK) return rc;
    // readback through the pinned block: counts, keypoints and descriptors are three copies on the stream and ONE
    // synchronisation (copying by the exact counts needs the counts on the host first, i.e. a second round trip)
    const size_t o_k = ((sizeof(int) * (size_t)nframes + 255) & ~(size_t)255), kb = sizeof(slamit_kp) * (size_t)h->pl.max_out * nframes;
    const size_t o_d = (o_k + kb + 255) & ~(size_t)255, db = (size_t)SLAMIT_DESC_BYTES * h->pl.max_out * nframes;
    HIP_TRY(hipMemcpyAsync(h->h_out, h->d_out_n, sizeof(int) * nframes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(h->h_out + o_k, h->d_out_kps, kb, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(h->h_out + o_d, h->d_out_desc, db, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    memcpy(n_out, h->h_out, sizeof(int) * nframes);
    for (int f = 0; f < nframes; ++f) {
        const int n = n_out[f];
        if (n > 0) {
            memcpy(kps + (size_t)f * cap, h->h_out + o_k + sizeof(slamit_kp) * (size_t)f * h->pl.max_out, sizeof(slamit_kp) * n);
            memcpy(desc + (size_t)f * cap * SLAMIT_DESC_BYTES, h->h_out + o_d + (size_t)SLAMIT_DESC_BYTES * f * h->pl.max_out, (size_t)SLAMIT_DESC_BYTES * n);
        }
    }
    return SLAMIT_OK;
}

int slamit_orb_extract(slamit_orb* h, const uint8_t* gray, size_t stride, slamit_kp* kps, uint8_t* desc, int cap,
                       int* n_out) {
    return slamit_orb_extract_batch(h, gray, stride, stride * (size_t)(h ? h->p.height : 0), 1, kps, desc, cap, n_out);
}

int slamit_orb_profile(slamit_orb* h, int enable, float* stage_ms, int32_t* stage_calls, int nstages) {
    if (!h) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_profile: null handle");
    SLAMIT_USE_DEVICE(h->device);
    if (stage_ms || stage_calls) {
        for (int i = 0; i < nstages; ++i) { if (stage_ms) stage_ms[i] = 0.f; if (stage_calls) stage_calls[i] = 0; }
        for (size_t i = 0; i < h->prof_stage.size() && 2 * i + 1 < h->prof_ev.size(); ++i) {
            HIP_TRY(hipEventSynchronize(h->prof_ev[2 * i + 1]));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, h->prof_ev[2 * i], h->prof_ev[2 * i + 1]));
            int s = h->prof_stage[i];
            if (s < nstages) { if (stage_ms) stage_ms[s] += ms; if (stage_calls) stage_calls[s] += 1; }
        }
    }
    for (hipEvent_t e : h->prof_ev) hipEventDestroy(e);
    h->prof_ev.clear(); h->prof_stage.clear();
    h->prof_on = enable;
    h->prof_call = 0;
    return SLAMIT_OK;
}

int slamit_orb_level(slamit_orb* h, int frame, int level, uint8_t* dst, size_t dst_bytes, int* w, int* h_out) {
    if (!h || level < 0 || level >= h->nlevels) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_level: bad level");
    if (h->p.width == 0 || h->p.height == 0) return slamit_fail(SLAMIT_ERR_STATE, "slamit_orb_level: empty image");
    const OrbLevel& L = h->pl.levels[level];
    if (w) *w = L.w;
    if (h_out) *h_out = L.h;
    if (!dst) return SLAMIT_OK;
    if (frame < 0 || frame >= h->last_nframes || !h->last_img0) return slamit_fail(SLAMIT_ERR_STATE, "slamit_orb_level: no such frame in the last extract call");
    size_t need = (size_t)(L.w + 38) * (L.h + 38);
    if (dst_bytes < need) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_orb_level: dst too small");
    SLAMIT_USE_DEVICE(h->device);
    const uint8_t* src = level == 0 ? h->last_img0 + (size_t)frame * h->last_frame
                                    : h->d_pyr + L.plane_off + (size_t)frame * h->pl.pyr_frame_total;
    orbk_pad(h->stream, src, L.w, L.h, level == 0 ? h->last_stride : (size_t)L.stride, h->d_scratch);
    HIP_TRY(hipMemcpyAsync(dst, h->d_scratch, need, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAMIT_OK;
}

int slamit_orb_pyramid_view(const slamit_orb* h, slamit_pyramid_view* out) {
    if (!h || !out) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_pyramid_view: null argument");
    memset(out, 0, sizeof(*out));
    if (h->p.width == 0 || h->p.height == 0) return slamit_fail(SLAMIT_ERR_STATE, "slamit_orb_pyramid_view: empty image");
    if (!h->last_img0 || h->last_nframes < 1) return slamit_fail(SLAMIT_ERR_STATE, "slamit_orb_pyramid_view: no extract call yet");
    out->nlevels = h->nlevels; out->nframes = h->last_nframes;
    for (int l = 0; l < h->nlevels; ++l) {
        const OrbLevel& L = h->pl.levels[l];
        slamit_pyramid_level& V = out->level[l];
        V.plane = l == 0 ? h->last_img0 : h->d_pyr + L.plane_off;
        V.w = L.w; V.h = L.h;
        V.stride = l == 0 ? h->last_stride : (size_t)L.stride;
        V.frame_stride = l == 0 ? h->last_frame : h->pl.pyr_frame_total;
    }
    return SLAMIT_OK;
}

int slamit_orb_debug_blurred(slamit_orb* h, int frame, int level, uint8_t* dst, size_t dst_bytes, int* w, int* h_out) {
    if (!h || level < 0 || level >= h->nlevels) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_debug_blurred: bad level");
    if (h->p.width == 0 || h->p.height == 0) return slamit_fail(SLAMIT_ERR_STATE, "slamit_orb_debug_blurred: empty image");
    const OrbLevel& L = h->pl.levels[level];
    if (w) *w = L.w;
    if (h_out) *h_out = L.h;
    if (!dst) return SLAMIT_OK;
    if (frame < 0 || frame >= h->last_nframes) return slamit_fail(SLAMIT_ERR_STATE, "slamit_orb_debug_blurred: no such frame in the last extract call");
    if (dst_bytes < (size_t)L.w * L.h) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_orb_debug_blurred: dst too small");
    SLAMIT_USE_DEVICE(h->device);
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)L.w, h->d_blur + L.blur_off + (size_t)frame * h->pl.blur_frame_total, (size_t)L.stride, (size_t)L.w,
                             (size_t)L.h, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAMIT_OK;
}

int slamit_orb_debug_candidates(slamit_orb* h, int frame, int level, int32_t* xys, int cap, int* n_out) {
    if (!h || level < 0 || level >= h->nlevels || !n_out) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_debug_candidates: bad argument");
    if (frame < 0 || frame >= h->last_nframes) return slamit_fail(SLAMIT_ERR_STATE, "slamit_orb_debug_candidates: no such frame");
    SLAMIT_USE_DEVICE(h->device);
    const OrbLevel& L = h->pl.levels[level];
    int n = 0;
    HIP_TRY(hipMemcpy(&n, h->d_counts + (size_t)(frame * h->nlevels + level) * ORB_CC_PAD + 1, sizeof(int), hipMemcpyDeviceToHost));   // word 1: the count the octree pass consumed
    n = std::min(n, L.cand_cap);
    *n_out = n;
    if (!xys || n == 0) return SLAMIT_OK;
    if (cap < n) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_orb_debug_candidates: cap too small");
    unsigned long long* d_order = (unsigned long long*)h->d_scratch;
    int* d_xys = (int*)(d_order + round_up((size_t)n, 64));
    orbk_decode_candidates(h->stream, h->d_levels, level, h->d_cand + L.cand_off + (size_t)frame * h->pl.cand_frame_stride, n, d_order, d_xys);
    std::vector<unsigned long long> order(n);
    std::vector<int> raw(3 * (size_t)n);
    HIP_TRY(hipMemcpyAsync(order.data(), d_order, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(raw.data(), d_xys, sizeof(int) * 3 * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    // present in the reference's vToDistributeKeys order (the device list is unordered)
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int a, int b) { return order[a] < order[b]; });
    for (int i = 0; i < n; ++i) { xys[3 * i] = raw[3 * idx[i]]; xys[3 * i + 1] = raw[3 * idx[i] + 1]; xys[3 * i + 2] = raw[3 * idx[i] + 2]; }
    return SLAMIT_OK;
}

int slamit_orb_debug_octree_path(slamit_orb* h, int frame, int level, int* path_out) {
    if (!h || level < 0 || level >= h->nlevels || !path_out) return slamit_fail(SLAMIT_ERR_ARG, "slamit_orb_debug_octree_path: bad argument");
    if (frame < 0 || frame >= h->last_nframes) return slamit_fail(SLAMIT_ERR_STATE, "slamit_orb_debug_octree_path: no such frame");
    SLAMIT_USE_DEVICE(h->device);
    HIP_TRY(hipMemcpy(path_out, h->d_counts + (size_t)(frame * h->nlevels + level) * ORB_CC_PAD + 2, sizeof(int), hipMemcpyDeviceToHost));   // word 2: octree_kernel's path word
    return SLAMIT_OK;
}

}  // extern "C"

// stereo.hip: the device a handle was created on
int slamit_orb_device_of(const slamit_orb* h) { return h ? h->device : -1; }
