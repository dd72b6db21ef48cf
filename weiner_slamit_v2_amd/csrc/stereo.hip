// stereo.hip — Frame::ComputeStereoMatches on the GPU (include/slamit.h, slamit_stereo_match*).
//
// Reference: ORB_SLAM2/src/Frame.cc:591-763.  Every float expression and every gate is csrc/stereo.h's; this file is the three
// launches round it, for a batch of frame pairs that two extract calls left in HBM:
//   records   one lane per right keypoint: {uR, first row, last row, octave} of its band, 16 bytes, into the workspace.  The
//             reference's table of keypoints by row is the set of records whose band holds the row; no list per row is built, so
//             no launch depends on how many rows a band covers.
//   match     one wavefront per left keypoint.  Lanes stride over the frame's records: band, gate, 256-bit Hamming distance, and
//             the wave minimum of (distance << 16 | right index), which is "strict <, first wins" whatever the order.  Then the
//             lanes share the 121 pixels of the patch: each takes up to two, subtracts the centres and adds its 11 absolute
//             differences; 11 wave sums give the shifts' SADs as exact integers.  Lane 0 writes what stereo_subpixel returns.
//   median    one workgroup per frame: the size / 2-th smallest SAD from two 256-bin LDS histograms (high byte, then low byte
//             within the chosen bin: exact for 16-bit values), thDist, status 7 and the count of the survivors.
// What bounds every read: counts are clamped to [0, cap] with cap <= SLAMIT_STEREO_MAX_KP on the host; a right index comes out
// of the key, so it is below the clamped count; octaves are tested against nlevels <= SLAMIT_MAX_LEVELS before they index a view
// or a table; pixel addresses are formed only after stereo.h's window tests have placed both windows inside their planes.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "stereo.h"
#include "wave_ops.h"

static_assert(STEREO_MAX_LEVELS == SLAMIT_MAX_LEVELS, "stereo.h's tables are SLAMIT_MAX_LEVELS long");
static_assert(SLAMIT_STEREO_MAX_KP < 65536, "the selection key keeps the right index in 16 bits");
static_assert(121 * 510 < 65536, "the median's two histograms cover 16 bits");

struct StLevel { const uint8_t* plane; int32_t w, h; uint64_t stride, frame_stride; };
struct StView { int32_t nlevels, nframes; StLevel level[SLAMIT_MAX_LEVELS]; };
static_assert(sizeof(StLevel) == sizeof(slamit_pyramid_level) && sizeof(StView) == sizeof(slamit_pyramid_view), "StView is slamit_pyramid_view");

struct StDev {
    int32_t nframes, cap_l, cap_r, rows, nlevels;
    StView L, R;
    const slamit_kp* kps_l; const uint8_t* desc_l; const int32_t* n_l;
    const slamit_kp* kps_r; const uint8_t* desc_r; const int32_t* n_r;
    const float* mb; const float* mbf; const float* scale; const float* inv_scale;
    int4* recs;   // [nframes][cap_r]
    float* u_right; float* depth; uint8_t* status; int32_t* best_r; int32_t* ham; int32_t* sad; int32_t* n_matched;
};

__device__ __forceinline__ int clamp_count(int n, int cap) { return min(max(n, 0), cap); }

__device__ __forceinline__ int wave_sum_i32(int v) {   // every lane active; the same value in every lane
    v += dpp<0xB1>(v);
    v += dpp<0x4E>(v);
    v += dpp<0x141>(v);
    v += dpp<0x140>(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// grid (ceil(cap_r / 256), frames), 256 threads: lane t of block b takes right keypoint 256 b + t
__global__ __launch_bounds__(256) void stereo_records_kernel(StDev D) {
    const int f = blockIdx.y;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= clamp_count(D.n_r[f], D.cap_r)) return;
    const slamit_kp* kp = D.kps_r + (size_t)f * D.cap_r + i;
    const float x = kp->x, y = kp->y;
    const int octave = kp->octave;
    int minr, maxr;
    stereo_band(y, x, octave, D.nlevels, D.scale, D.rows, minr, maxr);
    D.recs[(size_t)f * D.cap_r + i] = make_int4(__float_as_int(x), minr, maxr, octave);
}

// grid (ceil(cap_l / 4), frames), 256 threads: wavefront w of block b takes left keypoint 4 b + w
__global__ __launch_bounds__(256) void stereo_match_kernel(StDev D) {
    const int f = blockIdx.y;
    const int lane = (int)(threadIdx.x & 63);
    const int iL = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (iL >= clamp_count(D.n_l[f], D.cap_l)) return;
    const int nR = clamp_count(D.n_r[f], D.cap_r);
    const size_t oL = (size_t)f * D.cap_l + iL;
    const slamit_kp* kp = D.kps_l + oL;
    const float uL = kp->x, vL = kp->y;
    const int levelL = kp->octave;
    const float mbf = D.mbf[f];
    int row;
    float minU, maxU, maxD;
    int st = stereo_entry(uL, vL, levelL, D.nlevels, D.rows, D.mb[f], mbf, row, minU, maxU, maxD);
    float uR = -1.0f, depth = -1.0f;
    int bestR = -1, ham = -1, sad = -1;
    if (st < 0) {
        const int4* recs = D.recs + (size_t)f * D.cap_r;
        const uint4* dl = reinterpret_cast<const uint4*>(D.desc_l + 32 * oL);
        const uint4* dr = reinterpret_cast<const uint4*>(D.desc_r + 32 * (size_t)f * D.cap_r);
        const uint4 a0 = dl[0], a1 = dl[1];
        unsigned key = 0xFFFFFFFFu;
        bool any = false;
        for (int i = lane; i < nR; i += 64) {
            const int4 r = recs[i];
            if (row < r.y || row > r.z) continue;
            any = true;
            if (!stereo_gate(r.w, levelL, __int_as_float(r.x), minU, maxU)) continue;
            const unsigned d = (unsigned)hamming256(a0, a1, dr[2 * i], dr[2 * i + 1]);
            key = min(key, (d << 16) | (unsigned)i);
        }
        const bool any_wave = __ballot(any) != 0;
        key = wave_min_u32(key);
        if (!any_wave) st = STEREO_NO_CANDIDATE;
        else if ((key >> 16) >= (unsigned)STEREO_TH_HIGH) st = STEREO_NO_DESCRIPTOR;   // 0xFFFF: nothing passed the gate
        else {
            bestR = (int)(key & 0xFFFFu);                                              // < nR: it was a loop index
            ham = (int)(key >> 16);
            const slamit_kp* kr = D.kps_r + (size_t)f * D.cap_r + bestR;
            const float uR0 = kr->x;
            const int octR = kr->octave;
            if (octR < 0 || octR >= D.nlevels) st = STEREO_DEPARTURE;
            else {
                const float inv = D.inv_scale[levelL];
                const float su = stereo_scaled(uL, inv), sv = stereo_scaled(vL, inv), suR0 = stereo_scaled(uR0, inv);
                const StLevel& PL = D.L.level[levelL];
                const StLevel& PR = D.R.level[levelL];
                if (!stereo_left_window_inside(su, sv, PL.w, PL.h)) st = STEREO_DEPARTURE;
                else if (!stereo_right_window_ref(suR0, PR.w)) st = STEREO_RIGHT_WINDOW;
                else if (!stereo_right_strip_inside(suR0, sv, PR.w, PR.h)) st = STEREO_DEPARTURE;
                else {
                    // both windows are inside their planes: x0 >= 0, x0 + 10 < PL.w, xr >= 0, xr + 20 < PR.w, y0 >= 0, y0 + 10 < both h
                    const int x0 = (int)su - STEREO_W, y0 = (int)sv - STEREO_W, xr = (int)suR0 - STEREO_L - STEREO_W;
                    const uint8_t* pl = PL.plane + (size_t)f * PL.frame_stride + (size_t)y0 * PL.stride + x0;
                    const uint8_t* pr = PR.plane + (size_t)f * PR.frame_stride + (size_t)y0 * PR.stride + xr;
                    const int lc = pl[(size_t)STEREO_W * PL.stride + STEREO_W];
                    int rc[STEREO_SHIFTS], acc[STEREO_SHIFTS];
#pragma unroll
                    for (int k = 0; k < STEREO_SHIFTS; ++k) { rc[k] = pr[(size_t)STEREO_W * PR.stride + STEREO_W + k]; acc[k] = 0; }
                    for (int p = lane; p < STEREO_PATCH * STEREO_PATCH; p += 64) {
                        const int i = p / STEREO_PATCH, j = p - STEREO_PATCH * i;
                        const int l = (int)pl[(size_t)i * PL.stride + j] - lc;
                        const uint8_t* b = pr + (size_t)i * PR.stride + j;
#pragma unroll
                        for (int k = 0; k < STEREO_SHIFTS; ++k) {
                            const int v = l - ((int)b[k] - rc[k]);
                            acc[k] += v < 0 ? -v : v;
                        }
                    }
                    int d[STEREO_SHIFTS];
#pragma unroll
                    for (int k = 0; k < STEREO_SHIFTS; ++k) d[k] = wave_sum_i32(acc[k]);
                    int bestinc;
                    stereo_best_shift(d, bestinc, sad);
                    st = stereo_subpixel(d, bestinc, D.scale[levelL], suR0, uL, maxD, mbf, uR, depth);
                }
            }
        }
    }
    if (lane == 0) {
        D.u_right[oL] = uR; D.depth[oL] = depth; D.status[oL] = (uint8_t)st;
        D.best_r[oL] = bestR; D.ham[oL] = ham; D.sad[oL] = sad;
    }
}

// grid (frames), 256 threads
__global__ __launch_bounds__(256) void stereo_median_kernel(StDev D) {
    __shared__ int hist[256];
    __shared__ int sh[4];   // chosen bin, rank inside it, matches, survivors
    const int f = blockIdx.x, t = (int)threadIdx.x;
    const int nL = clamp_count(D.n_l[f], D.cap_l);
    const uint8_t* status = D.status + (size_t)f * D.cap_l;
    const int32_t* sad = D.sad + (size_t)f * D.cap_l;
    hist[t] = 0;
    if (t < 4) sh[t] = 0;
    __syncthreads();
    for (int i = t; i < nL; i += 256)
        if (status[i] == STEREO_MATCHED) atomicAdd(&hist[min(sad[i] >> 8, 255) & 255], 1);
    __syncthreads();
    if (t == 0) {
        int m = 0;
        for (int b = 0; b < 256; ++b) m += hist[b];
        sh[2] = m;
        int acc = 0;
        for (int b = 0; b < 256 && m > 0; ++b) {
            if (acc + hist[b] > m / 2) { sh[0] = b; sh[1] = m / 2 - acc; break; }
            acc += hist[b];
        }
    }
    __syncthreads();
    if (sh[2] == 0) {                     // an empty match list: no median (the same for every thread)
        if (t == 0) D.n_matched[f] = 0;
        return;
    }
    const int hi = sh[0], rank = sh[1];
    __syncthreads();
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < nL; i += 256)
        if (status[i] == STEREO_MATCHED && (min(sad[i] >> 8, 255) & 255) == hi) atomicAdd(&hist[sad[i] & 255], 1);
    __syncthreads();
    if (t == 0) {
        int acc = 0, lo = 255;
        for (int b = 0; b < 256; ++b) {
            if (acc + hist[b] > rank) { lo = b; break; }
            acc += hist[b];
        }
        sh[0] = (hi << 8) | lo;
    }
    __syncthreads();
    const float th = stereo_th_dist(sh[0]);
    float* u_right = D.u_right + (size_t)f * D.cap_l;
    float* depth = D.depth + (size_t)f * D.cap_l;
    uint8_t* status_w = D.status + (size_t)f * D.cap_l;
    int kept = 0;
    for (int i = t; i < nL; i += 256) {
        if (status[i] != STEREO_MATCHED) continue;
        if (stereo_removed(sad[i], th)) { status_w[i] = STEREO_MEDIAN; u_right[i] = -1.0f; depth[i] = -1.0f; }
        else ++kept;
    }
    if (kept) atomicAdd(&sh[3], kept);
    __syncthreads();
    if (t == 0) D.n_matched[f] = sh[3];
}

static size_t stereo_workspace_bytes(int nframes, int cap_right) {
    return sizeof(int4) * (size_t)std::max(nframes, 0) * (size_t)std::max(cap_right, 0) + 256;
}

static int view_check(const slamit_pyramid_view& V, int nframes, const char* msg) {
    if (V.nlevels < 1 || V.nlevels > SLAMIT_MAX_LEVELS || V.nframes < nframes) return slamit_fail(SLAMIT_ERR_ARG, msg);
    for (int l = 0; l < V.nlevels; ++l) {
        const slamit_pyramid_level& P = V.level[l];
        if (!P.plane || P.w < 1 || P.h < 1 || P.stride < (size_t)P.w) return slamit_fail(SLAMIT_ERR_ARG, msg);
    }
    return SLAMIT_OK;
}

// the three launches; the caller has made the device current and checked nothing yet
static int stereo_launch(const slamit_stereo_batch* B, hipStream_t stream) {
    const char* const where = "slamit_stereo_match_batch_dev";
    if (!B || B->nframes < 0 || B->cap_left < 0 || B->cap_right < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_stereo_match_batch_dev: bad argument");
    if (B->cap_left > SLAMIT_STEREO_MAX_KP || B->cap_right > SLAMIT_STEREO_MAX_KP)
        return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_stereo_match_batch_dev: more than SLAMIT_STEREO_MAX_KP keypoints per side");
    if (B->nframes == 0) return SLAMIT_OK;
    if (B->nframes > 65535) return slamit_fail(SLAMIT_ERR_ARG, "slamit_stereo_match_batch_dev: more than 65535 frames");
    int rc = view_check(B->left, B->nframes, "slamit_stereo_match_batch_dev: bad left pyramid view");
    if (rc == SLAMIT_OK) rc = view_check(B->right, B->nframes, "slamit_stereo_match_batch_dev: bad right pyramid view");
    if (rc != SLAMIT_OK) return rc;
    if (B->left.nlevels != B->right.nlevels) return slamit_fail(SLAMIT_ERR_ARG, "slamit_stereo_match_batch_dev: the two views differ in levels");
    if (!B->d_n_left || !B->d_n_right || !B->d_mb || !B->d_mbf || !B->d_scale || !B->d_inv_scale || !B->d_u_right || !B->d_depth || !B->d_status ||
        !B->d_best_r || !B->d_ham_dist || !B->d_sad_dist || !B->d_n_matched || (B->cap_left && (!B->d_kps_left || !B->d_desc_left)) ||
        (B->cap_right && (!B->d_kps_right || !B->d_desc_right || !B->d_workspace)))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_stereo_match_batch_dev: null array");
    if (((uintptr_t)B->d_desc_left | (uintptr_t)B->d_desc_right | (uintptr_t)B->d_workspace) & 15)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_stereo_match_batch_dev: descriptors and workspace must be 16-byte aligned");
    if (B->workspace_bytes < stereo_workspace_bytes(B->nframes, B->cap_right))
        return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_stereo_match_batch_dev: workspace smaller than slamit_stereo_match_workspace()");
    StDev D;
    memset(&D, 0, sizeof(D));
    D.nframes = B->nframes; D.cap_l = B->cap_left; D.cap_r = B->cap_right; D.rows = B->left.level[0].h; D.nlevels = B->left.nlevels;
    memcpy(&D.L, &B->left, sizeof(D.L)); memcpy(&D.R, &B->right, sizeof(D.R));
    D.kps_l = B->d_kps_left; D.desc_l = B->d_desc_left; D.n_l = B->d_n_left;
    D.kps_r = B->d_kps_right; D.desc_r = B->d_desc_right; D.n_r = B->d_n_right;
    D.mb = B->d_mb; D.mbf = B->d_mbf; D.scale = B->d_scale; D.inv_scale = B->d_inv_scale;
    D.recs = reinterpret_cast<int4*>(B->d_workspace);
    D.u_right = B->d_u_right; D.depth = B->d_depth; D.status = B->d_status; D.best_r = B->d_best_r; D.ham = B->d_ham_dist; D.sad = B->d_sad_dist;
    D.n_matched = B->d_n_matched;
    if (B->cap_right) hipLaunchKernelGGL(stereo_records_kernel, dim3((B->cap_right + 255) / 256, B->nframes), dim3(256), 0, stream, D);
    if (B->cap_left) hipLaunchKernelGGL(stereo_match_kernel, dim3((B->cap_left + 3) / 4, B->nframes), dim3(256), 0, stream, D);
    hipLaunchKernelGGL(stereo_median_kernel, dim3(B->nframes), dim3(256), 0, stream, D);
    HIP_TRY_AT(where, hipGetLastError());
    return SLAMIT_OK;
}

extern "C" {

size_t slamit_stereo_match_workspace(int nframes, int cap_right) { return stereo_workspace_bytes(nframes, cap_right); }

int slamit_stereo_match_batch_dev(int device, const slamit_stereo_batch* B, void* stream) {
    if (!B) return slamit_fail(SLAMIT_ERR_ARG, "slamit_stereo_match_batch_dev: bad argument");
    if (B->cap_left > SLAMIT_STEREO_MAX_KP || B->cap_right > SLAMIT_STEREO_MAX_KP)
        return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_stereo_match_batch_dev: more than SLAMIT_STEREO_MAX_KP keypoints per side");
    SLAMIT_USE_DEVICE(device);
    return stereo_launch(B, (hipStream_t)stream);
}

int slamit_stereo_match(slamit_orb* left, slamit_orb* right, int frame, const slamit_kp* kps_left, const uint8_t* desc_left, int n_left,
                        const slamit_kp* kps_right, const uint8_t* desc_right, int n_right, float mb, float mbf, float* u_right, float* depth,
                        uint8_t* status, int32_t* best_r, int32_t* ham_dist, int32_t* sad_dist, int32_t* n_matched) {
    const char* const where = "slamit_stereo_match";
    if (!left || !right || n_left < 0 || n_right < 0 || frame < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_stereo_match: bad argument");
    if (n_left > SLAMIT_STEREO_MAX_KP || n_right > SLAMIT_STEREO_MAX_KP)
        return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_stereo_match: more than SLAMIT_STEREO_MAX_KP keypoints per side");
    if ((n_left && (!kps_left || !desc_left || !u_right || !depth || !status)) || (n_right && (!kps_right || !desc_right)))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_stereo_match: null array");
    slamit_pyramid_view VL, VR;
    int rc = slamit_orb_pyramid_view(left, &VL);
    if (rc == SLAMIT_OK) rc = slamit_orb_pyramid_view(right, &VR);
    if (rc != SLAMIT_OK) return rc;
    float scale[2][SLAMIT_MAX_LEVELS] = {}, inv[2][SLAMIT_MAX_LEVELS] = {};
    rc = slamit_orb_tables(left, scale[0], inv[0], nullptr, nullptr, nullptr);
    if (rc == SLAMIT_OK) rc = slamit_orb_tables(right, scale[1], inv[1], nullptr, nullptr, nullptr);
    if (rc != SLAMIT_OK) return rc;
    const int device = slamit_orb_device_of(left);
    if (device != slamit_orb_device_of(right) || VL.nlevels != VR.nlevels || VL.level[0].w != VR.level[0].w || VL.level[0].h != VR.level[0].h ||
        memcmp(scale[0], scale[1], sizeof(scale[0])) != 0)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_stereo_match: the two extractors differ in device, geometry or levels");
    if (frame >= VL.nframes || frame >= VR.nframes) return slamit_fail(SLAMIT_ERR_STATE, "slamit_stereo_match: no such frame in the last extract calls");
    for (int l = 0; l < VL.nlevels; ++l) {    // frame `frame` of the handles becomes frame 0 of a batch of one
        VL.level[l].plane += (size_t)frame * VL.level[l].frame_stride;
        VR.level[l].plane += (size_t)frame * VR.level[l].frame_stride;
    }
    VL.nframes = VR.nframes = 1;
    SLAMIT_USE_DEVICE(device);
    // [keypoints and descriptors of both sides | counts, mb, mbf, tables] go up; the six outputs and the count come down
    StageLayout L;
    const size_t nl = (size_t)n_left, nr = (size_t)n_right;
    const StageSpan<slamit_kp> s_kl = L.take<slamit_kp>(nl, 16), s_kr = L.take<slamit_kp>(nr, 16);
    const StageSpan<uint8_t> s_dl = L.take<uint8_t>(32 * nl, 16), s_dr = L.take<uint8_t>(32 * nr, 16);
    const StageSpan<int32_t> s_n = L.take<int32_t>(2, 16);
    const StageSpan<float> s_f = L.take<float>(2 + 2 * SLAMIT_MAX_LEVELS, 16);
    L.end_inputs();
    const StageSpan<float> s_u = L.take<float>(nl, 16), s_d = L.take<float>(nl, 16);
    const StageSpan<int32_t> s_br = L.take<int32_t>(nl, 16), s_h = L.take<int32_t>(nl, 16), s_s = L.take<int32_t>(nl, 16), s_nm = L.take<int32_t>(1, 16);
    const StageSpan<uint8_t> s_st = L.take<uint8_t>(nl, 16);
    L.end_outputs();
    const StageSpan<uint8_t> s_ws = L.take<uint8_t>(stereo_workspace_bytes(1, n_right), 256);
    static thread_local SlamitScratch S;
    HIP_TRY_AT(where, slamit_stage_reserve(S, device, L));
    if (nl) { memcpy(s_kl.at(S.host), kps_left, s_kl.bytes()); memcpy(s_dl.at(S.host), desc_left, s_dl.bytes()); }
    if (nr) { memcpy(s_kr.at(S.host), kps_right, s_kr.bytes()); memcpy(s_dr.at(S.host), desc_right, s_dr.bytes()); }
    s_n.at(S.host)[0] = n_left; s_n.at(S.host)[1] = n_right;
    float* fl = s_f.at(S.host);
    fl[0] = mb; fl[1] = mbf;
    memcpy(fl + 2, scale[0], sizeof(scale[0])); memcpy(fl + 2 + SLAMIT_MAX_LEVELS, inv[0], sizeof(inv[0]));
    HIP_TRY_AT(where, slamit_stage_upload(S, L));
    slamit_stereo_batch B;
    memset(&B, 0, sizeof(B));
    B.nframes = 1; B.cap_left = n_left; B.cap_right = n_right;
    B.left = VL; B.right = VR;
    B.d_kps_left = s_kl.at(S.dev); B.d_desc_left = s_dl.at(S.dev); B.d_n_left = s_n.at(S.dev);
    B.d_kps_right = s_kr.at(S.dev); B.d_desc_right = s_dr.at(S.dev); B.d_n_right = s_n.at(S.dev) + 1;
    B.d_mb = s_f.at(S.dev); B.d_mbf = s_f.at(S.dev) + 1; B.d_scale = s_f.at(S.dev) + 2; B.d_inv_scale = s_f.at(S.dev) + 2 + SLAMIT_MAX_LEVELS;
    B.d_workspace = s_ws.at(S.dev); B.workspace_bytes = s_ws.bytes();
    B.d_u_right = s_u.at(S.dev); B.d_depth = s_d.at(S.dev); B.d_status = s_st.at(S.dev); B.d_best_r = s_br.at(S.dev); B.d_ham_dist = s_h.at(S.dev);
    B.d_sad_dist = s_s.at(S.dev); B.d_n_matched = s_nm.at(S.dev);
    rc = stereo_launch(&B, S.st);
    if (rc != SLAMIT_OK) return rc;
    HIP_TRY_AT(where, slamit_stage_download_and_wait(S, L));
    if (nl) {
        memcpy(u_right, s_u.at(S.host), s_u.bytes()); memcpy(depth, s_d.at(S.host), s_d.bytes()); memcpy(status, s_st.at(S.host), s_st.bytes());
        if (best_r) memcpy(best_r, s_br.at(S.host), s_br.bytes());
        if (ham_dist) memcpy(ham_dist, s_h.at(S.host), s_h.bytes());
        if (sad_dist) memcpy(sad_dist, s_s.at(S.host), s_s.bytes());
    }
    if (n_matched) *n_matched = s_nm.at(S.host)[0];
    return SLAMIT_OK;
}

}  // extern "C"
