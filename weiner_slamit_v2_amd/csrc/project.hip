// project.hip — the projections in front of the guided search on the GPU (include/slamit.h, slamit_project*).
//
// Reference: the six loops of shim/ORBmatcher.h that csrc/project.h restates (ORB_SLAM2/src/ORBmatcher.cc:293-407, :829-1100,
// :1102-1330, :1332-1603).  Every map point is independent: ONE LANE takes one point, runs project.h on it and writes the point's
// query at its own index, in the layout the guided search reads.  blockIdx.y is the problem, so the camera record and its form are
// the same for every lane of a wavefront: the record arrives through scalar loads and the switch over the form does not diverge.
// The point arrays are planes, so the 64 loads of a wavefront are contiguous.  No LDS, no atomics.  Host form: the accepted points
// of a wavefront are a ballot's popcount, one slot per wavefront, summed on the host.  Device form: frustum.hip's count launch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "project.h"

static_assert(sizeof(ProjectCamera) == sizeof(slamit_project_camera) && offsetof(ProjectCamera, form) == offsetof(slamit_project_camera, form) &&
                  offsetof(ProjectCamera, R2) == offsetof(slamit_project_camera, R2) && offsetof(ProjectCamera, fx) == offsetof(slamit_project_camera, fx) &&
                  offsetof(ProjectCamera, min_x) == offsetof(slamit_project_camera, min_x) && offsetof(ProjectCamera, th) == offsetof(slamit_project_camera, th) &&
                  offsetof(ProjectCamera, scale_factors) == offsetof(slamit_project_camera, scale_factors) &&
                  offsetof(ProjectCamera, direction) == offsetof(slamit_project_camera, direction),
              "slamit_project_camera is ProjectCamera");
static_assert(PRJ_SIM3_PAIR == SLAMIT_PROJECT_SIM3_PAIR && PRJ_LAST_FRAME == SLAMIT_PROJECT_LAST_FRAME, "the forms of project.h are the C-ABI's");

// The arrays of one camera's points; `plane` is the distance between the x, y and z planes of pos / normal.  An input the form does
// not read is never dereferenced (host form: it may be null); the last three of the device form may be null.
struct PrjArrays {
    const SLAMIT_GLOBAL float* pos; const SLAMIT_GLOBAL float* normal; const SLAMIT_GLOBAL float* max_dist; const SLAMIT_GLOBAL float* min_dist;
    const SLAMIT_GLOBAL int32_t* octave; const SLAMIT_GLOBAL uint8_t* skip;
    SLAMIT_GLOBAL float* uvr; SLAMIT_GLOBAL int32_t* level_min; SLAMIT_GLOBAL int32_t* level_max; SLAMIT_GLOBAL uint8_t* valid;
    SLAMIT_GLOBAL uint8_t* status; SLAMIT_GLOBAL float* proj; SLAMIT_GLOBAL int32_t* level;
    SLAMIT_GLOBAL float* ur;   // the right-image column of the stereo calls, or null (wave-uniform)
};

struct PrjProb {
    ProjectCamera C;
    int32_t n, plane;
    float bf;   // mbf of the stereo call (0 without)
    PrjArrays A;
    SLAMIT_GLOBAL int32_t* wave_counts;   // (n + 63) / 64
};

// point i (< n, checked by the caller) of a camera: true = accepted
__device__ __forceinline__ bool project_lane(const ProjectCamera& C, const PrjArrays& A, float bf, size_t plane, size_t i) {
    const int form = C.form;   // wave-uniform
    const float P[3] = {A.pos[i], A.pos[plane + i], A.pos[2 * plane + i]};
    float Pn[3] = {0.f, 0.f, 0.f};
    float max_dist = 0.f, min_dist = 0.f;
    int octave = 0;
    if (prj_form_reads_normal(form)) { Pn[0] = A.normal[i]; Pn[1] = A.normal[plane + i]; Pn[2] = A.normal[2 * plane + i]; }
    if (prj_form_reads_distances(form)) { max_dist = A.max_dist[i]; min_dist = A.min_dist[i]; }
    if (prj_form_reads_octave(form)) octave = A.octave[i];
    ProjectOut o;
    // a form the header does not know (device form only: the host form refuses it) skips every point
    float ur;
    const int st = project_point_stereo(C, P, Pn, max_dist, min_dist, octave, A.skip[i] != 0 || (unsigned)form >= (unsigned)PRJ_FORMS, bf, o, ur);
    float uvr[3];
    int l0, l1;
    unsigned char valid;
    project_query(C, st, o, uvr, l0, l1, valid);
    A.uvr[3 * i] = uvr[0]; A.uvr[3 * i + 1] = uvr[1]; A.uvr[3 * i + 2] = uvr[2];
    A.level_min[i] = l0; A.level_max[i] = l1; A.valid[i] = valid;
    if (A.status) A.status[i] = (uint8_t)st;
    if (A.proj) { A.proj[2 * i] = o.u; A.proj[2 * i + 1] = o.v; }
    if (A.level) A.level[i] = o.level;
    if (A.ur) A.ur[i] = ur;
    return st == PRJ_OK;
}

// grid (ceil(max n / 256), problems), 256 threads: lane t of block b takes point 256 b + t of problem blockIdx.y
__global__ __launch_bounds__(256) void project_kernel(const PrjProb* __restrict__ probs) {
    const PrjProb& P = probs[blockIdx.y];
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P.n) return;
    const bool in = project_lane(P.C, P.A, P.bf, (size_t)P.plane, (size_t)i);
    const unsigned long long m = __ballot(in);   // the lanes past n have left: they count as 0
    // the point index rises with the lane, so lane 0 of a wavefront that has any live lane is live itself
    if ((threadIdx.x & 63) == 0) P.wave_counts[i >> 6] = __popcll(m);
}

// The device form's records stay where the caller keeps them; the batch itself travels as the kernel's argument.
struct PrjDev {
    int32_t q_cap;
    const ProjectCamera* cameras; const int32_t* m;
    const float* bf;   // [nframes] or null
    PrjArrays A;   // frame 0's; frame f's start f * q_cap entries (3 f * q_cap for the planes and uvr, 2 f * q_cap for proj) further on
};

__global__ __launch_bounds__(256) void project_dev_kernel(PrjDev D) {
    const size_t f = blockIdx.y, q_cap = (size_t)D.q_cap;
    const int m = min(D.m[f], D.q_cap);
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= m) return;
    const size_t o = f * q_cap;
    PrjArrays A;
    A.pos = D.A.pos + 3 * o; A.normal = D.A.normal + 3 * o; A.max_dist = D.A.max_dist + o; A.min_dist = D.A.min_dist + o;
    A.octave = D.A.octave + o; A.skip = D.A.skip + o;
    A.uvr = D.A.uvr + 3 * o; A.level_min = D.A.level_min + o; A.level_max = D.A.level_max + o; A.valid = D.A.valid + o;
    A.status = D.A.status ? D.A.status + o : nullptr; A.proj = D.A.proj ? D.A.proj + 2 * o : nullptr; A.level = D.A.level ? D.A.level + o : nullptr;
    A.ur = D.A.ur ? D.A.ur + o : nullptr;
    // n_levels is the caller's, unchecked: project_point accepts a level only below min(n_levels, FRU_MAX_LEVELS) and masks the index
    project_lane(D.cameras[f], A, D.bf ? D.bf[f] : 0.f, q_cap, (size_t)i);
}

extern "C" {

int slamit_project_batch_stereo(int device, int nprob, const slamit_project_problem* probs, slamit_project_result* results, const float* bf,
                                float* const* ur) {
    const char* const where = "slamit_project_batch";
    if (nprob < 0 || (nprob && (!probs || !results))) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch: bad argument");
    if (!bf != !ur) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch_stereo: exactly one of bf / ur is null");
    if (nprob == 0) return SLAMIT_OK;
    if (nprob > 65535) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch: more than 65535 problems");
    int max_n = 0;
    for (int f = 0; f < nprob; ++f) {
        const slamit_project_problem& P = probs[f];
        const slamit_project_result& R = results[f];
        if (P.n < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch: negative count");
        if (P.n > SLAMIT_PROJECT_MAX_N) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch: more than SLAMIT_PROJECT_MAX_N points");
        if (P.n == 0) continue;   // nothing to project, nothing read
        const int form = P.camera.form;
        if (form < 0 || form >= PRJ_FORMS) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch: unknown form");
        if (P.camera.direction < 0 || P.camera.direction > 2) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch: unknown direction");
        if (P.camera.n_levels < 1 || P.camera.n_levels > SLAMIT_MAX_LEVELS)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch: n_levels outside [1, SLAMIT_MAX_LEVELS]");
        if (!P.pos || !P.skip || (prj_form_reads_normal(form) && !P.normal) || (prj_form_reads_distances(form) && (!P.max_dist || !P.min_dist)) ||
            (prj_form_reads_octave(form) && !P.octave) || !R.status || !R.proj || !R.level || !R.uvr || !R.level_min || !R.level_max || !R.valid)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch: null array");
        if (ur && !ur[f]) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch_stereo: null ur of a problem with points");
        max_n = std::max(max_n, (int)P.n);
    }
    for (int f = 0; f < nprob; ++f) results[f].n_valid = 0;
    if (max_n == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(device);
    // [records | per problem: pos normal (planes) max_dist min_dist octave skip] go up; [per problem: the seven outputs, wave counts, ur] come
    // down; an input the form does not read takes no room
    std::vector<StageView<int32_t>> waves(nprob);
    static thread_local SlamitScratch S;
    const int rc = slamit_staged_batch<PrjProb>(
        where, S, device, nprob,
        [&](StageBinder& b, int f, PrjProb& Q) {
            const slamit_project_problem& P = probs[f];
            const slamit_project_result& R = results[f];
            const size_t n = (size_t)P.n;
            const int form = P.camera.form;
            Q.n = P.n; Q.plane = P.n; Q.bf = bf ? bf[f] : 0.f;
            if (n) memcpy(&Q.C, &P.camera, sizeof(Q.C));
            const size_t nn = prj_form_reads_normal(form) ? n : 0, nd = prj_form_reads_distances(form) ? n : 0, no = prj_form_reads_octave(form) ? n : 0;
            float *pp, *pn;
            Q.A.pos = slamit_global(b.in_fill<float>(3 * n, &pp)); Q.A.normal = slamit_global(b.in_fill<float>(3 * nn, &pn));
            if (pp)   // the caller's n x 3 rows become three planes
                for (int c = 0; c < 3; ++c) {
                    for (size_t i = 0; i < n; ++i) pp[c * n + i] = P.pos[3 * i + c];
                    for (size_t i = 0; i < nn; ++i) pn[c * n + i] = P.normal[3 * i + c];
                }
            Q.A.max_dist = slamit_global(b.in(P.max_dist, nd)); Q.A.min_dist = slamit_global(b.in(P.min_dist, nd));
            Q.A.octave = slamit_global(b.in(P.octave, no)); Q.A.skip = slamit_global(b.in(P.skip, n));
            Q.A.status = slamit_global(b.out(R.status, n)); Q.A.proj = slamit_global(b.out(R.proj, 2 * n));
            Q.A.level = slamit_global(b.out(R.level, n));
            Q.A.uvr = slamit_global(b.out(R.uvr, 3 * n)); Q.A.level_min = slamit_global(b.out(R.level_min, n));
            Q.A.level_max = slamit_global(b.out(R.level_max, n)); Q.A.valid = slamit_global(b.out(R.valid, n));
            Q.A.ur = ur && n ? slamit_global(b.out(ur[f], n)) : nullptr;
            Q.wave_counts = slamit_global(b.out_view((n + 63) / 64, &waves[f]));
        },
        [&](const PrjProb* d_recs) {
            hipLaunchKernelGGL(project_kernel, dim3((max_n + 255) / 256, nprob), dim3(256), 0, S.st, d_recs);
            return hipGetLastError();
        });
    if (rc != SLAMIT_OK) return rc;
    for (int f = 0; f < nprob; ++f) results[f].n_valid = stage_sum(waves[f].data, waves[f].count);
    return SLAMIT_OK;
}

int slamit_project_batch(int device, int nprob, const slamit_project_problem* probs, slamit_project_result* results) {
    return slamit_project_batch_stereo(device, nprob, probs, results, nullptr, nullptr);
}

int slamit_project(int device, const slamit_project_problem* prob, slamit_project_result* res) {
    return slamit_project_batch(device, 1, prob, res);
}

int slamit_project_batch_dev_stereo(int device, const slamit_project_batch_rec* B, const float* d_bf, float* d_ur, void* stream) {
    if (!B || B->nframes < 0 || B->q_cap < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch_dev: bad argument");
    if (!d_bf != !d_ur) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch_dev_stereo: exactly one of d_bf / d_ur is null");
    if (B->q_cap > SLAMIT_PROJECT_MAX_N) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch_dev: q_cap above SLAMIT_PROJECT_MAX_N");
    if (B->nframes == 0 || B->q_cap == 0) return SLAMIT_OK;
    if (!B->d_cameras || !B->d_m || !B->d_pos || !B->d_normal || !B->d_max_dist || !B->d_min_dist || !B->d_octave || !B->d_skip || !B->d_uvr ||
        !B->d_level_min || !B->d_level_max || !B->d_valid)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch_dev: null array");
    if (B->nframes > 65535) return slamit_fail(SLAMIT_ERR_ARG, "slamit_project_batch_dev: more than 65535 frames");
    SLAMIT_USE_DEVICE(device);
    PrjDev D;
    D.q_cap = B->q_cap;
    D.cameras = reinterpret_cast<const ProjectCamera*>(B->d_cameras); D.m = B->d_m;
    D.A.pos = (const SLAMIT_GLOBAL float*)B->d_pos; D.A.normal = (const SLAMIT_GLOBAL float*)B->d_normal;
    D.A.max_dist = (const SLAMIT_GLOBAL float*)B->d_max_dist; D.A.min_dist = (const SLAMIT_GLOBAL float*)B->d_min_dist;
    D.A.octave = (const SLAMIT_GLOBAL int32_t*)B->d_octave; D.A.skip = (const SLAMIT_GLOBAL uint8_t*)B->d_skip;
    D.A.uvr = (SLAMIT_GLOBAL float*)B->d_uvr; D.A.level_min = (SLAMIT_GLOBAL int32_t*)B->d_level_min;
    D.A.level_max = (SLAMIT_GLOBAL int32_t*)B->d_level_max; D.A.valid = (SLAMIT_GLOBAL uint8_t*)B->d_valid;
    D.A.status = (SLAMIT_GLOBAL uint8_t*)B->d_status; D.A.proj = (SLAMIT_GLOBAL float*)B->d_proj; D.A.level = (SLAMIT_GLOBAL int32_t*)B->d_level;
    D.bf = d_bf; D.A.ur = (SLAMIT_GLOBAL float*)d_ur;
    hipLaunchKernelGGL(project_dev_kernel, dim3((B->q_cap + 255) / 256, B->nframes), dim3(256), 0, (hipStream_t)stream, D);
    HIP_TRY_AT("slamit_project_batch_dev", hipGetLastError());
    if (B->d_n_valid)
        HIP_TRY_AT("slamit_project_batch_dev", slamit_launch_valid_count(B->d_valid, B->d_m, B->q_cap, B->nframes, B->d_n_valid, (hipStream_t)stream));
    return SLAMIT_OK;
}

int slamit_project_batch_dev(int device, const slamit_project_batch_rec* B, void* stream) {
    return slamit_project_batch_dev_stereo(device, B, nullptr, nullptr, stream);
}

}  // extern "C"
