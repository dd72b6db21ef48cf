// project.h — one map point of the six projection loops that sit in front of the guided search in shim/ORBmatcher.h: world ->
// camera, the depth, bounds, distance and viewing-angle gates, MapPoint::PredictScale and the window radius.  Plain C++ over IEEE
// +,-,*,/ and sqrt, float and double exactly where the shim's loops have them; it must be compiled with -ffp-contract=off.
// project.hip runs it one lane per point; the CPU test of the restatement and tools build the same text with g++ for the host.
// fru_gemm_row3, fru_logf and fru_predict_scale are csrc/frustum.h's.  project_point_stereo also gives the right-image column the
// guided search's `er` gate reads.
//
// THE PINNED READING is the host loop of each driver in shim/ORBmatcher.h; a difference from it is a bug here.
//
//   form        driver (reference)                                  transform            depth test          invz
//   LAST_FRAME  SearchByProjection(Current, Last)  ORBmatcher.cc:1332  gemm rows (R, t)     invz < 0 rejects    (float)(1.0 / (double)zc)
//   RELOC       SearchByProjection(Frame, KF, set) :1476               gemm rows            none                (float)(1.0 / (double)zc)
//   FUSE        Fuse(KF, points, th)               :829                gemm rows            zc < 0.0f           1.0f / zc
//   SIM3_PROJ   SearchByProjection(KF, Scw, ...)   :293                all-float R p + t    z < 0               1.0f / z
//   SIM3_FUSE   Fuse(KF, Scw, ...)                 :981                all-float            z < 0               (float)(1.0 / (double)z)
//   SIM3_PAIR   SearchBySim3, one direction        :1102               (R, t) then (R2, t2) z < 0               (float)(1.0 / (double)z)
//
//   u, v        LAST_FRAME, RELOC: ((fx * xc) * invz) + cx.  The others: x = xc * invz; (fx * x) + cx
//   bounds      LAST_FRAME, RELOC: the frame's closed test `u < min_x || u > max_x`, which a NaN passes.
//               The others: KeyFrame::IsInImage, `u >= min_x && u < max_x`, which a NaN fails.  u decides code 3, then v code 4.
//   dist        (float)sqrt(double sum of double squares, in order) of P - O; of the camera-frame point for SIM3_PAIR; none for LAST_FRAME
//   gates       dist < 0.8f * min_dist || dist > 1.2f * max_dist on the RAW distances (= Get{Min,Max}DistanceInvariance())
//   angle       FUSE, SIM3_PROJ, SIM3_FUSE: (((double)PO0 Pn0 + (double)PO1 Pn1) + (double)PO2 Pn2) < 0.5 * (double)dist rejects
//   level       LAST_FRAME: the octave given; the others: fru_predict_scale(max_dist, dist, log_scale_factor)
//   window      r = th * scale_factors[level].  Levels: LAST_FRAME by direction (0: l-1..l+1; 1 forward: l..-1 = no upper bound;
//               2 backward: 0..l); RELOC l-1..l+1; the others l-1..l
//
//   ur          project_point_stereo only: u - bf * invz, two roundings, with the form's own invz above (LAST_FRAME :1413, FUSE :874).
//               Only LAST_FRAME and FUSE have a reader of it in the reference.  Status 0 only; zero otherwise.
//
// ONE STATED DEPARTURE, csrc/frustum.h's: the loops index mvScaleFactors with the level unchecked.  Here a level outside
// [0, n_levels), predicted or given as an octave, and a ratio no level comes from, is status PRJ_LEVEL (7): no query, and the level
// reported is INT32_MIN.
//
// Outputs of a rejected point: every field the walk did not reach is zero.  u and v are written once the depth test has passed
// (codes 3..7 and 0); level and r for code 0 only (code 7 reports INT32_MIN).
#ifndef SLAMIT_PROJECT_H
#define SLAMIT_PROJECT_H
#include "frustum.h"

enum { PRJ_LAST_FRAME = 0, PRJ_RELOC = 1, PRJ_FUSE = 2, PRJ_SIM3_PROJ = 3, PRJ_SIM3_FUSE = 4, PRJ_SIM3_PAIR = 5, PRJ_FORMS = 6 };
enum { PRJ_OK = 0, PRJ_SKIPPED = 1, PRJ_DEPTH = 2, PRJ_U = 3, PRJ_V = 4, PRJ_DISTANCE = 5, PRJ_ANGLE = 6, PRJ_LEVEL = 7 };

// What the camera contributes, computed once on the host as the shim does today (sim3detail::decompose; the -Rcw.t() * tcw rows
// summed in double; SearchBySim3's sR12 / sR21 / t21).  Layout of slamit_project_camera.
struct ProjectCamera {
    int form;                      // PRJ_*
    float R[9], t[3], O[3];        // world -> camera (SIM3_PAIR: the pose of the keyframe the points come from), the camera centre
    float R2[9], t2[3];            // SIM3_PAIR: the similarity into the other camera (sR21, t21 or sR12, t12)
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y;
    float log_scale_factor, th;
    int n_levels;
    float scale_factors[FRU_MAX_LEVELS];
    int direction;                 // LAST_FRAME: 0, 1 = forward, 2 = backward
};

struct ProjectOut {
    float u, v, r;
    int level;
};

// sim3detail::apply: R p + t, all float, left to right
FRU_HD void prj_apply(const float* R, const float* t, const float p[3], float out[3]) {
    out[0] = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + t[0];
    out[1] = R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + t[1];
    out[2] = R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + t[2];
}

FRU_HD bool prj_form_reads_normal(int form) { return form == PRJ_FUSE || form == PRJ_SIM3_PROJ || form == PRJ_SIM3_FUSE; }
FRU_HD bool prj_form_reads_distances(int form) { return form != PRJ_LAST_FRAME; }
FRU_HD bool prj_form_reads_octave(int form) { return form == PRJ_LAST_FRAME; }

// One point: the code of the first test that rejects it (0 = a query).  Pn, max_dist, min_dist and octave are read only by the
// forms the three predicates above name.  bf is the camera's mbf, ur the right-image column of an accepted point.
FRU_HD int project_point_stereo(const ProjectCamera& C, const float P[3], const float Pn[3], float max_dist, float min_dist, int octave, bool skip,
                                float bf, ProjectOut& o, float& ur) {
    o.u = 0.f; o.v = 0.f; o.r = 0.f; o.level = 0;
    ur = 0.f;
    if (skip) return PRJ_SKIPPED;
    const int form = C.form;
    float pc[3];
    if (form <= PRJ_FUSE) {
        pc[0] = fru_gemm_row3(&C.R[0], P, C.t[0]);
        pc[1] = fru_gemm_row3(&C.R[3], P, C.t[1]);
        pc[2] = fru_gemm_row3(&C.R[6], P, C.t[2]);
    } else if (form == PRJ_SIM3_PAIR) {
        float pa[3];
        prj_apply(C.R, C.t, P, pa);
        prj_apply(C.R2, C.t2, pa, pc);
    } else {
        prj_apply(C.R, C.t, P, pc);
    }
    float invz;
    if (form == PRJ_LAST_FRAME) {
        invz = (float)(1.0 / (double)pc[2]);
        if (invz < 0) return PRJ_DEPTH;
    } else if (form == PRJ_RELOC) {
        invz = (float)(1.0 / (double)pc[2]);
    } else {
        if (pc[2] < 0.0f) return PRJ_DEPTH;
        invz = (form == PRJ_FUSE || form == PRJ_SIM3_PROJ) ? 1.0f / pc[2] : (float)(1.0 / (double)pc[2]);
    }
    float u, v;
    if (form <= PRJ_RELOC) {
        u = C.fx * pc[0] * invz + C.cx;
        v = C.fy * pc[1] * invz + C.cy;
    } else {
        const float x = pc[0] * invz, y = pc[1] * invz;
        u = C.fx * x + C.cx;
        v = C.fy * y + C.cy;
    }
    o.u = u; o.v = v;
    if (form <= PRJ_RELOC) {
        if (u < C.min_x || u > C.max_x) return PRJ_U;
        if (v < C.min_y || v > C.max_y) return PRJ_V;
    } else {
        if (!(u >= C.min_x && u < C.max_x)) return PRJ_U;
        if (!(v >= C.min_y && v < C.max_y)) return PRJ_V;
    }
    int level = octave;
    if (form != PRJ_LAST_FRAME) {
        float D[3] = {P[0] - C.O[0], P[1] - C.O[1], P[2] - C.O[2]};
        if (form == PRJ_SIM3_PAIR) { D[0] = pc[0]; D[1] = pc[1]; D[2] = pc[2]; }
        const float dist = (float)sqrt(((double)D[0] * (double)D[0] + (double)D[1] * (double)D[1]) + (double)D[2] * (double)D[2]);
        if (dist < 0.8f * min_dist || dist > 1.2f * max_dist) return PRJ_DISTANCE;
        if (prj_form_reads_normal(form)) {
            const double dot = ((double)D[0] * (double)Pn[0] + (double)D[1] * (double)Pn[1]) + (double)D[2] * (double)Pn[2];
            if (dot < 0.5 * (double)dist) return PRJ_ANGLE;
        }
        if (!fru_predict_scale(max_dist, dist, C.log_scale_factor, level)) level = FRU_LEVEL_NONE;
    }
    if (level < 0 || level >= C.n_levels || level >= FRU_MAX_LEVELS) { o.level = FRU_LEVEL_NONE; return PRJ_LEVEL; }
    o.level = level;
    o.r = C.th * C.scale_factors[level & (FRU_MAX_LEVELS - 1)];
    ur = u - bf * invz;
    return PRJ_OK;
}

// The same without the right-image column
FRU_HD int project_point(const ProjectCamera& C, const float P[3], const float Pn[3], float max_dist, float min_dist, int octave, bool skip,
                         ProjectOut& o) {
    float ur;
    return project_point_stereo(C, P, Pn, max_dist, min_dist, octave, skip, 0.f, o, ur);
}

// The slamit_search_queries row of a point; queries are not compacted: a rejected point is a query with valid = 0 and zeros.
FRU_HD void project_query(const ProjectCamera& C, int status, const ProjectOut& o, float uvr[3], int& level_min, int& level_max, unsigned char& valid) {
    const bool in = status == PRJ_OK;
    const int l = in ? o.level : 0;   // a rejected point's level may be INT32_MIN: no arithmetic on it
    int l0 = l - 1, l1 = l;
    if (C.form == PRJ_RELOC) l1 = l + 1;
    if (C.form == PRJ_LAST_FRAME) {
        if (C.direction == 1) { l0 = l; l1 = -1; }
        else if (C.direction == 2) { l0 = 0; l1 = l; }
        else l1 = l + 1;
    }
    uvr[0] = in ? o.u : 0.f; uvr[1] = in ? o.v : 0.f; uvr[2] = in ? o.r : 0.f;
    level_min = in ? l0 : 0; level_max = in ? l1 : 0;
    valid = in ? 1 : 0;
}

#endif
