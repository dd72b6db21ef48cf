/*
 * slamit.h — C-ABI of libslamit_hip.so: the MI355X (gfx950) implementation of the ORB-SLAM2
 * per-frame hot path of serviceberry3/weiner_slamit_v2.
 *
 * Every entry point replaces one reference interface (paths relative to
 * oRB_SLAM2_Android/src/main/jni/ORB_SLAM2/ unless they start with Thirdparty/):
 *
 *   slamit_orb_*        <- ORBextractor::ORBextractor / operator()      include/ORBextractor.h:45-85,
 *                                                                        src/ORBextractor.cc:415-482,1064-1136
 *   slamit_orb_level    <- public member ORBextractor::mvImagePyramid    include/ORBextractor.h:85
 *   slamit_hamming_*    <- ORBmatcher::DescriptorDistance + best/second  src/ORBmatcher.cc:1651-1667, 85-117,
 *                          selection loops                               440-461, 1404-1428
 *   slamit_stereo_*     <- Frame::ComputeStereoMatches                   src/Frame.cc:591-763
 *   slamit_ba_*         <- Optimizer::LocalBundleAdjustment (the g2o     src/Optimizer.cc:453-778 and
 *                          BlockSolver_6_3 + Levenberg it instantiates)  Thirdparty/g2o/g2o/core/block_solver.hpp
 *
 * Conventions: plain C types only; `int` status return (0 = SLAMIT_OK, <0 = error, text from
 * slamit_last_error()); nothing throws across the boundary; the caller owns every buffer it
 * passes; the library owns device memory inside opaque handles.  Functions with the suffix
 * `_dev` take DEVICE pointers (HBM-resident buffers, e.g. a torch tensor's data_ptr) and a HIP
 * stream handle (`void*` = hipStream_t, NULL = the handle's own stream) and do not synchronise;
 * all others take HOST pointers and return when the result is in the caller's memory.
 * A handle may be used by one thread at a time; distinct handles are independent (the reference
 * runs two extractors on two threads for stereo, src/Frame.cc:93-94).
 */
#ifndef SLAMIT_H
#define SLAMIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAMIT_OK 0
#define SLAMIT_ERR_ARG (-1)      /* bad argument / unsupported geometry */
#define SLAMIT_ERR_DEVICE (-2)   /* HIP runtime error (no GPU, launch failure, out of memory) */
#define SLAMIT_ERR_CAPACITY (-3) /* caller buffer too small */
#define SLAMIT_ERR_STATE (-4)    /* call order (e.g. level requested before any extract) */

#define SLAMIT_DESC_BYTES 32
#define SLAMIT_EDGE_THRESHOLD 19 /* src/ORBextractor.cc:79 */

/* Field order and size identical to cv::KeyPoint (28 bytes) so the ORBextractor shim can
 * memcpy into std::vector<cv::KeyPoint>. */
typedef struct slamit_kp {
    float x, y;     /* level-0 pixel coordinates (already multiplied by the level scale) */
    float size;     /* (float)(int)(31 * scale[octave])        src/ORBextractor.cc:857,866 */
    float angle;    /* degrees in [0,360], fastAtan2 of IC     src/ORBextractor.cc:108 */
    float response; /* FAST-9/16 corner score */
    int32_t octave;
    int32_t class_id; /* always -1 */
} slamit_kp;

/* ---- ORB extractor --------------------------------------------------------------------- */

typedef struct slamit_orb_params {
    int32_t nfeatures;  /* 1000 (tracking) / 2000 (initialiser)  src/Tracking.cc:149,162 */
    float scale_factor; /* 1.2f */
    int32_t nlevels;    /* 8, at most SLAMIT_MAX_LEVELS */
    int32_t ini_th_fast; /* 20 */
    int32_t min_th_fast; /* 7 */
    int32_t width, height; /* frame geometry is fixed per handle */
    int32_t max_batch;     /* frames per extract_batch call the handle is sized for (>=1) */
} slamit_orb_params;

#define SLAMIT_MAX_LEVELS 16

typedef struct slamit_orb slamit_orb;

int slamit_orb_create(const slamit_orb_params* params, int device, slamit_orb** out);
void slamit_orb_destroy(slamit_orb* h);

/* Scale tables (GetScaleFactors & friends, include/ORBextractor.h:64-82). Each out array has
 * nlevels entries; any may be NULL. */
int slamit_orb_tables(const slamit_orb* h, float* scale, float* inv_scale, float* sigma2,
                      float* inv_sigma2, int32_t* features_per_level);

/* Upper bound on keypoints one frame can return: nfeatures + 3*nlevels (the octree may
 * overshoot each level's quota by up to 3, src/ORBextractor.cc:743-744). */
int slamit_orb_max_keypoints(const slamit_orb* h);

/* One frame, host buffers: gray is h rows of `stride` bytes. Writes *n_out keypoints
 * (level-major order as the reference concatenates them) and n_out*32 descriptor bytes.
 * cap must be >= slamit_orb_max_keypoints(). Empty image (w or h == 0 at create) -> n_out = 0. */
int slamit_orb_extract(slamit_orb* h, const uint8_t* gray, size_t stride, slamit_kp* kps,
                       uint8_t* desc, int cap, int* n_out);

/* nframes frames, host buffers; frame f at gray + f*frame_stride; outputs for frame f at
 * kps + f*cap, desc + f*cap*32, n_out[f]. */
int slamit_orb_extract_batch(slamit_orb* h, const uint8_t* gray, size_t stride,
                             size_t frame_stride, int nframes, slamit_kp* kps, uint8_t* desc,
                             int cap, int* n_out);

/* Same, device buffers (all pointers are HBM addresses), asynchronous on `stream`. */
int slamit_orb_extract_batch_dev(slamit_orb* h, const uint8_t* d_gray, size_t stride,
                                 size_t frame_stride, int nframes, slamit_kp* d_kps,
                                 uint8_t* d_desc, int cap, int32_t* d_n_out, void* stream);

/* Per-stage device timing with HIP events recorded on the launch stream (the counterpart of
 * g2o's G2OBatchStatistics idea, Thirdparty/g2o/g2o/core/batch_stats.h:39-77, for the extractor).
 * Reads (and clears) what was accumulated since the last call into stage_ms / stage_calls
 * (either may be NULL), then switches recording on/off.  Stages: 0 pyramid resize, 1 FAST cells,
 * 2 octree, 3 IC angle, 4 Gaussian blur, 5 rBRIEF + output.  A "call" is one stage of one
 * extract_batch call (the resize stage launches one kernel per level).  enable: 0 off, 1 every stage,
 * n >= 2 only stage 1 (the dominant kernel) on every (n-1)-th extract call: an event between two kernels costs
 * ~10 us of pipeline drain, so a throughput run that still wants the dominant kernel's live duration samples it. */
#define SLAMIT_ORB_STAGES 6
int slamit_orb_profile(slamit_orb* h, int enable, float* stage_ms, int32_t* stage_calls, int nstages);

/* mvImagePyramid[level] of frame `frame` of the last extract call: copies the padded plane
 * ((w+38) x (h+38), REFLECT_101 border of 19) to host memory. dst may be NULL to query sizes;
 * *w,*h are the un-padded level size, the plane is (*h+38) rows of (*w+38) bytes. */
int slamit_orb_level(slamit_orb* h, int frame, int level, uint8_t* dst, size_t dst_bytes, int* w,
                     int* h_out);

/* Where mvImagePyramid of the last extract call lives in HBM, for callers that read the planes on the device (slamit_stereo_match*):
 * frame f of level l is level[l].plane + f * level[l].frame_stride, h rows of `stride` bytes of which the first w are pixels (no
 * border).  Level 0 is the image the extract call was given (the caller's device buffer for the _dev form, the handle's staging
 * copy for the host forms) with that call's strides; levels >= 1 are the handle's own planes.  The pointers are valid until the
 * next extract call on the handle.  SLAMIT_ERR_STATE before the first extract call, and for a handle created with an empty image. */
typedef struct slamit_pyramid_level {
    const uint8_t* plane;   /* DEVICE pointer: frame 0 of the level */
    int32_t w, h;
    size_t stride;          /* bytes between rows */
    size_t frame_stride;    /* bytes between the frames of a batch */
} slamit_pyramid_level;

typedef struct slamit_pyramid_view {
    int32_t nlevels;
    int32_t nframes;        /* frames of the extract call the planes belong to */
    slamit_pyramid_level level[SLAMIT_MAX_LEVELS];
} slamit_pyramid_view;

int slamit_orb_pyramid_view(const slamit_orb* h, slamit_pyramid_view* out);

/* Stage outputs of the last extract call, for parity debugging (host buffers):
 *  candidates of (frame, level) before the octree as (x, y, score) int32 triplets, x/y relative
 *  to the (16,16) detection border like vToDistributeKeys (src/ORBextractor.cc:840-845), sorted
 *  in the reference's (cell row, cell col, y, x) order. */
int slamit_orb_debug_candidates(slamit_orb* h, int frame, int level, int32_t* xys, int cap,
                                int* n_out);
/*  how the octree pass of (frame, level) ran: bits 0-7 the passes it served from its path table, bit 8 (0x100) set when a pass
 *  needed a depth the table does not hold (or no table fits) and the keys were walked instead.  0 for a level without candidates. */
int slamit_orb_debug_octree_path(slamit_orb* h, int frame, int level, int* path_out);
/*  the blurred level the descriptors were sampled from: GaussianBlur(mvImagePyramid[level].clone(), 7x7, sigma 2,
 *  BORDER_REFLECT_101) of src/ORBextractor.cc:1116-1117, *h_out rows of *w bytes (no border). dst may be NULL
 *  to query the size. */
int slamit_orb_debug_blurred(slamit_orb* h, int frame, int level, uint8_t* dst, size_t dst_bytes, int* w,
                             int* h_out);

/* ---- Hamming matcher -------------------------------------------------------------------- */

#define SLAMIT_HAMMING_MAX_TRAIN 65535   /* train rows per set in the best/second entry points (index packed in 16 bits) */
/* For each of nq query descriptors: best and second-best Hamming distance over the train
 * descriptors, and the index of the best (strict '<', first index wins; the reference's
 * selection rule, src/ORBmatcher.cc:1404-1428). With nt == 0: best = second = 256, idx = -1.  A train row 256 bits
 * away is still a row: when every row is, idx = 0 and best = second = 256 (the reference's loop, which starts from 256, would keep -1;
 * no caller accepts such a match). */
int slamit_hamming_best2(const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* best_idx,
                         int32_t* best, int32_t* second);

/* Batched device form: pair p matches d_q + p*q_stride (nq[p] rows) against d_t + p*t_stride
 * (nt[p] rows); outputs at p*out_stride. d_nq / d_nt are device int32 arrays (they are the
 * d_n_out of extract_batch_dev), max_n bounds both. */
int slamit_hamming_best2_batch_dev(const uint8_t* d_q, const int32_t* d_nq, size_t q_stride,
                                   const uint8_t* d_t, const int32_t* d_nt, size_t t_stride,
                                   int npairs, int max_n, int32_t* d_best_idx, int32_t* d_best,
                                   int32_t* d_second, size_t out_stride, int device, void* stream);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:248-314), batched:
 * map point p owns descriptor rows [offsets[p], offsets[p+1]) of `desc` (its observations, in the
 * reference's iteration order).  For each point: all-pairs Hamming distances, per row the median
 * vDists[(int)(0.5*(N-1))] of the sorted row (self distance 0 included), and the row with the least
 * median (first one on ties) -> best_idx[p] (relative to offsets[p]; -1 for a point without rows),
 * best_median[p].  At most SLAMIT_DISTINCTIVE_MAX rows per point. */
#define SLAMIT_DISTINCTIVE_MAX 128
int slamit_distinctive_batch(const uint8_t* desc, const int32_t* offsets, int npoints, int32_t* best_idx,
                             int32_t* best_median);

/* ---- Guided search ------------------------------------------------------
 * The common core of ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th)
 * (src/ORBmatcher.cc:47-131) and SearchByProjection(CurrentFrame, LastFrame, th, bMono) (:1332-1474):
 * for each query, in order, Frame::GetFeaturesInArea(u, v, r, minLevel, maxLevel)
 * (src/Frame.cc:447-502 over the 64x48 grid of Frame::AssignFeaturesToGrid, :336-357, :505-517),
 * skip keypoints that already carry a map point, take the nearest (and second nearest) descriptor in
 * the reference's candidate order, accept, and MARK THE KEYPOINT TAKEN for the queries that follow
 * (the reference assigns F.mvpMapPoints[bestIdx] inside the loop).  Projection, viewing-cosine radius
 * and the rotation histogram stay with the caller (shim/ORBmatcher.h), except for SearchLocalPoints, whose
 * queries slamit_frustum* below writes in this layout.  slamit_guided_search is the monocular loop; the right-image test that
 * three of the drivers apply to a stereo keypoint (mvuRight) is slamit_guided_search_stereo below. */
typedef struct slamit_frame_view {
    int32_t n;                 /* keypoints */
    const float* kp_xy;        /* n x 2: mvKeysUn[i].pt */
    const int32_t* kp_octave;  /* n */
    const uint8_t* desc;       /* n x 32: mDescriptors */
    const uint8_t* kp_taken;   /* n: 1 = mvpMapPoints[i] && mvpMapPoints[i]->Observations() > 0 on entry */
    float min_x, min_y;        /* mnMinX, mnMinY */
    float inv_w, inv_h;        /* mfGridElementWidthInv, mfGridElementHeightInv */
} slamit_frame_view;

typedef struct slamit_search_queries {
    int32_t m;
    const float* uvr;          /* m x 3: window centre u, v and half-size r (already scaled) */
    const int32_t* level_min;  /* m */
    const int32_t* level_max;  /* m: -1 = no upper bound (GetFeaturesInArea's default) */
    const uint8_t* desc;       /* m x 32: pMP->GetDescriptor() */
    const uint8_t* valid;      /* m: 0 = query skipped (mbTrackInView false, bad point, behind camera ...) */
    const uint8_t* takes;      /* m or NULL (= all 1): 1 = pMP->Observations() > 0, i.e. a keypoint matched to
                                  this query is skipped by the queries that follow */
} slamit_search_queries;

typedef struct slamit_search_rule {
    int32_t th_dist;           /* accept iff bestDist <= th_dist (TH_HIGH = 100, TH_LOW = 50) */
    int32_t use_ratio;         /* 1: also reject when bestLevel == bestLevel2 && bestDist > nnratio * bestDist2 */
    float nnratio;
    /* ORBmatcher::Fuse's per-candidate gate (src/ORBmatcher.cc:925-936): with e2 = (u - kp.x)^2 + (v - kp.y)^2 a
     * candidate is skipped when e2 * inv_level_sigma2[kp.octave] > chi2_gate (5.99).  chi2_gate <= 0: no gate. */
    float chi2_gate;
    float inv_level_sigma2[16];
    /* mode 0: the SearchByProjection / Fuse loop described above.
     * mode 1: ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:409-474): instead of the taken flag a keypoint
     *   carries the distance of its current match; a candidate is skipped when that distance is <= the query's
     *   distance to it (:448); accept iff bestDist <= th_dist && bestDist < (float)bestDist2 * nnratio (bestDist2 =
     *   INT_MAX without a second candidate); an accepted query takes the keypoint over from the query that held it,
     *   whose match_kp entry goes back to -1.  kp_taken / takes / use_ratio / chi2_gate are ignored.  best_level then
 *   reports the keypoint a query was matched to AT ITS OWN TURN (-1 if it was not accepted), which a later take-over
 *   does not reset: the reference bins exactly those into its rotation histogram (:467-477). */
    int32_t mode;
} slamit_search_rule;

/* match_kp[q] = index of the keypoint the query took, or -1; *nmatches = number of accepted queries.
 * best_dist / best_level / second_dist / second_level (any may be NULL) report the selection of every
 * query that had candidates (256 / -1 otherwise).  At most SLAMIT_SEARCH_MAX_KP keypoints per frame.  A window may hold any
 * number of them: SLAMIT_SEARCH_MAX_CAND is only the length of the stored candidate list a query's re-scan reads; a query
 * with more candidates whose tentative pair was taken by an earlier query walks the frame's keypoints again. */
#define SLAMIT_SEARCH_MAX_KP 8191
#define SLAMIT_SEARCH_MAX_CAND 1024
int slamit_guided_search(int device, const slamit_frame_view* frame, const slamit_search_queries* queries,
                         const slamit_search_rule* rule, int32_t* match_kp, int32_t* nmatches, int32_t* best_dist,
                         int32_t* best_level, int32_t* second_dist, int32_t* second_level);

/* The right-image gate of the three guided-search loops that read mvuRight.  It is one more test on a candidate
 * keypoint idx, after the window and level tests and before the descriptor distance:
 *   SLAMIT_SEARCH_ER_RADIUS  SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:93-98; q_ur = mTrackProjXR) and
 *       SearchByProjection(CurrentFrame, LastFrame, th, bMono) (:1411-1417; q_ur = u - mbf * invzc): when kp_ur[idx] > 0 the
 *       candidate is skipped if fabs(q_ur - kp_ur[idx]) > r, r being the query's own uvr[3q + 2].  A NaN passes, as there; a
 *       kp_ur of exactly 0 counts as monocular.
 *   SLAMIT_SEARCH_ER_CHI2    Fuse(pKF, vpMapPoints, th) (:918-942), with rule->chi2_gate > 0: when kp_ur[idx] >= 0 the candidate is
 *       skipped if ((u - x)^2 + (v - y)^2 + (q_ur - kp_ur[idx])^2) * inv_level_sigma2[octave] > chi2_gate_stereo (7.8); a keypoint
 *       with kp_ur < 0 keeps the two-term test against rule->chi2_gate (5.99).  A kp_ur of exactly 0 counts as stereo.
 * The relocalisation search and the three Sim3 drivers have no stereo branch in the reference: they use slamit_guided_search.
 * NOT built: the mapping side (SearchForTriangulation with stereo keypoints or bOnlyStereo, CreateNewMapPoints' stereo branch).
 * st == NULL or er_mode == SLAMIT_SEARCH_ER_NONE is slamit_guided_search.  An er_mode outside 0..2, q_ur_stride < 1, an er_mode
 * other than 0 with rule->mode == 1, or with a null kp_ur / q_ur where there is work, fails with SLAMIT_ERR_ARG and a message
 * before anything is launched or written. */
enum { SLAMIT_SEARCH_ER_NONE = 0, SLAMIT_SEARCH_ER_RADIUS = 1, SLAMIT_SEARCH_ER_CHI2 = 2 };

typedef struct slamit_search_stereo {
    int32_t er_mode;            /* SLAMIT_SEARCH_ER_* */
    float chi2_gate_stereo;     /* mode 2: 7.8 (ORBmatcher.cc:929) */
    const float* kp_ur;         /* n: mvuRight of the searched frame / keyframe */
    const float* q_ur;          /* query q at q_ur[q * q_ur_stride] */
    int32_t q_ur_stride;        /* 1, or 3 with q_ur = slamit_frustum_result.proj + 2 */
} slamit_search_stereo;

int slamit_guided_search_stereo(int device, const slamit_frame_view* frame, const slamit_search_queries* queries,
                                const slamit_search_rule* rule, const slamit_search_stereo* st, int32_t* match_kp, int32_t* nmatches,
                                int32_t* best_dist, int32_t* best_level, int32_t* second_dist, int32_t* second_level);

/* ---- Vocabulary-node search (beyond SURVEY.md §8f: the BoW drivers of ORBmatcher) ----------------------
 * The loop bodies of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (src/ORBmatcher.cc:161-290),
 * ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (:526-657) and ORBmatcher::SearchForTriangulation (:659-826):
 * features of the two sides that fall into the same vocabulary node (DBoW2::FeatureVector: slamit_voc_transform below, or the
 * reference's vendored DBoW2 on the host) are compared with DescriptorDistance.  A group = one node present on both sides:
 * its side-1 feature indices in processing order (queries) and its side-2 feature indices in scan order (candidates).
 * A feature belongs to one node, so groups are independent (checked: an index may appear once per side); one
 * wavefront walks a group's queries in order.
 *
 * mode 0 (SearchByBoW): per query best / second best with strict '<' over the candidates that are allowed (valid2)
 *   and not yet matched by an earlier query; accepted iff best <= th (th_inclusive, :243) or best < th (:601) and
 *   (float)best < nnratio * (float)second (second = 256 without one); an accepted query takes its candidate.
 * mode 1 (SearchForTriangulation; stereo keypoints through slamit_bow_search_stereo): per query the candidate of minimum distance among those with
 *   dist <= th that pass the epipole test (:737-743) and CheckDistEpipolarLine (:135-158), the LAST such candidate on
 *   ties (:731 'dist > bestDist' lets an equal one replace); candidates are never marked (the reference declares
 *   vbMatched2 but does not set it).  Float expressions are evaluated as written, without contraction.
 * The rotation-histogram filter that follows in all three drivers (mbCheckOrientation) is host logic (shim). */
typedef struct slamit_bow_groups {
    int32_t n_groups;
    const int32_t* q_ptr;      /* n_groups + 1: queries of group g are q_idx[q_ptr[g] .. q_ptr[g+1]) */
    const int32_t* q_idx;      /* side-1 feature indices */
    const int32_t* c_ptr;      /* n_groups + 1 */
    const int32_t* c_idx;      /* side-2 feature indices */
} slamit_bow_groups;

typedef struct slamit_bow_rule {
    int32_t mode;              /* 0 SearchByBoW, 1 SearchForTriangulation */
    int32_t th;                /* TH_LOW = 50 */
    int32_t th_inclusive;      /* mode 0: 1 = best <= th (KeyFrame/Frame), 0 = best < th (KeyFrame/KeyFrame) */
    float nnratio;             /* mode 0 */
    /* mode 1 only */
    float F12[9];              /* fundamental matrix, row-major */
    float ex, ey;              /* epipole of camera 1 in image 2 */
    const float* kp1_xy;       /* n1 x 2: mvKeysUn of side 1 */
    const float* kp2_xy;       /* n2 x 2 */
    const int32_t* kp2_octave; /* n2 */
    float scale_factor[16];    /* pKF2->mvScaleFactors */
    float level_sigma2[16];    /* pKF2->mvLevelSigma2 */
} slamit_bow_rule;

#define SLAMIT_BOW_MAX_GROUP 2048   /* candidates of one group */
/* valid1[i] != 0: side-1 feature i is a query (has a good MapPoint / has none yet); valid2[i] != 0: side-2 feature i
 * may be matched; either may be NULL (= all).  match12[i] = matched side-2 index or -1, dist12[i] (may be NULL) = the
 * best distance query i saw (256 if none); both have n1 entries.  *nmatches = accepted queries. */
int slamit_bow_search(int device, const uint8_t* desc1, int32_t n1, const uint8_t* valid1, const uint8_t* desc2, int32_t n2,
                      const uint8_t* valid2, const slamit_bow_groups* groups, const slamit_bow_rule* rule, int32_t* match12,
                      int32_t* dist12, int32_t* nmatches);

/* SearchForTriangulation on stereo keyframes (src/ORBmatcher.cc:695-793): bStereo = mvuRight >= 0 (0.0f counts, NaN does not).
 * The epipole test (:747-753) runs only when neither the query nor the candidate is stereo; with only_stereo a query that is not
 * stereo is skipped (:711-713: match12 = -1, dist12 = 256) and so is a candidate that is not (:734-736).  Everything else is
 * mode 1 of slamit_bow_search.  st == NULL is slamit_bow_search; a record with rule->mode == 0 (SearchByBoW has no stereo branch)
 * or with a null ur1 / ur2 where there is work to do fails with SLAMIT_ERR_ARG. */
struct slamit_bow_stereo {
    const float* ur1;          /* n1: mvuRight of side 1 */
    const float* ur2;          /* n2 */
    int32_t only_stereo;       /* bOnlyStereo */
};
typedef struct slamit_bow_stereo slamit_bow_stereo;

int slamit_bow_search_stereo(int device, const uint8_t* desc1, int32_t n1, const uint8_t* valid1, const uint8_t* desc2, int32_t n2,
                             const uint8_t* valid2, const slamit_bow_groups* groups, const slamit_bow_rule* rule,
                             const slamit_bow_stereo* st, int32_t* match12, int32_t* dist12, int32_t* nmatches);

/* ---- Vocabulary transform (Frame::ComputeBoW / KeyFrame::ComputeBoW) -----------------------------------
 * mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4) (src/Frame.cc:520-527, src/KeyFrame.cc:63-72) of the
 * reference's vendored DBoW2 (Thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1133-1201, :1225-1266): every
 * descriptor descends the vocabulary tree (per level the child of least Hamming distance, strict '<', first one wins),
 * then the frame's words become the BowVector (Thirdparty/DBoW2/src/BowVector.cpp:34-46, :62-84) and its nodes `levelsup`
 * levels above the leaves the FeatureVector (Thirdparty/DBoW2/src/FeatureVector.cpp:31-45) that slamit_bow_groups is
 * cut from.  Every id in and out is the reference's: node ids count the text file's lines from 1 (0 = root), word ids
 * count its leaves from 0.  The BowVector equals the reference's bit for bit: its fp64 sums run in the reference's order.
 *
 * A vocabulary arrives as arrays (entry i describes node i + 1) or as the text file of
 * TemplatedVocabulary::loadFromTextFile (:1345-1440).  Built: weighting TF_IDF (0) or TF (1) with scoring L1_NORM (0),
 * which is what the ORB vocabulary ("10 6 0 0") uses; anything else fails with SLAMIT_ERR_ARG, as does a parent id that
 * is not smaller than the node's own, more than SLAMIT_VOC_MAX_K children, a depth beyond SLAMIT_VOC_MAX_L, an is_leaf
 * flag that disagrees with "has no children" (the descent stops on children.empty()), or a header outside the bounds
 * of :1377.  Two departures from the reference, both where it reads something it never wrote:
 *  - an empty line (the text file's last one, which the reference's while(!f.eof()) loop at :1396 turns into a phantom
 *    child of the root) is skipped;
 *  - a leaf reached ABOVE level L - levelsup (unbalanced trees) leaves the reference's node id uninitialised (:1158,
 *    :1258); here it is the leaf's own id.  With L - levelsup <= 0 it is the root, 0, as in the reference (:1234). */
#define SLAMIT_VOC_MAX_K 20          /* children per node (:1377) */
#define SLAMIT_VOC_MAX_L 10          /* levels below the root (:1377) */
#define SLAMIT_VOC_MAX_FEATURES 8191 /* descriptors per frame (= SLAMIT_SEARCH_MAX_KP) */

typedef struct slamit_voc_desc {
    int32_t k, L;              /* the header's branching factor and depth; L - levelsup is the FeatureVector's level */
    int32_t scoring;           /* 0 = L1_NORM */
    int32_t weighting;         /* 0 = TF_IDF, 1 = TF */
    int32_t n_nodes;           /* nodes without the root; entry i of the arrays is node id i + 1 */
    const int32_t* parent;     /* n_nodes: parent node id, 0 = root */
    const uint8_t* is_leaf;    /* n_nodes */
    const uint8_t* desc;       /* n_nodes x 32: centroids */
    const double* weight;      /* n_nodes: a word's weight; <= 0 stops the word */
} slamit_voc_desc;

typedef struct slamit_voc slamit_voc;

int slamit_voc_create(const slamit_voc_desc* desc, int device, slamit_voc** out);
int slamit_voc_load_text(const char* path, int device, slamit_voc** out);
void slamit_voc_destroy(slamit_voc* v);
/* any out pointer may be NULL; n_nodes excludes the root, n_words counts the leaves */
int slamit_voc_info(const slamit_voc* v, int32_t* k, int32_t* L, int32_t* n_nodes, int32_t* n_words);

/* One frame, host pointers.  A vocabulary is shared between threads (tracking and local mapping both call ComputeBoW):
 * the handle is const here and the call keeps its state in the calling thread's scratch.
 * word_id / node_id: n entries each, word_id[i] = -1 for a stopped word (weight <= 0), which enters neither vector.
 * BowVector: *bow_n unique word ids ascending in bow_word with their normalised values in bow_value (capacity n).
 * FeatureVector as CSR: *fv_n unique node ids ascending in fv_node (capacity n), the features of node j are
 * fv_items[fv_ptr[j] .. fv_ptr[j + 1]) ascending; fv_ptr has capacity n + 1, fv_items n.  Entries past the counts are
 * not written.  (bow_n, bow_word, bow_value) and (fv_n, fv_node, fv_ptr, fv_items) may each be NULL as a whole.
 * n == 0 writes *bow_n = *fv_n = 0; n > SLAMIT_VOC_MAX_FEATURES fails with SLAMIT_ERR_CAPACITY. */
int slamit_voc_transform(const slamit_voc* v, const uint8_t* desc, int n, int levelsup, int32_t* word_id, int32_t* node_id,
                         int32_t* bow_n, int32_t* bow_word, double* bow_value, int32_t* fv_n, int32_t* fv_node,
                         int32_t* fv_ptr, int32_t* fv_items);

/* nframes frames resident in HBM as slamit_orb_extract_batch_dev writes them (frame f: d_desc + f * cap * 32, d_n[f]
 * descriptors).  Outputs are [nframes][cap] strided (d_fv_ptr [nframes][cap + 1], d_bow_n / d_fv_n [nframes]); the same
 * pairs may be NULL.  Asynchronous on `stream` (NULL: the legacy default stream of the vocabulary's device), no
 * synchronisation, no state in the handle: the scratch is the caller's workspace of slamit_voc_transform_workspace()
 * bytes.  The host cannot see d_n without waiting for the device, so a frame whose d_n[f] lies outside [0, cap] is
 * reported by the device: it writes d_bow_n[f] = d_fv_n[f] = -1 and nothing else for that frame. */
size_t slamit_voc_transform_workspace(int nframes, int cap);
int slamit_voc_transform_batch_dev(const slamit_voc* v, const uint8_t* d_desc, const int32_t* d_n, int cap, int nframes,
                                   int levelsup, int32_t* d_word_id, int32_t* d_node_id, int32_t* d_bow_n,
                                   int32_t* d_bow_word, double* d_bow_value, int32_t* d_fv_n, int32_t* d_fv_node,
                                   int32_t* d_fv_ptr, int32_t* d_fv_items, void* d_workspace, size_t workspace_bytes,
                                   void* stream);

/* ---- Keyframe database (KeyFrameDatabase, ORBVocabulary::score) -----------------------------------------
 * What KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:84-206, :208-328)
 * read from the inverted file and from L1Scoring::score (Thirdparty/DBoW2/src/ScoringObject.cpp:23-68), computed densely:
 * the handle keeps every keyframe's BowVector in HBM (the forward index, no inverted file) and one pass compares a query
 * with all of them.  Per slot that pass gives
 *   common      how many word ids the two vectors share (mnLoopWords / mnRelocWords); -1 for a dead slot
 *   first_word  the smallest shared word id, -1 if there is none
 *   seq         the slot's value of a 64-bit counter that add / add_dev advance and nothing sets back: the keyframe's
 *               position in every list of the reference's inverted file (push_back at :52-53; erase keeps the order of the
 *               rest).  The reference's walk (:94-112, :219-237) first meets the keyframes in (first_word, seq) order.
 *   score       L1Scoring::score as a double, bit for bit: from 0.0, one term fabs(vi - wi) - fabs(vi) - fabs(wi) per shared
 *               word in ascending word id (vi the query's value), left to right and uncontracted, then -sum / 2.0.
 *               Written as 0.0, and meaningless, where common < 1.
 * Everything after that (the minCommonWords filter, the covisibility sums) is host logic over the caller's graph:
 * shim/KeyFrameDatabase.h, api.KeyFrameDatabase.
 *
 * A slot holds up to max_words (<= SLAMIT_VOC_MAX_FEATURES) words; add takes the lowest free slot and fails with
 * SLAMIT_ERR_CAPACITY when there is none.  Word ids are strictly ascending (a BowVector is a std::map): the host forms check
 * that, before they look at the handle, and fail with SLAMIT_ERR_ARG; the _dev forms take what slamit_voc_transform_batch_dev
 * wrote for one frame (d_bow_n: one int) and store or read a count outside [0, max_words] / [0, cap] as an empty vector.
 * add_dev and query_batch_dev are asynchronous on `stream` and never wait for the device; the handle orders them against
 * each other and against its host forms with events of its own, so no call sees a slot half written.  A handle is used by
 * one thread at a time.  erase of a dead slot is a no-op (the reference's erase of an absent keyframe, :56-75). */
typedef struct slamit_kfdb slamit_kfdb;

int slamit_kfdb_create(int max_kf, int max_words, int device, slamit_kfdb** out);
void slamit_kfdb_destroy(slamit_kfdb* db);
int slamit_kfdb_clear(slamit_kfdb* db);
/* any out pointer may be NULL */
int slamit_kfdb_info(const slamit_kfdb* db, int32_t* max_kf, int32_t* max_words, int32_t* n_live);
int slamit_kfdb_add(slamit_kfdb* db, const int32_t* bow_word, const double* bow_value, int n, int32_t* slot);
int slamit_kfdb_add_dev(slamit_kfdb* db, const int32_t* d_bow_n, const int32_t* d_bow_word, const double* d_bow_value,
                        void* stream, int32_t* slot);
int slamit_kfdb_erase(slamit_kfdb* db, int slot);
/* One query, host pointers; common / first_word / seq / score have max_kf entries each, indexed by slot (seq may be NULL;
 * it is -1 for a dead slot).  The call's workspace lives in the calling thread's scratch. */
int slamit_kfdb_query(slamit_kfdb* db, const int32_t* bow_word, const double* bow_value, int n, int32_t* common,
                      int32_t* first_word, int64_t* seq, double* score);
/* nq queries resident in HBM as slamit_voc_transform_batch_dev writes them (query q: d_bow_word + q * cap, d_bow_n[q]
 * entries); outputs are [nq][max_kf]. */
int slamit_kfdb_query_batch_dev(slamit_kfdb* db, const int32_t* d_bow_n, const int32_t* d_bow_word, const double* d_bow_value,
                                int cap, int nq, int32_t* d_common, int32_t* d_first_word, double* d_score, void* stream);

/* ---- Frame epilogue -------------------------------------------------------
 * What Frame's constructors do right after the extractor: Frame::UndistortKeyPoints (src/Frame.cc:529-559, through
 * cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK)) and Frame::AssignFeaturesToGrid (:336-357, PosInGrid
 * :505-517), fused so that keypoints never leave the GPU between extraction and the guided search.
 * cv::undistortPoints is OpenCV's (absent from the reference tree): restated from the published cvUndistortPoints,
 * parity unpinned (oracle/orb_oracle.cc).  k1 == 0 leaves the keypoints untouched like Frame.cc:531-535. */
typedef struct slamit_camera {
    float fx, fy, cx, cy;      /* mK */
    float k1, k2, p1, p2, k3;  /* mDistCoef (k3 = 0 for a 4-coefficient model) */
} slamit_camera;

#define SLAMIT_FRAME_GRID_COLS 64   /* FRAME_GRID_COLS, include/Frame.h:41 */
#define SLAMIT_FRAME_GRID_ROWS 48   /* FRAME_GRID_ROWS, include/Frame.h:40 */
#define SLAMIT_FRAME_GRID_CELLS (SLAMIT_FRAME_GRID_COLS * SLAMIT_FRAME_GRID_ROWS)
#define SLAMIT_FRAME_MAX_KP 30000    /* one workgroup per frame keeps a short per keypoint slot in LDS: 12,320 B static + 2 B per slot,
                                       72,320 B at the ceiling; the library raises the kernel's limit itself past 48 KiB */

/* cv::undistortPoints(xy, xy, K, D, Mat(), K) on n points (what Frame::ComputeImageBounds feeds the four image
 * corners to, Frame.cc:561-590).  No k1 == 0 shortcut here: that belongs to Frame::UndistortKeyPoints. */
int slamit_undistort_points(int device, const slamit_camera* cam, const float* xy_in, int n, float* xy_out);

/* kps_un[i] = kps[i] with the undistorted pt (mvKeysUn); the grid mGrid[x][y] as CSR: the indices of cell
 * c = x * 48 + y are cell_items[cell_start[c] .. cell_start[c+1]) in keypoint (push_back) order, cell_start has
 * SLAMIT_FRAME_GRID_CELLS + 1 entries, cell_start[last] = number of keypoints inside the grid.
 * min_x/min_y/inv_w/inv_h = mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv. */
int slamit_frame_finish(int device, const slamit_camera* cam, const slamit_kp* kps, int n, float min_x, float min_y,
                        float inv_w, float inv_h, slamit_kp* kps_un, int32_t* cell_start, int32_t* cell_items);

/* Same for a batch of frames resident in HBM in the layout slamit_orb_extract_batch_dev writes (frame f: d_kps +
 * f * cap, d_n[f] keypoints); d_cell_start is [nframes][SLAMIT_FRAME_GRID_CELLS + 1], d_cell_items [nframes][cap].
 * Asynchronous on `stream`. */
int slamit_frame_finish_batch_dev(int device, const slamit_camera* cam, const slamit_kp* d_kps, const int32_t* d_n, int cap,
                                  int nframes, float min_x, float min_y, float inv_w, float inv_h, slamit_kp* d_kps_un,
                                  int32_t* d_cell_start, int32_t* d_cell_items, void* stream);

/* The same for a batch of frames whose data is resident in HBM (one wavefront walks each frame's queries, all frames
 * in parallel): keypoints in the layout slamit_frame_finish_batch_dev writes, everything else [nframes][cap] strided.
 * SLAMIT_SEARCH_BATCH_CAND candidates are stored per query (the workspace's size); windows with more are still exact: a re-scan of
 * such a query walks the frame's keypoints again (the reference has no limit, ORBmatcher.cc:85-117). */
#define SLAMIT_SEARCH_BATCH_CAND 128
typedef struct slamit_search_batch {
    int32_t nframes, kp_cap, q_cap;
    const int32_t* d_n;            /* [nframes] keypoints per frame */
    const slamit_kp* d_kps_un;     /* [nframes][kp_cap] (pt and octave are read) */
    const uint8_t* d_desc;         /* [nframes][kp_cap][32] */
    const uint8_t* d_kp_taken;     /* [nframes][kp_cap] */
    float min_x, min_y, inv_w, inv_h;
    const int32_t* d_m;            /* [nframes] queries per frame */
    const float* d_uvr;            /* [nframes][q_cap][3] */
    const int32_t* d_level_min;    /* [nframes][q_cap] */
    const int32_t* d_level_max;
    const uint8_t* d_qdesc;        /* [nframes][q_cap][32] */
    const uint8_t* d_valid;        /* [nframes][q_cap] */
    const uint8_t* d_takes;        /* [nframes][q_cap] */
} slamit_search_batch;
size_t slamit_guided_search_workspace(int nframes, int q_cap);
/* d_match_kp [nframes][q_cap], d_nmatches [nframes], d_out4 [nframes][q_cap][4] or NULL (best dist / level, second
 * dist / level).  Asynchronous on `stream`. */
int slamit_guided_search_batch_dev(int device, const slamit_search_batch* batch, const slamit_search_rule* rule,
                                   int32_t* d_match_kp, int32_t* d_nmatches, int32_t* d_out4, void* d_workspace,
                                   size_t workspace_bytes, void* stream);

/* The batch form with the right-image gate of slamit_guided_search_stereo, resident: the chain extract -> stereo match -> frustum
 * or projection -> search needs no host copy of mvuRight or mTrackProjXR.  The workspace is slamit_guided_search_workspace's.  The
 * host cannot see d_n / d_m: with er_mode != 0 a null d_q_ur (or a null d_kp_ur with kp_cap > 0) is refused whenever nframes and
 * q_cap are not zero. */
typedef struct slamit_search_stereo_dev {
    int32_t er_mode;
    float chi2_gate_stereo;
    const float* d_kp_ur;       /* [nframes][kp_cap]: what slamit_stereo_match_batch_dev writes as d_u_right when cap_left == kp_cap */
    const float* d_q_ur;        /* frame f, query q at d_q_ur[(f * q_cap + q) * q_ur_stride] */
    int32_t q_ur_stride;        /* 1 (slamit_project_batch_dev_stereo's d_ur) or 3 (slamit_frustum_batch_dev's d_proj + 2) */
} slamit_search_stereo_dev;
int slamit_guided_search_stereo_batch_dev(int device, const slamit_search_batch* batch, const slamit_search_rule* rule,
                                          const slamit_search_stereo_dev* st, int32_t* d_match_kp, int32_t* d_nmatches, int32_t* d_out4,
                                          void* d_workspace, size_t workspace_bytes, void* stream);

/* Full distance matrix (nq x nt, uint16), the batched form of DescriptorDistance. */
int slamit_hamming_matrix(const uint8_t* q, int nq, const uint8_t* t, int nt, uint16_t* out);

/* ---- Local bundle adjustment ------------------------------------------------------------ */

typedef struct slamit_ba_problem {
    int32_t n_kf;           /* local + fixed keyframes */
    int32_t n_pt;
    int32_t n_edge;
    const double* kf_pose;  /* n_kf x 12: R row-major (9) then t (3), world->camera, already widened
                               from float like Converter::toSE3Quat (src/Converter.cc:37-47) */
    const uint8_t* kf_fixed; /* n_kf: 1 = fixed vertex (KF id 0 or lFixedCameras) */
    const double* kf_intr;  /* n_kf x 4: fx fy cx cy */
    const double* pt_xyz;   /* n_pt x 3 */
    const int32_t* edge_kf; /* n_edge, in the reference's insertion order (per point, per observation) */
    const int32_t* edge_pt; /* n_edge */
    const double* edge_uv;  /* n_edge x 2 */
    const double* edge_inv_sigma2; /* n_edge */
    /* Stereo observations (EdgeStereoSE3ProjectXYZ, Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:112-141; built by
       src/Optimizer.cc:621-650).  Both NULL: every edge is monocular.  Otherwise edge_ur[e] is the keypoint's column in
       the right image (KeyFrame::mvuRight), negative for a monocular edge (the test at src/Optimizer.cc:596), and
       kf_bf[k] is keyframe k's baseline x fx (KeyFrame::mbf). */
    const double* edge_ur;  /* n_edge, nullable */
    const double* kf_bf;    /* n_kf, nullable (required when edge_ur is given) */
} slamit_ba_problem;

typedef struct slamit_ba_opts {
    int32_t its_robust;     /* 5   src/Optimizer.cc:660 */
    int32_t its_final;      /* 10  src/Optimizer.cc:707 */
    double huber_delta;     /* (double)(float)sqrt(5.991)  src/Optimizer.cc:569 */
    double chi2_gate;       /* 5.991 src/Optimizer.cc:680,723 */
    const volatile uint8_t* stop; /* nullable; polled like SparseOptimizer::terminate() */
    double huber_delta_stereo; /* (double)(float)sqrt(7.815)  src/Optimizer.cc:570; <= 0: that default */
    double chi2_gate_stereo;   /* 7.815 src/Optimizer.cc:696,740; <= 0: that default */
} slamit_ba_opts;

#define SLAMIT_BA_MAX_ITS 32

typedef struct slamit_ba_stats {
    int32_t n_its[2];                       /* LM iterations run in stage 1 / stage 2 */
    double chi2[2][SLAMIT_BA_MAX_ITS];      /* robust cost after each iteration */
    double lambda[2][SLAMIT_BA_MAX_ITS];    /* lambda after each iteration */
    int32_t trials[2][SLAMIT_BA_MAX_ITS];   /* LM trials used by each iteration */
    double chi2_init[2];                    /* cost before the first iteration of each stage */
} slamit_ba_stats;

typedef struct slamit_ba_result {
    double* kf_pose;        /* n_kf x 12 out */
    double* pt_xyz;         /* n_pt x 3 out */
    double* edge_chi2;      /* n_edge out: chi2 at the final estimate */
    uint8_t* edge_outlier;  /* n_edge out: 1 = chi2 > gate or depth <= 0 at the end (vToErase) */
    uint8_t* edge_stage1_outlier; /* n_edge out: 1 = removed after the robust stage (setLevel(1)) */
    slamit_ba_stats* stats; /* nullable */
} slamit_ba_result;

typedef struct slamit_ba slamit_ba;

/* A BA handle owns device workspaces sized for up to max_kf/max_pt/max_edge and max_batch
 * independent windows.  max_kf <= 85: the blocked LDLt of the reduced system keeps its panel
 * (rup(6 * max_kf + 1, 64) rows: 512 at 85 keyframes, 576 at 86) in LDS, and the create call
 * fails with SLAMIT_ERR_ARG when that panel does not fit.  Fixed keyframes count toward
 * max_kf, although they do not enter the reduced system. */
int slamit_ba_create(int max_kf, int max_pt, int max_edge, int max_batch, int device,
                     slamit_ba** out);

/* The same handle with the reduced system sized apart from the keyframe tables: max_kf counts free and fixed keyframes together
 * (poses, intrinsics, bf: memory only), max_free_kf (1 .. max_kf) the free ones, which alone enter the reduced system
 * (rup(6 * max_free_kf + 1, 64) rows).  Windows of up to 512 rows solve as on a slamit_ba_create handle (same plan, same kernels);
 * larger ones take a tiled LDLt through HBM.  max_free_kf > SLAMIT_BA_MAX_FREE_KF fails with SLAMIT_ERR_ARG; a window with more
 * free keyframes than max_free_kf fails its solve with SLAMIT_ERR_CAPACITY.  slamit_ba_create(k, ...) sizes like
 * slamit_ba_create_ex(k, k, ...) and keeps its own limit, k <= 85.
 *
 *   limit                      slamit_ba_create        slamit_ba_create_ex
 *   free keyframes per window  85 (with fixed ones)    max_free_kf <= 341 (reduced system <= 2048 rows)
 *   fixed keyframes            within max_kf           max_kf - free ones: memory only (~0.4 KB per keyframe and window)
 *   device bytes per window    16 Npad^2 + Npad^2 + Npad Kpad doubles and the edge / point arrays; at Npad 2048: 512 MiB
 *   (Npad = rup(6 max_free_kf + 1, 64),        of split-K partials, 32 MiB for S, and Npad x Kpad doubles of the Schur
 *    Kpad = rup(3 max_pt, 512))                operand (75 MiB per 1,000 points of max_pt) */
#define SLAMIT_BA_MAX_FREE_KF 341
int slamit_ba_create_ex(int max_kf, int max_free_kf, int max_pt, int max_edge, int max_batch, int device,
                        slamit_ba** out);
void slamit_ba_destroy(slamit_ba* h);

/* One window, host buffers, synchronous. */
int slamit_ba_solve(slamit_ba* h, const slamit_ba_problem* prob, const slamit_ba_opts* opts,
                    slamit_ba_result* res);

/* nwin independent windows solved concurrently (one workgroup cluster per window). */
int slamit_ba_solve_batch(slamit_ba* h, int nwin, const slamit_ba_problem* probs,
                          const slamit_ba_opts* opts, slamit_ba_result* results);

/* Per-phase device time of the LM trial slots -- the analogue of g2o's G2OBatchStatistics (Thirdparty/g2o/g2o/core/batch_stats.h:39-77:
 * timeLinearize + timeQuadraticForm, timeSchurComplement, timeLinearSolver, timeUpdate, timeResiduals), which the reference never
 * switches on.  After slamit_ba_profile(h, 1) every solve on the handle records HIP events at the phase boundaries of each slot
 * (an event between two kernels drains the pipeline: such a solve runs slower and is not for timed runs);
 * slamit_ba_profile_read returns the sums over the slots of the LAST profiled solve (all windows of a batch run a phase in one launch). */
#define SLAMIT_BA_PHASES 5
typedef struct slamit_ba_profile_out {
    double phase_ms[SLAMIT_BA_PHASES]; /* 0 linearise + quadratic form + damping, 1 Schur complement (product + reduction),
                                          2 reduced solve (LDLt), 3 update (back-substitution + oplus), 4 residuals + LM decision */
    int32_t slots;                     /* LM trial slots queued */
    int32_t nwin;
    double schur_exec_mflop;           /* flops (1e6) the Schur product executes per trial, summed over the windows: its tile granules,
                                          against the algorithmic count of SURVEY.md 8(d) */
} slamit_ba_profile_out;
int slamit_ba_profile(slamit_ba* h, int on);
int slamit_ba_profile_read(slamit_ba* h, slamit_ba_profile_out* out);

/* ---- Pose-only optimisation (SURVEY.md §8f "next" rank 1) ----------------------------------
 * Optimizer::PoseOptimization (src/Optimizer.cc:239-451): one SE3 pose, n unary reprojection edges
 * (g2o EdgeSE3ProjectXYZOnlyPose, Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h:143-170,cpp:266-288}),
 * four rounds of 10 Levenberg-Marquardt iterations, each restarted from the INPUT pose over the
 * current inliers; after every round an edge is an outlier iff (float)chi2 > 5.991f; the Huber
 * kernel is dropped after the third round.  Runs in one workgroup per frame, whole schedule on the
 * device.  Returns through n_inliers what the reference returns (nInitialCorrespondences - nBad;
 * 0 and an untouched pose when n < 3). */
typedef struct slamit_pose_problem {
    int32_t n;               /* correspondences (map point <-> undistorted keypoint) */
    const double* pose;      /* 12: R row-major, t — pFrame->mTcw widened like Converter::toSE3Quat */
    const double* intr;      /* 4: fx fy cx cy */
    const double* xw;        /* n x 3 world points (float positions widened) */
    const double* uv;        /* n x 2 */
    const double* inv_sigma2;/* n */
    /* Stereo correspondences (EdgeStereoSE3ProjectXYZOnlyPose, Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:174-202;
       src/Optimizer.cc:319-356): ur[i] = the keypoint's column in the right image (Frame::mvuRight), negative for a
       monocular one; bf = Frame::mbf.  ur NULL: every correspondence is monocular and bf is not read. */
    const double* ur;        /* n, nullable */
    double bf;
} slamit_pose_problem;

typedef struct slamit_pose_result {
    double* pose;            /* 12 out */
    uint8_t* outlier;        /* n out: pFrame->mvbOutlier after the last round */
    int32_t n_inliers;       /* out */
    int32_t n_its[4];        /* out: LM iterations run in each round */
    double chi2[4];          /* out: robust cost of the last evaluated trial of each round */
} slamit_pose_result;

/* One workgroup per frame keeps a flag byte per correspondence in LDS: n + 16 B beside the kernel's 1,496 B of static LDS, 67,048 B
 * at the ceiling, of the 160 KiB a gfx950 workgroup may hold (a frame has a few thousand correspondences).  A frame with more fails
 * the whole call with SLAMIT_ERR_CAPACITY before anything is launched. */
#define SLAMIT_POSE_MAX_N 65536

/* nframes independent frames in one launch (host pointers, synchronous). */
int slamit_pose_optimize_batch(int device, int nframes, const slamit_pose_problem* probs, slamit_pose_result* results);
int slamit_pose_optimize(int device, const slamit_pose_problem* prob, slamit_pose_result* res);

/* ---- Sim3 between two keyframes (beyond SURVEY.md §8f: loop closing) ---------------------------------
 * Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1247) with the g2o it instantiates: one VertexSim3Expmap
 * (Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h, sim3.h), per correspondence a fixed point in each camera frame and
 * the pair EdgeSim3ProjectXYZ (x1 = K1 proj(S12 X2)) / EdgeInverseSim3ProjectXYZ (x2 = K2 proj(S12^-1 X1)), Huber kernels
 * of width (float)sqrt(th2), NUMERIC Jacobians (g2o's central differences, delta 1e-9, core/base_binary_edge.hpp:131-200:
 * the analytic ones are commented out in the reference), Levenberg-Marquardt on the dense 7 x 7 system.  Schedule:
 * 5 iterations, drop every pair with chi2 > th2 on either edge, return 0 if fewer than 10 pairs are left, 10 more
 * iterations (5 if nothing was dropped), count the pairs with both chi2 <= th2.  One workgroup per problem. */
typedef struct slamit_sim3_problem {
    int32_t n;                   /* correspondences that pass the reference's validity tests (:1112-1136) */
    const double* p1;            /* n x 3: P3D1c = R1w P1 + t1w (float values widened) */
    const double* p2;            /* n x 3: P3D2c */
    const double* obs1;          /* n x 2: kpUn1.pt */
    const double* obs2;          /* n x 2: kpUn2.pt */
    const double* inv_sigma2_1;  /* n: pKF1->mvInvLevelSigma2[kpUn1.octave] */
    const double* inv_sigma2_2;  /* n */
    double intr1[4], intr2[4];   /* fx fy cx cy of K1, K2 */
    double r12[9], t12[3], s12;  /* g2oS12 on entry: rotation (row-major), translation, scale */
    double th2;                  /* chi2 threshold (10 in LoopClosing::ComputeSim3) */
    int32_t fix_scale;           /* bFixScale */
} slamit_sim3_problem;

typedef struct slamit_sim3_result {
    double r12[9], t12[3], s12;  /* optimised g2oS12 (the input when the function returns 0 at the 10-pair test) */
    uint8_t* inlier;             /* n out: 0 = the reference sets vpMatches1[idx] to NULL */
    int32_t n_inliers;           /* the reference's return value */
    int32_t n_its[2];            /* LM iterations run in each stage */
    double chi2[2];              /* robust cost of the last evaluated trial of each stage */
} slamit_sim3_result;

/* As for the pose: n + 16 B of flags beside 3,680 B of static LDS, 69,232 B at the ceiling; more fails with SLAMIT_ERR_CAPACITY. */
#define SLAMIT_SIM3_MAX_N 65536

int slamit_sim3_optimize_batch(int device, int nproblems, const slamit_sim3_problem* probs, slamit_sim3_result* results);
int slamit_sim3_optimize(int device, const slamit_sim3_problem* prob, slamit_sim3_result* res);

/* ---- Sim3Solver: batched RANSAC hypotheses over Horn's closed form (loop closing, between SearchByBoW and SearchBySim3) ----
 * Sim3Solver::ComputeSim3 + CheckInliers (src/Sim3Solver.cc:226-364) for n_hyp sampled triples of one candidate keyframe:
 * per hypothesis the closed-form similarity of its three correspondences (float / double exactly where the reference has
 * them), then both projections of all n correspondences and the count of those with err1 < max_err1 && err2 < max_err2.
 * One wavefront per (problem, hypothesis); a batch of candidates is one launch.  Sampling and iterate()'s acceptance scan
 * stay with the caller (shim/Sim3Solver.h, api.Sim3Solver).  The sampler of the reference can repeat an index inside a
 * triple (:166-177): that is legal input and yields some count in [0, n].  An index outside [0, n), n above
 * SLAMIT_SIM3_RANSAC_MAX_N or n_hyp above SLAMIT_SIM3_RANSAC_MAX_HYP fails with SLAMIT_ERR_ARG and a message; n == 0 or
 * n_hyp == 0 is allowed and writes nothing. */
#define SLAMIT_SIM3_RANSAC_MAX_N 8192      /* correspondences per problem (a keyframe holds a few thousand keypoints at most) */
#define SLAMIT_SIM3_RANSAC_MAX_HYP 1024    /* hypotheses per problem (LoopClosing asks for 300) */

typedef struct slamit_sim3_ransac_problem {
    int32_t n;                 /* correspondences kept by the Sim3Solver constructor (:62-103) */
    const float* x1;           /* n x 3: mvX3Dc1 (Rcw1*X+tcw1, float) */
    const float* x2;           /* n x 3: mvX3Dc2 */
    const float* max_err1;     /* n: (float)(size_t)(9.210*sigma2): mvnMaxError1 is a vector<size_t>, the bound is truncated */
    const float* max_err2;     /* n */
    float intr1[4], intr2[4];  /* fx fy cx cy of mK1, mK2 */
    int32_t fix_scale;
    int32_t n_hyp;             /* hypotheses to evaluate */
    const int32_t* triples;    /* n_hyp x 3 indices into the n correspondences */
} slamit_sim3_ransac_problem;

typedef struct slamit_sim3_ransac_result {
    float* t12;                /* n_hyp x 13: R12 row-major (9), t12 (3), s12 */
    int32_t* n_inliers;        /* n_hyp: mnInliersi of each hypothesis */
    uint32_t* inlier_bits;     /* n_hyp x ((n+31)/32), nullable: bit i = mvbInliersi[i] */
} slamit_sim3_ransac_result;

/* nproblems candidates in one launch (host pointers, synchronous). */
int slamit_sim3_ransac_batch(int device, int nproblems, const slamit_sim3_ransac_problem* probs, slamit_sim3_ransac_result* results);
int slamit_sim3_ransac(int device, const slamit_sim3_ransac_problem* prob, slamit_sim3_ransac_result* res);

/* ---- PnPsolver: batched EPnP RANSAC (relocalisation, between SearchByBoW and PoseOptimization) ----
 * PnPsolver::compute_pose + CheckInliers (src/PnPsolver.cc:316-347, :383-958) for n_hyp sampled quadruples of one candidate
 * keyframe: per hypothesis the EPnP pose of its four correspondences in double, then the reprojection of all n correspondences
 * (float / double exactly where the reference has them) and the count of those with error2 < max_err.  One wavefront per
 * (problem, hypothesis); a batch of candidates is one launch.  slamit_pnp_refine_batch is Refine() (:268-313): the EPnP pose of
 * a subset given as a bit mask (a hypothesis' inlier_bits), then CheckInliers over all n; one workgroup per problem.  Sampling,
 * SetRansacParameters and iterate()'s scan stay with the caller (shim/PnPsolver.h, api.PnPsolver).
 * The reference's pose depends on which basis cvSVD returns for the four-dimensional null space of a four-point set and on the
 * sign of its PCA axes; both are pinned here (csrc/epnp.h).  Every decomposition runs a fixed number of
 * sweeps: the reference's sampler can repeat an index inside a quadruple (:196-209), which is legal input and yields a pose that
 * need not be finite and some count in [0, n].  A subset of four takes the four-point path, one of five is accepted and
 * unspecified, one of fewer than four fails with SLAMIT_ERR_ARG.  An index outside [0, n), n above SLAMIT_PNP_MAX_N, n_hyp above
 * SLAMIT_PNP_MAX_HYP or a null array with n > 0 fails with SLAMIT_ERR_ARG and a message before anything is launched; n == 0 or
 * n_hyp == 0 is allowed and writes nothing.  (The four structs are declared tag first, typedef after, like the stereo record above.) */
#define SLAMIT_PNP_MAX_N 8192       /* correspondences per problem */
#define SLAMIT_PNP_MAX_HYP 1024     /* hypotheses per problem (Tracking::Relocalization asks for 300 at most) */

struct slamit_pnp_problem {
    int32_t n;                 /* correspondences the PnPsolver constructor keeps (:87-109) */
    const float* p3d;          /* n x 3: mvP3Dw */
    const float* p2d;          /* n x 2: mvP2D (kpUn.pt) */
    const float* max_err;      /* n: (float)(mvSigma2[i] * th2) */
    double intr[4];            /* fu fv uc vc: doubles holding F.fx, F.fy, F.cx, F.cy */
    int32_t n_hyp;             /* hypotheses to evaluate */
    const int32_t* quads;      /* n_hyp x 4 indices into the n correspondences */
};
typedef struct slamit_pnp_problem slamit_pnp_problem;

struct slamit_pnp_result {
    double* pose;              /* n_hyp x 12: mRi row-major (9), mti (3) */
    int32_t* n_inliers;        /* n_hyp: mnInliersi of each hypothesis */
    uint32_t* inlier_bits;     /* n_hyp x ((n+31)/32), nullable: bit i = mvbInliersi[i] */
};
typedef struct slamit_pnp_result slamit_pnp_result;

struct slamit_pnp_refine_problem {
    int32_t n;
    const float* p3d;          /* as in slamit_pnp_problem */
    const float* p2d;
    const float* max_err;
    double intr[4];
    const uint32_t* subset_bits;   /* (n+31)/32 words: bit i = correspondence i takes part (mvbBestInliers); bits past n are ignored */
};
typedef struct slamit_pnp_refine_problem slamit_pnp_refine_problem;

struct slamit_pnp_refine_result {
    double pose[12];           /* out: mRi row-major, mti */
    int32_t n_inliers;         /* out: mnRefinedInliers */
    uint32_t* inlier_bits;     /* (n+31)/32 words, nullable: mvbRefinedInliers */
};
typedef struct slamit_pnp_refine_result slamit_pnp_refine_result;

/* nproblems candidates in one launch (host pointers, synchronous). */
int slamit_pnp_ransac_batch(int device, int nproblems, const slamit_pnp_problem* probs, slamit_pnp_result* results);
int slamit_pnp_ransac(int device, const slamit_pnp_problem* prob, slamit_pnp_result* res);
int slamit_pnp_refine_batch(int device, int nproblems, const slamit_pnp_refine_problem* probs, slamit_pnp_refine_result* results);

/* ---- Initializer: batched H / F RANSAC and the motion check (monocular initialisation, after SearchForInitialization) ----
 * slamit_init_hyp_batch is the body of FindHomography and FindFundamental (src/Initializer.cc:133-232) for n_hyp eight-match sets of
 * one frame pair: per set ComputeH21 and ComputeF21 on the normalised pairs, H21i = T2inv Hn T1 and F21i = T2t Fn T1, then
 * CheckHomography / CheckFundamental over all n matches; the score is the reference's float sum in match order, bit for bit.  One
 * wavefront per (problem, hypothesis, model); a batch of frame pairs is one launch.  Normalize runs on the host over ALL keypoints
 * of each frame.  slamit_init_reconstruct_batch is ReconstructH up to its eight motions or ReconstructF's four (:479-741) with
 * CheckRT (:807-916) for each over the matches of subset_bits (the kept hypothesis' inlier_bits); one workgroup per (problem,
 * motion).  Sampling and the scans stay with the caller (shim/Initializer.h, api.Initializer); the scans are the five small
 * functions below.  cv::SVDecomp is unpinned: every decomposition is a Jacobi in double with a fixed number of sweeps, its
 * singular vectors carry sign rule (a) and are rounded to float once (csrc/two_view.h).
 * n < 8, an index outside its table, a set that repeats an index, n above SLAMIT_INIT_MAX_N, n_hyp above SLAMIT_INIT_MAX_HYP or a
 * null array fails with SLAMIT_ERR_ARG and a message before anything is launched; nproblems == 0 or n_hyp == 0 writes nothing. */
#define SLAMIT_INIT_MAX_N 8192      /* matches per problem */
#define SLAMIT_INIT_MAX_HYP 1024    /* hypotheses per problem (Tracking asks for 200) */
#define SLAMIT_INIT_H 0
#define SLAMIT_INIT_F 1

struct slamit_init_problem {
    int32_t n1;                /* keypoints of the reference frame */
    const float* keys1;        /* n1 x 2: mvKeysUn[i].pt of frame 1 */
    int32_t n2;
    const float* keys2;        /* n2 x 2: frame 2 */
    int32_t n;                 /* matches: mvMatches12 */
    const int32_t* matches;    /* n x 2: index into keys1, index into keys2 */
    float sigma;               /* mSigma */
    int32_t n_hyp;             /* sets to evaluate */
    const int32_t* sets;       /* n_hyp x 8 indices into the n matches, distinct inside a set */
};
typedef struct slamit_init_problem slamit_init_problem;

struct slamit_init_result {    /* every array holds the n_hyp entries of the homographies first, then those of the fundamentals */
    float* model;              /* 2 x n_hyp x 9: H21i, F21i row-major */
    float* score;              /* 2 x n_hyp: currentScore */
    int32_t* n_inliers;        /* 2 x n_hyp: members of vbCurrentInliers */
    uint32_t* inlier_bits;     /* 2 x n_hyp x ((n+31)/32), nullable: bit i = vbCurrentInliers[i] */
};
typedef struct slamit_init_result slamit_init_result;

struct slamit_init_reconstruct_problem {
    int32_t n1;
    const float* keys1;        /* as in slamit_init_problem */
    int32_t n2;
    const float* keys2;
    int32_t n;
    const int32_t* matches;
    float sigma;
    int32_t kind;              /* SLAMIT_INIT_H or SLAMIT_INIT_F */
    float model[9];            /* the kept H21 or F21 */
    float K[9];                /* mK row-major */
    const uint32_t* subset_bits;   /* (n+31)/32 words: bit i = vbMatchesInliers[i]; bits past n are ignored */
};
typedef struct slamit_init_reconstruct_problem slamit_init_reconstruct_problem;

struct slamit_init_reconstruct_result {
    int32_t decomposable;      /* out: 0 = ReconstructH's d1/d2, d2/d3 early return (no motion was checked); 1 otherwise */
    int32_t n_motions;         /* out: 8 for H, 4 for F; only that many entries of the arrays below are written */
    float R[72];               /* out: n_motions x 9 */
    float t[24];               /* out: n_motions x 3 */
    int32_t n_good[8];         /* out: CheckRT's return value */
    float cos_sel[8];          /* out: the min(50, n_good - 1)-th smallest accepted cosParallax; 1 when n_good is 0 */
    uint8_t* status;           /* n_motions x n, nullable: 0 counted in n_good, 1 outside the subset, 2 point not finite, 3 / 4 depth in
                                  camera 1 / 2, 5 / 6 reprojection in image 1 / 2 */
    float* points;             /* n_motions x n x 3, nullable: p3dC1 of match i (zero for status 1 and 2) */
    uint32_t* good_bits;       /* n_motions x ((n+31)/32), nullable: bit i = vbGood of match i's keypoint */
};
typedef struct slamit_init_reconstruct_result slamit_init_reconstruct_result;

/* nproblems frame pairs in one launch each (host pointers, synchronous). */
int slamit_init_hyp_batch(int device, int nproblems, const slamit_init_problem* probs, slamit_init_result* results);
int slamit_init_hyp(int device, const slamit_init_problem* prob, slamit_init_result* res);
int slamit_init_reconstruct_batch(int device, int nproblems, const slamit_init_reconstruct_problem* probs, slamit_init_reconstruct_result* results);
int slamit_init_reconstruct(int device, const slamit_init_reconstruct_problem* prob, slamit_init_reconstruct_result* res);
/* The host scans.  best_hypothesis: the first strict maximum of the scores above 0 (-1: none).  choose_h: SH / (SH + SF) > 0.40.
 * parallax_deg: acos(cos_sel) * 180 / pi, 0 when n_good is 0.  pick_f / pick_h: the winning motion of ReconstructF's nsimilar /
 * nMinGood / maxGood cascade and of ReconstructH's best / second-best rule, -1 when the initialisation is rejected. */
int slamit_init_best_hypothesis(int n_hyp, const float* score);
int slamit_init_choose_h(float SH, float SF);
float slamit_init_parallax_deg(int n_good, float cos_sel);
int slamit_init_pick_f(const int32_t* n_good, const float* parallax, int n_inliers, float min_parallax, int min_triangulated);
int slamit_init_pick_h(const int32_t* n_good, const float* parallax, int n_inliers, float min_parallax, int min_triangulated);

/* ---- CreateNewMapPoints: batched two-view triangulation (local mapping, between SearchForTriangulation and the new map point) ----
 * The per-pair body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:348-483), monocular: parallax of the two rays, the
 * 4x4 linear triangulation (smallest right singular vector, one-sided Jacobi in float), both depth tests, both reprojection
 * gates (5.991 sigma2) and the scale-consistency test; float / double exactly where the reference has them (csrc/triangulate.h).
 * One problem is one (current keyframe, neighbour) pair with its n matched keypoints; one lane per pair, a batch is one launch.
 * status[i] is the first gate that rejected pair i, in the reference's order:
 *   0 accepted   1 parallax   2 w == 0   3 z1 <= 0   4 z2 <= 0   5 reprojection in keyframe 1   6 reprojection in keyframe 2
 *   7 dist1 == 0 or dist2 == 0   8 scale consistency
 * x3d[3i..] is the point of pair i (zero for codes 1 and 2, which have none).  Stereo keypoints go through
 * slamit_triangulate_stereo* below: there is no right-image coordinate in this problem.  n above SLAMIT_TRIANGULATE_MAX_N, n_levels outside [1, SLAMIT_MAX_LEVELS], an octave
 * outside [0, n_levels) or a null array with n > 0 fails with SLAMIT_ERR_ARG and a message before anything is launched;
 * n == 0 and nproblems == 0 are valid and write nothing but n_accepted = 0. */
#define SLAMIT_TRIANGULATE_MAX_N 8192      /* pairs per problem (the keypoints of a frame) */

typedef struct slamit_triangulate_problem {
    float Tcw1[12], Tcw2[12];      /* row-major 3x4 poses of the current keyframe and of the neighbour */
    float intr1[6], intr2[6];      /* fx fy cx cy invfx invfy of each keyframe */
    int32_t n;                     /* matched pairs */
    int32_t n_levels;              /* entries of the four tables */
    const float* kp1_xy;           /* n x 2: mvKeysUn[idx1].pt, gathered by the match indices */
    const float* kp2_xy;           /* n x 2 */
    const int32_t* octave1;        /* n: mvKeysUn[idx1].octave */
    const int32_t* octave2;        /* n */
    const float* scale_factors1;   /* n_levels: mvScaleFactors of the current keyframe */
    const float* level_sigma2_1;   /* n_levels: mvLevelSigma2 */
    const float* scale_factors2;   /* n_levels: the neighbour's */
    const float* level_sigma2_2;   /* n_levels */
    float ratio_factor;            /* 1.5f * mfScaleFactor (:260) */
} slamit_triangulate_problem;

typedef struct slamit_triangulate_result {
    uint8_t* status;               /* n out */
    float* x3d;                    /* n x 3 out */
    int32_t n_accepted;            /* out: pairs with status 0 */
} slamit_triangulate_result;

/* nproblems keyframe pairs in one launch (host pointers, synchronous). */
int slamit_triangulate_batch(int device, int nproblems, const slamit_triangulate_problem* probs, slamit_triangulate_result* results);
int slamit_triangulate(int device, const slamit_triangulate_problem* prob, slamit_triangulate_result* res);

/* Stereo keypoints in CreateNewMapPoints (src/LocalMapping.cc:335-465, src/KeyFrame.cc:623-639).  A pair whose keypoint in either
 * keyframe has mvuRight >= 0 (0.0f counts, NaN does not) takes the reference's stereo branches: the stereo cosine
 * cos(2 atan2(mb / 2, mvDepth)) of keyframe 1, ELSE of keyframe 2, beside the parallax of the rays; triangulation without the
 * 0.9998 gate; otherwise KeyFrame::UnprojectStereo of the keyframe with the smaller stereo cosine, from the RAW keypoint mvKeys;
 * the three-term reprojection gate 7.8 sigma2 with u_r = u - bf / z, bf being the CURRENT keyframe's mbf for both keyframes (:458).
 * Codes 0..8 keep their meaning; 9 = the keypoint chosen for UnprojectStereo has depth <= 0 (the reference would read an empty
 * matrix; Frame::ComputeStereoMatches never produces it), x3d zero.  source[i]: 0 no point (codes 1, 2, 9), 1 triangulated,
 * 2 UnprojectStereo of keyframe 1, 3 of keyframe 2.  The record's tag is also the name of the single-problem entry point, so the
 * type is written with its struct keyword or as slamit_triangulate_stereo_rec. */
struct slamit_triangulate_stereo {
    const float* ur1;              /* n: mvuRight[idx1] of the current keyframe */
    const float* ur2;              /* n: mvuRight[idx2] of the neighbour */
    const float* depth1;           /* n: mvDepth[idx1] */
    const float* depth2;           /* n */
    const float* raw1_xy;          /* n x 2: mvKeys[idx1].pt, the distorted keypoint */
    const float* raw2_xy;          /* n x 2 */
    float mb1, mb2;                /* mb of the current keyframe and of the neighbour */
    float bf;                      /* mbf of the current keyframe */
};
typedef struct slamit_triangulate_stereo slamit_triangulate_stereo_rec;

/* stereo (may be NULL) has nproblems entries; a NULL entry makes that problem monocular: it computes exactly what
 * slamit_triangulate_batch computes.  source (may be NULL) has nproblems entries, each NULL or n bytes out.  A null per-pair
 * array in a present record with n > 0 fails with SLAMIT_ERR_ARG before anything is launched. */
int slamit_triangulate_stereo_batch(int device, int nproblems, const slamit_triangulate_problem* probs,
                                    const struct slamit_triangulate_stereo* const* stereo, slamit_triangulate_result* results,
                                    uint8_t* const* source);
int slamit_triangulate_stereo(int device, const slamit_triangulate_problem* prob, const struct slamit_triangulate_stereo* stereo,
                              slamit_triangulate_result* res, uint8_t* source);

/* ---- SearchLocalPoints: the frustum test that feeds the guided search (tracking, between UpdateLocalMap and SearchByProjection) ----
 * Frame::isInFrustum with MapPoint::PredictScale (src/Frame.cc:389-445, src/MapPoint.cc:391-400) for every local map point of
 * Tracking::SearchLocalPoints (src/Tracking.cc:1409-1464), and the query ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th)
 * builds from what isInFrustum stored (src/ORBmatcher.cc:47-71): float / double exactly where the reference has them
 * (csrc/frustum.h, which also says which log PredictScale calls and carries its own).  One lane per point; a batch is one launch.
 * status[i] is the first test that rejected point i, in the reference's order:
 *   0 in view   1 skipped by the caller (skip[i] != 0: bad, or already seen this frame)   2 depth (PcZ < 0)   3 u outside
 *   4 v outside   5 distance (outside [0.8 min_dist, 1.2 max_dist])   6 viewing angle   7 level outside the table
 * ONE DEPARTURE: this reference's PredictScale does not clamp, and a level outside [0, n_levels) then indexes mvScaleFactors out of
 * bounds.  Here such a point, and one whose max_dist / dist is not finite and positive (level = INT32_MIN), is status 7: it keeps
 * its projection, viewing cosine and raw level, produces no query and is not counted in view.
 * proj[3i..] = mTrackProjX, mTrackProjY, mTrackProjXR; view_cos[i] = mTrackViewCos; level[i] = mnTrackScaleLevel; fields the walk
 * did not reach are zero (csrc/frustum.h lists which).  The query arrays are slamit_search_queries' own: uvr[3i..] = (u, v,
 * r * scale_factors[level]) with r = (view_cos > 0.998 ? 2.5 : 4.0) * (th != 1 ? th : 1), level_min = level - 1, level_max = level,
 * valid = 1 for status 0; zeros and valid = 0 otherwise.  Queries are NOT compacted: query i is point i, so the order of the
 * reference's walk over mvpLocalMapPoints is kept, and a valid = 0 query matches nothing and takes no keypoint.
 * proj[3i + 2] is mTrackProjXR = u - bf * invz (src/Frame.cc:439): slamit_guided_search_stereo reads it in place as q_ur = proj + 2 with
 * q_ur_stride 3 (device form: d_proj + 2), mode SLAMIT_SEARCH_ER_RADIUS; with bf = 0 it equals u and nothing reads it.  n above SLAMIT_FRUSTUM_MAX_N, n_levels outside [1, SLAMIT_MAX_LEVELS] or
 * a null array with n > 0 fails with SLAMIT_ERR_ARG and a message before anything is launched; n == 0 and nproblems == 0 are
 * valid and write nothing but n_in_view = 0. */
#define SLAMIT_FRUSTUM_MAX_N 65536         /* points per problem / q_cap of the device form (a local map holds a few thousand) */

typedef struct slamit_frustum_frame {
    float Rcw[9], tcw[3], Ow[3];   /* mRcw (row-major), mtcw, mOw: the camera centre AS THE FRAME HOLDS IT */
    float fx, fy, cx, cy, bf;      /* bf = mbf; 0 for a monocular frame */
    float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY */
    float view_cos_limit;          /* 0.5 (Tracking.cc:1440) */
    float log_scale_factor;        /* mfLogScaleFactor */
    float th;                      /* SearchByProjection's th: 1, 3 (RGBD) or 5 (after relocalisation) */
    int32_t n_levels;              /* entries of scale_factors in use */
    float scale_factors[SLAMIT_MAX_LEVELS]; /* mvScaleFactors */
} slamit_frustum_frame;

typedef struct slamit_frustum_problem {
    slamit_frustum_frame frame;
    int32_t n;                     /* local map points */
    const float* pos;              /* n x 3: GetWorldPos() */
    const float* normal;           /* n x 3: GetNormal() */
    const float* max_dist;         /* n: the RAW mfMaxDistance (GetMaxDistanceInvariance() / 1.2f) */
    const float* min_dist;         /* n: the raw mfMinDistance */
    const uint8_t* skip;           /* n: 1 = mnLastFrameSeen == the frame's id, or isBad() */
} slamit_frustum_problem;

typedef struct slamit_frustum_result {
    uint8_t* status;               /* n out */
    float* proj;                   /* n x 3 out: u, v, uR */
    float* view_cos;               /* n out */
    int32_t* level;                /* n out */
    float* uvr;                    /* n x 3 out: slamit_search_queries.uvr */
    int32_t* level_min;            /* n out */
    int32_t* level_max;            /* n out */
    uint8_t* valid;                /* n out */
    int32_t n_in_view;             /* out: points with status 0 (nToMatch) */
} slamit_frustum_result;

/* nproblems frames in one launch (host pointers, synchronous). */
int slamit_frustum_batch(int device, int nproblems, const slamit_frustum_problem* probs, slamit_frustum_result* results);
int slamit_frustum(int device, const slamit_frustum_problem* prob, slamit_frustum_result* res);

/* Everything resident in HBM: nframes frames, frame f with d_m[f] points (clamped to [0, q_cap]; entries past it are neither read
 * nor written).  The point arrays are PLANES, so that a wavefront's loads are contiguous: coordinate c of point i of frame f is
 * d_pos[(f * 3 + c) * q_cap + i].  d_uvr, d_level_min, d_level_max and d_valid are the arrays slamit_search_batch reads, in its
 * layout; the five optional outputs may be NULL.  The host cannot see d_frames: the device accepts a level only below
 * min(n_levels, SLAMIT_MAX_LEVELS), so an n_levels <= 0 makes every point that reaches the level test status 7.  Asynchronous on `stream` (NULL: the legacy
 * default stream of `device`), no synchronisation, no state; d_n_in_view is summed by a second launch of one wavefront per
 * frame over d_valid, on the same stream. */
typedef struct slamit_frustum_batch_rec {
    int32_t nframes, q_cap;
    const slamit_frustum_frame* d_frames; /* [nframes] */
    const int32_t* d_m;            /* [nframes] points per frame */
    const float* d_pos;            /* [nframes][3][q_cap] */
    const float* d_normal;         /* [nframes][3][q_cap] */
    const float* d_max_dist;       /* [nframes][q_cap] */
    const float* d_min_dist;       /* [nframes][q_cap] */
    const uint8_t* d_skip;         /* [nframes][q_cap] */
    float* d_uvr;                  /* [nframes][q_cap][3] out */
    int32_t* d_level_min;          /* [nframes][q_cap] out */
    int32_t* d_level_max;          /* [nframes][q_cap] out */
    uint8_t* d_valid;              /* [nframes][q_cap] out */
    uint8_t* d_status;             /* [nframes][q_cap] out, nullable */
    float* d_proj;                 /* [nframes][q_cap][3] out, nullable */
    float* d_view_cos;             /* [nframes][q_cap] out, nullable */
    int32_t* d_level;              /* [nframes][q_cap] out, nullable */
    int32_t* d_n_in_view;          /* [nframes] out, nullable */
} slamit_frustum_batch_rec;
int slamit_frustum_batch_dev(int device, const slamit_frustum_batch_rec* batch, void* stream);

/* ---- The projections in front of the guided search: the other six ORBmatcher drivers ----
 * World -> camera, the depth, bounds, distance and viewing-angle gates, MapPoint::PredictScale and the window radius of
 *   form 0 LAST_FRAME  SearchByProjection(CurrentFrame, LastFrame, th, bMono)   src/ORBmatcher.cc:1332-1474
 *        1 RELOC       SearchByProjection(CurrentFrame, pKF, sAlreadyFound, ..) :1476-1603
 *        2 FUSE        Fuse(pKF, vpMapPoints, th)                               :829-979
 *        3 SIM3_PROJ   SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)    :293-407
 *        4 SIM3_FUSE   Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)             :981-1100
 *        5 SIM3_PAIR   SearchBySim3, one direction                              :1102-1330
 * float / double exactly where the loops of shim/ORBmatcher.h have them (csrc/project.h restates them and lists every split).  One
 * lane per point, a batch of cameras per launch; the problems of a batch may differ in form.  status[i] is the first test that
 * rejected point i:  0 accepted  1 skipped by the caller  2 depth  3 u outside  4 v outside  5 distance  6 viewing angle
 * 7 level outside the table (the departure of slamit_frustum: no query, level = INT32_MIN, whether the level was predicted or
 * given as an octave).  proj[2i..] = u, v; level[i]; fields the walk did not reach are zero.  The query arrays are
 * slamit_search_queries' own, NOT compacted: query i is point i, valid = 1 for status 0, zeros otherwise.
 * The camera record is computed on the host, once per camera, as the shim computes it.  The records carry no mbf: the right-image
 * column ur = u - bf * invz of the two forms whose search reads one (0 LAST_FRAME, :1413; 2 FUSE, :874) is the extra output of
 * slamit_project_batch_stereo / slamit_project_batch_dev_stereo below.
 * Arrays a form does not read may be NULL in the host form: normal is read by forms 2, 3, 4; max_dist / min_dist by all but form
 * 0; octave by form 0 only.  n above SLAMIT_PROJECT_MAX_N, an unknown form or direction, n_levels outside [1, SLAMIT_MAX_LEVELS]
 * or a missing array with n > 0 fails with SLAMIT_ERR_ARG and a message before anything is launched; n == 0 and nproblems == 0
 * are valid and write nothing but n_valid = 0. */
#define SLAMIT_PROJECT_MAX_N 65536
enum { SLAMIT_PROJECT_LAST_FRAME = 0, SLAMIT_PROJECT_RELOC = 1, SLAMIT_PROJECT_FUSE = 2, SLAMIT_PROJECT_SIM3_PROJ = 3,
       SLAMIT_PROJECT_SIM3_FUSE = 4, SLAMIT_PROJECT_SIM3_PAIR = 5 };

typedef struct slamit_project_camera {
    int32_t form;                  /* SLAMIT_PROJECT_* */
    float R[9], t[3], O[3];        /* world -> camera, row-major, and the camera centre; form 5: the pose of the keyframe the points come from */
    float R2[9], t2[3];            /* form 5: the similarity into the searched camera (sR21, t21 or sR12, t12) */
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY */
    float log_scale_factor;        /* mfLogScaleFactor */
    float th;                      /* the driver's th: the radius is th * scale_factors[level] */
    int32_t n_levels;
    float scale_factors[SLAMIT_MAX_LEVELS];
    int32_t direction;             /* form 0: 0 = levels l-1..l+1, 1 (forward) = l.., 2 (backward) = 0..l */
} slamit_project_camera;

typedef struct slamit_project_problem {
    slamit_project_camera camera;
    int32_t n;
    const float* pos;              /* n x 3: GetWorldPos() */
    const float* normal;           /* n x 3: GetNormal() */
    const float* max_dist;         /* n: the RAW mfMaxDistance */
    const float* min_dist;         /* n: the raw mfMinDistance */
    const int32_t* octave;         /* n: LastFrame.mvKeys[i].octave */
    const uint8_t* skip;           /* n: 1 = the driver's own `continue` before the projection (null, bad, outlier, already found) */
} slamit_project_problem;

typedef struct slamit_project_result {
    uint8_t* status;               /* n out */
    float* proj;                   /* n x 2 out: u, v */
    int32_t* level;                /* n out */
    float* uvr;                    /* n x 3 out: slamit_search_queries.uvr */
    int32_t* level_min;            /* n out */
    int32_t* level_max;            /* n out */
    uint8_t* valid;                /* n out */
    int32_t n_valid;               /* out: points with status 0 */
} slamit_project_result;

/* nproblems cameras in one launch (host pointers, synchronous). */
int slamit_project_batch(int device, int nproblems, const slamit_project_problem* probs, slamit_project_result* results);
int slamit_project(int device, const slamit_project_problem* prob, slamit_project_result* res);

/* Everything resident in HBM, in slamit_frustum_batch_dev's conventions: frame f has d_m[f] points (clamped to [0, q_cap]; entries
 * past it are neither read nor written), the point arrays are PLANES [nframes][3][q_cap], the four query arrays are the ones
 * slamit_search_batch reads.  The host cannot see d_cameras: all six input arrays must be present whatever the forms, a level is
 * accepted only below min(n_levels, SLAMIT_MAX_LEVELS), and a form outside 0..5 makes every point of that frame status 1.
 * Asynchronous on `stream`, no synchronisation, no state. */
typedef struct slamit_project_batch_rec {
    int32_t nframes, q_cap;
    const slamit_project_camera* d_cameras; /* [nframes] */
    const int32_t* d_m;            /* [nframes] points per frame */
    const float* d_pos;            /* [nframes][3][q_cap] */
    const float* d_normal;         /* [nframes][3][q_cap] */
    const float* d_max_dist;       /* [nframes][q_cap] */
    const float* d_min_dist;       /* [nframes][q_cap] */
    const int32_t* d_octave;       /* [nframes][q_cap] */
    const uint8_t* d_skip;         /* [nframes][q_cap] */
    float* d_uvr;                  /* [nframes][q_cap][3] out */
    int32_t* d_level_min;          /* [nframes][q_cap] out */
    int32_t* d_level_max;          /* [nframes][q_cap] out */
    uint8_t* d_valid;              /* [nframes][q_cap] out */
    uint8_t* d_status;             /* [nframes][q_cap] out, nullable */
    float* d_proj;                 /* [nframes][q_cap][2] out, nullable */
    int32_t* d_level;              /* [nframes][q_cap] out, nullable */
    int32_t* d_n_valid;            /* [nframes] out, nullable */
} slamit_project_batch_rec;
int slamit_project_batch_dev(int device, const slamit_project_batch_rec* batch, void* stream);

/* The same two calls with the right-image column of every accepted point as one more output, for slamit_guided_search_stereo's
 * q_ur (stride 1): ur[i] = u - bf * invz, two roundings, with the invz the point's form already has -- (float)(1.0 / (double)zc) for
 * form 0 (src/ORBmatcher.cc:1369, :1413), 1.0f / zc for form 2 (:860, :874).  It is written for every point of status 0 and is zero
 * otherwise.  ONLY FORMS 0 AND 2 HAVE A READER of ur in the reference; for the other forms the same expression is written and
 * means nothing.  bf[f] is problem f's mbf (device form: d_bf[f], frame f's); ur[f] points at problem f's n floats (device form:
 * d_ur is [nframes][q_cap]).  bf and ur both NULL is slamit_project_batch / slamit_project_batch_dev; exactly one of them NULL
 * fails with SLAMIT_ERR_ARG, as does a NULL ur[f] for a problem with n > 0.  Every other output is that of the plain call. */
int slamit_project_batch_stereo(int device, int nproblems, const slamit_project_problem* probs, slamit_project_result* results,
                                const float* bf, float* const* ur);
int slamit_project_batch_dev_stereo(int device, const slamit_project_batch_rec* batch, const float* d_bf, float* d_ur, void* stream);

/* The rotation-consistency check of the searches that follow a projection (src/ORBmatcher.cc:1430-1471, ComputeThreeMaxima
 * :1605-1646) on what slamit_guided_search_batch_dev left in HBM, one wavefront per frame.  The queries of frame f are walked in
 * order; a query q matched to keypoint k = d_match_kp[f][q] makes d_kp_query[f][k] = q (a later query overwrites an earlier one:
 * that happens when the earlier point had takes = 0) and enters the histogram: rot = d_qangle[f][q] - d_kps_un[f][k].angle,
 * + 360 when negative, bin = (int)roundf(rot * (1.0f / 30)), 30 -> 0, an entry outside [0, 30) is dropped.  Then every entry of a
 * bin that is not one of the three maxima (the first bin on ties; the second and third fall when below 10 % of the first, in
 * float) sets d_kp_query[f][k] = -1 and takes 1 from d_nmatches[f], once per ENTRY as the reference does.
 * d_kp_query [nframes][kp_cap] out: the query that owns keypoint k (CurrentFrame.mvpMapPoints[k]) or -1; d_nmatches [nframes] in /
 * out; d_bins [nframes][3] out: the three maxima, -1 for none.  A match outside [0, min(d_n[f], kp_cap)) is ignored.
 * Asynchronous on `stream`, no synchronisation, no state; the result does not depend on scheduling. */
typedef struct slamit_rotation_batch {
    int32_t nframes, kp_cap, q_cap;
    const int32_t* d_n;            /* [nframes] keypoints per frame */
    const slamit_kp* d_kps_un;     /* [nframes][kp_cap] (angle is read) */
    const int32_t* d_m;            /* [nframes] queries per frame */
    const int32_t* d_match_kp;     /* [nframes][q_cap] */
    const float* d_qangle;         /* [nframes][q_cap]: LastFrame.mvKeysUn[q].angle */
    int32_t* d_kp_query;           /* [nframes][kp_cap] out */
    int32_t* d_nmatches;           /* [nframes] in / out */
    int32_t* d_bins;               /* [nframes][3] out */
} slamit_rotation_batch;
int slamit_rotation_check_batch_dev(int device, const slamit_rotation_batch* batch, void* stream);

/* ---- Stereo matching: Frame::ComputeStereoMatches (src/Frame.cc:591-763) -------------------------------------------
 * From two ORBextractor calls on a rectified pair to mvuRight / mvDepth, on the pyramids the two calls left in HBM.  Per left
 * keypoint: the right keypoints whose row band (y +- 2 scale[octave]) holds row (int)vL, gated by octave (+-1) and by
 * uR in [uL - mbf / mb, uL + 3]; the least Hamming distance strictly below TH_HIGH = 100, the smallest right index on ties; at the
 * left keypoint's level an 11 x 11 patch minus its centre against 11 shifts of the right image (L1, exact integers); a parabola
 * through the best shift and its neighbours; disparity and depth; then, over the frame, every match whose SAD is not below
 * 1.5f * 1.4f * median is removed.  float / double exactly where the reference has them (csrc/stereo.h).
 * status[i] is where the walk of left keypoint i ended:
 *   0 matched   1 no right keypoint in the row, or uL + 3 < 0   2 none under TH_HIGH   3 the reference's right-window test
 *   4 best shift at -5 or +5   5 deltaR outside [-1, 1]   6 disparity outside [0, mbf / mb) (a NaN deltaR ends here)
 *   7 removed by the median filter   8 departure
 * u_right = depth = -1 unless status is 0; best_r / ham_dist are the chosen right keypoint and its distance (statuses 0, 3 .. 7, and
 * 8 when it was reached after the selection), sad_dist the best shift's sum (0, 4 .. 7); -1 where the walk did not get there.
 * DEPARTURES, where the reference reads out of bounds, throws or has undefined behaviour: a left keypoint is status 8 when its
 * octave, or its chosen right keypoint's, is outside [0, nlevels); when uL or vL is not finite; when (int)vL is outside [0, rows);
 * when its 11 x 11 window leaves the left plane of its level; when the right 11 x 21 strip (columns scaleduR0 - 10 .. scaleduR0 + 10,
 * rows scaledvL +- 5) leaves the right plane, which the reference's own test admits for scaleduR0 in [0, 10).  A right keypoint's
 * band is clamped to [0, rows); one with a coordinate that is not finite has none; one with an octave outside the table takes the
 * nearest level's.  An empty match list skips the median (the reference indexes an empty vector).  No device read depends on
 * these being absent; the extractor's own keypoints never meet them (they lie 16 level pixels inside their plane).
 * At most SLAMIT_STEREO_MAX_KP keypoints per side (the selection packs the right index into 16 bits beside the distance): more
 * fails with SLAMIT_ERR_CAPACITY and a message before anything is launched. */
#define SLAMIT_STEREO_MAX_KP 8191          /* = SLAMIT_SEARCH_MAX_KP */

/* Everything resident in HBM; frame f of the batch is frame f of both views.  Keypoints, descriptors and counts are in the layout
 * slamit_orb_extract_batch_dev writes ([nframes][cap], d_n clamped to [0, cap]; descriptors 16-byte aligned); d_mb / d_mbf hold one
 * float per frame, d_scale / d_inv_scale SLAMIT_MAX_LEVELS floats (mvScaleFactors, mvInvScaleFactors).  The views may be
 * slamit_orb_pyramid_view's or describe any planes of the caller's; both need the same nlevels and nframes >= the batch's; the
 * row table has left.level[0].h rows.  Outputs are [nframes][cap_left], d_n_matched [nframes] (matches with status 0).  Entries
 * past a frame's count are neither read nor written.  Asynchronous on `stream` (NULL: the legacy default stream of `device`), no
 * synchronisation, no state: three launches, with nothing through the host. */
typedef struct slamit_stereo_batch {
    int32_t nframes, cap_left, cap_right, reserved;
    slamit_pyramid_view left, right;
    const slamit_kp* d_kps_left;   /* [nframes][cap_left] (pt and octave are read) */
    const uint8_t* d_desc_left;    /* [nframes][cap_left][32] */
    const int32_t* d_n_left;       /* [nframes] */
    const slamit_kp* d_kps_right;  /* [nframes][cap_right] */
    const uint8_t* d_desc_right;   /* [nframes][cap_right][32] */
    const int32_t* d_n_right;      /* [nframes] */
    const float* d_mb;             /* [nframes]: Frame::mb */
    const float* d_mbf;            /* [nframes]: Frame::mbf */
    const float* d_scale;          /* [SLAMIT_MAX_LEVELS] */
    const float* d_inv_scale;      /* [SLAMIT_MAX_LEVELS] */
    void* d_workspace;             /* slamit_stereo_match_workspace(nframes, cap_right) bytes, 16-byte aligned */
    size_t workspace_bytes;
    float* d_u_right;              /* [nframes][cap_left] out: mvuRight */
    float* d_depth;                /* [nframes][cap_left] out: mvDepth */
    uint8_t* d_status;             /* [nframes][cap_left] out */
    int32_t* d_best_r;             /* [nframes][cap_left] out */
    int32_t* d_ham_dist;           /* [nframes][cap_left] out */
    int32_t* d_sad_dist;           /* [nframes][cap_left] out */
    int32_t* d_n_matched;          /* [nframes] out */
} slamit_stereo_batch;
size_t slamit_stereo_match_workspace(int nframes, int cap_right);
int slamit_stereo_match_batch_dev(int device, const slamit_stereo_batch* batch, void* stream);

/* One pair, host pointers, synchronous: frame `frame` of the two handles' last extract calls (which must have completed: the
 * host extract forms have, after a _dev form the caller synchronises its stream first), keypoints and descriptors as the
 * reference's Frame holds them (mvKeys / mvKeysRight, mDescriptors / mDescriptorsRight).  One staged call.  Handles that differ in
 * device, image size, level count or scale factor fail with SLAMIT_ERR_ARG; outputs have n_left entries; best_r, ham_dist,
 * sad_dist and n_matched may be NULL. */
int slamit_stereo_match(slamit_orb* left, slamit_orb* right, int frame, const slamit_kp* kps_left, const uint8_t* desc_left, int n_left,
                        const slamit_kp* kps_right, const uint8_t* desc_right, int n_right, float mb, float mbf, float* u_right, float* depth,
                        uint8_t* status, int32_t* best_r, int32_t* ham_dist, int32_t* sad_dist, int32_t* n_matched);

/* ---- RGB-D depth lookup: Frame::ComputeStereoFromRGBD (src/Frame.cc:766-787) ----------------------------------------
 * Per keypoint: row = (int)kp.pt.y, column = (int)kp.pt.x of the RAW keypoint (truncation), d = (float)plane[row][column] * factor
 * in float -- Tracking::GrabImageRGBD (src/Tracking.cc:267-268) converts every depth image with convertTo(CV_32F, mDepthMapFactor),
 * a float one too -- and, when d > 0, depth = d and u_right = kpU.pt.x - mbf / d from the UNDISTORTED keypoint (float, two
 * roundings); otherwise both are -1.  csrc/unproject.h restates it.  status[i]: 0 no depth (d <= 0 or NaN), 1 depth, 2 DEPARTURE:
 * the truncated row or column lies outside the plane, or a coordinate is not finite, where the reference reads out of bounds;
 * u_right = depth = -1.  n above SLAMIT_STEREO_MAX_KP fails with SLAMIT_ERR_CAPACITY; an unknown element type, a pitch below a
 * row's bytes, a negative size or a missing array with n > 0 fails with SLAMIT_ERR_ARG; both with a message, before anything is
 * launched.  n == 0 and nproblems == 0 are valid and write nothing. */
enum { SLAMIT_DEPTH_F32 = 0, SLAMIT_DEPTH_U16 = 1 };

struct slamit_depth_plane {
    const void* data;              /* first element of row 0 */
    size_t pitch;                  /* bytes between rows, >= width * element size */
    int32_t width, height;
    int32_t type;                  /* SLAMIT_DEPTH_* */
    float factor;                  /* mDepthMapFactor: 1 / DepthMapFactor of the settings, 1 when that is 0 */
};
typedef struct slamit_depth_plane slamit_depth_plane;

struct slamit_rgbd_problem {
    slamit_depth_plane plane;      /* host memory */
    float mbf;                     /* Frame::mbf */
    int32_t n;
    const slamit_kp* kps;          /* n: mvKeys (pt is read) */
    const slamit_kp* kps_un;       /* n: mvKeysUn (pt.x is read) */
};
typedef struct slamit_rgbd_problem slamit_rgbd_problem;

struct slamit_rgbd_result {
    float* u_right;                /* n out: mvuRight */
    float* depth;                  /* n out: mvDepth */
    uint8_t* status;               /* n out */
};
typedef struct slamit_rgbd_result slamit_rgbd_result;

/* nproblems frames in one launch (host pointers, synchronous; the planes travel without their row padding). */
int slamit_rgbd_depth_batch(int device, int nproblems, const slamit_rgbd_problem* probs, slamit_rgbd_result* results);
int slamit_rgbd_depth(int device, const slamit_rgbd_problem* prob, slamit_rgbd_result* res);

/* Everything resident in HBM: the keypoints and counts slamit_orb_extract_batch_dev and slamit_frame_finish_batch_dev left
 * ([nframes][cap], d_n clamped to [0, cap]), one plane record per frame in device memory whose `data` is a device pointer, and the
 * outputs in the layout slamit_stereo_match_batch_dev writes.  Entries past a frame's count are neither read nor written.  The host
 * cannot see d_planes: a type other than SLAMIT_DEPTH_U16 is read as float.  Asynchronous on `stream` (NULL: the legacy default
 * stream of `device`), no synchronisation, no state. */
struct slamit_rgbd_batch_rec {
    int32_t nframes, cap;
    const slamit_depth_plane* d_planes; /* [nframes] */
    const float* d_mbf;            /* [nframes] */
    const slamit_kp* d_kps;        /* [nframes][cap] */
    const slamit_kp* d_kps_un;     /* [nframes][cap] */
    const int32_t* d_n;            /* [nframes] */
    float* d_u_right;              /* [nframes][cap] out */
    float* d_depth;                /* [nframes][cap] out */
    uint8_t* d_status;             /* [nframes][cap] out, nullable */
};
typedef struct slamit_rgbd_batch_rec slamit_rgbd_batch_rec;
int slamit_rgbd_depth_batch_dev(int device, const slamit_rgbd_batch_rec* batch, void* stream);

/* ---- Closest points: the walk of UpdateLastFrame, CreateNewKeyFrame and StereoInitialization -----------------------
 * Tracking::UpdateLastFrame (src/Tracking.cc:1039-1091), the stereo branch of CreateNewKeyFrame (:1334-1396) and
 * StereoInitialization (:712-727) with Frame::UnprojectStereo (src/Frame.cc:789-803) and what the new MapPoint stores
 * (src/MapPoint.cc:52-77, :336-377); float / double exactly where the reference has them (csrc/unproject.h lists every split).
 * The candidates are the keypoints with depth > 0 (a NaN is none, +inf is one), sorted by (depth, index).  Mode CLOSEST visits the
 * first n_visited = min(M, max(c, min_points) + 1) of them, M candidates of which c have !(depth > th_depth): the reference's loop,
 * which takes one far point beyond the close set whenever there is one.  Mode ALL visits every candidate in index order and does
 * not look at `tracked`, which may then be NULL.  status[i]:
 *   0 no depth   1 beyond the cut   2 visited, keeps its tracked point (tracked[i] != 0)   3 visited, point created
 *   4 DEPARTURE: visited and in need of a point, but the octave lies outside [0, n_levels), where the reference indexes
 *     mvScaleFactors unchecked; it counts in the walk and nothing is created
 * order[j] is the keypoint at walk position j < n_visited (-1 from there to n): creating the points in this order gives them the
 * reference's mnId.  pos, normal, max_dist (the RAW mfMaxDistance), min_dist are written for status 3 and are zero elsewhere.
 * ctor says which constructor's normal is wanted: they differ in the sign of a zero component only (csrc/unproject.h).
 * counts: n_candidates = M, n_close = c, n_visited, n_created, and NeedNewKeyFrame's two numbers (src/Tracking.cc:1244-1253):
 * n_total = keypoints with 0 < depth < th_depth (strict, unlike the cut), n_map = those of them with tracked[i] != 0.
 * n above SLAMIT_STEREO_MAX_KP fails with SLAMIT_ERR_CAPACITY; n_levels outside [1, SLAMIT_MAX_LEVELS], an unknown mode or ctor,
 * min_points < 0 or a missing array with n > 0 fails with SLAMIT_ERR_ARG; both with a message, before anything is launched.
 * n == 0 and nproblems == 0 are valid and write nothing but zero counts. */
enum { SLAMIT_UNPROJECT_CLOSEST = 0, SLAMIT_UNPROJECT_ALL = 1 };
enum { SLAMIT_UNPROJECT_CTOR_FRAME = 0, SLAMIT_UNPROJECT_CTOR_KEYFRAME = 1 };

struct slamit_unproject_frame {
    float fx, fy, cx, cy, invfx, invfy; /* as the frame holds them */
    float Rwc[9], Ow[3];           /* mRwc (row-major), mOw */
    float th_depth;                /* mThDepth */
    int32_t min_points;            /* 100 in both callers */
    int32_t mode;                  /* SLAMIT_UNPROJECT_CLOSEST / _ALL */
    int32_t ctor;                  /* SLAMIT_UNPROJECT_CTOR_FRAME (UpdateLastFrame) / _KEYFRAME (the other two) */
    int32_t n_levels;              /* entries of scale_factors in use */
    float scale_factors[SLAMIT_MAX_LEVELS]; /* mvScaleFactors */
};
typedef struct slamit_unproject_frame slamit_unproject_frame;

struct slamit_unproject_counts {
    int32_t n_candidates, n_close, n_visited, n_created, n_total, n_map;
};
typedef struct slamit_unproject_counts slamit_unproject_counts;

struct slamit_unproject_problem {
    slamit_unproject_frame frame;
    int32_t n;
    const slamit_kp* kps_un;       /* n: mvKeysUn (pt and octave are read) */
    const float* depth;            /* n: mvDepth */
    const uint8_t* tracked;        /* n: 1 = mvpMapPoints[i] is non-null with Observations() >= 1 */
};
typedef struct slamit_unproject_problem slamit_unproject_problem;

struct slamit_unproject_result {
    uint8_t* status;               /* n out */
    int32_t* order;                /* n out */
    float* pos;                    /* n x 3 out */
    float* normal;                 /* n x 3 out */
    float* max_dist;               /* n out */
    float* min_dist;               /* n out */
    slamit_unproject_counts counts; /* out */
};
typedef struct slamit_unproject_result slamit_unproject_result;

/* nproblems frames in one launch (host pointers, synchronous). */
int slamit_unproject_closest_batch(int device, int nproblems, const slamit_unproject_problem* probs, slamit_unproject_result* results);
int slamit_unproject_closest(int device, const slamit_unproject_problem* prob, slamit_unproject_result* res);

/* Everything resident in HBM, MERGED IN PLACE into the arrays slamit_project_batch_dev form 0 reads (q_cap = cap: query i is the
 * last frame's keypoint i).  The caller has filled the tracked points and set skip = 1 where there is none; for a created point
 * (status 3) this writes d_pos[f][c][i], d_octave[f][i], d_skip[f][i] = 0 and, where present, d_normal / d_max_dist / d_min_dist
 * in slamit_frustum_batch_dev's layout; every other entry of those arrays is left alone.  d_status, d_order ([nframes][cap]) and
 * d_counts ([nframes]) are written in full for the first min(d_n[f], cap) entries when present.  The host cannot see d_frames: an
 * octave is accepted only below min(n_levels, SLAMIT_MAX_LEVELS), a mode other than ALL is CLOSEST.  Asynchronous on `stream`
 * (NULL: the legacy default stream of `device`), no synchronisation, no state: UpdateLastFrame, slamit_project_batch_dev_stereo,
 * slamit_guided_search_stereo_batch_dev and slamit_rotation_check_batch_dev run on one stream without the host. */
struct slamit_unproject_batch_rec {
    int32_t nframes, cap;
    const slamit_unproject_frame* d_frames; /* [nframes] */
    const int32_t* d_n;            /* [nframes] keypoints per frame */
    const slamit_kp* d_kps_un;     /* [nframes][cap] */
    const float* d_depth;          /* [nframes][cap] */
    const uint8_t* d_tracked;      /* [nframes][cap] */
    float* d_pos;                  /* [nframes][3][cap] in / out */
    int32_t* d_octave;             /* [nframes][cap] in / out */
    uint8_t* d_skip;               /* [nframes][cap] in / out */
    float* d_normal;               /* [nframes][3][cap] in / out, nullable */
    float* d_max_dist;             /* [nframes][cap] in / out, nullable */
    float* d_min_dist;             /* [nframes][cap] in / out, nullable */
    uint8_t* d_status;             /* [nframes][cap] out, nullable */
    int32_t* d_order;              /* [nframes][cap] out, nullable */
    slamit_unproject_counts* d_counts; /* [nframes] out, nullable */
};
typedef struct slamit_unproject_batch_rec slamit_unproject_batch_rec;
int slamit_unproject_closest_batch_dev(int device, const slamit_unproject_batch_rec* batch, void* stream);

/* ---- UpdateLocalMap: keyframe votes, local keyframes, local points (tracking, in front of SearchLocalPoints) ----
 * Tracking::UpdateLocalKeyFrames and ::UpdateLocalPoints (src/Tracking.cc:1467-1626) and the skip flags of SearchLocalPoints' first
 * loop (:1412-1428), over tables of slots the caller keeps (csrc/local_map.h states the walk).  Integer work and
 * copies of stored floats only: the results are exact.  Every id is a slot (int32), -1 = none.
 *   (a) votes[k] = the entries of frame_mp that are non-null, not bad, and that keyframe k observes; a bad point's entry becomes -1
 *   (b) the voted non-bad keyframes, then the reference's one-hop expansion (first good unmarked of the best ten, first good
 *       unmarked child, the parent without a bad test, which ends the walk; no visit once the list exceeds 80), and the reference
 *       keyframe (the first with the strictly largest count).  With no vote at all local_kf, n_local_kf and ref_kf are left as
 *       they were; with every voted keyframe bad the list becomes empty and ref_kf stays.
 *   (c) the points of the local keyframes in list order and keypoint order, NULL and bad ones dropped, first occurrence kept;
 *       skip = 1 for a point among the frame's own non-null entries after (a) or in frame_seen.
 * ORDER: the reference walks std::map / std::set of pointers, i.e. in address order.  Here voted keyframes are taken in ASCENDING
 * SLOT order and children AS GIVEN; a caller that numbers keyframes by std::less<KeyFrame*> and lists children in set order
 * (shim/Tracking.h) gets the reference's own order on that run.
 * COST: building these tables from host objects costs about what the host loop itself costs, so the host forms are for parity and
 * tests; the gain is the resident form, where the tables live in HBM and are updated when the map changes.
 * Status bits, per frame: */
#define SLAMIT_LOCAL_MAP_BAD_SLOT 1       /* device form: a slot outside its table was skipped (never dereferenced) */
#define SLAMIT_LOCAL_MAP_KF_OVERFLOW 2    /* more local keyframes than kf_cap: n_local_kf is the number needed, the first kf_cap are written */
#define SLAMIT_LOCAL_MAP_MP_OVERFLOW 4    /* more local points than q_cap: n_local_mp is the number needed, the first q_cap are written */
#define SLAMIT_LOCAL_MAP_ROW_CUT 8        /* a keyframe with more than SLAMIT_LOCAL_MAP_MAX_ROW keypoints: the rest were not read */
#define SLAMIT_LOCAL_MAP_MAX_KF 65535     /* keyframes per map, and kf_cap: the upper 16 bits of the first-occurrence key */
#define SLAMIT_LOCAL_MAP_MAX_ROW 65536    /* keypoints per keyframe: the key's lower 16 bits */
#define SLAMIT_LOCAL_MAP_MIN_KF_CAP 83    /* kf_cap at least 80 + 3: the expansion then never overflows */
#define SLAMIT_LOCAL_MAP_MAX_MAPS 8       /* maps per batch: their records travel as the kernels' argument */
#define SLAMIT_LOCAL_MAP_BEST 10          /* GetBestCovisibilityKeyFrames(10) */

/* One map.  Host pointers in the host forms, device pointers in slamit_local_map_batch_rec.maps.  The pointer arrays of the three
 * CSR tables are trusted to ascend from 0; slots are checked. */
struct slamit_map_index {
    int32_t n_kf, n_mp;
    const int32_t* obs_ptr;        /* [n_mp + 1] */
    const int32_t* obs_kf;         /* the keyframes observing point p: obs_kf[obs_ptr[p] .. obs_ptr[p + 1]), any order */
    const uint8_t* mp_bad;         /* [n_mp] MapPoint::isBad() */
    const uint8_t* kf_bad;         /* [n_kf] KeyFrame::isBad() */
    const int32_t* kf_mp_ptr;      /* [n_kf + 1] */
    const int32_t* kf_mp;          /* GetMapPointMatches() of keyframe k by keypoint index, -1 for NULL */
    const int32_t* kf_best;        /* [n_kf][SLAMIT_LOCAL_MAP_BEST] the first ten of mvpOrderedConnectedKeyFrames, padded with -1 */
    const int32_t* kf_child_ptr;   /* [n_kf + 1] */
    const int32_t* kf_child;       /* GetChilds() in the order to walk them */
    const int32_t* kf_parent;      /* [n_kf] GetParent() */
    const float* mp_pos;           /* [n_mp][3] GetWorldPos()       -- the last four are read by the resident form only */
    const float* mp_normal;        /* [n_mp][3] GetNormal() */
    const float* mp_max_dist;      /* [n_mp] the RAW mfMaxDistance, as slamit_frustum_problem documents it */
    const float* mp_min_dist;      /* [n_mp] the raw mfMinDistance */
};
typedef struct slamit_map_index slamit_map_index;

/* (a) + (b) for one frame (host pointers, synchronous).  frame_mp[n] in / out (mvpMapPoints as slots, n <= SLAMIT_FRAME_MAX_KP);
 * votes[n_kf] out; local_kf[kf_cap], *n_local_kf, *ref_kf in / out; *status out.  Reads obs_*, mp_bad, kf_bad, kf_best, kf_child*,
 * kf_parent.  A null array, a slot outside its table, n_kf above SLAMIT_LOCAL_MAP_MAX_KF or kf_cap outside
 * [SLAMIT_LOCAL_MAP_MIN_KF_CAP, SLAMIT_LOCAL_MAP_MAX_KF] fails with SLAMIT_ERR_ARG and a message before anything is launched. */
int slamit_local_keyframes(int device, const slamit_map_index* map, int32_t n, int32_t* frame_mp, int32_t* votes, int32_t kf_cap,
                           int32_t* local_kf, int32_t* n_local_kf, int32_t* ref_kf, int32_t* status);

/* (c) for a given keyframe list (host pointers, synchronous).  frame_mp[n] is the list (a) cleaned; frame_seen[n_seen] may be NULL
 * with n_seen = 0; local_kf[n_local_kf].  local_mp[q_cap] and skip[q_cap] in / out: entries past min(*n_local_mp, q_cap) are left as
 * the caller filled them.  Reads kf_mp*, mp_bad.  q_cap above SLAMIT_FRUSTUM_MAX_N, n_local_kf above SLAMIT_LOCAL_MAP_MAX_KF, a row
 * above SLAMIT_LOCAL_MAP_MAX_ROW, a null array or a slot outside its table fails with SLAMIT_ERR_ARG before anything is launched. */
int slamit_local_points(int device, const slamit_map_index* map, int32_t n, const int32_t* frame_mp, int32_t n_seen,
                        const int32_t* frame_seen, int32_t n_local_kf, const int32_t* local_kf, int32_t q_cap, int32_t* local_mp,
                        uint8_t* skip, int32_t* n_local_mp, int32_t* status);

/* All three passes for nframes frames, everything resident in HBM.  `maps` is a HOST array of n_maps records holding DEVICE
 * pointers; frame f uses maps[d_frame_map[f]] (outside [0, n_maps): the frame is left alone but for n_local_mp = m = 0 and
 * SLAMIT_LOCAL_MAP_BAD_SLOT).  vote_cap >= every n_kf, mp_cap >= every n_mp.  Counts are clamped to their capacities.  The device
 * cannot be shown its tables first: a slot outside its table is skipped, never dereferenced, and sets SLAMIT_LOCAL_MAP_BAD_SLOT.
 * d_pos .. d_m are the arrays slamit_frustum_batch_dev reads, in its layout (d_m = min(n_local_mp, q_cap)), so that call and
 * slamit_guided_search_batch_dev follow on the same stream with no host visit.  Entries past d_m[f] are not written.
 * Asynchronous on `stream` (NULL: the legacy default stream of `device`), no synchronisation, no state; the workspace is cleared
 * on the stream by the call. */
struct slamit_local_map_batch_rec {
    int32_t nframes, n_maps, kp_cap, seen_cap, kf_cap, q_cap, vote_cap, mp_cap;
    const slamit_map_index* maps;  /* HOST [n_maps], device pointers inside; n_maps <= SLAMIT_LOCAL_MAP_MAX_MAPS */
    const int32_t* d_frame_map;    /* [nframes] */
    const int32_t* d_n;            /* [nframes] keypoints per frame */
    int32_t* d_frame_mp;           /* [nframes][kp_cap] in / out */
    const int32_t* d_n_seen;       /* [nframes], nullable together with d_frame_seen */
    const int32_t* d_frame_seen;   /* [nframes][seen_cap] */
    int32_t* d_votes;              /* [nframes][vote_cap] out: the first n_kf of a frame's row, the rest 0 */
    int32_t* d_local_kf;           /* [nframes][kf_cap] in / out */
    int32_t* d_n_local_kf;         /* [nframes] in / out */
    int32_t* d_ref_kf;             /* [nframes] in / out */
    int32_t* d_local_mp;           /* [nframes][q_cap] out */
    int32_t* d_n_local_mp;         /* [nframes] out: the number needed */
    float* d_pos;                  /* [nframes][3][q_cap] out */
    float* d_normal;               /* [nframes][3][q_cap] out */
    float* d_max_dist;             /* [nframes][q_cap] out */
    float* d_min_dist;             /* [nframes][q_cap] out */
    uint8_t* d_skip;               /* [nframes][q_cap] out */
    int32_t* d_m;                  /* [nframes] out */
    int32_t* d_status;             /* [nframes] out */
    void* d_workspace;             /* slamit_local_map_workspace(nframes, mp_cap, kf_cap) bytes */
    size_t workspace_bytes;
};
typedef struct slamit_local_map_batch_rec slamit_local_map_batch_rec;
size_t slamit_local_map_workspace(int nframes, int mp_cap, int kf_cap);
int slamit_local_map_batch_dev(int device, const slamit_local_map_batch_rec* batch, void* stream);

/* ---- Covisibility: KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling (local mapping) ----
 * UpdateConnections (src/KeyFrame.cc:296-386, with AddConnection / UpdateBestCovisibles :127-161) and KeyFrameCulling
 * (src/LocalMapping.cc:686-752) over the tables of slamit_map_index and the columns and graph rows of slamit_covis_index
 * (csrc/covis.h states both walks).  Integer work and float compares as the reference writes them: the results are
 * exact.  Every id is a slot (int32), -1 = none.
 * THE GRAPH: row j of cw_kf / cw_w (cw_n[j] entries, ASCENDING SLOT) is mConnectedKeyFrameWeights of keyframe j; row j of ord_kf /
 * ord_w (ord_n[j] entries) is mvpOrderedConnectedKeyFrames / mvOrderedWeights: descending weight and, within equal weight,
 * DESCENDING slot -- the reference's sort of (weight, pointer) pushed to the front, for a caller that numbers keyframes by
 * std::less<KeyFrame*> (shim/LocalMapping.h).  Rows hold row_cap entries; what lies past a row's count is neither read nor written.
 * UpdateConnections for keyframe k:
 *   (a) counts[j] = the non-null, non-bad points of k that keyframe j != k observes (a bad OBSERVER counts: the reference does not test)
 *   (b) no count at all: the reference returns; every row, kf_best and *parent stay byte for byte, SLAMIT_COVIS_NO_OBSERVER
 *   (c) k's cw row = the whole counter; k's ord row = the keyframes with count >= 15, or else the single one with the strictly
 *       largest count, first in ascending slot order
 *   (d) AddConnection(k, w) on each listed j: nothing of j changes if its cw row holds (k, w); else the entry is inserted or updated
 *       and j's ord row becomes the sort of j's WHOLE cw row (UpdateBestCovisibles: below-threshold entries are listed too)
 *   (e) kf_best rows of k and of every changed j = the first ten of the ord row, padded with -1; *parent = the front of k's list when
 *       first_connection is set and k != origin_kf, else -1.  The parent / children tables stay the caller's.
 *   (f) a counter above row_cap: only counts and *n_counted are written, SLAMIT_COVIS_ROW_OVERFLOW; a full row of j that lacks k
 *       leaves j as it was, with the same status.
 * KeyFrameCulling for current keyframe c: the candidates are c's ord row, in row order.  origin_kf is skipped (verdict 3).  A keypoint
 * whose point is non-null and not bad counts in n_mps unless (monocular == 0) depth > th_depth || depth < 0; it is redundant when
 * Observations() > 3 and at least 3 observers other than the candidate have octave <= own octave + 1; the candidate goes when
 * n_redundant > 0.9 * n_mps (double).  The cascade is kept: against the set S of keyframes culled earlier in the call an observer in S
 * is not there, Observations() is mp_nobs - the obs_weight of the observers in S, and a point that lost an observer and is left with
 * <= 2 is bad (mp_turned_bad).  A candidate with kf_not_erase gets verdict 2 and does not enter S.  No table is modified: applying
 * the verdicts is the caller's work.
 * COST: as for the local map, building the tables from host objects costs about what the host loops cost; the gain is the resident form.
 * Status bits, per item / problem: */
#define SLAMIT_COVIS_NO_OBSERVER 1        /* UpdateConnections: no keyframe shares a point with k; nothing was changed */
#define SLAMIT_COVIS_ROW_OVERFLOW 2       /* k's counter above row_cap (nothing changed), or a full row of a neighbour (left as it was) */
#define SLAMIT_COVIS_BAD_SLOT 4           /* device form: a slot outside its table was skipped (never dereferenced) */
#define SLAMIT_COVIS_MAX_ROW 1024         /* row_cap: a row is sorted in LDS */
#define SLAMIT_COVIS_TH 15                /* UpdateConnections' threshold */
#define SLAMIT_COVIS_KEPT 0               /* verdicts */
#define SLAMIT_COVIS_CULLED 1
#define SLAMIT_COVIS_TO_BE_ERASED 2
#define SLAMIT_COVIS_ORIGIN 3

/* The columns and graph rows beside one slamit_map_index.  Host pointers in the host forms, device pointers in the batch records. */
struct slamit_covis_index {
    int32_t row_cap;               /* entries per graph row, <= SLAMIT_COVIS_MAX_ROW */
    int32_t origin_kf;             /* slot of the keyframe with mnId 0, -1 = none */
    const uint8_t* obs_octave;     /* beside obs_kf: mvKeysUn[idx].octave of that observation in the observing keyframe */
    const uint8_t* obs_weight;     /* beside obs_kf: 2 if that keyframe's mvuRight[idx] >= 0, else 1 */
    const int32_t* mp_nobs;        /* [n_mp] MapPoint::Observations() */
    const uint8_t* kf_octave;      /* beside kf_mp: mvKeysUn[i].octave */
    const float* kf_depth;         /* beside kf_mp: mvDepth[i]; NULL = monocular */
    const float* kf_th_depth;      /* [n_kf] mThDepth; NULL together with kf_depth */
    const uint8_t* kf_not_erase;   /* [n_kf] mbNotErase */
    int32_t *cw_kf, *cw_w, *cw_n;      /* [n_kf][row_cap], [n_kf]: mConnectedKeyFrameWeights, ascending slot -- in / out */
    int32_t *ord_kf, *ord_w, *ord_n;   /* mvpOrderedConnectedKeyFrames / mvOrderedWeights -- in / out */
    int32_t* kf_best;              /* [n_kf][SLAMIT_LOCAL_MAP_BEST], nullable: the memory the map record's kf_best points to */
};
typedef struct slamit_covis_index slamit_covis_index;

/* UpdateConnections for keyframe k of one map (host pointers, synchronous).  Reads obs_*, mp_bad, kf_mp* of `map`; counts[n_kf],
 * *n_counted (the size of the counter), *n_listed (the length of k's new list, 0 when nothing was done) and *status out; *parent in /
 * out; the seven graph arrays of `covis` in / out.  A null table, k or a table's slot outside its table, or row_cap outside
 * [1, SLAMIT_COVIS_MAX_ROW] fails with SLAMIT_ERR_ARG and a message before anything is launched. */
int slamit_update_connections(int device, const slamit_map_index* map, const slamit_covis_index* covis, int32_t k, int32_t first_connection,
                              int32_t* counts, int32_t* n_counted, int32_t* n_listed, int32_t* parent, int32_t* status);

/* The same for nitems keyframes of nitems DIFFERENT maps, everything resident.  `maps`, `covis` and `item_map` are HOST arrays; the
 * records hold DEVICE pointers.  The reference is sequential over the keyframes of one map, so a second keyframe of a map is a second
 * call on the same stream: a map named twice in item_map fails with SLAMIT_ERR_ARG.  count_cap >= every n_kf.  The device cannot be
 * shown its tables first: a slot outside its table is skipped, never dereferenced, and sets SLAMIT_COVIS_BAD_SLOT (k itself outside
 * its map: that item does nothing else).  Asynchronous on `stream`, no synchronisation, no state, no workspace. */
struct slamit_covis_batch_rec {
    int32_t nitems, n_maps, count_cap, reserved;
    const slamit_map_index* maps;      /* HOST [n_maps], device pointers inside; n_maps <= SLAMIT_LOCAL_MAP_MAX_MAPS */
    const slamit_covis_index* covis;   /* HOST [n_maps], device pointers inside */
    const int32_t* item_map;           /* HOST [nitems], each in [0, n_maps), no repeat */
    const int32_t* d_kf;               /* [nitems] k */
    const int32_t* d_first;            /* [nitems] mbFirstConnection, 0 / 1 */
    int32_t* d_counts;                 /* [nitems][count_cap] out: the first n_kf of an item's row, the rest 0 */
    int32_t* d_n_counted;              /* [nitems] out */
    int32_t* d_n_listed;               /* [nitems] out */
    int32_t* d_parent;                 /* [nitems] in / out */
    int32_t* d_status;                 /* [nitems] out */
};
typedef struct slamit_covis_batch_rec slamit_covis_batch_rec;
int slamit_update_connections_batch_dev(int device, const slamit_covis_batch_rec* batch, void* stream);

/* KeyFrameCulling for current keyframe c (host pointers, synchronous).  Reads obs_*, mp_bad, kf_mp* of `map` and the columns, ord_kf
 * and ord_n of `covis`.  verdict / n_mps / n_redundant hold row_cap entries, in / out: the first *n_cand are written.  mp_turned_bad[n_mp]
 * in / out: bytes set to 1, the others left alone.  kf_depth NULL with monocular == 0, a null table, a slot outside its table or row_cap
 * outside [1, SLAMIT_COVIS_MAX_ROW] fails with SLAMIT_ERR_ARG before anything is launched. */
int slamit_keyframe_culling(int device, const slamit_map_index* map, const slamit_covis_index* covis, int32_t c, int32_t monocular,
                            uint8_t* verdict, int32_t* n_mps, int32_t* n_redundant, int32_t* n_cand, uint8_t* mp_turned_bad, int32_t* status);

/* The same for nprob current keyframes, resident; problems may share a map (nothing is modified).  Problem f uses
 * maps[d_prob_map[f]] (outside [0, n_maps): n_cand = 0 and SLAMIT_COVIS_BAD_SLOT).  cand_cap >= every row_cap, mp_cap >= every n_mp.
 * Asynchronous on `stream`, no state, no workspace. */
struct slamit_culling_batch_rec {
    int32_t nprob, n_maps, cand_cap, mp_cap;
    const slamit_map_index* maps;      /* HOST [n_maps] */
    const slamit_covis_index* covis;   /* HOST [n_maps] */
    const int32_t* d_prob_map;         /* [nprob] */
    const int32_t* d_kf;               /* [nprob] c */
    const int32_t* d_monocular;        /* [nprob] mbMonocular, 0 / 1 */
    uint8_t* d_verdict;                /* [nprob][cand_cap] in / out */
    int32_t* d_n_mps;                  /* [nprob][cand_cap] in / out */
    int32_t* d_n_redundant;            /* [nprob][cand_cap] in / out */
    int32_t* d_n_cand;                 /* [nprob] out */
    uint8_t* d_mp_turned_bad;          /* [nprob][mp_cap] in / out */
    int32_t* d_status;                 /* [nprob] out */
};
typedef struct slamit_culling_batch_rec slamit_culling_batch_rec;
int slamit_keyframe_culling_batch_dev(int device, const slamit_culling_batch_rec* batch, void* stream);

/* ---- Map-point upkeep: UpdateNormalAndDepth, ComputeDistinctiveDescriptors, MapPointCulling (local mapping) ----
 * MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:336-377), MapPoint::ComputeDistinctiveDescriptors (:248-313) and
 * LocalMapping::MapPointCulling (src/LocalMapping.cc:184-219) over the tables of slamit_map_index and the columns of
 * slamit_point_index (csrc/upkeep.h states the walks).  Every id is a slot (int32), -1 = none.
 * NORMAL AND DEPTH of point p (what & 1): a bad point or one without observations changes nothing.  Otherwise
 * normal = sum over EVERY observer i (bad keyframes too: the reference does not test) of (Pos - Ow_i) / |Pos - Ow_i|, taken in float
 * one observer after the other in ASCENDING SLOT (std::map<KeyFrame*, size_t> order for a caller that numbers keyframes by
 * address; the rows of obs_kf may come in any order), divided by their number; dist = |Pos - Ow_ref|; max_dist =
 * dist * scale_factors[level], min_dist = max_dist / scale_factors[n_levels - 1], level = obs_octave of the reference keyframe's
 * observation.  A reference keyframe that is not among the observers takes the octave of its keypoint 0, as observations[pRefKF]
 * default-inserts index 0 (SLAMIT_UPKEEP_REF_NOT_OBSERVER).  Where the reference reads out of bounds -- mp_ref_kf == -1, that
 * keyframe without keypoints, a level outside [0, n_levels) -- the normal and both distances stay as they were and the status says why.
 * The float / double evaluation is the one csrc/unproject.h states for these lines; PARITY UNPINNED as there.
 * DESCRIPTOR of point p (what & 2): the rows are kf_desc[kf_mp_ptr[k] + obs_idx] of the observers k that are NOT bad, in ascending
 * slot; the row with the least median distance to the others (vDists[(int)(0.5 * (N - 1))], the first on ties) is copied into
 * mp_desc[p].  A bad point, no observation or no good observer changes nothing; more than SLAMIT_DISTINCTIVE_MAX good observers
 * sets SLAMIT_UPKEEP_DESC_OVERFLOW and leaves the descriptor (the normal is still updated).  Exact.
 * MAPPOINTCULLING of a recent list with the current keyframe's mnId: per entry the first matching verdict of
 *   1 already bad | 2 (float)found / visible < 0.25f as written (visible == 0: inf or NaN, not below) | 3 (int)cur - (int)first_kf >= 2
 *   && nobs <= th (2 monocular, 3 otherwise) | 4 (int)cur - (int)first_kf >= 3 | 0 kept,
 * and the kept entries compacted in list order.  Nothing is applied: SetBadFlag on verdicts 2 and 3 is the caller's work.
 * COST: as for the local map, building the tables from host objects costs about what the host loops cost; the gain is the resident form.
 * Status bits, per listed point (the last also per recent list): */
#define SLAMIT_UPKEEP_REF_NOT_OBSERVER 1  /* the reference keyframe does not observe the point: the octave of its keypoint 0 was used */
#define SLAMIT_UPKEEP_NO_REF 2            /* mp_ref_kf == -1: normal and distances left as they were */
#define SLAMIT_UPKEEP_REF_NO_KP 4         /* that odd place with a reference keyframe without keypoints: left as they were */
#define SLAMIT_UPKEEP_OCTAVE 8            /* the level lies outside [0, n_levels): left as they were */
#define SLAMIT_UPKEEP_DESC_OVERFLOW 16    /* more than SLAMIT_DISTINCTIVE_MAX good observers: the descriptor was left as it was */
#define SLAMIT_UPKEEP_OBS_OVERFLOW 32     /* more than SLAMIT_UPKEEP_MAX_OBS observers: the point was left as it was */
#define SLAMIT_UPKEEP_BAD_SLOT 64         /* device form: a slot outside its table was skipped (never dereferenced) */
#define SLAMIT_UPKEEP_MAX_OBS 512         /* observers per point: a row is ordered in LDS */
#define SLAMIT_UPKEEP_MAX_POINTS 65536    /* listed points per call / per item of a batch */
#define SLAMIT_UPKEEP_MAX_RECENT 65536    /* entries of a recent list */
#define SLAMIT_UPKEEP_NORMAL 1            /* `what` */
#define SLAMIT_UPKEEP_DESC 2
#define SLAMIT_UPKEEP_KEPT 0              /* verdicts */
#define SLAMIT_UPKEEP_WAS_BAD 1
#define SLAMIT_UPKEEP_LOW_RATIO 2
#define SLAMIT_UPKEEP_FEW_OBS 3
#define SLAMIT_UPKEEP_AGED 4

/* The columns beside one slamit_map_index that map-point upkeep reads and writes.  Host pointers in the host forms, device pointers
 * in the batch records.  Of the map record these calls read obs_ptr, obs_kf, mp_bad, kf_bad, kf_mp_ptr and mp_pos. */
struct slamit_point_index {
    int32_t n_levels;              /* mnScaleLevels, in [1, SLAMIT_MAX_LEVELS] */
    int32_t reserved;
    float scale_factors[SLAMIT_MAX_LEVELS]; /* mvScaleFactors */
    const int32_t* obs_idx;        /* beside obs_kf: mObservations[pKF], the keypoint index in the observing keyframe */
    const uint8_t* obs_octave;     /* beside obs_kf: as slamit_covis_index.obs_octave (may be the same memory) */
    const uint8_t* kf_octave;      /* beside kf_mp: mvKeysUn[i].octave */
    const float* kf_center;        /* [n_kf][3] GetCameraCenter() */
    const uint8_t* kf_desc;        /* beside kf_mp: 32 bytes per keypoint, mDescriptors.row(i); 16-byte aligned in the device form */
    const int32_t* mp_ref_kf;      /* [n_mp] mpRefKF */
    const int32_t* mp_nobs;        /* [n_mp] Observations() */
    const int32_t* mp_found;       /* [n_mp] mnFound */
    const int32_t* mp_visible;     /* [n_mp] mnVisible */
    const int32_t* mp_first_kf;    /* [n_mp] mnFirstKFid */
    float* mp_normal;              /* [n_mp][3] in / out: the memory the map record's mp_normal points to */
    float* mp_max_dist;            /* [n_mp] in / out: likewise */
    float* mp_min_dist;            /* [n_mp] in / out: likewise */
    uint8_t* mp_desc;              /* [n_mp][32] in / out: mDescriptor; 16-byte aligned in the device form */
};
typedef struct slamit_point_index slamit_point_index;

/* The n listed points of one map (host pointers, synchronous).  `what` is SLAMIT_UPKEEP_NORMAL | SLAMIT_UPKEEP_DESC; status[n] out.
 * With what & 1 the call reads obs_octave, kf_octave, kf_center, mp_ref_kf and mp_pos and rewrites mp_normal, mp_max_dist, mp_min_dist;
 * with what & 2 it reads kf_bad, obs_idx, kf_desc and rewrites mp_desc; tables of the other part may be NULL.  A point listed twice is
 * written twice with the same bytes.  A null table, a slot outside its table (points, obs_kf, mp_ref_kf, obs_idx), `what` outside
 * 1..3 or n_levels outside [1, SLAMIT_MAX_LEVELS] fails with SLAMIT_ERR_ARG, n above SLAMIT_UPKEEP_MAX_POINTS with
 * SLAMIT_ERR_CAPACITY, each with a message and before anything is launched. */
int slamit_update_points(int device, const slamit_map_index* map, const slamit_point_index* pts, int32_t n, const int32_t* points,
                         int32_t what, int32_t* status);

/* The same for nitems lists over up to SLAMIT_LOCAL_MAP_MAX_MAPS maps, everything resident.  `maps` and `pts` are HOST arrays of
 * records holding DEVICE pointers; item i lists d_n[i] points (clamped to cap) of maps[d_item_map[i]] with d_what[i].  The device
 * cannot be shown its tables first: a slot outside its table is skipped, never dereferenced, and sets SLAMIT_UPKEEP_BAD_SLOT (a
 * map index or a listed point outside its table: that entry does nothing else).  Items may share a map; a point listed by two items
 * with the same `what` is written twice with the same bytes.  d_status entries past an item's count are not written.  Asynchronous
 * on `stream`, no synchronisation, no state, no workspace. */
struct slamit_points_batch_rec {
    int32_t nitems, n_maps, cap, reserved;
    const slamit_map_index* maps;      /* HOST [n_maps], device pointers inside; n_maps <= SLAMIT_LOCAL_MAP_MAX_MAPS */
    const slamit_point_index* pts;     /* HOST [n_maps], device pointers inside */
    const int32_t* d_item_map;         /* [nitems] */
    const int32_t* d_n;                /* [nitems] */
    const int32_t* d_what;             /* [nitems] */
    const int32_t* d_points;           /* [nitems][cap], cap <= SLAMIT_UPKEEP_MAX_POINTS */
    int32_t* d_status;                 /* [nitems][cap] out */
};
typedef struct slamit_points_batch_rec slamit_points_batch_rec;
int slamit_update_points_batch_dev(int device, const slamit_points_batch_rec* batch, void* stream);

/* MapPointCulling for one recent list (host pointers, synchronous).  Reads mp_bad of `map` and mp_found, mp_visible, mp_first_kf,
 * mp_nobs of `pts`.  verdict[n] and kept[n] in / out: verdict[j] for every j < n, kept[0 .. *n_kept) the kept slots in list order,
 * entries past the counts as the caller left them; *status out.  A null table or array, an entry outside [0, n_mp) fails with
 * SLAMIT_ERR_ARG, n above SLAMIT_UPKEEP_MAX_RECENT with SLAMIT_ERR_CAPACITY, before anything is launched. */
int slamit_map_point_culling(int device, const slamit_map_index* map, const slamit_point_index* pts, int32_t cur_id, int32_t monocular,
                             int32_t n, const int32_t* recent, uint8_t* verdict, int32_t* kept, int32_t* n_kept, int32_t* status);

/* The same for nlists recent lists, resident; lists may share a map (nothing is modified).  List f uses maps[d_list_map[f]] (outside
 * [0, n_maps): n_kept = 0 and SLAMIT_UPKEEP_BAD_SLOT).  An entry outside its table keeps its verdict byte, is not kept and sets
 * SLAMIT_UPKEEP_BAD_SLOT.  Asynchronous on `stream`, no state, no workspace. */
struct slamit_point_culling_batch_rec {
    int32_t nlists, n_maps, cap, reserved;
    const slamit_map_index* maps;      /* HOST [n_maps] */
    const slamit_point_index* pts;     /* HOST [n_maps] */
    const int32_t* d_list_map;         /* [nlists] */
    const int32_t* d_cur_id;           /* [nlists] mpCurrentKeyFrame->mnId */
    const int32_t* d_monocular;        /* [nlists] mbMonocular, 0 / 1 */
    const int32_t* d_n;                /* [nlists] entries, clamped to cap */
    const int32_t* d_recent;           /* [nlists][cap], cap <= SLAMIT_UPKEEP_MAX_RECENT */
    uint8_t* d_verdict;                /* [nlists][cap] in / out */
    int32_t* d_kept;                   /* [nlists][cap] in / out */
    int32_t* d_n_kept;                 /* [nlists] out */
    int32_t* d_status;                 /* [nlists] out */
};
typedef struct slamit_point_culling_batch_rec slamit_point_culling_batch_rec;
int slamit_map_point_culling_batch_dev(int device, const slamit_point_culling_batch_rec* batch, void* stream);

/* ---- Map edits: AddObservation, EraseObservation, SetBadFlag on the resident tables (local mapping) ----
 * MapPoint::AddObservation, ::EraseObservation and ::SetBadFlag (src/MapPoint.cc:104-174) with KeyFrame::AddMapPoint /
 * ::EraseMapPointMatch (src/KeyFrame.cc:215-243), applied to the tables of slamit_map_index and the columns of slamit_edit_index by
 * one call (csrc/map_edit.h states the walk).  A list of n edits is applied AS IF SEQUENTIALLY IN LIST ORDER; the
 * result equals the sequential walk exactly.  Every id is a slot (int32), -1 = none.
 *   SLAMIT_EDIT_ADD_OBS    kf already observes mp: nothing of the point changes.  Else (kf, idx, octave, weight) is appended to the
 *                          point's row and mp_nobs += weight (1, or 2 where mvuRight[idx] >= 0).  No bad test, as in the reference.
 *                          With SLAMIT_EDIT_MATCH also kf_mp[kf][idx] = mp, unconditional (KeyFrame::AddMapPoint).
 *   SLAMIT_EDIT_ERASE_OBS  with SLAMIT_EDIT_MATCH first kf_mp[kf][i] = -1 where the point holds kf at index i (EraseMapPointMatch).
 *                          Then, kf being an observer: mp_nobs -= its obs_weight, the entry goes; mp_ref_kf == kf becomes the remaining
 *                          observer with the smallest slot, or -1 with SLAMIT_EDIT_REF_END where the reference reads end();
 *                          mp_nobs <= 2 runs SET_BAD.  kf not an observer: nothing.
 *   SLAMIT_EDIT_SET_BAD    mp_bad = 1, kf_mp[k][i] = -1 for every observation (k, i) by index, the row is emptied; mp_nobs stays.
 * kf_mp[kf][idx] after the call is the value of the write with the largest list index.  The observation table is written OUT OF
 * PLACE: obs_ptr_out .. obs_weight_out are a packed CSR with ascending pointers from 0 that every reader of slamit_map_index takes
 * unchanged (a caller alternates two buffer sets); a new row is the old row's order with erased entries closed up and added ones
 * appended in list order.  mp_bad, mp_nobs, mp_ref_kf and kf_mp are rewritten IN PLACE.  MapPoint::Replace and KeyFrame::SetBadFlag's
 * spanning-tree walk are not here; appending a new keyframe's kf_mp row is slamit_map_grow_batch_dev's; Map::EraseMapPoint stays the caller's.
 * COST: as for the local map, the host form is for parity and tests; the gain is the resident form.
 * Kinds, flags, status bits (per point; BAD_SLOT and TABLE_OVERFLOW also per call) and ceilings: */
#define SLAMIT_EDIT_ADD_OBS 1
#define SLAMIT_EDIT_ERASE_OBS 2
#define SLAMIT_EDIT_SET_BAD 3
#define SLAMIT_EDIT_MATCH 1               /* flags: also the keyframe's side of the edit */
#define SLAMIT_EDIT_REF_END 1             /* the reference keyframe was erased as the last observer: mp_ref_kf = -1 */
#define SLAMIT_EDIT_EDIT_OVERFLOW 2       /* more than SLAMIT_EDIT_MAX_PER_POINT edits of this point: none of them was applied */
#define SLAMIT_EDIT_OBS_OVERFLOW 4        /* a row above SLAMIT_UPKEEP_MAX_OBS, or pushed past it: copied unchanged, none applied */
#define SLAMIT_EDIT_BAD_SLOT 8            /* device form: an edit or an observation with a slot outside its table was skipped */
#define SLAMIT_EDIT_TABLE_OVERFLOW 16     /* the new table needs more than obs_cap_out entries: NOTHING was written but n_obs_out */
#define SLAMIT_EDIT_MAX_PER_POINT 64      /* edits of one point per call: a bucket is ordered by one wavefront */
#define SLAMIT_EDIT_MAX_EDITS (1 << 20)   /* edits per list */

struct slamit_map_edit {
    int32_t kind, flags;
    int32_t mp, kf, idx;           /* the point, the keyframe, the keypoint index in it (ADD_OBS only) */
    uint8_t octave, weight;        /* ADD_OBS: what goes beside the new observation; weight is 1 or 2 */
    uint8_t pad[2];
};
typedef struct slamit_map_edit slamit_map_edit;

/* The arrays beside one slamit_map_index that the edits read and write.  Host pointers in the host form, device pointers in the batch
 * record.  Of the map record the call reads n_kf, n_mp, obs_ptr, obs_kf and kf_mp_ptr. */
struct slamit_edit_index {
    const int32_t* obs_idx;        /* beside obs_kf, read-only: may be the memory of slamit_point_index.obs_idx */
    const uint8_t* obs_octave;     /* beside obs_kf: as slamit_covis_index.obs_octave */
    const uint8_t* obs_weight;     /* beside obs_kf: as slamit_covis_index.obs_weight */
    uint8_t* mp_bad;               /* [n_mp] in / out: the memory the map record's mp_bad points to */
    int32_t* mp_nobs;              /* [n_mp] in / out: likewise the covis / point records' */
    int32_t* mp_ref_kf;            /* [n_mp] in / out */
    int32_t* kf_mp;                /* in / out: the memory the map record's kf_mp points to */
    int32_t* obs_ptr_out;          /* [n_mp + 1] out */
    int32_t* obs_kf_out;           /* [obs_cap_out] out, as the next three */
    int32_t* obs_idx_out;
    uint8_t* obs_octave_out;
    uint8_t* obs_weight_out;
    int32_t obs_cap_out;           /* entries the four output columns hold */
    int32_t reserved;
};
typedef struct slamit_edit_index slamit_edit_index;

/* One list over one map (host pointers, synchronous).  status_mp[n_mp] out: the status of every point (0 for one without edits);
 * touched[n_mp] in / out: the first *n_touched entries are the points of which an edit appended or removed an observation, in
 * ascending slot (the layout of slamit_points_batch_rec.d_points / d_n); *n_obs_out: the entries the new table needs; *status out.
 * Entries of the output columns past *n_obs_out and of touched past *n_touched are left as the caller filled them.  With
 * SLAMIT_EDIT_TABLE_OVERFLOW only *n_obs_out and *status are written.  A null table, a slot, index, kind or weight outside its range,
 * a CSR pointer array that does not ascend from 0 fails with SLAMIT_ERR_ARG, n above SLAMIT_EDIT_MAX_EDITS with SLAMIT_ERR_CAPACITY,
 * each with a message and before anything is launched. */
int slamit_map_edit_apply(int device, const slamit_map_index* map, const slamit_edit_index* edit, int32_t n, const slamit_map_edit* edits,
                          int32_t* status_mp, int32_t* touched, int32_t* n_touched, int32_t* n_obs_out, int32_t* status);

/* One list per map for n_maps maps, everything resident.  `maps` and `edit` are HOST arrays of records holding DEVICE pointers; map m
 * takes the first d_n[m] (clamped to [0, cap]) edits of d_edits[m].  mp_cap >= every n_mp; kfmp_cap >= every map's kf_mp_ptr[n_kf].
 * The device cannot be shown its tables first: an edit whose point lies outside the table is skipped (SLAMIT_EDIT_BAD_SLOT in
 * d_status[m]), an edit or an observation whose keyframe or index does is skipped, never dereferenced (the same bit in the point's
 * status).  Asynchronous on `stream`, no synchronisation, no state; the workspace is cleared on the stream by the call.
 * slamit_update_points_batch_dev can follow on the stream with d_touched / d_n_touched as its d_points / d_n (cap = mp_cap). */
struct slamit_map_edit_batch_rec {
    int32_t n_maps, cap, mp_cap, kfmp_cap;
    const slamit_map_index* maps;      /* HOST [n_maps], device pointers inside; n_maps <= SLAMIT_LOCAL_MAP_MAX_MAPS */
    const slamit_edit_index* edit;     /* HOST [n_maps], device pointers inside */
    const slamit_map_edit* d_edits;    /* [n_maps][cap], cap <= SLAMIT_EDIT_MAX_EDITS */
    const int32_t* d_n;                /* [n_maps] */
    int32_t* d_status_mp;              /* [n_maps][mp_cap] out */
    int32_t* d_touched;                /* [n_maps][mp_cap] in / out */
    int32_t* d_n_touched;              /* [n_maps] out */
    int32_t* d_n_obs_out;              /* [n_maps] out */
    int32_t* d_status;                 /* [n_maps] out */
    void* d_workspace;                 /* slamit_map_edit_workspace(n_maps, cap, mp_cap, kfmp_cap) bytes, 8-byte aligned */
    size_t workspace_bytes;
};
typedef struct slamit_map_edit_batch_rec slamit_map_edit_batch_rec;
size_t slamit_map_edit_workspace(int n_maps, int cap, int mp_cap, int kfmp_cap);
int slamit_map_edit_batch_dev(int device, const slamit_map_edit_batch_rec* batch, void* stream);

/* ---- MapPoint::Replace on the resident tables: the fuse lists of local mapping and loop closing ----
 * MapPoint::Replace (src/MapPoint.cc:183-221) as ORBmatcher::Fuse (ORBmatcher.cc:956-973), LoopClosing::SearchAndFuse (:614-625) and
 * ::CorrectLoop (:532-547) call it, with the AddObservation + AddMapPoint pair Fuse interleaves with it (csrc/map_replace.h states the
 * ops).  A list of n ops is applied AS IF SEQUENTIALLY IN LIST ORDER; the result equals the sequential walk exactly.
 *   SLAMIT_REPLACE_REPLACE  a = S, b = D.  a == b: nothing.  Else, for the entries (k, idx, octave, weight) of S's row in ascending
 *                           keyframe slot: D's row holds k: kf_mp[k][idx] = -1; otherwise kf_mp[k][idx] = D, the entry is appended to
 *                           D's row and mp_nobs[D] += weight.  S's row is emptied, mp_bad[S] = 1, mp_replaced[S] = D.
 *                           mp_found[D] += mp_found[S], mp_visible[D] += mp_visible[S] (int32 wrap), with the values held at that
 *                           moment.  No bad test on D; mp_nobs, mp_found, mp_visible of S stay; a replaced S can be replaced again.
 *   SLAMIT_REPLACE_ADD_OBS  a = the point, b = the keyframe, with idx, octave, weight: SLAMIT_EDIT_ADD_OBS | SLAMIT_EDIT_MATCH.
 * kf_mp[k][idx] after the call is the value of the write with the largest list index.  The observation table is written OUT OF PLACE
 * as for the map edits (a new row: the old order, moved-out entries gone, received ones appended as received); mp_bad, mp_nobs,
 * mp_found, mp_visible, mp_replaced and kf_mp are rewritten IN PLACE.  Map::EraseMapPoint of the replaced points and
 * ComputeDistinctiveDescriptors of the receivers (slamit_update_points_batch_dev over `touched`) are the caller's next steps.
 * ALL-OR-NOTHING: points are coupled, so each ceiling refuses the whole call; then nothing is written but the status (and n_obs_out
 * with TABLE_OVERFLOW).  Replace never creates an observation, so obs_cap_out = the old table + the number of ADD_OBS ops always
 * suffices.  Status bits of the call, the first overflow that holds being the one reported, and ceilings: */
#define SLAMIT_REPLACE_REPLACE 1
#define SLAMIT_REPLACE_ADD_OBS 2
#define SLAMIT_REPLACE_OP_OVERFLOW 1      /* a point is named by more than SLAMIT_REPLACE_MAX_PER_POINT ops */
#define SLAMIT_REPLACE_OBS_OVERFLOW 2     /* an involved row above SLAMIT_UPKEEP_MAX_OBS on input, or pushed past it */
#define SLAMIT_REPLACE_TABLE_OVERFLOW 4   /* the new table needs more than obs_cap_out entries: n_obs_out says how many */
#define SLAMIT_REPLACE_BAD_SLOT 8         /* device form: an op or an observation with a slot outside its table was skipped */
#define SLAMIT_REPLACE_MAX_OPS 16384      /* ops per list */
#define SLAMIT_REPLACE_MAX_PER_POINT 64   /* ops naming one point, as either side */
#define SLAMIT_CHECK_REPLACED_MAX_N 65536 /* entries of one frame's list of slamit_check_replaced */

struct slamit_map_replace {
    int32_t kind;
    int32_t a, b;                  /* REPLACE: S and D.  ADD_OBS: the point and the keyframe */
    int32_t idx;                   /* ADD_OBS: the keypoint index in the keyframe */
    uint8_t octave, weight;        /* ADD_OBS: what goes beside the new observation; weight is 1 or 2 */
    uint8_t pad[2];
};
typedef struct slamit_map_replace slamit_map_replace;

/* The arrays beside one slamit_map_index that the ops read and write: the very memory the map, covis and point records name.  Host
 * pointers in the host form, device pointers in the batch record.  Of the map record the call reads n_kf, n_mp, obs_ptr, obs_kf and
 * kf_mp_ptr. */
struct slamit_replace_index {
    const int32_t* obs_idx;        /* beside obs_kf, read-only */
    const uint8_t* obs_octave;
    const uint8_t* obs_weight;
    uint8_t* mp_bad;               /* [n_mp] in / out */
    int32_t* mp_nobs;              /* [n_mp] in / out */
    int32_t* mp_found;             /* [n_mp] in / out: mnFound, the memory of slamit_point_index.mp_found */
    int32_t* mp_visible;           /* [n_mp] in / out: mnVisible */
    int32_t* mp_replaced;          /* [n_mp] in / out: mpReplaced, -1 for none */
    int32_t* kf_mp;                /* in / out */
    int32_t* obs_ptr_out;          /* [n_mp + 1] out */
    int32_t* obs_kf_out;           /* [obs_cap_out] out, as the next three */
    int32_t* obs_idx_out;
    uint8_t* obs_octave_out;
    uint8_t* obs_weight_out;
    int32_t obs_cap_out;
    int32_t reserved;
};
typedef struct slamit_replace_index slamit_replace_index;

/* One list over one map (host pointers, synchronous).  moved[n] / erased[n] in / out: the entries op i appended to its target and the
 * ones it dropped (ADD_OBS: 1 or 0, and 0); touched[n_mp] in / out: the first *n_touched entries are the points that received an
 * observation, in ascending slot (the layout of slamit_points_batch_rec.d_points / d_n); *n_obs_out in / out; *status out.  Entries
 * past the counts are left as the caller filled them; with an overflow bit everything but *status (and *n_obs_out for
 * TABLE_OVERFLOW) is.  A null table, a slot, index, kind or weight outside its range, a CSR pointer array that does not ascend from 0
 * fails with SLAMIT_ERR_ARG, n above SLAMIT_REPLACE_MAX_OPS with SLAMIT_ERR_CAPACITY, each with a message and before anything is
 * launched. */
int slamit_map_replace_apply(int device, const slamit_map_index* map, const slamit_replace_index* index, int32_t n, const slamit_map_replace* ops,
                             int32_t* moved, int32_t* erased, int32_t* touched, int32_t* n_touched, int32_t* n_obs_out, int32_t* status);

/* One list per map for n_maps maps, everything resident.  `maps` and `index` are HOST arrays of records holding DEVICE pointers; map
 * m takes the first d_n[m] (clamped to [0, cap]) ops of d_ops[m].  The device cannot be shown its tables first: an op with a point,
 * keyframe, index or weight outside its range is skipped whole, never dereferenced; an observation whose (k, idx) lies outside kf_mp
 * is carried along without its kf_mp write; both set SLAMIT_REPLACE_BAD_SLOT in d_status[m].  Asynchronous on `stream`, no
 * synchronisation, no state; the head of the workspace is cleared on the stream by the call.  One workgroup per map walks the list in
 * rounds of independent ops: a chain of dependent ops costs a round each.
 * WORKSPACE, with S = mp_cap + 1, ninv = min(2 cap, mp_cap) and every array rounded up to 16 bytes, per map:
 *   8 kfmp_cap + 32 + 4 (6 S + 2 (ceil(S / 256) + 1)) + 4 * 7 cap + 4 (1 + 7) ninv + 10 * SLAMIT_UPKEEP_MAX_OBS * ninv bytes
 * -- the kf_mp words, the status words, six rows over the points, the scan's sums, buckets / predecessors / stamps / counts, and a
 * working row with its columns per involved point. */
struct slamit_map_replace_batch_rec {
    int32_t n_maps, cap, mp_cap, kfmp_cap;
    const slamit_map_index* maps;      /* HOST [n_maps], device pointers inside; n_maps <= SLAMIT_LOCAL_MAP_MAX_MAPS */
    const slamit_replace_index* index; /* HOST [n_maps], device pointers inside */
    const slamit_map_replace* d_ops;   /* [n_maps][cap], cap <= SLAMIT_REPLACE_MAX_OPS */
    const int32_t* d_n;                /* [n_maps] */
    int32_t* d_moved;                  /* [n_maps][cap] in / out */
    int32_t* d_erased;                 /* [n_maps][cap] in / out */
    int32_t* d_touched;                /* [n_maps][mp_cap] in / out */
    int32_t* d_n_touched;              /* [n_maps] in / out */
    int32_t* d_n_obs_out;              /* [n_maps] in / out */
    int32_t* d_status;                 /* [n_maps] out */
    void* d_workspace;                 /* slamit_map_replace_workspace(n_maps, cap, mp_cap, kfmp_cap) bytes, 8-byte aligned */
    size_t workspace_bytes;
};
typedef struct slamit_map_replace_batch_rec slamit_map_replace_batch_rec;
size_t slamit_map_replace_workspace(int n_maps, int cap, int mp_cap, int kfmp_cap);
int slamit_map_replace_batch_dev(int device, const slamit_map_replace_batch_rec* batch, void* stream);

/* Tracking::CheckReplacedInLastFrame (src/Tracking.cc:959-974), the reader of mp_replaced: every entry p >= 0 of a frame's point list
 * with mp_replaced[p] >= 0 becomes mp_replaced[p] -- one hop, as the reference follows one.  Host form: frame_mp[n] in / out, *status
 * out; an entry outside [-1, n_mp) fails with SLAMIT_ERR_ARG, n above SLAMIT_CHECK_REPLACED_MAX_N with SLAMIT_ERR_CAPACITY, before a
 * launch.  Resident form: frame f lists d_n[f] (clamped to cap) entries over map d_frame_map[f]; an entry outside the table is left
 * alone and sets SLAMIT_REPLACE_BAD_SLOT in d_status[f] (a map index outside [0, n_maps): the frame is left alone, the same bit).
 * Asynchronous on `stream`, no state, no workspace. */
int slamit_check_replaced(int device, int32_t n_mp, const int32_t* mp_replaced, int32_t n, int32_t* frame_mp, int32_t* status);
struct slamit_check_replaced_batch_rec {
    int32_t nframes, n_maps, cap, reserved;
    const int32_t* n_mp;                   /* HOST [n_maps] */
    const int32_t* const* d_mp_replaced;   /* HOST [n_maps] of device pointers, n_maps <= SLAMIT_LOCAL_MAP_MAX_MAPS */
    const int32_t* d_frame_map;            /* [nframes] */
    const int32_t* d_n;                    /* [nframes] */
    int32_t* d_frame_mp;                   /* [nframes][cap] in / out, cap <= SLAMIT_CHECK_REPLACED_MAX_N */
    int32_t* d_status;                     /* [nframes] out */
};
typedef struct slamit_check_replaced_batch_rec slamit_check_replaced_batch_rec;
int slamit_check_replaced_batch_dev(int device, const slamit_check_replaced_batch_rec* batch, void* stream);

/* ---- The tail of ORBmatcher::Fuse on the resident tables: an op that picks the replace direction ----
 * ORBmatcher::Fuse (src/ORBmatcher.cc:853, :955-975) looks at pKF->GetMapPoint(bestIdx) and at both points' Observations() AT THAT
 * MOMENT and replaces one way, the other way, or adds the observation (csrc/map_fuse.h states the op).  A list of n
 * ops in slamit_map_replace's record, of kinds SLAMIT_REPLACE_REPLACE, SLAMIT_REPLACE_ADD_OBS (both as above) and SLAMIT_FUSE_FUSE,
 * is applied AS IF SEQUENTIALLY IN LIST ORDER; the result equals the sequential walk exactly.
 *   SLAMIT_FUSE_FUSE  a = P, b = the keyframe k, idx = the matched keypoint, octave and weight what goes beside a new observation
 *                     (weight 2 where mvuRight[idx] >= 0).  Over the state as the earlier ops left it, in this order:
 *                     idx < 0: OUT_NOMATCH, nothing else is read.  mp_bad[P]: OUT_SKIP_BAD.  P's row holds k: OUT_SKIP_IN_KF.
 *                     Q = kf_mp[k][idx]; Q == -1: SLAMIT_REPLACE_ADD_OBS of (P, k, idx, octave, weight), OUT_ADDED.  mp_bad[Q]: nothing,
 *                     OUT_OCCUPANT_BAD.  mp_nobs[Q] > mp_nobs[P]: REPLACE(P -> Q), OUT_P_REPLACED; otherwise REPLACE(Q -> P),
 *                     OUT_Q_REPLACED (P == Q, on tables that hold one (k, idx) under two points, is Replace's a == b: nothing).
 * outcome[i] is that code, SLAMIT_FUSE_OUT_PLAIN for the other two kinds; *n_fused counts OUT_ADDED, OUT_OCCUPANT_BAD, OUT_P_REPLACED
 * and OUT_Q_REPLACED, the reference's return value.  Tables, moved / erased, touched, n_obs_out: as slamit_map_replace_apply.
 * ALL-OR-NOTHING as there; there is NO per-point ceiling.  obs_cap_out = the old table + the number of ADD_OBS and FUSE ops always
 * suffices.  Status bits (the values of SLAMIT_REPLACE_*), the first overflow that holds being the one reported: */
#define SLAMIT_FUSE_FUSE 3
#define SLAMIT_FUSE_OUT_PLAIN 0
#define SLAMIT_FUSE_OUT_NOMATCH 1
#define SLAMIT_FUSE_OUT_SKIP_BAD 2
#define SLAMIT_FUSE_OUT_SKIP_IN_KF 3
#define SLAMIT_FUSE_OUT_ADDED 4
#define SLAMIT_FUSE_OUT_OCCUPANT_BAD 5
#define SLAMIT_FUSE_OUT_P_REPLACED 6
#define SLAMIT_FUSE_OUT_Q_REPLACED 7
#define SLAMIT_FUSE_OBS_OVERFLOW 2        /* an involved row above SLAMIT_UPKEEP_MAX_OBS on input, or pushed past it */
#define SLAMIT_FUSE_TABLE_OVERFLOW 4      /* the new table needs more than obs_cap_out entries: n_obs_out says how many */
#define SLAMIT_FUSE_BAD_SLOT 8            /* device form: an op or an observation with a slot outside its table was skipped */
#define SLAMIT_FUSE_MAX_OPS 16384         /* ops per list */

/* One list over one map (host pointers, synchronous).  outcome[n], moved[n], erased[n], touched[n_mp], *n_touched, *n_fused,
 * *n_obs_out in / out, *status out: entries past the counts are left as the caller filled them; with an overflow bit everything but
 * *status (and *n_obs_out for TABLE_OVERFLOW) is.  What slamit_map_replace_apply refuses is refused here (a FUSE op with idx < 0 is
 * not read further), and so is an entry of kf_mp outside [-1, n_mp); n above SLAMIT_FUSE_MAX_OPS fails with SLAMIT_ERR_CAPACITY;
 * each with a message and before anything is launched. */
int slamit_map_fuse_apply(int device, const slamit_map_index* map, const slamit_replace_index* index, int32_t n, const slamit_map_replace* ops,
                          int32_t* outcome, int32_t* moved, int32_t* erased, int32_t* touched, int32_t* n_touched, int32_t* n_fused, int32_t* n_obs_out,
                          int32_t* status);

/* One list per map for n_maps maps, everything resident; records as slamit_map_replace_batch_dev takes them.  An op with idx >= 0
 * whose point, keyframe, index or weight lies outside its range is skipped whole, never dereferenced, and so is a FUSE op that meets
 * an occupant outside [-1, n_mp); an observation whose (k, idx) lies outside kf_mp is carried along without its kf_mp write; all set
 * SLAMIT_FUSE_BAD_SLOT in d_status[m].  Asynchronous on `stream`, no synchronisation, no state; the head of the workspace is cleared
 * on the stream by the call.  One wavefront per map walks the list in order.  ZERO-INITIALISE the record.
 * WORKSPACE, with S = mp_cap + 1, ninv = min(2 cap, mp_cap) and every array rounded up to 16 bytes, per map:
 *   32 + 4 (4 S + 2 (ceil(S / 256) + 1)) + 4 * 3 cap + 4 + 4 kfmp_cap + 4 (1 + 7) ninv + 10 * SLAMIT_UPKEEP_MAX_OBS * ninv bytes
 * -- the status words, four rows over the points, the scan's sums, outcome / moved / erased, the count, the working image of kf_mp,
 * and a working row with its columns per involved point. */
struct slamit_map_fuse_batch_rec {
    int32_t n_maps, cap, mp_cap, kfmp_cap;
    const slamit_map_index* maps;      /* HOST [n_maps], device pointers inside; n_maps <= SLAMIT_LOCAL_MAP_MAX_MAPS */
    const slamit_replace_index* index; /* HOST [n_maps], device pointers inside */
    const slamit_map_replace* d_ops;   /* [n_maps][cap], cap <= SLAMIT_FUSE_MAX_OPS */
    const int32_t* d_n;                /* [n_maps] */
    int32_t* d_outcome;                /* [n_maps][cap] in / out */
    int32_t* d_moved;                  /* [n_maps][cap] in / out */
    int32_t* d_erased;                 /* [n_maps][cap] in / out */
    int32_t* d_touched;                /* [n_maps][mp_cap] in / out */
    int32_t* d_n_touched;              /* [n_maps] in / out */
    int32_t* d_n_fused;                /* [n_maps] in / out */
    int32_t* d_n_obs_out;              /* [n_maps] in / out */
    int32_t* d_status;                 /* [n_maps] out */
    void* d_workspace;                 /* slamit_map_fuse_workspace(n_maps, cap, mp_cap, kfmp_cap) bytes, 8-byte aligned */
    size_t workspace_bytes;
};
typedef struct slamit_map_fuse_batch_rec slamit_map_fuse_batch_rec;
size_t slamit_map_fuse_workspace(int n_maps, int cap, int mp_cap, int kfmp_cap);
int slamit_map_fuse_batch_dev(int device, const slamit_map_fuse_batch_rec* batch, void* stream);

/* The FUSE ops of a guided search, written where slamit_map_fuse_batch_dev reads them: one lane per query, no workspace, asynchronous
 * on `stream`.  Target f (one frame of the search: the queries are map points projected into one keyframe) fills the slice
 * [d_base[f], d_base[f] + q_cap) of map d_frame_map[f]'s list: query q < d_m[f] becomes {FUSE, a = d_query_point[f][q], b =
 * d_frame_kf[f], idx = d_match_kp[f][q] (-1 stays -1), octave = d_kps_un[f][idx].octave, weight = 2 where d_kp_ur is given and
 * d_kp_ur[f][idx] >= 0, else 1}; a slot past d_m[f] becomes a no-match op, so slices lie back to back without compaction.  d_n[m] =
 * the end of map m's last slice (0 for a map without one).  A target whose map lies outside [0, n_maps) or whose slice does not fit
 * in [0, cap) writes nothing and sets SLAMIT_FUSE_BAD_SLOT in d_status[f].  ZERO-INITIALISE the record. */
struct slamit_fuse_list_batch_rec {
    int32_t nframes, n_maps, kp_cap, q_cap, cap, reserved;
    const int32_t* d_m;                /* [nframes] queries per target */
    const int32_t* d_match_kp;         /* [nframes][q_cap]: what the guided search wrote */
    const int32_t* d_query_point;      /* [nframes][q_cap]: the slot of query q's map point */
    const slamit_kp* d_kps_un;         /* [nframes][kp_cap] (octave is read) */
    const float* d_kp_ur;              /* [nframes][kp_cap] or NULL: mvuRight */
    const int32_t* d_frame_map;        /* [nframes] */
    const int32_t* d_frame_kf;         /* [nframes]: the target's keyframe slot */
    const int32_t* d_base;             /* [nframes]: where the target's slice begins in its map's list */
    slamit_map_replace* d_ops;         /* [n_maps][cap] out, cap <= SLAMIT_FUSE_MAX_OPS */
    int32_t* d_n;                      /* [n_maps] out */
    int32_t* d_status;                 /* [nframes] out */
};
typedef struct slamit_fuse_list_batch_rec slamit_fuse_list_batch_rec;
int slamit_fuse_list_batch_dev(int device, const slamit_fuse_list_batch_rec* batch, void* stream);

/* ---- KeyFrame::SetBadFlag on the resident tables: graph rows and the spanning tree ----
 * KeyFrame::SetBadFlag (src/KeyFrame.cc:460-552) with EraseConnection / UpdateBestCovisibles (:560-574, :142-161) and ChangeParent /
 * AddChild / EraseChild (:388-405) over the tables of slamit_map_index and the arrays of slamit_tree_index (csrc/kf_erase.h states the
 * walk).  A list of n ops is applied AS IF SEQUENTIALLY IN LIST ORDER; the result equals the sequential walk exactly.
 *   SLAMIT_KF_ERASE_SET_PARENT  kf = c, parent = p: kf_parent[c] = p, and c enters p's children row (ascending slot) unless it is
 *                               there.  No bad test, no erase from an old parent.  The caller issues it when
 *                               slamit_update_connections returned parent >= 0.
 *   SLAMIT_KF_ERASE_SET_BAD     kf = k.  k == origin_kf: nothing (ORIGIN).  kf_not_erase[k]: kf_to_be_erased[k] = 1, nothing else
 *                               (NOT_ERASE).  kf_parent[k] == -1, where the reference dereferences a null parent: nothing (NO_PARENT).
 *                               Else: every j of k's cw row whose own cw row holds k loses that entry, its ord row becomes the sort of
 *                               its whole remaining cw row and kf_best[j] its first ten (a j whose row lacks k stays byte for byte);
 *                               one SLAMIT_EDIT_ERASE_OBS edit without MATCH per non-null entry of k's kf_mp row is EMITTED into
 *                               `edits`, by op and then by keypoint index, from the kf_mp the call was given; cw_n[k] = ord_n[k] = 0,
 *                               kf_best[k] all -1; the spanning tree is repaired as the reference repairs it (the pair of child and
 *                               candidate with the strictly largest GetWeight, first in row order, again and again; the children left
 *                               over go to kf_parent[k] and stay in k's row); k leaves its parent's row; kf_bad[k] = 1; kf_parent[k] stays.
 * The point side of SetBadFlag is the emitted list handed to slamit_map_edit_batch_dev as the next call on the stream (cap = edit_cap,
 * d_n = d_n_edits_out).  IN PLACE: kf_bad, kf_parent, kf_to_be_erased and the seven graph arrays, the very memory the map and covis
 * records point to; a changed graph row is rewritten up to its new count.  OUT OF PLACE: the children table, a packed CSR ascending
 * from 0 that slamit_map_index takes unchanged (a caller alternates two buffer sets); a row no op touched is copied.
 * GATES: the new children table above child_cap_out entries, or more edits than edit_cap: NOTHING is written but n_edits_out,
 * n_child_out (the two needs) and the call's status.  The old table plus one entry per SET_PARENT op and per child of a SET_BAD keyframe
 * always suffices.  mTcp (the library holds no poses: read kf_parent[k]), Map::EraseKeyFrame, KeyFrameDatabase::erase
 * (slamit_kfdb_erase), SetErase() and the loop edges stay the caller's.
 * Kinds, status bits (per op: the first five; per call: BAD_SLOT, ROW_OVERFLOW and the two gates) and ceilings: */
#define SLAMIT_KF_ERASE_SET_PARENT 1
#define SLAMIT_KF_ERASE_SET_BAD 2
#define SLAMIT_KF_ERASE_ORIGIN 1           /* SET_BAD of origin_kf: nothing was done */
#define SLAMIT_KF_ERASE_NOT_ERASE 2        /* kf_not_erase: kf_to_be_erased = 1, nothing else */
#define SLAMIT_KF_ERASE_NO_PARENT 4        /* kf_parent == -1 on a keyframe that is not the origin: the op was skipped whole */
#define SLAMIT_KF_ERASE_BAD_SLOT 8         /* device form: an op or a table entry with a slot outside its table was skipped */
#define SLAMIT_KF_ERASE_ROW_OVERFLOW 16    /* more than SLAMIT_KF_ERASE_MAX_CHILD children: the op was skipped whole */
#define SLAMIT_KF_ERASE_CHILD_OVERFLOW 32  /* the new children table needs more than child_cap_out entries: n_child_out says how many */
#define SLAMIT_KF_ERASE_EDIT_OVERFLOW 64   /* more edits than edit_cap: n_edits_out says how many */
#define SLAMIT_KF_ERASE_MAX_OPS 1024       /* ops per list: one workgroup walks them */
#define SLAMIT_KF_ERASE_MAX_CHILD 1024     /* children of one SET_BAD keyframe: the row and the candidates live in LDS */

struct slamit_kf_op {
    int32_t kind;
    int32_t kf;                    /* SET_PARENT: the child.  SET_BAD: the keyframe */
    int32_t parent;                /* SET_PARENT: the new parent */
    int32_t reserved;
};
typedef struct slamit_kf_op slamit_kf_op;

/* The arrays beside one slamit_map_index that the ops read and write.  Host pointers in the host form, device pointers in the batch
 * record.  Of the map record the call reads n_kf, n_mp, kf_mp_ptr, kf_mp, kf_child_ptr and kf_child. */
struct slamit_tree_index {
    int32_t row_cap;               /* entries per graph row, <= SLAMIT_COVIS_MAX_ROW: slamit_covis_index.row_cap */
    int32_t origin_kf;             /* slot of the keyframe with mnId 0, -1 = none */
    const uint8_t* kf_not_erase;   /* [n_kf] mbNotErase */
    uint8_t* kf_bad;               /* [n_kf] in / out: the memory the map record's kf_bad points to */
    int32_t* kf_parent;            /* [n_kf] in / out: likewise kf_parent */
    uint8_t* kf_to_be_erased;      /* [n_kf] in / out: mbToBeErased */
    int32_t *cw_kf, *cw_w, *cw_n;      /* in / out: the memory of slamit_covis_index */
    int32_t *ord_kf, *ord_w, *ord_n;
    int32_t* kf_best;              /* in / out, nullable */
    int32_t* child_ptr_out;        /* [n_kf + 1] out */
    int32_t* child_out;            /* [child_cap_out] out */
    int32_t child_cap_out;         /* entries child_out holds */
    int32_t reserved;
};
typedef struct slamit_tree_index slamit_tree_index;

/* One list over one map (host pointers, synchronous).  op_status[n] in / out; edits[edit_cap] in / out: the first *n_edits_out are
 * written; *n_edits_out, *n_child_out and *status out.  Entries past the counts are left as the caller filled them; with a gate's bit
 * everything but the two needs and *status is.  A null table, a slot or a row count outside its range, a kind outside 1..2, a CSR
 * pointer array that does not ascend from 0 or a children row that does not ascend fails with SLAMIT_ERR_ARG, n above
 * SLAMIT_KF_ERASE_MAX_OPS with SLAMIT_ERR_CAPACITY, each with a message and before anything is launched. */
int slamit_kf_erase_apply(int device, const slamit_map_index* map, const slamit_tree_index* tree, int32_t n, const slamit_kf_op* ops,
                          int32_t* op_status, int32_t edit_cap, slamit_map_edit* edits, int32_t* n_edits_out, int32_t* n_child_out, int32_t* status);

/* One list per map for n_maps maps, everything resident.  `maps` and `tree` are HOST arrays of records holding DEVICE pointers; map m
 * takes the first d_n[m] (clamped to [0, cap]) ops of d_ops[m].  kf_cap >= every n_kf, row_cap >= every map's row_cap, child_cap >=
 * every map's kf_child_ptr[n_kf].  The device cannot be shown its tables first: an op whose keyframe or parent lies outside the table
 * is skipped whole, a neighbour or child outside it is skipped, never dereferenced; both set SLAMIT_KF_ERASE_BAD_SLOT.  Asynchronous
 * on `stream`, no synchronisation, no state; the head of the workspace is cleared on the stream by the call.  One workgroup per map
 * walks the list; the parallelism is inside an op.
 * WORKSPACE, every array rounded up to 16 bytes, per map: 16 + 3 kf_cap bytes of flags, 4 (4 row_cap + 15) kf_cap + 4 for the working
 * graph, columns, list heads and new pointers, 8 (child_cap + cap * min(SLAMIT_KF_ERASE_MAX_CHILD, kf_cap)) for the children lists,
 * 12 cap + 4 for the ops. */
struct slamit_kf_erase_batch_rec {
    int32_t n_maps, cap, kf_cap, row_cap, child_cap, edit_cap;
    const slamit_map_index* maps;      /* HOST [n_maps], device pointers inside; n_maps <= SLAMIT_LOCAL_MAP_MAX_MAPS */
    const slamit_tree_index* tree;     /* HOST [n_maps], device pointers inside */
    const slamit_kf_op* d_ops;         /* [n_maps][cap], cap <= SLAMIT_KF_ERASE_MAX_OPS */
    const int32_t* d_n;                /* [n_maps] */
    int32_t* d_op_status;              /* [n_maps][cap] in / out */
    slamit_map_edit* d_edits;          /* [n_maps][edit_cap] in / out: slamit_map_edit_batch_rec.d_edits with cap = edit_cap */
    int32_t* d_n_edits_out;            /* [n_maps] out: slamit_map_edit_batch_rec.d_n */
    int32_t* d_n_child_out;            /* [n_maps] out */
    int32_t* d_status;                 /* [n_maps] out */
    void* d_workspace;                 /* slamit_kf_erase_workspace(n_maps, cap, kf_cap, row_cap, child_cap) bytes, 8-byte aligned */
    size_t workspace_bytes;
};
typedef struct slamit_kf_erase_batch_rec slamit_kf_erase_batch_rec;
size_t slamit_kf_erase_workspace(int n_maps, int cap, int kf_cap, int row_cap, int child_cap);
int slamit_kf_erase_batch_dev(int device, const slamit_kf_erase_batch_rec* batch, void* stream);

/* ---- Map growth on the resident tables: new keyframes, new map points, the association loop of ProcessNewKeyFrame ----
 * KeyFrame::KeyFrame(Frame&, ...) with Map::AddKeyFrame, MapPoint::MapPoint(Pos, pRefKF, pMap) with its AddObservation / AddMapPoint /
 * Map::AddMapPoint (src/LocalMapping.cc:486-500, src/Tracking.cc:1376-1383, :718-723, :875-891) and the loop of
 * LocalMapping::ProcessNewKeyFrame (:156-175), appended IN PLACE to tables that have room (csrc/map_grow.h states the walk; DESIGN.md
 * §33).  A list of ops is applied AS IF SEQUENTIALLY IN LIST ORDER; the result equals the sequential walk exactly.  Every id is a slot.
 *   SLAMIT_GROW_NEW_KF     kf = the next free slot (n_kf + the NEW_KF ops applied before it), src = a frame record, kf_id = mnId (carried,
 *                          not stored).  Appends kf_mp_ptr[kf + 1], the kf_mp row as mvpMapPoints is copied (bad points stay), kf_octave,
 *                          kf_desc, kf_depth (-1 from a source without depth), kf_bad = 0, kf_parent = -1, kf_to_be_erased = 0,
 *                          kf_not_erase = 0, kf_th_depth, a kf_best row of -1, cw_n = ord_n = 0, kf_child_ptr[kf + 1] = kf_child_ptr[kf] and
 *                          kf_center = -Rcw^T tcw in float, each component ((R0j t0 + R1j t1) + R2j t2) negated (OpenCV's own evaluation
 *                          of that line is unpinned, as for the upkeep calls).
 *   SLAMIT_GROW_NEW_POINT  kf = ref, kf_id = first_kf_id, observers (kf_a, idx_a, weight_a) and (kf_b, idx_b, weight_b), kf_b = -1 for the
 *                          one-observer stereo point.  The point exists iff cand == -1 (position pos) or d_cand_status[cand] == 0
 *                          (position d_cand_x3d[3 cand ..], the layout of slamit_triangulate_result), so the list can be written before
 *                          the triangulation's verdicts exist; otherwise SLAMIT_GROW_OP_REJECTED.  Accepted points take slots n_mp, n_mp +
 *                          1, ... in list order with mp_pos, mp_normal = 0, both distances 0, mp_bad = 0, mp_nobs = 0, mp_ref_kf = ref,
 *                          mp_found = mp_visible = 1, mp_first_kf, mp_replaced = -1, mp_desc = 0 and an empty row of obs_ptr.  For a then
 *                          b: kf_mp[kf][idx] = the slot, unconditional (the last op of the list that names an entry wins), and one
 *                          SLAMIT_EDIT_ADD_OBS edit without MATCH is EMITTED into `edits` (octave from kf_octave).  SLAMIT_GROW_RECENT
 *                          appends the slot to the recent list (CreateNewMapPoints sets it, Tracking's stereo points do not).
 *   SLAMIT_GROW_ASSOCIATE  kf, src (its row has src's n_kp entries).  Over kf_mp[kf] as the ops before left it, in keypoint order: -1 and
 *                          bad points are skipped; a point for which IsInKeyFrame(kf) holds at that moment -- its row of the table the
 *                          call was given holds kf, or an ADD_OBS(p, kf) was emitted earlier in this call -- goes to the recent list; any
 *                          other emits ADD_OBS(p, kf, i, kf_octave, 2 where src.uright[i] >= 0 else 1).
 * The point side of every observation is the emitted list handed to slamit_map_edit_batch_dev as the next call on the stream (cap =
 * edit_cap, d_n = d_n_edits_out); its `touched` are the points UpdateNormalAndDepth / ComputeDistinctiveDescriptors is due for.  The
 * call READS THE TABLES AS THEY ARE: edits emitted by an earlier grow call must have been applied (and the edit index swapped) before a
 * call that depends on them.  UpdateConnections and SET_PARENT are the existing calls.
 * THE INERT TAIL: of the P NEW_POINT ops of a list A are accepted (d_n_new); slots n_mp + A .. n_mp + P - 1 become mp_bad = 1, mp_nobs =
 * 0, mp_ref_kf = mp_replaced = -1, empty rows, everything else 0, so records with n_kf + the NEW_KF ops and n_mp + P are valid at once,
 * without a host visit; a caller that later reads A may shrink to n_mp + A.  The call moves no record's n_kf / n_mp: the caller does.
 * ONE GATE per map, decided before anything is written, from the list and the frame records alone (upper bounds): kf_cap against n_kf +
 * the NEW_KF ops; mp_cap against n_mp + P; kfmp_cap against kf_mp_ptr[n_kf] + their n_kp; edit_cap against 2 P + the n_kp of the
 * ASSOCIATE ops; recent_cap against n_recent + the RECENT ops + that sum.  A map that fails one, names a frame record above
 * SLAMIT_FRAME_MAX_KP or has d_n above cap gets d_need and a status bit per failure and NOTHING else; its neighbours are written.
 * Not here: slot recycling and Map::EraseMapPoint, the temporal points of UpdateLastFrame, KeyFrameDatabase::add (slamit_kfdb_add_dev),
 * ComputeBoW (slamit_voc_transform_batch_dev).  Kinds, flag, op codes, status bits per map and ceilings: */
#define SLAMIT_GROW_NEW_KF 1
#define SLAMIT_GROW_NEW_POINT 2
#define SLAMIT_GROW_ASSOCIATE 3
#define SLAMIT_GROW_RECENT 1               /* flags of a NEW_POINT op */
#define SLAMIT_GROW_OP_REJECTED (-1)       /* d_op_status: the candidate's status was not 0 */
#define SLAMIT_GROW_OP_BAD (-2)            /* d_op_status: a slot, index, weight, kind or frame record outside its range: skipped whole, never dereferenced */
#define SLAMIT_GROW_KF_OVERFLOW 1
#define SLAMIT_GROW_MP_OVERFLOW 2
#define SLAMIT_GROW_KFMP_OVERFLOW 4
#define SLAMIT_GROW_EDIT_OVERFLOW 8
#define SLAMIT_GROW_RECENT_OVERFLOW 16
#define SLAMIT_GROW_KP_OVERFLOW 32         /* an op names a frame record with more than SLAMIT_FRAME_MAX_KP keypoints */
#define SLAMIT_GROW_OPS_OVERFLOW 64        /* d_n above cap */
#define SLAMIT_GROW_BAD_SLOT 128           /* an op was skipped (SLAMIT_GROW_OP_BAD), or an entry of a row outside the points that exist was skipped */
#define SLAMIT_GROW_REFUSED 127            /* with one of these bits nothing was written but d_need and d_status */
#define SLAMIT_GROW_MAX_OPS 65536          /* ops per list (cap); edit_cap is at most SLAMIT_EDIT_MAX_EDITS, recent_cap at most SLAMIT_UPKEEP_MAX_RECENT */
#define SLAMIT_GROW_MAX_FRAMES 16          /* frame records per call: they travel as the kernel's argument */
#define SLAMIT_GROW_NEEDS 5                /* d_need per map: keyframes, points, keypoints, edits, recent entries */

struct slamit_grow_op {
    int32_t kind, flags;
    int32_t kf;                    /* NEW_KF / ASSOCIATE: the keyframe.  NEW_POINT: ref */
    int32_t src;                   /* NEW_KF / ASSOCIATE: the frame record */
    int32_t kf_id;                 /* NEW_KF: mnId.  NEW_POINT: first_kf_id */
    int32_t cand;                  /* NEW_POINT: the candidate, -1 = accepted with pos */
    int32_t kf_a, idx_a, kf_b, idx_b;
    uint8_t weight_a, weight_b;    /* 1, or 2 where mvuRight[idx] >= 0 */
    uint8_t pad[2];
    float pos[3];                  /* NEW_POINT with cand = -1 */
};
typedef struct slamit_grow_op slamit_grow_op;

/* A frame that becomes a keyframe: DEVICE pointers in a HOST record. */
struct slamit_grow_frame {
    int32_t n_kp;                  /* <= SLAMIT_FRAME_MAX_KP */
    float th_depth;                /* mThDepth */
    const int32_t* frame_mp;       /* [n_kp] mvpMapPoints as slots, the layout of slamit_local_map_batch_rec.d_frame_mp */
    const uint8_t* octave;         /* [n_kp] mvKeysUn[i].octave */
    const uint8_t* desc;           /* [n_kp][32], 16-byte aligned */
    const float* depth;            /* [n_kp] mvDepth, nullable */
    const float* uright;           /* [n_kp] mvuRight, nullable: NULL = monocular */
    const float* Tcw;              /* [12] row-major 3x4 */
};
typedef struct slamit_grow_frame slamit_grow_frame;

/* The appendable arrays of one map, named once: the memory the map, covis, point, edit, replace and tree records point to, each with
 * room for kf_cap keyframes, mp_cap points (obs_ptr: mp_cap + 1, kf_mp_ptr and kf_child_ptr: kf_cap + 1) and kfmp_cap keypoints.  All in /
 * out device pointers.  obs_ptr and kf_child_ptr are the CURRENT sets of the edit and tree records' alternating tables. */
struct slamit_grow_index {
    int32_t kf_cap, mp_cap, kfmp_cap, reserved;
    int32_t* kf_mp_ptr; int32_t* kf_mp; uint8_t* kf_octave; uint8_t* kf_desc /* 16-byte aligned */; float* kf_depth /* nullable with kf_th_depth */;
    uint8_t* kf_bad; int32_t* kf_parent; uint8_t* kf_to_be_erased; uint8_t* kf_not_erase; float* kf_th_depth;
    int32_t* kf_best; int32_t* cw_n; int32_t* ord_n; int32_t* kf_child_ptr; float* kf_center;
    float* mp_pos; float* mp_normal; float* mp_max_dist; float* mp_min_dist;
    uint8_t* mp_bad; int32_t* mp_nobs; int32_t* mp_ref_kf; int32_t* mp_found; int32_t* mp_visible; int32_t* mp_first_kf; int32_t* mp_replaced;
    uint8_t* mp_desc; int32_t* obs_ptr;
};
typedef struct slamit_grow_index slamit_grow_index;

/* One list over one map (host pointers everywhere, the frame records' included; synchronous).  The arrays of `grow` hold their full
 * capacities and are in / out; of the map record the call reads n_kf, n_mp and obs_kf.  op_status[n], edits[edit_cap], recent[recent_cap],
 * *n_recent, *n_edits_out and *n_new in / out, need[SLAMIT_GROW_NEEDS] and *status out: what lies past every count is left as the caller
 * filled it, and with a bit of SLAMIT_GROW_REFUSED everything but need and *status is.  Where the resident form skips an op, this form
 * refuses the call: a NEW_KF that does not name the next free slot, a slot, index, weight, kind, cand or src outside its range, an
 * ASSOCIATE whose frame record does not have its keyframe's keypoints, a frame_mp, kf_mp or obs_kf entry outside its table, a null
 * table or a CSR pointer array that does not ascend from 0 fails with SLAMIT_ERR_ARG; n above SLAMIT_GROW_MAX_OPS, n_frames above
 * SLAMIT_GROW_MAX_FRAMES, edit_cap above SLAMIT_EDIT_MAX_EDITS or recent_cap above SLAMIT_UPKEEP_MAX_RECENT with SLAMIT_ERR_CAPACITY; each
 * with a message and before anything is launched.  COST: as for the other host forms, it stages every table both ways: for parity and tests. */
int slamit_map_grow_apply(int device, const slamit_map_index* map, const slamit_grow_index* grow, int32_t n_frames, const slamit_grow_frame* frames,
                          int32_t n, const slamit_grow_op* ops, int32_t cand_cap, const uint8_t* cand_status, const float* cand_x3d, int32_t* op_status,
                          int32_t edit_cap, slamit_map_edit* edits, int32_t* n_edits_out, int32_t recent_cap, int32_t* recent, int32_t* n_recent,
                          int32_t* n_new, int32_t* need, int32_t* status);

/* One list per map for n_maps maps, everything resident.  `maps`, `grow` and `frames` are HOST arrays of records holding DEVICE
 * pointers; of the map record the call reads n_kf, n_mp and obs_kf.  Map m takes the first d_n[m] ops of d_ops[m].  The device cannot be
 * shown its tables first: an op with a slot, index, weight or frame record outside its range is skipped whole, never dereferenced; the
 * pointer arrays kf_mp_ptr, obs_ptr and kf_child_ptr are trusted to ascend from 0 inside their tables, as everywhere in this family.
 * cap above SLAMIT_GROW_MAX_OPS, n_frames above SLAMIT_GROW_MAX_FRAMES, edit_cap above SLAMIT_EDIT_MAX_EDITS or recent_cap above
 * SLAMIT_UPKEEP_MAX_RECENT (the ceilings of the calls that read the two lists) fails with SLAMIT_ERR_CAPACITY before anything is launched.
 * What lies past every count is left as the caller filled it.  Asynchronous on `stream`, no synchronisation, no state; the workspace
 * (8 mp_cap bytes per map, rounded up to 16) is cleared on the stream by the call.  One workgroup per map walks the list. */
struct slamit_map_grow_batch_rec {
    int32_t n_maps, cap, n_frames, cand_cap, edit_cap, recent_cap, mp_cap, reserved;
    const slamit_map_index* maps;          /* HOST [n_maps], device pointers inside; n_maps <= SLAMIT_LOCAL_MAP_MAX_MAPS */
    const slamit_grow_index* grow;         /* HOST [n_maps], device pointers inside */
    const slamit_grow_frame* frames;       /* HOST [n_frames], device pointers inside; n_frames <= SLAMIT_GROW_MAX_FRAMES */
    const slamit_grow_op* d_ops;           /* [n_maps][cap], cap <= SLAMIT_GROW_MAX_OPS */
    const int32_t* d_n;                    /* [n_maps] */
    const uint8_t* d_cand_status;          /* [n_maps][cand_cap]: slamit_triangulate_result.status */
    const float* d_cand_x3d;               /* [n_maps][cand_cap][3]: slamit_triangulate_result.x3d */
    int32_t* d_op_status;                  /* [n_maps][cap] in / out: the slot given (NEW_KF, NEW_POINT), kf (ASSOCIATE), or a code below 0 */
    slamit_map_edit* d_edits;              /* [n_maps][edit_cap] in / out: slamit_map_edit_batch_rec.d_edits with cap = edit_cap */
    int32_t* d_n_edits_out;                /* [n_maps] out: slamit_map_edit_batch_rec.d_n */
    int32_t* d_recent;                     /* [n_maps][recent_cap] in / out: slamit_point_culling_batch_rec.d_recent with cap = recent_cap */
    int32_t* d_n_recent;                   /* [n_maps] in / out: slamit_point_culling_batch_rec.d_n */
    int32_t* d_n_new;                      /* [n_maps] out: A */
    int32_t* d_need;                       /* [n_maps][SLAMIT_GROW_NEEDS] out */
    int32_t* d_status;                     /* [n_maps] out */
    void* d_workspace;                     /* slamit_map_grow_workspace(n_maps, mp_cap) bytes, 8-byte aligned */
    size_t workspace_bytes;
};
typedef struct slamit_map_grow_batch_rec slamit_map_grow_batch_rec;
size_t slamit_map_grow_workspace(int n_maps, int mp_cap);
int slamit_map_grow_batch_dev(int device, const slamit_map_grow_batch_rec* batch, void* stream);

/* ---- Essential-graph optimisation (loop closing, between OptimizeSim3 / CorrectLoop's fusion and the global BA) ----------------
 * Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044) with the g2o it instantiates: one VertexSim3Expmap per good keyframe
 * (estimate Scw, _fix_scale = fix_scale), per edge an EdgeSim3 (Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h:99-126: error
 * log(C * S_v0 * S_v1^-1), information I7, no robust kernel, NUMERIC Jacobians -- core/base_binary_edge.hpp:131-200, central
 * differences with delta 1e-9, a fixed vertex skipped), Levenberg-Marquardt from lambda_init (setUserLambdaInit(1e-16)) for max_its
 * iterations (20) with the fork's stop rules, then [R | t / s] per keyframe and correctedSwr.map(Srw.map(Xw)) per good point.
 *
 * Two steps.  slamit_essential_plan (host only, nothing of the GPU) restates :847-983, the choice of edges, over slot-numbered
 * tables; slamit_essential_graph* takes that edge list with the Sim3s and runs the rest on the device.
 *
 * THE PLAN.  Slots need not be ordered: every `<` of the reference is taken on kf_id (mnId).  Edges come in the reference's
 * insertion order: first the LoopConnections ones (kind SLAMIT_EG_LOOP_CONNECTION: measured from Scw on both sides), then per
 * keyframe its spanning-tree edge, its loop edges and its covisibility edges (SLAMIT_EG_NORMAL: measured from Snc).  Kept as the
 * reference has them: the sInsertedEdges test applies to covisibility edges only; the (cur, loop) pair is exempt from the weight
 * gate; parallel edges between one pair are legal; pKFn != parent, !hasChild and !sLoopEdges.count exclude a covisible keyframe;
 * GetCovisiblesByWeight returns NOTHING for a row none of whose weights is below min_feat (KeyFrame.cc:195-197).
 * Departures: the reference walks std::map / std::set<KeyFrame*> in pointer order, this walks ascending slots;
 * GetWeight is read from the ordered row; a bad keyframe is skipped as a source (Map::GetAllKeyFrames holds none); an edge that
 * names a bad or out-of-range keyframe refuses the whole call with SLAMIT_ERR_ARG (the reference would hand g2o a NULL vertex).
 * inc_ptr / inc_edge: per keyframe slot the incident edges in list order, entry = 2 * edge + side (side 1: the slot is v1).
 * More than edge_cap edges fails with SLAMIT_ERR_CAPACITY (*n_edge then holds the count needed, nothing else is written). */
#define SLAMIT_EG_NORMAL 0
#define SLAMIT_EG_LOOP_CONNECTION 1
struct slamit_eg_graph {
    int32_t n_kf, row_cap;          /* keyframe slots; entries per ordered covisibility row */
    int32_t loop_kf, cur_kf;        /* slots of pLoopKF, pCurKF */
    int32_t min_feat, reserved;     /* 100 */
    const uint8_t* kf_bad;          /* [n_kf] */
    const int32_t* kf_id;           /* [n_kf] mnId */
    const int32_t* kf_parent;       /* [n_kf] slot, -1 = none */
    const int32_t* child_ptr;       /* [n_kf + 1] */
    const int32_t* child_kf;        /* mspChildrens */
    const int32_t* loop_ptr;        /* [n_kf + 1] */
    const int32_t* loop_kf_list;    /* mspLoopEdges (GetLoopEdges) */
    const int32_t* ord_kf;          /* [n_kf][row_cap] as slamit_covis_index.ord_kf */
    const int32_t* ord_w;           /* [n_kf][row_cap] */
    const int32_t* ord_n;           /* [n_kf] */
    const int32_t* conn_ptr;        /* [n_kf + 1] LoopConnections: row i = the set of keyframe i (empty: i is no key of the map) */
    const int32_t* conn_kf;
};
typedef struct slamit_eg_graph slamit_eg_graph;
int slamit_essential_plan(const slamit_eg_graph* g, int32_t edge_cap, int32_t* edge_v0, int32_t* edge_v1, int32_t* edge_kind,
                          int32_t* n_edge, int32_t* inc_ptr /* [n_kf + 1] */, int32_t* inc_edge /* [2 * edge_cap] */);

/* THE OPTIMISATION.  Ceilings: SLAMIT_EG_MAX_KF keyframes that are neither fixed nor bad (7,168 unknowns: the dense lower triangle,
 * 32 x 32 tiles, is 206 MB of the workspace), SLAMIT_EG_MAX_EDGES edges (64 per free keyframe at the ceiling -- the essential graph
 * is the spanning tree plus the covisibility edges of weight >= 100 plus the loop edges, a handful per keyframe; an edge keeps 120
 * doubles on the device, 63 MB at the ceiling), SLAMIT_EG_MAX_ITS iterations, SLAMIT_EG_MAX_POINTS points.  One past any of them
 * refuses the call with SLAMIT_ERR_CAPACITY; an edge or a point's reference outside [0, n_kf) or on a bad keyframe, an edge from a
 * keyframe to itself, a negative count or a missing array refuses it with SLAMIT_ERR_ARG; both before anything is launched or written.
 *
 * Numerics: double throughout.  (H + lambda I) x = b is solved DENSE by LDLt without pivoting (32-column panels, the trailing
 * update on v_mfma_f64_16x16x4_f64) where the reference runs Eigen's sparse SimplicialLDLT under an AMD ordering: the same system,
 * another elimination order, so results agree to rounding (1e-5 relative is what the tests hold them to), not bit for bit.  H and b
 * are summed edge by edge in list order, chi2 and the gain ratio's scale in a fixed order: two runs give identical bits.  A zero or
 * non-finite pivot fails the trial as SimplicialLDLT's NumericalIssue does (its cost counts as DBL_MAX; the state is not moved, where
 * g2o would apply the previous trial's x before undoing it).  The verdict of every trial is read back by the host (one 8-byte copy
 * and a stream wait per trial): the calls return when the result is complete.  lambda_init is taken literally: 0 (or less) is not
 * "choose for me" as g2o's setUserLambdaInit(0) is, it is the damping of the first trial, and a trial that fails leaves 0 at 0.
 *
 * A keyframe that is fixed or bad keeps its Scw; its pose is still written from it.  A bad point keeps its position and is not listed
 * in `touched`; `touched` holds the good points ascending, in the layout slamit_points_batch_rec.d_points / d_n read (one item,
 * cap >= n_pt), so that UpdateNormalAndDepth follows on the stream.  Entries past *n_touched: -1 in the host form, as the caller left
 * them in the device form. */
#define SLAMIT_EG_MAX_KF 1024
#define SLAMIT_EG_MAX_EDGES 65536
#define SLAMIT_EG_MAX_ITS 32
#define SLAMIT_EG_MAX_TRIALS 320          /* SLAMIT_EG_MAX_ITS x _maxTrialsAfterFailure */
#define SLAMIT_EG_MAX_POINTS (1 << 24)
struct slamit_eg_problem {
    int32_t n_kf, n_edge, n_pt;
    int32_t n_free;                  /* device form: keyframes neither fixed nor bad, which the caller states (the flags are on the
                                        device; a count that does not match fails the call with SLAMIT_ERR_ARG after the first launch,
                                        nothing of the result written; so does an edge, a good point's reference keyframe or an incidence
                                        pointer outside its table or on a bad keyframe, which a first kernel looks for before any other
                                        indexes by them).  Host form: ignored. */
    int32_t fix_scale;               /* bFixScale */
    int32_t max_its;                 /* 20 */
    double lambda_init;              /* 1e-16; used as given, 0 included (see Numerics) */
    const double* scw_r;             /* [n_kf][9] CorrectedSim3 where it has the keyframe, else (Rcw, tcw, 1): r row-major, */
    const double* scw_t;             /* [n_kf][3]   t, */
    const double* scw_s;             /* [n_kf]      s, as slamit_sim3_problem states a Sim3 */
    const double* snc_r;             /* [n_kf][9] NonCorrectedSim3 where it has the keyframe, else the keyframe's Scw */
    const double* snc_t;             /* [n_kf][3] */
    const double* snc_s;             /* [n_kf] */
    const uint8_t* fixed;            /* [n_kf] 1 = pLoopKF */
    const uint8_t* bad;              /* [n_kf] */
    const int32_t* edge_v0;          /* [n_edge] */
    const int32_t* edge_v1;          /* [n_edge] */
    const int32_t* edge_kind;        /* [n_edge] SLAMIT_EG_NORMAL / SLAMIT_EG_LOOP_CONNECTION */
    const int32_t* inc_ptr;          /* [n_kf + 1] as slamit_essential_plan writes them; host form: nullable (built from the edges) */
    const int32_t* inc_edge;         /* [2 n_edge] */
    const float* pt_pos;             /* [n_pt][3] GetWorldPos() */
    const int32_t* pt_ref;           /* [n_pt] slot of mnCorrectedReference where mnCorrectedByKF == pCurKF->mnId, else of the reference keyframe */
    const uint8_t* pt_bad;           /* [n_pt] */
};
typedef struct slamit_eg_problem slamit_eg_problem;

struct slamit_eg_stats {
    int32_t n_its;                               /* LM iterations run */
    int32_t n_trials;                            /* LM trials over all of them */
    int32_t n_free;                              /* keyframes in the system */
    int32_t status;                              /* 0 (a refused call does not write the record) */
    double chi2_init;                            /* cost before the first iteration */
    double chi2[SLAMIT_EG_MAX_ITS];              /* cost of the last evaluated trial of each iteration */
    double lambda[SLAMIT_EG_MAX_ITS];            /* lambda after each iteration */
    int32_t trials[SLAMIT_EG_MAX_ITS];           /* trials of each iteration */
    double trial_chi2[SLAMIT_EG_MAX_TRIALS];     /* per trial: cost at the tentative state (DBL_MAX: the factorisation failed) */
    double trial_rho[SLAMIT_EG_MAX_TRIALS];      /* per trial: the gain ratio; the step stood iff rho > 0 and the cost is finite */
};
typedef struct slamit_eg_stats slamit_eg_stats;

struct slamit_eg_result {
    double* sim3_r;                  /* [n_kf][9] corrected Siw */
    double* sim3_t;                  /* [n_kf][3] */
    double* sim3_s;                  /* [n_kf] */
    double* pose;                    /* [n_kf][12] R row-major, t / s */
    float* pt_pos;                   /* [n_pt][3] */
    int32_t* touched;                /* [n_pt] */
    int32_t* n_touched;              /* [1] */
    slamit_eg_stats* stats;          /* host form: nullable.  Device form: required, a DEVICE pointer */
};
typedef struct slamit_eg_result slamit_eg_result;

/* Host pointers, synchronous. */
int slamit_essential_graph(int device, const slamit_eg_problem* prob, slamit_eg_result* res);
/* Device pointers in both records, a caller-owned workspace of slamit_essential_graph_workspace(n_free, n_kf, n_edge, n_pt) bytes
 * (256-byte aligned).  Runs on `stream` and waits on it once per LM trial; complete when it returns. */
size_t slamit_essential_graph_workspace(int n_free, int n_kf, int n_edge, int n_pt);
int slamit_essential_graph_dev(int device, const slamit_eg_problem* prob, const slamit_eg_result* res, void* d_workspace,
                               size_t workspace_bytes, void* stream);

/* ---- misc -------------------------------------------------------------------------------- */

const char* slamit_last_error(void);
const char* slamit_version(void);
int slamit_device_count(void);

/* Devices and streams.  Every entry point runs on the device it is given (handles: the device of slamit_*_create) and
 * restores the caller's current device before it returns.  The host-pointer entry points WITHOUT a device argument
 * (slamit_hamming_best2, slamit_hamming_matrix, slamit_distinctive_batch) use the calling thread's slamit_set_device()
 * (-1 = whatever device is current, the default).  `stream` arguments: NULL means the handle's own stream for entry points
 * that take a handle, and the legacy default stream of `device` for the handle-less *_dev entry points; pass an explicit
 * stream to order several calls.  Host-pointer entry points keep one pinned block, one device slab and one stream per
 * calling thread and call site; they are released when the thread exits or by slamit_release_thread_scratch(). */
int slamit_set_device(int device);
void slamit_release_thread_scratch(void);

#ifdef __cplusplus
}
#endif
#endif /* SLAMIT_H */
