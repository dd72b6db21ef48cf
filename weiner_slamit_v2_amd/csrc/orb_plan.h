// orb_plan.h — host-side plan of an ORB extractor handle: scale tables and quotas, level geometry, the FAST cell table, the blur
// strip tables, the workgroups of the keypoint passes, the cv::resize tables of every pyramid path, the banded pyramid's row ranges and
// the fused pyramid's boxes, and where each read-only table sits in the handle's one device block.  Plain C++17 (no HIP): the extractor
// (orb_api.hip) and the CPU tests of the plan (tests/test_orb_plan.py, tests/test_orb_bands_plan.py, tests/test_orb_kp_blocks.py) build it.
#ifndef SLAMIT_ORB_PLAN_H
#define SLAMIT_ORB_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/slamit.h"
#include "orb_types.h"

// What steers the plan besides the parameters: SlamitSwitches::resize_no8 (no resize_rows8_kernel tables).
struct OrbPlanOptions {
    bool resize_no8;
};

// Blur strips (64 columns x ORB_BLUR_STRIP_H rows), level-major, 4 words each: level | bx | by0 | 0.
struct OrbStrips {
    std::vector<uint32_t> tab;
    int base[ORB_MAX_LEVELS + 1];   // first entry of level l; base[nlevels]: the total
    size_t off;                     // in the table block
};

// Level l from level l-1 (l >= 1): the reference-shaped cv::resize INTER_LINEAR 8U tables and the row kernels' packed ones.
struct OrbResizeTabs {
    std::vector<int32_t> xofs, yofs;
    std::vector<int16_t> ialpha, ibeta;
    std::vector<uint32_t> col4, row4;   // resize_rows4_kernel; empty where the level's geometry does not fit it
    std::vector<uint32_t> col8;         // resize_rows8_kernel (its row table is row4); empty where refused or resize_no8
    size_t xofs_off, ialpha_off, yofs_off, ibeta_off, col4_off, row4_off, col8_off;   // in the table block
};

// One segment of the banded pyramid: levels first + 1 .. last of every frame in one launch, level `first` read from HBM.  A level's
// rows are split into `nbands` owned ranges (band b of level l: rows b h / nbands .. (b + 1) h / nbands); a band computes, besides the
// rows it owns, the rows of each level that its rows of the next level read (worked out backwards from `last`).
struct OrbBandSeg {
    int first, last, nbands;
    std::vector<BandRows> rows;   // [nbands][last - first], level first + 1 first
    int tile0, smem;              // bytes of the first LDS tile (levels first + 1, first + 3, ...) and of both tiles
    size_t rows_off;              // in the table block
};

struct OrbPlan {
    // ORBextractor's tables (mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2, mnFeaturesPerLevel)
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> per_level;
    std::vector<OrbLevel> levels;   // none for an empty image (and then no tables either)
    // per-frame sizes: frames are the outer dimension of every per-frame array
    size_t pyr_frame_total, blur_frame_total, cand_frame_stride, kp_frame_stride;
    int max_out, node_cap, oct_key_cap, max_kp_level, max_wcell, max_hcell;
    // FAST: the non-empty cells in the reference's visiting order, 4 words each, and the per-level table the kernel takes by value
    std::vector<uint32_t> cells;
    size_t cells_off;
    FastTab fast;
    // orientation and descriptor passes: the workgroups of every level inside a frame (orb_plan_kp_blocks)
    KpBlockTab ic_blocks, desc_blocks;
    // blur: every strip (blur_all_kernel), and the same strips split into those inside the level (blur_stream_kernel) and the rest
    OrbStrips blur_all, blur_str, blur_edge;
    // pyramid: per-level tables ([nlevels], entry 0 unused); rows4_ok: every level fits the row kernels
    std::vector<OrbResizeTabs> rs;
    bool rows4_ok;
    // fused pyramid: [pyr_regions][nlevels] boxes and a PyrTabs per level; pyr_regions 0: no fused plan
    int pyr_regions, pyr_bufA, pyr_smem;
    std::vector<PyrBox> boxes;
    size_t levels_off, boxes_off, tabs_off;
    // banded pyramid: the segments that build levels 1 .. nlevels - 1 between them and the per-level table; no segments: no banded
    // plan (some level without rows8 tables, or a band that does not fit the LDS budget)
    std::vector<OrbBandSeg> bands;
    BandTab band_tab;
    size_t table_bytes;   // the table block
};

// Plans a handle for p.  Returns false with *why set when the geometry cannot be extracted (a level smaller than one FAST cell,
// an aspect ratio beyond ORB_MAX_ROOTS octree roots, or more features than the LDS octree holds).  p is range-checked already.
bool orb_plan(const slamit_orb_params& p, const OrbPlanOptions& o, OrbPlan& plan, const char** why);

// The workgroups of a keypoint pass that handles `per` keypoints per workgroup: level l gets ceil(kp_cap / per) of them, numbered
// level-major inside a frame.  False when a frame's count does not fit the table's 16 bits.
bool orb_plan_kp_blocks(const std::vector<OrbLevel>& levels, int per, KpBlockTab& tab);

// Plans the rows of one banded segment (levels first + 1 .. last, level `first` the source) over the plan's resize tables; false --
// nothing truncated -- when a level has fewer rows than bands or a band's two tiles pass lds_budget bytes.  Fills every field of
// `seg` but rows_off.
bool orb_plan_band_segment(const OrbPlan& plan, int first, int last, int nbands, size_t lds_budget, OrbBandSeg& seg);

// The table block as the device gets it (table_bytes): every table at its offset, the PyrTabs pointing into `base` (the block's
// device address; null gives offsets).
void orb_plan_image(const OrbPlan& plan, const uint8_t* base, std::vector<uint8_t>& img);

#endif
