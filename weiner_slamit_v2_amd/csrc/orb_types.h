// orb_types.h — host/device shared descriptors of the ORB pipeline's HBM layout, and the rules the host's planning (orb_plan.cc)
// and the kernels (orb_kernels.hip) both apply to it.  Plain C++ outside a HIP compile.
#ifndef SLAMIT_ORB_TYPES_H
#define SLAMIT_ORB_TYPES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define ORB_HD __host__ __device__
#else
#define ORB_HD
#endif

#define ORB_MAX_LEVELS 16
#define ORB_MAX_ROOTS 8          // octree root nodes = round(width/height) of the detection box
#define ORB_MIN_BORDER 16        // EDGE_THRESHOLD - 3   (ORBextractor.cc:789)
#define ORB_CELL_MAX 59          // wCell, hCell < 60 because nCols = floor(width/30)
#define ORB_TILE_MAX (ORB_CELL_MAX + 6)
#define ORB_CC_PAD 32            // ints between two (frame, level) candidate counters: one 128-byte line each, so the
                                 // FAST waves' atomics do not serialise on one L2 line
#define BLUR_STEPS 4             // 16-row steps of one blur strip
#define ORB_BLUR_STRIP_H (16 * BLUR_STEPS)   // rows of one blur strip (strips are 64 columns wide)

// LDS of one octree workgroup: the node arrays, then the key arrays (6 bytes per candidate)
ORB_HD inline size_t orbk_octree_node_bytes(int node_cap) {
    return ((size_t)node_cap * (8 + 2 * 8 + 2 * 4 + 4 * 4 + 5 * 4 + 4 + 4) + 64 + 15) & ~(size_t)15;
}
ORB_HD inline size_t orbk_octree_smem(int node_cap, int key_cap) { return orbk_octree_node_bytes(node_cap) + (size_t)key_cap * 6; }
#define OCT_LDS_KEYS_MAX 10240   // LDS key arrays hold at most this many candidates of one (frame, level), 6 bytes each
#define OCT_LDS_KEYS_MIN 2048
#define OCT_LDS_BUDGET (78 * 1024)   // per workgroup, so that two fit a CU

// One pyramid level.  Planes of all frames of a batch are stored level-major:
//   plane(level, frame) = pyr + plane_off + frame * plane_bytes, rows of `stride` bytes
// (stride = w rounded up to 64 so every row starts on a 64-byte boundary).  Level 0 lives in
// the caller's buffer (its own stride / frame stride) and has no plane of its own.
struct OrbLevel {
    int32_t w, h;
    int32_t stride;
    int32_t quota;             // mnFeaturesPerLevel[level]
    uint64_t plane_off;        // bytes, in the pyramid buffer (levels >= 1) ...
    uint64_t plane_bytes;      // ... per frame
    uint64_t blur_off;         // bytes, in the blurred-pyramid buffer (all levels)
    uint64_t blur_bytes;
    // FAST cell grid (ORBextractor.cc:797-803)
    int32_t nCols, nRows, wCell, hCell;
    int32_t maxBorderX, maxBorderY;   // w - 16, h - 16
    int32_t cell_base;         // index of this level's first cell in the per-frame cell list
    int32_t ncells;
    int32_t blur_tile_base;    // index of this level's first blur strip (64 x ORB_BLUR_STRIP_H) in the per-frame strip list
    // candidate list of (frame, level): cand + cand_off + frame * cand_frame_stride  (elements)
    uint64_t cand_off;
    int32_t cand_cap;
    // octree roots (ORBextractor.cc:556-576)
    int32_t nIni;
    float hX;
    int32_t rootUL[ORB_MAX_ROOTS], rootUR[ORB_MAX_ROOTS];
    int32_t boxH;              // maxBorderY - minBorderY
    // level keypoints: lkp + kp_off + frame * kp_frame_stride
    int32_t kp_off, kp_cap;    // kp_cap = node capacity = max(quota, 4*nIni) + 4
    float scale;               // mvScaleFactor[level]
    float patch_size;          // (float)(int)(31 * scale)
};

// What fast_cells_kernel needs of every level, passed BY VALUE in the kernel arguments: a wave finds its level
// and geometry with scalar loads of known addresses instead of a chain of dependent loads through a table in HBM.
struct FastLevel {
    int32_t cell_base, nCols, wCell, hCell, maxBorderX, maxBorderY, stride, cand_cap;
    uint64_t plane_off, plane_bytes, cand_off;
};
struct FastTab { FastLevel lv[ORB_MAX_LEVELS]; };

// Fused pyramid: one workgroup builds ALL levels of one image region, each level out of the
// previous one held in LDS.  Per (block, level): the region whose pixels this block stores to HBM
// ("own") and the superset it has to compute because deeper levels read it ("need").
struct PyrBox {
    int16_t ox0, oy0, ox1, oy1;
    int16_t nx0, ny0, nx1, ny1;
};
struct PyrTabs {               // cv::resize coefficient tables of level l (from level l-1), device pointers
    const int32_t* xofs; const int16_t* ialpha;
    const int32_t* yofs; const int16_t* ibeta;
};

// Banded pyramid (pyramid_bands_kernel): a workgroup is (frame, band of rows) and walks the levels of one segment, each level >= the
// segment's second out of the previous one's rows held in LDS.  Per level, BY VALUE in the kernel arguments (as FastTab): where the
// level's resize_rows8 tables sit in the table block, its plane, and the pitch of its LDS tile.
struct BandLevel {
    uint64_t col_off, row_off;   // bytes, in the table block: the rows8 column table and the row table
    uint64_t plane_off;          // OrbLevel::plane_off
    int32_t ngroups, dstride, pitch;
    uint32_t inv_groups;         // ceil(2^32 / ngroups)
};
struct BandTab { BandLevel lv[ORB_MAX_LEVELS]; };
struct BandRows { uint16_t own0, own1, cmp0, cmp1; };   // per (band, level): rows stored to HBM, rows computed (a superset)
#define ORB_BAND_LDS_BUDGET (78 * 1024)   // both tiles of a workgroup: at least two workgroups fit a CU's 160 KB
#define ORB_BAND_SLACK 16                 // bytes behind a tile: the 16-byte window of a row's last group may pass the row end

// Orientation and descriptor passes: a workgroup is four waves over consecutive keypoints of one (frame, level).  A frame's
// workgroups are numbered level-major and every level gets as many as its kp_cap needs (orb_plan_kp_blocks); the table goes BY VALUE
// in the kernel arguments (as FastTab) and a workgroup finds its level with a scalar walk over it.
#define ORB_IC_KP_PER_WG 32      // ic_angle_kernel: 4 waves x 8 keypoints
#define ORB_DESC_KP_PER_WG 16    // describe_kernel: 4 waves x 4 keypoints
// first workgroup of level l in a frame; from [nlevels] on: the workgroups per frame.  (Dword aligned: the kernels read it with scalar loads.)
struct alignas(4) KpBlockTab { uint16_t first[ORB_MAX_LEVELS + 1]; };

struct OrbLevelKp {            // a keypoint in level coordinates, after the octree
    int16_t x, y;
    float response;
    float angle;
    float cs, sn;              // cos / sin of the angle as computeOrbDescriptor needs them (set by the IC kernel)
};

#endif
