// orb_plan.cc — host-side plan of an ORB extractor handle (orb_plan.h).  Follows ORB_SLAM2::ORBextractor
// (src/ORBextractor.cc:415-482, 556-576, 789-822, 1138-1168) and cv::resize INTER_LINEAR 8U.
#include "orb_plan.h"

#include <math.h>
#include <string.h>

#include <algorithm>

namespace {

inline int cv_round(double v) { return (int)lrint(v); }  // cvRound: half-to-even
inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline short sat_short(float v) {
    int iv = cv_round((double)v);
    return (short)(iv < -32768 ? -32768 : iv > 32767 ? 32767 : iv);
}

// scale tables and quotas (ORBextractor.cc:422-455; scaleFactor is a double member)
void plan_scales(const slamit_orb_params& p, OrbPlan& P) {
    const int nl = p.nlevels;
    const double scaleFactor = (double)p.scale_factor;
    P.scale.assign(nl, 1.f); P.sigma2.assign(nl, 1.f); P.inv_scale.assign(nl, 1.f); P.inv_sigma2.assign(nl, 1.f);
    for (int i = 1; i < nl; ++i) {
        P.scale[i] = (float)(P.scale[i - 1] * scaleFactor);
        P.sigma2[i] = P.scale[i] * P.scale[i];
    }
    for (int i = 0; i < nl; ++i) { P.inv_scale[i] = 1.0f / P.scale[i]; P.inv_sigma2[i] = 1.0f / P.sigma2[i]; }
    P.per_level.assign(nl, 0);
    float factor = (float)(1.0f / scaleFactor);
    float nDesired = p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nl));
    int sum = 0;
    for (int l = 0; l < nl - 1; ++l) {
        P.per_level[l] = cv_round(nDesired);
        sum += P.per_level[l];
        nDesired *= factor;
    }
    P.per_level[nl - 1] = std::max(p.nfeatures - sum, 0);
}

// level geometry (ORBextractor.cc:1143-1147, 789-803, 556-571) and the per-frame layout; frames are the outer dimension of every
// per-frame array: plane(level, f) = base + level_off + f * frame_total, so plane_bytes / blur_bytes are the frame totals
bool plan_levels(const slamit_orb_params& p, OrbPlan& P, const char** why) {
    const int nl = p.nlevels;
    size_t pyr_off = 0, blur_off = 0, cand_off = 0;
    int kp_off = 0, cell_base = 0, sum_cap = 0;
    P.levels.assign(nl, OrbLevel());
    for (int l = 0; l < nl; ++l) {
        OrbLevel& L = P.levels[l];
        float sc = P.inv_scale[l];
        L.w = cv_round((float)p.width * sc);
        L.h = cv_round((float)p.height * sc);
        L.stride = (int)round_up((size_t)std::max(L.w, 1), 64);
        L.quota = P.per_level[l];
        const size_t plane = (size_t)L.stride * std::max(L.h, 1);
        L.plane_off = l >= 1 ? pyr_off : 0;
        if (l >= 1) pyr_off += round_up(plane, 256);
        L.blur_off = blur_off; blur_off += round_up(plane, 256);
        L.maxBorderX = L.w - ORB_MIN_BORDER; L.maxBorderY = L.h - ORB_MIN_BORDER;
        const float width = (float)(L.maxBorderX - ORB_MIN_BORDER), height = (float)(L.maxBorderY - ORB_MIN_BORDER);
        L.nCols = (int)(width / 30.f); L.nRows = (int)(height / 30.f);
        if (L.w < 1 || L.h < 1 || L.nCols < 1 || L.nRows < 1) {   // the reference divides by zero on such a level
            *why = "slamit_orb_create: pyramid level smaller than one 30x30 FAST cell";
            return false;
        }
        L.wCell = (int)ceil(width / L.nCols); L.hCell = (int)ceil(height / L.nRows);
        L.cell_base = cell_base; L.ncells = L.nCols * L.nRows; cell_base += L.ncells;
        P.max_wcell = std::max(P.max_wcell, L.wCell); P.max_hcell = std::max(P.max_hcell, L.hCell);
        L.cand_cap = L.ncells * ((L.wCell + 1) / 2) * ((L.hCell + 1) / 2);  // NMS: <= 1 per 2x2 in a cell
        L.cand_off = cand_off; cand_off += round_up((size_t)L.cand_cap, 64);
        const int bw = L.maxBorderX - ORB_MIN_BORDER, bh = L.maxBorderY - ORB_MIN_BORDER;
        L.nIni = (int)round(static_cast<float>(bw) / bh);
        if (L.nIni < 1 || L.nIni > ORB_MAX_ROOTS) {
            *why = "slamit_orb_create: unsupported aspect ratio (octree roots)";
            return false;
        }
        L.hX = static_cast<float>(bw) / L.nIni;
        for (int i = 0; i < L.nIni; ++i) {
            L.rootUL[i] = (int)(L.hX * static_cast<float>(i));
            L.rootUR[i] = (int)(L.hX * static_cast<float>(i + 1));
        }
        L.boxH = bh;
        L.kp_cap = std::max(L.quota, 4 * L.nIni) + 4;
        L.kp_off = kp_off; kp_off += L.kp_cap;
        L.scale = P.scale[l];
        L.patch_size = (float)(int)(31 * P.scale[l]);
        P.node_cap = std::max(P.node_cap, L.kp_cap);
        P.max_kp_level = std::max(P.max_kp_level, L.kp_cap);
        sum_cap += L.kp_cap;
    }
    for (OrbLevel& L : P.levels) { L.plane_bytes = pyr_off; L.blur_bytes = blur_off; }
    P.max_out = std::max(P.max_out, sum_cap);
    P.pyr_frame_total = pyr_off; P.blur_frame_total = blur_off;
    P.cand_frame_stride = cand_off; P.kp_frame_stride = (size_t)kp_off;
    return true;
}

// Key arrays of the octree pass: as many candidates as fit beside the node arrays in the workgroup's LDS budget (lists above that
// use the HBM workspace).  Two 78 KB workgroups fill a CU's LDS, which also keeps every other kernel off the chip while the
// octree pass (a few hundred workgroups, latency bound) runs; images up to about VGA rarely have more than 5,000 candidates on a
// level, so their handles take 48 KB and the blur runs beside the octree on the side stream.
int octree_key_cap(int node_cap, int width, int height) {
    long budget = (long)width * height <= 640L * 480L * 3 / 2 ? 48L * 1024 : (long)OCT_LDS_BUDGET;
    const long room = budget - (long)orbk_octree_node_bytes(node_cap);
    return (int)std::min<long>(OCT_LDS_KEYS_MAX, std::max<long>(OCT_LDS_KEYS_MIN, room / 6)) & ~7;
}

// Cell table: the non-empty FAST cells of every level in the reference's visiting order (level, row, column;
// ORBextractor.cc:805-822), 4 words per cell:
//   0: level | cell index in the level << 8      1: iniX | iniY << 16      2: cw | ch << 8 (window size)
//   3: division magic  floor(2^20 / g) + 1  for g = (sw + 3) / 4, the groups of four scan pixels per row
// and the per-level geometry fast_cells_kernel takes by value.
void fast_cells(OrbPlan& P) {
    auto magic = [](int g) { return (uint32_t)((1u << 20) / (unsigned)std::max(g, 1) + 1u); };
    for (int l = 0; l < (int)P.levels.size(); ++l) {
        const OrbLevel& L = P.levels[l];
        for (int c = 0; c < L.ncells; ++c) {
            const int ci = c / L.nCols, cj = c - ci * L.nCols;
            const int iniX = ORB_MIN_BORDER + cj * L.wCell, iniY = ORB_MIN_BORDER + ci * L.hCell;
            if (iniY >= L.maxBorderY - 3 || iniX >= L.maxBorderX - 6) continue;  // ORBextractor.cc:810,819
            const int cw = std::min(L.wCell + 6, L.maxBorderX - iniX), ch = std::min(L.hCell + 6, L.maxBorderY - iniY);
            const int sw = cw - 6, sh = ch - 6;
            if (sw <= 0 || sh <= 0) continue;
            const uint32_t w[4] = {(uint32_t)l | ((uint32_t)c << 8), (uint32_t)iniX | ((uint32_t)iniY << 16),
                                   (uint32_t)cw | ((uint32_t)ch << 8), magic((sw + 3) >> 2)};
            P.cells.insert(P.cells.end(), w, w + 4);
        }
        FastLevel& D = P.fast.lv[l];
        D.cell_base = L.cell_base; D.nCols = L.nCols; D.wCell = L.wCell; D.hCell = L.hCell;
        D.maxBorderX = L.maxBorderX; D.maxBorderY = L.maxBorderY; D.stride = L.stride; D.cand_cap = L.cand_cap;
        D.plane_off = L.plane_off; D.plane_bytes = L.plane_bytes; D.cand_off = L.cand_off;
    }
}

// One walk over the blur strips of every level fills all three strip tables; a strip goes to the stream table when its columns
// and their 4-pixel halo lie inside the level.
void blur_strips(OrbPlan& P) {
    const int nl = (int)P.levels.size();
    for (int l = 0; l < nl; ++l) {
        OrbLevel& L = P.levels[l];
        L.blur_tile_base = (int)(P.blur_all.tab.size() / 4);
        for (int by = 0; by < L.h; by += ORB_BLUR_STRIP_H)
            for (int bx = 0; bx < L.w; bx += 64) {
                const uint32_t t[4] = {(uint32_t)l, (uint32_t)bx, (uint32_t)by, 0u};
                const bool inside = bx >= 4 && bx + 68 <= L.w && (L.stride & 3) == 0;
                for (OrbStrips* S : {&P.blur_all, inside ? &P.blur_str : &P.blur_edge}) S->tab.insert(S->tab.end(), t, t + 4);
            }
        for (OrbStrips* S : {&P.blur_all, &P.blur_str, &P.blur_edge}) S->base[l + 1] = (int)(S->tab.size() / 4);
    }
}

// per-axis tables of cv::resize INTER_LINEAR 8U (fixed point, 11 bits); `clampx` applies the
// x-axis rule (offset clamped and weight zeroed at both ends), the y axis keeps its weights
void resize_axis(int dn, int sn, bool clampx, std::vector<int32_t>& ofs, std::vector<int16_t>& coef) {
    double inv_scale = (double)dn / sn;
    double scale = 1. / inv_scale;
    ofs.resize(dn);
    coef.resize(2 * (size_t)dn);
    for (int d = 0; d < dn; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floor(f);
        f -= s;
        if (clampx) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= sn - 1) { f = 0; s = sn - 1; }
        }
        ofs[d] = s;
        coef[2 * d] = sat_short((1.f - f) * 2048.f);
        coef[2 * d + 1] = sat_short(f * 2048.f);
    }
}

// Tables of resize_rows4_kernel for one level from the reference-shaped xofs/ialpha/yofs/ibeta tables.
// Coefficients are non-negative (bilinear) and <= 2048, rows/columns < 65536.
// Returns false when the geometry does not fit the kernel (scale factor > 2.3: taps of one group further than
// 8 bytes apart; planes of 64K pixels or more): the fused / generic kernels then build the pyramid.
bool rows4_tables(int dw, int dh, int sw, int sh, const int* xofs, const short* ialpha, const int* yofs,
                  const short* ibeta, std::vector<uint32_t>& col, std::vector<uint32_t>& row) {
    const int ng = (dw + 3) / 4, row_end = (sw + 3) & ~3;
    if (sw >= 65536 || sh >= 65536) return false;
    col.assign((size_t)ng * 12, 0u);
    for (int g = 0; g < ng; ++g) {
        int L[4], R[4];
        uint32_t a[4];
        for (int j = 0; j < 4; ++j) {
            const int x = 4 * g + j;
            if (x < dw) {
                L[j] = xofs[x]; R[j] = std::min(xofs[x] + 1, sw - 1);
                a[j] = (uint32_t)(unsigned short)ialpha[2 * x] | ((uint32_t)(unsigned short)ialpha[2 * x + 1] << 16);
            } else { L[j] = L[0]; R[j] = L[0]; a[j] = 0; }   // padding pixels of the last dword: written as 0
        }
        const int base = L[0] & ~3, s = L[0] & 3;
        const int off1 = base + 8 <= row_end ? 4 : 0, off2 = base + 12 <= row_end ? 8 : off1;
        uint32_t* c = &col[(size_t)g * 12];
        c[0] = (uint32_t)base | ((uint32_t)s << 16) | ((uint32_t)off1 << 20) | ((uint32_t)off2 << 24);
        for (int j = 0; j < 4; ++j) {   // byte index inside the 8 bytes that start at L[0]; selector byte 0x0C reads as zero
            if (L[j] < L[0] || R[j] < L[0] || L[j] - L[0] > 7 || R[j] - L[0] > 7 || ialpha[0] < 0) return false;
            c[1 + j] = (uint32_t)(L[j] - L[0]) | 0x0C00u | ((uint32_t)(R[j] - L[0]) << 16) | 0x0C000000u;
            c[5 + j] = a[j];
        }
    }
    row.assign((size_t)(dh + 7) * 2, 0u);   // + 7 copies of the last row: a lane loads its (up to 8) rows as whole 16-byte pairs
    for (int y = 0; y < dh; ++y) {
        const int sy0 = std::min(std::max(yofs[y], 0), sh - 1), sy1 = std::min(std::max(yofs[y] + 1, 0), sh - 1);
        row[2 * (size_t)y] = (uint32_t)sy0 | ((uint32_t)sy1 << 16);
        row[2 * (size_t)y + 1] = (uint32_t)(unsigned short)ibeta[2 * y] | ((uint32_t)(unsigned short)ibeta[2 * y + 1] << 16);
        if (ibeta[2 * y] < 0 || ibeta[2 * y + 1] < 0) return false;
    }
    for (int y = dh; y < dh + 7; ++y) { row[2 * (size_t)y] = row[2 * (size_t)(dh - 1)]; row[2 * (size_t)y + 1] = row[2 * (size_t)(dh - 1) + 1]; }
    for (int x = 0; x < dw; ++x) if (ialpha[2 * x] < 0 || ialpha[2 * x + 1] < 0) return false;
    return true;
}

// Column table of resize_rows8_kernel (the row table is rows4_tables'); false when some group's taps do not lie as
// the kernel assumes -- pixels 0 .. 3 within bytes 0 .. 7 of the window that starts at the group's first left tap, pixels
// 4 .. 7 within bytes 4 .. 11 -- or the 8-byte stores of the last group would pass the row pitch.
bool rows8_table(int dw, int sw, size_t dstride, const int* xofs, const short* ialpha, std::vector<uint32_t>& col) {
    const int ng = (dw + 7) / 8;
    if (sw >= 65536 || (size_t)ng * 8 > dstride) return false;
    col.assign((size_t)ng * 20, 0u);
    for (int g = 0; g < ng; ++g) {
        int L[8], R[8];
        uint32_t a[8];
        const int L0 = xofs[8 * g];
        for (int j = 0; j < 8; ++j) {
            const int x = 8 * g + j;
            if (x < dw) {
                L[j] = xofs[x]; R[j] = std::min(xofs[x] + 1, sw - 1);
                if (ialpha[2 * x] < 0 || ialpha[2 * x + 1] < 0) return false;
                a[j] = (uint32_t)(unsigned short)ialpha[2 * x] | ((uint32_t)(unsigned short)ialpha[2 * x + 1] << 16);
            } else { L[j] = R[j] = L0 + (j >= 4 ? 4 : 0); a[j] = 0; }   // padding pixels of the last group: written as 0
        }
        uint32_t* c = &col[(size_t)g * 20];
        c[0] = (uint32_t)(L0 & ~3) | ((uint32_t)(L0 & 3) << 16);
        for (int j = 0; j < 8; ++j) {
            const int lo = j >= 4 ? 4 : 0;   // byte index inside the dword pair the pixel reads
            const int bl = L[j] - L0 - lo, br = R[j] - L0 - lo;
            if (bl < 0 || bl > 7 || br < 0 || br > 7) return false;
            c[1 + j] = (uint32_t)bl | 0x0C00u | ((uint32_t)br << 16) | 0x0C000000u;
            c[9 + j] = a[j];
        }
    }
    return true;
}

// the resize tables of every level >= 1; a refused table is left empty
void plan_resize(const OrbPlanOptions& o, OrbPlan& P) {
    const int nl = (int)P.levels.size();
    P.rs.assign(nl, OrbResizeTabs());
    for (int l = 1; l < nl; ++l) {
        const OrbLevel &S = P.levels[l - 1], &D = P.levels[l];
        OrbResizeTabs& T = P.rs[l];
        resize_axis(D.w, S.w, true, T.xofs, T.ialpha);
        resize_axis(D.h, S.h, false, T.yofs, T.ibeta);
        if (!rows4_tables(D.w, D.h, S.w, S.h, T.xofs.data(), T.ialpha.data(), T.yofs.data(), T.ibeta.data(), T.col4, T.row4)) {
            P.rows4_ok = false;
            T.col4.clear(); T.row4.clear();
        }
        if (o.resize_no8 || !rows8_table(D.w, S.w, (size_t)D.stride, T.xofs.data(), T.ialpha.data(), T.col8)) T.col8.clear();
    }
}

// Fused pyramid: ONE launch builds every level.  Each workgroup reads its region of level 0 (128x96 pixels) and produces the
// following levels out of LDS; per region and level the boxes say what it stores ("own") and what it has to compute because a
// deeper level reads it ("need").  The per-level row kernels take aligned inputs; this kernel takes the rest, and the per-level
// generic kernel what it cannot plan (pyr_regions stays 0).
void plan_pyramid_boxes(const slamit_orb_params& p, OrbPlan& P) {
    const int nl = (int)P.levels.size(), last = nl - 1;
    if (nl < 2) return;
    const int GX = std::max(1, (p.width + 127) / 128), GY = std::max(1, (p.height + 95) / 96);
    std::vector<PyrBox> boxes((size_t)GX * GY * nl);
    bool ok = true;
    size_t capA = 16, capB = 16;
    for (int gy = 0; gy < GY && ok; ++gy)
        for (int gx = 0; gx < GX && ok; ++gx) {
            PyrBox* B = &boxes[((size_t)gy * GX + gx) * nl];
            for (int l = 0; l <= last; ++l) {
                const OrbLevel& L = P.levels[l];
                B[l].ox0 = (int16_t)((long)gx * L.w / GX); B[l].ox1 = (int16_t)((long)(gx + 1) * L.w / GX);
                B[l].oy0 = (int16_t)((long)gy * L.h / GY); B[l].oy1 = (int16_t)((long)(gy + 1) * L.h / GY);
                if (l == 0) { B[l].ox0 = B[l].ox1 = B[l].oy0 = B[l].oy1 = 0; }  // the source is only read
                else if (B[l].ox1 <= B[l].ox0 || B[l].oy1 <= B[l].oy0) ok = false;
            }
            B[last].nx0 = B[last].ox0; B[last].nx1 = B[last].ox1;
            B[last].ny0 = B[last].oy0; B[last].ny1 = B[last].oy1;
            for (int l = last; l > 0 && ok; --l) {
                const std::vector<int32_t> &XO = P.rs[l].xofs, &YO = P.rs[l].yofs;
                const int sw = P.levels[l - 1].w, sh = P.levels[l - 1].h;
                int sx0 = XO[B[l].nx0], sx1 = std::min(XO[B[l].nx1 - 1] + 1, sw - 1) + 1;
                int sy0 = std::min(std::max(YO[B[l].ny0], 0), sh - 1);
                int sy1 = std::min(std::max(YO[B[l].ny1 - 1] + 1, 0), sh - 1) + 1;
                if (l - 1 > 0) {
                    sx0 = std::min(sx0, (int)B[l - 1].ox0); sx1 = std::max(sx1, (int)B[l - 1].ox1);
                    sy0 = std::min(sy0, (int)B[l - 1].oy0); sy1 = std::max(sy1, (int)B[l - 1].oy1);
                }
                if (l - 1 == 0) sx0 &= ~3;  // dword-aligned source patch
                B[l - 1].nx0 = (int16_t)sx0; B[l - 1].nx1 = (int16_t)sx1; B[l - 1].ny0 = (int16_t)sy0; B[l - 1].ny1 = (int16_t)sy1;
            }
            for (int l = 0; l <= last; ++l) {
                if (l > 0 && (B[l].nx1 - B[l].nx0 > 256 || B[l].ny1 - B[l].ny0 > 256)) ok = false;  // <= 4 columns per lane, row tables of 256
                size_t bytes = (size_t)(((B[l].nx1 - B[l].nx0) + 3) & ~3) * (B[l].ny1 - B[l].ny0);
                if (l & 1) capB = std::max(capB, bytes); else capA = std::max(capA, bytes);
            }
        }
    const int bufA = (int)round_up(capA, 16), smem = bufA + (int)round_up(capB, 16);
    if (!ok || smem > 150 * 1024) return;
    P.pyr_regions = GX * GY;
    P.pyr_bufA = bufA;
    P.pyr_smem = smem;
    P.boxes.swap(boxes);
}

// Banded pyramid: which rows of which level a (frame, band) workgroup computes and which of them it stores.
#ifndef ORB_BAND_COUNT
#define ORB_BAND_COUNT 8    // bands per frame
#define ORB_BAND_SPLIT 2    // the first segment ends at this level and the second reads it back from HBM; 0: one segment (measured: DESIGN.md section 4)
#endif

inline int band_pitch(int w) { return (int)round_up((size_t)((w + 7) / 8) * 8, 16); }   // whole 8-byte groups, rows on 16-byte boundaries

void plan_bands(OrbPlan& P) {
    const int nl = (int)P.levels.size();
    if (nl < 2 || !P.rows4_ok) return;
    for (int l = 1; l < nl; ++l) {
        const OrbResizeTabs& T = P.rs[l];
        if (T.col8.empty() || T.row4.empty() || P.levels[l].h >= 65536) return;   // some level keeps the four-pixel kernel
        BandLevel& V = P.band_tab.lv[l];
        V.ngroups = (P.levels[l].w + 7) / 8;
        V.inv_groups = (uint32_t)((0x100000000ull + (unsigned)V.ngroups - 1) / (unsigned)V.ngroups);
        V.dstride = P.levels[l].stride;
        V.pitch = band_pitch(P.levels[l].w);
        V.plane_off = P.levels[l].plane_off;
    }
    const int split = ORB_BAND_SPLIT > 0 && ORB_BAND_SPLIT < nl - 1 ? ORB_BAND_SPLIT : nl - 1;
    std::vector<OrbBandSeg> segs;
    for (int first = 0; first < nl - 1; first = segs.back().last) {
        segs.emplace_back();
        int nb = ORB_BAND_COUNT;   // wider frames than VGA take more, thinner bands until two tiles fit the budget
        while (!orb_plan_band_segment(P, first, first == 0 ? split : nl - 1, nb, ORB_BAND_LDS_BUDGET, segs.back()))
            if ((nb *= 2) > 8 * ORB_BAND_COUNT) return;
    }
    P.bands.swap(segs);
}

// offsets of the read-only tables in one block, each on a 256-byte boundary
void plan_table_block(OrbPlan& P) {
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = round_up(off, 256); off = at + bytes; return at; };
    const int nl = (int)P.levels.size();
    P.levels_off = take(sizeof(OrbLevel) * nl);
    P.cells_off = take(sizeof(uint32_t) * P.cells.size());
    for (OrbStrips* S : {&P.blur_all, &P.blur_str, &P.blur_edge}) S->off = take(sizeof(uint32_t) * S->tab.size());
    for (int l = 1; l < nl; ++l) {
        OrbResizeTabs& T = P.rs[l];
        T.xofs_off = take(sizeof(int32_t) * T.xofs.size()); T.ialpha_off = take(sizeof(int16_t) * T.ialpha.size());
        T.yofs_off = take(sizeof(int32_t) * T.yofs.size()); T.ibeta_off = take(sizeof(int16_t) * T.ibeta.size());
        T.col4_off = take(sizeof(uint32_t) * T.col4.size()); T.row4_off = take(sizeof(uint32_t) * T.row4.size());
        T.col8_off = take(sizeof(uint32_t) * T.col8.size());
    }
    P.boxes_off = take(sizeof(PyrBox) * P.boxes.size());
    P.tabs_off = take(P.pyr_regions ? sizeof(PyrTabs) * nl : 0);
    for (OrbBandSeg& G : P.bands) G.rows_off = take(sizeof(BandRows) * G.rows.size());
    if (!P.bands.empty())
        for (int l = 1; l < nl; ++l) { P.band_tab.lv[l].col_off = P.rs[l].col8_off; P.band_tab.lv[l].row_off = P.rs[l].row4_off; }
    P.table_bytes = round_up(off, 256);
}

}  // namespace

bool orb_plan(const slamit_orb_params& p, const OrbPlanOptions& o, OrbPlan& plan, const char** why) {
    plan = OrbPlan();   // value-initialised: every size, count and offset starts at zero
    OrbPlan& P = plan;
    P.node_cap = 8; P.max_kp_level = 1;
    P.rows4_ok = true;
    plan_scales(p, P);
    P.max_out = p.nfeatures + 3 * p.nlevels;
    const bool empty = p.width == 0 || p.height == 0;   // an empty image: no levels, no tables
    if (!empty && !plan_levels(p, P, why)) return false;
    P.oct_key_cap = octree_key_cap(P.node_cap, p.width, p.height);
    if (orbk_octree_smem(P.node_cap, P.oct_key_cap) > 160 * 1024 - 1024 || P.node_cap >= 4096) {   // labels carry the node in 12 bits
        *why = "slamit_orb_create: nfeatures too large for the LDS octree";
        return false;
    }
    if (!orb_plan_kp_blocks(P.levels, ORB_IC_KP_PER_WG, P.ic_blocks) || !orb_plan_kp_blocks(P.levels, ORB_DESC_KP_PER_WG, P.desc_blocks)) {
        *why = "slamit_orb_create: nfeatures too large for the keypoint passes";   // (the octree's limit is far below this one)
        return false;
    }
    fast_cells(P);
    blur_strips(P);
    plan_resize(o, P);
    plan_pyramid_boxes(p, P);
    plan_bands(P);
    plan_table_block(P);
    return true;
}

bool orb_plan_kp_blocks(const std::vector<OrbLevel>& levels, int per, KpBlockTab& tab) {
    const int nl = (int)levels.size();
    if (nl > ORB_MAX_LEVELS || per < 1) return false;
    long at = 0;
    for (int l = 0; l <= ORB_MAX_LEVELS; ++l) {   // the entries behind [nlevels] repeat the total: the kernels' walk needs no level count
        if (at > 65535) return false;
        tab.first[l] = (uint16_t)at;
        if (l < nl) at += (std::max(levels[l].kp_cap, 0) + per - 1) / per;
    }
    return true;
}

bool orb_plan_band_segment(const OrbPlan& P, int first, int last, int nbands, size_t lds_budget, OrbBandSeg& seg) {
    const int nl = (int)P.levels.size(), nlv = last - first;
    if (first < 0 || last >= nl || nlv < 1 || nbands < 1) return false;
    seg = OrbBandSeg();
    seg.first = first; seg.last = last; seg.nbands = nbands;
    seg.rows.assign((size_t)nbands * nlv, BandRows());
    size_t tile[2] = {0, 0};
    for (int b = 0; b < nbands; ++b) {
        BandRows* R = &seg.rows[(size_t)b * nlv];   // R[l - first - 1]
        int need0 = 0, need1 = 0;                   // the rows of level l that the band's rows of level l + 1 read
        for (int l = last; l > first; --l) {
            const int h = P.levels[l].h;
            if (h < nbands || h >= 65536 || P.rs[l].row4.size() < 2 * (size_t)h) return false;
            const int own0 = (int)((long)b * h / nbands), own1 = (int)((long)(b + 1) * h / nbands);
            const int cmp0 = l == last ? own0 : std::min(own0, need0), cmp1 = l == last ? own1 : std::max(own1, need1);
            R[l - first - 1] = BandRows{(uint16_t)own0, (uint16_t)own1, (uint16_t)cmp0, (uint16_t)cmp1};
            need0 = 65535; need1 = 0;
            for (int y = cmp0; y < cmp1; ++y) {     // the row table's clamped source rows (sy0 | sy1 << 16)
                const uint32_t s = P.rs[l].row4[2 * (size_t)y];
                need0 = std::min(need0, (int)(s & 0xFFFFu)); need1 = std::max(need1, (int)(s >> 16) + 1);
            }
            if (l < last) {   // only the last level of a segment stays out of LDS
                size_t& t = tile[(l - first - 1) & 1];
                t = std::max(t, (size_t)(cmp1 - cmp0) * band_pitch(P.levels[l].w) + ORB_BAND_SLACK);
            }
        }
    }
    seg.tile0 = (int)round_up(tile[0], 16);
    seg.smem = seg.tile0 + (int)round_up(tile[1], 16);
    return (size_t)seg.smem <= lds_budget;
}

void orb_plan_image(const OrbPlan& P, const uint8_t* base, std::vector<uint8_t>& img) {
    img.assign(P.table_bytes, 0);
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(img.data() + off, src, bytes); };
    auto put_vec = [&](size_t off, const auto& v) { put(off, v.data(), sizeof(v[0]) * v.size()); };
    put(P.levels_off, P.levels.data(), sizeof(OrbLevel) * P.levels.size());
    put_vec(P.cells_off, P.cells);
    for (const OrbStrips* S : {&P.blur_all, &P.blur_str, &P.blur_edge}) put_vec(S->off, S->tab);
    for (size_t l = 1; l < P.rs.size(); ++l) {
        const OrbResizeTabs& T = P.rs[l];
        put_vec(T.xofs_off, T.xofs); put_vec(T.ialpha_off, T.ialpha); put_vec(T.yofs_off, T.yofs); put_vec(T.ibeta_off, T.ibeta);
        put_vec(T.col4_off, T.col4); put_vec(T.row4_off, T.row4); put_vec(T.col8_off, T.col8);
    }
    put_vec(P.boxes_off, P.boxes);
    for (const OrbBandSeg& G : P.bands) put_vec(G.rows_off, G.rows);
    if (!P.pyr_regions) return;
    std::vector<PyrTabs> tabs(P.levels.size(), PyrTabs{nullptr, nullptr, nullptr, nullptr});   // level 0 has none
    auto at = [&](size_t off) { return (uintptr_t)base + off; };
    for (size_t l = 1; l < tabs.size(); ++l) {
        const OrbResizeTabs& T = P.rs[l];
        tabs[l].xofs = reinterpret_cast<const int32_t*>(at(T.xofs_off)); tabs[l].ialpha = reinterpret_cast<const int16_t*>(at(T.ialpha_off));
        tabs[l].yofs = reinterpret_cast<const int32_t*>(at(T.yofs_off)); tabs[l].ibeta = reinterpret_cast<const int16_t*>(at(T.ibeta_off));
    }
    put_vec(P.tabs_off, tabs);
}
