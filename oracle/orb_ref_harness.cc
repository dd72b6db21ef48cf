// orb_ref_harness.cc — drives the REFERENCE's own ORB_SLAM2/src/ORBextractor.cc (compiled by oracle/Makefile.ref where it lies, against
// the stand-in headers of oracle/cvstub_orb) from POD inputs.  TEST INFRASTRUCTURE ONLY: a stand-alone program, oracle/_ref/orb_ref_harness,
// used in the authoring container by tools/gen_orb_ref_golden.py (tests/golden/orb_ref_*.npz) and by tests/test_orb_ref_live.py.
//
// What is pinned: THE REFERENCE UNDER A MONOTONE ALLOCATOR.  DistributeOctTree sorts pair<int, ExtractorNode*> (ORBextractor.cc:697), so
// among equal-sized nodes the order of expansion is the order of the nodes' heap addresses.  This program replaces the global operator
// new with a bump allocator that never reuses memory (operator delete does nothing), which makes the addresses of the std::list nodes
// of one DistributeOctTree call increase in creation order and line 697 a function of the inputs alone: the only deterministic reading
// of that line.  `--system-allocator` leaves malloc / free in place; it exists for one observation, no test uses it.
// The allocator lives in this program only, never in a library that python loads.
//
// Everything ORBextractor.cc wrote itself runs as written: constructor tables, ComputePyramid's views, the cell walk, the FAST retry,
// DistributeOctTree / DivideNode, IC_Angle, computeOrbDescriptor, the order of operator().  The six OpenCV primitives it calls are NOT
// OpenCV: the stand-in headers hand them to oracle/orb_oracle.cc's exported functions (linked in here), so they stay restated.  cos / sin
// of computeOrbDescriptor are this platform's libm.
//
//   orb_ref_harness [--system-allocator] REQUEST REPLY          little-endian binary files
// REQUEST  i32 mode
//   mode 1 (extract)  i32 nfeatures, f32 scaleFactor, i32 nlevels, iniThFAST, minThFAST, width, height; u8 image[height * width]
//   mode 2 (octree)   i32 n, minX, maxX, minY, maxY, N, level; f32 xyr[n * 3]
// REPLY
//   mode 1  i32 n; kp[n] (x y size angle response: f32, octave class_id: i32); u8 desc[n * 32]        operator()'s output
//           per level: i32 w, h; u8 plane[(h + 38) * (w + 38)]                                        the buffer mvImagePyramid[level] looks into
//           per level: i32 m; kp[m]                                                                   as they leave ComputeKeyPointsOctTree
//           f32 mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2 [nlevels]; i32 mnFeaturesPerLevel[nlevels]; i32 umax[16]
//           i64 bytes handed out by the allocator
//   mode 2  i32 m; f32 xyr[m * 3]                                                                     DistributeOctTree's result in list order
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <new>
#include <string>
#include <vector>

#include "ORBextractor.h"

// ---- the monotone allocator ------------------------------------------------------------------------------------------------------
// One reservation, sized from runs: a 640x480 noise frame at 1000 features hands out 137 MB and the 2000-feature extractor on a rich
// frame 70 MB (every DivideNode reserves four key vectors of its parent's size and nothing is given back); the fixtures, all sub-VGA,
// stay below 20 MB.  8 GB of address space leaves room for 1280x720; the pages are touched only as the pointer reaches them.
namespace {
const size_t kArenaBytes = (size_t)8 << 30;
char* g_arena = 0;
size_t g_used = 0;
bool g_system = false;

void* bump(size_t n) {
    if (!g_arena) {
        void* p = mmap(0, kArenaBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) { fputs("orb_ref_harness: cannot reserve the arena\n", stderr); abort(); }
        g_arena = (char*)p;
    }
    n = (n + 15) & ~(size_t)15;
    if (n > kArenaBytes - g_used) { fputs("orb_ref_harness: arena exhausted\n", stderr); abort(); }
    void* r = g_arena + g_used;
    g_used += n ? n : 16;
    return r;
}
inline bool in_arena(void* p) { return g_arena && (char*)p >= g_arena && (char*)p < g_arena + kArenaBytes; }
}  // namespace

void* operator new(size_t n) {
    if (g_system) {
        void* p = malloc(n ? n : 1);
        if (!p) throw std::bad_alloc();
        return p;
    }
    return bump(n);
}
void* operator new[](size_t n) { return operator new(n); }
void operator delete(void* p) noexcept { if (p && !in_arena(p)) free(p); }
void operator delete[](void* p) noexcept { operator delete(p); }

namespace {

// the protected members, reached through a derived class
struct Ext : public ORB_SLAM2::ORBextractor {
    Ext(int nf, float sf, int nl, int ini, int mn) : ORB_SLAM2::ORBextractor(nf, sf, nl, ini, mn) {}
    void levels(const cv::Mat& image, std::vector<std::vector<cv::KeyPoint> >& all) {
        ComputePyramid(image);
        ComputeKeyPointsOctTree(all);
    }
    std::vector<cv::KeyPoint> octree(const std::vector<cv::KeyPoint>& keys, int minX, int maxX, int minY, int maxY, int N, int level) {
        return DistributeOctTree(keys, minX, maxX, minY, maxY, N, level);
    }
    const std::vector<int>& per_level() const { return mnFeaturesPerLevel; }
    const std::vector<int>& u_max() const { return umax; }
};

struct Out {
    FILE* f;
    void put(const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { fputs("orb_ref_harness: short write\n", stderr); exit(3); } }
    void i32(int32_t v) { put(&v, 4); }
    void f32s(const std::vector<float>& v) { put(v.data(), 4 * v.size()); }
    void kps(const std::vector<cv::KeyPoint>& v) {
        i32((int32_t)v.size());
        for (size_t i = 0; i < v.size(); ++i) {
            const cv::KeyPoint& k = v[i];
            float f[5] = {k.pt.x, k.pt.y, k.size, k.angle, k.response};
            int32_t o[2] = {k.octave, k.class_id};
            put(f, 20);
            put(o, 8);
        }
    }
};

std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> b;
    FILE* f = fopen(path, "rb");
    if (!f) return b;
    unsigned char tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) b.insert(b.end(), tmp, tmp + n);
    fclose(f);
    return b;
}

int extract(const unsigned char* req, size_t len, Out& out) {
    if (len < 32) return 2;
    int32_t p[8];
    memcpy(p, req, 32);
    float sf;
    memcpy(&sf, req + 8, 4);
    const int nf = p[1], nl = p[3], ini = p[4], mn = p[5], w = p[6], h = p[7];
    if (nl < 1 || w < 1 || h < 1 || len != 32 + (size_t)w * h) return 2;
    cv::Mat image(h, w, CV_8UC1);
    for (int r = 0; r < h; ++r) memcpy(image.ptr(r), req + 32 + (size_t)r * w, w);

    Ext ext(nf, sf, nl, ini, mn);
    std::vector<std::vector<cv::KeyPoint> > all;
    ext.levels(image, all);                       // the lists before operator() scales them
    std::vector<cv::KeyPoint> kps;
    cv::Mat desc;
    ext(image, cv::Mat(), kps, desc);             // and the whole call, from the top
    if (!kps.empty() && (desc.rows != (int)kps.size() || desc.cols != 32)) return 4;

    out.kps(kps);
    for (size_t i = 0; i < kps.size(); ++i) out.put(desc.ptr((int)i), 32);
    for (int l = 0; l < nl; ++l) {
        const cv::Mat& v = ext.mvImagePyramid[l];
        cv::Size whole;
        cv::Point ofs;
        v.locateROI(whole, ofs);
        if (ofs.x != 19 || ofs.y != 19 || whole.width != v.cols + 38 || whole.height != v.rows + 38) return 5;
        out.i32(v.cols);
        out.i32(v.rows);
        for (int r = -19; r < v.rows + 19; ++r) out.put(v.data + (ptrdiff_t)r * (ptrdiff_t)v.step - 19, (size_t)whole.width);
    }
    for (int l = 0; l < nl; ++l) out.kps(all[l]);
    out.f32s(ext.GetScaleFactors());
    out.f32s(ext.GetInverseScaleFactors());
    out.f32s(ext.GetScaleSigmaSquares());
    out.f32s(ext.GetInverseScaleSigmaSquares());
    for (int l = 0; l < nl; ++l) out.i32(ext.per_level()[l]);
    for (int i = 0; i < 16; ++i) out.i32(ext.u_max()[i]);
    int64_t used = (int64_t)g_used;
    out.put(&used, 8);
    return 0;
}

int octree(const unsigned char* req, size_t len, Out& out) {
    if (len < 32) return 2;
    int32_t p[8];
    memcpy(p, req, 32);
    const int n = p[1];
    if (n < 0 || len != 32 + (size_t)n * 12) return 2;
    std::vector<cv::KeyPoint> keys;
    for (int i = 0; i < n; ++i) {
        float v[3];
        memcpy(v, req + 32 + (size_t)i * 12, 12);
        keys.push_back(cv::KeyPoint(v[0], v[1], 7.f, -1.f, v[2]));   // as cv::FAST makes them
    }
    Ext ext(1000, 1.2f, 8, 20, 7);   // DistributeOctTree reads nfeatures for one reserve() and nothing else of the object
    std::vector<cv::KeyPoint> res = ext.octree(keys, p[2], p[3], p[4], p[5], p[6], p[7]);
    out.i32((int32_t)res.size());
    for (size_t i = 0; i < res.size(); ++i) {
        float v[3] = {res[i].pt.x, res[i].pt.y, res[i].response};
        out.put(v, 12);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    int a = 1;
    if (a < argc && !strcmp(argv[a], "--system-allocator")) { g_system = true; ++a; }
    if (argc - a != 2) { fputs("usage: orb_ref_harness [--system-allocator] REQUEST REPLY\n", stderr); return 2; }
    std::vector<unsigned char> req = slurp(argv[a]);
    if (req.size() < 4) return 2;
    int32_t mode;
    memcpy(&mode, req.data(), 4);
    Out out;
    out.f = fopen(argv[a + 1], "wb");
    if (!out.f) return 3;
    int rc = mode == 1 ? extract(req.data(), req.size(), out) : mode == 2 ? octree(req.data(), req.size(), out) : 2;
    if (fclose(out.f) != 0) return 3;
    return rc;
}
