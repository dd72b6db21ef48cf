// voc.hip — the vocabulary transform on the device (include/slamit.h, slamit_voc_*): Frame::ComputeBoW / KeyFrame::ComputeBoW.
//
// Reference: Thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1225-1266 (descent of one feature), :1133-1201 (the frame's
// BowVector and FeatureVector), Thirdparty/DBoW2/src/BowVector.cpp:34-46 (addWeight), :62-84 (normalize),
// Thirdparty/DBoW2/src/FeatureVector.cpp:31-45 (addFeature).  The tree is packed by voc_pack.cc (device order: siblings adjacent).
//
// Descent: one lane group per descriptor (16 lanes = one DPP row, or 32 when a node of the vocabulary has more than 16 children),
// one lane per child.  A lane loads its child's centroid (two 16-byte loads: siblings are adjacent, so a level is one coalesced read)
// and the child's own (first child, child count), and forms the key  distance << 42 | child position << 37 | count << 32 | first.
// The group's minimum is "the first child of least distance" -- (distance, position) is unique in the high bits -- and carries the
// next level's children along, so a level costs one round of loads, not two dependent ones.  The query stays in registers.
//
// Assembly: one workgroup per frame.  (word id << 13 | feature index) keys are sorted in LDS (bitonic), a scan numbers the segments of
// equal word id, one thread per segment adds the word's weight once per feature -- the sums of BowVector::addWeight in ascending
// feature order; the terms of one word are the same number -- and one wavefront adds the |values| in ascending word order, lane by lane
// (BowVector::normalize).  Both are sequential fp64 sums in the reference's order: the result equals the reference's bit for bit.
// The same sort over (node id, feature index) gives the FeatureVector as CSR.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/slamit.h"
#include "slamit_internal.h"
#include "voc_pack.h"
#include "wave_ops.h"

struct VocTree {
    const uint4* desc;       // two per device node
    const int2* kids;        // (first child, child count) per device node
    const int* orig_id;
    const int* word_id;
    const double* weight;
    int L;
};

struct slamit_voc {
    int device;
    int k, L, n_nodes, n_words, max_fanout;
    unsigned char* block;    // the one device allocation the tree's arrays live in
    VocTree tree;
};

struct VocJob {
    const uint8_t* desc; const int* n; int cap, nframes, levelsup;
    int* word_id; int* node_id;
    int* bow_n; int* bow_word; double* bow_value;
    int* fv_n; int* fv_node; int* fv_ptr; int* fv_items;
    double* w;               // workspace: the weight of every feature's word, [nframes][cap]
};

#define VOC_IDX_BITS 13      // a feature index (< 8192 > SLAMIT_VOC_MAX_FEATURES) in a sort key
#define VOC_NONE (~0ULL)

template <int G>
__global__ __launch_bounds__(256) void voc_descend_kernel(VocTree T, VocJob J) {
    const int f = blockIdx.y, sub = threadIdx.x & (G - 1);
    const int i = blockIdx.x * (256 / G) + (int)(threadIdx.x / G);
    const int n = J.n[f];
    if (n < 0 || n > J.cap || i >= n) return;      // whole lane groups leave: the group reductions below see all of their lanes
    const size_t row = (size_t)f * J.cap + i;
    const uint4* q = reinterpret_cast<const uint4*>(J.desc + 32 * row);
    const uint4 a0 = q[0], a1 = q[1];
    const int nid_level = T.L - J.levelsup;         // :1233; <= 0: the root (:1234)
    const int2 root = T.kids[0];
    int first = root.x, cnt = root.y, node = 0, nid_node = 0, level = 0;
    while (cnt > 0) {                               // :1239-1261, isLeaf() = children.empty()
        ++level;
        unsigned long long key = VOC_NONE;
        if (sub < cnt) {
            const int c = first + sub;
            const uint4 t0 = T.desc[2 * (size_t)c], t1 = T.desc[2 * (size_t)c + 1];
            const int2 kc = T.kids[c];
            const unsigned d = (unsigned)hamming256(a0, a1, t0, t1);
            key = ((unsigned long long)d << 42) | ((unsigned long long)sub << 37) | ((unsigned long long)kc.y << 32) | (unsigned)kc.x;
        }
        key = group_min_u64<G>(key);                // strict '<', first one wins (:1251)
        node = first + (int)((key >> 37) & 31u);
        cnt = (int)((key >> 32) & 31u);
        first = (int)(unsigned)key;
        if (level == nid_level) nid_node = node;    // :1258
    }
    if (nid_level > 0 && level < nid_level) nid_node = node;   // a leaf above the FeatureVector's level: its own id (slamit.h)
    if (sub == 0) {
        const double w = T.weight[node];
        J.word_id[row] = w > 0 ? T.word_id[node] : -1;          // :1164: a stopped word enters neither vector
        J.node_id[row] = T.orig_id[nid_node];
        J.w[row] = w;
    }
}

#define VOC_ASM_THREADS 1024
static size_t voc_asm_lds(int cap_pad) { return (size_t)cap_pad * 8 + 8 + ((size_t)cap_pad + 1 + 16 + 1) * 4; }

// LDS: keys[cap_pad] | norm | headpos[cap_pad + 1] | wave totals[16] | m
__global__ __launch_bounds__(VOC_ASM_THREADS) void voc_assemble_kernel(VocJob J, int cap_pad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char voc_lds[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(voc_lds);
    double* s_norm = reinterpret_cast<double*>(keys + cap_pad);
    int* headpos = reinterpret_cast<int*>(s_norm + 1);
    int* wtot = headpos + cap_pad + 1;
    int* s_m = wtot + 16;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = J.n[f];
    if (n <= 0 || n > J.cap) {                      // block-uniform
        if (tid == 0) {
            const int v = n == 0 ? 0 : -1;
            if (J.bow_n) J.bow_n[f] = v;
            if (J.fv_n) { J.fv_n[f] = v; if (n == 0) J.fv_ptr[(size_t)f * (J.cap + 1)] = 0; }
        }
        return;
    }
    const size_t base = (size_t)f * J.cap;
    const int n_pad = n <= 2 ? 2 : 1 << (32 - __clz(n - 1));   // <= cap_pad
    const int E = n_pad > VOC_ASM_THREADS ? n_pad / VOC_ASM_THREADS : 1;   // elements per thread in the scan
    for (int pass = 0; pass < 2; ++pass) {          // 0: BowVector (word ids), 1: FeatureVector (node ids)
        if (pass == 0 ? !J.bow_n : !J.fv_n) continue;
        const int* id = (pass == 0 ? J.word_id : J.node_id) + base;
        if (tid == 0) *s_m = 0;
        for (int p = tid; p < n_pad; p += VOC_ASM_THREADS) {
            unsigned long long key = VOC_NONE;
            if (p < n && J.word_id[base + p] >= 0) key = ((unsigned long long)(unsigned)id[p] << VOC_IDX_BITS) | (unsigned)p;
            keys[p] = key;
        }
        __syncthreads();
        for (int k = 2; k <= n_pad; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (n_pad >> 1); t += VOC_ASM_THREADS) {
                    const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                    const unsigned long long ka = keys[a], kb = keys[b];
                    if ((ka > kb) == ((a & k) == 0)) { keys[a] = kb; keys[b] = ka; }
                }
                __syncthreads();
            }
        // segments of equal id: number their heads, note where the valid keys end
        int cnt = 0;
        for (int e = 0; e < E; ++e) {
            const int p = tid * E + e;
            if (p >= n_pad) break;
            const unsigned long long kp = keys[p];
            if (kp == VOC_NONE) break;
            cnt += p == 0 || (kp >> VOC_IDX_BITS) != (keys[p - 1] >> VOC_IDX_BITS);
            if (p == n_pad - 1 || keys[p + 1] == VOC_NONE) *s_m = p + 1;
        }
        const int incl = wave_inclusive_scan_i32(cnt);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int j0 = incl - cnt, total = 0;
        for (int w = 0; w < VOC_ASM_THREADS / 64; ++w) { const int t = wtot[w]; total += t; if (w < wave) j0 += t; }
        for (int e = 0; e < E; ++e) {
            const int p = tid * E + e;
            if (p >= n_pad) break;
            const unsigned long long kp = keys[p];
            if (kp == VOC_NONE) break;
            if (p == 0 || (kp >> VOC_IDX_BITS) != (keys[p - 1] >> VOC_IDX_BITS)) headpos[j0++] = p;
        }
        const int m = *s_m;
        if (tid == 0) headpos[total] = m;
        __syncthreads();
        if (pass == 0) {
            for (int j = tid; j < total; j += VOC_ASM_THREADS) {
                const int p = headpos[j], len = headpos[j + 1] - p;
                const unsigned long long kp = keys[p];
                const double w = J.w[base + (int)(kp & ((1u << VOC_IDX_BITS) - 1))];
                double v = w;                        // the first feature inserts the value, the later ones add to it (BowVector.cpp:34-46)
                for (int t = 1; t < len; ++t) v += w;
                J.bow_word[base + j] = (int)(kp >> VOC_IDX_BITS);
                J.bow_value[base + j] = v;
            }
            __syncthreads();
            if (wave == 0) {                         // BowVector.cpp:62-71: norm += fabs(value) over ascending word ids, from 0.0
                double norm = 0.0;
                for (int b = 0; b < total; b += 64) {
                    const double x = b + lane < total ? fabs(J.bow_value[base + b + lane]) : 0.0;
                    const int c = min(64, total - b);
                    if (c == 64) {
#pragma unroll
                        for (int l = 0; l < 64; ++l) norm += readlane_d(x, l);
                    } else {
                        for (int l = 0; l < c; ++l) norm += readlane_d(x, l);
                    }
                }
                if (lane == 0) *s_norm = norm;
            }
            __syncthreads();
            const double norm = *s_norm;
            if (norm > 0.0)                          // :79-83
                for (int j = tid; j < total; j += VOC_ASM_THREADS) J.bow_value[base + j] /= norm;
            if (tid == 0) J.bow_n[f] = total;
        } else {
            int* ptr = J.fv_ptr + (size_t)f * (J.cap + 1);
            for (int j = tid; j <= total; j += VOC_ASM_THREADS) {
                const int p = headpos[j];
                ptr[j] = p;
                if (j < total) J.fv_node[base + j] = (int)(keys[p] >> VOC_IDX_BITS);
            }
            for (int p = tid; p < m; p += VOC_ASM_THREADS) J.fv_items[base + p] = (int)(keys[p] & ((1u << VOC_IDX_BITS) - 1));
            if (tid == 0) J.fv_n[f] = total;
        }
        __syncthreads();                             // the next pass refills keys
    }
}

static int voc_pow2_ceil(int v) { int p = 2; while (p < v) p <<= 1; return p; }

// both launches of one transform on stream st; J.cap <= SLAMIT_VOC_MAX_FEATURES, the caller has made V->device current
static hipError_t voc_launch(const slamit_voc* V, const VocJob& J, hipStream_t st) {
    const int cap_pad = voc_pow2_ceil(J.cap);
    const size_t lds = voc_asm_lds(cap_pad);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(voc_assemble_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (J.cap == 0) {
        // nothing to descend; the assembly still reports every frame (0, or -1 for a d_n outside [0, cap])
    } else if (V->max_fanout <= 16)
        hipLaunchKernelGGL(voc_descend_kernel<16>, dim3((J.cap + 15) / 16, J.nframes), dim3(256), 0, st, V->tree, J);
    else
        hipLaunchKernelGGL(voc_descend_kernel<32>, dim3((J.cap + 7) / 8, J.nframes), dim3(256), 0, st, V->tree, J);
    if (J.bow_n || J.fv_n) hipLaunchKernelGGL(voc_assemble_kernel, dim3(J.nframes), dim3(VOC_ASM_THREADS), lds, st, J, cap_pad);
    return hipGetLastError();
}

static int voc_create(const slamit_voc_desc& d, int device, slamit_voc** out, const char* where) {
    VocPacked P;
    std::string why;
    if (!voc_pack(d, P, why)) return slamit_fail(SLAMIT_ERR_ARG, (std::string(where) + ": " + why).c_str());   // before any device call
    SLAMIT_USE_DEVICE(device);
    const size_t N = (size_t)P.n_nodes + 1;
    StageLayout L;   // (only its offsets: the block is uploaded array by array)
    const StageSpan<uint8_t> sd = L.take<uint8_t>(N * SLAMIT_DESC_BYTES);
    const StageSpan<int2> sk = L.take<int2>(N);
    const StageSpan<int> so = L.take<int>(N), sw = L.take<int>(N);
    const StageSpan<double> sg = L.take<double>(N);
    std::vector<int2> kids(N);
    for (size_t i = 0; i < N; ++i) kids[i] = make_int2(P.child_first[i], P.child_count[i]);
    slamit_voc* V = new slamit_voc();
    V->device = device; V->k = P.k; V->L = P.L; V->n_nodes = P.n_nodes; V->n_words = P.n_words; V->max_fanout = P.max_fanout;
    V->block = nullptr;
    hipError_t e = hipMalloc((void**)&V->block, L.dev_bytes);
    if (e == hipSuccess) e = hipMemcpy(sd.at(V->block), P.desc.data(), sd.bytes(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(sk.at(V->block), kids.data(), sk.bytes(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(so.at(V->block), P.orig_id.data(), so.bytes(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(sw.at(V->block), P.word_id.data(), sw.bytes(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(sg.at(V->block), P.weight.data(), sg.bytes(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (V->block) hipFree(V->block);
        delete V;
        return slamit_fail_hip(e, where);
    }
    V->tree.desc = reinterpret_cast<const uint4*>(sd.at(V->block)); V->tree.kids = sk.at(V->block);
    V->tree.orig_id = so.at(V->block); V->tree.word_id = sw.at(V->block); V->tree.weight = sg.at(V->block); V->tree.L = P.L;
    *out = V;
    return SLAMIT_OK;
}

extern "C" int slamit_voc_create(const slamit_voc_desc* desc, int device, slamit_voc** out) {
    if (!desc || !out) return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_create: null argument");
    *out = nullptr;
    return voc_create(*desc, device, out, "slamit_voc_create");
}

extern "C" int slamit_voc_load_text(const char* path, int device, slamit_voc** out) {
    if (!path || !out) return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_load_text: null argument");
    *out = nullptr;
    VocArrays A;
    std::string why;
    if (!voc_load_text(path, A, why)) return slamit_fail(SLAMIT_ERR_ARG, ("slamit_voc_load_text: " + why).c_str());
    return voc_create(A.view(), device, out, "slamit_voc_load_text");
}

extern "C" void slamit_voc_destroy(slamit_voc* V) {
    if (!V) return;
    {
        SlamitDeviceGuard g(V->device);
        if (g.err == hipSuccess) { hipDeviceSynchronize(); hipFree(V->block); }
    }
    delete V;
}

extern "C" int slamit_voc_info(const slamit_voc* V, int32_t* k, int32_t* L, int32_t* n_nodes, int32_t* n_words) {
    if (!V) return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_info: null handle");
    if (k) *k = V->k;
    if (L) *L = V->L;
    if (n_nodes) *n_nodes = V->n_nodes;
    if (n_words) *n_words = V->n_words;
    return SLAMIT_OK;
}

extern "C" size_t slamit_voc_transform_workspace(int nframes, int cap) {
    if (nframes < 0 || cap < 0) return 0;
    return (size_t)nframes * cap * sizeof(double) + 256;
}

// the output pairs: all of a group or none of it
static bool voc_pairs_ok(const void* bow_n, const void* bow_word, const void* bow_value, const void* fv_n, const void* fv_node,
                         const void* fv_ptr, const void* fv_items) {
    const int b = (bow_n != nullptr) + (bow_word != nullptr) + (bow_value != nullptr);
    const int v = (fv_n != nullptr) + (fv_node != nullptr) + (fv_ptr != nullptr) + (fv_items != nullptr);
    return (b == 0 || b == 3) && (v == 0 || v == 4);
}

extern "C" int slamit_voc_transform_batch_dev(const slamit_voc* V, const uint8_t* d_desc, const int32_t* d_n, int cap, int nframes,
                                              int levelsup, int32_t* d_word_id, int32_t* d_node_id, int32_t* d_bow_n,
                                              int32_t* d_bow_word, double* d_bow_value, int32_t* d_fv_n, int32_t* d_fv_node,
                                              int32_t* d_fv_ptr, int32_t* d_fv_items, void* d_workspace, size_t workspace_bytes,
                                              void* stream) {
    if (!V || cap < 0 || nframes < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_transform_batch_dev: bad argument");
    if (nframes == 0) return SLAMIT_OK;
    if (!d_desc || !d_n || !d_word_id || !d_node_id || !d_workspace) return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_transform_batch_dev: null array");
    if (!voc_pairs_ok(d_bow_n, d_bow_word, d_bow_value, d_fv_n, d_fv_node, d_fv_ptr, d_fv_items))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_transform_batch_dev: the BowVector / FeatureVector outputs are NULL as a whole or not at all");
    if (((uintptr_t)d_desc & 15) != 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_transform_batch_dev: d_desc is not 16-byte aligned");
    if (cap > SLAMIT_VOC_MAX_FEATURES) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_voc_transform_batch_dev: cap > SLAMIT_VOC_MAX_FEATURES");
    if (workspace_bytes < slamit_voc_transform_workspace(nframes, cap))
        return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_voc_transform_batch_dev: workspace smaller than slamit_voc_transform_workspace()");
    SLAMIT_USE_DEVICE(V->device);
    VocJob J;
    J.desc = d_desc; J.n = d_n; J.cap = cap; J.nframes = nframes; J.levelsup = levelsup;
    J.word_id = d_word_id; J.node_id = d_node_id;
    J.bow_n = d_bow_n; J.bow_word = d_bow_word; J.bow_value = d_bow_value;
    J.fv_n = d_fv_n; J.fv_node = d_fv_node; J.fv_ptr = d_fv_ptr; J.fv_items = d_fv_items;
    J.w = reinterpret_cast<double*>(((uintptr_t)d_workspace + 255) & ~(uintptr_t)255);
    HIP_TRY_AT("slamit_voc_transform_batch_dev", voc_launch(V, J, (hipStream_t)stream));
    return SLAMIT_OK;
}

extern "C" int slamit_voc_transform(const slamit_voc* V, const uint8_t* desc, int n, int levelsup, int32_t* word_id, int32_t* node_id,
                                    int32_t* bow_n, int32_t* bow_word, double* bow_value, int32_t* fv_n, int32_t* fv_node,
                                    int32_t* fv_ptr, int32_t* fv_items) {
    if (!V || n < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_transform: bad argument");
    if (!voc_pairs_ok(bow_n, bow_word, bow_value, fv_n, fv_node, fv_ptr, fv_items))
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_transform: the BowVector / FeatureVector outputs are NULL as a whole or not at all");
    if (n > SLAMIT_VOC_MAX_FEATURES) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_voc_transform: n > SLAMIT_VOC_MAX_FEATURES");
    if (n == 0) {
        if (bow_n) *bow_n = 0;
        if (fv_n) { *fv_n = 0; fv_ptr[0] = 0; }
        return SLAMIT_OK;
    }
    if (!desc || !word_id || !node_id) return slamit_fail(SLAMIT_ERR_ARG, "slamit_voc_transform: null array");
    SLAMIT_USE_DEVICE(V->device);
    const size_t N = n;
    StageLayout L;
    const StageSpan<uint8_t> sd = L.take<uint8_t>(32 * N);
    const StageSpan<int> sn = L.take<int>(1);
    L.end_inputs();
    const StageSpan<int> ow = L.take<int>(N), on = L.take<int>(N), oc = L.take<int>(2);
    const StageSpan<int> bw = L.take<int>(bow_n ? N : 0);
    const StageSpan<double> bv = L.take<double>(bow_n ? N : 0);
    const StageSpan<int> fn = L.take<int>(fv_n ? N : 0), fp = L.take<int>(fv_n ? N + 1 : 0), fi = L.take<int>(fv_n ? N : 0);
    L.end_outputs();
    const StageSpan<double> ws = L.take<double>(N);
    static thread_local SlamitScratch S;
    HIP_TRY_AT("slamit_voc_transform: scratch", slamit_stage_reserve(S, V->device, L));
    memcpy(sd.at(S.host), desc, sd.bytes());
    *sn.at(S.host) = n;
    HIP_TRY_AT("slamit_voc_transform", slamit_stage_upload(S, L));
    VocJob J;
    J.desc = sd.at(S.dev); J.n = sn.at(S.dev); J.cap = n; J.nframes = 1; J.levelsup = levelsup;
    J.word_id = ow.at(S.dev); J.node_id = on.at(S.dev);
    J.bow_n = bow_n ? oc.at(S.dev) : nullptr; J.bow_word = bw.at(S.dev); J.bow_value = bv.at(S.dev);
    J.fv_n = fv_n ? oc.at(S.dev) + 1 : nullptr; J.fv_node = fn.at(S.dev); J.fv_ptr = fp.at(S.dev); J.fv_items = fi.at(S.dev);
    J.w = ws.at(S.dev);
    HIP_TRY_AT("slamit_voc_transform", voc_launch(V, J, S.st));
    HIP_TRY_AT("slamit_voc_transform", slamit_stage_download_and_wait(S, L));
    memcpy(word_id, ow.at(S.host), ow.bytes());
    memcpy(node_id, on.at(S.host), on.bytes());
    if (bow_n) {
        const int c = oc.at(S.host)[0];
        *bow_n = c;
        memcpy(bow_word, bw.at(S.host), sizeof(int) * (size_t)c);
        memcpy(bow_value, bv.at(S.host), sizeof(double) * (size_t)c);
    }
    if (fv_n) {
        const int c = oc.at(S.host)[1];
        *fv_n = c;
        memcpy(fv_node, fn.at(S.host), sizeof(int) * (size_t)c);
        memcpy(fv_ptr, fp.at(S.host), sizeof(int) * ((size_t)c + 1));
        memcpy(fv_items, fi.at(S.host), sizeof(int) * (size_t)fp.at(S.host)[c]);
    }
    return SLAMIT_OK;
}
