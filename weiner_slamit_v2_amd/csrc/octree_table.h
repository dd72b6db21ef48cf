// octree_table.h — the part of DistributeOctTree (ORBextractor.cc:552-776) that does not need the keys, shared by octree_kernel
// (orb_kernels.hip) and tests/test_octree_table.py (through a g++ driver).  Plain integer C++ outside a HIP compile.
//
// The result of the octree pass depends on the keys only through
//   * the population of every (root, depth, quadrant path), and
//   * per leaf of the final list, the key with the largest response, the first such key in vToDistributeKeys order.
// A key's quadrant path below its root follows from the root's box alone (a child's box follows from its parent's), so ONE sweep
// over the keys can fill a path table down to depth FD: a histogram of the depth-FD paths, from which the shallower populations are
// sums of four, and per depth-FD bin the best key as a packed u64.  While no node that has to be split lies at depth FD already, a
// pass -- one that splits every expandable node as well as a "largest first" one -- takes its children's populations from the
// table, and when the loop ends there every non-empty bin hands its best key to the node that covers it.  A pass that needs depth
// FD + 1 leaves the table: the caller then runs the walk over the keys from the start.
//
// Table layout per root: HS = 4 + 16 + .. + 4^FD ints, depth d (1 .. FD) at oct_depth_off(d), 4^d entries indexed by the path
// (two bits per depth, the shallowest quadrant in the highest bits).  A node of the list is the code root << 16 | depth << 12 | path.
#ifndef SLAMIT_OCTREE_TABLE_H
#define SLAMIT_OCTREE_TABLE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define OCT_HD __host__ __device__ __forceinline__
#else
#define OCT_HD static inline
#endif

#define OCT_FD_MAX 4   // deepest table: 340 ints and 256 best keys per root

struct Box16 { short x0, y0, x1, y1; };

OCT_HD int box_quadrant(const Box16& b, int x, int y, int* mx, int* my) {
    int midx = b.x0 + ((b.x1 - b.x0 + 1) >> 1);  // UL.x + ceil((UR.x-UL.x)/2)
    int midy = b.y0 + ((b.y1 - b.y0 + 1) >> 1);
    *mx = midx; *my = midy;
    return (x < midx ? 0 : 1) + (y < midy ? 0 : 2);  // 0:n1 1:n2 2:n3 3:n4
}
OCT_HD Box16 child_box(const Box16& b, int q) {
    int midx = b.x0 + ((b.x1 - b.x0 + 1) >> 1);
    int midy = b.y0 + ((b.y1 - b.y0 + 1) >> 1);
    Box16 c;
    c.x0 = (q & 1) ? midx : b.x0; c.x1 = (q & 1) ? b.x1 : midx;
    c.y0 = (q & 2) ? midy : b.y0; c.y1 = (q & 2) ? b.y1 : midy;
    return c;
}

// depth of the path table: the deepest of 4, 3, 2 whose table (4 + .. + 4^depth ints per root) fits `room` ints; 0 = no table
OCT_HD int nIniFD(int nIni, int room) {
    return nIni * 340 <= room ? 4 : nIni * 84 <= room ? 3 : nIni * 20 <= room ? 2 : 0;
}
OCT_HD int oct_table_ints(int FD) { return ((4 << (2 * FD)) - 4) / 3; }                  // HS: 4 + 16 + .. + 4^FD
OCT_HD int oct_depth_off(int d) { return ((4 << (2 * d)) - 4) / 3 - (1 << (2 * d)); }   // first entry of depth d (>= 1) in a root's table
OCT_HD int oct_bins(int FD) { return 1 << (2 * FD); }                                    // depth-FD paths per root
// the table path also needs the per-bin best keys, 8 bytes each, in `key_bytes` of LDS, and ranks the nodes of a "largest first"
// pass by population << 12 | (4095 - list position) in 32 bits
#define OCT_TABLE_KEYS_MAX (1 << 20)
OCT_HD bool oct_table_fits(int nIni, int FD, long key_bytes, int n_keys) {
    return FD > 0 && (long)nIni * 8 * oct_bins(FD) <= key_bytes && n_keys < OCT_TABLE_KEYS_MAX;
}
OCT_HD unsigned oct_rank_key(int cnt, int pos) { return ((unsigned)cnt << 12) | (unsigned)(4095 - pos); }   // larger = split sooner

// vpIniNodes[kp.pt.x / hX], ORBextractor.cc:582 (the last root also takes what float rounding puts behind it)
OCT_HD int oct_key_root(int x, float hX, int nIni) {
    const int r = (int)((float)x / hX);
    return r < nIni - 1 ? r : nIni - 1;
}
// quadrant path of (x, y) from the root's box down to depth FD
OCT_HD int oct_key_path(Box16 b, int x, int y, int FD) {
    int path = 0;
    for (int d = 0; d < FD; ++d) {
        int mx, my;
        const int q = box_quadrant(b, x, y, &mx, &my);
        b = child_box(b, q);
        path = path * 4 + q;
    }
    return path;
}

// the pick of a leaf is the maximum of this key: largest response, then the earliest position in vToDistributeKeys
OCT_HD unsigned long long oct_pick_key(unsigned response, unsigned order) {
    return ((unsigned long long)response << 32) | (0xFFFFFFFFu - order);
}
OCT_HD unsigned oct_pick_response(unsigned long long k) { return (unsigned)(k >> 32); }
OCT_HD unsigned oct_pick_order(unsigned long long k) { return 0xFFFFFFFFu - (unsigned)k; }

OCT_HD int oct_code(int root, int depth, int path) { return (root << 16) | (depth << 12) | path; }
OCT_HD int oct_code_root(int c) { return c >> 16; }
OCT_HD int oct_code_depth(int c) { return (c >> 12) & 15; }
OCT_HD int oct_code_path(int c) { return c & 4095; }
OCT_HD int oct_code_child(int c, int q) { return oct_code(oct_code_root(c), oct_code_depth(c) + 1, 4 * oct_code_path(c) + q); }
// index of the population of node `c`'s child q in the table (c at depth < FD)
OCT_HD int oct_child_slot(int c, int q, int HS) {
    return oct_code_root(c) * HS + oct_depth_off(oct_code_depth(c) + 1) + 4 * oct_code_path(c) + q;
}
// index of node `c` itself (depth >= 1)
OCT_HD int oct_node_slot(int c, int HS) { return oct_code_root(c) * HS + oct_depth_off(oct_code_depth(c)) + oct_code_path(c); }

// A pass can be served from the table when every node it may split (population > 1) has its children in it: depth + 1 <= FD.
OCT_HD bool oct_node_leaves_table(int cnt, int code, int FD) { return cnt > 1 && oct_code_depth(code) >= FD; }

// populations of the paths shallower than FD from the depth-FD histogram, one root's table
OCT_HD void oct_table_sum_up(int* tab, int FD) {
    for (int d = FD - 1; d >= 1; --d)
        for (int p = 0; p < (1 << (2 * d)); ++p) {
            const int* c = &tab[oct_depth_off(d + 1) + 4 * p];
            tab[oct_depth_off(d) + p] = (c[0] + c[1]) + (c[2] + c[3]);
        }
}

// the word octree_kernel leaves for slamit_orb_debug_octree_path: the passes served from the table, and whether the workgroup
// left it (and walked the keys from the start)
#define OCT_PATH_LEFT 0x100
OCT_HD int oct_path_word(int passes, bool left) { return (passes & 0xFF) | (left ? OCT_PATH_LEFT : 0); }

enum { OCT_EXIT_AT_ONCE = 0, OCT_EXIT_SORTED_STAGE = 1, OCT_EXIT_EXHAUSTED = 2 };   // how the loop ended (:682, :747)

struct OctSeqResult {
    int n;          // nodes of the final list (finished inside the table), in list order in code[] / key[]
    int passes;     // passes served from the table
    int exit;       // OCT_EXIT_*, when finished
    int left_at;    // 0: finished inside the table; p >= 1: pass p (counted from 1) needed depth FD + 1
};

// The whole pass on one thread, from the tables alone: the specification of octree_kernel's table path.
//   hist      nIni * HS ints, every depth filled (oct_table_sum_up)
//   bin_best  nIni * 4^FD pick keys, the maximum of each depth-FD bin (anything where the bin is empty)
//   N         the level's quota, cap >= max(N, 4 nIni) + 4 the node capacity
//   code      [2 * cap]  out: code[0 .. n) the final list, front of the reference's std::list first
//   key       [cap]      out: the pick key of each node
//   work      [8 * cap]  scratch
// List order as in the kernel: children go to the front, so after a pass the list is reverse(creation order of the new children)
// ++ (surviving old nodes in old order); "largest first" ranks by (population desc, list position asc).
OCT_HD OctSeqResult oct_table_seq(int nIni, int FD, const int* hist, const unsigned long long* bin_best, int N, int cap,
                                  int* code, unsigned long long* key, int* work) {
    OctSeqResult res; res.n = 0; res.passes = 0; res.exit = -1; res.left_at = 0;
    const int HS = oct_table_ints(FD);
    int* cnt = work;                 // [2 * cap]
    int* childcnt = work + 2 * cap;  // [4 * cap]
    int* rankv = work + 6 * cap;     // [cap]
    int* sorted = work + 7 * cap;    // [cap]
    int cur = 0, n = 0;
    if (FD <= 0) { res.left_at = 1; return res; }
    for (int r = 0; r < nIni; ++r) {   // roots without keys are erased, the others keep their order (:586-598)
        const int* t = &hist[r * HS];
        const int c = (t[0] + t[1]) + (t[2] + t[3]);
        if (c > 0) { code[n] = oct_code(r, 0, 0); cnt[n] = c; ++n; }
    }
    bool finish = n == 0, careful = false;
    while (!finish) {
        const int prevSize = n;
        const int* ccode = code + cur * cap; const int* ccnt = cnt + cur * cap;
        int* ncode = code + (cur ^ 1) * cap; int* ncnt = cnt + (cur ^ 1) * cap;
        for (int i = 0; i < n; ++i)
            if (oct_node_leaves_table(ccnt[i], ccode[i], FD)) { res.left_at = res.passes + 1; return res; }
        for (int i = 0; i < n; ++i)
            for (int q = 0; q < 4; ++q) childcnt[4 * i + q] = ccnt[i] > 1 ? hist[oct_child_slot(ccode[i], q, HS)] : 0;
        int kproc = 0;
        if (careful) {
            int m = 0;
            for (int i = 0; i < n; ++i) {
                rankv[i] = -1;
                if (ccnt[i] <= 1) continue;
                int r = 0;
                for (int j = 0; j < n; ++j) r += ccnt[j] > 1 && oct_rank_key(ccnt[j], j) > oct_rank_key(ccnt[i], i);
                rankv[i] = r; sorted[r] = i; ++m;
            }
            kproc = m;
            int size = n;
            for (int s = 0; s < m; ++s) {   // split in rank order until the list reaches N (:745-751)
                const int* cc = &childcnt[4 * sorted[s]];
                size += (cc[0] > 0) + (cc[1] > 0) + (cc[2] > 0) + (cc[3] > 0) - 1;
                if (size >= N) { kproc = s + 1; break; }
            }
        }
        int m_new = 0, nToExpand = 0;
        const int nsplit = careful ? kproc : n;
        for (int e = 0; e < 4 * nsplit; ++e) {
            const int i = careful ? sorted[kproc - 1 - (e >> 2)] : n - 1 - (e >> 2), q = 3 - (e & 3);
            const int cc = childcnt[4 * i + q];
            if (ccnt[i] > 1 && cc > 0) {
                if (m_new < cap) { ncode[m_new] = oct_code_child(ccode[i], q); ncnt[m_new] = cc; }
                ++m_new;
                nToExpand += cc > 1;
            }
        }
        for (int i = 0; i < n; ++i) {
            const bool stays = careful ? !(rankv[i] >= 0 && rankv[i] < kproc) : ccnt[i] <= 1;
            if (stays) {
                if (m_new < cap) { ncode[m_new] = ccode[i]; ncnt[m_new] = ccnt[i]; }
                ++m_new;
            }
        }
        cur ^= 1;
        n = m_new < cap ? m_new : cap;
        ++res.passes;
        if (n >= N || n == prevSize) {
            finish = true;
            res.exit = n >= N ? (careful ? OCT_EXIT_SORTED_STAGE : OCT_EXIT_AT_ONCE) : OCT_EXIT_EXHAUSTED;
        } else if (!careful && n + nToExpand * 3 > N) careful = true;
    }
    // every non-empty bin hands its best key to the node that covers it (the list's nodes are disjoint)
    const int nb = oct_bins(FD);
    for (int i = 0; i < n; ++i) key[i] = 0ull;
    for (int i = 0; i < n; ++i) {
        const int c = code[cur * cap + i], r = oct_code_root(c), d = oct_code_depth(c), sh = 2 * (FD - d);
        const int first = oct_code_path(c) << sh;
        for (int b = first; b < first + (1 << sh); ++b)
            if (hist[r * HS + oct_depth_off(FD) + b] > 0 && bin_best[r * nb + b] > key[i]) key[i] = bin_best[r * nb + b];
    }
    if (cur) for (int i = 0; i < n; ++i) code[i] = code[cap + i];
    res.n = n;
    return res;
}

#endif
