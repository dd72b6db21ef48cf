// voc_pack.h — host-side packing of a DBoW2 vocabulary tree for the device transform (voc.hip): the text loader of
// TemplatedVocabulary::loadFromTextFile, the validation of either input form, and the renumbering of the nodes into device order.
// Plain C++17 (no HIP): the vocabulary handle (voc.hip) and the CPU test of the packing (tests/test_voc_pack.py) both build it.
#ifndef SLAMIT_VOC_PACK_H
#define SLAMIT_VOC_PACK_H

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/slamit.h"

// A vocabulary in the array form of slamit_voc_desc, owning its arrays (what the text loader fills)
struct VocArrays {
    int32_t k = 0, L = 0, scoring = 0, weighting = 0;
    std::vector<int32_t> parent;
    std::vector<uint8_t> is_leaf;
    std::vector<uint8_t> desc;     // 32 bytes per node
    std::vector<double> weight;
    slamit_voc_desc view() const {
        slamit_voc_desc d;
        d.k = k; d.L = L; d.scoring = scoring; d.weighting = weighting; d.n_nodes = (int32_t)parent.size();
        d.parent = parent.data(); d.is_leaf = is_leaf.data(); d.desc = desc.data(); d.weight = weight.data();
        return d;
    }
};

// The tree in device order: node 0 is the root, and the children of one node are adjacent, in the order of the reference's
// `children` vector (ascending reference id: the loader pushes them in file order), which is the order that decides ties in the
// descent.  Device order is breadth first, so a level is one contiguous range.  Ids that leave the library are orig_id / word_id.
struct VocPacked {
    int32_t k = 0, L = 0, n_nodes = 0, n_words = 0;   // n_nodes without the root
    int32_t max_fanout = 0, depth = 0;                // most children of one node; deepest level (root = 0)
    std::vector<int32_t> child_first;   // device id of the first child (0 for a node without children)
    std::vector<int32_t> child_count;
    std::vector<uint8_t> desc;          // 32 bytes per device node (the root's are zero and never read)
    std::vector<int32_t> orig_id;       // the reference's node id (file order from 1, root 0)
    std::vector<int32_t> word_id;       // the reference's word id (leaves in file order), -1 for an inner node
    std::vector<double> weight;
};

// Both return false with the reason in `why`.
bool voc_load_text(const char* path, VocArrays& out, std::string& why);
bool voc_pack(const slamit_voc_desc& d, VocPacked& out, std::string& why);

#endif
