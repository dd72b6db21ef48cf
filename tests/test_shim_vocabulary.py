"""shim/ORBVocabulary.h: the reference's class surface, and (on the GPU) the C++ class over the C-ABI against api.ORBVocabulary."""
import os
import subprocess

import numpy as np
import pytest

from tests import bow_voc_ref as ref
from tests.helpers import ROOT

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
PKG = os.path.join(ROOT, "weiner_slamit_v2_amd")

DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include "ORBVocabulary.h"
using namespace ORB_SLAM2;
// driver <voc.txt> <desc.bin> <n> <levelsup>: prints size(), then both maps in iteration order (doubles as bit patterns)
int main(int argc, char** argv) {
    if (argc < 5) return 2;
    ORBVocabulary voc;
    if (!voc.empty() || voc.size() != 0) return 3;
    if (voc.loadFromTextFile(std::string(argv[1]) + ".absent")) return 4;
    if (!voc.loadFromTextFile(argv[1])) { fprintf(stderr, "%s\n", slamit_last_error()); return 5; }
    const int n = atoi(argv[3]), levelsup = atoi(argv[4]);
    cv::Mat all(n > 0 ? n : 1, 32, CV_8U);
    FILE* f = fopen(argv[2], "rb");
    if (!f || (n && fread(all.data, 32, n, f) != (size_t)n)) return 6;
    fclose(f);
    std::vector<cv::Mat> vCurrentDesc;           // Converter::toDescriptorVector: one 1 x 32 row each
    for (int i = 0; i < n; ++i) vCurrentDesc.push_back(all.row(i));
    DBoW2::BowVector mBowVec;
    DBoW2::FeatureVector mFeatVec;
    mBowVec[99] = 1.0;                           // transform() clears what it is given
    voc.transform(vCurrentDesc, mBowVec, mFeatVec, levelsup);
    printf("size %u empty %d\n", voc.size(), voc.empty() ? 1 : 0);
    for (DBoW2::BowVector::const_iterator it = mBowVec.begin(); it != mBowVec.end(); ++it) {
        unsigned long long bits;
        memcpy(&bits, &it->second, 8);
        printf("w %u %llu\n", it->first, bits);
    }
    for (DBoW2::FeatureVector::const_iterator it = mFeatVec.begin(); it != mFeatVec.end(); ++it) {
        printf("n %u", it->first);
        for (size_t j = 0; j < it->second.size(); ++j) printf(" %u", it->second[j]);
        printf("\n");
    }
    return 0;
}
'''


def _build():
    from weiner_slamit_v2_amd import build as hb

    hb.build()
    subprocess.check_call(["make", "-s", "-C", SHIM, "-f", "Makefile", "all"])


def test_shim_header_keeps_the_reference_surface():
    _build()
    hdr = open(os.path.join(SHIM, "ORBVocabulary.h")).read()
    for want in ("class ORBVocabulary", "bool loadFromTextFile(const std::string& filename)",
                 "void transform(const std::vector<cv::Mat>& features, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const",
                 "unsigned int size() const", "bool empty() const", "typedef std::map<WordId, WordValue> BowVector;",
                 "typedef std::map<NodeId, std::vector<unsigned int> > FeatureVector;", '#include "cvlite.h"'):
        assert want in hdr, want
    mk = open(os.path.join(SHIM, "Makefile")).read()
    assert "ORBVocabulary.h" in mk


@pytest.mark.gpu
def test_shim_vocabulary_matches_the_binding(tmp_path):
    from weiner_slamit_v2_amd import api

    _build()
    src, exe = str(tmp_path / "driver.cc"), str(tmp_path / "driver")
    open(src, "w").write(DRIVER)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-I", SHIM, src, "-o", exe, "-L", PKG, "-lslamit_hip", "-L", rocm + "/lib",
                           "-Wl,-rpath-link," + rocm + "/lib", "-Wl,-rpath," + PKG, "-Wl,-rpath," + rocm + "/lib"])
    voc = ref.full_tree(6, 3, 31, stop_frac=0.2)
    q = ref.queries(voc, 500, 32)
    vp, dp = str(tmp_path / "voc.txt"), str(tmp_path / "desc.bin")
    ref.write_text(voc, vp)
    q.tofile(dp)
    v = api.ORBVocabulary.load_text(vp)
    for levelsup in (1, 4):
        out = subprocess.check_output([exe, vp, dp, str(len(q)), str(levelsup)]).decode().splitlines()
        r = v.transform(q, levelsup)
        assert out[0] == "size %d empty 0" % v.info()["n_words"]
        bow = [ln.split()[1:] for ln in out if ln.startswith("w ")]
        fv = [[int(x) for x in ln.split()[1:]] for ln in out if ln.startswith("n ")]
        assert [int(b[0]) for b in bow] == r["bow_word"].tolist() and len(bow) > 50
        assert np.array_equal(np.array([int(b[1]) for b in bow], np.uint64), r["bow_value"].view(np.uint64))
        assert [f[0] for f in fv] == r["fv_node"].tolist()
        for j, f in enumerate(fv):
            assert f[1:] == r["fv_items"][r["fv_ptr"][j]:r["fv_ptr"][j + 1]].tolist()
        same = ref.Vocabulary(voc).transform(q, levelsup)
        assert np.array_equal(same["bow_value"].view(np.uint64), r["bow_value"].view(np.uint64)) and np.array_equal(same["fv_items"], r["fv_items"])
    v.close()
