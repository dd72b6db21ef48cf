"""The checker of the stereo triangulation on the CPU (tests/triangulate_stereo_ref.py): the fixtures are admissible by the
reference's restatement alone, and tri_pair_stereo of csrc/triangulate.h, built with g++ for the host, agrees with it.

Measured on the fixtures: 0 undecided pairs of 2,122; Y = 5.62e-8 (bound 4 Y = 2.25e-7); the unprojected points
of the g++-built header equal ref32's bit for bit; with every ur = -1 tri_pair_stereo returns tri_pair's status and bits on the
twelve monocular fixtures of tests/triangulate_ref.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import test_triangulate_ref as base
from tests import triangulate_ref as mono
from tests import triangulate_stereo_ref as ref

HOST_DRIVER = r'''
#include <stdio.h>
#include <string.h>
#include <vector>
#include "triangulate.h"
// stereo <in> <out>: a problem followed by its stereo side -> status (n bytes), source (n bytes), X (3 n floats)
// both <in> <out>: the same input -> tri_pair's status and X, then tri_pair_stereo's with every ur = -1
int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    FILE* o = fopen(argv[3], "wb");
    if (!f || !o) return 2;
    int hdr[2];
    if (fread(hdr, 4, 2, f) != 2) return 2;
    const int n = hdr[0], nl = hdr[1];
    TriView c1, c2;
    float rf, mbbf[3];
    std::vector<float> sf1(nl), s1(nl), sf2(nl), s2(nl), kp1(2 * n), kp2(2 * n), ur1(n), ur2(n), dp1(n), dp2(n), raw1(2 * n), raw2(2 * n);
    std::vector<int> o1(n), o2(n);
    size_t got = fread(c1.T, 4, 12, f) + fread(c2.T, 4, 12, f) + fread(&c1.fx, 4, 6, f) + fread(&c2.fx, 4, 6, f) + fread(&rf, 4, 1, f);
    got += fread(sf1.data(), 4, nl, f) + fread(s1.data(), 4, nl, f) + fread(sf2.data(), 4, nl, f) + fread(s2.data(), 4, nl, f);
    got += fread(kp1.data(), 4, 2 * n, f) + fread(kp2.data(), 4, 2 * n, f) + fread(o1.data(), 4, n, f) + fread(o2.data(), 4, n, f);
    got += fread(mbbf, 4, 3, f) + fread(ur1.data(), 4, n, f) + fread(ur2.data(), 4, n, f) + fread(dp1.data(), 4, n, f) + fread(dp2.data(), 4, n, f);
    got += fread(raw1.data(), 4, 2 * n, f) + fread(raw2.data(), 4, 2 * n, f);
    if (got != (size_t)(40 + 4 * nl + 14 * n)) return 2;
    tri_centre(c1); tri_centre(c2);
    std::vector<unsigned char> st(n), src(n), st0(n);
    std::vector<float> X(3 * n), X0(3 * n);
    const bool both = !strcmp(argv[1], "both");
    for (int i = 0; i < n; ++i) {
        TriStereoPair s = {ur1[i], ur2[i], dp1[i], dp2[i], {raw1[2 * i], raw1[2 * i + 1]}, {raw2[2 * i], raw2[2 * i + 1]}};
        if (both) {
            s.ur1 = -1.f; s.ur2 = -1.f;
            st0[i] = (unsigned char)tri_pair(c1, c2, &kp1[2 * i], &kp2[2 * i], s1[o1[i]], s2[o2[i]], sf1[o1[i]], sf2[o2[i]], rf, &X0[3 * i]);
        }
        int source;
        st[i] = (unsigned char)tri_pair_stereo(c1, c2, &kp1[2 * i], &kp2[2 * i], s, mbbf[0], mbbf[1], mbbf[2], s1[o1[i]], s2[o2[i]], sf1[o1[i]],
                                               sf2[o2[i]], rf, &X[3 * i], source);
        src[i] = (unsigned char)source;
    }
    if (both) { fwrite(st0.data(), 1, n, o); fwrite(X0.data(), 4, 3 * n, o); }
    fwrite(st.data(), 1, n, o); fwrite(src.data(), 1, n, o); fwrite(X.data(), 4, 3 * n, o);
    fclose(f); fclose(o);
    return 0;
}
'''


def stereo_blob(pr):
    f32 = np.float32
    parts = [base.problem_blob(pr), struct.pack("<fff", float(pr["mb1"]), float(pr["mb2"]), float(pr["bf"]))]
    for key in ref.STEREO_KEYS:
        parts.append(np.ascontiguousarray(pr[key], f32).tobytes())
    return b"".join(parts)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("tri_stereo_host")
    open(str(d / "host.cc"), "w").write(HOST_DRIVER)
    out = str(d / "host")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-I", base.CSRC, str(d / "host.cc"), "-o", out])
    return out


def host_stereo(exe, tmp_path, pr, both=False):
    """-> (status, source, x3d) of tri_pair_stereo; with both=True (status0, x0) of tri_pair come first and every ur is -1."""
    n = int(pr["n"])
    open(str(tmp_path / "in.bin"), "wb").write(stereo_blob(pr))
    subprocess.check_call([exe, "both" if both else "stereo", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(str(tmp_path / "out.bin"), "rb").read()
    out = []
    if both:
        out += [np.frombuffer(raw[:n], np.uint8).copy(), np.frombuffer(raw[n:13 * n], np.float32).reshape(n, 3).copy()]
        raw = raw[13 * n:]
    return tuple(out + [np.frombuffer(raw[:n], np.uint8).copy(), np.frombuffer(raw[n:2 * n], np.uint8).copy(),
                        np.frombuffer(raw[2 * n:], np.float32).reshape(n, 3).copy()])


def special_counts(a):
    """The outcomes the fixtures must hold, counted over the decided pairs of one analysis."""
    r, d = a["r32"], a["decided"]
    s1, s2 = r["stereo1"], r["stereo2"]
    c = dict(kinds=[int((~s1 & ~s2).sum()), int((s1 & ~s2).sum()), int((~s1 & s2).sum()), int((s1 & s2).sum())],
             above_9998=int((d & (r["source"] == 1) & (s1 | s2) & (r["cosp"] >= 0.9998)).sum()),
             both_unproject1=int((d & s1 & s2 & (r["source"] == 2)).sum()), third_term_alone=0, between_5991_and_78=0)
    for side, code in (("1", 5), ("2", 6)):
        st, sg, e2, e3 = r["stereo" + side], r["sigma2_" + side], r["err2_" + side], r["err3_" + side]
        with np.errstate(invalid="ignore"):
            c["third_term_alone"] += int((d & st & (r["status"] == code) & (e2 < 5.991 * sg) & (e3 > 7.8 * sg)).sum())
            passed = (r["status"] == 0) | (r["status"] > code)
            c["between_5991_and_78"] += int((d & st & passed & (e2 > 5.991 * sg) & (e2 < 7.8 * sg)).sum())
    return c


def test_fixtures_are_admissible():
    """By the reference alone: at most 2 % undecided pairs per fixture and overall, no status or source disagreement among the
    variants on decided pairs, every status 0, 1, 3, 4, 5, 6, 8 and every source 1, 2, 3 among them, and the stereo outcomes."""
    seen_st, seen_src = set(), set()
    total = undecided = 0
    tot = dict(above_9998=0, both_unproject1=0, third_term_alone=0, between_5991_and_78=0)
    for k in range(len(ref.FIXTURES)):
        assert int(ref.fixture(k)["n"]) <= 300
        a = ref.admissibility(k)
        n = len(a["decided"])
        total += n
        undecided += int((~a["decided"]).sum())
        d = a["decided"]
        c = special_counts(a)
        print("fixture %d: n %d, undecided %d, codes %s, sources %s, %s" % (k, n, int((~d).sum()), np.bincount(a["r32"]["status"][d], minlength=10).tolist(),
                                                                             np.bincount(a["r32"]["source"][d], minlength=4).tolist(), c))
        assert a["undecided_frac"] <= 0.02, (k, a["undecided_frac"])
        for key in ("status", "source"):
            assert np.array_equal(a["r32"][key][d], a["r32j"][key][d]) and np.array_equal(a["r32"][key][d], a["r64"][key][d]), (k, key)
        seen_st |= set(int(s) for s in a["r32"]["status"][d])
        seen_src |= set(int(s) for s in a["r32"]["source"][d])
        for key in tot:
            tot[key] += c[key]
        if k == ref.MIXED:                                      # all four kinds inside single wavefronts of the fixture the size cuts come from
            r = a["r32"]
            kind = r["stereo1"].astype(int) + 2 * r["stereo2"].astype(int)
            for w in range(0, n - 63, 64):
                assert set(kind[w:w + 64].tolist()) == {0, 1, 2, 3}, w
                assert set(r["source"][w:w + 64].tolist()) >= {1, 2, 3}, w
    print("undecided %d of %d, Y = %.3e, %s" % (undecided, total, ref.yardstick(), tot))
    assert undecided <= 0.02 * total
    assert seen_st == {0, 1, 3, 4, 5, 6, 8}, seen_st
    assert seen_src == {0, 1, 2, 3}, seen_src
    assert min(tot.values()) >= 1, tot
    assert 0 < ref.yardstick() < 1e-6


def test_the_stereo_cosine_is_not_the_identity_in_the_restatement():
    """The restatement evaluates cos(2 atan2(mb / 2, depth)) as a chain; the header's identity agrees with it to float rounding:
    3.3e-7 absolute over the depths of a rig, which is what makes a cosine comparison undecided, never wrong."""
    rs = np.random.RandomState(5)
    mb, dp = rs.uniform(0.05, 0.6, 20000).astype(np.float32), np.exp(rs.uniform(np.log(0.3), np.log(60.0), 20000)).astype(np.float32)
    chain = np.cos(np.float32(2) * np.arctan2(mb / np.float32(2), dp)).astype(np.float32)
    h = (mb / np.float32(2)).astype(np.float64)
    ident = ((dp.astype(np.float64) ** 2 - h * h) / (dp.astype(np.float64) ** 2 + h * h)).astype(np.float32)
    assert np.abs(chain.astype(np.float64) - ident).max() <= 3.3e-7


@pytest.mark.parametrize("k", range(len(ref.FIXTURES)))
def test_the_header_on_the_host_agrees_with_the_restatement(exe, tmp_path, k):
    """Statuses and sources equal ref32j's on every decided pair, triangulated points within 4 Y of ref64, unprojected points equal
    ref32's bit for bit."""
    pr, a = ref.fixture(k), ref.admissibility(k)
    st, src, x = host_stereo(exe, tmp_path, pr)
    check_against(a, st, src, x)


def check_against(a, st, src, x, n=None):
    """A result (header on the host, or device) against the analysis a, cut to its first n pairs; -> the largest e."""
    n = len(st) if n is None else n
    d = a["decided"][:n]
    assert st.shape == (n,) and src.shape == (n,) and x.shape == (n, 3)
    assert np.array_equal(st[d], a["r32j"]["status"][:n][d]), np.flatnonzero(d & (st != a["r32j"]["status"][:n]))
    assert np.array_equal(src[d], a["r32j"]["source"][:n][d]), np.flatnonzero(d & (src != a["r32j"]["source"][:n]))
    acc = (st == 0) & (src == 1) & a["all_accept"][:n]
    e = mono.point_error({"A": a["r64"]["A"][:n], "x3d": a["r64"]["x3d"][:n]}, x)
    worst = float(e[acc].max()) if acc.any() else 0.0
    print("e max %.3e over %d triangulated points, bound %.3e" % (worst, int(acc.sum()), 4 * ref.yardstick()))
    assert np.all(e[acc] <= 4 * ref.yardstick())
    un = d & (src >= 2)
    assert np.array_equal(x[un].view(np.uint32), a["r32"]["x3d"][:n][un].view(np.uint32))
    assert np.all(x[src == 0] == 0) and np.all((src == 0) == ((st == 1) | (st == 2) | (st == 9)))
    return worst


@pytest.mark.parametrize("k", range(len(mono.FIXTURES)))
def test_without_stereo_keypoints_it_is_tri_pair(exe, tmp_path, k):
    """Every ur = -1: status and the bits of X are tri_pair's on the twelve monocular fixtures."""
    pr = ref.with_mono_stereo(mono.fixture(k))
    st0, x0, st, src, x = host_stereo(exe, tmp_path, pr, both=True)
    assert np.array_equal(st0, st) and np.array_equal(x0.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(src, np.where((st == 1) | (st == 2), 0, 1))
    a = mono.admissibility(k)
    assert np.array_equal(st[a["decided"]], a["r32j"]["status"][a["decided"]])
    r = ref.evaluate(mono.fixture(k), "32j")                     # the stereo restatement without stereo keypoints is the monocular one
    assert np.array_equal(r["status"], a["r32j"]["status"]) and np.array_equal(r["x3d"].view(np.uint32), a["r32j"]["x3d"].view(np.uint32))


def test_hand_made_single_pairs(exe, tmp_path):
    """One pair per stereo branch: ur == 0.0f is stereo, depth <= 0 on the chosen keypoint is code 9 with X zero, rays more than
    90 degrees apart, the else-if of the cosines, the dropped 0.9998 gate, the 7.8 three-term gate, bf on keyframe 2, mvKeys."""
    cases = ref.hand_cases()
    for name, (pr, want_st, want_src) in cases.items():
        a = ref.analyse(pr)
        assert a["decided"][0], name
        st, src, x = host_stereo(exe, tmp_path, pr)
        print("%-62s status %d source %d X %s" % (name, st[0], src[0], x[0]))
        assert st[0] == a["r32j"]["status"][0] and src[0] == a["r32j"]["source"][0], name
        assert src[0] == want_src and (want_st is None or st[0] == want_st), (name, st[0], src[0])
        if st[0] in (1, 2, 9):
            assert np.all(x[0] == 0), name
        if src[0] >= 2:
            assert np.array_equal(x[0].view(np.uint32), a["r32"]["x3d"][0].view(np.uint32)), name
    x = host_stereo(exe, tmp_path, cases["UnprojectStereo reads mvKeys"][0])[2][0]
    assert abs(x[0] - (21.0 - 320.0) / 500.0 * 4.0) < 1e-5 and abs(x[1] - (256.5 - 240.0) / 500.0 * 4.0) < 1e-5
