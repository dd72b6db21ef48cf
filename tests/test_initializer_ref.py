"""The Initializer restatement (tests/initializer_ref.py) and the g++-built csrc/two_view.h on the CPU.

Measured on the CPU over the eleven fixtures (891 sets, each solved for H and for F):
  admission   variants A (float64 svd) and B (float64 eigh of A^T A) give the same H on every set (gap 0) and F within 8.2e-8;
              the bound is ADMIT = 2^-23 and every hypothesis is admitted.  C (numpy's float32 svd) lies up to 1.9e-5 from A on F:
              what a float decomposition would cost.
  decided     A and B agree on the best H and F hypothesis, the side of RH = 0.40 (|RH - 0.40| >= 0.06), the winning motion and
              the return value of every fixture.
  header      the g++-built header against A: models of admitted hypotheses 0, motions R, t 3.6e-7, accepted points of the winning
              motion 7.1e-6 (relative to max(1, |entry|)): ref.HOST_GAP.  No match of any motion lies within 1e-3 of a gate;
              statuses, best hypotheses, model choice, winning motion, return value and vbTriangulated are equal.
"""
import numpy as np
import pytest

from tests import initializer_ref as ref

f32, f64 = np.float32, np.float64
DECIDED = 1e-3      # a match is decided when no gate it met is closer than this, relatively (ref.check_rt's margin)


def rel(x, a):
    return np.abs(np.asarray(x, f64) - np.asarray(a, f64)) / np.maximum(1, np.abs(a))


@pytest.mark.parametrize("name", ref.NAMES)
def test_fixture_is_admitted_and_decided(name):
    a, b, adm = ref.initialize(name, "A"), ref.initialize(name, "B"), ref.admitted(name)
    gaps = [ref.model_gap(a["models"][k], b["models"][k]).max() for k in (ref.H, ref.F)]
    print("%s: A-B model gap H %.3g F %.3g, admitted %d of %d" % (name, gaps[0], gaps[1], adm.sum(), adm.size))
    assert adm.mean() >= 0.98                                    # §11's cap on unadmitted hypotheses
    assert a["best"] == b["best"]
    assert np.isfinite(a["RH"]) and abs(float(a["RH"]) - 0.40) >= 0.02 and abs(float(b["RH"]) - 0.40) >= 0.02
    assert (a["kind"], a["motion"], a["ok"]) == (b["kind"], b["motion"], b["ok"])
    kind, ok = ref.fixture(name)["expect"]
    assert a["ok"] == ok and kind in (None, a["kind"])


def test_fixtures_fail_for_the_reason_they_are_named_for():
    rot, few, amb, eight = (ref.initialize(n, "A") for n in ("rotation", "few", "ambiguous", "eight"))
    assert max(rot["n_good"]) > 0.9 * rot["N"] and max(rot["parallax"][:4]) < 1.0           # triangulates, but under one degree
    assert max(few["n_good"]) >= 0.9 * few["N"] and max(few["n_good"]) < 50                  # minTriangulated
    assert sum(1 for g in few["n_good"] if g > 0.7 * max(few["n_good"])) == 1
    s = sorted(amb["n_good"])
    assert s[-2] >= 0.75 * s[-1] and s[-1] > 50 and s[-1] > 0.9 * amb["N"] and max(amb["parallax"]) > 1.0   # only the second best stands in the way
    assert eight["best"][ref.H] == -1 and eight["SH"] == 0                                    # no homography score above 0
    assert len(ref.fixture("eight")["matches"]) == 8 and len(ref.fixture("eight")["sets"]) == 1


def test_float32_svd_is_recorded():
    worst = 0.0
    for name in ("general", "planar"):
        c = ref.models(ref.fixture(name), "C")
        worst = max(worst, max(ref.model_gap(c[k], ref.initialize(name, "A")["models"][k]).max() for k in (ref.H, ref.F)))
    print("variant C (float32 svd) against A: %.3g" % worst)
    assert worst > ref.ADMIT                                     # recorded, not a yardstick: it would cost this much


@pytest.mark.parametrize("name", ref.NAMES)
def test_header_against_variant_a(name):
    pr, a, adm = ref.fixture(name), ref.initialize(name, "A"), ref.admitted(name)
    hyp, pick, reco = ref.host_initialize(name)
    nm = len(a["n_good"])
    g_model = rel(hyp["model"], a["models"])[adm].max()
    g_pose = max(rel(reco["R"][:nm].reshape(nm, 3, 3), a["R"]).max(), rel(reco["t"][:nm], a["t"]).max())
    print("%s: header against A: model %.3g pose %.3g" % (name, g_model, g_pose))
    assert g_model <= ref.HOST_GAP["model"] and g_pose <= ref.HOST_GAP["pose"]
    assert (pick["best_h"], pick["best_f"]) == tuple(a["best"])
    assert (pick["kind"], pick["N"], pick["motion"]) == (a["kind"], a["N"], a["motion"])
    assert reco["decomposable"] == a["decomposable"]
    for kind in (ref.H, ref.F):                                  # counts and bits are the restated check on the header's own matrix
        for h in range(0, hyp["model"].shape[1], 7):
            score, inl = ref.check(kind, hyp["model"][kind, h], ref.m12_of(pr), pr["sigma"])
            assert hyp["score"][kind, h].view(np.uint32) == score.view(np.uint32) and hyp["n_inliers"][kind, h] == inl.sum()
            assert np.array_equal(ref.unpack_bits(hyp["inlier_bits"][kind, h], len(inl)), inl)
    n = len(pr["matches"])
    for mi, c in enumerate(a["rt"]):
        dec = c["margin"] > DECIDED
        assert np.array_equal(reco["status"][mi][dec], c["status"][dec])
        assert np.array_equal(ref.unpack_bits(reco["good_bits"][mi], n)[dec], c["good"][dec])
        assert dec[a["subset"]].all()                            # measured: every match of every fixture is decided
        assert reco["n_good"][mi] == c["n_good"]
    if a["ok"]:
        mi = a["motion"]
        c = a["rt"][mi]
        acc = c["status"] == ref.RT_OK
        g_pts = rel(reco["points"][mi][acc], c["points"][acc]).max()
        print("%s: accepted points of the winning motion against A: %.3g" % (name, g_pts))
        assert g_pts <= ref.HOST_GAP["points"]
        vb = np.zeros(len(pr["keys1"]), bool)
        vb[pr["matches"][:, 0][ref.unpack_bits(reco["good_bits"][mi], n)]] = True
        assert np.array_equal(vb, a["vbTriangulated"])
        par = ref.parallax_deg(reco["n_good"][mi], reco["cos_sel"][mi])
        assert abs(float(par) - float(a["parallax"][mi])) < 1e-3 and par > 1.0


@pytest.mark.parametrize("count", [50, 51, 52])
def test_parallax_index_on_the_header(count):
    c = ref.parallax_case(count)
    reco = ref.host_run(ref.fixture("general"), 1, kind=c["kind"], model=c["model"], subset_bits=ref.pack_bits(c["subset"]))
    mo = c["motion"]
    assert reco["n_good"][mo] == count == int(c["subset"].sum())
    rt = ref.check_rt(reco["R"][mo], reco["t"][mo], ref.m12_of(ref.fixture("general")), c["subset"], 1.0)
    assert rt["n_good"] == count
    k = min(50, count - 1)
    assert k == (49 if count == 50 else 50)
    # the header's selection against the restated cosines: the same rank, a last-place difference at the most
    assert abs(float(reco["cos_sel"][mo]) - float(rt["cos_sel"])) <= 2.0 ** -22


# the tables of csrc/two_view.h: sweeps -> largest gap to A over the admitted hypotheses of these fixtures
SWEEP_FIXTURES = ("general", "planar", "rotation", "n63")
SVD9_TABLE = {5: 4.0, 6: 1.0e-2, 7: 0.0, 9: 0.0}
SVD3_TABLE = {2: (7.4e-2, 0.17), 3: (9.5e-7, 3.6e-7), 4: (0.0, 3.6e-7), 6: (0.0, 3.6e-7)}


def sweep_gaps(macro, k):
    extra = ("-D%s=%d" % (macro, k),)
    g_model = g_pose = 0.0
    for name in SWEEP_FIXTURES:
        pr, a, adm = ref.fixture(name), ref.initialize(name, "A"), ref.admitted(name)
        hyp = ref.host_run(pr, 0, extra=extra)
        g = np.where(np.isfinite(hyp["model"]), rel(hyp["model"], a["models"]), np.inf)
        g_model = max(g_model, g[adm].max())
        kind = a["kind"]                                         # the motions of A's own kept model: the 3 x 3 count alone
        r = ref.host_run(pr, 1, extra=extra, kind=kind, model=a["models"][kind, a["best"][kind]], subset_bits=ref.pack_bits(a["subset"]))
        nm = len(a["n_good"])
        g_pose = max(g_pose, rel(r["R"][:nm].reshape(nm, 3, 3), a["R"]).max(), rel(r["t"][:nm], a["t"]).max())
    return g_model, g_pose


def close(x, want):
    return x == 0 if want == 0 else 0.9 * want <= x <= 1.1 * want


def test_sweep_count_tables_are_reproduced():
    hdr = open(ref.CSRC + "/two_view.h").read()
    assert "#define TV_SVD9_SWEEPS 9" in hdr and "#define TV_SVD3_SWEEPS 6" in hdr
    for k, want in SVD9_TABLE.items():
        g, _ = sweep_gaps("TV_SVD9_SWEEPS", k)
        print("9 columns, %d sweeps: %.3g" % (k, g))
        assert close(g, want), (k, g)
    for k, (wm, wp) in SVD3_TABLE.items():
        gm, gp = sweep_gaps("TV_SVD3_SWEEPS", k)
        print("3 x 3, %d sweeps: models %.3g motions %.3g" % (k, gm, gp))
        assert close(gm, wm) and close(gp, wp), (k, gm, gp)
    # the gap stops falling at 7 and at 4 sweeps; two more ship


def test_header_and_driver_under_address_and_undefined_sanitizers():
    """The header behind its stand-alone driver, every fixture end to end and the three parallax cases."""
    exe = ref.host_exe(("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"))
    for name in ref.NAMES:
        plain = ref.host_initialize(name)
        hyp, pick, reco = ref.host_run(ref.fixture(name), 2, exe=exe)
        assert pick == plain[1] and np.array_equal(hyp["n_inliers"], plain[0]["n_inliers"]) and np.array_equal(reco["status"], plain[2]["status"])
    for count in (50, 51, 52):
        c = ref.parallax_case(count)
        r = ref.host_run(ref.fixture("general"), 1, exe=exe, kind=c["kind"], model=c["model"], subset_bits=ref.pack_bits(c["subset"]))
        assert r["n_good"][c["motion"]] == count
    degenerate = dict(ref.fixture("n63"))                          # every keypoint in one place: NaN models, bounded time, no fault
    degenerate["keys1"] = np.full_like(degenerate["keys1"], 100)
    degenerate["keys2"] = np.full_like(degenerate["keys2"], 100)
    hyp, pick, reco = ref.host_run(degenerate, 2, exe=exe)
    assert pick["motion"] == -1 and not np.isfinite(hyp["score"]).all()


def test_host_scans_through_the_library_equal_the_restatement():
    from weiner_slamit_v2_amd import api

    L = api.lib()
    rs = np.random.RandomState(3)
    for _ in range(300):
        N = int(rs.randint(8, 200))
        for m, pick, lib_pick in ((4, ref.pick_f, L.slamit_init_pick_f), (8, ref.pick_h, L.slamit_init_pick_h)):
            ng = rs.randint(0, N + 1, m).astype(np.int32)
            if rs.rand() < 0.5:
                ng[rs.randint(m)] = N
            par = rs.uniform(0, 3, m).astype(f32)
            assert lib_pick(ng.ctypes.data, par.ctypes.data, N, 1.0, 50) == pick(list(ng), list(par), N)
    sc = np.array([0, -1, 3, 3, np.nan, 5, 5], f32)
    assert L.slamit_init_best_hypothesis(len(sc), sc.ctypes.data) == 5 == ref.best_hypothesis(sc)
    z = np.zeros(4, f32)
    assert L.slamit_init_best_hypothesis(4, z.ctypes.data) == -1
    assert L.slamit_init_choose_h(41.0, 59.0) == 1 and L.slamit_init_choose_h(39.0, 61.0) == 0 and L.slamit_init_choose_h(0.0, 0.0) == 0
    assert L.slamit_init_choose_h(40.0, 60.0) == 1               # the float 0.4f lies above the double literal 0.40, as in the reference
    assert L.slamit_init_parallax_deg(0, 0.5) == 0 and abs(L.slamit_init_parallax_deg(3, 0.5) - 60.0) < 1e-4
