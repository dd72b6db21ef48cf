"""The checker of the device projections on the CPU (tests/project_ref.py): the committed fixtures are admissible by the restatement
alone, and the text the kernel compiles (csrc/project.h), built with g++ for the host, equals variant "32" bit for bit.

Measured on the committed fixtures: 0 undecided points of 9,255 in 13 fixtures; the two variants agree on every
status; every code a form can produce occurs at least 9 times in each of its fixtures, and among the first 65 points of its first."""
import subprocess

import numpy as np
import pytest

from tests import project_ref as ref


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fixtures_are_admissible():
    """What keeps the GPU test honest, by the restatement alone: no undecided point, the variants agree on every status, every code a
    form can produce occurs at least 3 times in every fixture of that form (and no other code does), every form has a fixture of 300
    to 2000 points, LAST_FRAME has all three directions and octaves of -1 and n_levels."""
    total, directions = 0, set()
    assert set(f[0] for f in ref.FIXTURES) == set(range(6))
    for k, (form, seed, n, th, direction) in enumerate(ref.FIXTURES):
        a, pr = ref.admissibility(k), ref.fixture(k)
        r32, r64 = a["r32"], a["r64"]
        counts = np.bincount(r32["status"], minlength=8)
        print("fixture %d: %s n %d, th %g, undecided %d, codes %s" % (k, ref.FORMS[form], n, th, a["undecided"], counts.tolist()))
        assert 300 <= n <= 2000 and len(r32["status"]) == n
        assert a["undecided"] == 0, k
        assert np.array_equal(r32["status"], r64["status"]), k
        for code in range(8):
            assert (counts[code] >= 3) if code in ref.POSSIBLE[form] else (counts[code] == 0), (k, code, counts.tolist())
        if form == ref.LAST_FRAME:
            directions.add(direction)
            assert (pr["octave"] == -1).sum() >= 3 and (pr["octave"] == pr["n_levels"]).sum() >= 3
            assert pr["normal"] is None and pr["max_dist"] is None
        total += n
    print("points: %d" % total)
    assert directions == {0, 1, 2}
    for form in range(6):                                           # the GPU test's wavefront-edge heads see every code from n = 65 on
        k = ref.first_fixture(form)
        assert ref.FIXTURES[k][2] == 300
        assert set(int(s) for s in ref.evaluate(ref.head(ref.fixture(k), 65), "32")["status"]) == ref.POSSIBLE[form]


def test_the_sim3_fixtures_carry_a_scale():
    for k, f in enumerate(ref.FIXTURES):
        if f[0] in (ref.SIM3_PROJ, ref.SIM3_FUSE):
            Scw = ref.fixture(k)["true"]["Scw"]
            assert abs(np.linalg.norm(Scw[0, :3].astype(np.float64)) - 1.3) < 1e-5
        if f[0] == ref.SIM3_PAIR:
            assert abs(np.linalg.norm(np.asarray(ref.fixture(k)["R2"], np.float64)[:3]) - 1 / 1.3) < 1e-5


@pytest.mark.parametrize("k", range(len(ref.FIXTURES)))
def test_the_header_on_the_host_equals_ref32(k):
    """The text the kernel compiles, run on the CPU: statuses and levels equal, u, v, r bit-equal to variant "32" on every point, and
    the query rows are the ones the drivers' loops build."""
    a, h, pr = ref.admissibility(k), ref.host_fixture(k), ref.fixture(k)
    r32 = a["r32"]
    assert a["decided"].all()
    assert np.array_equal(h["status"], r32["status"]), np.flatnonzero(h["status"] != r32["status"])[:5]
    assert np.array_equal(h["level"], r32["level"])
    for f in ref.FLOATS:
        assert np.array_equal(bits(h[f]), bits(r32[f])), (k, f, np.flatnonzero(bits(h[f]) != bits(r32[f]))[:5])
    uvr, l0, l1, valid = ref.queries_of(pr, r32)
    assert np.array_equal(bits(h["uvr"]), bits(uvr)) and np.array_equal(h["level_min"], l0) and np.array_equal(h["level_max"], l1)
    assert np.array_equal(h["valid"], valid)
    s7, s0 = h["status"] == 7, h["status"] == 0
    assert np.all(h["level"][s7] == ref.LEVEL_NONE) and not h["valid"][s7].any() and np.all(h["r"][s7] == 0)
    assert np.all((h["level"][s0] >= 0) & (h["level"][s0] < 8)) and np.all(h["r"][s0] > 0)
    assert np.all(h["u"][(h["status"] == 1) | (h["status"] == 2)] == 0) and np.all(h["level"][(h["status"] > 0) & (h["status"] < 7)] == 0)
    th = np.float32(ref.FIXTURES[k][3])
    assert np.array_equal(bits(h["r"][s0]), bits(th * pr["scale_factors"][h["level"][s0]]))


def test_the_level_windows_of_the_forms():
    want = {0: (-1, 1), 3: (-1, 1), 5: (-1, 0), 7: (-1, 0), 9: (-1, 0), 11: (-1, 0)}
    for k, (lo, hi) in want.items():
        h = ref.host_fixture(k)
        s0 = h["status"] == 0
        assert np.array_equal(h["level_min"][s0], h["level"][s0] + lo) and np.array_equal(h["level_max"][s0], h["level"][s0] + hi), k
    fwd, back = ref.host_fixture(1), ref.host_fixture(2)
    assert ref.FIXTURES[1][4] == 1 and ref.FIXTURES[2][4] == 2
    s0 = fwd["status"] == 0
    assert np.array_equal(fwd["level_min"][s0], fwd["level"][s0]) and np.all(fwd["level_max"][s0] == -1)
    s0 = back["status"] == 0
    assert np.all(back["level_min"][s0] == 0) and np.array_equal(back["level_max"][s0], back["level"][s0])


@pytest.mark.parametrize("form", range(6))
def test_the_boundary_fixture(form):
    """+-0 depth, u and v exactly on the bounds (the closed frame bounds and the half-open IsInImage differ on the upper one), a NaN
    projection (passes the frame bounds, fails IsInImage) and dist == 0: the header and both variants give the statuses worked out by
    hand in project_ref.boundary_fixture."""
    pr, want = ref.boundary_fixture(form)
    a, h = ref.analyse(pr), ref.host_points(pr)
    assert h["status"].tolist() == want == a["r32"]["status"].tolist() == a["r64"]["status"].tolist()
    for f in ref.FLOATS:
        assert np.array_equal(bits(h[f]), bits(a["r32"][f])), f
    assert np.array_equal(h["level"], a["r32"]["level"])
    assert np.isposinf(h["u"][0])
    if form == ref.LAST_FRAME:
        assert h["u"][1] == 0 and np.isnan(h["u"][2]) and h["valid"][2] == 1      # the reference searches around a NaN centre too
    else:
        assert np.isnan(h["u"][1]) and np.isnan(h["u"][2])
    if form == ref.RELOC:
        assert h["level"][1] == ref.LEVEL_NONE                                    # dist == 0: the ratio is +inf
    assert h["u"][3] == 0.0 and h["u"][4] == 640.0 and h["v"][5] == 480.0
    on_max = [int(h["status"][4]), int(h["status"][5])]
    assert on_max == ([0, 0] if form <= ref.RELOC else [3, 4])


def test_the_header_runs_clean_under_the_sanitizers():
    """The same main, built with -fsanitize=address,undefined as a stand-alone host program, on one fixture per form and on the boundary
    fixtures: it exits 0 (either sanitizer aborts otherwise) and gives the same bytes."""
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")
    try:
        ref.host_exe(flags)
    except subprocess.CalledProcessError:
        pytest.fail("g++ could not build the host driver with the sanitizers")
    for form in range(6):
        for pr, plain in ((ref.fixture(ref.first_fixture(form)), ref.host_fixture(ref.first_fixture(form))), (ref.boundary_fixture(form)[0], None)):
            san = ref.host_points(pr, flags)
            plain = plain if plain is not None else ref.host_points(pr)
            assert np.array_equal(san["status"], plain["status"]) and np.array_equal(san["level"], plain["level"])
            assert np.array_equal(bits(san["uvr"]), bits(plain["uvr"])) and np.array_equal(bits(san["proj"]), bits(plain["proj"]))
