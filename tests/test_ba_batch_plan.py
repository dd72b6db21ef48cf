"""The batch plan of the local BA (BaBatchPlan, csrc/ba_plan.cc) on the CPU: where each window of a batch sits in the slabs and the pinned
block, the maxima the launches are sized by, and the checks that refuse a batch.  Built with g++ beside the drivers of test_ba_plan.py and
test_ba_large_plan.py; every expected value is computed here, in numpy, from the per-window plans those drivers return."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import test_ba_large_plan as large
from tests.test_ba_plan import CSRC, build_plan_lib, limits, pinned_cases
from tests.helpers import ROOT
from weiner_slamit_v2_amd import api, synth

BA_TILE, BA_TL_CHUNK = 64, 128
BAND, BLOCKED, TILED = 0, 1, 2
SIZEOF_BASTATE = 1456          # ba_types.h: 10 int32, 5 doubles, one 64-bit word, then the per-stage statistics and eight stamps
SLAMIT_OK, SLAMIT_ERR_ARG, SLAMIT_ERR_CAPACITY = 0, -1, -3
WIN_BYTES, SLAB = 1 << 24, 1 << 32   # a slab pitch and a (never dereferenced) device address

HEAD = 10    # int64 words in front of the per-window records
PER_WIN = 9

DRIVER = r'''
#include <string.h>
#include <vector>
#include "ba_plan.h"

extern "C" size_t drv_sizeof_state() { return sizeof(BaState); }

// carve_io of P's sizes with a side table of `side_words`: {in_bytes, out_off, bytes}
extern "C" void drv_carve(const slamit_ba_problem* P, size_t side_words, size_t* out) {
    const IoLayout L = carve_io(nullptr, P->n_kf, P->n_pt, P->n_edge, P->edge_ur != nullptr, side_words);
    out[0] = L.in_bytes; out[1] = L.out_off; out[2] = L.bytes;
}

// out: nwin, st_off, pin_need, mk, mp, me, Npad, Npad_ldlt, solvers, tl_grid entries | per window: side_w, in_off, out_off, dio.in_bytes,
// dio.out_off, dio.bytes, and dio.in_pose / out_pose / side as offsets from `slab` (-1: null) | tl_grid.  Returns the words written, 0 when a
// window's plan fails, -need when `cap` is too small.
extern "C" long drv_batch_plan(const slamit_ba_problem* probs, int nwin, const int32_t* lim, size_t win_bytes, uint8_t* slab, int64_t* out, long cap) {
    BaBatchPlan B;
    ba_batch_layout(probs, nwin, win_bytes, slab, B);
    std::vector<BaWin> wins(nwin);
    std::vector<BaWindowPlan> plans(nwin);
    const BaPlanLimits L{lim[0], lim[1], lim[2] != 0, lim[3] != 0, lim[4] != 0, lim[5]};
    for (int b = 0; b < nwin; ++b) {
        memset(&wins[b], 0, sizeof(BaWin));
        if (!ba_plan_window(probs[b], L, wins[b], plans[b])) return 0;
        wins[b].side = B.dio[b].side;   // as the solve leaves it: a device address, which the batch plan must not read through
    }
    ba_batch_launches(wins.data(), plans.data(), B);
    const long need = 10 + 9 * (long)nwin + (long)B.tl_grid.size();
    if (need > cap) return -need;
    int64_t* o = out;
    *o++ = B.nwin; *o++ = (int64_t)B.st_off; *o++ = (int64_t)B.pin_need; *o++ = B.mk; *o++ = B.mp; *o++ = B.me;
    *o++ = B.Npad; *o++ = B.Npad_ldlt; *o++ = B.solvers; *o++ = (int64_t)B.tl_grid.size();
    auto rel = [&](const void* p) { return p ? (int64_t)((const uint8_t*)p - slab) : (int64_t)-1; };
    for (int b = 0; b < nwin; ++b) {
        const IoLayout& D = B.dio[b];
        *o++ = (int64_t)B.side_w[b]; *o++ = (int64_t)B.in_off[b]; *o++ = (int64_t)B.out_off[b];
        *o++ = (int64_t)D.in_bytes; *o++ = (int64_t)D.out_off; *o++ = (int64_t)D.bytes;
        *o++ = rel(D.in_pose); *o++ = rel(D.out_pose); *o++ = rel(D.side);
    }
    for (int v : B.tl_grid) *o++ = v;
    return need;
}

// caps: max_kf, max_free_kf, max_pt, max_edge, max_batch.  Returns the code; the text (empty: accepted) in msg
extern "C" int drv_batch_check(const slamit_ba_problem* probs, const slamit_ba_result* results, int nwin, const int32_t* caps, char* msg, int cap) {
    const BaRefusal r = ba_batch_check(probs, results, nwin, BaCaps{caps[0], caps[1], caps[2], caps[3], caps[4]});
    msg[0] = 0;
    if (r.msg) { strncpy(msg, r.msg, cap - 1); msg[cap - 1] = 0; }
    return r.code;
}
'''

# The sanitizer build: the same batches and refusals, from a file the test writes (per window: n_kf, n_pt, n_edge, stereo, then the arrays)
MAIN = r'''
#include <stdio.h>
#include <stdlib.h>

struct Loaded {
    std::vector<std::vector<uint8_t>> blobs;
    slamit_ba_problem P;
};

static void* blob(FILE* f, Loaded& w, size_t bytes) {
    w.blobs.emplace_back(bytes ? bytes : 1);
    if (bytes && fread(w.blobs.back().data(), 1, bytes, f) != bytes) { printf("short file\n"); exit(2); }
    return w.blobs.back().data();
}

int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t nwin = 0;
    if (fread(&nwin, 4, 1, f) != 1) return 2;
    std::vector<Loaded> W(nwin);
    for (Loaded& w : W) {
        int32_t h[4];
        if (fread(h, 4, 4, f) != 4) return 2;
        slamit_ba_problem& P = w.P;
        memset(&P, 0, sizeof(P));
        P.n_kf = h[0]; P.n_pt = h[1]; P.n_edge = h[2];
        P.kf_pose = (const double*)blob(f, w, 96 * (size_t)h[0]); P.kf_fixed = (const uint8_t*)blob(f, w, h[0]);
        P.kf_intr = (const double*)blob(f, w, 32 * (size_t)h[0]); P.pt_xyz = (const double*)blob(f, w, 24 * (size_t)h[1]);
        P.edge_kf = (const int32_t*)blob(f, w, 4 * (size_t)h[2]); P.edge_pt = (const int32_t*)blob(f, w, 4 * (size_t)h[2]);
        P.edge_uv = (const double*)blob(f, w, 16 * (size_t)h[2]); P.edge_inv_sigma2 = (const double*)blob(f, w, 8 * (size_t)h[2]);
        if (h[3]) { P.edge_ur = (const double*)blob(f, w, 8 * (size_t)h[2]); P.kf_bf = (const double*)blob(f, w, 8 * (size_t)h[0]); }
    }
    fclose(f);
    std::vector<slamit_ba_problem> probs;
    for (Loaded& w : W) probs.push_back(w.P);
    std::vector<int64_t> out(1 << 16);
    const int32_t lim[6] = {2048, nwin, 0, 0, 0, 0}, lim1[6] = {2048, 1, 0, 0, 0, 0};
    uint8_t* slab = (uint8_t*)(uintptr_t)(1ull << 32);
    long words = drv_batch_plan(probs.data(), nwin, lim, 1u << 24, slab, out.data(), (long)out.size());
    if (words <= 0) { printf("batch plan failed %ld\n", words); return 1; }
    for (int b = 0; b < nwin; ++b) {
        const long w1 = drv_batch_plan(&probs[b], 1, lim1, 1u << 24, slab, out.data(), (long)out.size());
        if (w1 <= 0) { printf("single plan failed %ld\n", w1); return 1; }
        words += w1;
    }
    // the refusals: every window against capacities one short of it, and a null array in each place
    std::vector<double> sink(1);
    std::vector<slamit_ba_result> res(nwin);
    for (slamit_ba_result& r : res) { memset(&r, 0, sizeof(r)); r.kf_pose = sink.data(); r.pt_xyz = sink.data(); }
    char msg[256];
    int codes = 0;
    for (int b = 0; b < nwin; ++b) {
        const slamit_ba_problem& P = probs[b];
        const int32_t caps[][5] = {{P.n_kf, P.n_kf, P.n_pt, P.n_edge, 1}, {P.n_kf - 1, P.n_kf, P.n_pt, P.n_edge, 1}, {P.n_kf, 0, P.n_pt, P.n_edge, 1},
                                   {P.n_kf, P.n_kf, P.n_pt - 1, P.n_edge, 1}, {P.n_kf, P.n_kf, P.n_pt, P.n_edge - 1, 1}, {P.n_kf, P.n_kf, P.n_pt, P.n_edge, 0}};
        for (const auto& c : caps) codes += drv_batch_check(&P, &res[b], 1, c, msg, sizeof(msg)) != 0;
        slamit_ba_problem Q = P;
        Q.kf_pose = nullptr;
        codes += drv_batch_check(&Q, &res[b], 1, caps[0], msg, sizeof(msg)) != 0;
        Q = P; Q.edge_ur = sink.data(); Q.kf_bf = nullptr;
        codes += drv_batch_check(&Q, &res[b], 1, caps[0], msg, sizeof(msg)) != 0;
    }
    codes += drv_batch_check(nullptr, res.data(), nwin, lim, msg, sizeof(msg)) != 0;
    printf("words %ld refusals %d\n", words, codes);
    return 0;
}
'''


def _large_plan(L, prob):
    return large.plan(L, prob)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("ba_batch_plan"))
    extra = []
    for name, text in (("batch_driver.cc", DRIVER), ("large_driver.cc", large.DRIVER)):
        extra.append(os.path.join(tmp, name))
        with open(extra[-1], "w") as f:
            f.write(text)
    L = build_plan_lib(tmp, [os.path.join(CSRC, "ba_plan.cc")] + extra)
    L.drv_sizeof_state.restype = C.c_size_t
    L.drv_batch_plan.restype = C.c_long
    L.drv_batch_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_long]
    L.drv_carve.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.drv_batch_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    return L


@pytest.fixture(scope="module")
def windows():
    """One window per solver kind, and a second tiled one whose structure travels in the side table."""
    cases = pinned_cases()
    return {"band": cases["ba_stereo_window8"][0], "blocked": cases["synth_50_2000_dense"][0],
            "tiled": synth.synth_map(**large.WINDOWS["free90"]), "tiled_side": synth.synth_map(**large.WINDOWS["global150"])}


def _problems(probs):
    P = (api.BaProblem * len(probs))()
    keeps = []
    for i, prob in enumerate(probs):
        P[i], keep = api._ba_problem(prob)
        keeps.append(keep)
    return P, keeps


def batch_plan(L, probs):
    P, keeps = _problems(probs)
    out = np.zeros(1 << 14, np.int64)
    n = L.drv_batch_plan(P, len(probs), limits(max_kf=341, nwin=len(probs)).ctypes.data, WIN_BYTES, SLAB, out.ctypes.data, len(out))
    assert n > 0
    nwin, tl_n = int(out[0]), int(out[9])
    assert n == HEAD + PER_WIN * nwin + tl_n
    B = dict(zip(("nwin", "st_off", "pin_need", "mk", "mp", "me", "Npad", "Npad_ldlt", "solvers"), (int(v) for v in out[:9])))
    rec = out[HEAD:HEAD + PER_WIN * nwin].reshape(nwin, PER_WIN)
    for i, k in enumerate(("side_w", "in_off", "out_off", "in_bytes", "dio_out_off", "bytes", "in_pose", "out_pose", "side")):
        B[k] = rec[:, i].tolist()
    B["tl_grid"] = out[HEAD + PER_WIN * nwin:n].tolist()
    return B


def ldlt_tiled_ntiles(below):
    """k_ldlt_tiled_update's workgroups: the lower 64 x 64 tiles (rt, ct), ct <= min(rt, CT - 1), of `below` rows and the right-hand side's."""
    RT, CT = -(-(below + 1) // BA_TILE), -(-below // BA_TILE)
    return sum(min(rt + 1, CT) for rt in range(RT))


def panel_steps(o):
    """Per panel step of a tiled window: rows below the panel that its columns reach (the plan's row envelope)."""
    n = o["nS"]
    return [max(int(o["panel_hi"][i]) + 1 - min(32 * i + 32, n), 0) for i in range(-(-n // 32))]


def expected(L, probs):
    plans = [_large_plan(L, p) for p in probs]
    E = {"nwin": len(probs)}
    E["mk"] = max([1] + [len(p["kf_fixed"]) for p in probs])
    E["mp"] = max([1] + [len(p["pt_xyz"]) for p in probs])
    E["me"] = max([1] + [len(p["edge_kf"]) for p in probs])
    E["Npad"] = max([BA_TILE] + [o["Npad"] for o in plans])
    E["Npad_ldlt"] = max([BA_TILE] + [o["Npad"] for o in plans if o["solver"] != TILED])
    E["solvers"] = int(np.bitwise_or.reduce([1 << o["solver"] for o in plans]))
    grid = []
    for o in plans:
        if o["solver"] != TILED:
            continue
        below = panel_steps(o)
        grid += [0] * (2 * len(below) - len(grid))
        for i, r in enumerate(below):
            grid[2 * i] = max(grid[2 * i], -(-(r + 1) // BA_TL_CHUNK))
            grid[2 * i + 1] = max(grid[2 * i + 1], ldlt_tiled_ntiles(r))
    E["tl_grid"] = grid
    # the offsets: running sums of the windows' carve_io sections
    P, keeps = _problems(probs)
    carve = np.zeros((len(probs), 3), np.uint64)
    E["side_w"] = [4 * o["T"] + 2 * o["P"] if o["needed"] else 0 for o in plans]
    for b in range(len(probs)):
        L.drv_carve(C.byref(P[b]), E["side_w"][b], carve[b].ctypes.data)
    carve = carve.astype(np.int64)
    in_bytes, out_bytes = carve[:, 0], carve[:, 2] - carve[:, 1]
    E["in_bytes"], E["dio_out_off"], E["bytes"] = carve[:, 0].tolist(), carve[:, 1].tolist(), carve[:, 2].tolist()
    E["in_off"] = (np.cumsum(in_bytes) - in_bytes).tolist()
    E["out_off"] = (in_bytes.sum() + np.cumsum(out_bytes) - out_bytes).tolist()
    total = int(in_bytes.sum() + out_bytes.sum())
    E["st_off"] = -(-total // 256) * 256
    E["pin_need"] = E["st_off"] + 2 * SIZEOF_BASTATE * len(probs)
    # the device layout: window b's io section starts its slab
    E["in_pose"] = [b * WIN_BYTES for b in range(len(probs))]
    E["out_pose"] = [b * WIN_BYTES + int(carve[b, 1]) for b in range(len(probs))]
    return E, plans


BATCHES = (("band", "blocked", "tiled"), ("band",), ("blocked",), ("tiled",), ("tiled_side",), ("tiled", "tiled_side"), ("tiled_side", "band"))


def test_batch_plan_fields(lib, windows):
    assert lib.drv_sizeof_state() == SIZEOF_BASTATE
    kinds = {}
    for names in BATCHES:
        probs = [windows[n] for n in names]
        got = batch_plan(lib, probs)
        want, plans = expected(lib, probs)
        for n, o in zip(names, plans):
            kinds[n] = (o["solver"], o["needed"])
        side = got.pop("side")
        for k in want:
            assert got[k] == want[k], (names, k)
        assert sorted(got) == sorted(want), names
        assert got["st_off"] % 256 == 0 and all(v % 256 == 0 for v in got["in_off"] + got["out_off"]), names
        for b, o in enumerate(plans):   # the side table is the last of the inputs, there only when the window needs one
            assert (side[b] >= 0) == o["needed"], (names, b)
            if o["needed"]:
                assert b * WIN_BYTES < side[b] and side[b] + 4 * want["side_w"][b] <= b * WIN_BYTES + want["in_bytes"][b], (names, b)
    assert kinds == {"band": (BAND, False), "blocked": (BLOCKED, False), "tiled": (TILED, False), "tiled_side": (TILED, True)}


def test_tiled_grid_covers_every_panel_step(lib, windows):
    for names in (("tiled",), ("tiled_side",), ("band", "blocked", "tiled"), ("tiled", "tiled_side")):
        probs = [windows[n] for n in names]
        grid = batch_plan(lib, probs)["tl_grid"]
        for n in names:
            o = _large_plan(lib, windows[n])
            if o["solver"] != TILED:
                continue
            below = panel_steps(o)
            assert len(grid) >= 2 * len(below), (names, n)
            for i, r in enumerate(below):
                assert grid[2 * i] * BA_TL_CHUNK >= r + 1, (names, n, i)         # k_ldlt_tiled_panel: every row below, and the right-hand side's
                assert grid[2 * i + 1] >= ldlt_tiled_ntiles(r), (names, n, i)   # k_ldlt_tiled_update: every lower tile
            assert below[-1] == 0 and max(below) > 0, (names, n)
    assert batch_plan(lib, [windows["band"], windows["blocked"]])["tl_grid"] == []


def _check(L, P, R, nwin, caps):
    msg = C.create_string_buffer(256)
    code = L.drv_batch_check(P, R, nwin, np.array(caps, np.int32).ctypes.data, msg, 256)
    return code, msg.value.decode()


def test_refused_batches(lib, windows):
    """The codes and texts slamit_ba_solve_batch has always answered with, in the order it checks."""
    probs = [windows["band"], windows["tiled"]]   # 50 keyframes (stereo); 150 keyframes, 90 of them free
    P, keeps = _problems(probs)
    R = (api.BaResult * 2)()
    outs = []
    for b in range(2):
        R[b], out, st = api.Optimizer._result(P[b].n_kf, P[b].n_pt, P[b].n_edge)
        outs.append((out, st))
    nfree = int((probs[1]["kf_fixed"] == 0).sum())
    assert (P[0].n_kf, P[1].n_kf, nfree) == (50, 150, 90)
    mp, me = max(P[0].n_pt, P[1].n_pt), max(P[0].n_edge, P[1].n_edge)
    caps = [150, 90, mp, me, 2]   # max_kf, max_free_kf, max_pt, max_edge, max_batch: the batch fits exactly
    pre = "slamit_ba_solve_batch: "
    assert _check(lib, P, R, 2, caps) == (SLAMIT_OK, "")
    assert _check(lib, P, R, 0, caps) == (SLAMIT_OK, "")
    for args in ((None, R, 2), (P, None, 2), (P, R, -1)):
        assert _check(lib, *args, caps) == (SLAMIT_ERR_ARG, pre + "bad argument")
    assert _check(lib, P, R, 2, caps[:4] + [1]) == (SLAMIT_ERR_CAPACITY, pre + "nwin > max_batch")
    over = (SLAMIT_ERR_CAPACITY, pre + "window exceeds the handle's capacity")
    assert _check(lib, P, R, 2, [149] + caps[1:]) == over
    assert _check(lib, P, R, 2, caps[:2] + [mp - 1] + caps[3:]) == over
    assert _check(lib, P, R, 2, caps[:3] + [me - 1] + caps[4:]) == over
    assert _check(lib, P, R, 2, [150, 89] + caps[2:]) == (
        SLAMIT_ERR_CAPACITY, pre + "window has more free keyframes than the handle's max_free_kf")

    def with_field(obj, b, field, value):
        keep = getattr(obj[b], field)
        setattr(obj[b], field, value)
        return keep

    for b, field in ((0, "kf_pose"), (0, "kf_fixed"), (1, "kf_intr"), (1, "pt_xyz"), (0, "edge_kf"), (1, "edge_pt"), (0, "edge_uv"), (1, "edge_inv_sigma2")):
        keep = with_field(P, b, field, None)
        assert _check(lib, P, R, 2, caps) == (SLAMIT_ERR_ARG, pre + "null input array"), field
        setattr(P[b], field, keep)
    keep = with_field(P, 0, "kf_bf", None)
    assert _check(lib, P, R, 2, caps) == (SLAMIT_ERR_ARG, pre + "stereo observations (edge_ur) without the keyframes' bf (kf_bf)")
    setattr(P[0], "kf_bf", keep)
    for b, field in ((0, "kf_pose"), (1, "pt_xyz")):
        keep = with_field(R, b, field, None)
        assert _check(lib, P, R, 2, caps) == (SLAMIT_ERR_ARG, pre + "null output array"), field
        # the order: a window is checked whole before the next one, capacity before its arrays
        assert _check(lib, P, R, 2, [149] + caps[1:]) == ((SLAMIT_ERR_ARG, pre + "null output array") if b == 0 else over), field
        setattr(R[b], field, keep)
    keep = with_field(P, 1, "kf_pose", None)
    assert _check(lib, P, R, 2, [149] + caps[1:]) == over                       # (capacity in front of the arrays)
    assert _check(lib, P, R, 2, [150, 89] + caps[2:]) == (SLAMIT_ERR_ARG, pre + "null input array")   # (the arrays in front of the free count)
    setattr(P[1], "kf_pose", keep)
    assert _check(lib, P, R, 2, caps) == (SLAMIT_OK, "")


def test_sanitized_driver_runs_clean(tmp_path, windows):
    names = BATCHES[0]
    path = os.path.join(str(tmp_path), "windows.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(names)).tobytes())
        for n in names:
            p, keep = api._ba_problem(windows[n])
            f.write(np.array([p.n_kf, p.n_pt, p.n_edge, "edge_ur" in keep], np.int32).tobytes())
            for k in ("kf_pose", "kf_fixed", "kf_intr", "pt_xyz", "edge_kf", "edge_pt", "edge_uv", "edge_inv_sigma2", "edge_ur", "kf_bf"):
                if k in keep:
                    f.write(keep[k].tobytes())
    src = os.path.join(str(tmp_path), "batch_asan.cc")
    with open(src, "w") as f:
        f.write(DRIVER + MAIN)
    exe = os.path.join(str(tmp_path), "batch_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           "-I", os.path.join(ROOT, "include"), src, os.path.join(CSRC, "ba_plan.cc"), "-o", exe])
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and r.stdout.decode().startswith("words "), r.stdout.decode()
