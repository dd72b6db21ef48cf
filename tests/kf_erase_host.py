"""What the SetBadFlag tests share: the arrays a call must leave, laid out from the restatement's result (tests/kf_erase_ref.py) over the
caller's arrays and prefilled outputs; csrc/kf_erase.h built with g++ behind a small main that takes any number of jobs; the
comparison, exact."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests.helpers import ROOT
from tests.kf_erase_ref import CHILD_OVERFLOW, EDIT_OVERFLOW, SET_BAD

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
BEST = 10
KF_OP_DTYPE = np.dtype([("kind", "<i4"), ("kf", "<i4"), ("parent", "<i4"), ("reserved", "<i4")])
EDIT_DTYPE = np.dtype([("kind", "<i4"), ("flags", "<i4"), ("mp", "<i4"), ("kf", "<i4"), ("idx", "<i4"), ("octave", "u1"), ("weight", "u1"), ("pad", "u1", 2)])
ERASE_OBS = 2
# what the caller leaves in the outputs before the call
FILL = {"child_ptr_out": -5, "child_out": -6, "op_status": -9, "edits": 0xee}
INPLACE = (("kf_bad", np.uint8), ("kf_parent", np.int32), ("kf_to_be_erased", np.uint8), ("cw_kf", np.int32), ("cw_w", np.int32), ("cw_n", np.int32),
           ("ord_kf", np.int32), ("ord_w", np.int32), ("ord_n", np.int32), ("kf_best", np.int32))
OUT_TYPES = (("child_ptr_out", np.int32), ("child_out", np.int32)) + INPLACE + (("op_status", np.int32), ("edits", np.uint8))
OUT_KEYS = tuple(k for k, _ in OUT_TYPES) + ("n_edits_out", "n_child_out", "status")


def records(ops):
    out = np.zeros(len(ops), KF_OP_DTYPE)
    for i, e in enumerate(ops):
        out[i] = tuple(int(v) for v in e) + (0,)
    return out


def source(fx, key):
    return fx["t"][key] if key in ("kf_bad", "kf_parent") else fx["x"][key]


def default_caps(fx):
    """(child_cap_out, edit_cap) that always suffice: the old table plus one entry per op and per child of a SET_BAD keyframe; the
    keypoints of the SET_BAD keyframes."""
    t = fx["t"]
    ks = [op[1] for op in fx["ops"] if op[0] == SET_BAD]
    return (int(t["kf_child_ptr"][-1]) + len(fx["ops"]) + sum(int(t["kf_child_ptr"][k + 1] - t["kf_child_ptr"][k]) for k in ks),
            sum(int(t["kf_mp_ptr"][k + 1] - t["kf_mp_ptr"][k]) for k in ks))


def fills(fx, child_cap, edit_cap):
    return {"child_ptr_out": np.full(fx["t"]["n_kf"] + 1, FILL["child_ptr_out"], np.int32), "child_out": np.full(child_cap, FILL["child_out"], np.int32),
            "op_status": np.full(len(fx["ops"]), FILL["op_status"], np.int32), "edits": np.full(edit_cap * EDIT_DTYPE.itemsize, FILL["edits"], np.uint8)}


def laid_out(fx, want, child_cap, edit_cap):
    """Every array of OUT_KEYS as the call must leave it over outputs prefilled with FILL: a rewritten graph row holds its new entries up
    to its new count and the caller's bytes past it, every other row its own; past the counts the fill stays; with a gate's bit
    everything but the two needs and the status keeps its bytes."""
    e = fills(fx, child_cap, edit_cap)
    for key, dt in INPLACE:
        e[key] = np.array(source(fx, key), dt).reshape(-1)
    need, n_edits = sum(len(r) for r in want["children"]), len(want["edits"])
    e["n_child_out"], e["n_edits_out"] = need, n_edits
    e["status"] = (CHILD_OVERFLOW if need > child_cap else 0) | (EDIT_OVERFLOW if n_edits > edit_cap else 0)
    if e["status"]:
        return e
    e["child_ptr_out"][:] = np.cumsum([0] + [len(r) for r in want["children"]])
    e["child_out"][:need] = [c for r in want["children"] for c in r]
    e["op_status"][:] = want["op_status"]
    ed = np.zeros(n_edits, EDIT_DTYPE)
    for i, (p, k) in enumerate(want["edits"]):
        ed[i] = (ERASE_OBS, 0, p, k, 0, 0, 0, (0, 0))
    e["edits"][:n_edits * EDIT_DTYPE.itemsize] = ed.view(np.uint8)
    for key in ("kf_bad", "kf_parent", "kf_to_be_erased"):
        e[key][:] = want[key]
    rc = fx["x"]["row_cap"]
    for k, (cw, order) in want["rows"].items():
        e["cw_n"][k], e["ord_n"][k] = len(cw), len(order)
        for i, (j, w) in enumerate(cw):
            e["cw_kf"][k * rc + i], e["cw_w"][k * rc + i] = j, w
        for i, (j, w) in enumerate(order):
            e["ord_kf"][k * rc + i], e["ord_w"][k * rc + i] = j, w
        e["kf_best"][k * BEST:(k + 1) * BEST] = ([j for j, _ in order] + [-1] * BEST)[:BEST]
    return e


def assert_same(got, want, what=""):
    for k in OUT_KEYS:
        a, b = np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1)
        assert a.shape == b.shape and np.array_equal(a, b), "%s %s: %s" % (what, k, (np.flatnonzero(a != b)[:8], a[:12], b[:12]) if a.shape == b.shape else (a.shape, b.shape))


def of_api(out):
    """api.kf_erase's result under the names of OUT_KEYS, the arrays in full."""
    got = {k: out["raw"][k] for k, _ in OUT_TYPES if k != "edits"}
    got["edits"] = out["raw"]["edits"].view(np.uint8)
    got.update(n_edits_out=out["n_edits_out"], n_child_out=out["n_child_out"], status=out["status"])
    return got


HOST_DRIVER = r"""
// csrc/kf_erase.h's sequential statement over any number of jobs: per job a header, the tables and the list in, every output out.
// The refusals of slamit_kf_erase_apply are restated by the caller: a job that reaches this program is valid.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "kf_erase.h"

template <typename T> static std::vector<T> rd(FILE* f) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) exit(2);
    std::vector<T> v((size_t)n + 1);   // never empty: data() is an address
    if (n && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) exit(2);
    v.resize((size_t)n);               // a sanitizer sees the true end; the storage stays
    return v;
}
template <typename T> static void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }   // a copy of an empty vector has no address

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) return 1;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 1;
    const int reps = argc == 4 ? atoi(argv[3]) : 1;   // the bench runs a job over fresh copies many times
    int32_t h[8];   // n_kf n_mp row_cap origin_kf n_ops child_cap_out edit_cap 0
    while (fread(h, 4, 8, f) == 8) {
        LmMap M = LmMap();
        KeIndex X = KeIndex();
        M.n_kf = h[0]; M.n_mp = h[1]; X.row_cap = h[2]; X.origin_kf = h[3]; X.child_cap_out = h[5];
        const std::vector<int32_t> kf_mp_ptr = rd<int32_t>(f), kf_mp = rd<int32_t>(f), kf_child_ptr = rd<int32_t>(f), kf_child = rd<int32_t>(f);
        const std::vector<uint8_t> not_erase = rd<uint8_t>(f);
        const std::vector<uint8_t> bad0 = rd<uint8_t>(f);
        const std::vector<int32_t> parent0 = rd<int32_t>(f);
        const std::vector<uint8_t> tbe0 = rd<uint8_t>(f);
        const std::vector<int32_t> cw_kf0 = rd<int32_t>(f), cw_w0 = rd<int32_t>(f), cw_n0 = rd<int32_t>(f), ord_kf0 = rd<int32_t>(f), ord_w0 = rd<int32_t>(f),
                                   ord_n0 = rd<int32_t>(f), best0 = rd<int32_t>(f);
        const std::vector<KeOp> ops = rd<KeOp>(f);
        const std::vector<int32_t> child_ptr0 = rd<int32_t>(f), child0 = rd<int32_t>(f), ost0 = rd<int32_t>(f);
        const std::vector<MeEdit> edits0 = rd<MeEdit>(f);
        if ((int)ops.size() != h[4] || (int)child0.size() != h[5] || (int)edits0.size() != h[6]) return 3;
        M.kf_mp_ptr = kf_mp_ptr.data(); M.kf_mp = kf_mp.data(); M.kf_child_ptr = kf_child_ptr.data(); M.kf_child = kf_child.data();
        X.kf_not_erase = not_erase.data();
        std::vector<double> ms;
        for (int r = 0; r < reps; ++r) {
            std::vector<uint8_t> bad = bad0, tbe = tbe0;
            std::vector<int32_t> parent = parent0, cw_kf = cw_kf0, cw_w = cw_w0, cw_n = cw_n0, ord_kf = ord_kf0, ord_w = ord_w0, ord_n = ord_n0, best = best0;
            std::vector<int32_t> child_ptr = child_ptr0, child = child0, ost = ost0, tail(3, -1);   // tail: n_edits_out n_child_out status
            std::vector<MeEdit> edits = edits0;
            X.kf_bad = bad.data(); X.kf_parent = parent.data(); X.kf_to_be_erased = tbe.data();
            X.cw_kf = cw_kf.data(); X.cw_w = cw_w.data(); X.cw_n = cw_n.data(); X.ord_kf = ord_kf.data(); X.ord_w = ord_w.data(); X.ord_n = ord_n.data();
            X.kf_best = best.data(); X.child_ptr_out = child_ptr.data(); X.child_out = child.data();
            const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            ke_apply_seq(M, X, h[4], ops.data(), ost.data(), h[6], edits.data(), &tail[0], &tail[1], &tail[2]);
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            if (r + 1 < reps) continue;
            std::sort(ms.begin(), ms.end());
            if (argc == 4) printf("%f %f\n", ms[ms.size() / 2], ms[0]);   // the job's median and fastest walk
            wr(o, child_ptr); wr(o, child); wr(o, bad); wr(o, parent); wr(o, tbe); wr(o, cw_kf); wr(o, cw_w); wr(o, cw_n); wr(o, ord_kf); wr(o, ord_w); wr(o, ord_n);
            wr(o, best); wr(o, ost); wr(o, edits); wr(o, tail);
        }
    }
    fclose(f);
    fclose(o);
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def host_exe(sanitize=False, opt="-O2"):
    d = tempfile.mkdtemp(prefix="kf_erase_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "kf_erase_host.cc"), os.path.join(d, "kf_erase_host")
    open(src, "w").write(HOST_DRIVER)
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", opt, "-std=c++11", "-Wall", "-I", CSRC, src, "-o", exe] + extra)   # without include/slamit.h
    return exe


def _arr(a, dt):
    a = np.ascontiguousarray(a, dt).reshape(-1)
    return np.int32(len(a)).tobytes() + a.tobytes()


def job_bytes(fx, child_cap, edit_cap):
    t, x = fx["t"], fx["x"]
    ed = records(fx["ops"])
    blob = np.array([t["n_kf"], t["n_mp"], x["row_cap"], x["origin_kf"], len(ed), child_cap, edit_cap, 0], np.int32).tobytes()
    for key in ("kf_mp_ptr", "kf_mp", "kf_child_ptr", "kf_child"):
        blob += _arr(t[key], np.int32)
    blob += _arr(x["kf_not_erase"], np.uint8)
    for key, dt in INPLACE:
        blob += _arr(source(fx, key), dt)
    blob += np.int32(len(ed)).tobytes() + ed.tobytes()
    f = fills(fx, child_cap, edit_cap)
    blob += _arr(f["child_ptr_out"], np.int32) + _arr(f["child_out"], np.int32) + _arr(f["op_status"], np.int32)
    blob += np.int32(edit_cap).tobytes() + f["edits"].tobytes()
    return blob


def _run(blob, sanitize):
    exe = host_exe(sanitize)
    d = os.path.dirname(exe)
    pin, pout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(pin, "wb").write(blob)
    subprocess.check_call([exe, pin, pout])
    return open(pout, "rb").read()


def host_run(jobs, sanitize=False):
    """jobs: (fixture, child_cap_out, edit_cap) through csrc/kf_erase.h on the host, in one process -> per job the arrays of OUT_KEYS."""
    return parse(_run(b"".join(job_bytes(fx, cc, ec) for fx, cc, ec in jobs), sanitize), jobs)


def parse(raw, jobs):
    o, outs = 0, []
    for fx, cc, ec in jobs:
        n_kf, rc, n = fx["t"]["n_kf"], fx["x"]["row_cap"], len(fx["ops"])
        counts = {"child_ptr_out": n_kf + 1, "child_out": cc, "kf_bad": n_kf, "kf_parent": n_kf, "kf_to_be_erased": n_kf, "cw_kf": n_kf * rc, "cw_w": n_kf * rc,
                  "cw_n": n_kf, "ord_kf": n_kf * rc, "ord_w": n_kf * rc, "ord_n": n_kf, "kf_best": n_kf * BEST, "op_status": n, "edits": ec * EDIT_DTYPE.itemsize}
        out = {}
        for key, dt in OUT_TYPES:
            out[key] = np.frombuffer(raw, dt, counts[key], o).copy()
            o += out[key].nbytes
        out["n_edits_out"], out["n_child_out"], out["status"] = (int(v) for v in np.frombuffer(raw, np.int32, 3, o))
        o += 12
        outs.append(out)
    assert o == len(raw)
    return outs


def resident_tables(fx):
    """The fixture's tables with every table api.MapIndex uploads (those the SetBadFlag calls do not read: empty or zero) and the dict
    api.CovisIndex takes."""
    t, x = fx["t"], fx["x"]
    n_mp = t["n_mp"]
    tables = dict(t, obs_ptr=np.zeros(n_mp + 1, np.int32), obs_kf=np.zeros(0, np.int32), mp_bad=np.zeros(n_mp, np.uint8), kf_best=x["kf_best"],
                  mp_pos=np.zeros((n_mp, 3), np.float32), mp_normal=np.zeros((n_mp, 3), np.float32), mp_max_dist=np.zeros(n_mp, np.float32),
                  mp_min_dist=np.zeros(n_mp, np.float32))
    covis = {k: x[k] for k in ("row_cap", "origin_kf", "kf_not_erase", "cw_kf", "cw_w", "cw_n", "ord_kf", "ord_w", "ord_n")}
    return tables, covis


def resident_run(fxs, caps, pad=3, indices=None):
    """One slamit_kf_erase_batch_dev call over the maps of fxs, every map with its own list length and its own (child_cap_out, edit_cap
    as far as the batch's edit_cap allows: the batch holds one edit_cap, so caps[m][1] must be equal across maps).  -> per map the arrays
    of OUT_KEYS in full (the children table: the whole other buffer set), and the index objects."""
    import torch
    from weiner_slamit_v2_amd import api

    B = len(fxs)
    edit_cap = caps[0][1]
    assert all(c[1] == edit_cap for c in caps)
    if indices is None:
        maps, covs, trees = [], [], []
        for fx, (cc, _) in zip(fxs, caps):
            tables, covis = resident_tables(fx)
            maps.append(api.MapIndex(tables))
            covs.append(api.CovisIndex(covis, maps[-1]))
            trees.append(api.TreeIndex({"kf_to_be_erased": fx["x"]["kf_to_be_erased"]}, maps[-1], covs[-1], cc))
    else:
        maps, covs, trees = indices
    for ti in trees:
        ti.sets[1]["kf_child_ptr"].fill_(FILL["child_ptr_out"])
        ti.sets[1]["kf_child"].fill_(FILL["child_out"])
    cap = max(len(fx["ops"]) for fx in fxs) + pad
    kf_cap, row_cap = max(fx["t"]["n_kf"] for fx in fxs) + 2, max(fx["x"]["row_cap"] for fx in fxs)
    child_cap = max(len(fx["t"]["kf_child"]) for fx in fxs) + 1
    h_ops = np.full((B, cap, 16), 0xff, np.uint8)
    for m, fx in enumerate(fxs):
        h_ops[m, :len(fx["ops"])] = records(fx["ops"]).view(np.uint8).reshape(-1, 16)
    cu = lambda a: torch.from_numpy(a).cuda()
    t = {"ops": cu(h_ops), "n": cu(np.array([len(fx["ops"]) for fx in fxs], np.int32)), "op_status": cu(np.full((B, cap), FILL["op_status"], np.int32)),
         "edits": cu(np.full((B, max(edit_cap, 1), EDIT_DTYPE.itemsize), FILL["edits"], np.uint8))[:, :edit_cap].contiguous(),
         "n_edits_out": cu(np.full(B, -3, np.int32)), "n_child_out": cu(np.full(B, -4, np.int32)), "status": cu(np.full(B, -1, np.int32)),
         "kf_cap": kf_cap, "row_cap": row_cap, "child_cap": child_cap,
         "workspace": torch.full((api.kf_erase_workspace(B, cap, kf_cap, row_cap, child_cap),), 0x5a, dtype=torch.uint8, device="cuda")}   # dirty: the call clears what it needs
    api.kf_erase_batch_dev(maps, trees, t, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    outs = []
    for m, (fx, mi, ci, ti) in enumerate(zip(fxs, maps, covs, trees)):
        n_kf, rc, n = fx["t"]["n_kf"], fx["x"]["row_cap"], len(fx["ops"])
        nxt = ti.sets[1]
        got = {"child_ptr_out": nxt["kf_child_ptr"].cpu().numpy()[:n_kf + 1], "child_out": nxt["kf_child"].cpu().numpy()[:ti.child_cap],
               "kf_bad": mi.t["kf_bad"].cpu().numpy()[:n_kf], "kf_parent": mi.t["kf_parent"].cpu().numpy()[:n_kf],
               "kf_to_be_erased": ti.t["kf_to_be_erased"].cpu().numpy()[:n_kf], "kf_best": mi.t["kf_best"].cpu().numpy()[:n_kf * BEST]}
        for key in ("cw_kf", "cw_w", "ord_kf", "ord_w"):
            got[key] = ci.t[key].cpu().numpy()[:n_kf * rc]
        for key in ("cw_n", "ord_n"):
            got[key] = ci.t[key].cpu().numpy()[:n_kf]
        row = lambda key: t[key][m].cpu().numpy()
        assert np.all(row("op_status")[n:] == FILL["op_status"])        # past the map's own list
        got.update(op_status=row("op_status")[:n], edits=row("edits").reshape(-1), n_edits_out=int(row("n_edits_out")), n_child_out=int(row("n_child_out")),
                   status=int(row("status")))
        outs.append(got)
    return outs, (maps, covs, trees), t
