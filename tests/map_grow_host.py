"""What the map-growth tests share: the arrays a call is given (the tables at their capacities, every output prefilled) and the arrays it must
leave, laid out from the restatement's result (tests/map_grow_ref.py); csrc/map_grow.h built with g++ behind a small main that takes any
number of jobs; one resident call over several maps; the comparison, exact and in full."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests.helpers import ROOT
from tests import map_grow_ref as ref

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
BEST = 10
OP_DTYPE = np.dtype([("kind", "<i4"), ("flags", "<i4"), ("kf", "<i4"), ("src", "<i4"), ("kf_id", "<i4"), ("cand", "<i4"), ("kf_a", "<i4"), ("idx_a", "<i4"),
                     ("kf_b", "<i4"), ("idx_b", "<i4"), ("weight_a", "u1"), ("weight_b", "u1"), ("pad", "u1", 2), ("pos", "<f4", 3)])
EDIT_DTYPE = np.dtype([("kind", "<i4"), ("flags", "<i4"), ("mp", "<i4"), ("kf", "<i4"), ("idx", "<i4"), ("octave", "u1"), ("weight", "u1"), ("pad", "u1", 2)])
REFUSED = 127
# slamit_grow_index in the record's order: name, type, entries as a function of (kf_cap, mp_cap, kfmp_cap)
INDEX = (("kf_mp_ptr", np.int32, lambda k, p, e: k + 1), ("kf_mp", np.int32, lambda k, p, e: e), ("kf_octave", np.uint8, lambda k, p, e: e),
         ("kf_desc", np.uint8, lambda k, p, e: 32 * e), ("kf_depth", np.float32, lambda k, p, e: e), ("kf_bad", np.uint8, lambda k, p, e: k),
         ("kf_parent", np.int32, lambda k, p, e: k), ("kf_to_be_erased", np.uint8, lambda k, p, e: k), ("kf_not_erase", np.uint8, lambda k, p, e: k),
         ("kf_th_depth", np.float32, lambda k, p, e: k), ("kf_best", np.int32, lambda k, p, e: BEST * k), ("cw_n", np.int32, lambda k, p, e: k),
         ("ord_n", np.int32, lambda k, p, e: k), ("kf_child_ptr", np.int32, lambda k, p, e: k + 1), ("kf_center", np.float32, lambda k, p, e: 3 * k),
         ("mp_pos", np.float32, lambda k, p, e: 3 * p), ("mp_normal", np.float32, lambda k, p, e: 3 * p), ("mp_max_dist", np.float32, lambda k, p, e: p),
         ("mp_min_dist", np.float32, lambda k, p, e: p), ("mp_bad", np.uint8, lambda k, p, e: p), ("mp_nobs", np.int32, lambda k, p, e: p),
         ("mp_ref_kf", np.int32, lambda k, p, e: p), ("mp_found", np.int32, lambda k, p, e: p), ("mp_visible", np.int32, lambda k, p, e: p),
         ("mp_first_kf", np.int32, lambda k, p, e: p), ("mp_replaced", np.int32, lambda k, p, e: p), ("mp_desc", np.uint8, lambda k, p, e: 32 * p),
         ("obs_ptr", np.int32, lambda k, p, e: p + 1))
OUTPUTS = (("op_status", np.int32), ("edits", np.uint8), ("recent", np.int32))
SCALARS = ("n_edits_out", "n_recent", "n_new", "status")
# what the caller leaves past the tables and in the outputs before the call
FILL = {np.int32: -7, np.uint8: 0xee, np.float32: -3.5}
FILL_SCALAR = -11


def records(ops):
    out = np.zeros(len(ops), OP_DTYPE)
    for k in OP_DTYPE.names:
        if k != "pad" and len(ops):
            out[k] = [e[k] for e in ops]
    return out


def default_caps(fx, pad=2, cap_pad=1):
    """Capacities that suffice by the gate's own bounds, and `pad` more of each."""
    need, _ = ref.needs(fx, dict(kf_cap=1 << 30, mp_cap=1 << 30, kfmp_cap=1 << 30, edit_cap=1 << 30, recent_cap=1 << 30))
    caps = {k: n + pad for k, n in zip(("kf_cap", "mp_cap", "kfmp_cap", "edit_cap", "recent_cap"), need)}
    caps.update(cand_cap=len(fx["cand_status"]) + pad, cap=len(fx["ops"]) + cap_pad)
    return caps


def inputs(fx, caps):
    """Every array the call reads or writes, at its capacity: the tables in front, the caller's fill behind; the outputs all fill."""
    t = fx["t"]
    a = {}
    for key, dt, count in INDEX:
        if t[key] is None:
            a[key] = None
            continue
        full = np.full(count(caps["kf_cap"], caps["mp_cap"], caps["kfmp_cap"]), FILL[dt], dt)
        src = np.ascontiguousarray(t[key], dt).reshape(-1)
        full[:len(src)] = src
        a[key] = full
    a["obs_kf"] = np.ascontiguousarray(t["obs_kf"], np.int32).reshape(-1)
    a["op_status"] = np.full(caps["cap"], FILL[np.int32], np.int32)
    a["edits"] = np.full(caps["edit_cap"] * EDIT_DTYPE.itemsize, FILL[np.uint8], np.uint8)
    a["recent"] = np.full(caps["recent_cap"], FILL[np.int32], np.int32)
    a["recent"][:len(fx["recent"])] = fx["recent"]
    a["cand_status"] = np.full(caps["cand_cap"], FILL[np.uint8], np.uint8)
    a["cand_status"][:len(fx["cand_status"])] = fx["cand_status"]
    a["cand_x3d"] = np.full((caps["cand_cap"], 3), FILL[np.float32], np.float32)
    a["cand_x3d"][:len(fx["cand_x3d"])] = fx["cand_x3d"]
    return a


def laid_out(fx, caps):
    """The arrays of INDEX and OUTPUTS, the scalars and the needs as the call must leave them, from the restatement."""
    want = ref.apply(fx, caps)
    e = inputs(fx, caps)
    e["need"] = list(want["need"])
    e.update({k: FILL_SCALAR for k in SCALARS}, n_recent=len(fx["recent"]), status=want["status"])
    if want["status"] & REFUSED:
        return e, want
    t = fx["t"]
    n_kf, n_mp, P = t["n_kf"], t["n_mp"], want["P"]
    end = int(t["kf_mp_ptr"][n_kf])
    for kf in want["kfs"]:
        if kf.new:
            k, n = kf.slot, len(kf.mvpMapPoints)
            e["kf_octave"][end:end + n] = kf.octave
            e["kf_desc"][32 * end:32 * (end + n)] = kf.desc.reshape(-1)
            if e["kf_depth"] is not None:
                e["kf_depth"][end:end + n] = kf.depth if kf.depth is not None else -1.0
                e["kf_th_depth"][k] = kf.th_depth
            end += n
            e["kf_mp_ptr"][k + 1] = end
            e["kf_bad"][k] = e["kf_to_be_erased"][k] = e["kf_not_erase"][k] = e["cw_n"][k] = e["ord_n"][k] = 0
            e["kf_parent"][k] = -1
            e["kf_best"][BEST * k:BEST * (k + 1)] = -1
            e["kf_child_ptr"][k + 1] = e["kf_child_ptr"][k]
            e["kf_center"][3 * k:3 * k + 3] = kf.center
        r0 = e["kf_mp_ptr"][kf.slot]
        e["kf_mp"][r0:r0 + len(kf.mvpMapPoints)] = kf.mvpMapPoints
    for q in range(n_mp, n_mp + P):
        mp = want["mps"][q] if q < len(want["mps"]) else None           # past the accepted ones: the inert tail
        e["mp_pos"][3 * q:3 * q + 3] = mp.pos if mp else 0
        e["mp_normal"][3 * q:3 * q + 3] = 0
        e["mp_max_dist"][q] = e["mp_min_dist"][q] = 0
        e["mp_bad"][q], e["mp_nobs"][q], e["mp_ref_kf"][q] = (0, 0, mp.mpRefKF) if mp else (1, 0, -1)
        e["mp_found"][q] = e["mp_visible"][q] = 1 if mp else 0
        e["mp_first_kf"][q], e["mp_replaced"][q] = mp.mnFirstKFid if mp else 0, -1
        e["mp_desc"][32 * q:32 * q + 32] = 0
        e["obs_ptr"][q + 1] = e["obs_ptr"][n_mp]
    n = len(fx["ops"])
    e["op_status"][:n] = want["op_status"]
    ed = np.zeros(len(want["edits"]), EDIT_DTYPE)
    for i, (kind, flags, p, k, idx, octave, weight) in enumerate(want["edits"]):
        ed[i] = (kind, flags, p, k, idx, octave, weight, (0, 0))
    e["edits"][:ed.nbytes] = ed.view(np.uint8)
    e["recent"][:len(want["recent"])] = want["recent"]
    e.update(n_edits_out=len(want["edits"]), n_recent=len(want["recent"]), n_new=want["n_new"])
    return e, want


def assert_same(got, want, what=""):
    for k in [k for k, _, _ in INDEX] + [k for k, _ in OUTPUTS] + list(SCALARS) + ["need"]:
        if want[k] is None:
            continue
        a, b = np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8) if a.dtype == np.float32 else a, b.view(np.uint8) if b.dtype == np.float32 else b), \
            "%s %s: %s" % (what, k, (np.flatnonzero(a != b)[:8], a[:16], b[:16]) if a.shape == b.shape else (a.shape, b.shape))


HOST_DRIVER = r"""
// csrc/map_grow.h's sequential statement over any number of jobs: per job a header and every array in (a length in bytes, -1 for NULL,
// then the bytes), every array the call may write out.  Every array lives in its own allocation of exactly its size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "map_grow.h"

struct Blob { unsigned char* p; int32_t n; };
static Blob rd(FILE* f) {
    Blob b = {0, 0};
    if (fread(&b.n, 4, 1, f) != 1) exit(2);
    if (b.n < 0) return b;
    b.p = (unsigned char*)malloc(b.n ? (size_t)b.n : 1);
    if (b.n && fread(b.p, 1, (size_t)b.n, f) != (size_t)b.n) exit(2);
    return b;
}
static void wr(FILE* f, const Blob& b) { if (b.p && b.n) fwrite(b.p, 1, (size_t)b.n, f); }

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) return 1;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 1;
    const int reps = argc == 4 && atoi(argv[3]) > 1 ? atoi(argv[3]) : 1;
    int32_t h[12];   // n_kf n_mp kf_cap mp_cap kfmp_cap n_frames n_given cap cand_cap edit_cap recent_cap n_recent
    while (fread(h, 4, 12, f) == 12) {
        std::vector<Blob> all;
        Blob ix[28];
        for (int q = 0; q < 28; ++q) { ix[q] = rd(f); all.push_back(ix[q]); }
        MgIndex X = MgIndex();
        X.kf_cap = h[2]; X.mp_cap = h[3]; X.kfmp_cap = h[4];
        void** slot = (void**)&X.kf_mp_ptr;
        for (int q = 0; q < 28; ++q) slot[q] = ix[q].p;
        const Blob obs_kf = rd(f);
        all.push_back(obs_kf);
        std::vector<MgFrame> frames((size_t)h[5] + 1);
        for (int q = 0; q < h[5]; ++q) {
            int32_t n_kp; float th;
            if (fread(&n_kp, 4, 1, f) != 1 || fread(&th, 4, 1, f) != 1) return 2;
            Blob b[6];
            for (int u = 0; u < 6; ++u) { b[u] = rd(f); all.push_back(b[u]); }
            MgFrame& F = frames[(size_t)q];
            F.n_kp = n_kp; F.th_depth = th; F.frame_mp = (const int32_t*)b[0].p; F.octave = b[1].p; F.desc = b[2].p; F.depth = (const float*)b[3].p;
            F.uright = (const float*)b[4].p; F.Tcw = (const float*)b[5].p;
        }
        const Blob ops = rd(f), cand_status = rd(f), cand_x3d = rd(f), ost = rd(f), edits = rd(f), recent = rd(f);
        const Blob rest[6] = {ops, cand_status, cand_x3d, ost, edits, recent};
        for (int u = 0; u < 6; ++u) all.push_back(rest[u]);
        int32_t tail[4 + MG_NNEED] = {-11, h[11], -11, -11, 0, 0, 0, 0, 0};   // n_edits_out n_recent n_new status need[5]
        // the bench runs a job many times over fresh copies of everything the walk writes
        std::vector<Blob> written(ix, ix + 28);
        written.push_back(ost); written.push_back(edits); written.push_back(recent);
        std::vector<std::vector<unsigned char> > fresh;
        for (size_t q = 0; q < written.size() && reps > 1; ++q) fresh.push_back(std::vector<unsigned char>(written[q].p, written[q].p + (written[q].p ? written[q].n : 0)));
        std::vector<double> ms;
        for (int r = 0; r < reps; ++r) {
            for (size_t q = 0; q < fresh.size(); ++q)
                if (!fresh[q].empty()) memcpy(written[q].p, fresh[q].data(), fresh[q].size());
            tail[0] = -11; tail[1] = h[11]; tail[2] = -11; tail[3] = -11;
            const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            mg_apply_seq(h[0], h[1], (const int32_t*)obs_kf.p, X, h[5], frames.data(), h[6], h[7], (const MgOp*)ops.p, h[8], cand_status.p, (const float*)cand_x3d.p,
                         (int32_t*)ost.p, h[9], (MeEdit*)edits.p, &tail[0], h[10], (int32_t*)recent.p, &tail[1], &tail[2], &tail[4], &tail[3]);
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        if (argc == 4) printf("%f %f\n", ms[ms.size() / 2], ms[0]);       // the job's median and fastest walk
        for (int q = 0; q < 28; ++q) wr(o, ix[q]);
        wr(o, ost); wr(o, edits); wr(o, recent);
        fwrite(tail, 4, 4 + MG_NNEED, o);
        for (size_t q = 0; q < all.size(); ++q) free(all[q].p);
    }
    fclose(f);
    fclose(o);
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def host_exe(sanitize=False, opt="-O2"):
    d = tempfile.mkdtemp(prefix="map_grow_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "map_grow_host.cc"), os.path.join(d, "map_grow_host")
    open(src, "w").write(HOST_DRIVER)
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", opt, "-std=c++11", "-Wall", "-ffp-contract=off", "-I", CSRC, src, "-o", exe] + extra)   # without include/slamit.h
    return exe


def _blob(a):
    if a is None:
        return np.int32(-1).tobytes()
    a = np.ascontiguousarray(a)
    return np.int32(a.nbytes).tobytes() + a.tobytes()


def job_bytes(fx, caps, n_given=None):
    t, a = fx["t"], inputs(fx, caps)
    ops = records(fx["ops"])
    held = np.zeros(caps["cap"], OP_DTYPE)
    held[:min(len(ops), caps["cap"])] = ops[:caps["cap"]]
    blob = np.array([t["n_kf"], t["n_mp"], caps["kf_cap"], caps["mp_cap"], caps["kfmp_cap"], len(fx["frames"]), len(ops) if n_given is None else n_given, caps["cap"],
                     caps["cand_cap"], caps["edit_cap"], caps["recent_cap"], len(fx["recent"])], np.int32).tobytes()
    for key, _, _ in INDEX:
        blob += _blob(a[key])
    blob += _blob(a["obs_kf"])
    for f in fx["frames"]:
        blob += np.int32(len(f["frame_mp"])).tobytes() + np.float32(f["th_depth"]).tobytes()
        for key in ("frame_mp", "octave", "desc", "depth", "uright", "Tcw"):
            blob += _blob(f[key])
    for key in ("cand_status", "cand_x3d", "op_status", "edits", "recent"):
        blob = blob + (_blob(held) if key == "cand_status" else b"") + _blob(a[key])
    return blob


def host_run(jobs, sanitize=False):
    """jobs: (fixture, caps) through csrc/map_grow.h on the host, in one process -> per job the arrays of INDEX and OUTPUTS, the scalars, need."""
    exe = host_exe(sanitize)
    d = os.path.dirname(exe)
    pin, pout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(pin, "wb").write(b"".join(job_bytes(fx, caps) for fx, caps in jobs))
    subprocess.check_call([exe, pin, pout])
    return parse(open(pout, "rb").read(), jobs)


def parse(raw, jobs):
    o, outs = 0, []
    for fx, caps in jobs:
        a, out = inputs(fx, caps), {}
        for key, dt in [(k, d_) for k, d_, _ in INDEX] + list(OUTPUTS):
            if a[key] is None:
                out[key] = None
                continue
            out[key] = np.frombuffer(raw, dt, len(a[key]), o).copy()
            o += out[key].nbytes
        tail = np.frombuffer(raw, np.int32, 9, o).tolist()
        o += 36
        out.update(n_edits_out=tail[0], n_recent=tail[1], n_new=tail[2], status=tail[3], need=tail[4:])
        outs.append(out)
    assert o == len(raw)
    return outs


def api_run(fx, caps):
    """api.map_grow (the host form) over the fixture with every output prefilled -> the arrays of INDEX and OUTPUTS in full, the scalars, need."""
    from weiner_slamit_v2_amd import api

    a, n = inputs(fx, caps), len(fx["ops"])
    fill = {k: a[k] for k, _, _ in INDEX if a[k] is not None}
    fill.update(op_status=a["op_status"][:n], edits=a["edits"], recent=a["recent"], n_edits_out=FILL_SCALAR, n_new=FILL_SCALAR)
    out = api.map_grow(fx["t"], None, records(fx["ops"]), fx["frames"], {"status": a["cand_status"], "x3d": a["cand_x3d"]}, recent=fx["recent"],
                       caps={k: caps[k] for k in ("kf_cap", "mp_cap", "kfmp_cap", "edit_cap", "recent_cap")}, fill=fill)
    got = {k: out["raw"].get(k) for k, _, _ in INDEX}
    got.update(op_status=np.concatenate([out["raw"]["op_status"], a["op_status"][n:]]), edits=out["raw"]["edits"], recent=out["raw"]["recent"], need=out["need"],
               n_edits_out=out["n_edits_out"], n_recent=out["n_recent"], n_new=out["n_new"], status=out["status"])
    return got, out


def resident_run(fxs, caps_list, pad=1):
    """One slamit_map_grow_batch_dev call over the maps of fxs, every map with its own tables, capacities and list; the frame records of all
    maps in one array (an op's src is moved by its map's base).  The batch holds one cap, cand_cap, edit_cap, recent_cap: those of
    caps_list must agree.  -> per map the arrays of INDEX and OUTPUTS in full, the scalars, need."""
    import copy

    import torch
    from weiner_slamit_v2_amd import api

    B = len(fxs)
    cap, cand_cap, edit_cap, recent_cap = (caps_list[0][k] for k in ("cap", "cand_cap", "edit_cap", "recent_cap"))
    assert all(c["cap"] == cap and c["cand_cap"] == cand_cap and c["edit_cap"] == edit_cap and c["recent_cap"] == recent_cap for c in caps_list)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep, tables, map_recs, grow_recs, frame_recs, ins = [], [], [], [], [], []
    h_ops = np.full((B, max(cap, 1), OP_DTYPE.itemsize), 0xff, np.uint8)
    for m, (fx, caps) in enumerate(zip(fxs, caps_list)):
        a = inputs(fx, caps)
        ins.append(a)
        dev = {k: cu(v if len(v) else np.zeros(1, v.dtype)) for k, v in a.items() if v is not None and k in [q for q, _, _ in INDEX] + ["obs_kf"]}
        tables.append(dev)
        mr = api.MapIndexRec(fx["t"]["n_kf"], fx["t"]["n_mp"])
        mr.obs_kf, mr.obs_ptr = dev["obs_kf"].data_ptr(), dev["obs_ptr"].data_ptr()
        map_recs.append(mr)
        grow_recs.append(api.grow_index_rec(dev, caps["kf_cap"], caps["mp_cap"], caps["kfmp_cap"]))
        base = len(frame_recs)
        for f in fx["frames"]:
            d = {k: cu(v if len(v) else np.zeros(16, v.dtype)) for k, v in f.items() if k != "th_depth" and v is not None}
            keep.append(d)
            fr = api.grow_frame_rec(dict(d, th_depth=f["th_depth"])) if len(f["frame_mp"]) else api.GrowFrameRec(0, f["th_depth"], d["frame_mp"].data_ptr(),
                                                                                                               d["octave"].data_ptr(), d["desc"].data_ptr(), None, None, d["Tcw"].data_ptr())
            frame_recs.append(fr)
        ops = copy.deepcopy(fx["ops"])
        for e in ops:
            if e["kind"] in (ref.NEW_KF, ref.ASSOCIATE) and 0 <= e["src"] < len(fx["frames"]):
                e["src"] += base
            elif e["kind"] in (ref.NEW_KF, ref.ASSOCIATE):
                e["src"] = -1 if e["src"] < 0 else 1000                  # outside the map's own records: outside the batch's
        h_ops[m, :len(ops)] = records(ops).view(np.uint8).reshape(-1, OP_DTYPE.itemsize)[:cap]
    mp_cap = max(c["mp_cap"] for c in caps_list) + pad
    t = {"ops": cu(h_ops)[:, :cap].contiguous(), "n": cu(np.array([len(fx["ops"]) for fx in fxs], np.int32)),
         "cand_status": cu(np.stack([a["cand_status"] for a in ins])), "cand_x3d": cu(np.stack([a["cand_x3d"] for a in ins])),
         "op_status": cu(np.stack([a["op_status"] for a in ins])), "edits": cu(np.stack([a["edits"] for a in ins]).reshape(B, edit_cap, EDIT_DTYPE.itemsize)),
         "n_edits_out": cu(np.full(B, FILL_SCALAR, np.int32)), "recent": cu(np.stack([a["recent"] for a in ins])),
         "n_recent": cu(np.array([len(fx["recent"]) for fx in fxs], np.int32)), "n_new": cu(np.full(B, FILL_SCALAR, np.int32)),
         "need": cu(np.full((B, api.GROW_NEEDS), -1, np.int32)), "status": cu(np.full(B, FILL_SCALAR, np.int32)), "mp_cap": mp_cap,
         "workspace": torch.full((api.map_grow_workspace(B, mp_cap),), 0x5a, dtype=torch.uint8, device="cuda")}   # dirty: the call clears what it needs
    api.map_grow_batch_dev(map_recs, grow_recs, frame_recs, t, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    outs = []
    for m, (fx, a) in enumerate(zip(fxs, ins)):
        got = {k: (tables[m][k].cpu().numpy()[:len(a[k])] if a[k] is not None else None) for k, _, _ in INDEX}
        row = lambda key: t[key][m].cpu().numpy()
        got.update(op_status=row("op_status"), edits=row("edits").reshape(-1), recent=row("recent"), need=row("need").tolist())
        got.update({k: int(row(k)) for k in SCALARS})
        outs.append(got)
    return outs, t
