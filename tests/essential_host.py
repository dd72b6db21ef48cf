"""Tensors of the resident essential-graph call (api.essential_graph_dev) from a problem on the host, and its result back: shared by
tests/test_gpu_essential.py, tests/test_gpu_essential_chain.py and tools/bench_essential.py."""
import ctypes as C

import numpy as np

from weiner_slamit_v2_amd import api

OUT_KEYS = ("sim3_r", "sim3_t", "sim3_s", "pose", "points")


def dev_tensors(g, n_free=None):
    import torch

    t = {}
    for k, dt in api._EG_PROBLEM_ARRAYS:
        t[k] = torch.from_numpy(np.ascontiguousarray(g[k], dt).reshape(-1).copy()).cuda()
    n, npt, ne = int(g["n_kf"]), len(g["pt_ref"]), len(g["edge_v0"])
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda")
    t.update(sim3_r=f64(n, 9), sim3_t=f64(n, 3), sim3_s=f64(n), pose=f64(n, 12), points=torch.full((npt, 3), -7.0, dtype=torch.float32, device="cuda"),
             touched=torch.full((npt,), -7, dtype=torch.int32, device="cuda"), n_touched=torch.full((1,), -7, dtype=torch.int32, device="cuda"),
             stats=torch.zeros(C.sizeof(api.EgStats), dtype=torch.uint8, device="cuda"))
    nf = int((~(np.asarray(g["fixed"]) | np.asarray(g["bad"])).astype(bool)).sum()) if n_free is None else n_free
    ws = api.essential_graph_workspace(min(nf, api.EG_MAX_KF), n, min(ne, api.EG_MAX_EDGES), npt)
    t["workspace"] = torch.zeros(ws + 256, dtype=torch.uint8, device="cuda")
    off = (-t["workspace"].data_ptr()) % 256
    t["workspace"] = t["workspace"][off:off + ws]
    return t, nf


def dev_result(t):
    out = {k: t[k].cpu().numpy() for k in OUT_KEYS}
    out["touched"] = t["touched"].cpu().numpy()[:int(t["n_touched"].cpu()[0])]
    out.update(api.eg_stats_from_bytes(t["stats"].cpu().numpy().tobytes()))
    return out
