"""Layout of the essential-graph entry points' structs: a C99 compile of include/slamit.h against the ctypes mirrors (no GPU)."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT

PAIRS = (("slamit_eg_graph", "EgGraph"), ("slamit_eg_problem", "EgProblem"), ("slamit_eg_stats", "EgStats"), ("slamit_eg_result", "EgResult"))
FUNCTIONS = ("slamit_essential_plan", "slamit_essential_graph", "slamit_essential_graph_dev")


def test_essential_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%d %d %d %d %d %d %d\\n", SLAMIT_EG_MAX_KF, SLAMIT_EG_MAX_EDGES, SLAMIT_EG_MAX_ITS, SLAMIT_EG_MAX_TRIALS, SLAMIT_EG_MAX_POINTS, SLAMIT_EG_NORMAL, SLAMIT_EG_LOOP_CONNECTION);\n'
    want = [api.EG_MAX_KF, api.EG_MAX_EDGES, api.EG_MAX_ITS, api.EG_MAX_TRIALS, api.EG_MAX_POINTS, api.EG_NORMAL, api.EG_LOOP_CONNECTION]
    for cname, pyname in PAIRS:
        mirror = getattr(api, pyname)
        src += '    printf("%%zu\\n", sizeof(%s));\n' % cname
        want.append(C.sizeof(mirror))
        for f, _ in mirror._fields_:
            src += '    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f)
            want.append(getattr(mirror, f).offset)
    src += "    return 0;\n}\n"
    c, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    assert [int(x) for x in subprocess.check_output([exe]).split()] == want
    assert (api.EG_MAX_KF, api.EG_MAX_EDGES, api.EG_MAX_ITS, api.EG_MAX_TRIALS, api.EG_MAX_POINTS) == (1024, 65536, 32, 320, 1 << 24)
    assert (C.sizeof(api.EgGraph), C.sizeof(api.EgProblem), C.sizeof(api.EgResult)) == (120, 160, 64)
    assert C.sizeof(api.EgStats) == 24 + 8 * 32 + 8 * 32 + 4 * 32 + 2 * 8 * 320


def test_essential_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in FUNCTIONS:
        assert "int %s(" % name in hdr and name in api.EXPORTS and hasattr(api.lib(), name)
    assert "size_t slamit_essential_graph_workspace(" in hdr and "slamit_essential_graph_workspace" in api.EXPORTS
    for src in ("essential.hip", "essential_plan.cc"):
        assert src in build.SOURCES and src not in build.PER_FILE      # -ffp-contract=off like the rest
    plan = open(os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc", "essential_plan.cc")).read() + \
        open(os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc", "essential_plan.h")).read()
    assert "hip" not in plan.replace("no HIP include", "").lower()      # the plan unit is host-only
    # the workspace: nothing for a count past a ceiling, the packed lower triangle at the ceiling
    L = api.lib()
    assert L.slamit_essential_graph_workspace(api.EG_MAX_KF + 1, 2000, 10, 0) == 0
    assert L.slamit_essential_graph_workspace(10, 20, api.EG_MAX_EDGES + 1, 0) == 0
    tri = 224 * 225 // 2 * 1024 * 8
    assert tri <= L.slamit_essential_graph_workspace(api.EG_MAX_KF, 1025, 1025, 0) < tri + (8 << 20)


def test_plan_through_the_library_needs_no_gpu():
    """slamit_essential_plan is host code: api.essential_plan equals the restatement on a machine without a device"""
    from tests import essential_ref as er
    from tests.test_essential_plan import as_lists
    from weiner_slamit_v2_amd import api, synth

    g = synth.synth_essential(n_kf=40, seed=6, mixed=True, n_pt=4)
    p = api.essential_plan(g)
    assert list(zip(p["edge_v0"].tolist(), p["edge_v1"].tolist(), p["edge_kind"].tolist())) == er.plan_edges(as_lists(g))
    g["kf_bad"][5] = 1
    try:
        api.essential_plan(g)
        raise AssertionError("a bad parent must refuse the call")
    except api.SlamitError as e:
        assert "(-1)" in str(e) and "bad" in str(e)
