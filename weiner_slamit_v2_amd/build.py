"""Builds libslamit_hip.so (HIP kernels + C-ABI) in-tree with hipcc for gfx950.

    python -m weiner_slamit_v2_amd.build [--force]

The library is git-ignored but travels to the GPU box with the snapshot.  hipcc cross-compiles
without a GPU.  -ffp-contract=off is part of the numerics (bit-exact float paths).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libslamit_hip.so")
SOURCES = ["slamit_misc.hip", "orb_kernels.hip", "orb_plan.cc", "orb_api.hip", "hamming.hip", "ba_kernels.hip", "ba_plan.cc", "ba_api.hip", "pose.hip", "search.hip", "frame.hip", "bow.hip", "voc_pack.cc", "voc.hip", "kfdb.hip", "sim3.hip", "sim3_ransac.hip", "pnp.hip", "initializer.hip", "triangulate.hip", "frustum.hip", "project.hip", "rotation.hip", "stereo.hip", "unproject.hip", "local_map.hip", "covis.hip", "upkeep.hip", "map_edit.hip", "map_replace.hip", "map_fuse.hip", "kf_erase.hip", "map_grow.hip", "essential_plan.cc", "essential.hip"]
# BA is fp64 with a 1e-5 tolerance, not bit-exact: let the compiler fuse multiply-adds there
# hamming.hip: the MFMA results feed VALU min / median directly, so its accumulators stay in VGPRs (no v_accvgpr moves)
PER_FILE = {"ba_kernels.hip": ["-ffp-contract=fast"], "pose.hip": ["-ffp-contract=fast"],
            "hamming.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}
FLAGS = [
    "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
    "-fno-gpu-rdc", "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def sources():
    return [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    deps += [os.path.join(HERE, "..", "include", f) for f in os.listdir(os.path.join(HERE, "..", "include"))]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not stale():
        return LIB
    objs = []
    procs = []
    for src in sources():
        obj = os.path.splitext(src)[0] + ".o"
        cmd = [hipcc()] + FLAGS + PER_FILE.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    failed = False
    for (src, p), obj in zip(procs, objs):
        out, _ = p.communicate()
        if p.returncode != 0 and "-mllvm" in PER_FILE.get(os.path.basename(src), []):
            # an internal compiler option (hamming.hip's accumulators in VGPRs) this hipcc may not know: the kernel is correct
            # without it (the compiler then moves the MFMA results out of the accumulator file itself), so build it plainly
            sys.stderr.write("%s: retrying without %s\n" % (os.path.basename(src), " ".join(PER_FILE[os.path.basename(src)])))
            cmd = [hipcc()] + FLAGS + ["-c", src, "-o", obj]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            p.returncode, out = r.returncode, r.stdout
        if p.returncode != 0:
            failed = True
            sys.stderr.write(out.decode(errors="replace"))
        elif verbose and out:
            sys.stderr.write(out.decode(errors="replace"))
    if failed:
        raise RuntimeError("hipcc failed")
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
