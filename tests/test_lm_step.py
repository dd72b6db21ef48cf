"""The scalar Levenberg rules on the CPU: csrc/lm_step.h (the damped single-block solve, the lambda seed, the accept / reject update,
the stop rules that pose.hip, sim3.hip and the local BA's k_decide all call) is built with g++ together with a small C driver (no HIP).
lm_solve is compared bit for bit with a restatement in Python floats (IEEE doubles, no fused multiply-add; the driver is built with
-ffp-contract=off, as oracle/Makefile builds the oracle) on normal matrices of the pose and Sim3 goldens; the rules are driven over every branch."""
import ctypes as C
import glob
import math
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT, load_pose_golden, load_sim3_golden

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
DBL_MAX = float(np.finfo(np.float64).max)

DRIVER = r'''
#include "lm_step.h"

extern "C" int drv_solve(int D, const double* H, double lambda, const double* b, double* x) {
    return D == 6 ? lm_solve<6>(H, lambda, b, x) : lm_solve<7>(H, lambda, b, x);
}
extern "C" double drv_lambda_init(int D, const double* H) { return D == 6 ? lm_lambda_init<6>(H) : lm_lambda_init<7>(H); }
// io: cur, lambda, ni in and out; returns rho
extern "C" double drv_accept(double temp, double scale, double* io, int* accepted) {
    bool a = false;
    const double rho = lm_accept(io[0], temp, scale, io[1], io[2], a);
    *accepted = a;
    return rho;
}
extern "C" int drv_try_again(double rho, int qmax) { return lm_try_again(rho, qmax); }
extern "C" int drv_stop(int qmax, double rho, double iniChi, double cur, int* nBad) { return lm_stop(qmax, rho, iniChi, cur, *nBad); }
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("lm_step"))
    drv = os.path.join(tmp, "lm_step_driver.cc")
    with open(drv, "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "liblm_step_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", CSRC, drv, "-o", so])
    L = C.CDLL(so)
    L.drv_solve.argtypes = [C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    L.drv_lambda_init.argtypes = [C.c_int, C.c_void_p]
    L.drv_lambda_init.restype = C.c_double
    L.drv_accept.argtypes = [C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    L.drv_accept.restype = C.c_double
    L.drv_try_again.argtypes = [C.c_double, C.c_int]
    L.drv_stop.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
    return L


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def solve(lib, H, lam, b):
    D = len(b)
    H = np.ascontiguousarray(H, np.float64).reshape(D * D)
    b = np.ascontiguousarray(b, np.float64)
    x = np.zeros(D)
    return bool(lib.drv_solve(D, _ptr(H), float(lam), _ptr(b), _ptr(x))), x


def solve_py(H, lam, b):
    """lm_solve in Python floats, operation for operation: LDLt of H + lambda I without pivoting (the factor in the lower triangle, D
    on the diagonal), forward substitution, the division by D, back substitution.  -> x, or None on a zero / non-finite pivot."""
    D = len(b)
    A = [float(H[i // D][i % D]) + (float(lam) if i % (D + 1) == 0 else 0.0) for i in range(D * D)]
    for j in range(D):
        d = A[(D + 1) * j]
        for k in range(j):
            d -= A[D * j + k] * A[D * j + k] * A[(D + 1) * k]
        if d == 0.0 or not abs(d) <= DBL_MAX:
            return None
        A[(D + 1) * j] = d
        for i in range(j + 1, D):
            s = A[D * i + j]
            for k in range(j):
                s -= A[D * i + k] * A[D * j + k] * A[(D + 1) * k]
            A[D * i + j] = s / d
    x = [0.0] * D
    for i in range(D):
        s = float(b[i])
        for k in range(i):
            s -= A[D * i + k] * x[k]
        x[i] = s
    for i in range(D):
        x[i] /= A[(D + 1) * i]
    for i in range(D - 1, -1, -1):
        s = x[i]
        for k in range(i + 1, D):
            s -= A[D * k + i] * x[k]
        x[i] = s
    return np.array(x)


def _proj_jac(X, fx, fy):
    """d (fx x / z, fy y / z) / d X, per point: n x 2 x 3"""
    x, y, iz = X[:, 0], X[:, 1], 1.0 / X[:, 2]
    J = np.zeros((len(X), 2, 3))
    J[:, 0, 0] = fx * iz; J[:, 0, 2] = -fx * x * iz * iz
    J[:, 1, 1] = fy * iz; J[:, 1, 2] = -fy * y * iz * iz
    return J


def _skew(X):
    S = np.zeros((len(X), 3, 3))
    S[:, 0, 1] = -X[:, 2]; S[:, 0, 2] = X[:, 1]; S[:, 1, 0] = X[:, 2]; S[:, 1, 2] = -X[:, 0]; S[:, 2, 0] = -X[:, 1]; S[:, 2, 1] = X[:, 0]
    return S


def _normal(J, r, w):
    """J: n x 2 x D, r: n x 2, w: n -> (J^T W J, -J^T W r), the Gauss-Newton system of the edges in front of the camera"""
    ok = np.isfinite(J).all(axis=(1, 2)) & np.isfinite(r).all(axis=1)
    J, r, w = J[ok], r[ok], w[ok]
    H = np.triu(np.einsum("nia,n,nib->ab", J, w, J))   # the upper triangle, mirrored: as the kernels fill H
    return H + np.triu(H, 1).T, -np.einsum("nia,n,ni->a", J, w, r)


def pose_system(path):
    """The 6 x 6 normal equations of a pose golden's monocular rows at its initial pose (increment = [omega, upsilon], pose.hip)."""
    p, _ = load_pose_golden(path)
    T = p["pose"].reshape(-1)
    R, t = T[:9].reshape(3, 3), T[9:12]
    fx, fy, cx, cy = p["intr"]
    X = p["xw"] @ R.T + t
    with np.errstate(all="ignore"):
        Jp = _proj_jac(X, fx, fy)
        J = -np.concatenate([Jp @ -_skew(X), Jp], axis=2)
        r = p["uv"] - np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], axis=1)
        return _normal(J, r, p["inv_sigma2"])


def sim3_system(path):
    """The 7 x 7 normal equations of a Sim3 golden's pairs at its initial S12 (increment = [omega, upsilon, sigma], sim3.hip)."""
    p, _ = load_sim3_golden(path)
    R, t, s = p["r12"].reshape(3, 3), p["t12"].reshape(3), p["s12"]
    with np.errstate(all="ignore"):
        Y = s * p["p2"] @ R.T + t                       # S p2, seen by camera 1
        dY = np.concatenate([-_skew(Y), np.tile(np.eye(3), (len(Y), 1, 1)), Y[:, :, None]], axis=2)
        f1, f2 = p["intr1"], p["intr2"]
        J12 = -_proj_jac(Y, f1[0], f1[1]) @ dY
        r12 = p["obs1"] - np.stack([f1[0] * Y[:, 0] / Y[:, 2] + f1[2], f1[1] * Y[:, 1] / Y[:, 2] + f1[3]], axis=1)
        Z = (p["p1"] - t) @ R / s                       # S^-1 p1, seen by camera 2
        dP = np.concatenate([-_skew(p["p1"]), np.tile(np.eye(3), (len(Z), 1, 1)), p["p1"][:, :, None]], axis=2)
        J21 = _proj_jac(Z, f2[0], f2[1]) @ (R.T / s) @ dP
        r21 = p["obs2"] - np.stack([f2[0] * Z[:, 0] / Z[:, 2] + f2[2], f2[1] * Z[:, 1] / Z[:, 2] + f2[3]], axis=1)
        Ha, ba = _normal(J12, r12, p["inv_sigma2_1"])
        Hb, bb = _normal(J21, r21, p["inv_sigma2_2"])
    return Ha + Hb, ba + bb


POSE_GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pose_*.npz")))
SIM3_GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sim3_*.npz")))
LAMBDA_FACTORS = [0.0, 1e-5, 1e-3, 2.0 / 3.0, 1.0, 37.5, 1e6]   # times the largest |H_jj|: the seed, and where rejects drive it


def test_the_goldens_are_there():
    assert len(POSE_GOLDEN) >= 10 and len(SIM3_GOLDEN) >= 6


@pytest.mark.parametrize("path", POSE_GOLDEN + SIM3_GOLDEN, ids=[os.path.basename(p)[:-4] for p in POSE_GOLDEN + SIM3_GOLDEN])
def test_solve_matches_the_restatement_bit_for_bit(lib, path):
    H, b = pose_system(path) if os.path.basename(path).startswith("pose_") else sim3_system(path)
    D = len(b)
    assert D == (6 if os.path.basename(path).startswith("pose_") else 7) and np.isfinite(H).all() and np.array_equal(H, H.T)
    top = np.abs(np.diag(H)).max()
    seed = lib.drv_lambda_init(D, _ptr(np.ascontiguousarray(H).reshape(-1)))
    assert seed == 1e-5 * top
    solved = 0
    for fac in LAMBDA_FACTORS:
        lam = fac * top
        ok, x = solve(lib, H, lam, b)
        want = solve_py(H, lam, b)
        assert ok == (want is not None), (path, fac)
        if ok:
            solved += 1
            assert np.array_equal(x.view(np.uint64), want.view(np.uint64)), (path, fac, x, want)
            if top > 0:   # and it IS the solution, to what the conditioning of a damped system allows
                A = H + lam * np.eye(D)
                assert np.abs(A @ x - b).max() <= 1e-6 * max(np.abs(b).max(), np.abs(A).max() * np.abs(x).max()), (path, fac)
    assert solved >= (len(LAMBDA_FACTORS) - 1 if top > 0 else 0), path   # (an undamped system of too few edges may be singular)


def test_solve_on_plain_systems(lib):
    for D in (6, 7):
        ok, x = solve(lib, np.eye(D), 1.0, np.arange(1.0, D + 1))
        assert ok and np.array_equal(x, np.arange(1.0, D + 1) / 2)
        rs = np.random.RandomState(D)
        for _ in range(50):
            M = rs.randn(D + 3, D)
            H, b, lam = M.T @ M, rs.randn(D), 10.0 ** rs.uniform(-6, 2)
            ok, x = solve(lib, H, lam, b)
            assert ok and np.array_equal(x.view(np.uint64), solve_py(H, lam, b).view(np.uint64))


def test_solve_refuses_a_zero_or_non_finite_pivot(lib):
    for D in (6, 7):
        b = np.ones(D)
        assert solve(lib, np.zeros((D, D)), 0.0, b)[0] is False                      # the first pivot is exactly zero
        H = np.eye(D)
        H[:2, :2] = [[1.0, 1.0], [1.0, 1.0]]
        assert solve(lib, H, 0.0, b)[0] is False and solve_py(H, 0.0, b) is None      # the second one cancels to exactly zero
        assert solve(lib, H, 0.5, b)[0] is True                                      # damped, the same block solves
        H = np.eye(D)
        H[D - 1, D - 1] = 0.0
        assert solve(lib, H, 0.0, b)[0] is False                                     # the last one
        for bad in (np.inf, -np.inf, np.nan):
            for j in (0, 3, D - 1):
                H = np.eye(D)
                H[j, j] = bad
                assert solve(lib, H, 1e-3, b)[0] is False, (D, bad, j)
        assert solve(lib, np.eye(D), np.inf, b)[0] is False and solve(lib, np.eye(D), np.nan, b)[0] is False
        H = np.eye(D) * 1e308
        H[1, 0] = H[0, 1] = 1e308 * 1.5                                               # 1e308 - 1.5^2 1e308 overflows: a non-finite pivot
        H[0, 0] = 1e-308
        assert solve(lib, H, 0.0, b)[0] is False


def accept(lib, cur, temp, scale, lam, ni):
    io = np.array([cur, lam, ni], np.float64)
    acc = C.c_int(-1)
    rho = lib.drv_accept(float(temp), float(scale), _ptr(io), C.byref(acc))
    return rho, bool(acc.value), io[0], io[1], io[2]


def test_accept_scales_lambda_between_a_third_and_two_thirds(lib):
    # rho = (cur - temp) / (scale + 1e-3); lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)); ni = 2; the cost becomes temp
    rho, acc, cur, lam, ni = accept(lib, 10.0, 9.0, 4.0 - 1e-3, 8.0, 16.0)       # rho = 0.25: 1 - (-0.5)^3 = 1.125, clamped at 2/3
    assert rho == 1.0 / 4.0 and acc and cur == 9.0 and lam == 8.0 * (2.0 / 3.0) and ni == 2.0
    rho, acc, cur, lam, ni = accept(lib, 10.0, 9.0, 2.0 - 1e-3, 8.0, 4.0)        # rho = 0.5: alpha = 1, clamped at 2/3
    assert rho == 0.5 and acc and lam == 8.0 * (2.0 / 3.0) and ni == 2.0
    rho, acc, cur, lam, ni = accept(lib, 10.0, 2.0, 8.0 - 1e-3, 3.0, 2.0)        # rho = 1: alpha = 0, the floor of 1/3
    assert rho == 1.0 and acc and cur == 2.0 and lam == 3.0 * (1.0 / 3.0) and ni == 2.0
    rho, acc, cur, lam, ni = accept(lib, 10.0, 1.0, 3.0 - 1e-3, 3.0, 2.0)        # rho = 3: alpha = -124, the floor
    assert rho == 3.0 and acc and lam == 3.0 * (1.0 / 3.0)
    scale = 1.0 / 0.85 - 1e-3                                                    # rho ~ 0.85: alpha = 1 - 0.7^3 = 0.657, between the clamps
    rho, acc, cur, lam, ni = accept(lib, 10.0, 9.0, scale, 1.0, 2.0)
    alpha = 1.0 - math.pow(2 * rho - 1, 3)
    assert abs(rho - 0.85) < 1e-12 and acc and 1.0 / 3.0 < alpha < 2.0 / 3.0 and lam == alpha and ni == 2.0


def test_reject_multiplies_lambda_by_a_doubling_ni(lib):
    cur, lam, ni = 10.0, 1.0, 2.0
    for k in range(6):   # consecutive rejects: lambda x 2, x 4, x 8 ..., the cost untouched
        rho, acc, cur, lam, ni = accept(lib, cur, 11.0, 1.0, lam, ni)
        assert rho < 0 and not acc and cur == 10.0 and ni == 2.0 ** (k + 2) and lam == 2.0 ** ((k + 1) * (k + 2) // 2)
    rho, acc, cur, lam, ni = accept(lib, cur, 9.0, 1.0, lam, ni)                  # an accepted step puts ni back to 2
    assert rho > 0 and acc and ni == 2.0 and cur == 9.0


def test_a_failed_solve_and_a_non_finite_cost_are_rejects(lib):
    rho, acc, cur, lam, ni = accept(lib, 10.0, DBL_MAX, 0.0, 5.0, 4.0)            # the solve failed: temp = DBL_MAX, x = 0, scale = 0
    assert rho < 0 and math.isinf(rho) and not acc and (cur, lam, ni) == (10.0, 20.0, 8.0)
    assert lib.drv_try_again(rho, 1) == 1
    rho, acc, cur, lam, ni = accept(lib, 10.0, np.inf, 1.0, 5.0, 4.0)
    assert not acc and (cur, lam, ni) == (10.0, 20.0, 8.0)
    rho, acc, cur, lam, ni = accept(lib, 10.0, np.nan, 1.0, 5.0, 4.0)             # rho is NaN: not > 0, a reject; not < 0, no further trial
    assert math.isnan(rho) and not acc and (cur, lam, ni) == (10.0, 20.0, 8.0) and lib.drv_try_again(rho, 1) == 0
    rho, acc, cur, lam, ni = accept(lib, 10.0, -np.inf, 1.0, 5.0, 4.0)            # rho = +inf but the cost is not finite
    assert rho == np.inf and not acc and (cur, lam, ni) == (10.0, 20.0, 8.0)


def stop(lib, qmax, rho, ini, cur, nbad):
    n = C.c_int(nbad)
    return bool(lib.drv_stop(qmax, float(rho), float(ini), float(cur), C.byref(n))), n.value


def test_a_zero_gain_ratio_rejects_and_stops(lib):
    rho, acc, cur, lam, ni = accept(lib, 10.0, 10.0, 1.0, 5.0, 2.0)               # rho == 0: not an improvement
    assert rho == 0.0 and not acc and (cur, lam, ni) == (10.0, 10.0, 4.0)
    assert lib.drv_try_again(0.0, 1) == 0                                         # ... and not < 0: the trials end
    assert stop(lib, 1, 0.0, 10.0, 10.0, 0) == (True, 0)                          # Terminate; the run of bad iterations is not touched
    assert stop(lib, 1, -0.0, 10.0, 10.0, 2) == (True, 2)


def test_ten_rejects_end_the_trials_and_stop(lib):
    cur, lam, ni, qmax = 10.0, 1.0, 2.0, 0
    while True:
        rho, acc, cur, lam, ni = accept(lib, cur, 12.0, 1.0, lam, ni)
        qmax += 1
        assert not acc
        if not lib.drv_try_again(rho, qmax):
            break
    assert qmax == 10 and ni == 2.0 ** 11 and lam == 2.0 ** 55
    assert lib.drv_try_again(-1.0, 9) == 1 and lib.drv_try_again(-1.0, 10) == 0
    assert stop(lib, 10, rho, 10.0, 10.0, 0) == (True, 0)
    assert stop(lib, 10, 0.5, 10.0, 1.0, 0) == (True, 0)                          # (the tenth trial was accepted: g2o stops all the same)
    assert stop(lib, 9, 0.5, 10.0, 1.0, 0) == (False, 0)


def test_three_iterations_without_a_thousandth_of_gain_stop(lib):
    # bad: (iniChi - cur) * 1e3 < iniChi
    nbad = 0
    done, nbad = stop(lib, 1, 0.5, 1000.0, 999.5, nbad)
    assert (done, nbad) == (False, 1)
    done, nbad = stop(lib, 2, 0.5, 999.5, 999.0, nbad)
    assert (done, nbad) == (False, 2)
    done, nbad = stop(lib, 1, 0.5, 999.0, 900.0, nbad)                            # a good one in between: the run starts over
    assert (done, nbad) == (False, 0)
    for want in ((False, 1), (False, 2), (True, 3)):
        done, nbad = stop(lib, 1, 0.5, 900.0, 899.9, nbad)
        assert (done, nbad) == want
    assert stop(lib, 1, 0.5, 1000.0, 999.0, 0) == (False, 0)                      # exactly a thousandth is not bad: (1000 - 999) * 1e3 == 1000
    assert stop(lib, 1, 0.5, 1000.0, 999.0 + 1e-9, 2) == (True, 3)
    assert stop(lib, 3, 1e-300, 0.0, 0.0, 0) == (False, 0)                        # a zero cost: 0 < 0 is false
