"""Error measures and assertions of the per-particle material parity tests, shared by the 3D test of ill-conditioned F
(tests/test_gpu_illcond.py), the 2D device tests (tests/test_gpu_materials2d.py) and their CPU twins
(tests/test_materials2d_cpu.py), which run the SAME assertions through the host build of csrc/mpm2d_math.h.

A `backend` is anything with
    force(type, gp, F, aux) -> out
    plasticity(type, gp, cdg, F, aux) -> (F2, aux2, next force)
    svd2(F) -> (cu, su, S)
on float32 rows (F: [n, 4] row-major)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MATS = ["jelly", "snow", "sand", "water", "linear", "elastic", "von_mises", "visco"]
FP = C.POINTER(C.c_float)


def fptr(a):
    return a.ctypes.data_as(FP)


# ---------------------------------------------------------------------------------------------------- error measures
def cond_classes(cond):
    """rows by the decade of their condition number: 1 (< 3), 10, 1e2, 1e3, 1e4 (and beyond: sand's clamp rows)"""
    dec = np.clip(np.round(np.log10(np.maximum(cond, 1.0))), 0, 4).astype(int)
    return [(10.0 ** d, dec == d) for d in range(5)]


def comparable(g, mat):
    """rows of an ill-conditioned fixture that enter the comparison, and those left out BY CONSTRUCTION:
    det F < 0 for the Hencky models (`use`: the reference takes the log of a negative sigma), and det F < 0 with all |sigma|
    equal — WHICH singular direction carries the sign is arbitrary there, the reference's svd and the device pick different
    ones and both are right; such an F has no well-defined polar decomposition.  Returns (ok, by_construction)."""
    by_construction = ~g[mat + "_use"] | (g["negdet"] & (g["cond"] < 1.5))
    want = [g[mat + "_force"], g[mat + "_F2"], g[mat + "_force2"]]
    finite = np.isfinite(want[0]).all(1) & np.isfinite(want[1]).all(1) & np.isfinite(want[2]).all(1)
    return ~by_construction & finite, by_construction


def errors(g, mat, got):
    """per condition class: max |error| of (force, F2, next force) relative to the largest entry of the row's reference value (at
    least 1 % of the class's largest), after the absolute floor of the F - R cancellation for the stresses (as in
    tests/test_gpu_ref.py::test_device_materials_match_the_reference)"""
    force, F2, aux2, force2 = got
    gp = g[mat + "_gp"]
    atol = 2 * gp[2] * gp[1] * 4e-6 if mat != "water" else 0.0
    use, _ = comparable(g, mat)
    rows = []
    for c, sel in cond_classes(g["cond"]):
        want = [g[mat + "_force"], g[mat + "_F2"], g[mat + "_force2"]]
        ok = sel & use
        if not ok.any():
            rows.append((c, 0, 0.0, 0.0, 0.0))
            continue
        e = []
        for have, w, floor in ((force, want[0], atol), (F2, want[1], 0.0), (force2, want[2], atol)):
            scale = np.abs(w[ok]).max(1, keepdims=True)
            scale = np.maximum(scale, 1e-2 * scale.max())  # (a rotation has no stress at all: such rows are measured against the class)
            with np.errstate(invalid="ignore"):
                err = np.maximum(np.abs(have[ok] - w[ok]) - floor, 0.0) / scale
            err = np.where(np.isfinite(have[ok]), err, np.inf)  # a non-finite output where the reference is finite is an error
            e.append(float(err.max()) if scale.max() > 0 else 0.0)
        rows.append((c, int(ok.sum()), e[0], e[1], e[2]))
    return rows


def print_illcond_table(mat, rows):
    print("\n%-9s  cond    rows   force     F_new     next force   (max error / largest entry of the row)" % mat)
    for c, n, ef, eF, en in rows:
        print("%-9s  %-7g %4d   %.2e  %.2e  %.2e" % (mat, c, n, ef, eF, en))


def assert_illcond_bounds(mat, rows):
    """the per-class bounds of the 3D path (an eps cond(F) method): the tolerances of the well-conditioned fixture up to cond 1e2"""
    for c, n, ef, eF, en in rows:
        if n == 0:
            continue
        if c <= 1e2:
            assert ef <= 3e-5 and eF <= 2e-5 and en <= 3e-5, (mat, c, ef, eF, en)
        elif c <= 1e3:  # the return maps of von Mises / visco divide by the deviator's norm and raise to a power: the error of
            # sigma_min is amplified in their NEXT stress
            assert ef <= 1e-4 and eF <= 4e-4 and en <= (8e-3 if mat in ("von_mises", "visco") else 2e-4), (mat, c, ef, eF, en)
        else:  # cond 1e4: eps cond = 6e-4 of sigma_min is all fp32 can hold of F itself
            assert ef <= 2e-3 and eF <= 5e-3 and en <= (0.15 if mat in ("von_mises", "visco") else 5e-3), (mat, c, ef, eF, en)


# ---------------------------------------------------------------------------------------------------- the 2D checks
def outputs2d(backend, g, mat, prefix=""):
    """(force, F2, aux2, next force) of the backend on a fixture's rows (prefix: "" for ref_illcond2d, mat + "_" for ref_materials2d)"""
    gp, t = np.ascontiguousarray(g[mat + "_gp"], np.float32), int(g[mat + "_type"])
    F, cdg = (np.ascontiguousarray(g[prefix + k], np.float32) for k in ("F", "cdg"))
    aux = np.ascontiguousarray(g[mat + "_aux"], np.float32)
    force = backend.force(t, gp, F, aux)
    F2, aux2, force2 = backend.plasticity(t, gp, cdg, F, aux)
    if mat == "water":
        assert np.array_equal(F2, F)  # water never updates dg_e (src/particles.cpp:469-478)
    return force, F2, aux2, force2


def check_materials2d(backend, mat):
    """force, F2, aux2 and the fused next force against ref_materials2d.npz, two measures, both asserted:
    (a) the one of tests/test_gpu_ref.py::test_device_materials_match_the_reference as it stands there — stress within 3e-5 of the
        FIXTURE's largest entry plus the absolute floor 2 mu vol 4e-6 of the F - R cancellation (none for water), F 2e-5 absolute,
        aux 2e-5 of max(1, largest);
    (b) the stresses per ROW: 3e-5 of the row's own largest reference entry after the floor.  The fixture mixes strains of 0.01
        and 0.2, and (a) alone would let the small ones hide behind the large.  Water has no F - R term, but its pressure
        k (j^-gamma - 1) cancels near j = 1 the same way: j^-gamma is about 1 and good to an ulp or two in fp32 — in the reference as
        on the device — so the row-wise measure gives water the floor vol k 4 eps (two evaluations, 2 ulp each, eps = 2^-23)."""
    g = np.load(os.path.join(GOLDEN, "ref_materials2d.npz"))
    force, F2, aux2, force2 = outputs2d(backend, g, mat, prefix=mat + "_")
    gp = g[mat + "_gp"]
    atol = 2 * gp[2] * gp[1] * 4e-6 if mat != "water" else 0.0
    row_floor = atol if mat != "water" else gp[1] * gp[2] * 4 * 2.0 ** -23
    wf, wF2, wa2, wf2 = (g[mat + k] for k in ("_force", "_F2", "_aux2", "_force2"))
    assert np.isfinite(wf).all() and np.isfinite(wF2).all() and np.isfinite(wa2).all() and np.isfinite(wf2).all()  # no row is left out
    for have in (force, F2, aux2, force2):
        assert np.isfinite(have).all(), mat
    assert np.abs(force - wf).max() <= 3e-5 * np.abs(wf).max() + atol, mat
    assert np.abs(force2 - wf2).max() <= 3e-5 * np.abs(wf2).max() + atol, mat
    ef = (np.maximum(np.abs(force - wf) - row_floor, 0.0) / np.maximum(np.abs(wf).max(1, keepdims=True), 1e-30)).max()
    en = (np.maximum(np.abs(force2 - wf2) - row_floor, 0.0) / np.maximum(np.abs(wf2).max(1, keepdims=True), 1e-30)).max()
    eF = np.abs(F2 - wF2).max()
    ea = np.abs(aux2 - wa2).max() / max(1.0, np.abs(wa2).max())
    print("\n%-9s materials2d: force %.2e  F_new %.2e  aux %.2e  next force %.2e  (%d rows, none left out)" % (mat, ef, eF, ea, en, len(wf)))
    assert ef <= 3e-5 and eF <= 2e-5 and ea <= 2e-5 and en <= 3e-5, (mat, ef, eF, ea, en)


def illcond2d():
    return np.load(os.path.join(GOLDEN, "ref_illcond2d.npz"))


def check_illcond2d(backend, mat):
    """the per-class bounds on ref_illcond2d.npz; at least 90 % of the rows of every (material, condition class) — the two
    exclusions by construction aside — must enter the comparison.  Returns the table."""
    g = illcond2d()
    ok, by_construction = comparable(g, mat)
    left_out = 0
    for c, sel in cond_classes(g["cond"]):
        pool = sel & ~by_construction
        assert pool.sum() > 0 and (ok & pool).sum() >= 0.9 * pool.sum(), (mat, c, int((ok & pool).sum()), int(pool.sum()))
        left_out += int((pool & ~ok).sum())
    rows = errors(g, mat, outputs2d(backend, g, mat))
    print_illcond_table(mat, rows)
    print("%-9s  left out: %d rows by construction (det F < 0: Hencky model, or cond < 1.5), %d for a non-finite reference"
          % (mat, int(by_construction.sum()), left_out))
    assert_illcond_bounds(mat, rows)
    return rows


def check_finite2d(backend, mat):
    """every output is finite wherever the reference's is — cond 1e4 and sand's clamp rows included"""
    g = illcond2d()
    force, F2, aux2, force2 = outputs2d(backend, g, mat)
    for have, key in ((force, "_force"), (F2, "_F2"), (aux2[:, None], "_aux2"), (force2, "_force2")):
        want = g[mat + key].reshape(len(have), -1)
        fin = np.isfinite(want).all(1)
        bad = np.flatnonzero(fin & ~np.isfinite(have).all(1))
        assert len(bad) == 0, (mat, key, bad, g["cond"][bad], g["tag"][bad])


def check_svd2(backend):
    """the rotation and the signed singular values the models consume, against the float64 singular values of the same float32
    matrices (ref_illcond2d.npz: sigma)"""
    g = illcond2d()
    F = np.ascontiguousarray(g["F"], np.float32)
    n = len(F)
    cu, su, S = backend.svd2(F)
    want = g["sigma"]  # descending, the sign of det F on the last
    assert np.isfinite(cu).all() and np.isfinite(su).all() and np.isfinite(S).all()
    assert np.abs(cu.astype(np.float64) ** 2 + su.astype(np.float64) ** 2 - 1.0).max() <= 2e-6
    assert np.array_equal(np.sign(S[:, 0] * S[:, 1]), np.sign(want[:, 1]))
    have = np.sort(np.abs(S.astype(np.float64)), 1)[:, ::-1]
    rel = np.abs(have - np.abs(want)) / np.abs(want)
    # U diag(S^2) U^T = F F^T: holds the rotation also where U itself is not unique (the fallback and the nearly repeated rows)
    c, s, S2 = cu.astype(np.float64), su.astype(np.float64), S.astype(np.float64) ** 2
    A = np.stack([c * c * S2[:, 0] + s * s * S2[:, 1], c * s * (S2[:, 0] - S2[:, 1]), c * s * (S2[:, 0] - S2[:, 1]),
                  s * s * S2[:, 0] + c * c * S2[:, 1]], 1)
    Fm = F.reshape(n, 2, 2).astype(np.float64)
    FFt = (Fm @ Fm.transpose(0, 2, 1)).reshape(n, 4)
    eA = (np.abs(A - FFt).max(1) / np.abs(FFt).max(1)).max()
    print("\ncond     rows   max relative error of sigma_max / sigma_min       (U diag(S^2) U^T - F F^T: %.2e of the largest entry)" % eA)
    for cnd, sel in cond_classes(g["cond"]):
        r = rel[sel].max(0)
        print("%-7g  %4d   %.2e  %.2e" % (cnd, sel.sum(), r[0], r[1]))
    for cnd, sel in cond_classes(g["cond"]):
        assert rel[sel].max() <= 4e-7 * max(cnd, 8.0), (cnd, rel[sel].max(0))  # eps cond(F), against eps cond(F)^2 of sqrt(eig(F F^T))
    assert eA <= 4e-6, eA


# ---------------------------------------------------------------------------------------------------- the host build
HOST_SRC = os.path.join(ROOT, "tests", "cpp", "mpm2d_math_host.cpp")
HOST_HDRS = [os.path.join(ROOT, "taichi_mpm_amd", "csrc", f) for f in ("mpm2d_math.h", "group_params.h")] + [os.path.join(ROOT, "include", "mpmhip.h")]
HOST_OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libmpm2d_math_host.so")


def build_host():
    """csrc/mpm2d_math.h compiled by g++ (tests/cpp/mpm2d_math_host.cpp) -> tests/cpp/_build/libmpm2d_math_host.so"""
    os.makedirs(os.path.dirname(HOST_OUT), exist_ok=True)
    if not os.path.exists(HOST_OUT) or max(os.path.getmtime(p) for p in [HOST_SRC] + HOST_HDRS) > os.path.getmtime(HOST_OUT):
        # -ffp-contract=off: the products and sums as written (the device contracts a * b + c on its own terms; the bounds have
        # room for either)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", HOST_SRC, "-o", HOST_OUT])
    return HOST_OUT


class HostBackend:
    def __init__(self):
        L = C.CDLL(build_host())
        L.mpm2d_host_force.argtypes = [C.c_int32, FP, C.c_int64, FP, FP, FP]
        L.mpm2d_host_plasticity.argtypes = [C.c_int32, FP, C.c_int64, FP, FP, FP, FP]
        L.mpm2d_host_svd2.argtypes = [C.c_int64, FP, FP, FP, FP]
        assert L.mpm2d_host_sizeof_group() == 80
        self.L = L

    def force(self, t, gp, F, aux):
        out = np.zeros_like(F)
        assert self.L.mpm2d_host_force(t, fptr(gp), len(F), fptr(F), fptr(aux), fptr(out)) == 0
        return out

    def plasticity(self, t, gp, cdg, F, aux, fused=True):
        F2, aux2, nf = F.copy(), aux.copy(), np.zeros_like(F)
        assert self.L.mpm2d_host_plasticity(t, fptr(gp), len(F), fptr(cdg), fptr(F2), fptr(aux2), fptr(nf) if fused else None) == 0
        return F2, aux2, nf

    def svd2(self, F):
        n = len(F)
        cu, su, S = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 2), np.float32)
        assert self.L.mpm2d_host_svd2(n, fptr(F), fptr(cu), fptr(su), fptr(S)) == 0
        return cu, su, S
