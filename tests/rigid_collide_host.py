"""Host build of the rigid-rigid collision arithmetic (taichi_mpm_amd/csrc/k_rigid_collide.h through tests/cpp/rigid_collide_host.cpp)
for tests/test_rigid_collide_cpu.py and tests/test_gpu_rigid_collide.py: the loader, the ctypes mirrors and the fixture."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rigid_collide_host.cpp")
HDRS = [os.path.join(ROOT, "taichi_mpm_amd", "csrc", h) for h in ("k_rigid_collide.h", "k_joints.h")]
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "librigid_collide_host.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "rigid_mpr.npz")
F = np.float32
fp = C.POINTER(C.c_float)


class JointBody(C.Structure):
    """mirror of mpm::JointBody (k_joints.h)"""
    _fields_ = [("pos", C.c_float * 3), ("vel", C.c_float * 3), ("omega", C.c_float * 3), ("R", C.c_float * 9),
                ("inv_mass", C.c_float), ("inv_I", C.c_float * 9), ("Iw", C.c_float * 9)]


class RigidCollision(C.Structure):
    """mirror of mpm::RigidCollision"""
    _fields_ = [("hit", C.c_int), ("i", C.c_int), ("j", C.c_int), ("calls", C.c_int), ("depth", C.c_float), ("dir", C.c_float * 3),
                ("pos", C.c_float * 3)]


class RigidImpulse(C.Structure):
    """mirror of mpm::RigidImpulse"""
    _fields_ = [("J", C.c_float), ("j", C.c_float), ("normal_i", C.c_float * 3), ("normal_j", C.c_float * 3),
                ("friction_i", C.c_float * 3), ("friction_j", C.c_float * 3)]


_lib = None


def build():
    """compile the host library when it is older than its sources.  -ffp-contract=off: the header's arithmetic is a pure function
    of its inputs only if nothing is fused (k_rigid_collide.h)"""
    if not os.path.exists(OUT) or any(os.path.getmtime(OUT) < os.path.getmtime(f) for f in [SRC] + HDRS):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", OUT])
    return OUT


def load():
    global _lib
    if _lib is not None:
        return _lib
    L = C.CDLL(build())
    assert L.rc_sizeof_body() == C.sizeof(JointBody) and L.rc_sizeof_collision() == C.sizeof(RigidCollision)
    assert L.rc_sizeof_impulse() == C.sizeof(RigidImpulse)
    lp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_int)
    L.rc_mpr.argtypes = [C.c_int, fp, lp, fp, fp, fp]
    L.rc_loop_bounds.argtypes = [ip]
    L.rc_resolve.argtypes = [C.c_int, C.POINTER(JointBody), fp, fp, C.c_int, C.POINTER(RigidCollision), C.c_int, C.c_int, C.c_float,
                             C.c_float, C.POINTER(RigidImpulse)]
    L.rc_rigidify.argtypes = [C.c_int, C.POINTER(JointBody), ip, fp, lp, fp, fp, C.c_int, C.c_int, C.c_float, C.c_float,
                              C.POINTER(RigidCollision)]
    _lib = L
    return L


def fixture():
    return np.load(FIXTURE)


def fixture_expected(g):
    """the fixture's results in the layout of rc_mpr / mpmhip_rigid_mpr_test: hit, depth, dir[3], pos[3], support calls"""
    return np.concatenate([(g["ret"] == 0).astype(F)[:, None], g["depth"][:, None], g["dir"], g["pos"], g["calls"].astype(F)[:, None]],
                          axis=1).astype(F)


def same_bits(a, b):
    """bit for bit.  A NaN counts as equal to a NaN: which NaN an invalid operation returns (0 * inf: the sign and payload of
    the default NaN) is a property of the processor, not of the arithmetic — x86 returns 0xFFC00000, the GPU 0x7FC00000"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def host_mpr(g):
    """rc_mpr on the whole fixture -> (rows [n, 9], pairs whose loop bound expired)"""
    L = load()
    n = len(g["ret"])
    out = np.zeros((n, 9), F)
    v, o = np.ascontiguousarray(g["verts"], F), np.ascontiguousarray(g["offsets"], np.int64)
    r, c = np.ascontiguousarray(g["rot"], F), np.ascontiguousarray(g["ctr"], F)
    expired = L.rc_mpr(n, v.ctypes.data_as(fp), o.ctypes.data_as(C.POINTER(C.c_int64)), r.ctypes.data_as(fp), c.ctypes.data_as(fp),
                       out.ctypes.data_as(fp))
    return out, expired


def make_bodies(states):
    """states: per body (body 0 = background first) a dict pos, vel, omega, R (3x3), inv_mass, inv_I (3x3, body frame)"""
    arr = (JointBody * len(states))()
    for b, s in zip(arr, states):
        b.pos[:] = [float(x) for x in s["pos"]]
        b.vel[:] = [float(x) for x in s["vel"]]
        b.omega[:] = [float(x) for x in s["omega"]]
        b.R[:] = [float(x) for x in np.asarray(s["R"], F).reshape(9)]
        b.inv_mass = float(s["inv_mass"])
        b.inv_I[:] = [float(x) for x in np.asarray(s["inv_I"], F).reshape(9)]
    return arr


def host_rigidify(states, scripted, hulls, fric, rest, iterations=5, position_iterations=True, penalty=1e3, dt=1e-4):
    """MPM::rigidify by the host build.  hulls: per body its body-frame vertices [n, 3] (None for the background).
    -> (collision rows [n, 9] as mpmhip_rigid_get_collisions gives them, vel [nb, 3], omega [nb, 3])"""
    L = load()
    nb = len(states)
    bodies = make_bodies(states)
    off = np.zeros(nb + 1, np.int64)
    for b in range(nb):
        off[b + 1] = off[b] + (0 if hulls[b] is None else len(hulls[b]))
    hv = np.ascontiguousarray(np.concatenate([np.asarray(h, F).reshape(-1, 3) for h in hulls if h is not None]), F)
    sc = np.ascontiguousarray(scripted, np.int32)
    fr, rs = np.ascontiguousarray(fric, F), np.ascontiguousarray(rest, F)
    cols = (RigidCollision * max(1, (nb - 1) * (nb - 2) // 2))()
    n = L.rc_rigidify(nb, bodies, sc.ctypes.data_as(C.POINTER(C.c_int)), hv.ctypes.data_as(fp), off.ctypes.data_as(C.POINTER(C.c_int64)),
                      fr.ctypes.data_as(fp), rs.ctypes.data_as(fp), int(iterations), int(position_iterations), float(penalty), float(dt), cols)
    rows = np.array([[c.i, c.j, c.depth] + list(c.dir) + list(c.pos) for c in cols[:n]], F).reshape(n, 9)
    vel = np.array([list(b.vel) for b in bodies], F)
    omega = np.array([list(b.omega) for b in bodies], F)
    return rows, vel, omega
