"""Rigid-body set-up without a GPU: taichi_mpm_amd/csrc/rigid_setup.h (creation of a CPIC body from a mesh and a config, scripted
steps, anchor kinematics, the boundary particles' rows of a .bgeo frame; 3D and 2D) compiled for the host by g++, the header alone
(tests/cpp/rigid_setup_host.cpp).  Creation is held to the reference's own add_rigid_particle output (tests/golden/ref_cpic.npz,
ref_cpic2d.npz) with the tolerances tests/test_gpu_cpic.py uses for the same quantities through the device, small shapes to the live
reference build (oracle.refmpm, CPU) where it completes them, the rows to a numpy model byte for byte.  The same source runs as a
program of its own under AddressSanitizer and UBSan."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from oracle import refmpm
from taichi_mpm_amd import _lib
from tests import cpic_scenes as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rigid_setup_host.cpp")
HDRS = [os.path.join(ROOT, "taichi_mpm_amd", "csrc", h) for h in ("rigid_setup.h", "rigid_records.h")] + [os.path.join(ROOT, "include", "mpmhip.h")]
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "librigid_setup_host.so")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "rigid_setup_host_san")
GOLDEN = os.path.join(ROOT, "tests", "golden")
F = np.float32
fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
needs_reference = pytest.mark.skipif(not refmpm.available(), reason="oracle/_ref (the reference build) is absent")


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(f) for f in [SRC] + HDRS) > os.path.getmtime(out)


def build():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", SRC, "-o", OUT])
    return OUT


_host = None


def host_lib():
    global _host
    if _host is None:
        L = C.CDLL(build())
        assert [L.rs_sizeof(k) for k in range(2)] == [C.sizeof(_lib.RigidConfig), C.sizeof(_lib.RigidConfig2D)]
        for d, cfg in ((3, _lib.RigidConfig), (2, _lib.RigidConfig2D)):
            g = lambda name: getattr(L, "rs%d_%s" % (d, name))  # noqa: E731
            g("new").restype = C.c_void_p
            g("free").argtypes = [C.c_void_p]
            g("add").argtypes = [C.c_void_p, C.POINTER(cfg), C.c_int64, fp, C.c_float, ip, C.c_float]
            g("why").argtypes, g("why").restype = [C.c_void_p], C.c_char_p
            g("next_pid").argtypes = [C.c_void_p, C.c_int32]
            g("samples").argtypes, g("samples").restype = [C.c_void_p, fp, ip], C.c_int64
            g("state").argtypes = g("record").argtypes = [C.c_void_p, C.c_int, fp]
            g("set_motion").argtypes = [C.c_void_p, C.c_int, fp, fp]
            g("mesh").argtypes, g("mesh").restype = [C.c_void_p, C.c_int, C.c_int64, fp], C.c_int64
            g("steps").argtypes = [C.c_void_p, C.c_float, C.c_float, fp]
            g("frame_rows").argtypes = [C.c_void_p, C.c_int, C.c_int64, ip, C.POINTER(C.c_uint8)]
        _host = L
    return _host


def _p(a, t=fp):
    return a.ctypes.data_as(t)


class Refused(Exception):
    pass


class Scene:
    """the bodies of one simulation: what a ctx keeps on the host, and the device records"""

    def __init__(self, dim, res, dx, next_pid=0):
        self.L, self.d, self.dx = host_lib(), dim, float(dx)
        self.res = np.full(dim, res, np.int32)
        self.h = self._f("new")()
        self.keep = []  # the script callbacks live as long as the scene
        self._f("next_pid")(self.h, next_pid)

    def _f(self, name):
        return getattr(self.L, "rs%d_%s" % (self.d, name))

    def __del__(self):
        self._f("free")(self.h)

    def add(self, mesh, t=0.0, **kw):
        """keys as add_particles(type='rigid') takes them; scripts are callables t -> values.  -> body index"""
        d = self.d
        c = (_lib.RigidConfig if d == 3 else _lib.RigidConfig2D)()
        c.codimensional, c.recenter, c.reverse_vertices = int(kw.get("codimensional", True)), int(kw.get("recenter", True)), int(kw.get("reverse_vertices", False))
        c.density = kw.get("density", 0.0)
        c.friction[:] = (kw["friction"],) * 2 if "friction" in kw else (kw.get("friction0", 0.0), kw.get("friction1", 0.0))
        c.scale[:] = kw.get("scale", (1.0,) * d)
        c.initial_position[:] = kw.get("initial_position", (0.0,) * d)
        c.initial_velocity[:] = kw.get("initial_velocity", (0.0,) * d)
        if d == 3:
            c.initial_rotation[:] = kw.get("initial_rotation", (0.0,) * 3)
            c.initial_angular_velocity[:] = kw.get("initial_angular_velocity", (0.0,) * 3)
        else:
            c.initial_rotation, c.initial_angular_velocity = kw.get("initial_rotation", 0.0), kw.get("initial_angular_velocity", 0.0)
        c.linear_damping, c.angular_damping = kw.get("linear_damping", 0.0), kw.get("angular_damping", 0.0)
        for key in ("scripted_position", "scripted_rotation"):
            if kw.get(key) is not None:
                def call(_user, t, out, fn=kw[key]):
                    v = np.atleast_1d(fn(float(t)))
                    for k in range(len(v)):
                        out[k] = float(v[k])
                self.keep.append(_lib.SCRIPT_FN(call))
                setattr(c, key, self.keep[-1])
        el = np.ascontiguousarray(mesh, F).reshape(-1, d * d)
        rid = self._f("add")(self.h, C.byref(c), len(el), _p(el), self.dx, _p(self.res, ip), t)
        if rid < 0:
            raise Refused(self._f("why")(self.h).decode())
        return rid

    def next_pid(self, add=0):
        return self._f("next_pid")(self.h, add)

    def samples(self):
        """every boundary particle: offset, world position and velocity (the header's anchor function), body, element, creation id"""
        d = self.d
        n = self._f("samples")(self.h, None, None)
        f, i = np.zeros((n, 3 * d), F), np.zeros((n, 3), np.int32)
        self._f("samples")(self.h, _p(f), _p(i, ip))
        return dict(off=f[:, :d], pos=f[:, d:2 * d], vel=f[:, 2 * d:], body=i[:, 0], elem=i[:, 1], id=i[:, 2])

    def of(self, rid):
        s = self.samples()
        return {k: v[s["body"] == rid] for k, v in s.items()}

    def state(self, rid):
        o = np.zeros(33 if self.d == 3 else 10, F)
        self._f("state")(self.h, rid, _p(o))
        return o

    def record(self, rid):
        o = np.zeros(17 if self.d == 3 else 5, F)
        self._f("record")(self.h, rid, _p(o))
        return o

    def set_motion(self, rid, v, w):
        self._f("set_motion")(self.h, rid, _p(np.asarray(v, F)), _p(np.atleast_1d(np.asarray(w, F))))

    def mesh(self, rid):
        n = self._f("mesh")(self.h, rid, 0, None)
        o = np.zeros((n, self.d, self.d), F)
        assert self._f("mesh")(self.h, rid, n, _p(o)) == n
        return o

    def steps(self, n_bodies, t, dt):
        o = np.zeros((n_bodies, 16 if self.d == 3 else 8), F)
        self._f("steps")(self.h, t, dt, _p(o))
        return o

    def frame_rows(self, verbose, mat_ids):
        ids = np.ascontiguousarray(mat_ids, np.int32)
        out = np.zeros((len(ids) + len(self.samples()["id"]), 92 if verbose else 48), np.uint8)
        self._f("frame_rows")(self.h, int(verbose), len(ids), _p(ids, ip), _p(out, C.POINTER(C.c_uint8)))
        return out


def scene3(next_pid=0):
    return Scene(3, cs.RES, cs.DX, next_pid)


def scene2(next_pid=0):
    return Scene(2, cs.RES2, cs.DX2, next_pid)


def body_keys(body):
    b = dict(body)
    return b.pop("mesh"), b


def test_the_test_library_does_not_pull_in_the_hip_runtime():
    build()
    needed = subprocess.check_output(["readelf", "-d", OUT], text=True)
    assert "amdhip64" not in needed and "libhsa" not in needed, needed


def test_every_scenario_under_the_sanitizers():
    """the same source as a stand-alone program (its main() runs creation, steps, meshes and frames of fixed 3D and 2D scenes, the
    frames into heap buffers of exactly their size) with -fsanitize=address,undefined; the runtime is linked statically"""
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if _stale(SAN):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", SAN])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "scenarios ok" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------- creation against the goldens
def add_case3(s, body):
    if body == "scripted":
        pos, rot = cs.script_functions()
        return s.add(cs.plate(), codimensional=True, friction=0.4, scripted_position=pos, scripted_rotation=rot)
    mesh, kw = body_keys(cs.BODIES[body])
    return s.add(mesh, **kw)


def add_case2(s, body):
    if body == "scripted":
        q = cs.SCRIPT2
        return s.add(cs.bar2(), codimensional=True, friction=0.4,
                     scripted_position=lambda t: [F(q["p0"][k]) + F(q["vel"][k]) * F(t) for k in range(2)],
                     scripted_rotation=lambda t: F(q["a0"]) + F(q["rate"]) * F(t))
    mesh, kw = body_keys(cs.BODIES2[body])
    return s.add(mesh, **kw)


@pytest.mark.parametrize("case", cs.CASES, ids=[c[0] for c in cs.CASES])
def test_creation_3d_matches_the_reference(case):
    """mass, inertia, initial pose and the boundary particles of MPM::add_rigid_particle (src/mpm_rigid_body.cpp:130-252): the
    tolerances of tests/test_gpu_cpic.py::test_rigid_body_creation_matches_the_reference"""
    name, body = case[0], case[1]
    gold = np.load(os.path.join(GOLDEN, "ref_cpic.npz"))
    s = scene3()
    rid = add_case3(s, body)
    st, a = s.state(rid), gold[name + "_body0"]
    np.testing.assert_allclose(st[:13], a[:13], rtol=0, atol=1e-6)
    assert abs(st[13] - a[13]) <= 1e-5 * a[13]
    np.testing.assert_allclose(st[15:24].reshape(3, 3), gold[name + "_inertia"], rtol=1e-5, atol=1e-7 * np.abs(gold[name + "_inertia"]).max())
    p = s.of(rid)
    assert len(p["pos"]) == len(gold[name + "_samples"]) > 50
    np.testing.assert_allclose(p["pos"], gold[name + "_samples"], rtol=0, atol=2e-7)
    assert (p["id"] == np.arange(len(p["id"]))).all() and s.next_pid() == len(p["id"])  # nothing near the wall: consecutive ids


@pytest.mark.parametrize("case", cs.CASES2, ids=[c[0] for c in cs.CASES2])
def test_creation_2d_matches_the_reference(case):
    """the tolerances in the first lines of tests/test_gpu_cpic.py::test_2d_colored_distance_field_and_colours_match_the_reference"""
    name, body = case[0], case[1]
    gold2 = np.load(os.path.join(GOLDEN, "ref_cpic2d.npz"))
    s = scene2()
    rid = add_case2(s, body)
    st0 = s.state(rid)
    np.testing.assert_allclose(st0[:6], gold2[name + "_body0"][:6], rtol=0, atol=1e-6)
    np.testing.assert_allclose(st0[6:], gold2[name + "_body0"][6:], rtol=1e-5)
    p = s.of(rid)
    assert len(p["pos"]) == len(gold2[name + "_samples"]) >= 10
    np.testing.assert_allclose(p["pos"], gold2[name + "_samples"], rtol=0, atol=2e-7)


# ---------------------------------------------------------------------------------------------- small shapes
DX = cs.DX
POSE = dict(codimensional=True, density=40.0, initial_position=(0.503, 0.497, 0.501), initial_rotation=(20.0, 0.0, 10.0))
TRI_SHORT = np.array([[[0, 0, 0], [0.4 * DX, 0, 0], [0, 0, 2.3 * DX]]], F)               # an edge shorter than dx / 2
TRI_MULTIPLE = np.array([[[0, 0, 0], [3 * DX - 1e-6, 0, 0], [0, 3 * DX + 1e-6, 0]]], F)  # just under / over a multiple of dx
OFF_CENTRE_BOX = cs.box() + F((0.03, -0.02, 0.01))
SMALL3 = {
    "short_edge": (TRI_SHORT, POSE),
    "edges_about_3dx": (TRI_MULTIPLE, POSE),
    "near_the_wall": (cs.plate(), dict(POSE, initial_position=(0.3, 0.497, 0.75))),
    "box_outward": (OFF_CENTRE_BOX, dict(POSE, codimensional=False, density=400.0)),
    "box_inward": (OFF_CENTRE_BOX[:, ::-1], dict(POSE, codimensional=False, density=400.0)),
    "reverse_vertices": (cs.plate(), dict(POSE, reverse_vertices=True)),
    "scale_with_a_zero": (cs.plate(), dict(POSE, scale=(0.5, 0.0, 1.5))),
}


@needs_reference
@pytest.mark.parametrize("name", list(SMALL3))
def test_small_shapes_3d_match_the_live_reference(name):
    """the reference build creates the same body: state and inertia as in the creation test; the boundary particles one by one, in
    the same order — body-frame offsets and world positions to 2e-7 (the creation test's bound)"""
    mesh, kw = SMALL3[name]
    ref = refmpm.Sim(cs.RES, cs.DX, cs.DT, gravity=(0, -10, 0))
    rr = ref.add_rigid(mesh, **kw)
    a, pr = ref.rigid_state(rr), ref.rigid_samples(rr)
    s = scene3()
    rid = s.add(mesh, **kw)
    st, p = s.state(rid), s.of(rid)
    np.testing.assert_allclose(st[:13], cs.rigid_vector(a)[:13], rtol=0, atol=1e-6)
    assert abs(st[13] - a["mass"]) <= 1e-5 * a["mass"] and a["mass"] > 0
    np.testing.assert_allclose(st[15:24].reshape(3, 3), a["inertia"], rtol=1e-5, atol=1e-7 * np.abs(a["inertia"]).max())
    assert len(p["pos"]) == len(pr["pos"]) > 0
    np.testing.assert_allclose(p["off"], pr["offset"], rtol=0, atol=2e-7)
    np.testing.assert_allclose(p["pos"], pr["pos"], rtol=0, atol=2e-7)


def _rotate(q, v):
    w, x, y, z = [float(c) for c in q]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return np.asarray(v, np.float64) @ R.T


def test_short_and_near_multiple_edges_sample_counts():
    """the loop's own rule, written out: along an edge of length l the lattice starts at min(l / 3, dx / 2) and runs while < l + dx.
    Edge 0.4 dx: 0.133 dx, 1.133 dx -> 2 columns; 2.3 dx: 0.5, 1.5, 2.5 -> 3 rows; kept where x / xl + y / yl <= 1 - 1e-6 (the last
    column sits at _x - dx / 2 = 0.633 dx > xl: dropped): (0.133, 0.5), (0.133, 1.5) dx.  Edges xl = 3 dx (1 - e), yl = 3 dx (1 + e) with e = 1e-6 / (3 dx) = 1.07e-5: 0.5 .. 3.5 dx, four
    each; the fourth is pulled back to 3 dx, beyond the hypotenuse.  Of the 3 x 3 rest x + y < 3 dx keeps (0.5, 0.5), (0.5, 1.5),
    (1.5, 0.5) dx, and on x + y = 3 dx the two edges decide: (0.5, 2.5) gives 1 - 2 e / 3 = 1 - 7e-6: kept; (2.5, 0.5) gives
    1 + 2 e / 3 and (1.5, 1.5) gives 1 + O(e^2) > 1 - 1e-6: dropped.  In the loop's order (x outer): four samples."""
    s = scene3()
    kw = dict(codimensional=True, recenter=False, initial_position=(0.5, 0.5, 0.5), scripted_position=lambda t: (0.5, 0.5, 0.5),
              scripted_rotation=lambda t: (0.0, 0.0, 0.0))
    a = s.of(s.add(TRI_SHORT, **kw))["off"] / DX
    np.testing.assert_allclose(a, [(0.4 / 3, 0, 0.5), (0.4 / 3, 0, 1.5)], rtol=0, atol=1e-5)
    b = s.of(s.add(TRI_MULTIPLE, **kw))["off"] / DX
    np.testing.assert_allclose(b, [(0.5, 0.5, 0), (0.5, 1.5, 0), (0.5, 2.5, 0), (1.5, 0.5, 0)], rtol=0, atol=1e-5)


def test_a_triangle_without_area_gets_no_samples_and_still_counts_as_an_element():
    good0, good1 = cs.plate()[0], cs.plate()[1]
    flat = np.array([good0[0], good0[0], good0[2]], F)  # two vertices coincide: an edge of length 0
    s = scene3()
    p = s.of(s.add(np.stack([good0, flat, good1]), **POSE))
    assert set(p["elem"]) == {0, 2} and (np.diff(p["elem"]) >= 0).all()
    alone = scene3()
    q = alone.of(alone.add(np.stack([good0, good1]), **POSE))
    assert len(p["off"]) == len(q["off"]) and (p["elem"] == 2 * q["elem"]).all()
    np.testing.assert_array_equal(p["off"], q["off"])  # (it has no mass either: the centre of mass does not move)
    assert s.mesh(1).shape == (3, 3, 3)


def test_a_2d_segment_shorter_than_dx_gets_two_samples():
    """max(ceil(length / dx), 2) at the mid points of equal parts: 1/4 and 3/4 of the segment"""
    seg = np.array([[[0.0, 0.0], [0.6 * cs.DX2, 0.0]]], F)
    kw = dict(codimensional=True, density=40.0, initial_position=(0.503, 0.497), initial_rotation=20.0)
    s = scene2()
    p = s.of(s.add(seg, **kw))
    np.testing.assert_allclose(p["off"], [(-0.15 * cs.DX2, 0), (0.15 * cs.DX2, 0)], rtol=0, atol=1e-8)
    assert list(p["id"]) == [0, 1] and s.next_pid() == 2
    if refmpm.available():
        ref = refmpm.Sim(cs.RES2, cs.DX2, cs.DT, dim=2, gravity=(0, -10))
        rr = ref.add_rigid2(seg, **kw)
        np.testing.assert_allclose(p["pos"], ref.rigid_samples2(rr), rtol=0, atol=2e-7)
        np.testing.assert_allclose(s.state(1)[:6], ref.rigid_state2(rr)[:6], rtol=0, atol=1e-6)
        np.testing.assert_allclose(s.state(1)[6:], ref.rigid_state2(rr)[6:], rtol=1e-5)


@pytest.mark.parametrize("dim", [3, 2])
def test_samples_within_7_cells_of_the_wall_are_absent_and_still_take_ids(dim):
    """the same body in the middle of the domain (nothing dropped: consecutive ids) and reaching towards the wall: the kept samples
    are those of the first whose world position is 7 cells or more inside, each with the id its place in the full sequence gives it;
    the counter advances by the full count, so the material particles added afterwards are numbered behind every one of them"""
    if dim == 3:
        mesh, res, dx = cs.plate(), cs.RES, cs.DX
        kw, shift = dict(codimensional=True, initial_rotation=(20.0, 0.0, 10.0)), np.array((0.3, 0.5, 0.75), F)
        mid = (0.5, 0.5, 0.5)
    else:
        mesh, res, dx = cs.bar2(), cs.RES2, cs.DX2
        kw, shift, mid = dict(codimensional=True, initial_rotation=20.0), np.array((0.2, 0.88), F), (0.5, 0.5)
    s = Scene(dim, res, dx, next_pid=5)  # (five material particles came first)
    full = s.of(s.add(mesh, initial_position=mid, **kw))
    n = len(full["id"])
    assert list(full["id"]) == list(range(5, 5 + n)) and s.next_pid() == 5 + n
    s.next_pid(3)  # three more material particles
    cut = s.of(s.add(mesh, initial_position=tuple(shift), **kw))
    g = cut["pos"] / F(dx)
    assert ((g >= 7) & (g - res <= -7)).all() and 0 < len(cut["id"]) < n
    where = np.array([np.flatnonzero((full["off"] == o).all(axis=1))[0] for o in cut["off"]])
    assert (np.diff(where) > 0).all() and where[-1] > len(where) - 1  # in order, with gaps
    assert list(cut["id"]) == list(5 + n + 3 + where)
    moved = (full["pos"] - np.asarray(mid, F) + shift) / F(dx)
    inside = ((moved >= 7 + 1e-3) & (moved - res <= -7 - 1e-3)).all(axis=1)
    outside = ((moved < 7 - 1e-3) | (moved - res > -7 + 1e-3)).any(axis=1)
    assert set(np.flatnonzero(inside)) <= set(where) and not set(np.flatnonzero(outside)) & set(where)
    assert s.next_pid() == 5 + n + 3 + n


def test_an_inward_facing_box_has_the_mass_inertia_and_centre_of_the_outward_one():
    kw = dict(POSE, codimensional=False, density=400.0)
    s = scene3()
    out, inw = s.add(OFF_CENTRE_BOX, **kw), s.add(OFF_CENTRE_BOX[:, ::-1], **kw)
    a, b = s.state(out), s.state(inw)
    assert a[13] > 0 and b[13] > 0
    np.testing.assert_allclose(b[13:], a[13:], rtol=1e-6, atol=1e-6 * np.abs(a[15:24]).max())  # mass, inverse, inertia, inverse
    np.testing.assert_allclose(s.mesh(inw)[:, ::-1], s.mesh(out), rtol=0, atol=1e-7)               # recentred by the same centre
    np.testing.assert_allclose(s.mesh(out).reshape(-1, 3).mean(axis=0), POSE["initial_position"], rtol=0, atol=1e-6)


def test_reverse_vertices_and_a_scale_with_a_zero_component():
    """reverse_vertices swaps the first two vertices of every element; a scale component of 0 means 1"""
    ident = dict(codimensional=True, initial_position=(0.5, 0.5, 0.5))
    s = scene3()
    a, b = s.add(cs.plate(), **ident), s.add(cs.plate(), reverse_vertices=True, **ident)
    np.testing.assert_array_equal(s.mesh(b), s.mesh(a)[:, [1, 0, 2]])
    c, d = s.add(cs.plate(), scale=(0.5, 0.0, 1.5), **ident), s.add(cs.plate(), scale=(0.5, 1.0, 1.5), **ident)
    np.testing.assert_array_equal(s.mesh(c), s.mesh(d))
    np.testing.assert_allclose(s.mesh(c) - F(0.5), s.mesh(a) * F((0.5, 1.0, 1.5)) - F(0.5) * F((0.5, 1.0, 1.5)), rtol=0, atol=1e-7)
    s2 = scene2()
    e, f = s2.add(cs.box2(), initial_position=(0.5, 0.5)), s2.add(cs.box2(), initial_position=(0.5, 0.5), reverse_vertices=True, scale=(0.0, 2.0))
    np.testing.assert_allclose(s2.mesh(f) - F(0.5), (s2.mesh(e)[:, ::-1] - F(0.5)) * F((1.0, 2.0)), rtol=0, atol=1e-7)


def test_refusals_by_their_texts():
    s, s2 = scene3(), scene2()
    pos, rot = cs.script_functions()
    flat = np.array([[[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0]]], F)
    for kw in (dict(scripted_position=pos), dict(scripted_rotation=rot), dict()):
        with pytest.raises(Refused, match=r"^recenter = 0 needs a scripted position and rotation \(src/mpm_rigid_body.cpp:186-190\)$"):
            s.add(cs.plate(), recenter=False, **kw)
        with pytest.raises(Refused, match=r"^recenter = 0 needs a scripted position and rotation$"):
            s2.add(cs.bar2(), recenter=False, **{k: (lambda t: 0.0) if "rot" in k else (lambda t: (0.5, 0.5)) for k in kw})
    s.add(cs.plate(), recenter=False, scripted_position=pos, scripted_rotation=rot)
    for mesh, kw in ((flat, dict(codimensional=True)),           # a shell without area: no mass
                     (cs.plate(), dict(codimensional=False)),    # a flat "solid": no volume
                     (flat[:, [0, 1, 1]], dict(codimensional=True))):
        with pytest.raises(Refused, match=r"^rigid body: the mesh has no mass or a singular inertia tensor$"):
            s.add(mesh, **kw)
    with pytest.raises(Refused, match=r"^rigid body: the mesh has no mass or a singular inertia tensor$"):
        s.add(np.array([[[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0]], [[0.2, 0, 0], [0.3, 0, 0], [0, 0, 0]]], F), codimensional=True)
    with pytest.raises(Refused, match=r"^rigid body without mass$"):
        s2.add(np.array([[[0.1, 0.1], [0.1, 0.1]]], F))
    assert len(s.samples()["id"]) == len(s.of(1)["id"]) and s.mesh(1).shape == (2, 3, 3)  # a refusal leaves the store as it was


# ---------------------------------------------------------------------------------------------- scripts
def euler_quaternion64(deg, order=(0, 1, 2)):
    """X * Y * Z in float64 (src/mpm_rigid_body.cpp:108-114), or the three axis rotations multiplied in another order"""
    def mul(a, b):
        return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])
    q = [np.zeros(4) for _ in range(3)]
    for k in range(3):
        h = np.deg2rad(np.float64(deg[k])) / 2
        q[k][0], q[k][1 + k] = np.cos(h), np.sin(h)
    return mul(mul(q[order[0]], q[order[1]]), q[order[2]])


def test_scripted_steps_evaluate_the_scripts_at_t_and_t_plus_dt():
    """3D: position and Euler angles (degrees, X * Y * Z) at exactly t and t + dt in float; the quaternion against a float64 model
    (5e-7: unit quaternions, a dozen float operations) and, at t = 0, against the reference's scripted_plate_jelly body"""
    seen = []
    pos, rot = cs.script_functions()
    s = scene3()
    s.add(cs.plate(), **POSE)  # a free body: no script, no step
    s.add(cs.plate(), codimensional=True, friction=0.4, scripted_position=lambda t: (seen.append(("p", t)), pos(t))[1],
          scripted_rotation=lambda t: (seen.append(("r", t)), rot(t))[1])
    assert seen == [("p", 0.0), ("r", 0.0)]  # creation: the pose at the current time
    gold = np.load(os.path.join(GOLDEN, "ref_cpic.npz"))["scripted_plate_jelly_body0"]
    np.testing.assert_allclose(s.state(2)[3:7], gold[3:7], rtol=0, atol=1e-6)
    np.testing.assert_allclose(s.state(2)[3:7], euler_quaternion64(cs.SCRIPT["e0"]), rtol=0, atol=5e-7)
    rec = s.record(2)
    np.testing.assert_allclose(rec[:9].reshape(3, 3), _rotate(s.state(2)[3:7], np.eye(3)).T, rtol=0, atol=5e-7)
    assert rec[16] == 3 and s.state(2)[14] == 0 and not s.state(2)[24:33].any() and not s.state(2)[7:13].any()
    del seen[:]
    t, dt = F(0.0123), F(1e-4)
    st = s.steps(2, t, dt)
    assert seen == [("p", float(t)), ("p", float(F(t + dt))), ("r", float(t)), ("r", float(F(t + dt)))]
    assert not st[0].any() and list(st[1, :2]) == [1, 1]
    np.testing.assert_array_equal(st[1, 2:5], np.asarray(pos(t), F))
    np.testing.assert_array_equal(st[1, 5:8], np.asarray(pos(F(t + dt)), F))
    np.testing.assert_allclose(st[1, 8:12], euler_quaternion64(rot(t)), rtol=0, atol=5e-7)
    np.testing.assert_allclose(st[1, 12:16], euler_quaternion64(rot(F(t + dt))), rtol=0, atol=5e-7)
    # the order is X * Y * Z: the other five products of these three rotations are further away than the bound
    for order in itertools.permutations(range(3)):
        if order != (0, 1, 2):
            assert np.abs(euler_quaternion64(rot(t), order) - st[1, 8:12]).max() > 1e-4


def test_scripted_steps_2d_hold_radians():
    seen = []
    s = scene2()
    s.add(cs.bar2(), codimensional=True, scripted_position=lambda t: (seen.append(t), (0.5 + 0.25 * t, 0.5))[1], scripted_rotation=lambda t: 10.0 + 180.0 * t)
    assert s.state(1)[2] == F(10.0) * F(np.pi / 180.0) and s.record(1)[4] == 3 and s.state(1)[7] == 0 and s.state(1)[9] == 0
    t, dt = F(0.25), F(0.125)
    st = s.steps(1, t, dt)[0]
    assert seen == [0.0, 0.25, 0.375] and list(st[:2]) == [1, 1]
    np.testing.assert_array_equal(st[2:6], F((0.5625, 0.5, 0.59375, 0.5)))
    np.testing.assert_array_equal(st[6:8], F((55.0, 77.5)) * F(np.pi / 180.0))
    only_rot = scene2()
    only_rot.add(cs.bar2(), codimensional=True, initial_position=(0.5, 0.5), scripted_rotation=lambda t: 90.0)
    assert list(only_rot.steps(1, t, dt)[0, :2]) == [0, 1] and only_rot.record(1)[4] == 2 and only_rot.state(1)[7] > 0


# ---------------------------------------------------------------------------------------------- frame rows
def model_rows(s, verbose):
    """the boundary particles' rows in numpy, float by float in the order the row writer takes: x y z 1 | type 1 | id | limits 1 1 1 |
    v; big-endian; zeros behind (verbose)"""
    p, d = s.samples(), s.d
    rows = np.zeros((len(p["id"]), 23 if verbose else 12), ">u4")
    for j in range(len(rows)):
        b, off = int(p["body"][j]), p["off"][j]
        if d == 3:
            R, st = s.record(b)[:9], s.state(b)
            ro = [F(F(F(R[3 * r] * off[0]) + F(R[3 * r + 1] * off[1])) + F(R[3 * r + 2] * off[2])) for r in range(3)]
            x = [F(ro[r] + st[r]) for r in range(3)]
            v, w = st[7:10], st[10:13]
            vel = [F(v[0] + F(F(w[1] * ro[2]) - F(w[2] * ro[1]))), F(v[1] + F(F(w[2] * ro[0]) - F(w[0] * ro[2]))), F(v[2] + F(F(w[0] * ro[1]) - F(w[1] * ro[0])))]
        else:
            st = s.state(b)
            c, sn = F(np.cos(np.float64(st[2]))), F(np.sin(np.float64(st[2])))
            ro = [F(F(c * off[0]) - F(sn * off[1])), F(F(sn * off[0]) + F(c * off[1]))]
            x = [F(ro[0] + st[0]), F(ro[1] + st[1]), F(0)]
            vel = [F(st[3] - F(st[5] * ro[1])), F(st[4] + F(st[5] * ro[0])), F(0)]
        rows[j, 0:4] = np.array(x + [F(1)], F).view(np.uint32)
        rows[j, 4], rows[j, 5], rows[j, 6:9] = 1, p["id"][j], 1
        rows[j, 9:12] = np.array(vel, F).view(np.uint32)
    return rows.view(np.uint8).reshape(len(rows), -1)


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("verbose", [0, 1])
def test_boundary_rows_byte_for_byte_and_their_merge_with_material_rows(dim, verbose):
    """48 / 92 bytes per row.  The material rows are markers (0xAB, the id's low byte in front).  Ids interleaved (a body added
    between two particle groups), every boundary particle first, and no material particle at all"""
    s = scene3(next_pid=4) if dim == 3 else scene2(next_pid=4)
    if dim == 3:
        s.add(cs.plate(), **dict(POSE, initial_position=(0.3, 0.497, 0.75)))  # (some samples dropped: gaps in the ids)
        s.add(*body_keys(cs.BODIES["box"])[:1], **body_keys(cs.BODIES["box"])[1])
        s.set_motion(1, (0.3, -0.5, 0.1), (0.4, 2.0, -1.0))
    else:
        s.add(cs.bar2(), codimensional=True, initial_position=(0.2, 0.88), initial_rotation=20.0)
        s.add(cs.box2(), **body_keys(cs.BODIES2["box"])[1])
        s.set_motion(1, (0.3, -0.5), 2.5)
    bnd, want = s.samples()["id"], model_rows(s, verbose)
    assert want.shape[1] == (92 if verbose else 48) and (np.diff(bnd) > 0).all() and bnd[0] >= 4 and np.diff(bnd).max() > 1
    last = s.next_pid()
    for mat in ([0, 1, 2, 3, last, last + 1, last + 5], [last, last + 1], []):
        got = s.frame_rows(verbose, mat)
        is_mat = (got[:, 1:] == 0xAB).all(axis=1)
        assert is_mat.sum() == len(mat)
        order = sorted([(i, 0) for i in mat] + [(int(i), 1) for i in bnd])  # ascending creation id
        assert [kind == 0 for _, kind in order] == list(is_mat)
        assert list(np.ascontiguousarray(got[~is_mat][:, 20:24]).view(">u4")[:, 0]) == list(bnd)
        np.testing.assert_array_equal(got[~is_mat], want)
        assert list(got[is_mat][:, 0]) == [m % 256 for m in mat]
