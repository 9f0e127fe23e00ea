"""Rigid-rigid collisions (MPM::rigidify, src/mpm_rigid_body.cpp:306-345) without a GPU: the arithmetic the device runs
(taichi_mpm_amd/csrc/k_rigid_collide.h) compiled for the host by g++ (tests/cpp/rigid_collide_host.cpp).

  detection   against libccd's own single-precision answers (tests/golden/rigid_mpr.npz, recorded by
              tests/golden/make_rigid_mpr.py from the reference's external/libccd): every pair, bit for bit
  resolution  against a float64 numpy restatement of Collision::project_velocity / project_position
              (src/rigid_body_solver.h:39-87) and the loops of rigidify (src/mpm_rigid_body.cpp:325-344), written below
tests/test_gpu_rigid_collide.py holds the device to the same host build."""
import ctypes as C

import numpy as np
import pytest

from tests import rigid_collide_host as rh

F = np.float32

# Largest deviation of the fp32 host build's vel / omega from the float64 restatement over CASES, relative to the largest velocity
# change of the case (linear and angular changes together, as they are numbers of one scale here: lengths of order 1).
# Measured with g++ -O2 -ffp-contract=off on x86-64: 1.92e-7 (case "restitution_0"); no tolerance can be derived for a
# sequential impulse chain, so the assertion stands at 8 x the measured value: room for another compiler's scheduling of the
# float operations, none for a wrong formula (those are off by orders of magnitude — a missing restitution term alone is 0.3).
RESOLVE_MEASURED = 1.92e-7
RESOLVE_BOUND = 8 * RESOLVE_MEASURED


# ---------------------------------------------------------------------------------------------------------------- detection
@pytest.fixture(scope="module")
def golden():
    return rh.fixture()


@pytest.fixture(scope="module")
def host_rows(golden):
    return rh.host_mpr(golden)


def test_detection_reproduces_libccd_bit_for_bit(golden, host_rows):
    """every pair of the fixture: the same return value, depth, dir, pos (bits) and the same number of support calls"""
    got, expired = host_rows
    want = rh.fixture_expected(golden)
    assert expired == 0
    assert len(got) == len(golden["ret"]) == len(golden["cls"]) >= 80  # no pair left out
    same = rh.same_bits(got, want)
    bad = np.nonzero(~same.all(axis=1))[0]
    assert len(bad) == 0, [(int(k), str(golden["cls"][k]), got[k].tolist(), want[k].tolist()) for k in bad[:5]]
    assert np.array_equal(got[:, 8].astype(np.int32), golden["calls"])
    assert np.array_equal(got[:, 0] == 1, golden["ret"] == 0)


def test_loop_bounds_are_four_times_the_largest_recorded_count(golden):
    bounds = (C.c_int * 3)()
    rh.load().rc_loop_bounds(bounds)
    worst = int(golden["calls"].max())
    assert worst == int(golden["max_support_calls"]) and worst >= 10
    assert all(b >= 4 * worst for b in bounds), (list(bounds), worst)


def test_fixture_covers_every_class(golden):
    """the generator's input pairs cover what the issue lists: vertex counts at the wave's edges and beyond a workgroup round,
    tied axis-aligned boxes from apart to deep, a hull inside another with equal centres, both early exits of portal discovery"""
    cls, off, ret, calls = golden["cls"], golden["offsets"], golden["ret"], golden["calls"]
    counts = np.diff(off)
    for n in (8, 63, 64, 65, 200, 257):
        assert (counts == n).any(), n
    assert (counts >= 1400).any()
    a, b = counts[0::2], counts[1::2]
    assert (np.abs(a - b) > 1000).any()  # two bodies of very different sizes
    for name in ("aligned_boxes_separated", "aligned_boxes_barely_separated", "aligned_boxes_shallow", "aligned_boxes_deep",
                 "inside_equal_centres", "touch_exit", "segment_exit", "clouds_separated", "clouds_overlapping", "different_sizes"):
        assert (cls == name).any(), name
    assert (ret[cls == "aligned_boxes_separated"] == -1).all() and (ret[cls == "aligned_boxes_barely_separated"] == -1).all()
    assert (ret[cls == "aligned_boxes_shallow"] == 0).all() and (ret[cls == "aligned_boxes_deep"] == 0).all()
    assert (golden["depth"][cls == "aligned_boxes_shallow"] < 2e-3).all() and (golden["depth"][cls == "aligned_boxes_deep"] > 0.1).all()
    # equal centres
    ctr = golden["ctr"]
    for k in np.nonzero(cls == "inside_equal_centres")[0]:
        assert np.array_equal(ctr[2 * k], ctr[2 * k + 1]) and ret[k] == 0
    # the exits of portal discovery: a hit after ONE support call; touch: depth 0 and no direction, segment: a depth
    t, s = cls == "touch_exit", cls == "segment_exit"
    assert (ret[t] == 0).all() and (calls[t] == 1).all() and (golden["depth"][t] == 0).all() and not golden["dir"][t].any()
    assert (ret[s] == 0).all() and (calls[s] == 1).all() and (golden["depth"][s] > 0).all()
    # aligned boxes: the support mapping ties (several vertices share the largest value) — the first index has to win
    k = int(np.nonzero(cls == "aligned_boxes_deep")[0][0])
    v = golden["verts"][off[2 * k]:off[2 * k + 1]]
    assert (v[:, 0] == v[:, 0].max()).sum() >= 4


# --------------------------------------------------------------------------------------------------------------- resolution
def rot(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def body(pos, vel=(0, 0, 0), omega=(0, 0, 0), R=None, mass=1.0, inertia=(0.4, 0.4, 0.4), scripted=False):
    return dict(pos=np.array(pos, float), vel=np.array(vel, float), omega=np.array(omega, float), R=np.eye(3) if R is None else R,
                inv_mass=0.0 if scripted else 1.0 / mass, inv_I=np.zeros((3, 3)) if scripted else np.diag(1.0 / np.asarray(inertia, float)))


BACKGROUND = dict(pos=np.zeros(3), vel=np.zeros(3), omega=np.zeros(3), R=np.eye(3), inv_mass=0.0, inv_I=np.zeros((3, 3)))


def collision(i, j, depth, normal, pos):
    n = np.asarray(normal, float)
    return dict(i=i, j=j, depth=depth, n=n / np.linalg.norm(n), p=np.asarray(pos, float))


# name -> (bodies 1.., friction per body, restitution per body, collisions, settings)
CASES = {
    "head_on": ([body((1.9, 0, 0), vel=(-1, 0, 0)), body((0, 0, 0), vel=(1, 0, 0))], (0, 0), (0, 0),
                [collision(2, 1, 0.1, (1, 0, 0), (0.95, 0, 0))], {}),
    "glancing_with_friction": ([body((1.8, 0.4, 0), vel=(-1, 0.3, 0.2), omega=(0.5, -1.0, 2.0)), body((0, 0, 0), vel=(1, -0.5, 0), omega=(0, 0, -1.5))],
                               (0.5, 0.8), (0, 0), [collision(2, 1, 0.05, (1, 0.2, 0), (0.9, 0.25, 0.1))], {}),
    "restitution_0": ([body((1.9, 0.1, 0), vel=(-2, 0, 0), mass=2.0, inertia=(0.8, 0.9, 1.0)), body((0, 0, 0), vel=(0.5, 0, 0))], (0.3, 0.3), (0, 0),
                      [collision(2, 1, 0.1, (1, 0, 0), (0.95, 0.05, 0))], {}),
    "restitution_half": ([body((1.9, 0.1, 0), vel=(-2, 0, 0), mass=2.0, inertia=(0.8, 0.9, 1.0)), body((0, 0, 0), vel=(0.5, 0, 0))], (0.3, 0.3),
                         (0.5, 0.5), [collision(2, 1, 0.1, (1, 0, 0), (0.95, 0.05, 0))], {}),
    "one_scripted": ([body((0, -1, 0), scripted=True), body((0.1, 0, 0.05), vel=(0.2, -1.5, 0), omega=(0.3, 0, 0.4), mass=0.5, inertia=(0.1, 0.2, 0.15))],
                     (0.4, 0.4), (0.2, 0.2), [collision(2, 1, 0.02, (0, -1, 0), (0.1, -0.5, 0.05))], {}),
    "position_iterations_off": ([body((1.9, 0, 0), vel=(-1, 0.1, 0)), body((0, 0, 0), vel=(1, 0, 0.1), omega=(0, 1, 0))], (0.2, 0.2), (0.1, 0.1),
                                [collision(2, 1, 0.1, (1, 0, 0), (0.95, 0, 0))], dict(position_iterations=False)),
    "separating": ([body((1.9, 0, 0), vel=(1, 0, 0)), body((0, 0, 0), vel=(-1, 0, 0))], (0.5, 0.5), (0.5, 0.5),
                   [collision(2, 1, 0.1, (1, 0, 0), (0.95, 0, 0))], dict(position_iterations=False)),
    "three_bodies_rotated": ([body((0, 0, 0), vel=(0.3, 0, 0), R=rot((1, 2, 3), 25), inertia=(0.2, 0.5, 0.9)),
                              body((1.7, 0.2, 0), vel=(-0.6, 0, 0.1), omega=(0, 0.4, 0), R=rot((0, 1, 1), -40), mass=1.5, inertia=(0.6, 0.3, 0.7)),
                              body((3.3, 0, 0.2), vel=(-1.2, 0.2, 0), R=rot((1, 0, 0), 70), mass=0.7, inertia=(0.3, 0.3, 0.5))],
                             (0.5, 0.3, 0.6), (0.3, 0.1, 0.4),
                             [collision(2, 1, 0.08, (-1, 0.1, 0), (0.85, 0.1, 0)), collision(3, 2, 0.05, (-1, 0, 0.05), (2.5, 0.1, 0.1))], {}),
}


def reference_f64(bodies, fric, rest, cols, iterations=5, position_iterations=True, penalty=1e3, dt=1e-4):
    """rigid_body_solver.h:39-87 and mpm_rigid_body.cpp:325-344 in float64.  bodies[0] is the background."""
    B = [dict(b, vel=b["vel"].copy(), omega=b["omega"].copy(), Iw=b["R"] @ b["inv_I"] @ b["R"].T) for b in bodies]

    def vel_at(b, p):
        return b["vel"] + np.cross(b["omega"], p - b["pos"])

    def contribution(b, r, n):
        return b["inv_mass"] + np.dot(np.cross(b["Iw"] @ np.cross(r, n), r), n)

    def apply(b, imp, p):
        b["vel"] = b["vel"] + imp * b["inv_mass"]
        b["omega"] = b["omega"] + b["Iw"] @ np.cross(p - b["pos"], imp)

    def project_velocity(c):
        o0, o1, n, p = B[c["i"]], B[c["j"]], c["n"], c["p"]
        friction = np.sqrt(fric[c["i"]] * fric[c["j"]])
        restitution = np.sqrt(rest[c["i"]] * rest[c["j"]])
        v10 = vel_at(o1, p) - vel_at(o0, p)
        r0, r1 = p - o0["pos"], p - o1["pos"]
        v0 = -np.dot(n, v10)
        J = ((1 + restitution) * v0) / (contribution(o0, r0, n) + contribution(o1, r1, n))
        if J < 0:
            return
        apply(o0, -J * n, p)
        apply(o1, J * n, p)
        v10 = vel_at(o1, p) - vel_at(o0, p)
        tao = v10 - n * np.dot(n, v10)
        if np.abs(tao).max() > 1e-7:
            tao = tao / np.linalg.norm(tao)
            j = -np.dot(v10, tao) / (contribution(o0, r0, tao) + contribution(o1, r1, tao))
            j = max(min(j, friction * J), -friction * J)
            apply(o0, -j * tao, p)
            apply(o1, j * tao, p)

    def project_position(c):
        o0, o1, n, p = B[c["i"]], B[c["j"]], c["n"], c["p"]
        r0, r1 = p - o0["pos"], p - o1["pos"]
        J = penalty * dt * c["depth"] / (contribution(o0, r0, n) + contribution(o1, r1, n))
        if J < 0:
            return
        apply(o0, -J * n, p)
        apply(o1, J * n, p)

    for _ in range(iterations):
        if position_iterations:
            for c in cols:
                project_position(c)
        for c in cols:
            project_velocity(c)
    for _ in range(iterations):
        for c in cols:
            project_velocity(c)
    return np.array([b["vel"] for b in B]), np.array([b["omega"] for b in B])


def run_host(bodies, fric, rest, cols, iterations=5, position_iterations=True, penalty=1e3, dt=1e-4):
    """the fp32 host build on the same case (inputs rounded to fp32 once: the float64 reference starts from the rounded values too)
    -> vel, omega, the impulse log"""
    L = rh.load()
    arr = rh.make_bodies(bodies)
    cc = (rh.RigidCollision * len(cols))()
    for d, c in zip(cc, cols):
        d.hit, d.i, d.j, d.calls, d.depth = 1, c["i"], c["j"], 0, float(c["depth"])
        d.dir[:] = [float(x) for x in c["n"]]
        d.pos[:] = [float(x) for x in c["p"]]
    fr, rs = np.ascontiguousarray(fric, F), np.ascontiguousarray(rest, F)
    log = (rh.RigidImpulse * (3 * iterations * max(len(cols), 1)))()
    n = L.rc_resolve(len(bodies), arr, fr.ctypes.data_as(rh.fp), rs.ctypes.data_as(rh.fp), len(cols), cc, iterations, int(position_iterations),
                     float(penalty), float(dt), log)
    return (np.array([list(b.vel) for b in arr], F), np.array([list(b.omega) for b in arr], F), log[:n])


def as_f32_inputs(case):
    """the case with every input rounded to fp32 (what both sides then compute with)"""
    bodies, fric, rest, cols, kw = case
    r32 = lambda a: np.asarray(a, F).astype(float)
    bodies = [BACKGROUND] + [dict(b, pos=r32(b["pos"]), vel=r32(b["vel"]), omega=r32(b["omega"]), R=r32(b["R"]), inv_I=r32(b["inv_I"]),
                                  inv_mass=float(F(b["inv_mass"]))) for b in bodies]
    fric = [0.0] + [float(F(f)) for f in fric]
    rest = [0.0] + [float(F(r)) for r in rest]
    cols = [dict(c, depth=float(F(c["depth"])), n=r32(c["n"]), p=r32(c["p"])) for c in cols]
    return bodies, fric, rest, cols, kw


def deviation(case):
    bodies, fric, rest, cols, kw = as_f32_inputs(case)
    v64, w64 = reference_f64(bodies, fric, rest, cols, **kw)
    v32, w32, _ = run_host(bodies, fric, rest, cols, **kw)
    v0 = np.array([b["vel"] for b in bodies])
    w0 = np.array([b["omega"] for b in bodies])
    change = max(np.abs(v64 - v0).max(), np.abs(w64 - w0).max())
    err = max(np.abs(v32 - v64).max(), np.abs(w32 - w64).max())
    return err, change


@pytest.mark.parametrize("name", sorted(CASES))
def test_resolution_matches_the_float64_restatement(name):
    err, change = deviation(CASES[name])
    if name == "separating":
        assert change == 0.0 and err == 0.0  # no impulse at all
        return
    assert change > 0.05  # the case does collide
    print("%s: deviation %.3g relative to the largest velocity change %.3g -> %.3g" % (name, err, change, err / change))
    assert err / change <= RESOLVE_BOUND, (err, change, err / change)


def test_measured_deviation_is_the_recorded_one():
    """RESOLVE_MEASURED is the figure DESIGN.md quotes: the largest relative deviation over the cases, not a guess"""
    worst = max(e / c for e, c in (deviation(CASES[n]) for n in CASES if n != "separating"))
    print("largest relative deviation over the cases: %.3g" % worst)
    assert worst <= RESOLVE_BOUND


def test_a_negative_impulse_changes_nothing():
    bodies, fric, rest, cols, kw = as_f32_inputs(CASES["separating"])
    v, w, log = run_host(bodies, fric, rest, cols, **kw)
    assert np.array_equal(v, np.array([b["vel"] for b in bodies], F)) and np.array_equal(w, np.array([b["omega"] for b in bodies], F))
    assert len(log) == 10 and all(e.J == 0.0 and e.j == 0.0 and not any(e.normal_i) and not any(e.normal_j) for e in log)


@pytest.mark.parametrize("name", ["glancing_with_friction", "one_scripted", "three_bodies_rotated", "restitution_half"])
def test_impulses_are_equal_and_opposite_and_friction_stays_in_its_cone(name):
    bodies, fric, rest, cols, kw = as_f32_inputs(CASES[name])
    _, _, log = run_host(bodies, fric, rest, cols, **kw)
    iterations, nc = 5, len(cols)
    assert len(log) == 3 * iterations * nc
    applied = friction_seen = 0
    for k, e in enumerate(log):
        ni, nj, fi, fj = (np.array(list(x), F) for x in (e.normal_i, e.normal_j, e.friction_i, e.friction_j))
        for on_i, on_j in ((ni, nj), (fi, fj)):  # exactly opposite, bit for bit (a projection that returned early logs zeros)
            if on_i.any() or on_j.any():
                assert np.array_equal(on_i.view(np.uint32) ^ np.uint32(0x80000000), on_j.view(np.uint32))
        assert e.J >= 0.0
        # which projection this is: rounds of [positions, velocities] first, then velocities alone
        first_half = k < 2 * iterations * nc
        c = cols[k % nc]
        is_velocity = (not first_half) or (k // nc) % 2 == 1
        if is_velocity:
            mu = np.sqrt(F(fric[c["i"]]) * F(fric[c["j"]]), dtype=F)
            assert abs(F(e.j)) <= mu * F(e.J)  # exact: the clamp compares against this very product
            friction_seen += int(e.j != 0.0)
        else:
            assert e.j == 0.0 and not fi.any()
        applied += int(e.J > 0.0)
    assert applied > 0 and friction_seen > 0


# --------------------------------------------------------------------------------------------------------------- the layers
def test_the_config_keys_reach_the_simulation_and_2d_refuses():
    import taichi_mpm_amd as tm
    from taichi_mpm_amd.mpm import MPMError
    sim = tm.mpm.Simulation3D.__new__(tm.mpm.Simulation3D)
    sim._L = None
    tm.mpm.Simulation3D.initialize(sim, dict(res=(32,) * 3, rigid_body_collision=True, rigid_body_iterations=3, rigid_penalty=50.0,
                                             rigid_body_position_iterations=False))
    assert (sim.rigid_body_collision, sim.rigid_body_iterations, sim.rigid_penalty, sim.rigid_body_position_iterations) == (True, 3, 50.0, False)
    tm.mpm.Simulation3D.initialize(sim, dict(res=(32,) * 3))
    assert (sim.rigid_body_collision, sim.rigid_body_iterations, sim.rigid_penalty, sim.rigid_body_position_iterations) == (False, 5, 1e3, True)
    with pytest.raises(MPMError, match="rigid_body_iterations"):
        tm.mpm.Simulation3D.initialize(sim, dict(res=(32,) * 3, rigid_body_iterations=-1))
    # the scene-script driver and the `taichi` alias package hand every keyword through to initialize()
    import os
    import sys
    sys.path.insert(0, os.path.join(rh.ROOT, "compat"))
    try:
        import taichi as tc
        m = tc.dynamics.MPM(res=(32, 32, 32), rigid_body_collision=True, rigid_body_iterations=2, rigid_penalty=7.0)
        assert (m.c.rigid_body_collision, m.c.rigid_body_iterations, m.c.rigid_penalty, m.c.rigid_body_position_iterations) == (True, 2, 7.0, True)
    finally:
        sys.path.remove(os.path.join(rh.ROOT, "compat"))
    s2 = tm.mpm2d.Simulation2D.__new__(tm.mpm2d.Simulation2D)
    with pytest.raises(MPMError, match="rigid_body_collision"):
        tm.mpm2d.Simulation2D.initialize(s2, dict(res=(32, 32), rigid_body_collision=True))
