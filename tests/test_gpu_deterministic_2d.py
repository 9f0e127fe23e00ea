"""The deterministic mode of the 2D solver (include/mpmhip.h: mpmhip2d_config.deterministic; csrc/k_mpm2d_det.h).

The default 2D substep scatters with global float atomics (grid terms, body impulses), so its last bits depend on arrival order.
In the mode a substep is a function of the particle set (state + creation id) and the bodies: cell sort with every cell in ascending
(creation id, slot), one staged record per particle, a gather P2G that writes every node once, impulse rows added in a fixed order.
What must then hold BIT FOR BIT (np.array_equal on every particle field sorted by id, on get_grid(), and with bodies on every body's
state and the colour words): two runs; a shuffled upload with the same creation ids (mpmhip2d_upload_ids); all eight materials;
crowded cells and particles dying in mid-run; the mode switched on in mid-run and snapshot round trips; five CPIC scenes.  Against the
reference's fixtures the mode keeps the tolerances of the default path's tests, and one substep of the mode agrees with the default
path to the project's P2G tolerances.  The new kernels have no tuning knob (tile and chunk sizes are compile-time constants), so there
is no launch-shape case."""
import os

import numpy as np
import pytest

from tests import cpic_scenes as cs
from tests.common import rel_l2
from tests.test_gpu_mpm2d import MATS, _cases, _levelset

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
PFIELDS = ("id", "x", "v", "F", "B", "aux")


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def _build(tm, res, groups, cfg=None, levelset=None, bodies=(), joints=(), seed=None, deterministic=True, room=0):
    """a 2D scene; `seed`: every group is added in a seeded random permutation and upload_ids gives the particles the ids the
    straight order would have given them.  groups: dicts for add_particles with positions / velocities / F / B / aux arrays."""
    n = sum(len(g["positions"]) for g in groups)
    sim = tm.create_simulation2("mpm").initialize(dict(res=(res, res), delta_x=1.0 / res, base_delta_t=1e-4, max_particles=n + room + 64,
                                                       deterministic=deterministic, **(cfg or {})))
    if levelset is not None:
        sim.set_levelset(levelset)
    rids = [int(sim.add_particles(dict(type="rigid", **b))) for b in bodies]
    for j in joints:
        assert sim.general_action(dict(action="add_articulation", **j)) == ""
    rng = np.random.default_rng(seed) if seed is not None else None
    order = []
    for g in groups:
        k = len(g["positions"])
        o = rng.permutation(k) if rng is not None else np.arange(k)
        order.append(o + sum(len(q) for q in order))
        sim.add_particles({key: (val[o] if key in ("positions", "velocities", "F", "B", "aux") else val) for key, val in g.items()})
    if groups:
        order = np.concatenate(order)
        ids = sim.get_particles(sort_by_id=False)["id"]
        assert len(ids) == n and np.array_equal(ids, ids[0] + np.arange(n))  # nothing was filtered: slots carry sequential ids
        if rng is not None:
            sim.upload_ids(ids[0] + order)
    return sim, rids


def _state(sim, rids=()):
    p = sim.get_particles()
    out = {f: p[f] for f in PFIELDS}
    out["grid"] = sim.get_grid()
    if rids:
        o = np.argsort(sim.get_particles(sort_by_id=False)["id"], kind="stable")
        out["states"] = sim.download_colours()["states"][o]
        for r in rids:
            out["body%d" % r] = sim.get_rigid_state(r)
    return out


def _run(tm, steps, *a, **kw):
    sim, rids = _build(tm, *a, **kw)
    sim.run_substeps(steps)
    out = _state(sim, rids)
    sim.close()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape, (k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()))


def _sand_on_floor(tm, res=256, lo=(78, 40), cells=100, seed=9):
    """the scene of test_mpm2d_against_the_live_reference_at_scale"""
    from tests.golden.make_golden import mpm2d_state
    x, v, F, B = mpm2d_state(res, lo=lo, cells=cells, seed=seed)
    vol = (1.0 / res) ** 2 / 4
    gp, _ = tm.group_params("sand", 400.0 * vol, vol)
    ls = tm.mpm.LevelSet(friction=0.5).add_plane((0, 1, 0), d=-0.12)
    return res, [dict(type="sand", positions=x, velocities=v, F=F, B=B, params=gp)], ls


def test_two_runs_and_a_shuffled_upload_agree_bit_for_bit(tm):
    """checks 1 and 2: 256^2, 40 000 sand particles on a friction floor, 200 substeps"""
    res, groups, ls = _sand_on_floor(tm)
    a = _run(tm, 200, res, groups, levelset=ls)
    assert len(a["id"]) == 40000 and np.isfinite(a["F"]).all() and a["grid"][..., 2].max() > 0
    _same(a, _run(tm, 200, res, groups, levelset=ls))
    _same(a, _run(tm, 200, res, groups, levelset=ls, seed=21))


@pytest.mark.parametrize("mat", MATS)
def test_every_material_straight_against_shuffled(tm, mat):
    """check 3"""
    from tests.golden.make_golden import mpm2d_state
    res = 64
    x, v, F, B = mpm2d_state(res)
    vol = (1.0 / res) ** 2 / 4
    gp, _ = tm.group_params(mat, 400.0 * vol, vol)
    groups = [dict(type=mat, positions=x, velocities=v, F=F, B=B, params=gp)]
    ls = tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.37)
    a = _run(tm, 20, res, groups, levelset=ls)
    assert len(a["id"]) == len(x) and np.isfinite(a["x"]).all()
    _same(a, _run(tm, 20, res, groups, levelset=ls, seed=5))


def test_crowded_cells_and_particles_dying_in_mid_run(tm):
    """check 4: one cell with 300 particles, and a jet that leaves through clean_boundary"""
    from tests.golden.make_golden import mpm2d_state
    res = 64
    dx = 1.0 / res
    rng = np.random.default_rng(17)
    x, v, F, B = mpm2d_state(res, lo=(20, 25), cells=16, seed=8)
    crowd = ((np.array([28.5, 30.5]) + rng.uniform(0.05, 0.95, (300, 2))) * dx).astype(np.float32)  # base node (28, 30)
    jet = ((np.array([50.0, 28.0]) + rng.uniform(0.0, 1.0, (200, 2)) * np.array([4.0, 6.0])) * dx).astype(np.float32)
    x = np.concatenate([x, crowd, jet])
    v = np.concatenate([v, 0.3 * rng.normal(size=(300, 2)), np.tile([40.0, 0.0], (200, 1)) + rng.normal(size=(200, 2))]).astype(np.float32)
    eye = np.tile(np.float32([1, 0, 0, 1]), (500, 1))
    F, B = np.concatenate([F, eye]), np.concatenate([B, np.zeros((500, 4), np.float32)])
    cell = np.floor(x / dx - 0.5).astype(np.int64)
    assert np.unique(cell[:, 0] * 1000 + cell[:, 1], return_counts=True)[1].max() >= 200
    vol = dx * dx / 4
    gp, _ = tm.group_params("jelly", 400.0 * vol, vol)
    groups = [dict(type="jelly", positions=x, velocities=v, F=F, B=B, params=gp)]
    ls = tm.mpm.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.3)
    a = _run(tm, 60, res, groups, levelset=ls)
    assert len(x) - 200 <= len(a["id"]) < len(x) - 50 and np.isfinite(a["x"]).all() and np.isfinite(a["F"]).all()  # the jet died in mid-run
    b = _run(tm, 60, res, groups, levelset=ls, seed=33)
    assert len(a["id"]) == len(b["id"])
    _same(a, b)


def test_switched_on_in_mid_run_and_snapshot_round_trips(tm, tmp_path):
    """check 5: default path for 10 substeps, snapshot, mode on, 15 substeps == a fresh deterministic ctx that loads the blob and runs
    15; and a snapshot taken inside the deterministic run, loaded into a fresh ctx, continues with the same bits"""
    res, groups, ls = _sand_on_floor(tm, res=64, lo=(20, 25), cells=20, seed=4)
    ls = tm.mpm.LevelSet(friction=0.5).add_plane((0, 1, 0), d=-0.37)
    a, _ = _build(tm, res, groups, levelset=ls, deterministic=False)
    a.run_substeps(10)
    p0, p1 = str(tmp_path / "s0.bin"), str(tmp_path / "s1.bin")
    a.save_snapshot(p0)
    a.set_deterministic(True)
    a.run_substeps(15)
    mid = _state(a)
    a.save_snapshot(p1)
    a.run_substeps(10)
    end = _state(a)
    room = len(groups[0]["positions"])
    b, _ = _build(tm, res, [], levelset=ls, room=room)  # the scene without particles: they come out of the blob
    b.load_snapshot(p0)
    b.run_substeps(15)
    _same(mid, _state(b))
    c, _ = _build(tm, res, [], levelset=ls, room=room)
    c.load_snapshot(p1)
    c.run_substeps(10)
    _same(end, _state(c))
    for s in (a, b, c):
        s.close()


def _cpic_scene(tm, name):
    """(groups, cfg, levelset, bodies, joints, substeps): the device halves of the 2D CPIC tests of tests/test_gpu_cpic.py"""
    from oracle import oracle as orc
    f32 = np.float32
    for case, body, material, _, cfg in cs.CASES2:
        if case == name:
            x, v = cs.block2()
            if body == "scripted":
                s = cs.SCRIPT2
                bd = dict(mesh=cs.bar2(), codimensional=True, friction=0.4,
                          scripted_position=lambda t: [f32(s["p0"][k]) + f32(s["vel"][k]) * f32(t) for k in range(2)],
                          scripted_rotation=lambda t: f32(s["a0"]) + f32(s["rate"]) * f32(t))
            else:
                bd = dict(cs.BODIES2[body])
            gp = orc.group_params(material, cs.MASS2, cs.VOL2)[0]
            return [dict(type=material, positions=x, velocities=v, params=gp)], dict(gravity=(0, -10), **cfg), None, [bd], [], 40
    if name == "rotation_joint":  # test_2d_rotation_joint_matches_the_live_reference
        x, v = cs.block2()
        bodies = [dict(mesh=cs.box2(0.07, 0.04), codimensional=False, density=400.0, friction=0.3, initial_position=(0.44, 0.50),
                       initial_rotation=25.0, initial_velocity=(0.2, -0.3), initial_angular_velocity=3.0),
                  dict(mesh=cs.bar2(0.09), codimensional=True, density=60.0, friction=0.3, initial_position=(0.585, 0.56),
                       initial_rotation=-40.0, initial_velocity=(-0.1, -0.2), initial_angular_velocity=-1.0)]
        gp = orc.group_params("jelly", cs.MASS2, cs.VOL2)[0]
        return ([dict(type="jelly", positions=x, velocities=v, params=gp)], dict(gravity=(0, -10), penalty=1e3), None, bodies,
                [dict(type="rotation", obj0=1, obj1=2)], 40)
    assert name == "box_on_floor"  # test_2d_rigid_body_levelset_collision_matches_the_live_reference (friction 0.4, restitution 0.5)
    x, v = cs.block2(lo=24, hi=30)
    x = x + np.float32([0.0, 0.22])
    gp = orc.group_params("jelly", cs.MASS2, cs.VOL2)[0]
    body = dict(mesh=cs.box2(), codimensional=False, density=300.0, friction=0.4, restitution=0.5, initial_position=(0.5, 0.385),
                initial_rotation=17.0, initial_velocity=(0.6, -1.5), initial_angular_velocity=2.5)
    ls = tm.mpm.LevelSet(friction=0.3).add_plane((0, 1, 0), d=-0.3).add_plane((-1, 0, 0), d=0.605)
    return ([dict(type="jelly", positions=x, velocities=v, params=gp)], dict(gravity=(0, -10), rigid_body_levelset_collision=True), ls,
            [body], [], 300)


@pytest.mark.parametrize("name", [c[0] for c in cs.CASES2] + ["rotation_joint", "box_on_floor"])
def test_cpic_scenes_twice_and_shuffled(tm, name):
    """check 6: body state and colour words included"""
    groups, cfg, ls, bodies, joints, steps = _cpic_scene(tm, name)
    kw = dict(cfg=cfg, levelset=ls, bodies=bodies, joints=joints)
    a = _run(tm, steps, cs.RES2, groups, **kw)
    assert np.isfinite(a["x"]).all() and all(np.isfinite(a[k]).all() for k in a if k.startswith("body"))
    if name != "box_on_floor":
        assert (a["states"] != 0).any()  # particles on both sides of a body: the colour test and the impulses are in the run
    else:
        assert a["body1"][4] > -1.5  # the contact is inside the run: the box (thrown at -1.5, falling) was stopped / thrown back
    _same(a, _run(tm, steps, cs.RES2, groups, **kw))
    _same(a, _run(tm, steps, cs.RES2, groups, seed=77, **kw))


def _grid_close(a, b):
    """the project's P2G tolerances (a reordered fp32 sum of a node's ~36 terms differs by ~1.2e-7 rel-L2)"""
    m = rel_l2(a[..., 2], b[..., 2])
    v = rel_l2(a[..., :2], b[..., :2])
    print("grid m rel-L2 %.3e  v rel-L2 %.3e" % (m, v))
    assert m <= 1e-6 and v <= 1e-5, (m, v)


def test_duplicate_ids_give_a_valid_run(tm):
    """check 8: two particles of one cell with the same id — the tie is broken by slot, so the index is still a permutation"""
    res, groups, ls = _sand_on_floor(tm, res=64, lo=(20, 25), cells=20, seed=4)
    ls = tm.mpm.LevelSet(friction=0.5).add_plane((0, 1, 0), d=-0.37)
    x = groups[0]["positions"]
    cell = np.floor(x * res - 0.5).astype(np.int64)
    key = cell[:, 0] * 1000 + cell[:, 1]
    keys, first, counts = np.unique(key, return_index=True, return_counts=True)
    j = int(first[np.argmax(counts >= 2)])  # a particle whose cell holds another one
    i = int(np.flatnonzero(key == key[j])[1])
    det, _ = _build(tm, res, groups, levelset=ls)
    ids = det.get_particles(sort_by_id=False)["id"].copy()
    ids[i] = ids[j]
    det.upload_ids(ids)
    dflt, _ = _build(tm, res, groups, levelset=ls, deterministic=False)
    det.substep(); dflt.substep()
    _grid_close(det.get_grid(), dflt.get_grid())
    p, q = det.get_particles(sort_by_id=False), dflt.get_particles(sort_by_id=False)  # by slot: the ids no longer name a particle
    assert len(p["x"]) == len(q["x"]) == len(x)
    assert rel_l2(p["v"], q["v"]) <= 1e-5 and np.abs(p["x"] - q["x"]).max() <= 1e-7
    det.run_substeps(20)
    p = det.get_particles(sort_by_id=False)
    assert len(p["x"]) == len(x) and np.isfinite(p["x"]).all() and (p["id"] == ids[j]).sum() == 2
    det.close(); dflt.close()


@pytest.mark.parametrize("case,mat", _cases()[2])
def test_the_mode_matches_the_reference_fixture(tm, case, mat):
    """check 9: test_mpm2d_matches_the_reference_fixture with deterministic=True; tolerances copied from tests/test_gpu_mpm2d.py:62-68"""
    g, cases, _ = _cases()
    c = cases[case]
    res, dx, dt = int(g["res"]), float(g["dx"]), float(g["dt"])
    sim = tm.create_simulation2("mpm").initialize(dict(res=(res, res), delta_x=dx, base_delta_t=dt, deterministic=True, **c["cfg"]))
    if c.get("shapes1"):
        sim.set_levelset(tm.mpm.DynamicLevelSet().initialize(0.0, c["t1"], _levelset(tm, c["shapes"], c["friction"]),
                                                             _levelset(tm, c["shapes1"], c["friction"])))
    else:
        sim.set_levelset(_levelset(tm, c["shapes"], c["friction"]))
    aux0 = {"snow": 1.0, "water": 1.0, "visco": 1000.0}.get(mat, 0.0)
    sim.add_particles(dict(type=mat, positions=g["x"], velocities=g["v"], F=g["F"], B=g["B"], aux=np.full(len(g["x"]), aux0, np.float32),
                           params=g["gp_" + mat]))
    for _ in range(3):
        sim.substep()
    got = sim.get_particles()
    want = g["%s_%s" % (case, mat)]
    assert np.array_equal(got["id"], g["%s_%s_ids" % (case, mat)])
    assert np.abs(got["x"] - want[:, 0:2]).max() <= 5e-7
    assert rel_l2(got["v"], want[:, 2:4]) <= 5e-5
    if mat != "water":
        assert rel_l2(got["F"], want[:, 4:8]) <= 1e-4
    assert rel_l2(got["B"], want[:, 8:12]) <= 2e-4
    assert np.abs(got["aux"] - want[:, 12]).max() <= 5e-5 * max(1.0, np.abs(want[:, 12]).max())
    sim.close()


@pytest.mark.parametrize("case", cs.CASES2, ids=[c[0] for c in cs.CASES2])
def test_the_mode_with_a_rigid_body_matches_the_reference_fixture(tm, case):
    """check 9: test_2d_substeps_with_a_rigid_body_match_the_reference with deterministic=True; tolerances copied from
    tests/test_gpu_cpic.py:291-300"""
    gold2 = np.load(os.path.join(HERE, "golden", "ref_cpic2d.npz"))
    name, body, material, n, cfg = case
    sim, rid = cs.build_device2(tm, body, material, deterministic=True, **cfg)
    sim.run_substeps(n)
    h = sim.get_particles(sort_by_id=True)
    assert len(h["x"]) == len(gold2[name + "_x"])
    assert np.abs(h["x"] - gold2[name + "_x"]).max() <= 5e-6
    assert rel_l2(h["v"], gold2[name + "_v"]) <= 2e-4
    assert rel_l2(h["F"], gold2[name + "_F"]) <= 1e-4
    o = np.argsort(sim.get_particles(sort_by_id=False)["id"], kind="stable")
    assert (sim.download_colours()["states"][o] != gold2[name + "_states"]).sum() <= 3
    a, b = gold2[name + "_body"], sim.get_rigid_state(rid)
    np.testing.assert_allclose(b[0:3], a[0:3], rtol=0, atol=2e-6)
    np.testing.assert_allclose(b[3:5], a[3:5], rtol=0, atol=2e-4 * max(np.abs(a[3:5]).max(), 1e-2))
    np.testing.assert_allclose(b[5], a[5], rtol=0, atol=2e-4 * max(abs(a[5]), 1e-1))
    sim.close()


def test_one_substep_of_the_mode_against_the_default_path(tm):
    """check 10: the scene of checks 1 and 2"""
    res, groups, ls = _sand_on_floor(tm)
    det, _ = _build(tm, res, groups, levelset=ls)
    dflt, _ = _build(tm, res, groups, levelset=ls, deterministic=False)
    det.substep(); dflt.substep()
    _grid_close(det.get_grid(), dflt.get_grid())
    det.close(); dflt.close()
