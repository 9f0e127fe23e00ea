"""The deterministic mode on CPIC scenes and in calculate_energy (include/mpmhip.h: mpmhip_config.deterministic).

The impulses and torques the colour-aware transfers hand to a rigid body used to meet in float atomics, and calculate_energy summed
with double atomics (kinetic) and in slot order (potential).  In the deterministic mode every flagged block writes its per-body sums
into its own row and one launch adds the rows in the Morton order of the blocks (k_rigid.h: MAT_DET, k_rigid_rows_apply); the energy is
formed from partial sums stored per node block / per wave over the sorted particles and added in a fixed order (k_grid.h: MODE 5,
k_particles.h).
What must then hold, BIT FOR BIT, on a CPIC scene: two runs; one stream against two (MPMHIP_RIGID_CONCURRENT); few workgroups
against many (MPMHIP_RIGID_WGS); the two sort forms (MPMHIP_SORT_V1); physical reorders; a shuffled upload with the same creation ids;
and the mode switched on in mid-run.  For the energy: repeated calls, a shuffled upload, the sort forms, reorders, both G2P walks and
both grid walks."""
import os

import numpy as np
import pytest

from tests import cpic_scenes as cs
from tests.common import lattice_cube, make_state, rel_l2
from tests.test_gpu_cpic import paddle
from tests.test_gpu_deterministic import _det_sim

pytestmark = pytest.mark.gpu
PFIELDS = ("id", "x", "v", "F", "B", "aux", "states")
RFIELDS = ("position", "rotation", "velocity", "angular_velocity", "mass", "inv_mass", "inertia", "inv_inertia")


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


class _env:
    """environment switches of the library, read when a ctx is created"""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------ the two CPIC scenes
def _wheel_scene(sim, res):
    """test_gpu_cpic.test_one_stream_and_two_streams_give_the_same_run: a scripted paddle wheel, a free box, >= 100 k sand particles"""
    wheel = int(sim.add_particles(dict(type="rigid", mesh=paddle(0.2, 0.15), codimensional=True, friction=-2,
                                       scripted_position=lambda t: (0.5, 0.5, 0.5), scripted_rotation=lambda t: (0.0, 0.0, 720.0 * t))))
    free = int(sim.add_particles(dict(type="rigid", mesh=cs.box() * 0.5, codimensional=False, friction=0.3, density=40.0,
                                      initial_position=(0.5, 0.72, 0.5))))
    return [wheel, free], free


def _wheel_particles(res):
    return lattice_cube(res, 20, 44, 1.0 / res, jitter=0.15, seed=5), "sand"


def _joint_scene(sim, res):
    """examples/water_wheel.py at a reduced size: spokes and buckets, two bodies on a fixed axle (scripted position, spin about z
    free), tied by a `rotation` joint; water around the right-hand spoke turns them"""
    from examples.water_wheel import buckets, spokes
    axle = dict(type="rigid", codimensional=True, density=40, friction=0.2, rotation_axis=(0, 0, 1), angular_damping=3,
                scripted_position=lambda t: (0.5, 0.5, 0.5))
    a = int(sim.add_particles(dict(mesh=spokes(), **axle)))
    b = int(sim.add_particles(dict(mesh=buckets(), **axle)))
    sim.add_articulation(dict(type="rotation", obj0=a, obj1=b))
    return [a, b], a


def _joint_particles(res):
    rng = np.random.default_rng(9)
    g = np.mgrid[33:46:0.5, 27:44:0.5, 27:37:0.5].reshape(3, -1).T + 0.25  # cells of the upper and lower right quadrant
    g = g + rng.uniform(-0.1, 0.1, g.shape)
    return (g / res).astype(np.float32), "water"


SCENES = {"paddle_wheel": (64, _wheel_scene, _wheel_particles, dict()),
          "water_wheel_joint": (64, _joint_scene, _joint_particles, dict(penalty=1e3))}


def _cpic_run(tm, scene, steps=40, det=True, reorder=0, perm=None, ids=None, switch_snapshot=None, load_snapshot=None):
    """the scene run for `steps` substeps -> (particles sorted by id, [rigid state of every body], ids in slot order at creation)
    perm / ids: particles added in the order perm, with these creation ids (F_ID); switch_snapshot: deterministic mode off for the
    first substep, a snapshot saved there, then switched on; load_snapshot: the first substep comes from that snapshot"""
    from taichi_mpm_amd.mpm import F_ID
    res, add_bodies, particles, cfg = SCENES[scene]
    x, mat = particles(res)
    sim = tm.create_simulation3("mpm").initialize(dict(res=(res,) * 3, delta_x=1.0 / res, base_delta_t=1e-4, gravity=(0, -10, 0),
                                                       max_particles=len(x) + 16, reorder_interval=reorder,
                                                       deterministic=det and switch_snapshot is None, **cfg))
    bodies, probe = add_bodies(sim, res)
    order = np.arange(len(x)) if perm is None else perm
    sim.add_particles(dict(type=mat, positions=x[order]))
    if ids is not None:
        sim.upload(F_ID, ids[order].astype(np.int32))
    ids0 = sim.get_particles(sort_by_id=False)["id"]
    done = 0
    if switch_snapshot is not None:
        sim.run_substeps(1)
        sim.save_snapshot(switch_snapshot)
        sim.set_deterministic(True)
        done = 1
    if load_snapshot is not None:
        sim.load_snapshot(load_snapshot)
        done = 1
    sim.run_substeps(steps - done)
    p = sim.get_particles(sort_by_id=True)
    st = [sim.get_rigid_state(b) for b in bodies]
    sim.close()
    return p, st, ids0, bodies.index(probe)


def _assert_same(name, a, b):
    pa, sa = a[0], a[1]
    pb, sb = b[0], b[1]
    assert np.array_equal(pa["id"], pb["id"]), name
    for f in PFIELDS:
        assert np.array_equal(pa[f], pb[f]), (name, f, float(np.abs(pa[f].astype(np.float64) - pb[f]).max()), int((pa[f] != pb[f]).sum()))
    for k, (ra, rb) in enumerate(zip(sa, sb)):
        for f in RFIELDS:
            assert np.array_equal(ra[f], rb[f]), (name, "body %d" % k, f, ra[f], rb[f])


def _guards(scene, base):
    p, st, _, probe = base
    assert (p["states"] != 0).sum() > 1000, "the scene must colour particles"
    if scene == "paddle_wheel":  # the free box: gravity alone would give (0, -10 t, 0) exactly; the sand's impulses change it
        v = st[probe]["velocity"]
        assert np.abs(v - np.float32([0.0, -10.0 * 40 * 1e-4, 0.0])).max() > 1e-3, v
    else:  # the wheel: neither gravity (applied at the centre of mass) nor its script turns it; only the water's impulses do
        w = st[probe]["angular_velocity"]
        assert abs(float(w[2])) > 1e-3 and abs(float(w[0])) == 0.0 and abs(float(w[1])) == 0.0, w


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_two_runs_of_a_cpic_scene_agree_bit_for_bit(tm, scene):
    """(a) the same scene twice in the deterministic mode"""
    base = _cpic_run(tm, scene)
    _guards(scene, base)
    _assert_same("again", base, _cpic_run(tm, scene))


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_one_stream_and_two_streams_agree_bit_for_bit(tm, scene):
    """(b) MPMHIP_RIGID_CONCURRENT=0 (everything on the ctx stream) against the default 7"""
    base = _cpic_run(tm, scene)
    with _env(MPMHIP_RIGID_CONCURRENT=0):
        one = _cpic_run(tm, scene)
    _assert_same("one stream", base, one)


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_few_rigid_workgroups_agree_bit_for_bit(tm, scene):
    """(c) MPMHIP_RIGID_WGS=2: two workgroups of k_p2g_rigid (one of k_g2p_rigid), each walking many flagged blocks"""
    base = _cpic_run(tm, scene)
    with _env(MPMHIP_RIGID_WGS=2):
        few = _cpic_run(tm, scene)
    _assert_same("MPMHIP_RIGID_WGS=2", base, few)


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_sort_forms_and_reorders_agree_bit_for_bit(tm, scene):
    """(d) MPMHIP_SORT_V1=1 against the default sort; (e) reorder_interval=3 against 0"""
    base = _cpic_run(tm, scene)
    with _env(MPMHIP_SORT_V1=1):
        v1 = _cpic_run(tm, scene)
    _assert_same("MPMHIP_SORT_V1=1", base, v1)
    _assert_same("reorder_interval=3", base, _cpic_run(tm, scene, reorder=3))


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_shuffled_upload_agrees_bit_for_bit(tm, scene):
    """(f) the same particles uploaded in a shuffled slot order with the same creation ids"""
    base = _cpic_run(tm, scene)
    n = len(base[2])
    perm = np.random.default_rng(3).permutation(n)
    _assert_same("shuffled slots", base, _cpic_run(tm, scene, perm=perm, ids=base[2]))


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_mode_switched_on_in_mid_run_takes_effect_at_the_next_substep(tm, scene, tmp_path):
    """(g) set_deterministic(True) after one default-mode substep, against a deterministic run that starts from the same first
    substep (a snapshot of it)"""
    snap = str(tmp_path / "first_substep.bin")
    switched = _cpic_run(tm, scene, switch_snapshot=snap)
    loaded = _cpic_run(tm, scene, load_snapshot=snap)
    _assert_same("switched on in mid-run", loaded, switched)


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_the_deterministic_mode_changes_no_physics(tm, scene):
    """the default mode against the deterministic one, within the bounds of test_gpu_cpic.test_one_stream_and_two_streams_give_the_same_run"""
    (a, sa, _, _), (b, sb, _, _) = _cpic_run(tm, scene), _cpic_run(tm, scene, det=False)
    assert np.array_equal(a["id"], b["id"])
    assert np.abs(a["x"] - b["x"]).max() <= 2e-6 and rel_l2(a["v"], b["v"]) <= 1e-4 and rel_l2(a["F"], b["F"]) <= 1e-5
    assert (a["states"] != b["states"]).sum() <= 5
    for ra, rb in zip(sa, sb):
        np.testing.assert_allclose(ra["velocity"], rb["velocity"], atol=2e-5)
        np.testing.assert_allclose(ra["position"], rb["position"], atol=1e-6)


def test_two_bodies_deterministic_match_the_live_reference(tm):
    """test_gpu_cpic.test_two_bodies_at_once_match_the_live_reference with deterministic=True, same scene, same bounds"""
    from oracle import refmpm
    if not refmpm.available():
        pytest.skip("oracle/_ref/libmpm_ref.so did not travel to this box")
    from oracle import oracle as orc
    refmpm.set_threads(1)
    x, v = cs.block_of_particles()
    gp = orc.group_params("sand", cs.MASS, cs.VOL)[0]
    s = cs.SCRIPT
    box_cfg = dict(cs.BODIES["box"])
    box_mesh = box_cfg.pop("mesh")
    box_cfg["initial_position"] = (0.42, 0.47, 0.46)
    ref = refmpm.Sim(cs.RES, cs.DX, cs.DT, gravity=(0, -10, 0), penalty=1e3)
    r1 = ref.add_rigid(box_mesh, **box_cfg)
    r2 = ref.add_rigid(cs.plate(0.12), script=refmpm.rigid_script((0.58, 0.56, 0.55), s["vel"], s["amp"], s["omega"], s["e0"], s["rate"]),
                       codimensional=True, friction=0.4)
    ref.add_particles("sand", cs.MASS, cs.VOL, x, v)
    sim = tm.create_simulation3("mpm").initialize(dict(res=(cs.RES,) * 3, delta_x=cs.DX, base_delta_t=cs.DT, gravity=(0, -10, 0),
                                                       max_particles=len(x) + 16, penalty=1e3, deterministic=True))
    f32 = np.float32
    p0 = (0.58, 0.56, 0.55)
    assert int(sim.add_particles(dict(type="rigid", mesh=box_mesh, **box_cfg))) == r1 == 1
    assert int(sim.add_particles(dict(
        type="rigid", mesh=cs.plate(0.12), codimensional=True, friction=0.4,
        scripted_position=lambda t: [f32(p0[k]) + f32(s["vel"][k]) * f32(t) + f32(s["amp"][k]) * f32(np.sin(f32(s["omega"]) * f32(t))) for k in range(3)],
        scripted_rotation=lambda t: [f32(s["e0"][k]) + f32(s["rate"][k]) * f32(t) for k in range(3)]))) == r2 == 2
    sim.add_particles(dict(type="sand", positions=x, velocities=v, params=gp))
    ref.substep(6)
    sim.run_substeps(6)
    r, h = ref.download(by_id=True), sim.get_particles(sort_by_id=True)
    np.testing.assert_array_equal(h["id"], r["id"])
    assert np.abs(h["x"] - r["x"]).max() <= 5e-6
    assert rel_l2(h["v"], r["v"]) <= 2e-4
    o = np.argsort(ref.download(by_id=False)["id"], kind="stable")
    st = ref.particle_cdf()["states"][o]
    assert ((st & 0xC) != 0).sum() > 300 and ((st & 0x30) != 0).sum() > 300  # both bodies colour particles
    assert (st != h["states"].astype(np.uint32)).sum() <= 5
    for rid in (r1, r2):
        a, b = cs.rigid_vector(ref.rigid_state(rid)), cs.rigid_vector(sim.get_rigid_state(rid))
        np.testing.assert_allclose(b[0:7], a[0:7], rtol=0, atol=2e-6)
        np.testing.assert_allclose(b[7:13], a[7:13], rtol=0, atol=2e-4 * max(np.abs(a[7:13]).max(), 1e-2))
    sim.close()


# ------------------------------------------------------------------------------------------ calculate_energy
E_RES, E_DX, E_DT = 32, 1.0 / 32, 1e-4


def _energy_state(orc):
    """the three-material scene of test_gpu_parity.test_calculate_energy_matches_numpy (jelly, linear, elastic)"""
    x = lattice_cube(E_RES, 9, 17, E_DX, jitter=0.2, seed=61)
    parts = [make_state(x[i::3], m, E_DX, perturb_F=0.05, seed=62 + i) for i, m in enumerate(("jelly", "linear", "elastic"))]
    return orc.State(np.concatenate([p.x for p in parts]), np.concatenate([p.v for p in parts]),
                     np.concatenate([p.B for p in parts]), np.concatenate([p.F for p in parts]),
                     np.concatenate([p.aux for p in parts]), np.concatenate([np.full(p.n, i, np.int32) for i, p in enumerate(parts)]),
                     np.concatenate([p.gparams for p in parts]), np.concatenate([p.gtype for p in parts]))


def _energy_run(tm, s, perm=None, reorder=0, steps=20):
    """(energy at creation, the same again, energy after `steps` substeps); particles added per group in the order perm, every
    particle with creation id = its index in s"""
    from taichi_mpm_amd.mpm import F_ID
    sim = tm.create_simulation3("mpm").initialize(dict(res=(E_RES,) * 3, delta_x=E_DX, base_delta_t=E_DT, gravity=(0, -10, 0),
                                                       particle_gravity=False, max_particles=s.n + 64, reorder_interval=reorder,
                                                       deterministic=True))
    names = {v: k for k, v in tm.MATERIAL_IDS.items()}
    order = np.arange(s.n) if perm is None else perm
    slots = []
    for gi in range(len(s.gtype)):
        sel = order[s.gid[order] == gi]
        sim.add_particles(dict(type=names[int(s.gtype[gi])], positions=s.x[sel], velocities=s.v[sel], F=s.F[sel], B=s.B[sel],
                               aux=s.aux[sel], params=s.gparams[gi]))
        slots.append(sel)
    sim.upload(F_ID, np.concatenate(slots).astype(np.int32))
    e0 = sim.calculate_energy()
    e1 = sim.calculate_energy()
    sim.run_substeps(steps)
    e2 = sim.calculate_energy()
    sim.close()
    return e0, e1, e2


def _bits(e):
    return tuple(np.float64(v).tobytes() for v in e)


ENERGY_CASES = {"shuffled_upload": (dict(), dict(shuffle=True)), "sort_v1": (dict(MPMHIP_SORT_V1=1), dict()),
                "reorder_interval_1": (dict(), dict(reorder=1)), "g2p_packed_0": (dict(MPMHIP_G2P_PACKED=0), dict()),
                "g2p_packed_1": (dict(MPMHIP_G2P_PACKED=1), dict()), "grid_walk_0": (dict(MPMHIP_GRID_WALK=0), dict()),
                "grid_walk_2": (dict(MPMHIP_GRID_WALK=2), dict())}


def test_energy_of_repeated_calls_is_the_same_bits(tm, orc):
    """calculate_energy twice on the same state in the deterministic mode: the same (kinetic, potential) bits"""
    e0, e1, _ = _energy_run(tm, _energy_state(orc))
    assert _bits(e0) == _bits(e1), (e0, e1)


@pytest.mark.parametrize("case", sorted(ENERGY_CASES))
def test_energy_is_the_same_bits_across_slots_sorts_reorders_and_walks(tm, orc, case):
    """calculate_energy in the deterministic mode, at creation and after 20 substeps: the same (kinetic, potential) bits as the plain
    run for a shuffled upload with the same ids, MPMHIP_SORT_V1=1, reorder_interval=1, MPMHIP_G2P_PACKED=0 / 1, MPMHIP_GRID_WALK=0 / 2"""
    s = _energy_state(orc)
    base = _energy_run(tm, s)
    env, kw = ENERGY_CASES[case]
    perm = np.random.default_rng(5).permutation(s.n) if kw.get("shuffle") else None
    with _env(**env):
        r = _energy_run(tm, s, perm=perm, reorder=kw.get("reorder", 0))
    for k in (0, 2):
        assert _bits(r[k]) == _bits(base[k]), (case, "after %d substeps" % (20 * (k // 2)), r[k], base[k])


def test_deterministic_energy_matches_numpy(tm, orc):
    """the values still match numpy within the bounds of test_gpu_parity.test_calculate_energy_matches_numpy"""
    from tests.test_gpu_parity import ocfg
    s = _energy_state(orc)
    kin, pot = _energy_run(tm, s, steps=0)[0]
    g = orc.p2g(ocfg(orc, planes=(), particle_gravity=False), s.copy()).astype(np.float64)
    m = g[..., 3]
    ref_kin = (0.5 * (g[..., :3] ** 2).sum(-1)[m > 0] / m[m > 0]).sum()
    F = s.F.reshape(-1, 3, 3).astype(np.float64)
    U, sig, Vt = np.linalg.svd(F)
    R = U @ Vt
    J = np.linalg.det(F)
    gp = s.gparams[s.gid].astype(np.float64)
    vol, mu, la = gp[:, 1], gp[:, 2], gp[:, 3]
    e_j = vol * (mu * ((F - R) ** 2).sum((1, 2)) + 0.5 * la * (J - 1) ** 2)
    eps = 0.5 * (F + F.transpose(0, 2, 1)) - np.eye(3)
    e_l = vol * (mu * (eps ** 2).sum((1, 2)) + 0.5 * la * np.trace(eps, axis1=1, axis2=2) ** 2)
    ls = np.log(sig)
    e_e = vol * (mu * (ls ** 2).sum(1) + 0.5 * la * ls.sum(1) ** 2)
    ref_pot = np.where(s.gid == 0, e_j, np.where(s.gid == 1, e_l, e_e)).sum()
    assert np.isclose(kin, ref_kin, rtol=1e-5)
    assert np.isclose(pot, ref_pot, rtol=1e-4)


def test_tiled_energy_of_two_virtual_ranks_is_the_same_bits_twice(tm):
    """a two-rank virtual job (built as test_gpu_deterministic._virtual builds it, kept open to be read) through
    mpmhip_calculate_energy_group, twice: the same kinetic bits (with sand only the kinetic part is valid, as in test_gpu_tiled)"""
    import ctypes as C

    from taichi_mpm_amd import tiled
    from tests.test_gpu_tiled import DX, RES, _two_material_state

    def run():
        s = _two_material_state()
        ids = np.arange(s.n)
        part = tiled.Partition.balanced((RES,) * 3, 2, s.x, DX, margin=2)
        owner = part.rank_of_cells(tiled.base_cells(s.x, DX))
        sims = [_det_sim(tm, s, owner == r, ids, s.n + 1024) for r in range(2)]
        job = tiled.NativeVirtualJob([tiled.HipEngine(sim, 0) for sim in sims], part, migrate_interval=2, overlap=False)
        job.run(6)
        L = sims[0]._L
        arr = (C.c_void_p * 2)(*[sim._ctx for sim in sims])
        out = []
        for _ in range(2):
            k, p = C.c_double(), C.c_double()
            rc = L.mpmhip_calculate_energy_group(arr, 2, C.byref(k), C.byref(p))
            assert rc in (0, -5), rc  # (-5: sand has no potential_energy(); the kinetic part is valid)
            out.append(k.value)
            job.run(1)
        for sim in sims:
            sim.close()
        return out

    a, b = run(), run()
    assert a[0] > 0.0
    assert [np.float64(v).tobytes() for v in a] == [np.float64(v).tobytes() for v in b], (a, b)
