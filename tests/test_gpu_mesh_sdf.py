"""Triangle meshes voxelised on the device into sampled level sets (include/mpmhip.h: mpmhip_mesh_to_sdf, mpmhip_set_levelset_mesh,
mpmhip_download_levelset_sdf; run with -m gpu on an MI355X).  The yardstick is the float64 model of the rules,
tests/mesh_sdf_model.py, itself checked against closed forms in tests/test_mesh_sdf_cpu.py.

Figures of the last run (world units, MI355X), model = float64:
    none recorded yet — DESIGN.md says which runs are missing."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import mesh_sdf_model as M
from tests.sdf_model import SdfModel

pytestmark = pytest.mark.gpu
INF = float("inf")
LAT = (M.RES, M.ORIGIN, M.SPACING)
ALIGNED = (M.ALIGNED_RES, M.ALIGNED_ORIGIN, M.ALIGNED_SPACING)


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@functools.lru_cache(maxsize=None)
def _model(name):
    """(triangles as the device gets them, float64 model, tol): tol = 8 x the largest difference between the model's own float32
    transcription and its float64 run on the same inputs"""
    if name == "aligned_cube":
        tri, lat = M.cube_mesh(*M.ALIGNED_CUBE).astype(np.float32), ALIGNED
    elif name == "aligned_octa":
        tri, lat = M.octahedron_mesh(*M.ALIGNED_OCTA).astype(np.float32), ALIGNED
    elif name == "cube_moved":
        tri, lat = (M.cube_mesh(*M.CUBE) + (0.02, 0.01, 0.0)).astype(np.float32), LAT
    else:
        tri, lat = M.case(name)[0], LAT
    p64, odd = M.voxelise(tri, *lat)
    p32, _ = M.voxelise(tri, *lat, dtype=np.float32)
    assert odd == 0
    return tri, p64, 8.0 * float(np.abs(p32.astype(np.float64) - p64).max())


def _voxelise(tm, tri, lat, band):
    return tm.SampledLevelSet.from_mesh(tri, lat[0], lat[1], lat[2], band=band).phi


def _sim(tm, res, dx, dt, **cfg):
    return tm.create_simulation3("mpm").initialize(dict(res=(res,) * 3, delta_x=dx, base_delta_t=dt, **cfg))


# ------------------------------------------------------------------------------------------ 1: the device against the model
@pytest.mark.parametrize("name", ["cube", "sphere", "torus"])
@pytest.mark.parametrize("band", [INF, 4 * M.SPACING])
def test_device_matches_the_float64_model(tm, name, band):
    """|phi_dev - phi_model| <= tol at every sample, tol = 8 x (model in float32 - model in float64): the device may contract and
    reorder what numpy does not, which changes single roundings, not their amplification.  The sign equals the model's at every
    sample with |phi_model| > tol, and those left out are at most 0.1 % (none, on these inputs)."""
    tri, p64, tol = _model(name)
    want = np.sign(p64) * np.minimum(np.abs(p64), np.float32(band).astype(np.float64))
    got = _voxelise(tm, tri, LAT, band).astype(np.float64)
    err = np.abs(got - want).max()
    clear = np.abs(p64) > tol
    print("%s band %s: tol %.3g, device - model %.3g, smallest |phi_model| %.3g, left out %d" % (name, band, tol, err, np.abs(p64).min(), (~clear).sum()))
    assert 0 < tol < 2e-6
    assert err <= tol
    assert np.array_equal(np.sign(got[clear]), np.sign(want[clear]))
    assert (~clear).mean() <= 1e-3


# ------------------------------------------------------------------------------------------ 2: band, and the ctx route
@pytest.mark.parametrize("name", ["cube", "sphere", "torus"])
def test_band_clamps_and_changes_no_bit_inside(tm, name):
    tri = _model(name)[0]
    band = np.float32(4 * M.SPACING)
    full, banded = _voxelise(tm, tri, LAT, INF), _voxelise(tm, tri, LAT, float(band))
    near = np.abs(full) < band
    assert 0.02 < near.mean() < 0.98
    assert np.array_equal(banded[near], full[near])
    assert np.array_equal(banded[~near], np.where(full[~near] < 0, -band, band))


def test_ctx_route_equals_mesh_to_sdf(tm):
    """set_levelset(MeshLevelSet) + download_levelset_sdf give the bits of SampledLevelSet.from_mesh, static and for two key frames,
    with a lattice change and a reuse of the device arrays in between"""
    sim = _sim(tm, 32, 1.0 / 32, 1e-4)
    sphere, torus = _model("sphere")[0], _model("torus")[0]
    band = 4 * M.SPACING
    sim.set_levelset(tm.MeshLevelSet(sphere, *LAT, band=band))
    phi, origin, spacing = sim.download_levelset_sdf()
    assert origin == M.ORIGIN and spacing == M.SPACING
    assert np.array_equal(phi, _voxelise(tm, sphere, LAT, band))
    with pytest.raises(tm.MPMError, match="key frame"):
        sim.download_levelset_sdf(1)
    sim.set_levelset(tm.DynamicLevelSet().initialize(0.0, 1.0, tm.MeshLevelSet(torus, *LAT, band=INF), tm.MeshLevelSet(sphere, *LAT, band=INF)))
    assert np.array_equal(sim.download_levelset_sdf(0)[0], _voxelise(tm, torus, LAT, INF))
    assert np.array_equal(sim.download_levelset_sdf(1)[0], _voxelise(tm, sphere, LAT, INF))
    cube = _model("aligned_cube")[0]
    sim.set_levelset(tm.MeshLevelSet(cube, M.ALIGNED_RES, M.ALIGNED_ORIGIN, band=0.2))  # spacing: the simulation's
    phi, origin, spacing = sim.download_levelset_sdf()
    assert spacing == 1.0 / 32 and np.array_equal(phi, _voxelise(tm, cube, ALIGNED, 0.2))
    # a voxelisation can be cached and come back as arrays: the same level set
    x = np.random.default_rng(2).uniform(0.1, 0.9, (20000, 3)).astype(np.float32)
    a = sim.sample_levelset(x)
    sim.set_levelset(tm.SampledLevelSet(phi, origin, spacing))
    b = sim.sample_levelset(x)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    sim.close()


# ------------------------------------------------------------------------------------------ 3: order-free
@pytest.mark.parametrize("band", [INF, 4 * M.SPACING])
def test_result_does_not_depend_on_order_or_orientation(tm, band):
    tri = _model("torus")[0]
    ref = _voxelise(tm, tri, LAT, band)
    assert np.array_equal(_voxelise(tm, tri, LAT, band), ref)
    rng = np.random.default_rng(17)
    assert np.array_equal(_voxelise(tm, tri[rng.permutation(len(tri))], LAT, band), ref)
    assert np.array_equal(_voxelise(tm, np.ascontiguousarray(tri[:, ::-1]), LAT, band), ref)
    rolled = np.stack([np.roll(t, k, axis=0) for t, k in zip(tri, rng.integers(0, 3, len(tri)))])
    assert np.array_equal(_voxelise(tm, rolled, LAT, band), ref)


# ------------------------------------------------------------------------------------------ 4: degenerate alignment
@pytest.mark.parametrize("name", ["aligned_cube", "aligned_octa"])
def test_lattice_aligned_meshes(tm, name):
    """faces, edges and vertices exactly on sample columns: the sign is right at every sample off the surface, |phi| <= tol on it"""
    tri, p64, tol = _model(name)
    f = M.cube_sdf(*M.ALIGNED_CUBE) if name == "aligned_cube" else M.octahedron_sign(*M.ALIGNED_OCTA)
    want = f(M.lattice_points(*ALIGNED)).reshape(M.ALIGNED_RES)
    off = want != 0
    assert (~off).sum() == (1026 if name == "aligned_cube" else 258)
    for t in (tri, np.ascontiguousarray(tri[:, ::-1])):
        got = _voxelise(tm, t, ALIGNED, INF)
        assert np.array_equal(np.sign(got[off]), np.sign(want[off]))
        assert np.abs(got[~off]).max() <= tol
        assert np.abs(got - p64).max() <= tol


# ------------------------------------------------------------------------------------------ 5: refusals
def _desc(res=M.RES, origin=M.ORIGIN, spacing=M.SPACING):
    from taichi_mpm_amd import _lib
    d = _lib.SdfDesc()
    d.res[:] = res
    d.origin[:] = origin
    d.spacing = spacing
    return C.byref(d)


def test_open_mesh_is_refused_and_the_installed_set_stays(tm):
    sim = _sim(tm, 32, 1.0 / 32, 1e-4)
    sphere = _model("sphere")[0]
    sim.set_levelset(tm.MeshLevelSet(sphere, *LAT, band=INF, friction=0.3))
    before = sim.download_levelset_sdf()[0]
    x = np.random.default_rng(4).uniform(0.1, 0.9, (5000, 3)).astype(np.float32)
    sampled = sim.sample_levelset(x)
    cube = M.cube_mesh(*M.CUBE).astype(np.float32)
    lid = np.ascontiguousarray(np.delete(cube, [4, 10], axis=0))  # the face z = lo is gone
    odd = M.parity(lid, *LAT)[1]
    assert odd > 100
    fp = C.POINTER(C.c_float)
    L = sim._L
    EINVAL = L.mpmhip_set_levelset_mesh(sim._ctx, None, 12, cube.ctypes.data_as(fp), 0, None, 0, 1, 0.1, 0.0)
    assert EINVAL < 0
    rc = L.mpmhip_set_levelset_mesh(sim._ctx, _desc(), len(lid), lid.ctypes.data_as(fp), 0, None, 0, 1, 0.1, 0.0)
    msg = L.mpmhip_last_error(sim._ctx).decode()
    assert rc == EINVAL and "not closed" in msg and ("%d lattice columns" % odd) in msg, msg
    # ... as the second key frame too, and on a lattice of another size (the arrays are not reallocated before the verdict)
    rc = L.mpmhip_set_levelset_mesh(sim._ctx, _desc(res=(20, 20, 20), spacing=0.05), 12, cube.ctypes.data_as(fp), len(lid), lid.ctypes.data_as(fp),
                                    0.0, 1.0, 0.1, 0.0)
    assert rc == EINVAL and "second key frame" in L.mpmhip_last_error(sim._ctx).decode()
    assert np.array_equal(sim.download_levelset_sdf()[0], before)
    for u, v in zip(sim.sample_levelset(x), sampled):
        assert np.array_equal(u, v)
    # the ctx-free entry: no output is written, the message is the library's
    out = np.full(M.RES, 7.0, np.float32)
    rc = L.mpmhip_mesh_to_sdf(0, _desc(), len(lid), lid.ctypes.data_as(fp), 0.1, out.ctypes.data_as(fp))
    assert rc == EINVAL and ("%d lattice columns" % odd) in L.mpmhip_last_error(None).decode() and np.all(out == 7.0)
    with pytest.raises(tm.MPMError, match="not closed"):
        tm.SampledLevelSet.from_mesh(lid, *LAT)
    sim.close()


def test_argument_checks(tm):
    sim = _sim(tm, 32, 1.0 / 32, 1e-4)
    sim._ensure_ctx()
    L, fp = sim._L, C.POINTER(C.c_float)
    cube = M.cube_mesh(*M.CUBE).astype(np.float32)
    p = cube.ctypes.data_as(fp)
    out = np.zeros(M.RES, np.float32)
    o = out.ctypes.data_as(fp)
    assert L.mpmhip_mesh_to_sdf(0, _desc(), 12, p, 0.1, o) == 0
    EINVAL = L.mpmhip_mesh_to_sdf(0, None, 12, p, 0.1, o)
    assert EINVAL < 0
    nan = cube.copy()
    nan[5, 2, 1] = np.inf
    flat = np.zeros((4, 3, 3), np.float32)  # zero-area triangles only
    calls = [lambda d, n, t, b: L.mpmhip_mesh_to_sdf(0, d, n, t, b, o),
             lambda d, n, t, b: L.mpmhip_set_levelset_mesh(sim._ctx, d, n, t, 0, None, 0.0, 1.0, b, 0.0),
             lambda d, n, t, b: L.mpmhip_set_levelset_mesh(sim._ctx, _desc(), 12, p, n, t if t else p, 0.0, 1.0, b, 0.0)]
    for i, call in enumerate(calls):
        err = (lambda: L.mpmhip_last_error(None)) if i == 0 else (lambda: L.mpmhip_last_error(sim._ctx))
        for d, n, t, b in ((_desc(), 0, p, 0.1), (_desc(), -3, p, 0.1), (_desc(), 12, p, 0.0), (_desc(), 12, p, -0.1), (_desc(), 12, p, float("nan")),
                           (_desc(), 12, nan.ctypes.data_as(fp), 0.1), (_desc(), 4, flat.ctypes.data_as(fp), 0.1)):
            assert call(d, n, t, b) == EINVAL, (i, n, b)
            assert len(err()) > 0
        if i < 2:
            assert call(_desc(), 12, None, 0.1) == EINVAL
            for bad in (_desc(res=(41, 1, 33)), _desc(spacing=0.0), _desc(spacing=float("nan")), _desc(origin=(0, float("inf"), 0)),
                        _desc(res=(4, 4, 8192))):
                assert call(bad, 12, p, 0.1) == EINVAL
    assert L.mpmhip_mesh_to_sdf(-1, _desc(), 12, p, 0.1, o) == EINVAL and L.mpmhip_mesh_to_sdf(4096, _desc(), 12, p, 0.1, o) == EINVAL
    assert L.mpmhip_mesh_to_sdf(0, _desc(), 12, p, 0.1, None) == EINVAL
    assert L.mpmhip_set_levelset_mesh(sim._ctx, _desc(), 12, p, 12, p, 1.0, 1.0, 0.1, 0.0) == EINVAL  # t0 < t1
    # download: nothing sampled installed, then too little room, then a frame that is not there
    assert L.mpmhip_download_levelset_sdf(sim._ctx, 0, o, out.size) == EINVAL
    assert L.mpmhip_set_levelset_mesh(sim._ctx, _desc(), 12, p, 0, None, 0.0, 1.0, 0.1, 0.0) == 0
    assert L.mpmhip_download_levelset_sdf(sim._ctx, 0, o, out.size - 1) == EINVAL
    assert L.mpmhip_download_levelset_sdf(sim._ctx, 1, o, out.size) == EINVAL
    assert L.mpmhip_download_levelset_sdf(sim._ctx, 0, None, out.size) == EINVAL
    assert L.mpmhip_download_levelset_sdf(sim._ctx, 0, o, out.size) == 0
    # rigid_body_levelset_collision and a mesh: refused both ways round, naming the combination
    assert L.mpmhip_set_rigid_levelset_collision(sim._ctx, 1) == EINVAL
    sim.set_levelset(tm.LevelSet().add_plane((0, 1, 0), d=-0.3))
    assert L.mpmhip_set_rigid_levelset_collision(sim._ctx, 1) == 0
    assert L.mpmhip_set_levelset_mesh(sim._ctx, _desc(), 12, p, 0, None, 0.0, 1.0, 0.1, 0.0) == EINVAL
    assert b"sampled" in L.mpmhip_last_error(sim._ctx)
    sim.close()
    sim = _sim(tm, 32, 1.0 / 32, 1e-4, rigid_body_levelset_collision=True)
    sim._ensure_ctx()
    with pytest.raises(tm.MPMError, match="rigid_body_levelset_collision"):
        sim.set_levelset(tm.MeshLevelSet(cube, *LAT))
    sim.close()


def test_a_call_inside_a_substep_is_refused(tm):
    from tests.common import lattice_cube, make_state
    res, dx = 32, 1.0 / 32
    sim = _sim(tm, res, dx, 1e-4)
    s = make_state(lattice_cube(res, 12, 16, dx, jitter=0.2, seed=1), "jelly", dx)
    sim.add_particles(dict(type="jelly", positions=s.x, velocities=s.v, F=s.F, B=s.B, aux=s.aux, params=s.gparams[0]))
    sim.substep()
    L, fp = sim._L, C.POINTER(C.c_float)
    cube = M.cube_mesh(*M.CUBE).astype(np.float32)
    assert L.mpmhip_substep_begin(sim._ctx) == 0
    rc = L.mpmhip_set_levelset_mesh(sim._ctx, _desc(), 12, cube.ctypes.data_as(fp), 0, None, 0.0, 1.0, 0.1, 0.0)
    msg = L.mpmhip_last_error(sim._ctx).decode()
    assert L.mpmhip_substep_end(sim._ctx) == 0
    assert rc < 0 and "inside a substep" in msg
    assert L.mpmhip_set_levelset_mesh(sim._ctx, _desc(), 12, cube.ctypes.data_as(fp), 0, None, 0.0, 1.0, 0.1, 0.0) == 0
    sim.close()


# ------------------------------------------------------------------------------------------ 6: key frames
def test_two_mesh_key_frames_blend_like_the_model(tm):
    """the cube and the cube moved by (0.02, 0.01, 0) as two mesh key frames; sample_levelset at 10^5 points and three times against
    tests/sdf_model.py fed the float64 model's two arrays.  The sampler's own bounds are those of
    tests/test_gpu_sdf.py::test_device_sampler_matches_the_model (2^-20 M on phi, M = the cell's largest |phi|); the arrays the device
    interpolates differ from the model's by at most w = tol + one float32 rounding of the model's value, and an interpolation or a blend
    of values within w stays within w: phi within 2^-20 M + w / dx, d phi / dt within (2^-20 M + 2 w / dx) / (t1 - t0).  A component of
    a sample's gradient is a difference of two values over one or two spacings: within e = 2 w / spacing, the raw vector within
    sqrt(3) e, and so is its interpolation.  A unit vector g / |g| moves by at most twice the raw error over |g|; the blend of two such
    normals, of length >= 0.97, normalised again, by twice that over 0.97: 2^-18 (the sampler's own bound) + 4.2 sqrt(3) e / |g|,
    asserted where the sampler's own bound applies and |g| >= 0.5 in both frames (a distance field's |g| is 1 off its medial axis)."""
    tri0, p0, tol0 = _model("cube")
    tri1, p1, tol1 = _model("cube_moved")
    band = 8 * M.SPACING
    clamp = lambda p: np.sign(p) * np.minimum(np.abs(p), np.float64(np.float32(band)))
    p0, p1 = clamp(p0), clamp(p1)
    w = max(tol0, tol1) + 2.0 ** -24 * max(np.abs(p0).max(), np.abs(p1).max())
    dx = 1.0 / 32
    sim = _sim(tm, 32, dx, 1e-4)
    t0, t1 = 0.5, 2.0
    sim.set_levelset(tm.DynamicLevelSet().initialize(t0, t1, tm.MeshLevelSet(tri0, *LAT, friction=0.3), tm.MeshLevelSet(tri1, *LAT, friction=0.3)))
    model = SdfModel(p0, M.ORIGIN, M.SPACING, dx, p1, t0, t1)
    rng = np.random.default_rng(23)
    lo, hi = np.array(M.ORIGIN), np.array(M.ORIGIN) + (np.array(M.RES) - 1) * M.SPACING
    x = np.concatenate([rng.uniform(lo, hi, (90000, 3)), rng.uniform(lo - 0.1, hi + 0.1, (10000, 3))]).astype(np.float32)
    hit_m, c, f = model.locate(x)
    Mx, G = model.cell_max_abs(c), model.cell_max_grad(c)
    for t in (0.7, 1.25, 1.9):
        phi, g, dphidt, hit = sim.sample_levelset(x, t)
        mphi, mg, mdphidt, _ = model.sample(x, t)
        assert np.array_equal(hit, hit_m) and 0.5 < hit.mean() < 0.99
        h = hit
        worst = (np.abs(phi - mphi)[h] / (2.0 ** -20 * Mx[h] + w / dx)).max()
        print("t=%s: |dphi| / (2^-20 M + w / dx) <= %.3f (w = %.3g)" % (t, worst, w))
        assert worst <= 1.0
        assert np.all(np.abs(dphidt - mdphidt)[h] <= (2.0 ** -20 * Mx[h] + 2 * w / dx) / (t1 - t0))
        raw0, raw1 = model.raw_gradient(model.phi0, c, f), model.raw_gradient(model.phi1, c, f)
        l0, l1 = np.linalg.norm(raw0, axis=1), np.linalg.norm(raw1, axis=1)
        n0, n1 = raw0 / np.maximum(l0, 1e-30)[:, None], raw1 / np.maximum(l1, 1e-30)[:, None]
        a = (t - t0) / (t1 - t0)
        lmin = np.minimum(l0, l1)
        well = h & (G <= 2 * l0) & (G <= 2 * l1) & (np.linalg.norm(n0 * (1 - a) + n1 * a, axis=1) >= 0.97) & (lmin >= 0.5)
        assert well.sum() > 0.3 * h.sum()
        bound = 2.0 ** -18 + 4.2 * np.sqrt(3.0) * (2 * w / M.SPACING) / lmin[well]
        worst = (np.abs(g - mg)[well].max(axis=1) / bound).max()
        print("t=%s: |dn| / bound <= %.3f over %d of %d points" % (t, worst, well.sum(), h.sum()))
        assert worst <= 1.0
    sim.close()


# ------------------------------------------------------------------------------------------ 7, 8: a scene
def _torus_mesh_set(tm):
    from tests.test_gpu_sdf import DX9, RES9, TORUS_C, TORUS_R, TUBE_R
    tri = M.torus_mesh(TORUS_R, TUBE_R, TORUS_C, 96, 48).astype(np.float32)
    return tm.MeshLevelSet(tri, (RES9 + 1,) * 3, (0, 0, 0), DX9, band=3 * DX9 + 2 * DX9, friction=0.4)


def test_sand_on_a_torus_given_as_a_mesh(tm):
    """the torus drop of tests/test_gpu_sdf.py (same block, 300 substeps, particle_collision) with the torus given as 96 x 48 quads
    through MeshLevelSet, band = 3 dx + 2 spacing: nothing is lost, everything is finite, and the device phi at every final position
    is >= -0.5 cells — that test's cap on gross failure, kept as a condition; the closed-form run beside it is held to the same cap.
    Lowest values of the last run: not recorded yet."""
    from tests.test_gpu_sdf import FIELDS, _drop, _sand, _torus_set
    s = _sand()
    lowest = {}
    for name, ls in (("mesh", _torus_mesh_set(tm)), ("closed form", _torus_set(tm))):
        sim = _drop(tm, s, ls, 300)
        p = sim.get_particles()
        assert len(p["x"]) == s.n, name
        for f in FIELDS:
            assert np.isfinite(p[f]).all(), (name, f)
        phi, _, _, hit = sim.sample_levelset(p["x"])
        sim.close()
        assert hit.all()
        assert (phi < 1.0).sum() > 100  # the sand did reach the torus
        lowest[name] = float(phi.min())
    print("lowest phi after 300 substeps: torus as a mesh %.4f cells, closed-form torus %.4f cells" % (lowest["mesh"], lowest["closed form"]))
    assert lowest["closed form"] >= -0.5
    assert lowest["mesh"] >= -0.5


def test_deterministic_mode_is_bitwise_with_a_mesh_installed_set(tm):
    from tests.test_gpu_sdf import DT9, FIELDS, _drop, _sand
    s = _sand()

    def run():
        sim = _drop(tm, s, _torus_mesh_set(tm), 120, deterministic=True)
        out = sim.get_particles()
        sim.close()
        return out
    a, b = run(), run()
    assert np.abs(a["v"][:, 1] - (-2.0 - 10.0 * 120 * DT9)).max() > 0.05  # not free fall any more: the torus acts on the sand
    assert np.array_equal(a["id"], b["id"])
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), f
