"""The mesh voxeliser without a GPU: the float64 model of its rules (tests/mesh_sdf_model.py, the yardstick of
tests/test_gpu_mesh_sdf.py) against closed forms, and the Python validation of MeshLevelSet / SampledLevelSet.from_mesh, which
raises before the library is touched."""
import numpy as np
import pytest

from tests import mesh_sdf_model as M


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    return tm


@pytest.mark.parametrize("name", ["cube", "sphere", "torus"])
def test_model_meets_the_closed_form(name):
    """|phi_model - closed form| at every sample of the 41 x 37 x 33 lattice is within the bound the geometry gives: rounding for
    the cube (its faces are the surface), the sag of the longest edge for the inscribed sphere, the two sags for the torus; and no
    sample farther from the surface than the bound has the wrong sign."""
    tri, f, bound = M.case(name, fp32=False)
    phi, odd = M.voxelise(tri, M.RES, M.ORIGIN, M.SPACING)
    want = f(M.lattice_points(M.RES, M.ORIGIN, M.SPACING)).reshape(M.RES)
    err = np.abs(phi - want).max()
    print("%s: %d triangles, bound %.3g, seen %.3g, smallest |phi| %.3g" % (name, len(tri), bound, err, np.abs(phi).min()))
    assert odd == 0
    assert len(tri) == {"cube": 12, "sphere": 1280, "torus": 4096}[name]
    assert err <= bound
    assert not ((np.sign(phi) != np.sign(want)) & (np.abs(want) > bound)).any()
    assert (phi < 0).any() and (phi > 0).any()
    if name == "sphere":  # inscribed and convex: the mesh lies inside the sphere
        assert (phi - want).min() >= -1e-12
    if name == "cube":
        assert np.abs(phi).min() > 1e-3  # no sample on the surface


def test_fp32_transcription_is_close_and_order_free():
    """the float32 transcription stays within a few ulp of the float64 run; shuffling the triangles or reversing their orientation
    changes no bit of either"""
    tri = M.icosphere(2, *M.SPHERE).astype(np.float32)
    p64, _ = M.voxelise(tri, M.RES, M.ORIGIN, M.SPACING)
    p32, _ = M.voxelise(tri, M.RES, M.ORIGIN, M.SPACING, dtype=np.float32)
    assert p32.dtype == np.float32
    assert np.abs(p32 - p64).max() < 5e-7
    other = tri[np.random.default_rng(3).permutation(len(tri))][:, ::-1]
    for dt, ref in ((np.float64, p64), (np.float32, p32)):
        assert np.array_equal(M.voxelise(other, M.RES, M.ORIGIN, M.SPACING, dtype=dt)[0], ref)
    banded, _ = M.voxelise(tri, M.RES, M.ORIGIN, M.SPACING, band=0.1)
    near = np.abs(p64) < 0.1
    assert np.array_equal(banded[near], p64[near]) and np.all(np.abs(banded[~near]) == 0.1)


@pytest.mark.parametrize("name", ["cube", "octahedron"])
def test_lattice_aligned_meshes_get_every_sign_right(name):
    """faces and edges of the cube, vertices of the octahedron lie exactly on sample columns of the 33^3 lattice: every sample off
    the surface has the closed form's sign, no column is odd, and reversing all triangles changes nothing"""
    if name == "cube":
        tri, f, on_surface = M.cube_mesh(*M.ALIGNED_CUBE), M.cube_sdf(*M.ALIGNED_CUBE), 1026
    else:
        tri, f, on_surface = M.octahedron_mesh(*M.ALIGNED_OCTA), M.octahedron_sign(*M.ALIGNED_OCTA), 258
    lat = (M.ALIGNED_RES, M.ALIGNED_ORIGIN, M.ALIGNED_SPACING)
    want = f(M.lattice_points(*lat)).reshape(M.ALIGNED_RES)
    phi, odd = M.voxelise(tri, *lat)
    off = want != 0
    assert odd == 0 and (~off).sum() == on_surface
    assert np.array_equal(np.sign(phi[off]), np.sign(want[off]))
    assert np.all(phi[~off] == 0)
    assert np.array_equal(M.voxelise(tri[:, ::-1], *lat)[0], phi)


def test_open_and_degenerate_meshes():
    tri = M.cube_mesh(*M.CUBE)
    lid = np.delete(tri, [4, 10], axis=0)  # the face z = lo is gone
    _, odd = M.parity(lid, M.RES, M.ORIGIN, M.SPACING)
    cols = M.lattice_axes(M.RES, M.ORIGIN, M.SPACING)
    inside = [((c > lo) & (c < hi)).sum() for c, lo, hi in zip(cols[:2], M.CUBE[0][:2], M.CUBE[1][:2])]
    assert odd == inside[0] * inside[1] > 0
    # zero-area triangles (a repeated vertex, three collinear points) change nothing
    extra = np.array([[tri[0, 0], tri[0, 0], tri[0, 1]], [tri[0, 0], (tri[0, 0] + tri[0, 1]) / 2, tri[0, 1]]])
    a, odd_a = M.voxelise(np.concatenate([tri, extra]), M.RES, M.ORIGIN, M.SPACING)
    b, _ = M.voxelise(tri, M.RES, M.ORIGIN, M.SPACING)
    assert odd_a == 0 and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ Python layer
def test_mesh_levelset_validation(tm, tmp_path):
    tri = M.cube_mesh(*M.CUBE)
    E = tm.MPMError
    ok = tm.MeshLevelSet(tri, M.RES, M.ORIGIN, M.SPACING, band=0.1, friction=0.3)
    assert ok.triangles.dtype == np.float32 and ok.triangles.shape == (12, 3, 3) and ok.res == M.RES
    assert ok.band_for(M.SPACING) == 0.1 and tm.MeshLevelSet(tri, M.RES, M.ORIGIN, M.SPACING).band_for(M.SPACING) == 8 * M.SPACING
    assert tm.MeshLevelSet(tri, M.RES, band=float("inf")).band_for(0.1) == float("inf")
    for bad in (tri[:, :2], tri.reshape(-1, 9), tri[:0], np.zeros((3, 3))):
        with pytest.raises(E):
            tm.MeshLevelSet(bad, M.RES, M.ORIGIN, M.SPACING)
    nan = tri.copy()
    nan[3, 1, 2] = np.nan
    with pytest.raises(E, match="non-finite"):
        tm.MeshLevelSet(nan, M.RES, M.ORIGIN, M.SPACING)
    for band in (0.0, -1.0, float("nan")):
        with pytest.raises(E, match="band"):
            tm.MeshLevelSet(tri, M.RES, M.ORIGIN, M.SPACING, band=band)
    for kw in (dict(res=(41, 1, 33)), dict(res=(41, 37)), dict(spacing=0.0), dict(spacing=float("nan")), dict(origin=(0, float("inf"), 0))):
        with pytest.raises(E):
            tm.MeshLevelSet(tri, **{**dict(res=M.RES, origin=M.ORIGIN, spacing=M.SPACING), **kw})
    # missing spacing: a MeshLevelSet takes the simulation's, from_mesh has no simulation to take it from
    assert tm.MeshLevelSet(tri, M.RES).spacing is None
    with pytest.raises(E, match="spacing"):
        tm.MeshLevelSet(tri, M.RES).get_delta_x()
    with pytest.raises(E, match="spacing"):
        tm.SampledLevelSet.from_mesh(tri, M.RES, M.ORIGIN)
    with pytest.raises(E, match="non-finite"):
        tm.SampledLevelSet.from_mesh(nan, M.RES, M.ORIGIN, M.SPACING)
    # a path goes through load_obj_triangles
    obj = tmp_path / "cube.obj"
    verts = np.unique(tri.reshape(-1, 3), axis=0)
    idx = [[int(np.nonzero((verts == v).all(1))[0][0]) + 1 for v in t] for t in tri]
    obj.write_text("".join("v %r %r %r\n" % tuple(float(a) for a in v) for v in verts) + "".join("f %d %d %d\n" % tuple(i) for i in idx))
    assert np.array_equal(tm.MeshLevelSet(str(obj), M.RES).triangles, tri.astype(np.float32))


def test_key_frames_and_transform(tm):
    tri = M.cube_mesh(*M.CUBE)
    a = tm.MeshLevelSet(tri, M.RES, M.ORIGIN, M.SPACING, band=0.1, friction=0.3)
    b = a.with_transform(translation=(0.02, 0.01, 0.0))
    assert b.same_lattice(a) and b.friction == 0.3 and b.band == 0.1
    assert np.allclose(b.triangles, tri + (0.02, 0.01, 0.0), atol=1e-7) and np.array_equal(a.triangles, tri.astype(np.float32))
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    assert np.allclose(a.with_transform(R, (0.1, 0, 0)).triangles, tri @ R.T + (0.1, 0, 0), atol=1e-7)
    with pytest.raises(tm.MPMError):
        a.with_transform(np.eye(2))
    dyn = tm.DynamicLevelSet().initialize(0.0, 1.0, a, b)
    assert dyn.levelset0 is a and dyn.levelset1 is b
    sampled = tm.SampledLevelSet(np.zeros(M.RES, np.float32), M.ORIGIN, M.SPACING)
    analytic = tm.LevelSet().add_plane((0, 1, 0), d=-0.3)
    for other in (sampled, analytic):
        for pair in ((a, other), (other, a)):
            with pytest.raises(tm.MPMError, match="mixed"):
                tm.DynamicLevelSet().initialize(0.0, 1.0, *pair)
    for other in (tm.MeshLevelSet(tri, M.RES, M.ORIGIN, 0.03, band=0.1), tm.MeshLevelSet(tri, (41, 37, 34), M.ORIGIN, M.SPACING, band=0.1),
                  tm.MeshLevelSet(tri, M.RES, M.ORIGIN, M.SPACING, band=0.2)):
        with pytest.raises(tm.MPMError, match="share"):
            tm.DynamicLevelSet().initialize(0.0, 1.0, a, other)


def test_new_entry_points_are_declared_and_exported():
    import os
    from taichi_mpm_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpmhip.h")).read()
    for sym in ("mpmhip_mesh_to_sdf", "mpmhip_set_levelset_mesh", "mpmhip_download_levelset_sdf"):
        assert sym in _lib.exported_symbols() and ("int %s(" % sym) in header
    assert "meshes -> SDF" not in header


def test_the_example_bowl_is_closed():
    """examples/sand_bowl.py generates its mesh in code: as float32 it is closed by the model's column test, and hollow"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "sand_bowl.py")
    spec = importlib.util.spec_from_file_location("sand_bowl_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tri = mod.bowl().astype(np.float32)
    inside, odd = M.parity(tri, (33, 33, 33), (0, 0, 0), 1.0 / 32)
    assert odd == 0
    c = [int(round(v * 32)) for v in mod.CENTRE]
    wall = int(round((mod.R_OUT + mod.R_IN) / 2 * 32))
    assert inside[c[0], c[1] - wall, c[2]] and not inside[c[0], c[1] - 4, c[2]] and not inside[c[0], c[1] + 2, c[2]]
