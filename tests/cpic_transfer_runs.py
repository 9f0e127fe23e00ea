"""Runs of the scenes of tests/cpic_transfer_scenes.py: the two builders (a ctx of the device, a simulation of the compiled reference),
the recorder of the reference's stage-by-stage run, and the step from a recorded colour field to the model's inputs
(tests/cpic_transfer_model.py: Cpic).  A RECORD is a dict of arrays: the colour field after sort + rasterize_rigid_boundary + gather_cdf
(cdf_idx / cdf_words: the non-zero node words, pstate, normal, dist, near per particle in creation order, samples: the boundary
particles' world positions, bodies0: the bodies' rows) and, where a whole run was recorded, the outputs of P2G, the grid update and G2P."""
import warnings

import numpy as np

from tests.common import MAT_KW
from tests.cpic_transfer_scenes import DT, GRAVITY, PENALTY, PUSHING_FORCE


# ---------------------------------------------------------------------------------------------- the two builders
def _move(sim, set_velocity, rid, delta, then_v, then_w):
    """body rid displaced by delta (world units): the velocity delta / dt for one advect_rigid_bodies(), then the given velocities
    (advect adds gravity's dt g to the velocity first: overwritten)"""
    set_velocity(rid, np.asarray(delta, np.float64) / DT, (0.0, 0.0, 0.0))
    sim.advect_rigid_bodies()
    set_velocity(rid, then_v, then_w)


def _place_bodies(sim, set_velocity, s, rids):
    for rid, b in zip(rids, s["bodies"]):
        if b["move"] is not None:
            _move(sim, set_velocity, rid, b["move"], b["velocity"], b["angular_velocity"])
        else:
            set_velocity(rid, b["velocity"], b["angular_velocity"])


def _presweep(sim, set_velocity, s, rids):
    """the particles take their colours from the bodies where they are, then body 1 moves on (scene `window`)"""
    if s["presweep"] is None:
        return
    sim.sort_particles_and_populate_grid() if hasattr(sim, "sort_particles_and_populate_grid") else sim.sort()
    sim.rasterize_rigid_boundary()
    sim.gather_cdf()
    b = s["bodies"][0]
    _move(sim, set_velocity, rids[0], np.asarray(s["presweep"]) * s["dx"], b["velocity"], b["angular_velocity"])


def _rigid_cfg(b):
    return {k: v for k, v in b.items() if k not in ("velocity", "angular_velocity", "move")}


def build_device(tm, s, **cfg):
    """a ctx holding the scene: the bodies first (their boundary particles take creation ids, as in the reference), then the state in
    upload order, group by group, past the Python layer's near-boundary filter.  Returns (sim, body ids)."""
    import ctypes as C
    sim = tm.create_simulation3("mpm").initialize(dict(res=s["res"], delta_x=s["dx"], base_delta_t=DT, gravity=GRAVITY, clean_boundary=False,
                                                       penalty=PENALTY, pushing_force=PUSHING_FORCE, **cfg))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (two free bodies: they do not collide with each other here)
        rids = [int(sim.add_particles(dict(type="rigid", **_rigid_cfg(b)))) for b in s["bodies"]]
    st = s["state"]
    sim._ensure_ctx(extra=st.n)
    for gi in range(len(st.gtype)):
        params = np.ascontiguousarray(st.gparams[gi], np.float32)
        sim._groups.append((int(st.gtype[gi]), params))
        sim._check(sim._L.mpmhip_add_group(sim._ctx, int(st.gtype[gi]), params.ctypes.data_as(C.POINTER(C.c_float))))
        m = st.gid == gi
        sim._upload_new(gi, st.x[m], st.v[m], st.F[m], st.B[m], st.aux[m])
    sim._n_added = st.n
    sv = lambda rid, v, w: sim.set_rigid_velocity(rid, velocity=v, angular_velocity=w)  # noqa: E731
    _place_bodies(sim, sv, s, rids)
    _presweep(sim, sv, s, rids)
    return sim, rids


def build_reference(refmpm, s):
    """the same scene in the compiled reference (oracle.refmpm), one thread"""
    refmpm.set_threads(1)
    ref = refmpm.Sim(s["res"], s["dx"], DT, gravity=GRAVITY, clean_boundary=False, penalty=PENALTY, pushing_force=PUSHING_FORCE)
    rids = []
    for b in s["bodies"]:
        c = _rigid_cfg(b)
        rids.append(ref.add_rigid(c.pop("mesh"), **c))
    st = s["state"]
    for gi, mat in enumerate(s["mat_names"]):
        m = st.gid == gi
        ref.add_particles(mat, st.gparams[gi][0], st.gparams[gi][1], st.x[m], st.v[m], st.F[m], st.B[m], st.aux[m], **MAT_KW.get(mat, {}))
    sv = lambda rid, v, w: ref.rigid_set_velocity(rid, v=v, w=w)  # noqa: E731
    _place_bodies(ref, sv, s, rids)
    _presweep(ref, sv, s, rids)
    return ref, rids


# ---------------------------------------------------------------------------------------------- records: what a run hands the model
def body_row(st):
    """a body's state as one row of 33 floats (the layout of mpmhip_rigid_get_state)"""
    return np.concatenate([st["position"], st["rotation"], st["velocity"], st["angular_velocity"], [st["mass"], st["inv_mass"]],
                           np.ravel(st["inertia"]), np.ravel(st["inv_inertia"])]).astype(np.float32)


def body_state(row):
    return dict(position=row[0:3], rotation=row[3:7], velocity=row[7:10], angular_velocity=row[10:13], mass=float(row[13]),
                inv_mass=float(row[14]), inertia=row[15:24].reshape(3, 3), inv_inertia=row[24:33].reshape(3, 3))


def record_reference(refmpm, s):
    """the compiled reference stage by stage on one thread: sort, rasterize_rigid_boundary, gather_cdf, P2G, the grid update, G2P.
    Returns the record (a dict of arrays, what tests/golden/ref_cpic_transfer.npz holds per scene): the colour field — the model's
    input — and the outputs of the three stages."""
    ref, rids = build_reference(refmpm, s)
    bodies = lambda: np.stack([body_row(ref.rigid_state(r)) for r in rids])  # noqa: E731
    ref.sort()
    ref.rasterize_rigid_boundary()
    ref.gather_cdf()
    o = np.argsort(ref.download(by_id=False)["id"], kind="stable")
    pc = ref.particle_cdf()
    words = ref.download_cdf()[0].reshape(-1)
    nz = np.flatnonzero(words)
    rec = dict(cdf_idx=nz.astype(np.int32), cdf_words=words[nz], pstate=pc["states"][o], normal=pc["normal"][o], dist=pc["distance"][o],
               near=pc["near"][o].astype(np.int8), samples=ref.rigid_samples(-1)["pos"], bodies0=bodies())
    ref.p2g()
    g = ref.download_grid()
    nz = np.flatnonzero(g[..., 3].reshape(-1))
    rec.update(grid_idx=nz.astype(np.int32), grid0=g.reshape(-1, 4)[nz], grid0_rest=np.abs(np.delete(g.reshape(-1, 4), nz, 0)).max(),
               bodies1=bodies())
    ref.grid_update()
    rec["grid1"] = ref.download_grid().reshape(-1, 4)[nz]
    ref.g2p()
    p = ref.download(by_id=True)
    rec.update(x=p["x"], v=p["v"], B=p["B"], F=p["F"], aux=p["aux"], bodies2=bodies())
    ref.close()
    return rec


def dense(s, idx, values):
    shape = tuple(r + 1 for r in s["res"]) + values.shape[1:]
    out = np.zeros((int(np.prod(shape[:3])),) + values.shape[1:], values.dtype)
    out[idx] = values
    return out.reshape(shape)


def model_of(s, rec, bodies_key="bodies0"):
    """(transfer_model.Scene, cpic_transfer_model.Cpic) of a scene and a record of its colour field"""
    from tests import cpic_transfer_model as cm
    from tests import transfer_model as tmod
    M = tmod.Scene(s["state"], s["res"], s["dx"], DT, False, gravity=GRAVITY)
    M.name = s["name"]
    bodies = [cm.body_of(body_state(row), (b["friction0"], b["friction1"])) for row, b in zip(rec[bodies_key], s["bodies"])]
    C = cm.Cpic(M, dense(s, rec["cdf_idx"], rec["cdf_words"]), rec["pstate"], rec["normal"], rec["dist"], rec["near"], rec["samples"], bodies,
                PENALTY, PUSHING_FORCE)
    return M, C
