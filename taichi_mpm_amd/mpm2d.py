"""MPM<2> — the reference's 2D simulation (`tc_core.create_simulation2('mpm')`, src/mpm.cpp:983-986) on top of the
mpmhip2d_* entry points of the C ABI (include/mpmhip.h).  Same surface as Simulation3D (taichi_mpm_amd/mpm.py) where it
applies: `initialize`, `add_particles`, `set_levelset`, `step`, `get_current_time`, `get_particles`.  MPM<2> runs the
generic transfer path (src/transfer.cpp:280-283,697-700).  `add_particles(region=...)` fills a LevelSet or a SampledLevelSet2D on
the device from the periodic Poisson-disk tile (include/mpmhip.h: mpmhip2d_seed_particles); `set_levelset` takes shapes or a
SampledBoundary2D — a sampled field with a friction (include/mpmhip.h: mpmhip2d_set_levelset_sdf)."""
import ctypes as C
import os

import numpy as np

from . import _lib
from .materials import MATERIAL_IDS, group_params, initial_aux
from .mpm import DynamicLevelSet, LevelSet, MPMError, Region, _SampledField, check_unsupported_keys, eval_shapes, read_snapshot, snapshot_groups


def lattice_square(lower, higher, dx):
    """4 particles per cell at cell centre +- 0.25 dx (the 2D analogue of the 3D benchmark lattice)"""
    r = np.arange(lower, higher, dtype=np.float64)
    ii, jj = np.meshgrid(r, r, indexing="ij")
    cells = np.stack([ii, jj], -1).reshape(-1, 1, 2) + 0.5
    signs = np.array([[-1, -1], [1, -1], [-1, 1], [1, 1]], np.float64)
    return ((cells + 0.25 * signs[None]) * dx).reshape(-1, 2).astype(np.float32)


class SampledLevelSet2D(_SampledField):
    """A signed-distance field sampled on a regular lattice in the plane: the region of add_particles(region=...) — a disc, a polygon,
    any free-form blob (it stands in for the reference's polygon and image textures).  `phi`: array of shape (res0, res1), world units,
    negative inside; sample (i, j) sits at origin + (i, j) * spacing.  spacing=None: the cell size of the simulation it is given to.
    Read bilinearly; outside the lattice there is no region.  It is a region: a boundary needs a friction, which as_boundary() adds
    (set_levelset takes the SampledBoundary2D it returns, not this)."""

    _DIM, _NAME, _COUNT = 2, "SampledLevelSet2D", "two"

    def __init__(self, phi, origin=(0.0, 0.0), spacing=None):
        self._set_field(phi, origin, spacing)

    @staticmethod
    def _coords(origin):
        return [float(origin[k]) for k in range(2)]

    @staticmethod
    def _origin(origin):
        o = tuple(float(v) for v in origin)
        if len(o) != 2 or not np.all(np.isfinite(o)):
            raise MPMError("SampledLevelSet2D: origin must be two finite numbers, got %r" % (origin,))
        return o

    @classmethod
    def from_function(cls, f, res, origin=(0.0, 0.0), spacing=None):
        """sample f, which maps an (n, 2) array of world positions to n values of phi"""
        return cls(cls._sample(f, res, origin, spacing), origin, spacing)

    @staticmethod
    def polygon_distance(vertices, pts):
        """signed distance (float64, negative inside) of the points pts (n, 2) to the simple closed polygon `vertices` (m, 2), in
        either orientation: the distance to the nearest edge, the sign from the even-odd rule (a ray towards +x; an end point AT the
        ray's height counts as below, so a vertex is crossed once)"""
        v = np.asarray(vertices, np.float64).reshape(-1, 2)
        if len(v) < 3 or not np.all(np.isfinite(v)):
            raise MPMError("SampledLevelSet2D: a polygon needs at least 3 finite vertices")
        p = np.asarray(pts, np.float64).reshape(-1, 2)
        a, b = v, np.roll(v, -1, axis=0)
        e = b - a
        ee = np.maximum((e * e).sum(axis=1), 1e-300)
        d2 = np.full(len(p), np.inf)
        odd = np.zeros(len(p), bool)
        for k in range(len(v)):
            w = p - a[k]
            t = np.clip((w @ e[k]) / ee[k], 0.0, 1.0)
            r = w - t[:, None] * e[k]
            d2 = np.minimum(d2, (r * r).sum(axis=1))
            up_a, up_b = a[k, 1] > p[:, 1], b[k, 1] > p[:, 1]
            cross = up_a != up_b
            with np.errstate(divide="ignore", invalid="ignore"):
                xc = a[k, 0] + (p[:, 1] - a[k, 1]) * (e[k, 0] / e[k, 1])
            odd ^= cross & (p[:, 0] < xc)
        return np.where(odd, -1.0, 1.0) * np.sqrt(d2)

    @classmethod
    def from_polygon(cls, vertices, res, origin=(0.0, 0.0), spacing=None):
        """bake the signed distance of a simple closed polygon, vertices (m, 2) in world units"""
        return cls.from_function(lambda x: cls.polygon_distance(vertices, x), res, origin, spacing)

    @classmethod
    def from_levelset(cls, ls, res, origin=(0.0, 0.0), spacing=None):
        """bake an analytic LevelSet's shapes read in the plane (z = 0, a cuboid unbounded along z: as mpmhip2d_set_levelset reads
        them), in float64"""
        if not ls.shapes:
            raise MPMError("SampledLevelSet2D.from_levelset: the LevelSet has no shapes")
        if spacing is None:
            spacing = ls.delta_x
        shapes = []
        for t_, io, p in ls.shapes:
            p = list(p)
            if t_ == 2:
                p[2], p[5] = -1e30, 1e30
            else:
                p[2] = 0.0
            shapes.append((t_, io, p))
        return cls.from_function(lambda x: eval_shapes(shapes, np.concatenate([x, np.zeros((len(x), 1))], axis=1)), res, origin, spacing)

    def as_boundary(self, friction=-1.0):
        """this field as a boundary for Simulation2D.set_levelset: the same phi, origin and spacing, and a friction code"""
        return SampledBoundary2D(self.phi, self.origin, self.spacing, friction)


class SampledBoundary2D(SampledLevelSet2D):
    """A sampled field as the BOUNDARY of the 2D simulation (include/mpmhip.h: mpmhip2d_set_levelset_sdf): a SampledLevelSet2D plus
    the friction code a boundary needs (LevelSet's: -1 sticky, -2 slip, >= 0 Coulomb).  spacing=None resolves to the simulation's
    delta_x when it is installed.  Two of one lattice make the key frames of a DynamicLevelSet."""

    sampled_key_frame = True  # (DynamicLevelSet.initialize: mixes with shapes and other lattices are refused)

    def __init__(self, phi, origin=(0.0, 0.0), spacing=None, friction=-1.0):
        super().__init__(phi, origin, spacing)
        self.friction = float(friction)

    def set_friction(self, f):
        self.friction = float(f)
        return self


class Simulation2D:
    def __init__(self):
        self._L = _lib.load()
        self._ctx = None
        self._staged = []
        self._groups = []
        self._levelset = None
        self._n_added = 0
        self.frame = 0
        self._rigids = []  # ctypes keep-alives of the rigid bodies' configs / script callbacks

    def initialize(self, config):
        cfg = dict(config)
        if "delta_t" in cfg:  # src/mpm.cpp:41-42
            raise MPMError("Please use 'base_delta_t' instead of 'delta_t'")
        check_unsupported_keys(cfg)
        if cfg.get("rigid_body_collision", False):  # RigidSolver<2>::detect_rigid_collision is TC_NOT_IMPLEMENTED (src/rigid_body_solver.h:154-158)
            raise MPMError("rigid_body_collision=True is not implemented by the 2D simulation (nor by the reference's: "
                           "src/rigid_body_solver.h:154-158); leave the key out or set it to False")
        for k in ("benchmark_rasterize", "benchmark_resample"):  # (built for the 3D simulation only)
            if cfg.get(k, False):
                raise MPMError("config key %r (src/mpm.cpp:516-538, 554-561) is not implemented by the 2D simulation" % k)
        res = cfg["res"]
        res = (int(res),) * 2 if np.isscalar(res) else tuple(int(r) for r in res)
        if len(res) != 2:
            raise MPMError("Simulation2D needs a 2-entry res")
        self.res = res
        self.delta_x = float(cfg.get("delta_x", 1.0 / res[0]))
        self.base_delta_t = float(cfg.get("base_delta_t", 1e-4)) * float(cfg.get("dt_multiplier", 1.0))
        g = cfg.get("gravity", (0.0, -10.0))
        self.gravity = (float(g[0]), float(g[1]))
        self.config = cfg
        self.max_particles = int(cfg.get("max_particles", 0))
        self.verbose_bgeo = bool(cfg.get("verbose_bgeo", False))  # src/visualize.cpp:22
        self.frame_directory = cfg.get("frame_directory")  # injected by the python driver, async_mpm.py:49
        self.frame_count = 0
        # bitwise reproducible runs (include/mpmhip.h: mpmhip2d_config.deterministic): cell sort + gather P2G instead of float atomics
        self.deterministic = bool(cfg.get("deterministic", False))
        return self

    def _check(self, rc):
        if rc < 0:
            raise MPMError("libmpmhip error %d: %s" % (rc, self._L.mpmhip2d_last_error(self._ctx).decode()))
        return rc

    def _ensure_ctx(self, extra=0):
        if self._ctx is not None:
            if self._resident_particles() + extra > self._capacity:
                raise MPMError("2D particle capacity exceeded: pass max_particles to initialize()")
            return
        cfg = self.config
        c = _lib.Config2D()
        c.res[:] = self.res
        c.dx, c.dt = self.delta_x, self.base_delta_t
        c.gravity[:] = self.gravity
        c.particle_gravity = int(bool(cfg.get("particle_gravity", True)))
        c.apic_damping, c.rpic_damping = float(cfg.get("apic_damping", 0.0)), float(cfg.get("rpic_damping", 0.0))
        c.clean_boundary = int(bool(cfg.get("clean_boundary", True)))
        c.particle_collision = int(bool(cfg.get("particle_collision", False)))
        self._capacity = max(self.max_particles, int((self._n_added + extra) * 1.5) + 1024)
        c.max_particles = self._capacity
        c.device = int(cfg.get("device", 0))
        c.deterministic = int(self.deterministic)
        ctx = C.c_void_p()
        rc = self._L.mpmhip2d_create(C.byref(c), C.byref(ctx))
        if rc != 0:
            raise MPMError("mpmhip2d_create failed (%d): %s" % (rc, self._L.mpmhip2d_last_error(None).decode()))
        self._ctx = ctx
        self._check(self._L.mpmhip2d_set_rigid_coupling(ctx, float(cfg.get("penalty", 0.0)), float(cfg.get("pushing_force", 20000.0))))
        self._check(self._L.mpmhip2d_set_articulation_iterations(ctx, int(cfg.get("articulation_iterations", 100))))  # src/mpm.h:279-280
        self._check(self._L.mpmhip2d_set_rigid_levelset_collision(ctx, int(bool(cfg.get("rigid_body_levelset_collision", False)))))  # src/mpm.cpp:535-538
        d = float(cfg.get("dirichlet_boundary_radius", 0.0))  # src/mpm.cpp:541-544 -> apply_dirichlet_boundary_conditions, :374-399
        vel = float(cfg.get("dirichlet_boundary_velocity", 0.0))
        self._check(self._L.mpmhip2d_set_dirichlet(ctx, int(d > 0.0), float(cfg.get("dirichlet_distance_left", d)), float(cfg.get("dirichlet_distance_right", d)),
                                                   float(cfg.get("dirichlet_boundary_left", vel)), float(cfg.get("dirichlet_boundary_right", vel))))
        self._apply_levelset()
        for gi, (mat, params, arrs) in enumerate(self._staged):
            self._add(mat, params, *arrs)
        self._staged = []

    def _resident_particles(self):
        """particles held by the object's arrays (what max_particles bounds)"""
        return self._n_added

    def close(self):
        if self._ctx is not None:
            self._L.mpmhip2d_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _add(self, mat, params, x, v, F, B, aux):
        fp = C.POINTER(C.c_float)
        gi = self._check(self._L.mpmhip2d_add_group(self._ctx, mat, params.ctypes.data_as(fp)))
        keep = []

        def ptr(a, w):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32).reshape(len(x), w) if w > 1 else np.ascontiguousarray(a, np.float32).reshape(len(x))
            keep.append(a)
            return a.ctypes.data_as(fp)
        self._check(self._L.mpmhip2d_add_particles(self._ctx, gi, len(x), ptr(x, 2), ptr(v, 2), ptr(F, 4), ptr(B, 4), ptr(aux, 1)))

    def add_particles(self, config):
        """MPM<2>::add_particles (src/mpm.cpp:77-270) with explicit `positions=` (n, 2), a `square=(lo, hi)` lattice, or `region=` —
        a LevelSet or SampledLevelSet2D filled on the device from the periodic Poisson-disk tile (_seed_region)"""
        cfg = dict(config)
        ptype = cfg.get("type")
        if ptype == "rigid":  # src/mpm.cpp:80-83
            return str(self.add_rigid_body(cfg))
        if ptype not in MATERIAL_IDS:
            raise MPMError("unknown particle type %r" % (ptype,))
        dx = self.delta_x
        maximum = float(cfg.get("ppc", cfg.get("maximum", 4)))
        if "region" in cfg:
            return self._seed_region(cfg, ptype, maximum)
        if "square" in cfg:
            x = lattice_square(int(cfg["square"][0]), int(cfg["square"][1]), dx)
        elif "positions" in cfg:
            x = np.ascontiguousarray(cfg["positions"], np.float32).reshape(-1, 2)
        else:
            raise MPMError("add_particles needs positions=, square=(lo, hi) or region=")
        X = x.astype(np.float64) / dx
        keep = ~((X.min(1) < 7.0) | ((X - np.asarray(self.res)).max(1) > -7.0))  # src/mpm.cpp:129-132
        x = x[keep]
        n = len(x)
        vol = dx ** 2 / maximum  # pow<dim>(delta_x) / maximum, src/mpm.cpp:134
        mass = vol * float(cfg.get("density", 400.0))
        params, mat = group_params(ptype, mass, vol, **{k: v for k, v in cfg.items() if isinstance(v, (int, float))})
        if "params" in cfg:
            params = np.ascontiguousarray(cfg["params"], np.float32).reshape(16).copy()

        def sel(key, w, default):
            if key in cfg:
                a = np.ascontiguousarray(cfg[key], np.float32)
                return (a.reshape(-1, w) if w > 1 else a.reshape(-1))[keep]
            return default
        v = sel("velocities", 2, None)
        F = sel("F", 4, None)
        B = sel("B", 4, None)
        aux = sel("aux", 1, np.full(n, initial_aux(ptype, **cfg), np.float32))
        if self._ctx is None:
            self._staged.append((mat, params, (x, v, F, B, aux)))
        else:
            self._ensure_ctx(extra=n)
            self._add(mat, params, x, v, F, B, aux)
        self._groups.append((mat, params))
        self._n_added += n
        return ""

    def _seed_desc(self, cfg, ptype, ppc):
        """the mpmhip2d_seed_desc of an add_particles(region=...) config, and the objects its pointers need alive"""
        region, dx = cfg["region"], self.delta_x
        if not (np.isfinite(ppc) and ppc > 0):
            raise MPMError("add_particles(region=): ppc must be a finite number > 0, got %r" % (ppc,))
        for k in ("velocities", "F", "B", "aux", "pd_packed", "point_cloud"):
            if k in cfg and cfg[k] is not False:
                raise MPMError("add_particles(region=) does not take %r" % k)
        if not cfg.get("pd", True) or not cfg.get("pd_periodic", True):
            raise MPMError("add_particles(region=) implements the periodic Poisson-disk tile only (pd and pd_periodic must stay True)")
        if initial_aux(ptype, **cfg) != initial_aux(ptype):
            raise MPMError("add_particles(region=) gives every particle the material's default state")
        d = _lib.SeedDesc2D()
        keep = []
        if isinstance(region, SampledLevelSet2D):
            sd = _lib.SdfDesc2D()
            sd.res[:] = region.res
            sd.origin[:] = region.origin
            sd.spacing = dx if region.spacing is None else region.spacing
            keep += [sd, region.phi]
            d.sdf = C.pointer(sd)
            d.phi = region.phi.ctypes.data_as(C.POINTER(C.c_float))
        elif isinstance(region, LevelSet):
            d.n_shapes = len(region.shapes)
            for i, (t_, io, p) in enumerate(region.shapes):
                d.shapes[i].type, d.shapes[i].inside_out = t_, io
                d.shapes[i].p[:] = p
        elif not isinstance(region, Region):  # (an expression travels beside the description: _seed_region)
            raise MPMError("add_particles(region=) takes a LevelSet or a SampledLevelSet2D, or a Region over them, got %r" % type(region).__name__)
        d.ppc = ppc
        v0 = cfg.get("initial_velocity", (0.0, 0.0))
        d.velocity[:] = (float(v0[0]), float(v0[1]))
        d.source = int(bool(cfg.get("pd_source", False)))
        d.source_delta_t = float(cfg.get("delta_t", 1e-3))  # src/mpm.cpp:224
        d.initial_dg = float(cfg.get("initial_dg", 1.0))  # src/particles.h:120
        return d, keep

    def _seed_region(self, cfg, ptype, ppc):
        """add_particles(region=...): the reference's default fill, add_particles(density_tex=...) with the periodic Poisson-disk
        tile (src/mpm.cpp:205-251), on the device (include/mpmhip.h: mpmhip2d_seed_particles).  region: a LevelSet (where its shapes,
        read in the plane, are negative), a SampledLevelSet2D, or a Region expression over these
        (mpmhip2d_seed_particles_region).  Keys: ppc (4), initial_velocity, pd_source, delta_t (1e-3), initial_dg, density and the
        material keys."""
        dx = self.delta_x
        d, keep = self._seed_desc(cfg, ptype, ppc)
        if isinstance(cfg["region"], Region):
            rd, rkeep = cfg["region"].compile(2, dx)  # (no mesh leaf in the plane: nothing is voxelised)
            seed = lambda: self._L.mpmhip2d_seed_particles_region(self._ctx, gi, C.byref(d), C.byref(rd), C.byref(n))
        else:
            seed = lambda: self._L.mpmhip2d_seed_particles(self._ctx, gi, C.byref(d), C.byref(n))
        vol = dx ** 2 / ppc  # pow<dim>(delta_x) / maximum, src/mpm.cpp:134
        mass = vol * float(cfg.get("density", 400.0))
        params, mat = group_params(ptype, mass, vol, **{k: v for k, v in cfg.items() if isinstance(v, (int, float))})
        if "params" in cfg:
            params = np.ascontiguousarray(cfg["params"], np.float32).reshape(16).copy()
        self._ensure_ctx()  # (particles staged before the ctx existed are uploaded first: creation ids follow call order)
        # an emitter calls before every frame with one material: its particles share a group row (a ctx holds 64 of them)
        gi = next((i for i, (m_, p_) in enumerate(self._groups) if m_ == mat and p_.tobytes() == params.tobytes()), len(self._groups))
        if gi == len(self._groups):
            self._groups.append((mat, params))
            self._check(self._L.mpmhip2d_add_group(self._ctx, mat, params.ctypes.data_as(C.POINTER(C.c_float))))
        n = C.c_int64(0)
        rc = seed()
        if rc == -4:  # MPMHIP_ECAPACITY: n is what the call needs; nothing was written
            cap = max(int((int(self._L.mpmhip2d_num_slots(self._ctx)) + n.value) * 1.5), self.max_particles)
            self._check(self._L.mpmhip2d_reserve(self._ctx, cap))
            self._capacity = int(self._L.mpmhip2d_capacity(self._ctx))  # (what the library has: it may give more than it was asked for)
            rc = seed()
        self._check(rc)
        self._n_added += n.value
        return ""

    def set_levelset(self, levelset):
        """a LevelSet (shapes), a SampledBoundary2D, or a DynamicLevelSet whose two key frames are of one of these kinds"""
        if isinstance(levelset, SampledLevelSet2D) and not isinstance(levelset, SampledBoundary2D):
            raise MPMError("set_levelset: a SampledLevelSet2D is a region for add_particles(region=...) only; a boundary needs a "
                           "friction: pass region.as_boundary(friction=...)")
        if isinstance(levelset, DynamicLevelSet):
            s0, s1 = (isinstance(l, SampledBoundary2D) for l in (levelset.levelset0, levelset.levelset1))
            if s0 != s1:
                raise MPMError("set_levelset: a sampled and an analytic key frame cannot be mixed")
            if s0 and not levelset.levelset0.same_lattice(levelset.levelset1):
                raise MPMError("set_levelset: the two sampled key frames must share one lattice (res, origin, spacing)")
            if not s0 and not all(isinstance(l, LevelSet) for l in (levelset.levelset0, levelset.levelset1)):
                raise MPMError("set_levelset: the key frames of a 2D DynamicLevelSet are LevelSets or SampledBoundary2D")
        sampled = isinstance(levelset, SampledBoundary2D) or (isinstance(levelset, DynamicLevelSet) and isinstance(levelset.levelset0, SampledBoundary2D))
        if sampled and getattr(self, "config", {}).get("rigid_body_levelset_collision", False):
            raise MPMError("rigid_body_levelset_collision is not supported with a sampled level set")
        self._levelset = levelset
        if self._ctx is not None:
            self._apply_levelset()

    @staticmethod
    def _shapes(ls):
        arr = (_lib.Shape * max(len(ls.shapes), 1))()
        for i, (t_, io, p) in enumerate(ls.shapes):
            arr[i].type, arr[i].inside_out = t_, io
            arr[i].p[:] = p
        return arr

    def _apply_levelset(self):
        ls = self._levelset
        if ls is None:
            return
        if isinstance(ls, DynamicLevelSet):
            l0, l1 = ls.levelset0, ls.levelset1
            if isinstance(l0, SampledBoundary2D):
                self._set_sdf(l0, l1, ls.t0, ls.t1)
                return
            self._check(self._L.mpmhip2d_set_levelset(self._ctx, len(l0.shapes), self._shapes(l0), len(l1.shapes), self._shapes(l1),
                                                      ls.t0, ls.t1, l0.friction))
        elif isinstance(ls, SampledBoundary2D):
            self._set_sdf(ls, None, 0.0, 1.0)
        else:
            self._check(self._L.mpmhip2d_set_levelset(self._ctx, len(ls.shapes), self._shapes(ls), -1, None, 0.0, 1.0, ls.friction))

    def _set_sdf(self, l0, l1, t0, t1):
        d = _lib.SdfDesc2D()
        d.res[:] = l0.res
        d.origin[:] = l0.origin
        d.spacing = l0.spacing if l0.spacing is not None else self.delta_x
        fp = C.POINTER(C.c_float)
        self._check(self._L.mpmhip2d_set_levelset_sdf(self._ctx, C.byref(d), l0.phi.ctypes.data_as(fp),
                                                      l1.phi.ctypes.data_as(fp) if l1 is not None else None, t0, t1, l0.friction))

    def sample_levelset(self, x, t=0.0):
        """the device's evaluation of the installed level set (sampled or shapes) at positions (n, 2) at time t:
        (phi in grid units, unit gradient (n, 2), d phi / dt, hit) — hit is False where there is no level set"""
        self._ensure_ctx()
        x = np.ascontiguousarray(x, np.float32).reshape(-1, 2)
        n = len(x)
        phi, grad, dphidt, hit = np.zeros(n, np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        if n:
            fp = C.POINTER(C.c_float)
            self._check(self._L.mpmhip2d_debug_levelset_sample(self._ctx, n, x.ctypes.data_as(fp), float(t), phi.ctypes.data_as(fp),
                                                               grad.ctypes.data_as(fp), dphidt.ctypes.data_as(fp),
                                                               hit.ctypes.data_as(C.POINTER(C.c_int32))))
        return phi, grad, dphidt, hit.astype(bool)

    def step(self, dt):
        self._ensure_ctx()
        self._check(self._L.mpmhip2d_step(self._ctx, float(dt)))

    def substep(self):
        self._ensure_ctx()
        self._check(self._L.mpmhip2d_substep(self._ctx))

    def run_substeps(self, n):
        for _ in range(int(n)):
            self.substep()

    def synchronize(self):
        self.get_num_particles()

    def set_deterministic(self, on=True):
        """config key `deterministic` of a live simulation, from the next substep on (include/mpmhip.h: mpmhip2d_set_deterministic)"""
        self.deterministic = bool(on)
        if self._ctx is not None:
            self._check(self._L.mpmhip2d_set_deterministic(self._ctx, int(self.deterministic)))

    def upload_ids(self, ids):
        """creation ids of the resident slots, in slot order (include/mpmhip.h: mpmhip2d_upload_ids): a scene added in another
        order keeps its particles' names, which is what the deterministic mode orders a cell by"""
        self._ensure_ctx()
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        self._check(self._L.mpmhip2d_upload_ids(self._ctx, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32))))

    def get_current_time(self):
        return self._L.mpmhip2d_current_time(self._ctx) if self._ctx is not None else 0.0

    # ---------------------------------------------------------------- CPIC rigid bodies (segments)
    def add_rigid_body(self, cfg):
        """MPM<2>::add_rigid_particle (src/mpm_rigid_body.cpp:130-252, dim = 2): mesh=(n, 2, 2) segments; keys as in 3D
        (codimensional is mandatory; initial_rotation / scripted_rotation are one angle in degrees)"""
        if "codimensional" not in cfg:
            raise MPMError("rigid bodies need the key 'codimensional'")
        if "scripted_position" not in cfg and "initial_position" not in cfg:
            raise MPMError("Please specify one (and only one) of 'scripted_position' and 'initial_position'.")
        seg = np.ascontiguousarray(cfg["mesh"], np.float32).reshape(-1, 4)
        r = _lib.RigidConfig2D()
        r.codimensional = int(bool(cfg["codimensional"]))
        r.recenter = int(bool(cfg.get("recenter", True)))
        r.reverse_vertices = int(bool(cfg.get("reverse_vertices", False)))
        r.density = float(cfg.get("density", 0.0))
        f0, f1 = (cfg["friction"],) * 2 if "friction" in cfg else (cfg.get("friction0", 0.0), cfg.get("friction1", 0.0))
        r.friction[:] = (float(f0), float(f1))
        r.restitution = float(cfg.get("restitution", 0.0))
        sc = cfg.get("scale", (1.0, 1.0))
        r.scale[:] = (float(sc[0]), float(sc[1]))
        p0 = cfg.get("initial_position", (0.0, 0.0))
        r.initial_position[:] = (float(p0[0]), float(p0[1]))
        r.initial_rotation = float(cfg.get("initial_rotation", 0.0))
        v0 = cfg.get("initial_velocity", (0.0, 0.0))
        r.initial_velocity[:] = (float(v0[0]), float(v0[1]))
        r.initial_angular_velocity = float(cfg.get("initial_angular_velocity", 0.0))
        r.linear_damping = float(cfg.get("linear_damping", 0.0))
        r.angular_damping = float(cfg.get("angular_damping", 0.0))
        if cfg.get("scripted_position") is not None:
            fn = cfg["scripted_position"]

            def pos(_u, t, out, fn=fn):
                v = fn(float(t))
                out[0], out[1] = float(v[0]), float(v[1])
            r.scripted_position = _lib.SCRIPT_FN(pos)
        if cfg.get("scripted_rotation") is not None:
            gn = cfg["scripted_rotation"]

            def rot(_u, t, out, gn=gn):
                out[0] = float(gn(float(t)))
            r.scripted_rotation = _lib.SCRIPT_FN(rot)
        self._ensure_ctx()
        rid = self._check(self._L.mpmhip2d_add_rigid_body(self._ctx, C.byref(r), len(seg), seg.ctypes.data_as(C.POINTER(C.c_float))))
        self._rigids.append(r)
        return rid

    def get_rigid_state(self, rid):
        """position 2, angle (radians), velocity 2, angular velocity, mass, inv_mass, inertia, inv_inertia"""
        o = np.zeros(10, np.float32)
        self._check(self._L.mpmhip2d_rigid_get_state(self._ctx, int(rid), o.ctypes.data_as(C.POINTER(C.c_float))))
        return o

    def get_rigid_samples(self, rid=-1):
        n = self._check(self._L.mpmhip2d_rigid_get_samples(self._ctx, int(rid), 0, None))
        pos = np.zeros((n, 2), np.float32)
        if n:
            self._check(self._L.mpmhip2d_rigid_get_samples(self._ctx, int(rid), n, pos.ctypes.data_as(C.POINTER(C.c_float))))
        return pos

    def get_rigid_mesh(self, rid):
        """the body's segments in world space, (n, 2, 2)"""
        fp = C.POINTER(C.c_float)
        n = self._check(self._L.mpmhip2d_rigid_get_mesh(self._ctx, int(rid), 0, None))
        seg = np.zeros((n, 2, 2), np.float32)
        if n:
            self._check(self._L.mpmhip2d_rigid_get_mesh(self._ctx, int(rid), n, seg.ctypes.data_as(fp)))
        return seg

    def write_rigid_body(self, rid, file_name):
        """MPM<2>::write_rigid_body (src/visualize.cpp:105-130): `file_name`.poly — POINTS, POLYS (one per segment), END"""
        seg = self.get_rigid_mesh(rid).reshape(-1, 2)
        with open(file_name + ".poly", "w") as f:
            f.write("POINTS\n")
            for i, v in enumerate(seg):
                f.write("%d: %.9g %.9g 0.0\n" % (i + 1, v[0], v[1]))
            f.write("POLYS\n")
            for i in range(1, len(seg) // 2 + 1):
                f.write("%d: %d %d\n" % (i, 2 * i - 1, 2 * i))
            f.write("END\n")
        return file_name + ".poly"

    def cdf_phase(self):
        """rasterize_rigid_boundary + gather_cdf as one phase (parity tests; substep() runs them itself)"""
        self._ensure_ctx(); self._check(self._L.mpmhip2d_cdf_phase(self._ctx))

    def download_cdf(self):
        shp = tuple(r + 1 for r in self.res)
        st, d = np.zeros(shp, np.uint32), np.zeros(shp, np.float32)
        self._check(self._L.mpmhip2d_download_cdf(self._ctx, st.ctypes.data_as(C.POINTER(C.c_uint32)), d.ctypes.data_as(C.POINTER(C.c_float))))
        return st, d

    def download_colours(self):
        """per live particle in slot order: states, boundary distance, normal, near flag"""
        n = self.get_num_particles()
        st, d, nr, near = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
        fp = C.POINTER(C.c_float)
        got = self._check(self._L.mpmhip2d_download_colours(self._ctx, n, st.ctypes.data_as(C.POINTER(C.c_uint32)), d.ctypes.data_as(fp),
                                                            nr.ctypes.data_as(fp), near.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(states=st[:got], distance=d[:got], normal=nr[:got], near=near[:got])

    def get_num_particles(self):
        if self._ctx is None:
            return self._n_added
        return int(self._check(self._L.mpmhip2d_num_particles(self._ctx)))

    def get_particles(self, sort_by_id=True):
        self._ensure_ctx()
        n = self.get_num_particles()
        out = dict(x=np.zeros((n, 2), np.float32), v=np.zeros((n, 2), np.float32), F=np.zeros((n, 4), np.float32),
                   B=np.zeros((n, 4), np.float32), aux=np.zeros(n, np.float32), gid=np.zeros(n, np.int32), id=np.zeros(n, np.int32))
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        got = self._check(self._L.mpmhip2d_download(self._ctx, n, out["x"].ctypes.data_as(fp), out["v"].ctypes.data_as(fp),
                                                    out["F"].ctypes.data_as(fp), out["B"].ctypes.data_as(fp), out["aux"].ctypes.data_as(fp),
                                                    out["gid"].ctypes.data_as(ip), out["id"].ctypes.data_as(ip)))
        out = {k: a[:got] for k, a in out.items()}
        if sort_by_id:
            o = np.argsort(out["id"], kind="stable")
            out = {k: a[o] for k, a in out.items()}
        return out

    def get_grid(self):
        self._ensure_ctx()
        g = np.zeros((self.res[0] + 1, self.res[1] + 1, 3), np.float32)
        self._check(self._L.mpmhip2d_download_grid(self._ctx, g.ctypes.data_as(C.POINTER(C.c_float))))
        return g

    def test(self):
        return True

    def get_name(self):
        return "mpm"

    def get_mpi_world_rank(self):
        return 0

    def get_debug_information(self):  # src/mpm.cpp:635-639
        return ""

    def get_vis_resolution(self):  # (scripts/async/async_mpm.py:79-81; see Simulation3D.get_vis_resolution)
        import types
        return types.SimpleNamespace(x=int(self.res[0]), y=int(self.res[1]))

    def add_articulation(self, cfg):
        """general_action(action='add_articulation', type='rotation', obj0=, obj1=) (src/mpm.cpp:923-933; the joint of
        scripts/mls-cpic/sand_wheel_2D.py:88): both bodies share one angular velocity.  The other joint types are 3D only."""
        if cfg.get("type") != "rotation":
            raise MPMError("add_articulation(type=%r): only 'rotation' is built for 2D simulations" % (cfg.get("type"),))
        if "obj0" not in cfg:
            raise MPMError("add_articulation needs 'obj0'")
        j = _lib.JointConfig()
        j.type, j.obj0, j.obj1 = 0, int(cfg["obj0"]), int(cfg.get("obj1", 0))
        self._ensure_ctx()
        self._check(self._L.mpmhip2d_add_articulation(self._ctx, C.byref(j)))
        return ""

    def general_action(self, config):
        """MPM<2>::general_action, src/mpm.cpp:920-978"""
        action = config.get("action")
        if action == "add_articulation":
            return self.add_articulation(config)
        if action == "save":  # src/mpm.cpp:940-949: whole-state snapshot
            self.save_snapshot(config["file_name"])
            return ""
        if action == "load":  # src/mpm.cpp:950-960
            self.load_snapshot(config["file_name"])
            return ""
        if action == "delete_particles_inside_level_set":  # src/mpm.cpp:962-974
            self._ensure_ctx()
            n = C.c_int64(0)
            self._check(self._L.mpmhip2d_delete_particles_inside_level_set(self._ctx, C.byref(n)))
            return ""
        raise MPMError("general_action(%r) is not part of the 2D build" % (action,))

    def save_snapshot(self, path):
        """groups, particles, clocks, the rigid bodies' records and joints, an asynchronous stepper's pools and block table
        (include/mpmhip.h: mpmhip2d_snapshot_save)"""
        self._ensure_ctx()
        n = int(self._check(self._L.mpmhip2d_snapshot_size(self._ctx)))
        buf = np.empty(max(n, 1), np.uint8)
        self._check(self._L.mpmhip2d_snapshot_save(self._ctx, buf.ctypes.data_as(C.c_void_p), n))
        with open(path, "wb") as f:
            f.write(np.array([self.frame, self.frame_count], np.int64).tobytes())
            f.write(buf[:n].tobytes())

    def load_snapshot(self, path):
        """into a simulation set up with the same grid and scene (level set, configuration, the rigid bodies — added before the
        load — come from the script, as in the reference); replaces all particles and groups"""
        (self.frame, self.frame_count), blob, h = read_snapshot(path, _lib.Snap2DHeader, frame_words=2)
        self._ensure_ctx()
        self._check(self._L.mpmhip2d_snapshot_load(self._ctx, blob.ctypes.data_as(C.c_void_p), len(blob)))
        self._groups = snapshot_groups(blob, h)
        self._staged = []
        self._n_added = max(self._n_added, int(h.n))

    def write_partio(self, file_name):
        """MPM<2>::write_partio (src/visualize.cpp:17-100): the same Houdini .bgeo as the 3D simulation writes, z = 0
        (include/mpmhip.h: mpmhip2d_write_bgeo)"""
        self._ensure_ctx()
        self._check(self._L.mpmhip2d_write_bgeo(self._ctx, os.fsencode(file_name), int(self.verbose_bgeo)))

    def bgeo_bytes(self, verbose=None):
        """the .bgeo image of the current state as bytes (no file)"""
        self._ensure_ctx()
        verbose = int(self.verbose_bgeo if verbose is None else verbose)
        n = C.c_size_t()
        self._check(self._L.mpmhip2d_bgeo_size(self._ctx, verbose, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        w = C.c_size_t()
        self._check(self._L.mpmhip2d_bgeo_encode(self._ctx, verbose, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(w)))
        return buf[:w.value].tobytes()

    def visualize(self):
        """MPM<2>::visualize -> write_bgeo (src/visualize.cpp:156-159, src/mpm.h:333-343): the next `frame_directory/%04d.bgeo`
        (frame numbers start at 1) and every rigid body's outline next to it"""
        if not self.frame_directory:
            raise MPMError("visualize() needs the config key 'frame_directory'")
        self.frame_count += 1
        os.makedirs(self.frame_directory, exist_ok=True)
        path = os.path.join(self.frame_directory, "%04d.bgeo" % self.frame_count)
        self.write_partio(path)
        for rid in range(1, len(self._rigids) + 1):
            self.write_rigid_body(rid, os.path.join(self.frame_directory, "rigid_%03d_%04d" % (rid, self.frame_count)))
        return path
