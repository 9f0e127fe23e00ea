"""A float64 model of the three transfer stages (P2G, grid update, G2P) of one substep that returns, beside every value, the bound
a fp32 implementation of the same stage is held to — TEST INFRASTRUCTURE ONLY.  Plain numpy, written from the maths (as
oracle/np_mpm.py is, which it is checked against in tests/test_transfer_model_cpu.py); the inputs are the fp32 arrays the device is
given, widened: idx is the device's fp32 1/dx, the base node of a stencil and the deleted set are the ones tests/common.py: sort_key
decides in fp32.

THE BOUND.  With u = 2^-24 (half an ulp, relative) a device value is held to

    u * (K + N - 1) * (sum of the absolute contributions)  +  u * (position term)  +  (stress term),

K = the fp32 roundings one contribution goes through (counted below from csrc/k_p2g.h, k_grid.h, k_g2p.h, k_particles.h), N = the
number of contributions summed into the value: any order of summing N terms is off by at most (N - 1) u (sum of |terms|), so the
bound holds for the tiles of k_p2g as for the plain loop of the CPU oracle (first order in u throughout).

POSITION TERM.  The kernels take fx = x * idx - base in fp32: off by |dfx| <= u |X| (one rounding of X = x * idx, or of the fused
form; the subtraction of the integer is exact).  The weights are quadratics of fx with |dw/dfx| <= 1 per axis, evaluated by
mpm_math.h: bspline_weights — w0 = fma(.5, t0 t0, fma(-1.5, t0, 1.125)) and its mirror for w2, w1 = fma(-1, t1 t1, .75) — whose
intermediate values reach 2.25 / 2 and 1.125 while the weight itself may be 0: the roundings are ABSOLUTE, (1.125 + 1.125 + 0.5) u
for w0 / w2 plus u for t2 = p - 1.5 (the one inexact shift), 4 u at the most.  So per axis |dw_a| <= u (|X_a| + 4) =: u PW_a, and a
node's weight w = w_x w_y w_z is off by  u sum_a PW_a prod_{b != a} w_b  (+ two relative roundings of the product, in K).  The offset
d = fx - (i, j, k) that multiplies the affine matrix is off by u |X| per axis.

STRESS TERM.  The affine matrix A = stress * S + 4 m B (S = -4 idx dt) holds the stress the device evaluates in fp32, which
tests/test_gpu_ref.py holds to 3e-5 max|stress| + 2 mu vol 4e-6 (the F - R cancellation); times |S| that is the error of an entry of
A, and it reaches a node through |w| sum_a |d_a|.  It vanishes where the stress is exactly 0 (F = I): there the bound is pure
transfer arithmetic."""
import numpy as np

from oracle import np_mpm
from tests.common import sort_key

U = 2.0 ** -24
W_ABS = 4.0      # absolute roundings of one axis weight, in u (above)
STRESS_REL = 3e-5
STRESS_ABS = 4e-6  # times 2 mu vol

# K of one P2G contribution w * (m v + A d) to a momentum sum (k_p2g.h: p2g_particle; k_particles.h: k_affine / k_g2p.h for A):
#   v + g dt (fma) 1;  m * v 1;  A: b * m4 and the fma onto it 2 (m4 = 4 m is exact);  node (0,0,0): three fma onto m v 3;
#   the walk to node (i,j,k): up to two subtractions of a column of A per axis 6;  w0 * w1, * w2 2;  the fma into the cell's sum 1.
# Every intermediate is at most m |v| + sum_a |A_ca| * 1.5 in magnitude (|d_a| <= 1.5 on the whole stencil): that is the absolute
# contribution the roundings are relative to.
K_P2G_MOM = 1 + 1 + 2 + 3 + 6 + 2 + 1
# mass: w0 * w1, * w2 2;  the fma 1 (the walk subtracts 0 from m: exact)
K_P2G_MASS = 2 + 1
# grid update (k_grid.h): im = 1 / m 1;  fma(v, im, 0) 1
K_GRID = 2
# friction_project (mpm_math.h) on a band node: dot, tangent, norm, scale, recombination — every step a few roundings relative to |v|;
# counted generously as 16.  The map itself is Lipschitz in v with constant <= 2 + mu (normal part 1, tangential part 1 + mu).
K_BC = 16
# G2P (k_g2p.h: g2p_particle): the gather is three nested fma chains, 3 + 3 + 3 roundings relative to the partial sums; B also has
# e = w * d (1) — d = r - 1, r - 2 are exact
K_G2P_V = 9
K_G2P_B = 10
# x' = fma(v, dt, x): 1.  F' = cdg F with cdg = fma(scale, b, I) (1), scale = -4 * idx * dt (2), three fma per entry of the product (3)
K_CDG = 3
K_F = 3


def _w(fx):
    return np.stack([0.5 * (1.5 - fx) ** 2, 0.75 - (fx - 1.0) ** 2, 0.5 * (fx - 0.5) ** 2], axis=1)  # [particle, offset, axis]


class Scene:
    """the live particles of a state (oracle.State, fp32) on a grid, widened; `live` = the slots the device keeps"""

    def __init__(self, state, res, dx, dt, clean_boundary, gravity=(0.0, -10.0, 0.0), planes=(), friction=0.4):
        self.res = tuple(res)
        self.dx = float(np.float32(dx))
        self.idx = float(np.float32(1.0) / np.float32(dx))
        self.dt = float(np.float32(dt))
        self.g = np.asarray(np.asarray(gravity, np.float32), np.float64)
        self.planes = [tuple(float(np.float32(c)) for c in p) for p in planes]
        self.friction = float(np.float32(friction))
        key = sort_key(state.x, dx, self.res, v=state.v, ids=state.ids, clean_boundary=clean_boundary)
        self.live = key >= 0
        m = self.live
        self.ids = state.ids[m]
        self.x = state.x[m].astype(np.float64)
        self.v = state.v[m].astype(np.float64)
        self.B = state.B[m].astype(np.float64).reshape(-1, 3, 3)
        self.F = state.F[m].astype(np.float64).reshape(-1, 3, 3)
        self.aux = state.aux[m].astype(np.float64)
        self.gid = state.gid[m]
        self.gp = state.gparams.astype(np.float64)[self.gid]
        self.types = state.gtype[self.gid]
        self.mass = self.gp[:, 0]
        X32 = state.x[m] * np.float32(self.idx)  # fp32, as particle_key has it
        self.base = np.floor(X32 - np.float32(0.5)).astype(np.int64)
        self.X = self.x * self.idx
        self.fx = self.X - self.base
        self.w = _w(self.fx)
        self.pw = np.abs(self.X) + W_ABS  # |dw_a| <= u pw_a
        self.S = -4.0 * self.idx * self.dt

    @property
    def n(self):
        return len(self.x)

    def stress_tol(self, stress):
        """the absolute error an entry of the device's stress is allowed (tests/test_gpu_ref.py), per particle"""
        if self.n == 0 or not np.any(stress):
            return np.zeros(self.n)
        return STRESS_REL * np.abs(stress).max() + 2.0 * self.gp[:, 2] * self.gp[:, 1] * STRESS_ABS * np.any(stress != 0, axis=(1, 2))

    def taps(self):
        """the 27 stencil taps: (i, j, k), node index arrays, weight, d = fx - (i, j, k), and the weight's error in u"""
        w, pw = self.w, self.pw
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    wa = (w[:, i, 0], w[:, j, 1], w[:, k, 2])
                    ww = wa[0] * wa[1] * wa[2]
                    dw = pw[:, 0] * np.abs(wa[1] * wa[2]) + pw[:, 1] * np.abs(wa[0] * wa[2]) + pw[:, 2] * np.abs(wa[0] * wa[1])
                    node = (self.base[:, 0] + i, self.base[:, 1] + j, self.base[:, 2] + k)
                    yield (i, j, k), node, ww, self.fx - np.array([i, j, k], np.float64), dw


def p2g(sc, drop=None):
    """raw (m v, m) sums of the grid, shape res + 1 x 4, and their bounds.  Returns dict(grid, bound, touched, count).
    drop: a function (tap, node, contrib) -> contrib, the hook of the seeded mutants of tests/test_transfer_model_cpu.py"""
    shape = tuple(r + 1 for r in sc.res)
    grid, absum, pos, strs = (np.zeros(shape + (4,)) for _ in range(4))
    count = np.zeros(shape, np.int64)
    v = sc.v + sc.g * sc.dt
    stress = np_mpm.kirchhoff_like_force(sc.types, sc.gp, sc.F, sc.aux) if sc.n else np.zeros((0, 3, 3))
    A = stress * sc.S + sc.B * (4.0 * sc.mass)[:, None, None]
    dA = sc.stress_tol(stress) * abs(sc.S)                                   # per entry of A
    mv = sc.mass[:, None] * v
    q_abs = np.abs(mv) + 1.5 * np.abs(A).sum(2)                              # every intermediate of the walk over the stencil
    ax_abs = np.abs(A) * np.abs(sc.X)[:, None, :]                            # |A_ca| |X_a|: the offset's error, in u
    for tap, node, ww, d, dw in sc.taps():
        q = mv + np.einsum("nij,nj->ni", A, d)
        c = np.concatenate([ww[:, None] * q, (ww * sc.mass)[:, None]], 1)
        if drop is not None:
            c, node = drop(tap, node, c)
        np.add.at(grid, node, c)
        aw = np.abs(ww)
        np.add.at(absum, node, np.concatenate([aw[:, None] * q_abs, (aw * sc.mass)[:, None]], 1))
        np.add.at(pos, node, np.concatenate([dw[:, None] * q_abs + aw[:, None] * ax_abs.sum(2), (dw * sc.mass)[:, None]], 1))
        np.add.at(strs, node, np.concatenate([np.repeat((aw * dA * 4.5)[:, None], 3, 1), np.zeros((sc.n, 1))], 1))  # sum_a |d_a| <= 4.5
        np.add.at(count, node, 1)
    K = np.array([K_P2G_MOM] * 3 + [K_P2G_MASS], np.float64)
    bound = U * ((K + np.maximum(count, 1)[..., None] - 1.0) * absum + pos) + strs
    return dict(grid=grid, bound=bound, touched=count > 0, count=count, absum=absum)


def plane_phi(sc):
    """(phi in cells, normal) of every node against the scene's planes: the nearest plane (smallest phi), as np_mpm takes it"""
    shape = tuple(r + 1 for r in sc.res)
    if not sc.planes:
        return np.full(shape, np.inf), np.zeros(shape + (3,))
    P = np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij"), -1).astype(np.float64) * sc.dx
    phis = np.stack([(P @ np.asarray(pl[:3]) + pl[3]) * sc.idx for pl in sc.planes], -1)
    which = phis.argmin(-1)
    return phis.min(-1), np.asarray([pl[:3] for pl in sc.planes])[which]


def band_margin(sc, touched):
    """the smallest distance (cells) of a touched node's phi from an edge of the boundary band (-3 and 0)"""
    phi, _ = plane_phi(sc)
    p = phi[touched]
    return float(np.minimum(np.abs(p), np.abs(p + 3.0)).min()) if len(p) else np.inf


def grid_update(sc, raw, raw_bound):
    """(v, m) of the grid from the raw sums: normalise, (gravity rides on the particles), plane boundary with friction.  The bound of
    a normalised velocity is (d(mv) + |v| dm) / m + K_GRID u |v|: a node of tiny mass gets the loose bound it deserves."""
    grid, bound = raw.copy(), raw_bound.copy()
    m = raw[..., 3]
    nz = m > 0
    vel = raw[nz, :3] / m[nz][:, None]
    grid[nz, :3] = vel
    bound[nz, :3] = (raw_bound[nz, :3] + np.abs(vel) * raw_bound[nz, 3:4]) / m[nz][:, None] + K_GRID * U * np.abs(vel)
    phi, nrm = plane_phi(sc)
    act = (m != 0) & (phi >= -3.0) & (phi <= 0.0)
    if act.any():
        vel, nn, mu = grid[act, :3], nrm[act], sc.friction
        if mu == -1:
            new = np.zeros_like(vel)
            nb = np.zeros_like(vel)
        else:
            slip = mu <= -2
            mu = -mu - 2 if slip else mu
            rn = (vel * nn).sum(1)
            rt = vel - rn[:, None] * nn
            tn = np.linalg.norm(rt, axis=1)
            s = np.maximum(tn + np.minimum(rn, 0) * mu, 0) / np.maximum(1e-30, tn)
            new = s[:, None] * rt + np.maximum(0, rn * (0.0 if slip else 1.0))[:, None] * nn
            nb = ((2.0 + mu) * np.linalg.norm(bound[act, :3], axis=1) + K_BC * U * np.linalg.norm(vel, axis=1))[:, None] * np.ones(3)
        grid[act, :3] = new
        bound[act, :3] = nb
    return dict(grid=grid, bound=bound, band=act)


def g2p(sc, grid, grid_bound=None, read=None):
    """G2P of the live particles from `grid` (res + 1 x 4; the velocities are read).  grid_bound: the bound the device's grid is held
    to, carried into the result (the whole substep); None = the device gathers from this very grid.  read: a function
    (tap, node) -> node, the hook of the mutant that reads one row off.  Returns dict of x, v, B, F, aux and <field>_bound."""
    n = sc.n
    v, B, va, Ba, vp, Bp, vg, Bg = (np.zeros((n, 3)) if k % 2 == 0 else np.zeros((n, 3, 3)) for k in range(8))
    for tap, node, ww, d, dw in sc.taps():
        if read is not None:
            node = read(tap, node)
        gv = grid[node][:, :3]
        ag, aw, ad = np.abs(gv), np.abs(ww), np.abs(d)
        v += ww[:, None] * gv
        B += np.einsum("ni,nj->nij", ww[:, None] * gv, d)
        va += aw[:, None] * ag
        Ba += np.einsum("ni,nj->nij", aw[:, None] * ag, ad)
        vp += dw[:, None] * ag
        Bp += np.einsum("ni,nj->nij", ag, dw[:, None] * ad + aw[:, None] * np.abs(sc.X))  # d(w d) <= dw |d| + w dfx
        if grid_bound is not None:
            gb = grid_bound[node][:, :3]
            vg += aw[:, None] * gb
            Bg += np.einsum("ni,nj->nij", aw[:, None] * gb, ad)
    v_b = U * (K_G2P_V * va + vp) + vg
    B_b = U * (K_G2P_B * Ba + Bp) + Bg
    x = sc.x + sc.dt * v
    x_b = sc.dt * v_b + U * np.abs(x)
    sdt = sc.dt * (-4.0 * sc.idx)
    cdg = np.eye(3) + sdt * B
    cdg_b = abs(sdt) * (B_b + K_CDG * U * np.abs(B)) + U * np.abs(cdg)
    F, aux = np_mpm.plasticity(sc.types, sc.gp, cdg, sc.F, sc.aux) if n else (sc.F.copy(), sc.aux.copy())
    F_b = np.einsum("nik,nkj->nij", cdg_b, np.abs(sc.F)) + K_F * U * np.einsum("nik,nkj->nij", np.abs(cdg), np.abs(sc.F))
    return dict(x=x, v=v, B=B, F=F, aux=aux, x_bound=x_b, v_bound=v_b, B_bound=B_b, F_bound=F_b)


def folded_B_bound(sc, out):
    """what the download of a ctx that folds apic_b into A adds to B's bound: B = (A - stress S) / (4 m), with A = fma(stress, S,
    b * 4m) from the fused G2P path and the stress evaluated AGAIN by the download (k_particles.h): two evaluations of the stress, each
    within stress_tol, and the roundings of A, of the fma back and of the division (4), relative to |stress S| + 4 m |B| — all over 4 m.
    Per particle: it is |stress S| / (4 m) scaled by the stress tolerance, not a global norm."""
    stress = np_mpm.kirchhoff_like_force(sc.types, sc.gp, out["F"], out["aux"]) if sc.n else np.zeros((0, 3, 3))
    m4 = (4.0 * sc.mass)[:, None, None]
    return (2.0 * sc.stress_tol(stress)[:, None, None] * abs(sc.S) + 4 * U * (np.abs(stress * sc.S) + m4 * np.abs(out["B"]))) / m4


def substep(sc):
    """the three stages in turn; the particles' bounds carry the grid's"""
    a = p2g(sc)
    b = grid_update(sc, a["grid"], a["bound"])
    out = g2p(sc, b["grid"], b["bound"])
    out.update(p2g=a, grid=b)
    return out


def ratio(got, want, bound):
    """largest |got - want| / bound (0 / 0 counts as 0: a value with no contribution has to be exactly 0), and where"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    if r.size == 0:
        return 0.0, None
    at = np.unravel_index(np.argmax(r), r.shape)
    return float(r[at]), tuple(int(i) for i in at)
