"""The float64 model of tests/transfer_model.py extended by the CPIC branches of the colour-aware transfers (csrc/k_rigid_transfer.h:
k_p2g_rigid, k_g2p_rigid; reference src/transfer.cpp:367-463, 706-835) — TEST INFRASTRUCTURE ONLY.  Written from the maths.  The colour
field is an INPUT (Cpic): the dense node words (24 tag bits | body id + 1 << 24), the particles' colour words, gather_cdf's (normal,
distance, near) per particle, the world positions of the bodies' boundary particles (which decide the FLAGGED blocks: the 4 x 4 x 8-node
page of a boundary particle's base node and its neighbours in the positive directions, src/mpm.cpp:1026-1076; everywhere else the
transfers ignore colours) and the bodies.  What is modelled is the transfers alone.

A particle's tap is of the OTHER COLOUR when its block is flagged and cdf_incompatible(node word, colour word) holds (restated on
integers below).  P2G gives such a tap nothing on the grid; if the node has a body id, the body gets the impulse

    m w (v - friction_project(v, v_body(node), n_p, mu_side))  +  dt force(F) grad w          and its torque about the body's centre.

G2P gathers, for such a tap, the particle's own post-gravity velocity — projected against the body's surface motion plus dt dx
pushing_force n_p when gather_cdf found a boundary for the particle (near) — instead of the node's; near particles lose B; inside the
penalty window -0.3 dx < distance < -0.05 dx the velocity gets -distance n penalty and the last body met the opposite impulse at x'.
substep_cpic stops BEFORE advect_rigid_bodies: the bodies' poses are those of the start of the substep, their velocities are updated by
the impulses of P2G (k_rigid_apply_tmp's arithmetic) before G2P reads them.

THE BOUNDS keep the form of tests/transfer_model.py: u (K + N - 1) sum |terms| + position term + stress term.  The chains counted here:
see the constants.  friction_project enters through its Lipschitz constant (2 + mu) and K_BC; the stress term of an impulse is
stress_tol * dt * sum_a |grad_a w|; a torque's bound is |r| x the impulse's bound plus the roundings of r and of the cross product."""
import numpy as np

from oracle import np_mpm
from tests import transfer_model as tmod
from tests.transfer_model import K_BC, K_CDG, K_F, K_P2G_MASS, K_P2G_MOM, U

STATE_MASK = 0xAAAAAAAA
TAG_MASK = 0x00FFFFFF
# The block-relative position takes the position term of tests/transfer_model.py as it is: k_p2g_rigid forms r = x * idx - (float)g as
# k_p2g does; k_g2p_rigid forms X0 = x * idx - origin and r = X0 - c0, integers taken off a float of the same or a larger exponent —
# exact, or (fused) one rounding no larger than that of X.
# one impulse term of the second pass of k_p2g_rigid: v + g dt (fma) 1; w = (wa wb) wc 2; mass * w 1; v - pv 1; their product 1 — 6 for the
# momentum part; dtF = force * dt 1; grad_a = da idx wb wc 3; three products and two additions of the row 5 — 9 for the stress part; the sum
# of the two parts 1.  K = max(6, 9) + 1, relative to the absolute sum of both parts.
K_IMP = 10
# v_body(node) = vel + omega x (node dx - pos): node * dx 1 (relative to |node dx|), the subtraction 1, a cross product component 3
# (relative to its absolute sum), the addition 1
K_RV_CROSS, K_RV_ADD = 4, 1
# a torque: r = at - centre 1; a cross product component (two products, one subtraction) 3
K_TRQ = 3
# derivative of a weight along its axis, (t - 1.5, -2 t, t + 1.5) with t = r - (0, 1, 2): |d/dr| <= 2, absolute roundings of values <= 2.5: 4 u
DW_LIP, DW_ABS = 2.0, 4.0
# k_g2p_rigid gathers v and b in FLAT chains (passes 2 and 3 share the accumulators): every tap enters once with a non-zero weight,
# 27 fma roundings relative to the partial sums, w = (w0 w1) w2 2; b: w * gv 1 more
K_G2P_RIGID_V = 27 + 2
K_G2P_RIGID_B = 27 + 3
# pass 3's substituted velocity: the push dt * dx * pushing_force 2, n * push 1, the addition 1 (relative to |fake| + |push|)
K_PUSH = 4
# the penalty: dist * n 1, * penalty 1, v - dv 1; the impulse dv * mass 1 more
K_PEN_V, K_PEN_IMP = 3, 3
# k_rigid_apply_tmp: vel += imp * inv_mass 2; omega += R (I^-1 (R^T trq)): three 3 x 3 products, 3 x 5 roundings relative to the absolute
# products, the addition 1
K_APPLY_V, K_APPLY_W = 2, 16


def incompatible(word, pstate):
    """cdf_incompatible of csrc/k_rigid.h (src/transfer.cpp:419-423) on integer arrays"""
    gs = word.astype(np.int64) & TAG_MASK
    ps = pstate.astype(np.int64)
    mask = (gs & ps & STATE_MASK) >> 1
    return (gs & mask) != (ps & mask)


def quat_R(q):
    w, x, y, z = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def body_of(state, friction):
    """a body of the model from get_rigid_state() / rigid_state() (inertia in the body frame) and its two friction coefficients"""
    R = quat_R(state["rotation"])
    inv_I = np.asarray(state["inv_inertia"], np.float64)
    return dict(position=np.asarray(state["position"], np.float64), velocity=np.asarray(state["velocity"], np.float64),
                angular_velocity=np.asarray(state["angular_velocity"], np.float64), mass=float(state["mass"]), inv_mass=float(state["inv_mass"]),
                Iw=R @ np.asarray(state["inertia"], np.float64) @ R.T, Iw_inv=R @ inv_I @ R.T,
                friction=tuple(float(np.float32(f)) for f in friction))


def abscross(a, b):
    """|a| x |b| with every product counted positive"""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def friction_project(v, vb, n, mu):
    """src/mpm_fwd.h:25-57 (csrc/mpm_math.h), per row; mu per row"""
    mu = np.broadcast_to(np.asarray(mu, np.float64), v.shape[:1]).copy()
    sticky, slip = mu == -1.0, mu <= -2.0
    mu = np.where(slip, -mu - 2.0, mu)
    r = v - vb
    nn = (n * r).sum(1)
    t = r - nn[:, None] * n
    tn = np.linalg.norm(t, axis=1)
    ts = np.maximum(tn + np.minimum(nn, 0.0) * mu, 0.0) / np.maximum(1e-30, tn)
    keep = np.where(slip, 0.0, np.maximum(0.0, nn))
    out = ts[:, None] * t + keep[:, None] * n + vb
    return np.where(sticky[:, None], vb, out), np.where(sticky, 1.0, 2.0 + np.abs(mu))


class Cpic:
    """the colour field and the bodies around a transfer_model.Scene `M` (all of whose particles are live, in creation order)"""

    def __init__(self, M, words, pstate, normal, dist, near, sample_pos, bodies, penalty, pushing_force):
        assert M.live.all()
        self.M = M
        self.words = np.asarray(words, np.uint32)
        self.pstate = np.asarray(pstate).astype(np.uint32)
        self.normal = np.asarray(normal, np.float64)
        self.dist32 = np.asarray(dist, np.float32)
        self.dist = self.dist32.astype(np.float64)
        self.near = np.asarray(near) != 0
        self.bodies = [None] + list(bodies)  # (body ids start at 1: 0 is the background)
        self.penalty, self.push = float(np.float32(penalty)), float(np.float32(pushing_force))
        # the flagged pages, from the boundary particles as k_cdf_alloc takes them (fp32)
        X = np.asarray(sample_pos, np.float32) * np.float32(M.idx)
        ok = ((X >= np.float32(0.5)) & (X < np.asarray(M.res, np.float32) - np.float32(1.5))).all(1)
        b = (X[ok] - np.float32(0.5)).astype(np.int64)
        pg = np.stack([b[:, 0] >> 2, b[:, 1] >> 2, b[:, 2] >> 3], 1)
        self.pages = set()
        for o in range(8):
            self.pages |= set(map(tuple, pg + np.array([o >> 2, (o >> 1) & 1, o & 1])))
        self.pw = M.pw
        self.flagged = self.flagged_block(M.base >> 2)

    def flagged_block(self, blk):
        """is the 4^3-node block (block coordinates, rows) handled by the colour-aware kernels"""
        blk = np.asarray(blk)
        return np.array([(int(b[0]), int(b[1]), int(b[2]) >> 1) in self.pages for b in blk], bool)

    def with_bodies(self, bodies):
        import copy
        c = copy.copy(self)
        c.bodies = [None] + list(bodies)
        return c

    def taps(self):
        """transfer_model's taps with the weight error, the weights per axis, `other` (the tap is of the other colour) and the
        body id of the node (the word holds id + 1; 0 here: none — body 0 is the background and owns no node)"""
        M, pw = self.M, self.pw
        for tap, node, ww, d, _ in M.taps():
            i, j, k = tap
            wa = (M.w[:, i, 0], M.w[:, j, 1], M.w[:, k, 2])
            dw = pw[:, 0] * np.abs(wa[1] * wa[2]) + pw[:, 1] * np.abs(wa[0] * wa[2]) + pw[:, 2] * np.abs(wa[0] * wa[1])
            word = self.words[node]
            yield tap, node, ww, d, dw, wa, incompatible(word, self.pstate) & self.flagged, np.maximum((word >> 24).astype(np.int64) - 1, 0)

    def body_velocity_at(self, rid, gp):
        """(v_body(gp), its rounding error in u, per row); rid per row, 0 = no body: zeros"""
        v, e = np.zeros(gp.shape), np.zeros(gp.shape)
        for b in range(1, len(self.bodies)):
            m = rid == b
            if m.any():
                B = self.bodies[b]
                r = gp[m] - B["position"]
                c = np.cross(B["angular_velocity"], r)
                v[m] = B["velocity"] + c
                ac = abscross(np.broadcast_to(B["angular_velocity"], r.shape), r)
                e[m] = K_RV_ADD * np.abs(v[m]) + K_RV_CROSS * ac + abscross(np.broadcast_to(B["angular_velocity"], r.shape), np.abs(gp[m]) + np.abs(r)) \
                    + B.get("velocity_bound", 0.0) / U + abscross(np.broadcast_to(B.get("angular_velocity_bound", np.zeros(3)), r.shape), r) / U
        return v, e

    def side_friction(self, rid, pstate, swap=False):
        """fric[(pstate >> 2 rid) & 1] of the node's body, per row (0 where the node has none); swap: the other side's (a seeded fault)"""
        mu = np.zeros(len(rid))
        for b in range(1, len(self.bodies)):
            m = rid == b
            f = np.asarray(self.bodies[b]["friction"])
            side = ((pstate[m] >> np.uint32(2 * b)) & 1).astype(np.int64)
            mu[m] = f[1 - side if swap else side]
        return mu


def _dweights(fx):
    """d w / d fx per (particle, offset, axis)"""
    return np.stack([fx - 1.5, -2.0 * (fx - 1.0), fx - 0.5], axis=1)


def impulse_terms(C, pre, row, hooks):
    """the impulse terms of one stencil tap for the particles `sel` that have a node of the other colour with a body there: (node
    positions, terms, their absolute sums, their bounds), rows of 3"""
    M = C.M
    (i, j, k), sel, node, ww, dw, wa, rid = row
    gp = np.stack(node, 1).astype(np.float64) * M.dx
    rv, rv_e = C.body_velocity_at(rid, gp)
    mu = C.side_friction(rid, C.pstate[sel], "side" in hooks)
    vs, dtF, m_ = pre["v"][sel], pre["dtF"][sel], M.mass[sel]
    pv, lip = friction_project(vs, rv, C.normal[sel], mu)
    dwa = (pre["dwt"][sel, i, 0], pre["dwt"][sel, j, 1], pre["dwt"][sel, k, 2])
    gr = M.idx * np.stack([dwa[0] * wa[1] * wa[2], wa[0] * dwa[1] * wa[2], wa[0] * wa[1] * dwa[2]], 1)
    term = (m_ * ww)[:, None] * (vs - pv) + np.einsum("nij,nj->ni", dtF, gr)
    t_abs = (m_ * np.abs(ww))[:, None] * (np.abs(vs) + np.abs(pv)) + np.einsum("nij,nj->ni", np.abs(dtF), np.abs(gr))
    dpv = lip[:, None] * (np.linalg.norm(np.abs(vs) + rv_e, axis=1))[:, None] + K_BC * (np.linalg.norm(vs, axis=1) + np.linalg.norm(rv, axis=1))[:, None]
    # the gradient's error: the derivative's own and the two other weights', per axis
    pwv, ddv = C.pw[sel], pre["ddw"][sel]
    awa = [np.abs(a) for a in wa]
    adw = [np.abs(a) for a in dwa]
    dgr = M.idx * np.stack([ddv[:, 0] * awa[1] * awa[2] + adw[0] * (pwv[:, 1] * awa[2] + awa[1] * pwv[:, 2]),
                            ddv[:, 1] * awa[0] * awa[2] + adw[1] * (pwv[:, 0] * awa[2] + awa[0] * pwv[:, 2]),
                            ddv[:, 2] * awa[0] * awa[1] + adw[2] * (pwv[:, 0] * awa[1] + awa[0] * pwv[:, 1])], 1)
    t_bound = U * (K_IMP * t_abs + (m_ * np.abs(ww))[:, None] * dpv + (m_ * dw)[:, None] * np.abs(vs - pv)
                   + np.einsum("nij,nj->ni", np.abs(dtF), dgr)) + (pre["stol"][sel] * M.dt * np.abs(gr).sum(1))[:, None]
    return gp, term, t_abs, t_bound


def p2g_cpic(C, hooks=None):
    """raw grid sums with the colour test and the impulses the bodies receive.  Returns dict(grid, bound, touched, count, impulse[body, 6],
    impulse_bound[body, 6], impulse_abs, impulse_n, boundary_count[block], other[particle], tap_body_count[particle, body],
    block_bodies[block]).
    hooks: the seeded mutants of tests/test_cpic_transfer_model_cpu.py, as transfer_model.p2g takes `drop` — a dict of functions:
    "other" (tap, node, other, rid) -> other;  "contrib" (tap, node, contribution) -> contribution;  "side": the friction side swapped;
    "credit" (particles, body, state) -> (body credited, keep) with state = dict(first_body, other, block, boundary_count)"""
    hooks = hooks or {}
    M = C.M
    n, nb = M.n, len(C.bodies)
    shape = tuple(r + 1 for r in M.res)
    grid, absum, pos, strs = (np.zeros(shape + (4,)) for _ in range(4))
    count = np.zeros(shape, np.int64)
    v = M.v + M.g * M.dt
    stress = np_mpm.kirchhoff_like_force(M.types, M.gp, M.F, M.aux) if n else np.zeros((0, 3, 3))
    A = stress * M.S + M.B * (4.0 * M.mass)[:, None, None]
    stol = M.stress_tol(stress)
    dA = stol * abs(M.S)
    mv = M.mass[:, None] * v
    q_abs = np.abs(mv) + 1.5 * np.abs(A).sum(2)
    ax_abs = np.abs(A) * np.abs(M.X)[:, None, :]
    pre = dict(v=v, dtF=stress * M.dt, stol=stol, dwt=_dweights(M.fx), ddw=DW_LIP * np.abs(M.X) + DW_ABS)  # |d (dw_a)| <= u ddw_a
    blk = M.base >> 2
    nblk = tuple(int(x) for x in ((np.asarray(M.res) + 3) >> 2))
    other = np.zeros(n, bool)
    rows = []
    # the grid: transfer_model.p2g with the taps of the other colour left out
    for tap, node, ww, d, dw, wa, oth, rid in C.taps():
        if "other" in hooks:
            oth = hooks["other"](tap, node, oth, rid)
        other |= oth
        ok = ~oth
        q = mv + np.einsum("nij,nj->ni", A, d)
        c = np.concatenate([ww[:, None] * q, (ww * M.mass)[:, None]], 1) * ok[:, None]
        if "contrib" in hooks:
            c = hooks["contrib"](tap, node, c)
        np.add.at(grid, node, c)
        aw = np.abs(ww) * ok
        np.add.at(absum, node, np.concatenate([aw[:, None] * q_abs, (aw * M.mass)[:, None]], 1))
        np.add.at(pos, node, np.concatenate([(dw * ok)[:, None] * q_abs + aw[:, None] * ax_abs.sum(2), (dw * ok * M.mass)[:, None]], 1))
        np.add.at(strs, node, np.concatenate([np.repeat((aw * dA * 4.5)[:, None], 3, 1), np.zeros((n, 1))], 1))
        np.add.at(count, node, ok.astype(np.int64))
        sel = np.flatnonzero(oth & (rid > 0))
        if len(sel):
            rows.append((tap, sel, tuple(a[sel] for a in node), ww[sel], dw[sel], tuple(a[sel] for a in wa), rid[sel]))
    K = np.array([K_P2G_MOM] * 3 + [K_P2G_MASS], np.float64)
    bound = U * ((K + np.maximum(count, 1)[..., None] - 1.0) * absum + pos) + strs
    bcount = np.zeros(nblk, np.int64)  # boundary particles per block
    np.add.at(bcount, tuple(blk[other].T), 1)
    # the bodies: the taps of the other colour, in the kernels' tap order
    imp, imp_b, imp_abs = np.zeros((nb, 6)), np.zeros((nb, 6)), np.zeros((nb, 6))
    imp_n = np.zeros(nb, np.int64)
    tap_body = np.zeros((n, nb), np.int64)
    block_body = np.zeros(nblk + (nb,), bool)
    state = dict(first_body=np.zeros(n, np.int64), other=other, block=blk, boundary_count=bcount)
    for row in rows:
        sel, rid = row[1], row[6]
        gp, term, t_abs, t_bound = impulse_terms(C, pre, row, hooks)
        to, keep = hooks["credit"](sel, rid, state) if "credit" in hooks else (rid, np.ones(len(sel), bool))
        state["first_body"][sel] = np.where(state["first_body"][sel] > 0, state["first_body"][sel], rid)
        for b in range(1, nb):
            mb = rid == b
            if not mb.any():
                continue
            np.add.at(tap_body[:, b], sel[mb], 1)
            block_body[tuple(blk[sel[mb]].T) + (b,)] = True
            r = gp[mb] - C.bodies[b]["position"]
            trq = np.cross(r, term[mb])
            dr = np.abs(gp[mb]) + np.abs(r)
            trq_abs = abscross(r, term[mb])
            trq_b = abscross(r, t_bound[mb]) + U * (abscross(dr, term[mb]) + K_TRQ * trq_abs)
            imp_abs[b] += np.concatenate([np.abs(term[mb]).sum(0), trq_abs.sum(0)])
            imp_b[b] += np.concatenate([t_bound[mb].sum(0), trq_b.sum(0)])
            imp_n[b] += int(mb.sum())
            for tb in np.unique(to[mb]):
                mt = (to[mb] == tb) & keep[mb]
                imp[tb] += np.concatenate([term[mb][mt].sum(0), trq[mt].sum(0)])
    imp_b += U * np.maximum(imp_n - 1, 0)[:, None] * imp_abs
    return dict(grid=grid, bound=bound, touched=count > 0, count=count, absum=absum, impulse=imp, impulse_bound=imp_b, impulse_abs=imp_abs,
                impulse_n=imp_n, boundary_count=bcount, other=other, tap_body_count=tap_body, block_bodies=block_body.sum(-1))


def apply_impulses(C, imp, imp_bound):
    """the bodies after k_rigid_apply_tmp: vel += imp / m, omega += R I^-1 R^T torque; their velocities carry the impulses' bounds (on
    top of the bounds they carried already)"""
    out = []
    for b in range(1, len(C.bodies)):
        B = dict(C.bodies[b])
        dv, dw = imp[b, :3] * B["inv_mass"], B["Iw_inv"] @ imp[b, 3:]
        B["velocity"] = B["velocity"] + dv
        B["angular_velocity"] = B["angular_velocity"] + dw
        B["velocity_bound"] = B.get("velocity_bound", 0.0) + imp_bound[b, :3] * B["inv_mass"] + U * (K_APPLY_V * np.abs(dv) + np.abs(B["velocity"]))
        B["angular_velocity_bound"] = B.get("angular_velocity_bound", 0.0) + np.abs(B["Iw_inv"]) @ (imp_bound[b, 3:] + K_APPLY_W * U * np.abs(imp[b, 3:])) \
            + U * np.abs(B["angular_velocity"])
        out.append(B)
    return out


def advect_velocities(C, bodies):
    """what advect_rigid_bodies does to the VELOCITIES of free, undamped bodies without a rotation axis (k_rigid_advect; the poses are not
    modelled): the damping factors are exp(0) = 1, gravity adds g * mass * dt * inv_mass — three products (mass * inv_mass within a
    rounding of 1) and the addition"""
    out = []
    for B in bodies:
        B = dict(B)
        dv = C.M.g * C.M.dt
        B["velocity"] = B["velocity"] + dv
        B["velocity_bound"] = B["velocity_bound"] + U * (4 * np.abs(dv) + np.abs(B["velocity"]))
        out.append(B)
    return out


def measured_bound(B_before, v_after, w_after, imp_abs, imp_bound):
    """the bound of a body's impulse MEASURED as mass * dv and I_world * domega from its fp32 velocities before and after a stage: the
    impulse's own bound; the roundings of the conversion to a velocity change (k_rigid_apply_tmp converts the sum, the reference every
    single impulse before it adds it: the same roundings, relative to the absolute sum imp_abs); and half an ulp of each of the two
    velocities the difference is taken of, times the mass / through |I_world|"""
    B = B_before
    sv = np.abs(B["velocity"]) + np.abs(v_after)
    sw = np.abs(B["angular_velocity"]) + np.abs(w_after)
    lin = imp_bound[:3] + U * (K_APPLY_V * imp_abs[:3] + B["mass"] * sv)
    ang = imp_bound[3:] + np.abs(B["Iw"]) @ (U * (K_APPLY_W * np.abs(B["Iw_inv"]) @ imp_abs[3:] + sw))
    return np.concatenate([lin, ang])


def measured_impulse(B_before, v_after, w_after):
    return np.concatenate([(np.asarray(v_after, np.float64) - B_before["velocity"]) * B_before["mass"],
                           B_before["Iw"] @ (np.asarray(w_after, np.float64) - B_before["angular_velocity"])])


ELASTIC = ("jelly", "linear", "elastic")  # plasticity() leaves cdg F as it is
PLASTIC_K = 64  # roundings of a return mapping (an SVD, logarithms, the projection, exponentials, two 3 x 3 products), relative to |F|


def plasticity_bound(M, cdg, Ft_bound):
    """(bound of F, bound of aux) behind plasticity(), from the bound of the trial F = cdg F: the trial's own bound for the elastic
    materials; for the others the return mapping's Jacobian (central differences of the float64 mapping, one entry of the trial at a
    time) applied to it entry by entry — first order, like every bound here — plus PLASTIC_K u |F| for the mapping's own arithmetic"""
    from oracle import oracle as orc
    elastic = np.isin(M.types, [orc.TYPE_IDS[m] for m in ELASTIC])
    aux_b = np.zeros(M.n)
    if elastic.all() or M.n == 0:
        return Ft_bound, aux_b
    Ft = np.einsum("nik,nkj->nij", cdg, M.F)
    eye = np.broadcast_to(np.eye(3), Ft.shape)
    out, h = np.zeros_like(Ft_bound), 1e-7
    for i in range(3):
        for j in range(3):
            E = np.zeros((3, 3))
            E[i, j] = h
            Fp, ap = np_mpm.plasticity(M.types, M.gp, eye, Ft + E, M.aux)
            Fm, am = np_mpm.plasticity(M.types, M.gp, eye, Ft - E, M.aux)
            out += np.abs(Fp - Fm) / (2 * h) * Ft_bound[:, i, j][:, None, None]
            aux_b += np.abs(ap - am) / (2 * h) * Ft_bound[:, i, j]
    F0, a0 = np_mpm.plasticity(M.types, M.gp, eye, Ft, M.aux)
    out += PLASTIC_K * U * np.abs(F0).max((1, 2))[:, None, None]
    aux_b += PLASTIC_K * U * np.maximum(np.abs(a0), np.abs(F0).max((1, 2)))
    return np.where(elastic[:, None, None], Ft_bound, out), np.where(elastic, 0.0, aux_b)


def g2p_cpic(C, grid, grid_bound=None, hooks=None):
    """G2P from `grid` with the colour test.  Returns g2p's fields and bounds plus impulse, impulse_bound, impulse_abs [body, 6] and
    `penalised` (which particles got the penalty push), `last_body` / `first_body` (the body of the last / first tap of the other colour
    that has one, in the kernels' tap order; 0: none — the penalty's impulse goes to the last).
    hooks: "other" and "side" as p2g_cpic takes them;  "window" (lo, hi) -> (lo, hi), the penalty window's edges in fp32;
    "penalty_body" (first_body, last_body) -> the body that receives the penalty's impulse"""
    hooks = hooks or {}
    M = C.M
    n, nb = M.n, len(C.bodies)
    v, va, vp, vg = (np.zeros((n, 3)) for _ in range(4))
    B, Ba, Bp, Bg = (np.zeros((n, 3, 3)) for _ in range(4))
    own = M.v + M.g * M.dt
    last, first = np.zeros(n, np.int64), np.zeros(n, np.int64)
    push = M.dt * M.dx * C.push
    for tap, node, ww, d, dw, wa, oth, rid in C.taps():
        if "other" in hooks:
            oth = hooks["other"](tap, node, oth, rid)
        gv = grid[node][:, :3].copy()
        gb = grid_bound[node][:, :3].copy() if grid_bound is not None else np.zeros((n, 3))
        sel = np.flatnonzero(oth)
        if len(sel):
            r = rid[sel]
            last[sel] = np.where(r > 0, r, last[sel])
            first[sel] = np.where(first[sel] > 0, first[sel], r)
            gp = np.stack([a[sel] for a in node], 1).astype(np.float64) * M.dx
            vb, vb_e = C.body_velocity_at(r, gp)
            mu = C.side_friction(r, C.pstate[sel], "side" in hooks)
            fake, fb = own[sel].copy(), U * np.abs(own[sel])
            nr = C.near[sel]
            pv, lip = friction_project(own[sel], vb, C.normal[sel], mu)
            pb = U * (lip[:, None] * np.linalg.norm(np.abs(own[sel]) + vb_e, axis=1)[:, None]
                      + K_BC * (np.linalg.norm(own[sel], axis=1) + np.linalg.norm(vb, axis=1))[:, None]
                      + K_PUSH * (np.abs(pv) + np.abs(C.normal[sel] * push)))
            fake[nr] = pv[nr] + C.normal[sel][nr] * push
            fb[nr] = pb[nr]
            gv[sel], gb[sel] = fake, fb
        ag, aw, ad = np.abs(gv), np.abs(ww), np.abs(d)
        v += ww[:, None] * gv
        B += np.einsum("ni,nj->nij", ww[:, None] * gv, d)
        va += aw[:, None] * ag
        Ba += np.einsum("ni,nj->nij", aw[:, None] * ag, ad)
        vp += dw[:, None] * ag
        Bp += np.einsum("ni,nj->nij", ag, dw[:, None] * ad + aw[:, None] * np.abs(M.X))
        vg += aw[:, None] * gb
        Bg += np.einsum("ni,nj->nij", aw[:, None] * gb, ad)
    flat = C.flagged[:, None]  # (the plain kernels gather in nested chains: transfer_model's K; the colour-aware ones in flat chains)
    v_b = U * (np.where(flat, K_G2P_RIGID_V, tmod.K_G2P_V) * va + vp) + vg
    B_b = U * (np.where(flat[:, :, None], K_G2P_RIGID_B, tmod.K_G2P_B) * Ba + Bp) + Bg
    x = M.x + M.dt * v
    x_b = M.dt * v_b + U * np.abs(x)
    sdt = M.dt * (-4.0 * M.idx)
    cdg = np.eye(3) + sdt * B
    cdg_b = abs(sdt) * (B_b + K_CDG * U * np.abs(B)) + U * np.abs(cdg)
    F, aux = np_mpm.plasticity(M.types, M.gp, cdg, M.F, M.aux) if n else (M.F.copy(), M.aux.copy())
    F_b = np.einsum("nik,nkj->nij", cdg_b, np.abs(M.F)) + K_F * U * np.einsum("nik,nkj->nij", np.abs(cdg), np.abs(M.F))
    F_b, aux_b = plasticity_bound(M, cdg, F_b)
    lose = C.near & C.flagged
    B[lose], B_b[lose] = 0.0, 0.0
    lo, hi = np.float32(-M.dx) * np.float32(0.3), np.float32(-0.05) * np.float32(M.dx)
    if "window" in hooks:
        lo, hi = hooks["window"](lo, hi)
    pen = lose & (C.dist32 < hi) & (C.dist32 > lo)
    dv = (C.dist * C.penalty)[:, None] * C.normal * pen[:, None]
    v = v - dv
    v_b = v_b + U * (K_PEN_V * np.abs(dv) + np.abs(v)) * pen[:, None]
    imp, imp_b, imp_abs = np.zeros((nb, 6)), np.zeros((nb, 6)), np.zeros((nb, 6))
    imp_n = np.zeros(nb, np.int64)
    for b in range(1, nb):
        m = pen & ((hooks["penalty_body"](first, last) if "penalty_body" in hooks else last) == b)
        if not m.any():
            continue
        t = dv[m] * M.mass[m][:, None]
        tb = U * K_PEN_IMP * np.abs(t)
        r = x[m] - C.bodies[b]["position"]
        dr = x_b[m] + U * (np.abs(x[m]) + np.abs(r))
        ta = abscross(r, t)
        imp[b] = np.concatenate([t.sum(0), np.cross(r, t).sum(0)])
        imp_abs[b] = np.concatenate([np.abs(t).sum(0), ta.sum(0)])
        imp_b[b] = np.concatenate([tb.sum(0), (abscross(r, tb) + abscross(dr, t) + U * K_TRQ * ta).sum(0)])
        imp_n[b] = int(m.sum())
    imp_b += U * np.maximum(imp_n - 1, 0)[:, None] * imp_abs
    return dict(x=x, v=v, B=B, F=F, aux=aux, x_bound=x_b, v_bound=v_b, B_bound=B_b, F_bound=F_b, aux_bound=aux_b, impulse=imp, impulse_bound=imp_b,
                impulse_abs=imp_abs, impulse_n=imp_n, penalised=pen, last_body=last, first_body=first)


def substep_cpic(C):
    """P2G, the bodies' velocity update, the grid update, G2P with the updated bodies — up to, not including, advect_rigid_bodies;
    `bodies`: at G2P; `bodies_after`: their velocities behind G2P's impulses and advect's gravity (the poses are not modelled)"""
    a = p2g_cpic(C)
    bodies = apply_impulses(C, a["impulse"], a["impulse_bound"])
    b = tmod.grid_update(C.M, a["grid"], a["bound"])
    out = g2p_cpic(C.with_bodies(bodies), b["grid"], b["bound"])
    after = apply_impulses(C.with_bodies(bodies), out["impulse"], out["impulse_bound"])
    out.update(p2g=a, grid=b, bodies=bodies, bodies_after=advect_velocities(C, after))
    return out
