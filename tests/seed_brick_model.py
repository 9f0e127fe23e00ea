"""numpy model of mpmhip_seed_particles_brick and mpmhip_seed_histogram (include/mpmhip.h; csrc/k_seed.h) on top of tests/seed_model.py:
the call on rank r of a partition creates the survivors of the one-ctx call whose base cell lies in r's brick,

  owner   Partition.rank_of_cells(base_cells(x)): the brick that holds b[k] = int(fl(fl(x[k] * fl(1 / dx)) - 0.5))
  id      first_id + (rank of the survivor among ALL survivors, ascending candidate number)
  slot    its rank among the survivors of ITS brick: a rank's records ascend in id

and the histogram call counts, per axis, the survivors by base cell.  `brute_force` restates both with one Python loop over the
candidates and plain integers — no searchsorted, no cumulative sums, no masks — for a region small enough to loop over."""
import numpy as np

from taichi_mpm_amd import tiled
from tests.seed_model import SampledRegion, SeedModel

F = np.float32


def sampled_sphere(tm, centre, r, dx):
    """the sphere baked on a lattice of spacing dx / 2 that is not aligned with the grid (the region of tests/test_gpu_seed.py)"""
    origin = tuple(np.float32(c - 14.3 * dx + 0.0137 * dx) for c in centre)
    c = np.asarray(centre, np.float64)
    return tm.mpm.SampledLevelSet.from_function(lambda x: np.linalg.norm(x - c, axis=1) - r, (60, 60, 60), origin, dx / 2)


def sampled_model(sls, res, dx, tile, ppc=8.0, base_dt=1e-4, **kw):
    return SeedModel(res, dx, SampledRegion(sls.phi, sls.origin, sls.spacing, dx), ppc=ppc, tile=tile, base_dt=base_dt, **kw)


def split(x, part, dx, first_id=0):
    """the one-ctx survivors x (in order) as the ranks of `part` hold them: [dict(x, id)] by rank, each in slot order"""
    owner = part.rank_of_cells(tiled.base_cells(x, dx))
    ids = (first_id + np.arange(len(x))).astype(np.int32)
    return [dict(x=x[owner == r], id=ids[owner == r]) for r in range(part.world)]


def histograms(x, res, dx, chunk=256):
    """(hists, cell_lo, cell_hi, total) as the device accumulates them: rows per chunk of survivors, added up in integers"""
    b = tiled.base_cells(x, dx)
    hists = [np.zeros(int(r), np.int64) for r in res]
    for lo in range(0, len(b), chunk):
        for a in range(3):
            row = np.zeros(int(res[a]), np.int64)
            np.add.at(row, b[lo:lo + chunk, a], 1)
            hists[a] += row
    if not len(b):
        return hists, np.zeros(3, np.int64), np.zeros(3, np.int64), 0
    return hists, b.min(0).astype(np.int64), b.max(0).astype(np.int64) + 1, len(b)


def brute_force(model, part, first_id=0):
    """one loop over the candidates of `model` in ascending c: ([dict(x, id)] by rank, hists) with Python integers throughout"""
    idx = F(1.0) / F(model.dx)
    x = model.positions(0, len(model.tile))
    keep = model.region.inside(x) & ~model.near_boundary(x)
    if model.source:
        keep &= ~model.region.inside((x + model.advection[None, :]).astype(F))
    ranks = [dict(x=[], id=[]) for _ in range(part.world)]
    hists = [[0] * int(r) for r in model.res]
    seen = 0
    for c in range(len(x)):
        if not keep[c]:
            continue
        b = [int(F(F(x[c, k]) * idx) - F(0.5)) for k in range(3)]
        p = []
        for a in range(3):
            q = 0
            while q + 1 < part.dims[a] and b[a] >= part.cuts[a][q + 1]:
                q += 1
            p.append(q)
            hists[a][b[a]] += 1
        r = (p[0] * part.dims[1] + p[1]) * part.dims[2] + p[2]
        ranks[r]["x"].append(x[c])
        ranks[r]["id"].append(first_id + seen)
        seen += 1
    out = [dict(x=np.array(d["x"], F).reshape(-1, 3), id=np.array(d["id"], np.int32)) for d in ranks]
    return out, [np.array(h, np.int64) for h in hists]
