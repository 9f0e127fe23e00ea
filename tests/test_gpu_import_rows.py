"""mpmhip_import_particles and the apic_b rows of the arrivals (include/mpmhip.h, "migration").

A ctx with discard_apic_b (keep_apic_b off, the default) never writes the apic_b rows in a substep: they are behind the affine
matrices (RecordState::b_stale) until k_recover_b rewrites them.  The migration pack hands out the places in its buffer by atomics,
so WHICH stale row would land at which slot of the receiver depends on the order of arrival — and a tiled job's snapshot copies the
rows as they lie (tests/test_gpu_snapshot_job.py demands two deterministic runs to save the same bytes).  The arrivals' rows are
therefore stored as zero while the receiver's rows are stale; rows that are current (no substep yet, or keep_apic_b) arrive as sent.
The rows are read as they lie through mpmhip_snapshot_save of the one ctx (the blob's third section: 48 bytes per slot)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES, DX = 32, 1.0 / 32
N, K = 300, 7  # particles of the scene, arrivals


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


def _blob(sim):
    n = int(sim._check(sim._L.mpmhip_snapshot_size(sim._ctx)))
    buf = np.empty(n, np.uint8)
    sim._check(sim._L.mpmhip_snapshot_save(sim._ctx, buf.ctypes.data_as(C.c_void_p), n))
    return buf


def _sections(sim):
    """(header, RecG [slots][16], RecP [slots][16], apic_b rows [slots][12]) of the ctx's records as they lie, as float32 words"""
    from taichi_mpm_amd import _lib
    b = _blob(sim)
    h = _lib.SnapHeader.from_buffer_copy(b[:C.sizeof(_lib.SnapHeader)].tobytes())
    at = C.sizeof(_lib.SnapHeader) + h.n_groups * C.sizeof(_lib.GroupParams)
    n = h.n_slots
    rg = b[at:at + n * 64].view(np.float32).reshape(n, 16)
    rp = b[at + n * 64:at + n * 128].view(np.float32).reshape(n, 16)
    rb = b[at + n * 128:at + n * 176].view(np.float32).reshape(n, 12)
    return h, rg, rp, rb


def _scene(tm, substeps, **cfg):
    sim = tm.create_simulation3("mpm").initialize(dict(dict(res=(RES,) * 3, delta_x=DX, base_delta_t=1e-4, max_particles=N + 64), **cfg))
    sim.set_levelset(tm.mpm.LevelSet())
    rng = np.random.default_rng(5)
    x = ((12 + 8 * rng.random((N, 3))) * DX).astype(np.float32)
    sim.add_particles(dict(type="jelly", positions=x, B=rng.normal(0, 0.02, (N, 9)).astype(np.float32)))
    sim._ensure_ctx()
    if substeps:
        sim.run_substeps(substeps)
    sim.synchronize()
    return sim


def _import(sim, torch):
    """K copies of the ctx's first records with new ids and an apic_b row of sevens, appended by mpmhip_import_particles"""
    h, rg, rp, rb = _sections(sim)
    slots = int(h.n_slots)
    rec = np.zeros((K, 44), np.float32)
    rec[:, 0:16], rec[:, 16:32], rec[:, 32:44] = rg[:K], rp[:K], 7.0
    rec.view(np.int32)[:, 14] = 5000 + np.arange(K)  # RecG.pid
    buf = torch.from_numpy(rec).cuda()
    torch.cuda.synchronize()
    sim._check(sim._L.mpmhip_import_particles(sim._ctx, K, C.c_void_p(buf.data_ptr())))
    sim.synchronize()
    h2, rg2, rp2, rb2 = _sections(sim)
    assert int(h2.n_slots) == slots + K
    assert np.array_equal(rg2[slots:, 14].view(np.int32), 5000 + np.arange(K))  # the records themselves arrive as sent
    assert np.array_equal(rg2[slots:, :14].view(np.uint32), rec[:, :14].view(np.uint32)) and np.array_equal(rp2[slots:].view(np.uint32), rec[:, 16:32].view(np.uint32))
    assert np.array_equal(rb2[:slots].view(np.uint32), rb[:slots].view(np.uint32))  # nobody else's row moved
    return int(h2.b_stale), rb2[slots:]


def test_arrivals_on_a_ctx_with_stale_rows_get_zero_rows(tm):
    import torch
    sim = _scene(tm, 2)
    stale, rows = _import(sim, torch)
    assert stale == 1 and not rows.view(np.uint32).any()
    sim.close()


@pytest.mark.parametrize("case", ["before_the_first_substep", "keep_apic_b"])
def test_arrivals_on_a_ctx_with_current_rows_keep_their_rows(tm, case):
    import torch
    sim = _scene(tm, 0) if case == "before_the_first_substep" else _scene(tm, 2, keep_apic_b=True)
    stale, rows = _import(sim, torch)
    assert stale == 0 and (rows == 7.0).all()
    sim.close()
