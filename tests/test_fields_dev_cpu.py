"""Simulation3D.set_particle_tensors judges its arguments before a ctx is created or touched (taichi_mpm_amd/mpm.py:
check_particle_tensors): a tensor that is not on the simulation's device, another dtype than the field's, another shape than (n,) /
(n, width) and the key "gid" each raise MPMError naming the key.  No GPU is needed: the simulation never gets a ctx."""
import os
import subprocess
import sys

import pytest
import torch


@pytest.fixture(scope="module")
def tm():
    import taichi_mpm_amd as tm
    tm.load()
    return tm


@pytest.fixture()
def sim(tm):
    s = tm.create_simulation3("mpm").initialize(dict(res=(32,) * 3))
    yield s
    assert s._ctx is None  # no check needed the device


N = 10
CASES = {
    "cpu_tensor": ("x", lambda: torch.zeros((N, 3), dtype=torch.float32), "'x' is on cpu"),
    "float64": ("v", lambda: torch.zeros((N, 3), dtype=torch.float64), "'v' must be of dtype torch.float32"),
    "int64_ids": ("id", lambda: torch.zeros(N, dtype=torch.int64), "'id' must be of dtype torch.int32"),
    "float_states": ("states", lambda: torch.zeros(N, dtype=torch.float32), "'states' must be of dtype torch.int32"),
    "wrong_width": ("F", lambda: torch.zeros((N, 3), dtype=torch.float32), r"'F' must be of shape \(n, 9\)"),
    "flat_rows": ("x", lambda: torch.zeros(3 * N, dtype=torch.float32), r"'x' must be of shape \(n, 3\)"),
    "three_axes": ("aux", lambda: torch.zeros((N, 1, 1), dtype=torch.float32), "'aux' must be of shape"),
    "gid": ("gid", lambda: torch.zeros(N, dtype=torch.int32), "'gid' cannot be uploaded"),
    "unknown_key": ("mass", lambda: torch.zeros(N, dtype=torch.float32), "unknown field 'mass'"),
    "no_tensor": ("v", lambda: [[0.0, 0.0, 0.0]] * N, "'v' must be a torch.Tensor"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_set_particle_tensors_names_the_key_it_refuses(tm, sim, case):
    key, make, message = CASES[case]
    with pytest.raises(tm.mpm.MPMError, match=message):
        sim.set_particle_tensors({key: make()})


def test_set_particle_tensors_wants_one_row_count(tm, sim):
    with pytest.raises(tm.mpm.MPMError, match="'aux' has 9 rows"):
        sim.set_particle_tensors(dict(v=torch.zeros((N, 3)), aux=torch.zeros(N - 1)))


def test_set_particle_tensors_wants_a_field(tm, sim):
    with pytest.raises(tm.mpm.MPMError, match="no field given"):
        sim.set_particle_tensors({})


def test_get_particle_tensors_judges_the_names_first(tm, sim):
    with pytest.raises(tm.mpm.MPMError, match="unknown field 'mass'"):
        sim.get_particle_tensors(fields=("x", "mass"))
    with pytest.raises(tm.mpm.MPMError, match="no field asked for"):
        sim.get_particle_tensors(fields=())


def test_the_module_imports_without_torch():
    """torch is imported inside the tensor methods only"""
    code = ("import sys\n"
            "sys.modules['torch'] = None\n"  # (import torch now raises ImportError)
            "import taichi_mpm_amd.mpm as m\n"
            "assert hasattr(m.Simulation3D, 'get_particle_tensors')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root, timeout=120)
