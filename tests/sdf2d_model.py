"""The 2D side of the sampler tests: the model is tests/sdf_model.py's at D = 2; here are the lattice, the key-frame times and the
fields of tests/test_gpu_sdf2d.py::test_device_sampler_matches_the_model and of its CPU companion
(tests/test_sdf2d_cpu.py::test_the_sampler_tests_fields_are_well_conditioned): a shifted origin, a spacing that is not dx."""
import numpy as np

from tests.sdf_model import SdfModel as Sdf2DModel  # noqa: F401  (the dimension comes from phi0.ndim)

RES1, ORG1, H1 = (83, 77), (-0.1, 0.02), 0.013
T0, T1, TIMES = 0.5, 2.0, (0.7, 1.25, 1.9)


def sampler_fields():
    line = lambda n, d: (lambda x: x @ np.asarray(n, np.float64) + d)
    disc = lambda c, r: (lambda x: np.linalg.norm(x - np.asarray(c, np.float64), axis=1) - r)
    ring = lambda c, R, w: (lambda x: np.abs(np.linalg.norm(x - np.asarray(c, np.float64), axis=1) - R) - w)
    return {"line": (line((0.6, 0.8), -0.6), line((0.6, 0.8), -0.63)),
            "disc": (disc((0.4, 0.5), 0.3), disc((0.42, 0.5), 0.33)),
            "ring": (ring((0.42, 0.5), 0.3, 0.08), ring((0.42, 0.52), 0.31, 0.09))}
