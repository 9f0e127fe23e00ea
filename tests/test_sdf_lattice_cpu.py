"""What every entry point that takes a sampled field's lattice demands of it (taichi_mpm_amd/csrc/sdf_lattice.h), the header alone
compiled for the host by g++ (tests/cpp/sdf_lattice_host.cpp): the accepting and the refusing cases of both dimensions and the exact
words of every refusal, as a stand-alone program under AddressSanitizer and UBSan.  (The entry points' own prefixes are exercised on
the GPU: tests/test_gpu_sdf.py::test_argument_checks, tests/test_gpu_sdf2d.py::test_every_refusal and the seeding's and the mesh
voxeliser's argument tests.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sdf_lattice_host.cpp")
HDR = os.path.join(ROOT, "taichi_mpm_amd", "csrc", "sdf_lattice.h")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "sdf_lattice_host_san")


def test_every_case_under_the_sanitizers():
    """the runtime is linked statically, so nothing has to be preloaded and nothing that is preloaded comes before it"""
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if not os.path.exists(SAN) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SAN):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", SAN])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout
