"""MPM<3>::download_device / upload_device of the C++ host layer (include/mpm_amd/mpm.h) against the host path of the same object:
tests/cpp/fields_host_layer.cpp, built here against the library as it lies (a few seconds of g++; nothing is rebuilt when the
program is newer than its sources)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "fields_host_layer.cpp")
CPP_OUT = os.path.join(ROOT, "tests", "cpp", "_build", "fields_host_layer")


def build_cpp():
    from taichi_mpm_amd import _lib
    lib = _lib.lib_path()
    os.makedirs(os.path.dirname(CPP_OUT), exist_ok=True)
    deps = [CPP_SRC, os.path.join(ROOT, "include", "mpm_amd", "mpm.h"), os.path.join(ROOT, "include", "mpmhip.h")]
    if not os.path.exists(CPP_OUT) or any(os.path.getmtime(d) > os.path.getmtime(CPP_OUT) for d in deps):
        libdir = os.path.dirname(lib)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                               "-I", "/opt/rocm/include", CPP_SRC, "-o", CPP_OUT, "-L", libdir, "-lmpmhip", "-L", "/opt/rocm/lib",
                               "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return CPP_OUT


def test_cpp_download_device_and_upload_device_agree_with_the_host_path():
    exe = build_cpp()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.returncode, out.stdout, out.stderr)
    assert int(out.stdout.split()[1]) > 5000
