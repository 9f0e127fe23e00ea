"""The host's arithmetic over the container store of a resident asynchronous stepper (taichi_mpm_amd/csrc/async_sched.h:
AsyncStoreCount — one struct for AsyncMPM<3> and AsyncMPM<2>), the header alone compiled for the host by g++
(tests/cpp/async_store_host.cpp): folding a read-back into live / size / size_ub (n_freed > live included), the compaction rule
on both sides of both clauses, the growth sizes at 0, 1, 4095 / 4096 and near 2^32 — as a stand-alone program under
AddressSanitizer and UBSan.  (The store itself runs on the GPU: tests/test_gpu_async.py, tests/test_gpu_async2d.py,
tests/test_gpu_lifetime.py.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "async_store_host.cpp")
HDR = os.path.join(ROOT, "taichi_mpm_amd", "csrc", "async_sched.h")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "async_store_host_san")


def test_every_case_under_the_sanitizers():
    """the runtime is linked statically, so nothing has to be preloaded and nothing that is preloaded comes before it"""
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if not os.path.exists(SAN) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SAN):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", SAN])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout
