"""Which kernel instantiation each phase of a substep launches, and with how many workgroups (taichi_mpm_amd/csrc/launch_plan.h:
Knobs, Facts, plan_sort / plan_p2g / plan_grid / plan_g2p) compiled for the host by g++, the header alone: no HIP header is included,
no HIP runtime linked or loaded (tests/cpp/launch_plan_host.cpp).  The scenarios restate every rule and compare it with the header's
answer at both sides of each boundary: slot counts around 2 M and 6 M, block fills around 448 per block, owner counts, material
masks, every boolean fact, every environment switch unset, inside and outside its clamp.  The same source, with its main(), runs
once as a program of its own under AddressSanitizer and UBSan.  No GPU needed: the GPU suite checks what the kernels compute,
this checks that the intended ones are launched — and, against tests/kernel_forms.py, that every form of the transfer kernels
the plans can answer has a GPU test that compares it with the oracle or the reference."""
import ctypes as C
import importlib
import inspect
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "launch_plan_host.cpp")
HDR = os.path.join(ROOT, "taichi_mpm_amd", "csrc", "launch_plan.h")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "liblaunch_plan_host.so")
SAN = os.path.join(ROOT, "tests", "cpp", "_build", "launch_plan_host_san")


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(out)


def host_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", SRC, "-o", OUT])
    return C.CDLL(OUT)


def test_the_test_library_does_not_pull_in_the_hip_runtime():
    host_lib()
    needed = subprocess.check_output(["readelf", "-d", OUT], text=True)
    assert "amdhip64" not in needed and "libhsa" not in needed, needed


@pytest.mark.parametrize("scenario", ["lp_env", "lp_sort", "lp_p2g", "lp_grid", "lp_g2p", "lp_known_configurations", "lp_transfer_words", "lp_scan_grid"])
def test_plan(scenario):
    """lp_env: Knobs::from_env, today's defaults and clamps, nothing cached between two reads.  lp_sort: keyed front, blocks per
    chunk, owner list, rank and cell-order launches.  lp_p2g: launch sizes and the colour-aware kernel's material set.  lp_grid:
    the walk, its launch size, the sampled instantiation, the refusal of calculate_energy on a tiled ctx without the owner list.
    lp_g2p: packed or per block, material set, launch sizes.  lp_known_configurations: the plans of the measured configurations,
    written out by hand.  lp_transfer_words: the eight words of mpmhip_debug_transfer_plan by hand.  A scenario returns the line of its first failed check in tests/cpp/launch_plan_host.cpp."""
    assert getattr(host_lib(), scenario)() == 0


def test_every_scenario_under_the_sanitizers():
    """the same source as a stand-alone program (its main() runs every scenario) built with -fsanitize=address,undefined; the
    runtime is linked statically, so nothing has to be preloaded and nothing that is preloaded comes before it"""
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if _stale(SAN):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", SAN])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "scenarios ok" in r.stdout, r.stdout


def enumerate_forms():
    """{form: one (mask, slots, fill, flags, knob) that gives it}: the header's plans swept over every single-material mask, mixed
    masks without and with visco, every combination of rigid / store_b / tiled / deterministic / chunk table, MPMHIP_G2P_PACKED
    unset, 0 and 1, and slot counts and block fills at both sides of the size rule of the packed walk"""
    from taichi_mpm_amd import MATERIAL_IDS
    from taichi_mpm_amd.mpm import transfer_plan
    from tests import kernel_forms as kf
    lib = host_lib()
    lib.lp_transfer_plan.argtypes = [C.c_uint32, C.c_int64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    lib.lp_transfer_plan.restype = None
    bit = {m: 1 << MATERIAL_IDS[m] for m in kf.MATS}
    masks = [bit[m] for m in kf.MATS]
    masks += [bit["sand"] | bit["elastic"], sum(bit[m] for m in kf.PACKED_MATS), bit["sand"] | bit["visco"], sum(bit.values())]
    small = 2 << 20  # lp::SMALL_SLOTS
    sizes = [(4059, 0, 0), (4059, 4059, 30), (small - 1, small - 1, 8000), (small, 0, 0), (small, small, 8000), (small, small, 4096),
             (8 << 20, 8 << 20, 24000), (8 << 20, 8 << 20, 16384)]
    found = {}
    for mask, (slots, live, act), flags, knob in itertools.product(masks, sizes, range(32), (-1, 0, 1)):
        words = (C.c_int32 * 8)()
        lib.lp_transfer_plan(mask, slots, live, act, flags, knob, words)
        for form in kf.forms_of(transfer_plan(list(words))):
            found.setdefault(form, (mask, slots, live, act, flags, knob))
    return found


def test_every_form_the_plans_can_answer_has_a_gpu_test_against_the_oracle():
    """tests/kernel_forms.py: one row per form, no form without a row, no row for a form the plans never answer; the test a row
    names exists, carries the row's case among its parameters, and asserts the form it runs (kernel_forms.assert_runs)"""
    from tests import kernel_forms as kf
    found = enumerate_forms()
    rows = [form for form, _ in kf.MANIFEST]
    assert len(set(rows)) == len(rows)
    assert not set(found) - set(rows), "forms without a GPU test: %s" % sorted(set(found) - set(rows), key=str)
    assert not set(rows) - set(found), "rows no ctx can reach: %s" % sorted(set(rows) - set(found), key=str)
    # the count by hand: k_g2p 8 materials x RIGID + {NO_VISCO, ALL} x STORE_B x RIGID, k_g2p_packed 7, the colour-aware pair 10 each
    by_family = {fam: sum(1 for f in rows if f[0] == fam) for fam in ("k_g2p", "k_g2p_packed", "k_p2g_rigid", "k_g2p_rigid")}
    assert by_family == {"k_g2p": 24, "k_g2p_packed": 7, "k_p2g_rigid": 10, "k_g2p_rigid": 10}
    for form, test_id in kf.MANIFEST:
        path, _, name = test_id.partition("::")
        name, _, case = name.partition("[")
        mod = importlib.import_module(path[:-3].replace("/", "."))
        fn = getattr(mod, name, None)
        assert callable(fn) and mod.pytestmark.name == "gpu", test_id
        ids = set()
        for mark in getattr(fn, "pytestmark", []):
            if mark.name == "parametrize":
                given = mark.kwargs.get("ids")
                ids |= set(given if given is not None else [str(v) for v in mark.args[1]])
        # (an id joins the parameters of the stacked marks with "-"; no single id of these tests contains one)
        assert case.endswith("]") and set(case[:-1].split("-")) <= ids, (test_id, sorted(ids))
        assert "assert_runs(" in inspect.getsource(fn), test_id
