"""Which GPU test runs which instantiation of the transfer kernels against the oracle or the reference's recorded output.

A FORM is (family, material set, store_b, rigid, packed): what taichi_mpm_amd/csrc/launch_plan.h (plan_g2p / plan_p2g) can answer
and mpmhip.hip (g2p_kernel_of, g2p_packed_kernel, rigid_p2g_kernel, rigid_g2p_kernel) turns into a kernel pointer.  The material
set is a material's name (the one-material kernel), "NO_VISCO", "ALL" or "ALL_DET"; store_b is None for the families that are
not instantiated per STORE_B.  MANIFEST maps every form to the id of one GPU test that compares its output with the CPU oracle
(oracle/) or with a committed fixture of the reference's output, and that test calls assert_runs() before it compares numbers:
a ctx that was given another kernel than the test means to cover fails there.  tests/test_launch_plan_cpu.py enumerates the
forms the plans can answer on the host and holds them against this table, so a form routed into launch_plan.h without a GPU
case behind it fails without a GPU."""

MATS = ("jelly", "snow", "sand", "water", "linear", "elastic", "von_mises", "visco")
PACKED_MATS = MATS[:-1]  # (no packed instantiation for visco: launch_plan.h, plan_g2p)


def forms_of(plan):
    """the forms a substep launches on a ctx whose Simulation.transfer_kernels() answered `plan`"""
    kind, name = plan["mats"]
    mats = name if kind == "ONE" else kind
    if plan["packed"]:
        out = {("k_g2p_packed", mats, False, False, True)}
    else:
        out = {("k_g2p", mats, plan["store_b"], plan["rigid"], False)}
    kind, name = plan["rigid_mats"]
    rmats = name if kind == "ONE" else kind
    if plan["rigid"]:
        out.add(("k_g2p_rigid", rmats, None, True, False))
    if plan["p2g_rigid"]:
        out.add(("k_p2g_rigid", rmats, None, True, False))
    return out


def assert_runs(sim, *forms):
    """the next substep of `sim` launches exactly these forms (every particle group and body has to be added before)"""
    got = forms_of(sim.transfer_kernels())
    assert got == set(forms), (sorted(got, key=str), sorted(forms, key=str))


def g2p(mats, store_b=False, rigid=False):
    return ("k_g2p", mats, store_b, rigid, False)


def packed(mat):
    return ("k_g2p_packed", mat, False, False, True)


def beside_a_body(mats):
    """the two colour-aware kernels of a ctx with a body"""
    return ("k_p2g_rigid", mats, None, True, False), ("k_g2p_rigid", mats, None, True, False)


PARITY, CPIC = "tests/test_gpu_parity.py::", "tests/test_gpu_cpic.py::"
# the one-material scenes beside a body: three cases of the first fixture (ref_cpic.npz), five of ref_cpic_materials.npz
_BODY_CASE = {"jelly": "test_substeps_with_a_rigid_body_match_the_reference[box_jelly]",
              "sand": "test_substeps_with_a_rigid_body_match_the_reference[plate_sand]",
              "water": "test_substeps_with_a_rigid_body_match_the_reference[box_water]"}
for _m in ("snow", "linear", "elastic", "von_mises", "visco"):
    _BODY_CASE[_m] = "test_cpic_substeps_match_the_reference_for_every_material[box_%s]" % _m

MANIFEST = []  # rows (form, test id)
for _m in MATS:
    MANIFEST.append((g2p(_m), PARITY + "test_g2p_from_identical_grid_matches_oracle[%s-apic_b_folded]" % _m))
    MANIFEST.append((g2p(_m, rigid=True), CPIC + _BODY_CASE[_m]))
    MANIFEST.append((beside_a_body(_m)[0], CPIC + _BODY_CASE[_m]))
    MANIFEST.append((beside_a_body(_m)[1], CPIC + _BODY_CASE[_m]))
for _m in PACKED_MATS:
    MANIFEST.append((packed(_m), PARITY + "test_packed_g2p_from_identical_grid_matches_oracle[%s]" % _m))
for _set, _scene in (("NO_VISCO", "mixed7"), ("ALL", "mixed8")):
    MANIFEST += [
        (g2p(_set, store_b=False), PARITY + "test_mixed_g2p_from_identical_grid_matches_oracle[%s-apic_b_folded]" % _scene),
        (g2p(_set, store_b=True), PARITY + "test_mixed_g2p_from_identical_grid_matches_oracle[%s-apic_b_stored]" % _scene),
        (g2p(_set, store_b=False, rigid=True), CPIC + "test_cpic_mixed_materials_match_the_reference[box_%s-default]" % _scene),
        (g2p(_set, store_b=True, rigid=True), CPIC + "test_cpic_mixed_materials_match_the_reference[box_%s-keep_apic_b]" % _scene),
    ]
MANIFEST += [
    (beside_a_body("ALL")[0], CPIC + "test_cpic_mixed_materials_match_the_reference[box_mixed8-default]"),
    (beside_a_body("ALL")[1], CPIC + "test_cpic_mixed_materials_match_the_reference[box_mixed8-default]"),
    (beside_a_body("ALL_DET")[0], CPIC + "test_cpic_mixed_materials_match_the_reference[box_mixed8-deterministic]"),
    (beside_a_body("ALL_DET")[1], CPIC + "test_cpic_mixed_materials_match_the_reference[box_mixed8-deterministic]"),
]
