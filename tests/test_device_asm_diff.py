"""tools/device_asm_diff.py: the normalise-and-compare core on hand-written assembly (no compile runs)."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _kernel(name, body):
    return f"\t.globl\t{name}\n\t.type\t{name},@function\n{name}:\n{body}\ts_endpgm\n\t.size\t{name}, .-{name}\n"


BODY = "\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\tv_add_f32_e32 v0, v0, v1\n"
HELPER = "\ts_swappc_b64 s[30:31], s[0:1]\n"


def _unit(k_x6, fallback, k_sel, cuid, body=BODY, extra=""):
    """Two kernels, one of which names a device function (as a call does), and the per-compilation symbol."""
    return (_kernel(k_x6, body + f"\ts_getpc_b64 s[0:1]\n\ts_add_u32 s0, s0, {fallback}@rel32@lo+4\n" + HELPER)
            + _kernel(k_sel, BODY) + extra
            + f"\t.globl\t__hip_cuid_{cuid}\n__hip_cuid_{cuid}:\n\t.byte\t0\n"
            + f"\t.amdhsa_kernel {k_x6}\n  - .name: {k_x6}\n    .symbol: {k_x6}.kd\n")


OLD = _unit("_ZN3oaz7k_nn_x6INS_5X6CfgILi0EEEEEvPK9oaz_stateiPKfiPfS7_NS_7TileMapE",
            "_ZN3oaz14nn_h3_fallbackINS_5X6CfgILi0EEELi3EEEvPK9oaz_stateNS_8TileSpanEPKfiPfS8_S8_",
            "_ZN3oaz12k_select_segENS_8TreeViewEPK9oaz_statePKhPKdNS_12SearchParamsE", "1a2b3c")


def test_normalise_and_compare():
    sys.path.insert(0, str(ROOT / "tools"))
    from device_asm_diff import compare

    # the same code under other mangled names (a template parameter gone, substitution indices shifted) and
    # another __hip_cuid_: equal
    new = _unit("_ZN3oaz7k_nn_x6INS_5X6CfgEEEvPK9oaz_stateiPKfiPfS6_NS_7TileMapE",
                "_ZN3oaz14nn_h3_fallbackINS_5X6CfgELi3EEEvPK9oaz_stateNS_8TileSpanEPKfiPfS7_S7_",
                "_ZN3oaz12k_select_segENS_8TreeViewEPK9oaz_statePKhPKdNS_12SearchParamsE", "9f8e7d")
    assert new != OLD and compare(OLD, new) is None
    assert compare(OLD, OLD) is None
    # two names exchanged are not the same code: the numbering follows the first appearance
    swapped = _unit("_ZN3oaz7k_nn_x6INS_5X6CfgEEEvPK9oaz_stateiPKfiPfS6_NS_7TileMapE",
                    "_ZN3oaz7k_nn_x6INS_5X6CfgEEEvPK9oaz_stateiPKfiPfS6_NS_7TileMapE",
                    "_ZN3oaz12k_select_segENS_8TreeViewEPK9oaz_statePKhPKdNS_12SearchParamsE", "9f8e7d")
    assert compare(OLD, swapped) is not None
    # one changed instruction: different, and the report shows the line of both sides
    changed = new.replace("v_add_f32_e32 v0, v0, v1", "v_mul_f32_e32 v0, v0, v1", 1)
    report = compare(OLD, changed)
    assert report is not None and "normalised line 5 " in report
    assert "old| \tv_add_f32_e32 v0, v0, v1" in report and "new| \tv_mul_f32_e32 v0, v0, v1" in report
    # a kernel added, or removed: different
    added = _unit("_ZN3oaz7k_nn_x6INS_5X6CfgEEEvPK9oaz_stateiPKfiPfS6_NS_7TileMapE",
                  "_ZN3oaz14nn_h3_fallbackINS_5X6CfgELi3EEEvPK9oaz_stateNS_8TileSpanEPKfiPfS7_S7_",
                  "_ZN3oaz12k_select_segENS_8TreeViewEPK9oaz_statePKhPKdNS_12SearchParamsE", "9f8e7d",
                  extra=_kernel("_ZN3oaz8k_selectENS_8TreeViewE", BODY))
    assert compare(OLD, added) is not None and compare(added, OLD) is not None
    # a kernel added at the very end (one side a prefix of the other): different
    assert compare(OLD, OLD + _kernel("_ZN3oaz8k_selectENS_8TreeViewE", BODY)) is not None


def _function(name, index, body=BODY):
    """A function as the compiler prints it: its section, the "Begin function" line, labels numbered by the
    function's place in the unit."""
    return (f"\t.text\n\t.protected\t{name} ; -- Begin function {name}\n\t.globl\t{name}\n{name}:\n{body}"
            f"\ts_cbranch_execz .LBB{index}_2\n.LBB{index}_2:{' ' * (12 - len(str(index)))}; in Loop: Header=BB{index}_2\n"
            f"\ts_endpgm\n.Lfunc_end{index}:\n\t.size\t{name}, .Lfunc_end{index}-{name}\n")


def _meta(name, nargs):
    return "  - .args:\n" + "      - .offset: 0\n" * nargs + f"    .name:           {name}\n    .symbol:         {name}.kd\n"


def _whole(functions):
    """functions: [(symbol, body, kernel arguments)]"""
    return ("\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n"
            + "".join(_function(n, i, b) for i, (n, b, _) in enumerate(functions))
            + "\t.text\n\t.p2alignl 6, 3212836864\n\t.amdgpu_metadata\n---\namdhsa.kernels:\n"
            + "".join(_meta(n, k) for n, _, k in functions) + "amdhsa.target: x\n...\n\t.end_amdgpu_metadata\n")


def test_per_function_report():
    sys.path.insert(0, str(ROOT / "tools"))
    from device_asm_diff import compare, compare_functions, function_key

    assert function_key("_ZN2tr8k_gatherEPK10oaz_samplePKiS4_iiPfS5_S5_") == "tr::k_gather"
    assert function_key("_ZN2tr6k_convILi1ELi4ELi2EEEvNS_8ConvArgsE") == "tr::k_conv<1,4,2>"
    assert function_key("k_bn_stats_io") == "k_bn_stats_io"
    old = _whole([("_ZN2tr8k_gatherEPKiS1_i", BODY, 3), ("_ZN2tr11k_set_batchEPiii", BODY, 3),
                  ("_ZN2tr6k_convILi0ELi2ELi1EEEvNS_8ConvArgsE", BODY, 1),
                  ("_ZN2tr6k_convILi0ELi2ELi2EEEvNS_8ConvArgsE", BODY, 1), ("_ZN2tr5k_sgdEPf", BODY, 1),
                  ("_ZN2tr6k_packEPf", BODY, 1)])
    # a kernel and a template instance gone (so every later function's labels are renumbered), one signature and
    # one instruction changed, one argument layout changed under the same name, one kernel added
    new = _whole([("_ZN2tr8k_gatherEPKii", BODY.replace("v_add", "v_sub"), 2),
                  ("_ZN2tr6k_convILi0ELi2ELi2EEEvNS_8ConvArgsE", BODY, 1), ("_ZN2tr5k_sgdEPf", BODY, 2),
                  ("_ZN2tr6k_packEPf", BODY, 1), ("_ZN2tr5k_newEPf", BODY, 1)])
    assert compare(old, new) is not None
    assert compare_functions(old, new) == [
        ("tr::k_gather", "different"), ("tr::k_set_batch", "only in old"), ("tr::k_conv<0,2,1>", "only in old"),
        ("tr::k_conv<0,2,2>", "identical"), ("tr::k_sgd", "different"), ("tr::k_pack", "identical"),
        ("(rest of unit)", "identical"), ("tr::k_new", "only in new")]
    assert all(v == "identical" for _, v in compare_functions(old, old))
