"""scripts/isa_same.py on pairs of tiny hand-written assembly texts (two
kernels each): equal up to comments and the cuid symbol, one swapped
v_add_f32_e32, one extra v_mov_b32, one kernel renamed (--pair). No GPU and no
compiler."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_same", os.path.join(ROOT, "scripts", "isa_same.py"))
isa_same = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_same)


def unit(add, extra="", note="first build", cuid="0123abcd", vgpr=6):
    return f"""\t.text
\t.globl\t_Z4axpyPf
_Z4axpyPf:                              ; @_Z4axpyPf
; %bb.0:                                ; {note}
\ts_load_dwordx2 s[0:1], s[0:1], 0x0
.LBB0_1:                                ; =>This Inner Loop Header
\tv_mul_f32_e32 v1, 2.0, v0
\t{add}
{extra}\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
\t.amdhsa_kernel _Z4axpyPf
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
\t.globl\t_Z4copyPf
_Z4copyPf:                              ; @_Z4copyPf
\tv_mov_b32_e32 v0, 0                     ; {note}
\tglobal_store_dword v0, v0, s[0:1]
\ts_endpgm
\t.amdhsa_kernel _Z4copyPf
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr 1
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
\t.globl\t__hip_cuid_{cuid}
__hip_cuid_{cuid}:
\t.byte\t0
"""


BASE = unit("v_add_f32_e32 v2, v1, v3")
RECOMPILED = unit("v_add_f32_e32 v2, v1, v3", note="second build", cuid="89ef4567")
SWAPPED = unit("v_add_f32_e32 v2, v3, v1")
EXTRA = unit("v_add_f32_e32 v2, v1, v3", extra="\tv_mov_b32_e32 v4, v2\n")


def run(tmp_path, capsys, other, *flags):
    for d, text in (("a", BASE), ("b", other)):
        os.makedirs(tmp_path / d, exist_ok=True)
        (tmp_path / d / "unit.s").write_text(text)
    status = isa_same.main([str(tmp_path / "a"), str(tmp_path / "b"), *flags])
    return status, capsys.readouterr().out


def kinds(other):
    path = {}
    for name, text in (("a", BASE), ("b", other)):
        lines = text.splitlines()
        path[name] = {s: isa_same.normalised(lines[i:j + 1]) for s, i, j in isa_same.kernel_spans(lines)}
    assert sorted(path["a"]) == sorted(path["b"]) == ["_Z4axpyPf", "_Z4copyPf"]
    return {s: isa_same.classify(path["a"][s], path["b"][s]) for s in path["a"]}


def test_comments_and_cuid_do_not_count(tmp_path, capsys):
    assert kinds(RECOMPILED) == {"_Z4axpyPf": "identical", "_Z4copyPf": "identical"}
    status, out = run(tmp_path, capsys, RECOMPILED)
    assert status == 0
    assert out.splitlines() == ["unit.s: 2 kernels: 2 identical, 0 operand-order, 0 different, 0 only in A, 0 only in B"]


def test_swapped_sources_need_the_flag(tmp_path, capsys):
    assert kinds(SWAPPED) == {"_Z4axpyPf": "operand-order", "_Z4copyPf": "identical"}
    status, out = run(tmp_path, capsys, SWAPPED)
    assert status == 1
    assert "1 identical, 1 operand-order, 0 different" in out and "vgpr 6 -> 6" in out
    assert run(tmp_path, capsys, SWAPPED, "--allow-operand-order", "copy")[0] == 1  # names another kernel
    assert run(tmp_path, capsys, SWAPPED, "--allow-operand-order", "axpy")[0] == 0


def test_extra_instruction_is_different(tmp_path, capsys):
    assert kinds(EXTRA) == {"_Z4axpyPf": "different", "_Z4copyPf": "identical"}
    status, out = run(tmp_path, capsys, EXTRA)
    assert status == 1
    assert "1 identical, 0 operand-order, 1 different" in out and "v_mov_b32_e32 0 -> 1" in out
    assert run(tmp_path, capsys, EXTRA, "--allow-operand-order", "axpy")[0] == 1


# A build that renames one kernel (axpy gains a template argument): --pair keys
# it by the regex's groups and hides its own symbol inside its body.
RENAMED = BASE.replace("_Z4axpyPf", "_Z4axpyIfEvPT_")
RENAMED_EXTRA = EXTRA.replace("_Z4axpyPf", "_Z4axpyIfEvPT_")


def test_a_renamed_kernel_pairs_only_with_the_option(tmp_path, capsys):
    status, out = run(tmp_path, capsys, RENAMED)
    assert status == 1
    assert "1 identical, 0 operand-order, 0 different, 1 only in A, 1 only in B" in out
    status, out = run(tmp_path, capsys, RENAMED, "--pair", "(axpy)")
    assert status == 0
    assert out.splitlines() == ["unit.s: 2 kernels: 2 identical, 0 operand-order, 0 different, 0 only in A, 0 only in B"]


def test_an_ambiguous_pair_is_an_error(tmp_path, capsys):
    status, out = run(tmp_path, capsys, RENAMED, "--pair", "(p)")  # axpy and copy both key as ("p",)
    assert status == 2 and "the same key" in out
    assert run(tmp_path, capsys, RENAMED, "--pair", "axpy|copy")[0] == 2  # no groups: every match keys as ()


def test_a_paired_kernel_with_an_extra_instruction_is_different(tmp_path, capsys):
    status, out = run(tmp_path, capsys, RENAMED_EXTRA, "--pair", "(axpy)")
    assert status == 1
    assert "1 identical, 0 operand-order, 1 different, 0 only in A, 0 only in B" in out and "v_mov_b32_e32 0 -> 1" in out


def test_swap_with_other_registers_or_counts_is_different():
    assert kinds(unit("v_add_f32_e32 v2, v3, v1", vgpr=7))["_Z4axpyPf"] == "different"
    assert kinds(unit("v_add_f32_e32 v2, v3, v0"))["_Z4axpyPf"] == "different"
    assert kinds(unit("v_sub_f32_e32 v2, v3, v1"))["_Z4axpyPf"] == "different"
