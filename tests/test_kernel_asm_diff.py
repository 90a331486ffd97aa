"""tools/kernel_asm_diff.py (no GPU, no compiler): the splitter / normaliser on two short synthetic listings."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_asm_diff", os.path.join(ROOT, "tools", "kernel_asm_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _kernel(name, ordinal, body, vgprs=12):
    return f"""	.protected	{name}
	.globl	{name}
	.p2align	8
	.type	{name},@function
{name}:                                 ; @{name}
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0      ; a comment
.LBB{ordinal}_1:                        ; =>This Inner Loop Header: Depth=1
{body}
	s_cbranch_scc1 .LBB{ordinal}_1
.Ltmp{ordinal}:
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {name}
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr {vgprs}
	.end_amdhsa_kernel
	.text
.Lfunc_end{ordinal}:
	.size	{name}, .Lfunc_end{ordinal}-{name}
                                        ; -- End function
"""


A = "\tv_add_f32_e32 v1, v2, v3"
B = "\tv_mul_f32_e32 v4, v5, v6"
TAIL = """	.type	__hip_cuid_{0},@object
	.globl	__hip_cuid_{0}
__hip_cuid_{0}:
	.byte	0
	.size	__hip_cuid_{0}, 1
	.amdgpu_metadata
---
amdhsa.kernels:
  - .name: {1}
  - .name: {2}
...
	.end_amdgpu_metadata
"""


def test_same_kernels_under_other_ordinals_and_order_compare_equal():
    tool = _tool()
    old = tool.split_kernels(_kernel("_Z3fooPf", 0, A) + _kernel("_Z3barPf", 1, B) + TAIL.format("abc", "_Z3fooPf", "_Z3barPf"))
    new = tool.split_kernels(_kernel("_Z3barPf", 5, B) + _kernel("_Z3fooPf", 7, A + "   ; another comment") + TAIL.format("xyz", "_Z3barPf", "_Z3fooPf"))
    assert sorted(old) == ["_Z3barPf", "_Z3fooPf"]
    assert old["_Z3fooPf"][0] and old["_Z3fooPf"][1], "instruction text and descriptor are both captured"
    assert tool.diff_kernels(old, new) == ([], [], [])


def test_one_changed_instruction_is_reported():
    tool = _tool()
    old = tool.split_kernels(_kernel("_Z3fooPf", 0, A) + _kernel("_Z3barPf", 1, B))
    new = tool.split_kernels(_kernel("_Z3fooPf", 0, A) + _kernel("_Z3barPf", 1, B.replace("v6", "v7")))
    assert tool.diff_kernels(old, new) == ([], [], ["_Z3barPf"])
    assert "v7" in tool.first_difference(old["_Z3barPf"], new["_Z3barPf"])


def test_a_changed_descriptor_is_reported():
    tool = _tool()
    old = tool.split_kernels(_kernel("_Z3fooPf", 0, A))
    new = tool.split_kernels(_kernel("_Z3fooPf", 0, A, vgprs=13))
    assert tool.diff_kernels(old, new) == ([], [], ["_Z3fooPf"])


def test_an_extra_kernel_is_reported():
    tool = _tool()
    old = tool.split_kernels(_kernel("_Z3fooPf", 0, A))
    new = tool.split_kernels(_kernel("_Z3fooPf", 1, A) + _kernel("_Z3bazPf", 0, B))
    assert tool.diff_kernels(old, new) == ([], ["_Z3bazPf"], [])
    assert tool.diff_kernels(new, old) == (["_Z3bazPf"], [], [])


def _template_kernel(name, ordinal, body):
    """a kernel as a template instantiation is listed: the body returns to its own section, named after the symbol, behind the descriptor"""
    text = _kernel(name, ordinal, body)
    own = f'\t.section\t.text.{name},"axG",@progbits,{name},comdat\n'
    return own + text.replace("\t.text\n", own)


def test_a_renamed_kernel_with_the_same_code_is_paired():
    """foo<float> becomes foo<float, true> with the same instructions; bar<float> becomes bar<float, true> with another instruction
    and is not paired; nothing is paired with a kernel that exists on both sides"""
    tool = _tool()
    old = tool.split_kernels(_template_kernel("_Z3fooIfEvPT_", 0, A) + _template_kernel("_Z3barIfEvPT_", 1, B) + _kernel("_Z3bazPf", 2, A))
    new = tool.split_kernels(_template_kernel("_Z3barIfLb1EEvPT_", 3, B.replace("v6", "v7")) + _kernel("_Z3bazPf", 4, A)
                             + _template_kernel("_Z3fooIfLb1EEvPT_", 5, A))
    assert any("_Z3fooIfEvPT_" in line for line in old["_Z3fooIfEvPT_"][0]), "the body names its own symbol"
    only_old, only_new, differ = tool.diff_kernels(old, new)
    assert (only_old, only_new, differ) == (["_Z3barIfEvPT_", "_Z3fooIfEvPT_"], ["_Z3barIfLb1EEvPT_", "_Z3fooIfLb1EEvPT_"], [])
    assert tool.pair_renamed(old, new, only_old, only_new) == [("_Z3fooIfEvPT_", "_Z3fooIfLb1EEvPT_")]


def test_a_rename_with_a_changed_descriptor_is_not_paired():
    tool = _tool()
    old = tool.split_kernels(_template_kernel("_Z3fooIfEvPT_", 0, A))
    new = tool.split_kernels(_template_kernel("_Z3fooIfLb1EEvPT_", 0, A).replace(".amdhsa_next_free_vgpr 12", ".amdhsa_next_free_vgpr 13"))
    assert tool.pair_renamed(old, new, *tool.diff_kernels(old, new)[:2]) == []
