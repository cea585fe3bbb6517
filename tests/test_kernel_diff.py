"""tools/kernel_diff.py on two tiny synthetic assembly texts (CPU, text only)."""
import importlib.util
from pathlib import Path

_spec = importlib.util.spec_from_file_location(
    "kernel_diff", Path(__file__).resolve().parents[1] / "tools" / "kernel_diff.py")
kernel_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kernel_diff)

ASM = """
_ZN3m3d3fooEPf:                         ; @_ZN3m3d3fooEPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[0:1], 0x0
	s_cbranch_execz .LBB{fn}_{lab}
	v_mov_b32_e32 v0, 0                     ; a comment
.LBB{fn}_{lab}:
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _ZN3m3d3fooEPf
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr {vgpr}
		.amdhsa_next_free_sgpr 8
	.end_amdhsa_kernel
	.text
.Lfunc_end{fn}:
"""


def test_renumbered_label_is_same():
    out, rc = kernel_diff.compare(ASM.format(fn=3, lab=7, vgpr=4), [ASM.format(fn=0, lab=2, vgpr=4)])
    assert out == ["same  _ZN3m3d3fooEPf"] and rc == 0


def test_vgpr_count_is_descriptor_diff():
    out, rc = kernel_diff.compare(ASM.format(fn=3, lab=7, vgpr=4), [ASM.format(fn=3, lab=7, vgpr=5)])
    assert len(out) == 1 and out[0].startswith("DESCRIPTOR-DIFF  _ZN3m3d3fooEPf")
    assert "next_free_vgpr 4 -> 5" in out[0] and rc != 0


def test_missing_unless_removed():
    base = ASM.format(fn=3, lab=7, vgpr=4)
    assert kernel_diff.compare(base, [""]) == (["missing  _ZN3m3d3fooEPf"], 1)
    assert kernel_diff.compare(base, [""], removed=["foo"]) == (["removed  _ZN3m3d3fooEPf"], 0)


_BAR = "_ZN3m3d3barILi1EEEvPf"


def test_renamed_with_identical_stream_is_same():
    base = ASM.format(fn=3, lab=7, vgpr=4)
    new = ASM.format(fn=0, lab=2, vgpr=4).replace("_ZN3m3d3fooEPf", _BAR)
    assert kernel_diff.compare(base, [new], renamed=[("_ZN3m3d3fooEPf", _BAR)]) == ([f"same  {_BAR}"], 0)
    # without the option the kernel escapes the comparison: one missing, one new
    out, rc = kernel_diff.compare(base, [new])
    assert sorted(out) == ["missing  _ZN3m3d3fooEPf", f"new  {_BAR}"] and rc == 1


def test_renamed_to_an_absent_symbol_fails():
    base = ASM.format(fn=3, lab=7, vgpr=4)
    out, rc = kernel_diff.compare(base, [base], renamed=[("_ZN3m3d3fooEPf", _BAR)])
    assert rc != 0 and out[0].startswith(f"missing  {_BAR}")
