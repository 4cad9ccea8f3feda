"""tools/mfma_reuse.py on a hand-written assembly snippet: MFMA count, accumulator reuse, K-step counts, register counts.
No GPU and no compiler needed."""
import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mfma_reuse", os.path.join(REPO, "tools", "mfma_reuse.py"))
mr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mr)

ASM = """
	.text
	.globl	_ZN3gdx12gemm4_kernelILi2ELi1ELi64ELi3ELb1EEEvNS_10GemmParamsEiiiiPy
_ZN3gdx12gemm4_kernelILi2ELi1ELi64ELi3ELb1EEEvNS_10GemmParamsEiiiiPy: ; @_ZN3gdx12gemm4_kernelILi2ELi1ELi64ELi3ELb1EEEvNS_10GemmParamsEiiiiPy
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mfma_f32_16x16x4_f32 v[0:3], v8, v9, 0
.LBB0_1:                                ;   in Loop: Header=BB0_2 Depth=1
	s_waitcnt lgkmcnt(0)
	s_barrier
	v_mov_b32_e32 v30, v31
.LBB0_2:                                ; =>This Inner Loop Header: Depth=1
	v_add_u32_e32 v20, s2, v21
	v_mfma_f32_16x16x4_f32 v[0:3], v8, v12, v[0:3]
	ds_read_b128 v[22:25], v20 offset:64
	v_mfma_f32_16x16x4_f32 v[4:7], v8, v16, v[4:7]
	v_add_u32_e32 v26, s2, v27
	s_nop 1
	v_mfma_f32_16x16x4_f32 v[4:7], v9, v17, v[4:7]
	; sched_barrier mask(0x00000000)
	v_mfma_f32_16x16x4_f32 v[0:3], v9, v13, v[2:5]
	s_cbranch_scc1 .LBB0_4
; %bb.3:                                ;   in Loop: Header=BB0_2 Depth=1
	v_pk_add_f32 v[0:1], v[0:1], v[10:11]
	s_branch .LBB0_1
.LBB0_4:
	v_mfma_f32_16x16x4_f32 a[0:3], v9, v13, a[0:3]
	v_mfma_f32_16x16x4_f32 a[4:7], v9, v13, a[0:3]
	s_endpgm
.Lfunc_end0:
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _ZN3gdx12gemm4_kernelILi2ELi1ELi64ELi3ELb1EEEvNS_10GemmParamsEiiiiPy
		.amdhsa_next_free_vgpr 32
	.end_amdhsa_kernel
	.text
; Kernel info:
; NumVgprs: 32
; NumAgprs: 8
; TotalNumVgprs: 40
; ScratchSize: 16
	.globl	_ZN3gdx8no_mfmaEv
_ZN3gdx8no_mfmaEv:
	v_add_u32_e32 v0, v0, v1
	s_endpgm
; NumVgprs: 2
; NumAgprs: 0
; ScratchSize: 0
"""


def test_counts_of_the_snippet():
    ks = mr.parse(ASM)
    assert len(ks) == 1, "a function without an MFMA is not listed"
    k = ks[0]
    assert mr.short(k.name) == "gemm4_kernel<2,1,64,3,1>"
    assert (k.mfma, k.mfma_acc) == (7, 2)
    # reuse: v[4:7] twice in a row; v[2:5] overlaps the v[4:7] written just before; a[0:3] read right after it is written.
    # The first loop MFMA reads v[0:3] one MFMA after the prologue wrote it, across a label: counted too (textual order).
    assert k.reuse == 4
    # K step: the inner loop's four MFMAs, one LDS read, the v_add between them (the one in front of the first MFMA and the
    # epilogue's v_pk_add are outside the first-to-last-MFMA span), one s_nop
    assert (k.loop_mfma, k.loop_ds, k.loop_valu, k.loop_nop) == (4, 1, 1, 1)
    assert (k.vgprs, k.agprs, k.scratch) == (32, 8, 16)


def test_no_reuse_two_issues_apart():
    asm = ASM.replace("v_mfma_f32_16x16x4_f32 v[4:7], v9, v17, v[4:7]", "v_mfma_f32_16x16x4_f32 v[0:3], v9, v17, v[0:3]")
    # now v[0:3], v[4:7], v[0:3], then C = v[2:5] right behind D = v[0:3]: one pair in the loop, the label pair, the a[] pair
    assert mr.parse(asm)[0].reuse == 3


def test_report_lists_every_kernel():
    text = mr.report(mr.parse(ASM))
    assert "gemm4_kernel<2,1,64,3,1>" in text and len(text.splitlines()) == 2
