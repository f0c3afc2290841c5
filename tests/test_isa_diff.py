"""The parser and the comparison of tools/isa_diff.py on short synthetic assembly texts (no compiler): what it strips,
what it reports for identical kernels, for one operand changed and for a kernel that is missing."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _asm(fn, cuid, second_operand="v1", with_b=True, comment="first"):
    a = f"""\t.text
\t.protected\tk_a ; -- Begin function k_a
\t.globl\tk_a
\t.p2align\t8
\t.type\tk_a,@function
k_a:                                    ; @k_a
; %bb.0:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0   ; {comment}
\tv_add_f64 v[0:1], v[0:1],   {second_operand}
\ts_cbranch_scc1 .LBB{fn}_2
.LBB{fn}_1:
\ts_getpc_b64 s[4:5]
\ts_add_u32 s4, s4, __hip_cuid_{cuid}@rel32@lo+4
.LBB{fn}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel k_a
\t\t.amdhsa_next_free_vgpr 2
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn}:
\t.size\tk_a, .Lfunc_end{fn}-k_a
"""
    b = f"""\t.type\tk_b,@function
k_b:
\ts_endpgm
.Lfunc_end{fn + 1}:
"""
    tail = f"\t.type\t__hip_cuid_{cuid},@object\n__hip_cuid_{cuid}:\n\t.byte\t0\n"
    return a + (b if with_b else "") + tail


def test_parser_strips_comments_directives_label_numbers_and_the_cuid():
    t = _tool()
    k = t.parse_kernels(_asm(0, "1945e19d54e7444d"))
    assert sorted(k) == ["k_a", "k_b"]
    assert k["k_a"] == ["s_load_dwordx2 s[0:1], s[0:1], 0x0", "v_add_f64 v[0:1], v[0:1], v1", "s_cbranch_scc1 .LBB_2", ".LBB_1:",
                        "s_getpc_b64 s[4:5]", "s_add_u32 s4, s4, __hip_cuid@rel32@lo+4", ".LBB_2:", "s_endpgm"]
    assert k["k_b"] == ["s_endpgm"]
    assert len(t.instructions(k["k_a"])) == 6 and t.opcodes(k["k_a"])[:2] == ["s_load_dwordx2", "v_add_f64"]


def test_identical_kernels_under_other_numbering_cuid_and_comments():
    t = _tool()
    a, b = t.parse_kernels(_asm(0, "1945e19d54e7444d")), t.parse_kernels(_asm(7, "00ff00ff00ff00ff", comment="second"))
    assert t.diff_kernels(a, b) == []
    lines, n = t.report(a, b)
    assert n == 0 and lines == ["2 kernels, 0 differ"]


def test_one_operand_changed():
    t = _tool()
    a, b = t.parse_kernels(_asm(0, "aa")), t.parse_kernels(_asm(0, "aa", second_operand="v3"))
    assert t.diff_kernels(a, b) == [("k_a", 6, 6, True)]
    lines, n = t.report(a, b)
    assert n == 1 and lines == ["DIFFERS  k_a: 6 -> 6 instructions, same opcode sequence", "2 kernels, 1 differ"]
    c = dict(b, k_a=b["k_a"][:1] + ["v_mul_f64 v[0:1], v[0:1], v3"] + b["k_a"][2:])
    assert t.diff_kernels(a, c) == [("k_a", 6, 6, False)]
    assert t.report(a, c)[0][0].endswith("other opcode sequence")


def test_one_kernel_missing():
    t = _tool()
    a, b = t.parse_kernels(_asm(0, "aa")), t.parse_kernels(_asm(0, "aa", with_b=False))
    assert t.diff_kernels(a, b) == [("k_b", 1, None, False)]
    assert t.diff_kernels(b, a) == [("k_b", None, 1, False)]
    lines, n = t.report(a, b)
    assert n == 1 and lines == ["DIFFERS  k_b: 1 -> - instructions, missing in B", "2 kernels, 1 differ"]
