"""CPU: the loop view of tools/qp_insn_static.py (loop_stats: the exec regions of a kernel's main loop, DESIGN §3.3
"Lane guards and spill reloads") on a short assembly text.  No compile is involved."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The compiler's layout of one outer loop (header BB0_2) around an inner one (BB0_5), with a guarded region before the
# outer loop, a rolled loop after it (BB0_8) that must not be counted, and a block of the outer loop laid out of line
# behind the kernel's end (BB0_9) that must be.  In the outer loop: five exec regions, four under s[4:5] and one under
# vcc; two of them open directly after the previous one closed.
ASM = """
_Z6kernelv:
; %bb.0:
\ts_load_dwordx2 s[0:1], s[2:3], 0x0
\tv_cmp_gt_u32_e64 s[4:5], 49, v0
\ts_and_saveexec_b64 s[6:7], s[4:5]
\tv_readlane_b32 s9, v40, 3
\ts_or_b64 exec, exec, s[6:7]
\tv_writelane_b32 v40, s8, 0
.LBB0_2:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_5 Depth 2
\tv_readlane_b32 s8, v40, 0
\ts_nop 1
\ts_and_saveexec_b64 s[6:7], s[4:5]
\ts_cbranch_execz .LBB0_4
; %bb.3:                                ;   in Loop: Header=BB0_2 Depth=1
\tv_fma_f64 v[2:3], v[4:5], v[6:7], v[2:3]
\tv_accvgpr_read_b32 v8, a9
.LBB0_4:                                ;   in Loop: Header=BB0_2 Depth=1
\ts_or_b64 exec, exec, s[6:7]
\ts_and_saveexec_b64 s[6:7], s[4:5]
\tv_accvgpr_write_b32 a9, v8
\ts_or_b64 exec, exec, s[6:7]
\tv_cmp_lt_f64_e32 vcc, 0, v[2:3]
\ts_and_saveexec_b64 s[10:11], vcc
\ts_cbranch_execnz .LBB0_9
.LBB0_5:                                ;   Parent Loop BB0_2 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\tv_add_f64 v[2:3], v[2:3], v[2:3]
\ts_add_i32 s12, s12, -1
\ts_cmp_lg_u32 s12, 0
\ts_cbranch_scc1 .LBB0_5
; %bb.6:                                ;   in Loop: Header=BB0_2 Depth=1
\ts_or_b64 exec, exec, s[10:11]
\ts_and_saveexec_b64 s[6:7], s[4:5]
\tv_readlane_b32 s13, v40, 1
\ts_or_b64 exec, exec, s[6:7]
\ts_add_i32 s14, s14, 1
\ts_cmp_lt_i32 s14, 60
\ts_cbranch_scc1 .LBB0_2
; %bb.7:
\ts_mov_b32 s15, 0
.LBB0_8:                                ; =>This Inner Loop Header: Depth=1
\ts_and_saveexec_b64 s[6:7], s[4:5]
\tv_readlane_b32 s16, v40, 2
\ts_or_b64 exec, exec, s[6:7]
\ts_add_i32 s15, s15, 1
\ts_cmp_lt_i32 s15, 4
\ts_cbranch_scc1 .LBB0_8
; %bb.10:
\ts_endpgm
.LBB0_9:                                ;   in Loop: Header=BB0_2 Depth=1
\ts_and_saveexec_b64 s[12:13], s[4:5]
\tv_accvgpr_read_b32 v9, a10
\ts_or_b64 exec, exec, s[12:13]
\ts_branch .LBB0_5
"""


def _tool():
    spec = importlib.util.spec_from_file_location("qp_insn_static", os.path.join(ROOT, "tools", "qp_insn_static.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_loop_stats_counts_the_outer_loop():
    s = _tool().loop_stats(ASM.splitlines())
    assert s["exec_regions"] == 5
    assert s["regions_by_mask"] == {"s[4:5]": 4, "vcc": 1}
    assert s["reopen_after_close"] == 2
    assert s["v_readlane"] == 2 and s["v_writelane"] == 0
    assert s["v_accvgpr_read"] == 2 and s["v_accvgpr_write"] == 1
    assert s["s_nop"] == 1 and s["s_cbranch_execz"] == 1 and s["s_cbranch_execnz"] == 1 and s["s_branch"] == 1
    # the 24 instructions from .LBB0_2 to the branch back to it (4 + 2 + 7 + 4 + 7) and the 4 of the out-of-line block
    assert s["loop_insns"] == 28


def test_loop_stats_without_nesting_or_loops():
    tool = _tool()
    flat = tool.loop_stats(["\ts_and_saveexec_b64 s[6:7], s[4:5]", "\ts_or_b64 exec, exec, s[6:7]", "\ts_endpgm"])
    assert flat["exec_regions"] == 0 and flat["loop_insns"] == 0 and flat["regions_by_mask"] == {}
    one = tool.loop_stats([".LBB0_1:                    ; =>This Inner Loop Header: Depth=1",
                           "\ts_and_saveexec_b64 s[6:7], vcc", "\ts_or_b64 exec, exec, s[6:7]",
                           "\ts_cbranch_scc1 .LBB0_1"])
    assert one["exec_regions"] == 1 and one["regions_by_mask"] == {"vcc": 1} and one["loop_insns"] == 3
