#!/usr/bin/env python3
"""Static instruction table of every compiled QP class (DESIGN §3.3 "Non-arithmetic instructions"): compiles each
csrc/qp_inst*.hip of a source tree to gfx950 assembly (device only, the Makefile's flags) with
-Rpass-analysis=kernel-resource-usage and counts, per qp_ipm_kernel instantiation, the total instructions and the
kinds the issue's table names, next to the compiler's register / spill / scratch report.

usage: tools/qp_insn_static.py [PKG_DIR] [-o OUT.json]      (PKG_DIR defaults to this tree's package directory;
                                                              point it at a checkout of another commit to compare)
       tools/qp_insn_static.py --table PARENT.json THIS.json  prints the side-by-side table (markdown)
       tools/qp_insn_static.py --loop [PKG_DIR] [--kernel SUBSTR] [-o OUT.json]
                                                             the exec regions of each instantiation's IPM loop
                                                             (loop_stats; only the kernels whose name holds SUBSTR)
       tools/qp_insn_static.py --loop-table PARENT.json THIS.json  the side-by-side table of two --loop outputs
Static counts, not a profile: an unrolled loop counts once per copy, a rolled one once."""
import collections
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dynamic-programming-multiagent-trajectory-optimiziation_amd")
FP64 = re.compile(r"^v_(fma|fmac|add|mul|max|min|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|ldexp|trig_preop|fract|floor|ceil|rndne|trunc)_f64")
CANON = re.compile(r"^v_max_f64\s+\S+,\s*(\|?v\[\d+:\d+\]\|?),\s*(\|?v\[\d+:\d+\]\|?)\s*$")
KINDS = ("total", "fp64_arith", "v_accvgpr_read", "v_accvgpr_write", "v_readlane", "v_writelane", "s_nop", "v_cndmask",
         "v_mov_b32", "v_mov_b64", "s_and_saveexec", "s_or_b64", "s_and_b64", "s_cbranch_execz", "s_waitcnt",
         "v_max_canon", "v_cvt_f64_i32", "buffer_load", "buffer_store", "ds")
RES = ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]",
       "LDS Size [bytes/block]")


def count(lines):
    c = collections.Counter()
    for ln in lines:
        ln = ln.split(";")[0].strip()
        if not ln or ln.startswith(".") or ln.endswith(":"):
            continue
        op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", ln.split()[0])
        c["total"] += 1
        if FP64.match(op):
            c["fp64_arith"] += 1
        m = CANON.match(ln)
        if m and m.group(1) == m.group(2):
            c["v_max_canon"] += 1
        for k in ("v_accvgpr_read", "v_accvgpr_write", "v_readlane", "v_writelane", "v_cndmask", "s_and_saveexec",
                  "buffer_load", "buffer_store"):
            if op.startswith(k):
                c[k] += 1
        if op in ("s_nop", "v_mov_b32", "v_mov_b64", "s_or_b64", "s_and_b64", "s_cbranch_execz", "s_waitcnt",
                  "v_cvt_f64_i32"):
            c[op] += 1
        if op.startswith("ds_"):
            c["ds"] += 1
    return {k: c.get(k, 0) for k in KINDS}


LOOP_KINDS = ("v_readlane", "v_writelane", "v_accvgpr_read", "v_accvgpr_write", "s_nop", "s_cbranch_execz",
              "s_cbranch_execnz", "s_branch")
BLOCK = re.compile(r"^\s*(?:\.L(BB\d+_\d+):|;\s*%bb\.\d+:)")
IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")


def loop_stats(lines):
    """The exec regions of a kernel's main loop (DESIGN §3.3 "Lane guards and spill reloads").

    Loops are read from the compiler's block annotations (`=>This Loop Header: Depth=1`, `Parent Loop BB0_2 Depth=1`,
    `in Loop: Header=BB0_2 Depth=1`), so a block laid out of line still counts for its loop.  The main loop is the
    outermost (depth 1) loop with the most instructions among those that contain another loop -- for qp_ipm_kernel
    the IPM loop, around the factor's stage loop; a kernel whose loops do not nest gives its largest loop, one
    without loops gives zeros.  Counted over the loop's blocks in layout order: the exec regions
    (s_and_saveexec_b64), their number per mask operand, how many open directly after an `s_or_b64 exec, exec, ...`
    closed the previous one (the instruction before, labels aside), and the spill / accumulator-copy / branch
    instructions."""
    parent, depth = {}, {}        # loop header -> enclosing loop's header / its depth
    per = collections.defaultdict(list)   # innermost loop header -> instructions of its blocks
    cur, head = None, False       # the loop of the current block; still inside the block's leading comment lines
    for raw in lines:
        code, _, com = raw.partition(";")
        code = code.strip()
        m = BLOCK.match(raw)
        if m:
            cur, head = None, True
            name = m.group(1)
        if head and (m or not code):
            il, pl, hd = IN_LOOP.search(com), PARENT.findall(com), HEADER.search(com)
            if il:
                cur = il.group(1)
            if pl and name:
                d, p = max((int(d), p) for p, d in pl)
                parent[name] = p
            if hd and name:
                cur = name
                depth[name] = int(hd.group(1))
            if m or not code:
                continue
        head = False
        if code and not code.startswith(".") and not code.endswith(":") and cur:
            per[cur].append(code)
    def top(h):
        while h in parent and depth.get(h, 1) > 1:
            h = parent[h]
        return h
    total, nested = collections.defaultdict(list), set()
    for h, ins in per.items():
        total[top(h)] += ins
        if top(h) != h:
            nested.add(top(h))
    out = {"loop_insns": 0, "exec_regions": 0, "regions_by_mask": {}, "reopen_after_close": 0}
    out.update({k: 0 for k in LOOP_KINDS})
    if not total:
        return out
    body = max(((h in nested, len(i)), i) for h, i in total.items())[1]
    out["loop_insns"] = len(body)
    masks = collections.Counter()
    for i, ln in enumerate(body):
        op = re.sub(r"_(e32|e64)$", "", ln.split()[0])
        if op == "s_and_saveexec_b64":
            masks[ln.split(",")[-1].strip()] += 1
            if i > 0 and re.match(r"s_or_b64\s+exec,\s*exec,", body[i - 1]):
                out["reopen_after_close"] += 1
        for k in LOOP_KINDS:
            if op == k or (k.startswith("v_") and op.startswith(k)):
                out[k] += 1
    out["exec_regions"] = sum(masks.values())
    out["regions_by_mask"] = dict(masks.most_common())
    return out


def demangle(names):
    if not names:
        return []
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True)
    return out.stdout.split("\n")[:len(names)]


def one(pkg, src, tmp, loop=False):
    asm = os.path.join(tmp, os.path.basename(src) + ".s")
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", '-DSCVX_OFFLOAD_ARCH="gfx950"',
             "-I" + os.path.join(os.path.dirname(pkg), "include"), "-I" + os.path.join(pkg, "build"), "-w",
             "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]
    if src.endswith("qp_inst_quad.hip"):
        flags += ["-mllvm", "-pragma-unroll-threshold=500000"]   # the Makefile's per-file flag
    flags += os.environ.get("QP_EXTRA_FLAGS", "").split()
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + [src, "-o", asm], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(r.stderr[-4000:])
    res, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+)\b", ln)
        if m and cur and m.group(1) in RES:
            res[cur][m.group(1)] = int(m.group(2))
    body, cur = {}, None
    for ln in open(asm):
        m = re.match(r"^(_Z\w*qp_ipm_kernel\w*):", ln)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif cur and ln.startswith("\t.end_amdhsa_kernel") or ln.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            body[cur].append(ln)
    names = list(body)
    return {d.replace("scvx::", "").replace("void ", "").replace("(QPArgs)", ""):
            loop_stats(body[n]) if loop else dict(count(body[n]), **res.get(n, {}))
            for n, d in zip(names, demangle(names))}


def table(pa, th):
    a, b = json.load(open(pa)), json.load(open(th))
    cols = KINDS + RES
    print("| kernel | side | " + " | ".join(cols) + " |")
    print("|---|---|" + "---|" * len(cols))
    for k in sorted(set(a) | set(b)):
        for side, d in (("parent", a.get(k)), ("this", b.get(k))):
            if d is not None:
                print(f"| `{k}` | {side} | " + " | ".join(str(d.get(c, "")) for c in cols) + " |")
    worse = [k for k in a if k in b and b[k].get(RES[3], 0) > a[k].get(RES[3], 0)]
    print("\nclasses with more scratch than the parent:", worse or "none")


LOOP_COLS = ("loop_insns", "exec_regions", "reopen_after_close") + LOOP_KINDS


def loop_table(pa, th):
    """side-by-side markdown table of two --loop outputs; the last column is the largest number of regions under one
    mask operand (the same mask can sit in several operands over the loop, so it is a lower bound for one mask)"""
    a, b = json.load(open(pa)), json.load(open(th))
    print("| kernel | side | " + " | ".join(LOOP_COLS) + " | most regions under one mask operand |")
    print("|---|---|" + "---|" * (len(LOOP_COLS) + 1))
    for k in sorted(set(a) | set(b)):
        for side, d in (("parent", a.get(k)), ("this", b.get(k))):
            if d is not None:
                print(f"| `{k}` | {side} | " + " | ".join(str(d[c]) for c in LOOP_COLS) +
                      f" | {max(d['regions_by_mask'].values(), default=0)} |")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--table":
        return table(sys.argv[2], sys.argv[3])
    if len(sys.argv) > 1 and sys.argv[1] == "--loop-table":
        return loop_table(sys.argv[2], sys.argv[3])
    args = [x for x in sys.argv[1:]]
    loop = "--loop" in args
    if loop:
        args.remove("--loop")
    only = None
    if "--kernel" in args:
        only = args[args.index("--kernel") + 1]
        del args[args.index("--kernel"):args.index("--kernel") + 2]
    out = None
    if "-o" in args:
        out = args[args.index("-o") + 1]
        del args[args.index("-o"):args.index("-o") + 2]
    pkg = os.path.abspath(args[0]) if args else PKG
    subprocess.run(["make", "-s", "-C", pkg, "rtc-headers"], check=True)
    srcs = sorted(glob.glob(os.path.join(pkg, "csrc", "qp_inst*.hip")))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(int(os.environ.get("JOBS", "8"))) as ex:
        parts = list(ex.map(lambda s: one(pkg, s, tmp, loop), srcs))
    res = {k: v for p in parts for k, v in p.items() if only is None or only in k}
    text = json.dumps(res, indent=1, sort_keys=True)
    if out:
        open(out, "w").write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
