#!/usr/bin/env python3
"""VALU instructions, selects by encoding, compares, f64 reciprocals and division scalings, spilled-scalar traffic
(v_readlane_b32 / v_writelane_b32, v_readfirstlane_b32), s_nop and cross-lane operations (DPP, ds_bpermute) in line ranges
of a kept assembly file (CPU tool).

    python tools/isa_range_count.py miso_amd/csrc/.isa/kernels_k2m_m0w8.s 5200-5700 [FIRST-LAST ...]
    python tools/isa_range_count.py miso_amd/csrc/.isa/kernels_k2m_m0w8.s --label .LBB0_236 [--label ...]

A range is lines FIRST .. LAST of the file (1-based, inclusive); --label counts the basic block that starts at the label,
up to the next label.  The always-taken path of a loop body is read off the file by hand (follow the fall-throughs and the
branches that are taken when no special case applies) and given as its ranges; the tool only counts.  `select e32` is a
v_cndmask_b32 in the 32-bit encoding, whose mask is VCC by definition; `select e64` names its mask (VCC or another pair:
`of which vcc` says how many name VCC)."""
import argparse
import collections
import re


def count(lines):
    c = collections.Counter()
    for l in lines:
        t = l.strip().split()
        if not t or t[0].endswith(":") or t[0].startswith((".", ";")):
            continue
        op = t[0]
        if op.startswith("v_"):
            c["VALU"] += 1
        if op == "v_cndmask_b32_e32":
            c["select e32"] += 1
        elif op.startswith("v_cndmask_b32"):
            c["select e64"] += 1
            if re.search(r"\bvcc\b", l):
                c["of which vcc"] += 1
        if op.startswith("v_cmp"):
            c["compare"] += 1
        if op.startswith("v_rcp_f64"):
            c["rcp f64"] += 1
        if op.startswith("v_div_scale"):
            c["div_scale"] += 1
        if op == "v_readlane_b32":
            c["readlane"] += 1
        if op == "v_writelane_b32":
            c["writelane"] += 1
        if op == "v_readfirstlane_b32":
            c["readfirstlane"] += 1
        if op == "s_nop":
            c["s_nop"] += 1
        if op.endswith("_dpp") or re.search(r"\b(quad_perm|row_shl|row_shr|row_ror|row_bcast|row_share|row_xmask|row_mirror|row_half_mirror|wave_sh[lr]|wave_ro[lr]):?", l):
            c["dpp"] += 1
        if op.startswith("ds_bpermute") or op.startswith("ds_permute"):
            c["bpermute"] += 1
        if op.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("ranges", nargs="*", help="FIRST-LAST")
    ap.add_argument("--label", action="append", default=[])
    a = ap.parse_args()
    lines = open(a.asm).read().split("\n")
    spans = []
    for r in a.ranges:
        lo, hi = map(int, r.split("-"))
        spans.append((r, lo - 1, hi))
    for lab in a.label:
        starts = [i for i, l in enumerate(lines) if l.startswith(lab + ":")]
        if len(starts) != 1:
            raise SystemExit("%s: %d definitions" % (lab, len(starts)))
        end = next(i for i in range(starts[0] + 1, len(lines)) if re.match(r"^\.L\w+:", lines[i]))
        spans.append((lab, starts[0], end))
    total = collections.Counter()
    keys = ("VALU", "select e32", "select e64", "of which vcc", "compare", "rcp f64", "div_scale", "readlane", "writelane",
            "readfirstlane", "s_nop", "dpp", "bpermute", "branch")
    for name, lo, hi in spans:
        c = count(lines[lo:hi])
        total += c
        print("%-16s" % name, "  ".join("%s %d" % (k, c[k]) for k in keys))
    if len(spans) > 1:
        print("%-16s" % "total", "  ".join("%s %d" % (k, total[k]) for k in keys))


if __name__ == "__main__":
    main()
