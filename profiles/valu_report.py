#!/usr/bin/env python3
"""What one kernel issues: static instruction counts of its gfx950 assembly, per loop and per straight-line region.

A sibling of waitcnt_report.py, on the same device-only compile with the product's flags.  One kernel is cut out by its
demangled name and walked in program order.  A region is a loop (the compiler's own "Loop Header" comments; blocks of a
loop that were placed elsewhere are added to it) or the straight-line code between two barriers outside loops.  For
every region: vector instructions (VALU), those of them that are fp64 arithmetic (v_*_f64, compares not counted),
scalar ALU instructions (SALU), branches, LDS instructions and global / scratch memory instructions.  Instructions are
told apart by their mnemonic's class prefix only (v_, s_, ds_, global_ ...): no opcode table.  The first line gives the
kernel's registers, spills and scratch.

    profiles/valu_report.py "scale_frames_kernel<8, 4, 0, false>"                     # the tree
    profiles/valu_report.py --parent HEAD "scale_frames_kernel<8, 4, 0, false>"       # that commit against the tree
    profiles/valu_report.py --parent-asm old.s --asm new.s "scale_frames_kernel<4, 4, 0, true>"

With a parent the regions are matched in program order and printed side by side (parent | tree); when the two listings
do not have the same number of regions they are printed one after the other.  The counts are static: a loop's line is
one trip through all of its blocks, whichever of them a trip executes.
Needs no GPU."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import waitcnt_report as wr  # noqa: E402

COLS = ("VALU", "f64", "SALU", "br", "LDS", "mem")
NOT_SALU = re.compile(r"^s_(waitcnt|barrier|nop|endpgm|sleep|load_|buffer_load_|branch|cbranch|setprio|code_end)")


def classify(op):
    """Column of one instruction by its class prefix, or None."""
    name = op.split(None, 1)[0]
    if name.startswith("v_"):
        return "VALU"
    if name.startswith("ds_"):
        return "LDS"
    if re.match(r"^(global_|buffer_|flat_|scratch_|s_load_|s_buffer_load_)", name):
        return "mem"
    if re.match(r"^s_(branch|cbranch)", name):
        return "br"
    if name.startswith("s_") and not NOT_SALU.match(name):
        return "SALU"
    return None


def is_f64_arith(op):
    name = op.split(None, 1)[0]
    return name.startswith("v_") and "_f64" in name and not name.startswith("v_cmp")


def regions(body):
    """[(title, counts)] in order of first appearance."""
    order, table = [], {}
    region, straight = None, 0

    def slot(key, title):
        if key not in table:
            table[key] = (title, dict.fromkeys(COLS, 0))
            order.append(key)
        return table[key][1]

    for raw in body:
        line = raw.strip()
        m, b = wr.LABEL.match(line), wr.BLOCK.match(line)
        if m or b:
            label = m.group(1) if m else "%%bb.%s" % b.group(1)
            h, mem = wr.HEADER.search(line), wr.MEMBER.search(line)
            if h:
                region = (label[2:] if label.startswith(".L") else label, int(h.group(1)))
            elif mem:
                region = (mem.group(1), int(mem.group(2)))
            else:
                region = None
            continue
        if not line or line.startswith(";") or line.startswith("."):
            continue
        op = line.split(";")[0].strip()
        if not op:
            continue
        if region is None and op.startswith("s_barrier"):
            straight += 1
            continue
        col = classify(op)
        if col is None:
            continue
        c = slot(("loop",) + region, "loop %s (depth %d)" % region) if region else slot(("straight", straight), "straight #%d" % straight)
        c[col] += 1
        if is_f64_arith(op):
            c["f64"] += 1
    return [table[k] for k in order]


def total(rs):
    t = dict.fromkeys(COLS, 0)
    for _, c in rs:
        for k in COLS:
            t[k] += c[k]
    return t


def fmt(c):
    return " ".join("%5d" % c[k] for k in COLS)


def one(text, kernel):
    mangled, name, body = wr.kernel_body(text, kernel)
    return name, wr.resources(text, mangled), regions(body)


def parent_assembly(args):
    """The assembly of commit args.parent, compiled from a copy of its csrc and include directories."""
    root = os.path.join(HERE, "..")
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", root, "archive", args.parent, "mvoscalerecovery_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        csrc = os.path.join(tmp, "mvoscalerecovery_amd", "csrc")
        out = os.path.join(tmp, "kernels.s")
        subprocess.run([wr.HIPCC] + wr.FLAGS + args.flags + [os.path.join(csrc, args.src), "-o", out], check=True, cwd=csrc,
                       stderr=subprocess.DEVNULL if not args.verbose else None)
        with open(out) as f:
            text = f.read()
    if args.save_parent:
        with open(args.save_parent, "w") as f:
            f.write(text)
    return text


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", nargs="+", help="the end of a kernel's demangled name, e.g. 'scale_frames_kernel<8, 4, 0, false>'")
    ap.add_argument("--src", default="mvosr_kernels.hip", help="source file (relative to the csrc directory)")
    ap.add_argument("--asm", help="read the tree's assembly from this file instead of compiling")
    ap.add_argument("--save", help="keep the tree's compiled assembly in this file")
    ap.add_argument("--parent", help="a commit to compare with (compiled from `git archive`)")
    ap.add_argument("--parent-asm", help="the parent's assembly, made earlier with --save or --save-parent")
    ap.add_argument("--save-parent", help="keep the parent's compiled assembly in this file")
    ap.add_argument("--verbose", action="store_true", help="show the compiler's diagnostics")
    ap.add_argument("--flags", nargs="*", default=[], help="extra hipcc flags")
    args = ap.parse_args()
    tree = wr.assembly(args)
    parent = None
    if args.parent_asm:
        with open(args.parent_asm) as f:
            parent = f.read()
    elif args.parent:
        parent = parent_assembly(args)
    head = " ".join("%5s" % k for k in COLS)
    for kernel in args.kernel:
        name, res, rs = one(tree, kernel)
        print(name)
        if parent is None:
            print("  %s" % res)
            print("  %-28s %s" % ("region", head))
            for title, c in rs + [("total", total(rs))]:
                print("  %-28s %s" % (title, fmt(c)))
            continue
        _, pres, prs = one(parent, kernel)
        print("  parent: %s\n  tree:   %s" % (pres, res))
        if len(prs) == len(rs):
            print("  %-28s %s  | %s" % ("region (parent | tree)", head, head))
            for (pt, pc), (_, c) in zip(prs + [("total", total(prs))], rs + [("total", total(rs))]):
                print("  %-28s %s  | %s" % (pt if pt.startswith(("straight", "total")) else "loop", fmt(pc), fmt(c)))
        else:
            for who, rr in (("parent", prs), ("tree", rs)):
                print("  %-28s %s" % ("region (%s)" % who, head))
                for title, c in rr + [("total", total(rr))]:
                    print("  %-28s %s" % (title, fmt(c)))


if __name__ == "__main__":
    main()
