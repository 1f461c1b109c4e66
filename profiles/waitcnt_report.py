#!/usr/bin/env python3
"""Where one kernel waits: every s_waitcnt of its gfx950 assembly, with the memory and LDS instructions between them.

Compiles a .hip file device-only with the product's flags (or reads an assembly file made that way), cuts one kernel
out by its demangled name and walks it in program order.  The listing is split at loop boundaries (the compiler's own
"Loop Header" comments), so that a wait inside a loop can be told from one in front of it:

    profiles/waitcnt_report.py "scale_frames_kernel<8, 4, 0, false>"
    profiles/waitcnt_report.py --asm saved.s --labels "scale_frames_tiled_kernel<8>"
    profiles/waitcnt_report.py --summary "scale_frames_kernel<4, 4, 0, true>" -- -DMVOSR_STAMPS

Runs of the same instruction are folded ("3x ds_read_b64").  A wait is printed with the counters it names; vmcnt(0) and
lgkmcnt(0) are the full waits.  --summary prints one line per region: the number of waits of each kind.
Needs no GPU."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mvoscalerecovery_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
CXXFILT = "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]

MEM = re.compile(r"^(global_|buffer_|flat_|scratch_|ds_|s_load_|s_buffer_load_|s_barrier|s_waitcnt)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BLOCK = re.compile(r"^; %bb\.(\d+):")
HEADER = re.compile(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)")
MEMBER = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")


def assembly(args):
    if args.asm:
        with open(args.asm) as f:
            return f.read()
    src = args.src if os.path.isabs(args.src) else os.path.join(CSRC, args.src)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernels.s")
        subprocess.run([HIPCC] + FLAGS + args.flags + [src, "-o", out], check=True, cwd=CSRC,
                       stderr=subprocess.DEVNULL if not args.verbose else None)
        with open(out) as f:
            text = f.read()
    if args.save:
        with open(args.save, "w") as f:
            f.write(text)
    return text


def demangle(names):
    tool = next((t for t in (CXXFILT, shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if tool is None:
        sys.exit("no demangler found (llvm-cxxfilt or c++filt)")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return [re.sub(r"^void ", "", re.sub(r"\(.*", "", line)) for line in out.splitlines()]


def kernel_body(text, want):
    """(mangled name, demangled name, lines) of the one kernel whose demangled name ends with `want`."""
    lines = text.splitlines()
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):\s+; @", l)] if m]
    names = demangle([n for _, n in starts])
    norm = lambda s: s.replace(" ", "")
    hits = [(i, n, d) for (i, n), d in zip(starts, names) if norm(d).endswith(norm(want))]
    if len(hits) != 1:
        sys.exit("%d kernels match %r%s" % (len(hits), want, "".join("\n  " + d for _, _, d in hits) if hits else
                                            "; the file has:" + "".join("\n  " + d for d in sorted(set(names)))))
    i, n, d = hits[0]
    end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
    return n, d, lines[i + 1:end]


def resources(text, mangled):
    m = re.search(r"\.amdhsa_kernel " + re.escape(mangled) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S)
    blk = next((b for b in text.split("- .agpr_count")[1:] if re.search(r"\.name:\s+" + re.escape(mangled) + r"\n", b)), "")
    g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
    lds = (re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(1)) or [None, "?"])[1] if m else "?"
    return "vgpr %s sgpr %s spill %s/%s lds(static) %s scratch %s" % (g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"),
                                                                     g("sgpr_spill_count"), lds, g("private_segment_fixed_size"))


def events(body):
    """(region, kind, text) in program order.  region = the innermost loop's header label, or None outside loops."""
    region, label = None, "entry"
    for raw in body:
        line = raw.strip()
        m = LABEL.match(line)
        b = BLOCK.match(line)
        if m or b:
            label = m.group(1) if m else "%%bb.%s" % b.group(1)
            h, mem = HEADER.search(line), MEMBER.search(line)
            if h:
                region = (label[2:] if label.startswith(".L") else label, int(h.group(1)))
            elif mem:
                region = (mem.group(1), int(mem.group(2)))
            else:
                region = None
            yield region, "label", label
            continue
        if not line or line.startswith(";") or line.startswith("."):
            continue
        op = line.split(";")[0].strip()
        if MEM.match(op):
            yield region, "wait" if op.startswith("s_waitcnt") else "mem", op


def brief(op):
    """Mnemonic plus what tells loads apart at a glance: the destination registers and a non-temporal hint."""
    parts = op.split(None, 1)
    name = parts[0]
    if name in ("s_waitcnt", "s_barrier"):
        return op
    tail = parts[1] if len(parts) > 1 else ""
    return name + (" nt" if re.search(r"\bnt\b", tail) else "")


def report(body, labels, summary):
    cur = object()
    run, count = None, 0
    tally = {}

    def flush():
        nonlocal run, count
        if run is not None and not summary:
            print("      %s%s" % ("%dx " % count if count > 1 else "", run))
        run, count = None, 0

    def title(r):
        return "outside loops" if r is None else "loop %s (depth %d)" % r

    for region, kind, text in events(body):
        if region != cur:
            flush()
            cur = region
            if not summary:
                print("  -- %s" % title(region))
        if kind == "label":
            if labels:
                flush()
                if not summary:
                    print("    %s:" % text)
            continue
        if kind == "wait":
            flush()
            t = tally.setdefault(title(region), {"vmcnt(0)": 0, "vmcnt(n)": 0, "lgkmcnt(0)": 0, "lgkmcnt(n)": 0})
            for c, v in re.findall(r"(vmcnt|lgkmcnt)\((\d+)\)", text):
                t["%s(%s)" % (c, "0" if v == "0" else "n")] += 1
            if not summary:
                print("    %s" % text)
            continue
        b = brief(text)
        if b == run:
            count += 1
        else:
            flush()
            run, count = b, 1
    flush()
    print("  waits per region (static count):")
    for name, t in tally.items():
        print("    %-34s %s" % (name, "  ".join("%s %d" % kv for kv in t.items())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", help="the end of the kernel's demangled name, e.g. 'scale_frames_kernel<8, 4, 0, false>'")
    ap.add_argument("--src", default="mvosr_kernels.hip", help="source file (relative to the csrc directory)")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--save", help="keep the compiled assembly in this file")
    ap.add_argument("--labels", action="store_true", help="print the basic-block labels too")
    ap.add_argument("--summary", action="store_true", help="only the resource line and the per-region wait counts")
    ap.add_argument("--verbose", action="store_true", help="show the compiler's diagnostics")
    ap.add_argument("flags", nargs="*", help="extra hipcc flags (after --)")
    args = ap.parse_args()
    text = assembly(args)
    mangled, name, body = kernel_body(text, args.kernel)
    print("%s\n  %s" % (name, resources(text, mangled)))
    report(body, args.labels, args.summary)


if __name__ == "__main__":
    main()
