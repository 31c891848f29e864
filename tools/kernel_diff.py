#!/usr/bin/env python3
"""Compare the gfx950 device text of every kernel of this tree with another tree's (the parent commit's), kernel by kernel.

    python tools/kernel_diff.py PARENT_CSRC_DIR [unit.hip ...]          (default: every unit in the Makefile's SRCS)

Each unit is compiled in both csrc directories with the Makefile's flags plus --cuda-device-only -S (no GPU needed), the
result split by function symbol, block labels renumbered per function, comments and the .ident / .file / __hip_cuid_* lines
dropped.  One row per kernel:

    identical         the same text
    differs: order    the same multiset of lines once register numbers are blanked: instruction order and register names only
    differs           anything else
    only parent/new   the symbol exists in one tree only

with code length, scratch bytes, SGPRs, VGPRs and static LDS bytes of both sides.  Text comparison only; exits 0 always: the
caller reads the table (profiles/README.md).
"""
import collections
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_CSRC = os.path.join(HERE, "..", "vae_training_amd", "csrc")


def makefile_vars(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    var = {}
    for name, _, value in re.findall(r"^(\w+)\s*(\?=|=)\s*(.*)$", text, re.M):
        var[name] = value.strip()
    def expand(s):
        return re.sub(r"\$\((\w+)\)", lambda m: expand(os.environ.get(m.group(1), var.get(m.group(1), ""))), s)
    return os.environ.get("HIPCC", var["HIPCC"]), expand(var["CXXFLAGS"]).split(), var["SRCS"].split()


def compile_unit(csrc, hipcc, flags, unit, out):
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", unit, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write("%s: %s failed\n%s\n" % (csrc, " ".join(cmd), r.stdout))
        return None
    return open(out).read()


def split_functions(asm):
    """{symbol: (list of body lines, info dict)}; the body runs from the symbol's label to its .Lfunc_end, the kernel
    descriptor (.amdhsa_*) included."""
    info = collections.defaultdict(dict)
    # the code-object metadata at the end of the file: one YAML record per kernel
    for rec in re.split(r"\n\s*- \.agpr_count:", asm)[1:]:
        name = re.search(r"\.name:\s+(\S+)", rec)
        if not name:
            continue
        for key, field in (("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"),
                           ("sgpr", "sgpr_count"), ("vgpr", "vgpr_count")):
            m = re.search(r"\.%s:\s+(\d+)" % field, rec)
            if m:
                info[name.group(1)][key] = int(m.group(1))
    funcs = {}
    lines = asm.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+([\w.$]+),@function", lines[i])
        if not m:
            i += 1
            continue
        sym, body = m.group(1), []
        while i < len(lines) and not lines[i].startswith(sym + ":"):
            i += 1
        while i < len(lines) and not re.match(r"\.Lfunc_end\d+:", lines[i]):
            body.append(lines[i])
            i += 1
        while i < len(lines) and not re.match(r"\s*\.type\s", lines[i]):      # the "; Kernel info:" comments behind the function
            m = re.match(r"; codeLenInByte = (\d+)", lines[i])
            if m:
                info[sym]["len"] = int(m.group(1))
            i += 1
        funcs[sym] = (normalise(body), info[sym])
    return funcs


def normalise(body):
    labels = {}
    def relabel(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))
    out = []
    for line in body:
        line = line.split(";")[0].rstrip()
        if not line.strip() or re.match(r"\s*\.(ident|file)\b", line) or "__hip_cuid_" in line:
            continue
        out.append(re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", relabel, line))
    return out


def blank_registers(line):
    line = re.sub(r"\b([vsa])\[(\d+):(\d+)\]", lambda m: "%s[%d]" % (m.group(1), int(m.group(3)) - int(m.group(2)) + 1), line)
    line = re.sub(r"\b([vsa])\d+\b", r"\1#", line)
    return re.sub(r"\.L\d+", ".L", line)


def verdict(a, b):
    if a == b:
        return "identical"
    if collections.Counter(map(blank_registers, a)) == collections.Counter(map(blank_registers, b)):
        return "differs: order"
    return "differs"


def demangle(symbols):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([filt], input="\n".join(symbols), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
        return dict(zip(symbols, out))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in symbols}


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\((anonymous namespace|vaek)\)?::", "", name.replace("vaek::", ""))
    return re.sub(r"\(.*\)$", "", name)      # the argument list says nothing the template arguments do not


def main():
    if len(sys.argv) < 2:
        print(__doc__)
        return 0
    parent = os.path.abspath(sys.argv[1])
    new = os.path.abspath(NEW_CSRC)
    hipcc, flags, srcs = makefile_vars(new)
    p_hipcc, p_flags, _ = makefile_vars(parent)
    units = sys.argv[2:] or srcs
    tmp = tempfile.mkdtemp(prefix="kernel_diff_")
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for u in units:
            stem = os.path.splitext(os.path.basename(u))[0]
            jobs[u] = (pool.submit(compile_unit, parent, p_hipcc, p_flags, u, os.path.join(tmp, stem + ".parent.s")),
                       pool.submit(compile_unit, new, hipcc, flags, u, os.path.join(tmp, stem + ".new.s")))
    fmt = "%-92s %-16s %-15s %30s   %30s"
    print(fmt % ("kernel", "unit", "verdict", "parent len/scratch/sgpr/vgpr/lds", "new len/scratch/sgpr/vgpr/lds"))
    tally = collections.Counter()
    for u in units:
        a, b = (f.result() for f in jobs[u])
        if a is None or b is None:
            print("%-92s %-16s %s" % ("-", u, "did not compile"))
            continue
        fa, fb = split_functions(a), split_functions(b)
        names = demangle(sorted(set(fa) | set(fb)))
        def figures(f, s):
            i = f[s][1]
            return "%s / %s / %s / %s / %s" % tuple(i.get(k, "-") for k in ("len", "scratch", "sgpr", "vgpr", "lds"))
        for s in sorted(names, key=lambda s: names[s]):
            if s in fa and s in fb:
                v = verdict(fa[s][0], fb[s][0])
            else:
                v = "only parent" if s in fa else "only new"
            tally[v] += 1
            print(fmt % (short(names[s])[:92], u, v, figures(fa, s) if s in fa else "", figures(fb, s) if s in fb else ""))
    print("\n" + ", ".join("%d %s" % (n, v) for v, n in sorted(tally.items())))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
