"""Per-kernel comparison of two builds of libmcaq_hip.so: is each kernel's
gfx950 disassembly the same text, and what does each build's metadata say
about its registers (tools/kernel_regs.py)?

    python tools/kernel_isa_diff.py OLD.so NEW.so PATTERN [--rename RE=REPL ...] [--json OUT]

Kernels are paired by demangled name; --rename rewrites OLD's names first (a
kernel whose template arguments were renamed).  Addresses are stripped, so a
kernel that only moved inside the code object compares equal.  Verdicts:
`same` (the same text), `moved` (the same text but for the 32-bit literals of
s_add_u32 / s_addc_u32: pc-relative addresses of constant data, which shift
when other code of the object grows or shrinks) and `DIFF`.  Prints one line
per kernel of NEW whose name contains PATTERN, then the kernels of OLD that
have no partner."""
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402

LLVM = kernel_regs.LLVM
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(tool, *args, **kw):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, capture_output=True, text=True, **kw).stdout


def unmoved(text):
    """text with the literal operand of every s_add_u32 / s_addc_u32 masked"""
    return re.sub(r"^(s_addc?_u32 .*, )(?:0x[0-9a-f]+|\d+)$", r"\1LIT", text, flags=re.M)


def functions(so):
    """({mangled name: disassembly text without addresses}, {mangled name: demangled name})"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "gfx950.co")
        run("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat)
        run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
        text = run("llvm-objdump", "-d", "--no-show-raw-insn", co)
        plain = re.findall(r"^[0-9a-f]+ <(.+)>:$", run("llvm-objdump", "-d", "-C", "--no-show-raw-insn", co), re.M)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(re.sub(r"\s*//.*$", "", line).strip())
    assert len(plain) == len(out)       # the same symbols in the same order
    return {k: "\n".join(v) for k, v in out.items()}, dict(zip(out, plain))


def compare(old_so, new_so, pattern, renames=()):
    (fo, do), (fn, dn) = functions(old_so), functions(new_so)
    ro, rn = kernel_regs.kernels(old_so), kernel_regs.kernels(new_so)
    do, dn = ({k: v for k, v in d.items() if k in r} for d, r in ((do, ro), (dn, rn)))   # kernels only
    for rx, repl in renames:
        do = {k: re.sub(rx, repl, v) for k, v in do.items()}
    old_by_name = {v: k for k, v in do.items()}
    recs = []
    for mangled, name in sorted(dn.items(), key=lambda kv: kv[1]):
        if pattern not in mangled:
            continue
        o = old_by_name.pop(name, None)
        same = o is not None and fo[o] == fn[mangled]
        moved = o is not None and not same and unmoved(fo[o]) == unmoved(fn[mangled])
        recs.append({"kernel": name, "identical": same, "verdict": "same" if same else "moved" if moved else "DIFF",
                     "old": ro.get(o), "new": rn[mangled]})
    gone = sorted(v for v, k in old_by_name.items() if pattern in k)
    return recs, gone


if __name__ == "__main__":
    a = sys.argv[1:]
    renames, out = [], None
    while "--rename" in a:
        i = a.index("--rename")
        renames.append(tuple(a[i + 1].split("=", 1)))
        del a[i:i + 2]
    if "--json" in a:
        i = a.index("--json")
        out = a[i + 1]
        del a[i:i + 2]
    recs, gone = compare(a[0], a[1], a[2], renames)
    for r in recs:
        print(r["verdict"], r["kernel"],
              "vgpr %s->%s" % ((r["old"] or {}).get("vgpr_count"), r["new"]["vgpr_count"]))
    for g in gone:
        print("gone", g)
    print("%d kernels, %d identical, %d moved, %d only in the old build" % (
        len(recs), sum(r["identical"] for r in recs), sum(r["verdict"] == "moved" for r in recs), len(gone)))
    if out:
        with open(out, "w") as f:
            json.dump({"kernels": recs, "only_in_old": gone}, f, indent=1)
            f.write("\n")
