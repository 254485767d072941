"""Register / scratch / LDS record of kernels in the built library, from the
gfx950 code object's metadata (no GPU needed).

    python tools/kernel_regs.py [--lib PATH] PATTERN [PATTERN ...]

Prints one line per kernel whose (mangled) name contains a PATTERN:
vgpr_count, agpr_count, sgpr_count, private_segment_fixed_size (scratch bytes
a lane), group_segment_fixed_size (static LDS), vgpr_spill_count."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".vgpr_spill_count")


def kernels(lib):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "gfx950.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat],
                       check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True,
                               capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r"\n\s*- \.", notes):
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or ".vgpr_count" not in blk:
            continue
        rec = {}
        for k in KEYS:
            m = re.search(re.escape(k) + r":\s+(\d+)", "." + blk)
            rec[k[1:]] = int(m.group(1)) if m else None
        out[name.group(1)] = rec
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    lib = os.path.join(ROOT, "mcaq_yolo_amd", "lib", "libmcaq_hip.so")
    if "--lib" in a:
        i = a.index("--lib")
        lib = a[i + 1]
        del a[i:i + 2]
    for n, r in sorted(kernels(lib).items()):
        if any(p in n for p in a):
            print(n, " ".join("%s=%s" % kv for kv in r.items()))
