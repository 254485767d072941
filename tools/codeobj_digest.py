"""SHA-256 digests of the gfx950 code object inside a built libmcaq_hip.so.

    python tools/codeobj_digest.py mcaq_yolo_amd/lib/libmcaq_hip.so

Prints three lines: disassembly, kernel metadata (ELF notes), .rodata/.data.
Two builds of one source agree on all three although the raw .so bytes differ,
so equal digests before and after an edit prove the device code unchanged."""
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, capture_output=True, text=True).stdout


def digests(so):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, so, os.path.join(d, "unused.so"))
        run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
        dumps = (("disasm", run("llvm-objdump", "-d", "--no-show-raw-insn", co)),
                 ("notes", run("llvm-readelf", "--notes", co)),
                 ("data", run("llvm-objdump", "-s", "-j", ".rodata", "-j", ".data", co)))
    for name, text in dumps:
        body = "".join(l for l in text.splitlines(True) if "file format" not in l)
        yield name, hashlib.sha256(body.encode()).hexdigest()


if __name__ == "__main__":
    for name, h in digests(sys.argv[1]):
        print(f"{name:7s}{h}")
