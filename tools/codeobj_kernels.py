#!/usr/bin/env python3
"""One line per kernel of a .hip file's gfx950 code object: demangled name, VGPRs, SGPRs, LDS bytes, scratch
bytes and a hash of its disassembly (addresses and symbol names stripped; branches are relative, so the text
does not depend on where the kernel lands in the object).  Two trees hold the same machine code for a kernel
iff its line is the same in both: `diff <(codeobj_kernels.py a/x.hip) <(codeobj_kernels.py b/x.hip)`.
Needs hipcc and the ROCm LLVM tools only, no GPU.  Kernel count, object size and compile time go to stderr.

usage: tools/codeobj_kernels.py ginkgo_amd/csrc/csr_spmv.hip [--mangled]
"""
import hashlib, os, re, shutil, subprocess, sys, tempfile, time

ROCM = os.environ.get("ROCM", "/opt/rocm")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = next(d for d in (ROCM + "/llvm/bin", ROCM + "/lib/llvm/bin") if os.path.isdir(d))
# the device pass of ginkgo_amd/csrc/Makefile (CXXFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + ROOT + "/include",
         "-I" + ROOT + "/ginkgo_amd/csrc", "-Wall", "-Wno-unused-function", "--cuda-device-only"]


def run(*cmd, stdin=None):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, input=stdin).stdout


def main():
    src = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        out, co = tmp + "/dev.o", tmp + "/gfx950.co"
        t0 = time.time()
        run(ROCM + "/bin/hipcc", *FLAGS, "-c", src, "-o", out)
        secs = time.time() - t0
        if open(out, "rb").read(4) == b"\x7fELF":      # (a compiler that writes the bare code object)
            co = out
        else:
            run(LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + out, "--output=" + co,
                "--targets=hip-amdgcn-amd-amdhsa--gfx950")
        notes = run(LLVM + "/llvm-readelf", "--notes", co)
        asm = run(LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co)
        size = os.path.getsize(co)
    # metadata: one block per kernel, its keys one indentation level below "amdhsa.kernels:"
    meta, cur, indent = {}, None, None
    for line in notes.splitlines():
        m = re.match(r"(\s*)(- )?(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(2) and (indent is None or len(m.group(1)) == indent):
            indent, cur = len(m.group(1)), {}
        if cur is not None and len(m.group(1)) + 2 * bool(m.group(2)) == indent + 2:
            cur[m.group(3)] = m.group(4).strip("'\"")
            if m.group(3) == ".symbol":
                meta[cur[".symbol"][:-3]] = cur
    # disassembly: "<address> <symbol>:" opens a function; "// address" and "<symbol+offset>" are cut
    text, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            text[name] = []
        elif name and line.strip():
            text[name].append(re.sub(r"<[^>]*>", "", line.split("//")[0]).strip())
    names = sorted(meta)
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")     # (neither: mangled names)
    shown = names if "--mangled" in sys.argv or not filt else run(filt, stdin="\n".join(names)).splitlines()
    rows = []
    for sym, nm in zip(names, shown):
        k = meta[sym]
        h = hashlib.sha1("\n".join(text[sym]).encode()).hexdigest()[:16]
        rows.append("%s\tvgpr=%s sgpr=%s lds=%s scratch=%s\t%s" % (
            nm, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"],
            k[".private_segment_fixed_size"], h))
    print("\n".join(sorted(rows)))
    print("%d kernels, code object %d bytes, device pass %.0f s" % (len(rows), size, secs), file=sys.stderr)


if __name__ == "__main__":
    main()
