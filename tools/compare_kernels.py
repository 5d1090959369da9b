"""Compare the gfx950 machine code of two builds of libaogym.so kernel by kernel: which kernels are instruction for instruction the same,
which differ, which are new or gone.  Used to show that a change leaves the kernels of existing paths untouched (profiles/detector_noise.md).

    python tools/compare_kernels.py OLD_BUILD_DIR NEW_BUILD_DIR [unit ...]

The directories hold the object files of adaptive_optics_gym_amd/build.py (csrc/build/*.o); units default to every object both have.  Each
object's device code is unbundled (llvm-objcopy, clang-offload-bundler), disassembled (llvm-objdump -d) and split per symbol; addresses,
branch targets and the padding after a kernel's s_endpgm are dropped before the comparison.  Exit status 1 if a kernel both builds have differs."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(obj, tmp):
    base = os.path.join(tmp, os.path.basename(obj) + "." + str(abs(hash(obj))))
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={base}.fat", obj, os.devnull], check=True, stderr=subprocess.DEVNULL)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={base}.fat", f"--targets={TARGET}", f"--output={base}.co"], check=True)
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", f"{base}.co"], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            t = re.sub(r"^\s*[0-9a-f]+:\s*", "", line)
            t = re.sub(r"//.*$", "", re.sub(r"<[^>]+>", "<L>", t)).strip()
            cur.append(t)
    for body in out.values():   # (the assembler pads the end of a code object with s_nop / s_code_end)
        while body and (body[-1].startswith("s_nop") or body[-1].startswith("s_code_end")):
            body.pop()
    return out


def main(old_dir, new_dir, units):
    if not units:
        names = lambda d: {os.path.basename(p)[:-2] for p in glob.glob(os.path.join(d, "*.o"))}
        units = sorted(names(old_dir) & names(new_dir))
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            a, b = kernels(os.path.join(old_dir, u + ".o"), tmp), kernels(os.path.join(new_dir, u + ".o"), tmp)
            for k in sorted(set(a) | set(b)):
                state = "new" if k not in a else "gone" if k not in b else "same" if a[k] == b[k] else "DIFFERENT"
                differ += state == "DIFFERENT"
                print(f"{u:14s} {state:9s} {len(a.get(k, [])):6d} {len(b.get(k, [])):6d}  {k}")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
