#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libtetranerf_hip.so, kernel by kernel.

    python profiles/compare_device_code.py OLD.so NEW.so

Extracts the offload code objects of both libraries (llvm-objdump --offloading), disassembles them, splits the text at the
`<symbol>:` lines and compares the instruction text per symbol; compares .vgpr_count, .sgpr_count,
.private_segment_fixed_size, .group_segment_fixed_size and .kernarg_segment_size of every kernel (llvm-readelf --notes); and
compares the exported tn_* names (nm -D).  Exit status 0: every symbol of OLD exists in NEW with identical text and resources.
A symbol whose text differs only in the literal that follows an s_getpc_b64 -- the distance from the instruction to a constant of
the code object, which moves when a section between the two grows, not an instruction -- is reported as such, and still counted.
No GPU needed.
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def device_code(so):
    """{symbol: set of instruction texts}, {kernel: set of resource tuples} over every gfx950 code object of the library
    (a template instantiated in several translation units has one copy per code object: hence sets)"""
    text, blocks = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(so, os.path.join(tmp, "lib.so"))             # the code objects are written beside the library
        run(f"{LLVM}/llvm-objdump", "--offloading", "lib.so", cwd=tmp)
        for co in sorted(glob.glob(os.path.join(tmp, "*gfx950*"))):
            sym, per_co = None, {}
            for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
                m = re.match(r"^<(.+)>:$", line.strip())
                if m:
                    sym = m.group(1)
                    per_co[sym] = []
                elif sym and line.strip() and line.strip() != "...":      # ("...": zero padding behind a function)
                    per_co[sym].append(re.sub(r"\s*//.*$", "", line).strip())     # (address comments of branch targets)
            for k, v in per_co.items():
                text.setdefault(k, set()).add("\n".join(v))
            # the notes list every kernel as one YAML map under amdhsa.kernels: "  - .first_key:" opens it, its own keys
            # are indented by four columns (those of its arguments by more)
            block = None
            for line in run(f"{LLVM}/llvm-readelf", "--notes", co).splitlines():
                m = re.match(r"^  (- | {2})(\.\w+):\s*(\S+)\s*$", line)
                if not m:
                    continue
                if m.group(1) == "- ":
                    block = {}
                    blocks.append(block)
                if block is not None:
                    block[m.group(2)] = m.group(3)
    meta = {}
    for b in blocks:
        if ".symbol" in b:
            meta.setdefault(b[".symbol"], set()).add(tuple(b.get(f) for f in FIELDS))
    return text, meta


def pc_relative_only(old, new):
    """the texts (sets, one per code object) differ only in the literal added to a program counter read one line above"""
    if len(old) != len(new):
        return False
    for a, b in zip(sorted(old), sorted(new)):
        a, b = a.splitlines(), b.splitlines()
        if len(a) != len(b):
            return False
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y and not (i and a[i - 1].startswith("s_getpc_b64") and a[i - 1] == b[i - 1] and
                               re.sub(r"0x[0-9a-f]+$", "", x) == re.sub(r"0x[0-9a-f]+$", "", y) and x.startswith("s_add_u32")):
                return False
    return True


def exported(so):
    return sorted(l.split()[-1] for l in run("nm", "-D", "--defined-only", so).splitlines() if " T tn_" in l)


def main():
    old, new = sys.argv[1:3]
    bad = 0
    eo, en = exported(old), exported(new)
    print(f"exported tn_* names: {len(eo)} / {len(en)}: {'same' if eo == en else 'DIFFERENT'}")
    bad += eo != en
    (to, mo), (tn_, mn) = device_code(old), device_code(new)
    print(f"device symbols: {len(to)} / {len(tn_)}; kernels with notes: {len(mo)} / {len(mn)}")
    for sym in sorted(to):
        if sym not in tn_:
            print("MISSING in new:", sym); bad += 1
        elif to[sym] != tn_[sym]:
            only = pc_relative_only(to[sym], tn_[sym])
            print("TEXT DIFFERS (only the literal of a pc-relative address):" if only else "TEXT DIFFERS:", sym); bad += 1
    for sym in sorted(set(tn_) - set(to)):
        print("only in new:", sym)
    for k in sorted(mo):
        if mo[k] != mn.get(k):
            print("RESOURCES DIFFER:", k, mo[k], mn.get(k)); bad += 1
    print("identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
