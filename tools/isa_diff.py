"""Compare the gfx950 instruction streams of two builds of the engine library, kernel by kernel (no GPU needed):
    python tools/isa_diff.py OLD/libhehub_amd.so NEW/libhehub_amd.so [name filter] [--all]
prints, per demangled kernel name, whether the disassembled instruction text is identical (addresses and encodings stripped), both
instruction counts, and the kernel_meta.py resource numbers where they differ.  Identical kernels are only counted unless --all
is given.  Exit status 1 when any kernel differs or exists on one side only.  A source-only refactor should leave every kernel as
it was; this is how to check that it did."""
import re
import subprocess
import sys
import tempfile

from kernel_meta import LLVM, code_objects, kernel_meta

RES = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def instruction_text(lib):
    """{mangled symbol: [instruction lines]} of every function in the library's code objects"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                elif cur is not None and line[:1] in (" ", "\t"):
                    ins = line.split("//")[0].strip()   # drop "// address: encoding"
                    if ins:
                        cur.append(ins)
    for ins in out.values():   # (what follows the last s_endpgm pads the function to the next one's alignment)
        while ins and ins[-1] != "s_endpgm" and "s_endpgm" in ins:
            ins.pop()
    return out


def kernels(lib):
    """{demangled name: (instruction lines, resources)}"""
    text = instruction_text(lib)
    return {name: (text.get(r["name"], []), r) for name, r in kernel_meta(lib).items()}


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    if len(args) < 2:
        print(__doc__)
        return 2
    flt = args[2] if len(args) > 2 else ""
    old, new = kernels(args[0]), kernels(args[1])
    same = diff = 0
    for name in sorted(set(old) | set(new)):
        if flt not in name:
            continue
        if name not in old or name not in new:
            print(f"{'only in OLD' if name in old else 'only in NEW':12s} {name}")
            diff += 1
            continue
        (io, ro), (jn, rn) = old[name], new[name]
        if io == jn:
            same += 1
            if "--all" in argv:
                print(f"{'identical':12s} {name}  {len(io)}")
            continue
        diff += 1
        res = "  ".join(f"{k}: {ro.get(k)} -> {rn.get(k)}" for k in RES if ro.get(k) != rn.get(k))
        print(f"{'DIFFERS':12s} {name}  {len(io)} -> {len(jn)} instructions  {res}")
    print(f"{same} identical, {diff} differ")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
