"""Machine code of two builds of the library, kernel by kernel: python scripts/kernel_diff.py OLD.so NEW.so

Per kernel symbol of the gfx950 code objects: the disassembly without addresses and encodings, and the kernel's metadata note (VGPR / AGPR /
SGPR counts, scratch, LDS, kernarg size and layout).  Prints the counts -- kernels in OLD and NEW, compared, identical, differing, only in
one of them -- and the names that differ; also every symbol that more than one code object of a library holds.  Exit status 1 if a kernel
differs or is emitted twice."""
import collections, os, re, shutil, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import code_objects, kernel_notes, llvm_tool      # the reader of the metadata notes


def kernels(lib):
    """{symbol: (instruction text, metadata note)} and the symbols held by more than one code object"""
    work = tempfile.mkdtemp()
    code, notes, seen = {}, {}, collections.Counter()
    for co in code_objects(lib, work):
        notes.update(kernel_notes(co))
        dis = subprocess.run([llvm_tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, flags=re.S | re.M):
            if m.group(1) in notes:                                     # kernels only: device functions are inlined or local to their object
                seen[m.group(1)] += 1
                lines = [ln.split("//")[0].strip() for ln in m.group(2).split("\n")]
                # the padding behind a kernel: to the end of the code object, or zero words up to the next symbol's alignment (0x00000000 disassembles
                # as `v_cndmask_b32_e32 v0, s0, v0, vcc`; no kernel ends in one: the last instruction is s_endpgm or a branch)
                while lines and lines[-1] in ("", "...", "s_nop 0", "s_code_end", "v_cndmask_b32_e32 v0, s0, v0, vcc"):
                    lines.pop()
                code[m.group(1)] = "\n".join(lines)
    shutil.rmtree(work)
    return {k: (code[k], notes[k]) for k in code}, sorted(k for k, n in seen.items() if n > 1)


def main():
    (old, old_twice), (new, new_twice) = kernels(sys.argv[1]), kernels(sys.argv[2])
    both = sorted(set(old) & set(new))
    differ = [k for k in both if old[k] != new[k]]
    print(f"kernels: {len(old)} old, {len(new)} new; {len(both)} compared, {len(both) - len(differ)} identical, {len(differ)} differing, "
          f"{len(set(old) - set(new))} only old, {len(set(new) - set(old))} only new")
    for title, names in (("differs", differ), ("only old", sorted(set(old) - set(new))), ("only new", sorted(set(new) - set(old))),
                         ("in more than one code object of old", old_twice), ("in more than one code object of new", new_twice)):
        for k in names:
            what = "" if title != "differs" else " (code)" if old[k][0] != new[k][0] else " (metadata)"
            print(f"  {title}{what}: {k}")
    return 1 if differ or new_twice else 0


if __name__ == "__main__":
    sys.exit(main())
