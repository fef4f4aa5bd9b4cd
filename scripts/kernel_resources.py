"""VGPR / SGPR / scratch / LDS of every kernel in liboai_hip.so (code-object metadata): python scripts/kernel_resources.py [filter]"""
import glob, os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def llvm_tool(name):
    """llvm-objdump / llvm-readelf: on the PATH, or ROCm's own (located like build.py does)"""
    return shutil.which(name) or os.path.join("/opt/rocm/lib/llvm/bin", name)


def code_objects(lib, work):
    """the gfx950 code objects of `lib`, unbundled into the directory `work`"""
    shutil.copy(lib, os.path.join(work, "lib.so"))
    subprocess.run([llvm_tool("llvm-objdump"), "--offloading", "lib.so"], cwd=work, check=True, capture_output=True)
    return sorted(glob.glob(os.path.join(work, "lib.so*gfx950*")))


def kernel_notes(co):
    """(symbol, metadata block) of every kernel of one code object: the block is the kernel's entry of the amdhsa.kernels note, from .agpr_count on"""
    txt = subprocess.run([llvm_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    for blk in txt.split("- .agpr_count:")[1:]:
        blk = blk.split("amdhsa.")[0].strip()
        yield re.search(r"\.name:\s+(\S+)", blk).group(1), blk


def main():
    flt = sys.argv[1] if len(sys.argv) > 1 else ""
    lib = os.environ.get("OAI_LIB_PATH") or os.path.join(ROOT, "oai_analysis_2_amd", "liboai_hip.so")
    work = tempfile.mkdtemp()
    for co in code_objects(lib, work):
        for sym, blk in kernel_notes(co):
            get = lambda k: (re.search(rf"\.{k}:\s+(\S+)", blk) or [None, "?"])[1]
            name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            if flt in name:
                print(f"vgpr {get('vgpr_count'):>4} agpr {blk.split()[0]:>3} sgpr {get('sgpr_count'):>4} scratch {get('private_segment_fixed_size'):>5} "
                      f"lds {get('group_segment_fixed_size'):>6}  {name[:150]}")
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
