"""CPU: the C-ABI library builds, loads and exports every symbol include/oai_hip.h declares."""
import ctypes
import os
import re

from oai_analysis_2_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "oai_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(oai_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_everything():
    path = build.build_library(verbose=False)
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/oai_hip.h but not exported"
    # the ctypes table binds exactly the declared set
    assert sorted(_lib.SIGNATURES) == names
    assert _lib.load().oai_version() >= 100


def test_bad_arguments_are_reported_not_crashed():
    lib = _lib.load()
    rc = lib.oai_grid_sample3d(None, 1, 4, 4, 4, None, 4, 4, 4, None, None)
    assert rc != 0 and b"null" in lib.oai_last_error()
    rc = lib.oai_avgpool2_3d(None, 0, 0, 0, 0, None, None)
    assert rc != 0


def test_the_one_call_path_reports_status_stream_and_symbol_faults():
    """_lib.call, the one way the package reaches the C ABI: a non-zero status raises OaiError under the symbol's name; STREAM without a
    device and an undeclared symbol are refused before the library is touched.  No GPU is touched."""
    import pytest
    with pytest.raises(_lib.OaiError) as exc:
        _lib.call("oai_unet_set_precision", None, 3)
    assert str(exc.value).startswith("oai_unet_set_precision failed")

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the library was reached for {name}")
    real, _lib._lib = _lib._lib, Untouchable()
    try:
        with pytest.raises(ValueError):
            _lib.call("oai_grid_sample3d", None, 1, 4, 4, 4, None, 4, 4, 4, None, _lib.STREAM)
        with pytest.raises(_lib.OaiError, match="oai_no_such_symbol"):
            _lib.call("oai_no_such_symbol")
    finally:
        _lib._lib = real


def test_argument_checks_of_the_later_entry_points():
    """Bad arguments come back as a non-zero status with a message -- no GPU is touched before the checks."""
    import ctypes as C
    lib = _lib.load()
    nv, nt = C.c_longlong(), C.c_longlong()
    assert lib.oai_mc_count(None, 8, 8, 8, 0.5, None, 0, C.byref(nv), C.byref(nt), None) != 0 and b"null" in lib.oai_last_error()
    dummy = (C.c_float * 8)()
    assert lib.oai_mc_count(dummy, 1, 8, 8, 0.5, dummy, 32, C.byref(nv), C.byref(nt), None) != 0 and b"at least 2" in lib.oai_last_error()
    assert lib.oai_mc_count(dummy, 8, 8, 8, 0.5, dummy, 32, C.byref(nv), C.byref(nt), None) != 0 and b"workspace" in lib.oai_last_error()
    assert lib.oai_mc_workspace_bytes(1, 8, 8) == 0 and lib.oai_mc_workspace_bytes(160, 384, 384) > 160 * 384 * 384 * 17
    assert lib.oai_mesh_smooth(None, 10, None, None, 5, 0.1, None, None, None) != 0
    assert lib.oai_mesh_point_distance(dummy, 1, dummy, dummy, 0, dummy, None) != 0 and b"triangle" in lib.oai_last_error()
    gd = (C.c_int * 3)(4, 4, 4)
    assert lib.oai_mesh_grid_workspace_bytes(gd, 100) > 0 and lib.oai_mesh_grid_workspace_bytes(gd, 0) == 0
    glo = (C.c_float * 3)(0, 0, 0)
    assert lib.oai_mesh_point_distance_grid(dummy, 1, dummy, dummy, 4, glo, -1.0, gd, dummy, 1 << 20, dummy, None) != 0
    assert lib.oai_mesh_point_distance_grid(dummy, 1, dummy, dummy, 4, glo, 1.0, gd, dummy, 16, dummy, None) != 0 and b"workspace" in lib.oai_last_error()
    t = (C.c_int * 3)(32, 128, 128)
    o = (C.c_int * 3)(16, 64, 64)                                     # overlap eats the whole tile
    assert lib.oai_stitch_blocks(dummy, 2, 16, 16, 16, t, o, None, dummy, None) != 0 and b"overlap" in lib.oai_last_error()
    assert lib.oai_unet_set_precision(None, 3) != 0
    assert lib.oai_image_normalize(None, 10, 0.1, 99.9, 0.0, 1.0, None, None, None, 0, None) != 0


def test_no_valu_written_sgpr_reaches_a_vmem_instruction_too_early():
    """`VALU writes an SGPR -> VMEM reads it` needs five wait states; hipcc pads its own code but cannot see inside inline assembly (the
    SGPR-base weight-fragment loads of unet_sres2.h / unet_wino.h).  build.py refuses such a library; this is the same scan as a test."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sgpr_hazard_scan", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "sgpr_hazard_scan.py"))
    import shutil
    assert os.path.exists(shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"), "no llvm-objdump: the guard cannot run (a skipped guard is a failed guard)"
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.scan_library(build.build_library(verbose=False)) == []
    # the scanner itself: a v_readfirstlane two instructions in front of a global load of that SGPR pair is a hit, five s_nop states later it is not
    bad = "0000 <k>:\n\tv_readfirstlane_b32 s11, v6\n\tv_lshlrev_b32_e32 v192, 4, v190\n\tglobal_load_dwordx4 v[130:133], v192, s[10:11]\n"
    assert len(mod.scan(bad)) == 1
    assert mod.scan(bad.replace("\tv_lshlrev_b32_e32 v192, 4, v190\n", "\ts_nop 4\n")) == []
    # ... and across a back-edge: an SGPR reload at the loop tail, the asm load at the loop head
    loop = ("0000000000001000 <k>:\n"
            "\tglobal_load_dwordx4 v[130:133], v192, s[10:11]   // 000000001000: DC000000\n"
            "\tv_add_u32_e32 v1, v2, v3                          // 000000001008: 68000000\n"
            "\tv_add_u32_e32 v1, v2, v3                          // 00000000100C: 68000000\n"
            "\tv_add_u32_e32 v1, v2, v3                          // 000000001010: 68000000\n"
            "\tv_add_u32_e32 v1, v2, v3                          // 000000001014: 68000000\n"
            "\tv_add_u32_e32 v1, v2, v3                          // 000000001018: 68000000\n"
            "\tv_readlane_b32 s11, v6, 3                         // 00000000101C: D2890000\n"
            "\ts_cbranch_scc1 65528                              // 000000001024: BF85FFF8 <k+0x0>\n")
    assert len(mod.scan(loop)) == 1
    assert mod.scan(loop.replace("\tv_readlane_b32 s11, v6, 3 ", "\tv_readlane_b32 s12, v6, 3 ")) == []


def test_no_packed_fp32_valu_and_hot_kernels_are_mfma(tmp_path):
    """Code-object checks of the shipped library (no GPU needed): (a) no packed fp32 VALU instruction anywhere -- round 2 measured
    v_pk_fma_f32 / v_pk_mul_f32 returning wrong values in 16-lane groups when a kernel runs beside the MFMA kernels
    (profiles/r02_packed_fp32_hazard.md; build.py turns the feature off); (b) the hot kernels are what DESIGN.md says: 3-pass fp16
    MFMAs fed by LDS-DMA in the conv, fp32 MFMAs in the exact path."""
    import glob
    import shutil
    import subprocess
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
    assert os.path.exists(objdump), "no llvm-objdump: the code-object checks cannot run (a skipped guard is a failed guard)"
    path = build.build_library(verbose=False)
    work = str(tmp_path)
    shutil.copy(path, os.path.join(work, "lib.so"))
    subprocess.run([objdump, "--offloading", "lib.so"], cwd=work, check=True, capture_output=True)      # extracts the bundles next to the copy
    objs = sorted(glob.glob(os.path.join(work, "lib.so.*gfx950*")))      # (one order everywhere: the searches below end a kernel at the next symbol)
    assert objs, "no gfx950 code object in the library"
    text = "".join(subprocess.run([objdump, "-d", o], check=True, capture_output=True, text=True).stdout for o in objs)
    packed = re.findall(r"\bv_pk_(?:fma|mul|add)_f32\b", text)
    assert not packed, f"{len(packed)} packed fp32 VALU instructions in the library"
    assert text.count("v_mfma_f32_32x32x16_f16") > 5000 and text.count("v_mfma_f32_32x32x2_f32") > 1000
    assert text.count("global_load_lds_dwordx4") > 100
    # (c) the copy-out of the default conv kernel (and of its ec0-fused instantiation) is a run of stores with nothing in between that waits
    # for memory: `vmcnt` counts stores on this ISA, so a reload from scratch or a late load between them makes every store wait for all
    # earlier ones to reach memory (profiles/r02_conv_per_layer.md section 5).  Chunk loop: no scratch traffic at all.
    for sym in ("_ZN3oai16conv3_igemm_sresILi4ELi16ELi2ELi4ELi1ELb0ELb0EEEvNS_8ConvArgsEPKh",
                "_ZN3oai16conv3_igemm_sresILi4ELi16ELi2ELi4ELi1ELb1ELb0EEEvNS_8ConvArgsEPKh"):
        m = re.search(r"^[0-9a-f]+ <" + sym + r">:\n(.*?)(?=^[0-9a-f]+ <)", text, flags=re.S | re.M)
        assert m, f"{sym} not in the library"
        body = m.group(1).split("\n")
        mf = [i for i, ln in enumerate(body) if "v_mfma_f32_32x32x16_f16" in ln]
        nt = [i for i, ln in enumerate(body) if "global_store_dwordx4" in ln and " nt" in ln]
        assert len(mf) >= 600 and len(nt) >= 32
        between = body[nt[0]:nt[-1] + 1]
        # (the ec0-fused instantiation also holds the scatter copy-out of the shared encoder pass: each candidate tile's box -- 6 ints -- is read by
        # SCALAR loads from the constant address space, i.e. waited for with lgkmcnt: no vector load, no vmcnt wait there either)
        assert not [ln for ln in between if "scratch_" in ln or "vmcnt(0)" in ln or ("global_load_dword" in ln and "lds" not in ln)], \
            "something waits for memory between the copy-out stores"
        for i0, i1 in zip(mf, mf[1:]):                                   # inside a tap stream (MFMAs a few lines apart; the four ML variants lie far apart)
            if i1 - i0 <= 60:
                assert not [ln for ln in body[i0:i1] if "scratch_" in ln], "scratch traffic inside the tap stream"
    # (d) conv3_igemm_sres2 counts vmcnt by hand (unet_sres2.h): between the first and the last MFMA of a tap stream there must be no vector-memory
    # operation the compiler added on its own (a scratch reload is a load: it shifts every counted wait) and no wait other than the counted ones
    sym = "_ZN3oai17conv3_igemm_sres2ILi16ELi2ELi4ELi1ELi0EEEvNS_8ConvArgsEPKh"
    m = re.search(r"^[0-9a-f]+ <" + sym + r">:\n(.*?)(?=^[0-9a-f]+ <)", text, flags=re.S | re.M)
    assert m, f"{sym} not in the library"
    body = m.group(1).split("\n")
    mf = [i for i, ln in enumerate(body) if "v_mfma_f32_32x32x16_f16" in ln]
    assert len(mf) >= 1600                                               # 27 taps x 24 MFMAs for ML = 4, 18 / 12 / 6 for the trimmed variants
    streams, start = [], mf[0]
    for i0, i1 in zip(mf, mf[1:] + [10 ** 9]):
        if i1 - i0 > 120:                                               # a gap: chunk-loop boundary or the next ML variant
            streams.append((start, i0)); start = i1
    assert len(streams) >= 4
    for s0, s1 in streams:
        seg = body[s0:s1]
        assert not [ln for ln in seg if "scratch_" in ln], "scratch traffic inside conv3_igemm_sres2's tap stream"
        loads = [ln for ln in seg if "global_load_dwordx4" in ln or "global_load_lds_dwordx4" in ln]
        assert all("s[" in ln.split("//")[0] or "lds" in ln for ln in loads), "a weight-fragment load that is not the SGPR-base asm form"
    # (e) conv3_wino_sres (unet_wino.h) counts vmcnt by hand as well: 9 taps x 24 MFMAs per chunk for ML = 4; no scratch anywhere in the kernel
    for sym, n_mf in (("_ZN3oai15conv3_wino_sresILi2ELi8ELi4ELi1ELb0ELb0EEEvNS_8ConvArgsEPKh", 540), ("_ZN3oai15conv3_wino_sresILi1ELi8ELi4ELi2ELb0ELb0EEEvNS_8ConvArgsEPKh", 162),
                      ("_ZN3oai15conv3_wino_sresILi1ELi8ELi4ELi1ELb1ELb0EEEvNS_8ConvArgsEPKh", 540)):       # (the specialised form: four multiplying waves, ML = 4 .. 1)
        m = re.search(r"^[0-9a-f]+ <" + sym + r">:\n(.*?)(?=^[0-9a-f]+ <)", text, flags=re.S | re.M)
        assert m, f"{sym} not in the library"
        body = m.group(1).split("\n")
        assert len([ln for ln in body if "v_mfma_f32_32x32x16_f16" in ln]) == n_mf
        mf_i = [i for i, ln in enumerate(body) if "v_mfma_f32_32x32x16_f16" in ln]
        assert not [ln for i0, i1 in zip(mf_i, mf_i[1:]) if i1 - i0 <= 60 for ln in body[i0:i1] if "scratch_" in ln], "scratch traffic inside a tap stream of conv3_wino_sres"
        loads = [ln for ln in body if "global_load_dwordx4" in ln and "lds" not in ln]
        assert len(loads) >= 36 and all("s[" in ln.split("//")[0] for ln in loads), "a weight-fragment load that is not the SGPR-base asm form"
    # (f) the default two-group form (round 4): the same kernel with its taps on v_mfma_f32_16x16x32_f16, K = a pair of taps -- 14 steps x 32
    # MFMAs per chunk for ML = 4 (448 + 336 + 224 + 112); its counted waits need a tap stream free of compiler-made vector-memory operations
    # (a scratch reload drains vmcnt: every prefetched fragment with it), and its halo pieces come from an SGPR base + 32-bit offset
    for sym in ("_ZN3oai15conv3_wino_sresILi2ELi8ELi4ELi1ELb0ELb1EEEvNS_8ConvArgsEPKh", "_ZN3oai15conv3_wino_sresILi1ELi8ELi4ELi1ELb1ELb1EEEvNS_8ConvArgsEPKh"):
        m = re.search(r"^[0-9a-f]+ <" + sym + r">:\n(.*?)(?=^[0-9a-f]+ <)", text, flags=re.S | re.M)
        assert m, f"{sym} not in the library"
        body = m.group(1).split("\n")
        mf_i = [i for i, ln in enumerate(body) if "v_mfma_f32_16x16x32_f16" in ln]
        # (the specialised form's tap-pair variant, round 5: slice-major steps on two fragment sets, the chunk loop unrolled by two + a tail = three bodies of 1120)
        assert len(mf_i) == (1120 if "ILi2E" in sym else 3360) and not [ln for ln in body if "v_mfma_f32_32x32x16_f16" in ln]
        # (the counted waits are the two-group form's: the specialised variant waits with vmcnt(0) only -- a compiler-made reload cannot shift a count there; it
        #  keeps 256 B of scratch, is not the default and not faster, profiles/r05_persistent.md section 4)
        if "ILi2E" in sym:
            assert not [ln for i0, i1 in zip(mf_i, mf_i[1:]) if i1 - i0 <= 60 for ln in body[i0:i1] if "scratch_" in ln], "scratch traffic inside a tap stream of the 16x16x32 form"
        loads = [ln for ln in body if "global_load_dwordx4" in ln and "lds" not in ln]
        assert len(loads) >= 40 and all("s[" in ln.split("//")[0] for ln in loads), "a fragment load that is not the SGPR-base asm form"
    # (the two-group form's halo pieces also come from an SGPR base + 32-bit offset; the specialised form's stagers keep the per-lane 64-bit form)
    assert all("s[" in ln.split("//")[0] for ln in re.search(r"^[0-9a-f]+ <_ZN3oai15conv3_wino_sresILi2ELi8ELi4ELi1ELb0ELb1EEEvNS_8ConvArgsEPKh>:\n(.*?)(?=^[0-9a-f]+ <)", text, flags=re.S | re.M).group(1).split("\n") if "global_load_lds_dwordx4" in ln)
    # (g) round 5: the direct kernel on 16x16x32 tap pairs (conv3_igemm_sres<..., M16>, default for the layers with Cout % 128 != 0): 14 steps of
    # 96 / 64 MFMAs per chunk for ML = 4 (1312 + 984 + 656 + 328), no 32x32x16, no scratch in a tap stream, every fragment load the SGPR-base asm
    # form -- and NO BRANCH WHILE A FRAGMENT LOAD IS IN FLIGHT: an inline-asm load is invisible to the compiler (it believes the result register
    # holds the value from the asm statement on), so a load in flight across a control-flow edge can be copied (`v_mov` of a stale register) or its
    # register re-used.  A first version requested the next chunk's fragments during the last step and the first chunk's in the prologue: the
    # pre-headers of the ML = 1 / 3 loop variants copied the in-flight registers -- intermittently wrong results at small tile levels.
    for sym, first in (("_ZN3oai16conv3_igemm_sresILi4ELi16ELi2ELi4ELi1ELb0ELb1EEEvNS_8ConvArgsEPKh", False),
                       ("_ZN3oai16conv3_igemm_sresILi4ELi16ELi2ELi4ELi1ELb1ELb1EEEvNS_8ConvArgsEPKh", True)):
        m = re.search(r"^[0-9a-f]+ <" + sym + r">:\n(.*?)(?=^[0-9a-f]+ <)", text, flags=re.S | re.M)
        assert m, f"{sym} not in the library"
        body = [ln.split("//")[0] for ln in m.group(1).split("\n")]
        mf_i = [i for i, ln in enumerate(body) if "v_mfma_f32_16x16x32_f16" in ln]
        assert len(mf_i) == (1312 if first else 3280) and not [ln for ln in body if "v_mfma_f32_32x32x16_f16" in ln]
        assert not [ln for i0, i1 in zip(mf_i, mf_i[1:]) if i1 - i0 <= 60 for ln in body[i0:i1] if "scratch_" in ln], "scratch traffic inside a tap stream of the direct 16x16x32 form"
        loads = [ln for ln in body if "global_load_dwordx4" in ln and "lds" not in ln]
        assert len(loads) >= 100 and all("s[" in ln for ln in loads), "a fragment load that is not the SGPR-base asm form"
        in_flight = False
        for ln in body:
            if "global_load_dwordx4" in ln and "lds" not in ln:
                in_flight = True
            elif "s_waitcnt" in ln and "vmcnt(0)" in ln:
                in_flight = False
            elif in_flight and ("s_cbranch" in ln or "s_branch" in ln or "s_setpc" in ln):
                raise AssertionError(f"{sym}: a branch while an inline-asm fragment load is in flight: {ln.strip()}")
    # (h) ADVICE r5 (medium): launch_conv3_shape instantiates the M16 variant for FIVE strip shapes x MREP 2 / 4 as well, all with the same hand-counted
    # `s_waitcnt vmcnt(N)` over inline-asm fragment loads -- a compiler-made spill, reload or edge copy in any of them shifts the counts silently.  The
    # guards run over EVERY conv3_igemm_sres<..., M16 = true> symbol of the library (found by its mangled name, not a hard-coded list): no branch while
    # a fragment load is in flight, no scratch traffic anywhere between two MFMAs of a tap stream, no compiler-made vector-memory load (anything but
    # the asm forms: SGPR-base global_load_dwordx4 and the LDS-DMA pieces) inside a tap stream, only the 16x16x32 shape.
    syms = re.findall(r"^[0-9a-f]+ <(_ZN3oai16conv3_igemm_sresI\w*Lb1EEEvNS_8ConvArgsEPKh)>:", text, flags=re.M)
    assert len(syms) >= 13, f"expected the main, FIRST and 5 x 2 strip instantiations of the M16 direct kernel, found {len(syms)}"
    for sym in syms:
        body = [ln.split("//")[0] for ln in re.search(r"^[0-9a-f]+ <" + sym + r">:\n(.*?)(?=^[0-9a-f]+ <)", text, flags=re.S | re.M).group(1).split("\n")]
        mf_i = [i for i, ln in enumerate(body) if "v_mfma_f32_16x16x32_f16" in ln]
        assert len(mf_i) >= 984 and not [ln for ln in body if "v_mfma_f32_32x32x16_f16" in ln], sym
        assert not [ln for i0, i1 in zip(mf_i, mf_i[1:]) if i1 - i0 <= 60 for ln in body[i0:i1] if "scratch_" in ln], f"{sym}: scratch traffic inside a tap stream"
        loads = [ln for ln in body if "global_load_dwordx4" in ln and "lds" not in ln]
        assert len(loads) >= 100 and all("s[" in ln for ln in loads), f"{sym}: a fragment load that is not the SGPR-base asm form"
        in_flight = False
        for ln in body:
            if "global_load_dwordx4" in ln and "lds" not in ln:
                in_flight = True
            elif "s_waitcnt" in ln and "vmcnt(0)" in ln:
                in_flight = False
            elif in_flight and ("s_cbranch" in ln or "s_branch" in ln or "s_setpc" in ln):
                raise AssertionError(f"{sym}: a branch while an inline-asm fragment load is in flight: {ln.strip()}")
        # (the counted waits live in the tap streams: there every vector-memory load must be one of the two asm forms.  Outside them -- the scatter
        #  copy-out of the FIRST instantiation reads tile boxes -- the compiler issues and waits for its own loads)
        made = [ln.strip() for i0, i1 in zip(mf_i, mf_i[1:]) if i1 - i0 <= 60 for ln in body[i0:i1]
                if re.search(r"\b(scratch_load|buffer_load|global_load_(?!dwordx4|lds_dwordx4))", ln)]
        assert not made, f"{sym}: compiler-made vector-memory loads inside a counted tap stream: {made[:3]}"
    # (i) round 6: conv3_wino_f32 (the exact-fp32 path's k3 kernel).  Its chunk loop leans on the COMPILER's counted waits: every thread issues a fixed
    # number of global loads per chunk (zero padding reads 16 zero bytes instead of skipping the load), so that the weight ring's waits stay
    # `vmcnt(N > 0)` -- with a load under a branch the compiler falls back to full waits and the inputs' latency lands in front of tap 0
    # (profiles/r06_wino_f32.md).  Per instantiation: 9 taps x 16 MFMAs, one barrier per chunk, no full wait and no scratch traffic in the loop.
    for shape in ("ILi8ELi4E", "ILi16ELi2E", "ILi4ELi8E"):
        sym = "_ZN3oai14conv3_wino_f32" + shape + "EEvNS_8ConvArgsEPKf"
        m = re.search(r"^[0-9a-f]+ <" + sym + r">:\n(.*?)(?=^[0-9a-f]+ <)", text, flags=re.S | re.M)
        assert m, f"{sym} not in the library"
        body = [ln.split("//")[0] for ln in m.group(1).split("\n")]
        mf_i = [i for i, ln in enumerate(body) if "v_mfma_f32_32x32x2_f32" in ln]
        assert len(mf_i) == 144, (sym, len(mf_i))
        loop = body[mf_i[0]:mf_i[-1] + 1]
        assert not [ln for ln in body if "scratch_" in ln], f"{sym}: scratch traffic"
        assert not [ln for ln in loop if "s_waitcnt" in ln and "vmcnt(0)" in ln], f"{sym}: a full vmcnt wait inside the chunk loop"
        assert len([ln for ln in loop if "s_barrier" in ln]) == 1, f"{sym}: more than one barrier per chunk"


def test_every_kernel_is_emitted_by_one_translation_unit(tmp_path):
    """The U-Net kernel headers are included by several sources (unet.hip, unet_direct.hip, unet_direct_m16.hip, unet_wino.hip, unet_small.hip): a kernel is compiled
    where its launcher names it, and nowhere else -- no kernel symbol of the whole library is in more than one gfx950 code object (a second copy
    of an instantiation would cost its compile time again and could differ from the first)."""
    import collections
    import glob
    import shutil
    import subprocess
    llvm = os.path.dirname(shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump")
    assert os.path.exists(os.path.join(llvm, "llvm-readelf")), "no llvm-readelf: the code-object checks cannot run (a skipped guard is a failed guard)"
    work = str(tmp_path)
    shutil.copy(build.build_library(verbose=False), os.path.join(work, "lib.so"))
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=work, check=True, capture_output=True)
    where = collections.defaultdict(set)                                 # kernel symbol -> the code objects whose metadata list it
    for o in glob.glob(os.path.join(work, "lib.so.*gfx950*")):
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", o], check=True, capture_output=True, text=True).stdout
        for name in re.findall(r"^\s*\.name:\s+(\S+)$", notes, flags=re.M):
            if re.search(r"^\s*\.symbol:\s+" + re.escape(name) + r"\.kd$", notes, flags=re.M):      # (.name is also a key of kernel arguments)
                where[name].add(o)
    assert len(where) > 300, f"only {len(where)} kernels found in the library's metadata"
    twice = sorted(k for k, objs in where.items() if len(objs) > 1)
    assert not twice, f"kernels in more than one code object: {twice[:5]}"
    assert any("conv3_wino_sres" in k for k in where) and any("conv3_igemm_sres2" in k for k in where) and any("upconv2_igemm_sres" in k for k in where)
