"""CPU checks of the conv kernels' dynamic-LDS geometry (csrc/conv_lds.h): the one statement of
every plane size, offset, launch size and admission test that kernels, planners and launchers
share."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monodepth2.jl_amd", "csrc")
LIB = os.path.join(ROOT, "monodepth2.jl_amd", "lib", "libmd2hip.so")


def _host_cxx():
    for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError("no host C++ compiler")


def test_conv_lds_geometry_sweep(tmp_path):
    """tests/stubs/conv_lds_check.cpp, compiled for the host only: over every geometry the
    planners can see, fits => need <= bytes <= cap, fits equals the admission test the planners
    used to write out, the bench shapes are admitted and the fixed sizes are 141312 / 79872 /
    65280 bytes (62080 for conv_whalo at 32 x 104)."""
    exe = str(tmp_path / "conv_lds_check")
    subprocess.run([_host_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "stubs", "conv_lds_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout, r.stdout


def test_lds_sizes_stated_only_in_the_header():
    """Planners and launchers keep no LDS byte count or plane formula of their own."""
    names = sorted(n for n in os.listdir(CSRC) if n.startswith("conv") and n != "conv_lds.h")
    assert names
    attr_files = []
    for name in names:
        src = open(os.path.join(CSRC, name)).read()
        for pat in (r"65536", r"163840", r"\b448\b", r"16 \* 7 \* 4", r"HX_PLANE =", r"\* 64\) \+ ",
                    r"hipFuncAttributeMaxDynamicSharedMemorySize"):
            hits = [m.start() for m in re.finditer(pat, src)]
            # the one attribute call is lds_launch's, in the file that defines it
            allowed = 1 if (pat.startswith("hipFunc") and re.search(r"\bint lds_launch\(", src)) else 0
            assert len(hits) == allowed, (name, pat, len(hits))
            attr_files += [name] * (len(hits) if pat.startswith("hipFunc") else 0)
    assert len(attr_files) == 1, attr_files


def test_timing_variants_not_in_the_library():
    """The wrong-result timing kernels and their knobs are a -DMD2_TIMING_VARIANTS=1 build only."""
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    blob = open(LIB, "rb").read()
    for knob in (b"MD2_HX_DBG", b"MD2_WHX_DBG", b"MD2_STEM_DBG", b"MD2_WSTEM_DBG"):
        assert knob not in blob, knob
