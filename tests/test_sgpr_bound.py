"""The build-time SGPR bound of the steady kernels (build.py check_sgpr_bound).

A CU admits 256-lane workgroups by their scalar registers as well as by VGPRs
and LDS: floor(800 / (ceil(sgprs / 16) * 16 + 16)) of them, so an instance above
80 SGPRs runs 7 waves per SIMD where the compiler's occupancy remark says 8.
The check reads TotalSGPRs (the code object's .sgpr_count) from the same
resource remarks as check_no_scratch.
"""
import glob
import os

import pytest

from dragonboat_amd import build

REMARK = "gr_kernels.h:479:1: remark: "
TAIL = " [-Rpass-analysis=kernel-resource-usage]"


def _remarks(name, sgprs, scratch=0):
    return "\n".join(REMARK + ln + TAIL for ln in (
        f"Function Name: {name}", f"    TotalSGPRs: {sgprs}", "    VGPRs: 56",
        f"    ScratchSize [bytes/lane]: {scratch}", "    Occupancy [waves/SIMD]: 8"))


STEADY = "_ZN2gr16gr_steady_kernelILi3ELi3ELb0EEEvNS_10StepParamsEPjS2_jPKj"
ROLES = "_ZN2gr15gr_roles_kernelILi3ELi3EEEvNS_10StepParamsEPjS2_j"


def admitted(sgprs):
    """256-lane workgroups (= waves per SIMD) a CU admits by SGPRs, at most 8."""
    return min(8, 800 // (-(-sgprs // 16) * 16 + 16))


def test_bound_is_the_eighth_wave():
    assert admitted(build.STEADY_MAX_SGPRS) == 8
    assert admitted(build.STEADY_MAX_SGPRS + 2) == 7  # SGPRs are allocated in pairs


def test_steady_kernel_at_the_bound_passes():
    build.check_sgpr_bound(_remarks(STEADY, build.STEADY_MAX_SGPRS), "x.hip")


def test_steady_kernel_above_the_bound_fails():
    with pytest.raises(RuntimeError, match="gr_steady_kernel.*87 SGPRs"):
        build.check_sgpr_bound(_remarks(STEADY, 87), "x.hip")


def test_other_kernels_are_not_bounded():
    build.check_sgpr_bound(_remarks(ROLES, 106), "x.hip")
    # a steady kernel after another kernel's block is still checked
    with pytest.raises(RuntimeError):
        build.check_sgpr_bound(_remarks(ROLES, 106) + "\n" + _remarks(STEADY, 92), "x.hip")


def test_built_steady_instances_hold_eight_waves():
    """The remarks the product build left: every steady instance within the SGPR
    bound and, at S = 3 (the headline's slot count), within 64 VGPRs."""
    files = glob.glob(os.path.join(build.ENGINE_LIB + ".o.d", "gr_kernels_s*.hip.o.remarks.txt"))
    if not files:  # a library that came without its build directory
        build.build_engine(force=True)
        files = glob.glob(os.path.join(build.ENGINE_LIB + ".o.d", "gr_kernels_s*.hip.o.remarks.txt"))
    assert files
    seen = 0
    for f in files:
        name = None
        for ln in open(f):
            if "Function Name:" in ln:
                name = ln.split("Function Name:", 1)[1].split("[")[0].strip()
            elif name and "gr_steady_kernel" in name and ("TotalSGPRs" in ln or " VGPRs:" in ln):
                n = int(ln.split(":")[-1].split("[")[0].strip())
                if "TotalSGPRs" in ln:
                    seen += 1
                    assert n <= build.STEADY_MAX_SGPRS, (name, n)
                elif "ILi3E" in name:
                    assert n <= 64, (name, n)
    assert seen >= 4  # S = 3: two route modes x LC
