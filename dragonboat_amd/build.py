"""Build recipes for the native parts (run by __graft_entry__.build()).

- libgpuraft.so: the product, HIP for gfx950 (hipcc).
- liboracle.so, kat_tests: the CPU oracle (g++), test infrastructure.
- libhostlane.so: the engine's lane code compiled for the host, test-only.
- libconfig_change_host.so: gr_config_change.h for the host and its reference side, test-only.
- libhostlane_snap.so, libhostlane_snap_elect.so: the host lane with snapshots compiled on and
  their reference side, test-only.
- libhostlane_cc.so, libhostlane_cc_elect.so: the host lane with config-change entries compiled
  on and their reference side, test-only.
- libhostlane_all.so: the host lane with elections, snapshots and config-change entries all
  compiled on and the reference side for that configuration, test-only.
Outputs stay in-tree (git-ignored) so they travel to the GPU box.
"""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

CSRC = os.path.join(ROOT, "dragonboat_amd", "csrc")
# the C-ABI + boundary passes, and one translation unit per slot count (compiled in parallel)
ENGINE_SRC = [os.path.join(CSRC, "gr_engine.hip")] + [os.path.join(CSRC, f"gr_kernels_s{s}.hip") for s in (1, 3, 5, 8)]
ENGINE_DEPS = ENGINE_SRC + [os.path.join(CSRC, f)
                            for f in ("gr_lane.h", "gr_layout.h", "gr_host.h", "gr_fast.h", "gr_steady.h", "gr_tick.h", "gr_io.h",
                                      "gr_cover.h", "gr_kernels.h", "gr_scan.h", "gr_quiesce.h", "gr_config_change.h")] + \
    [os.path.join(ROOT, "include", "gpuraft.h")]
JOBS = max(1, min(8, os.cpu_count() or 1))
ENGINE_LIB = os.path.join(ROOT, "dragonboat_amd", "_build", "libgpuraft.so")
COVER_LIB = os.path.join(ROOT, "dragonboat_amd", "_build", "libgpuraft_cover.so")
ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
KAT_BIN = os.path.join(ROOT, "oracle", "_build", "kat_tests")
HOSTLANE_LIB = os.path.join(ROOT, "tests", "_build", "libhostlane.so")
HOSTLANE_ELECT_LIB = os.path.join(ROOT, "tests", "_build", "libhostlane_elect.so")
QUIESCE_HOST_LIB = os.path.join(ROOT, "tests", "_build", "libquiesce_host.so")
STEADY_WU_HOST_LIB = os.path.join(ROOT, "tests", "_build", "libsteady_wu_host.so")
CONFIG_CHANGE_HOST_LIB = os.path.join(ROOT, "tests", "_build", "libconfig_change_host.so")
HOSTLANE_SNAP_LIB = os.path.join(ROOT, "tests", "_build", "libhostlane_snap.so")
HOSTLANE_SNAP_ELECT_LIB = os.path.join(ROOT, "tests", "_build", "libhostlane_snap_elect.so")
HOSTLANE_CC_LIB = os.path.join(ROOT, "tests", "_build", "libhostlane_cc.so")
HOSTLANE_CC_ELECT_LIB = os.path.join(ROOT, "tests", "_build", "libhostlane_cc_elect.so")
HOSTLANE_ALL_LIB = os.path.join(ROOT, "tests", "_build", "libhostlane_all.so")
WIRE_SRC = os.path.join(ROOT, "dragonboat_amd", "csrc", "gr_wire.hip")
WIRE_DEPS = [WIRE_SRC, os.path.join(ROOT, "include", "gpuraft_wire.h"), os.path.join(ROOT, "include", "gpuraft.h"),
             os.path.join(CSRC, "gr_scan.h")]
WIRE_LIB = os.path.join(ROOT, "dragonboat_amd", "_build", "libgrwire.so")
WIRE_ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "liboraclewire.so")
HBM_CALIB = os.path.join(ROOT, "tools", "hbm_calib")


def _code_only(text):
    """C/C++ source without comments or blank lines (string literals kept)."""
    import re
    pat = re.compile(r'"(?:\\.|[^"\\])*"|//[^\n]*|/\*.*?\*/', re.S)
    text = pat.sub(lambda m: m.group(0) if m.group(0).startswith('"') else " ", text)
    return "\n".join(ln.rstrip() for ln in text.splitlines() if ln.strip())


def source_digest(deps=None):
    """Digest of the engine's code (comments and blank lines stripped): ties a
    PMC measurement (profiles/) to the build it measured; comment edits keep it.
    deps: another target's sources (its build record's digest)."""
    import hashlib
    h = hashlib.sha1()
    for f in sorted(deps or ENGINE_DEPS):
        with open(f, encoding="utf-8") as fh:
            h.update(_code_only(fh.read()).encode())
    return h.hexdigest()[:16]


def _locked(out):
    """An exclusive lock on `out`'s build (test workers build on first use, side
    by side: one builds, the others wait and then find it fresh)."""
    import fcntl
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lk = open(out + ".lock", "w")
    fcntl.flock(lk, fcntl.LOCK_EX)
    return lk


def _stale(out, deps, extra=None):
    """A target needs building when it is missing or its build record's digest
    (and flags, when given) differ from its sources' now. Digests, not mtimes: a
    prebuilt library pushed with a tree whose sources differ (the GPU box gets
    fresh mtimes for both) is rebuilt; a comment-only edit is not. A target
    without a record falls back to mtimes (the CPU-only test builds)."""
    if not os.path.exists(out):
        return True
    rec = build_record(out)
    if rec is not None and "source_digest" in rec:
        if extra is not None and list(rec.get("flags", [])) != list(extra):
            return True
        return rec["source_digest"] != source_digest(deps)
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"build failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return r.stderr


# Kernels that must not touch scratch memory: one spilled register array in the
# lean lane made a 1M x 3 pass 6x slower (0.82 vs 0.13 ms) and moved 3 GB of
# scratch traffic per launch. The compiler's resource remarks are checked at
# build time, so such a build fails instead of shipping.
NO_SCRATCH_KERNELS = ("gr_fast_kernel", "gr_roles_kernel", "gr_steady_kernel",
                      "update_classify")  # gr_collect_updates' first pass reads rows, builds no record
RESOURCE_REMARKS = "-Rpass-analysis=kernel-resource-usage"


def check_no_scratch(remarks, src):
    """Parse hipcc's kernel-resource-usage remarks; raise if a NO_SCRATCH kernel uses scratch."""
    name = None
    for ln in remarks.splitlines():
        if "Function Name:" in ln:
            name = ln.split("Function Name:", 1)[1].split("[")[0].strip()
        elif "ScratchSize" in ln and name and any(k in name for k in NO_SCRATCH_KERNELS):
            size = int(ln.split(":")[-1].split("[")[0].strip())
            if size:
                raise RuntimeError(f"{os.path.basename(src)}: {name} uses {size} B/lane of scratch")


# Kernels that must stay within a scalar-register count: a CU admits 256-lane
# workgroups by their SGPRs too, floor(800 / (ceil(sgprs / 16) * 16 + 16)) of
# them, so a steady-kernel instance above 80 runs 7 waves per SIMD, not 8, while
# the compiler's occupancy remark still says 8 (gr_kernels.h kSteadySgprs).
# TotalSGPRs of the remarks is the code object's .sgpr_count.
STEADY_MAX_SGPRS = 80
SGPR_BOUND_KERNELS = {"gr_steady_kernel": STEADY_MAX_SGPRS}


def check_sgpr_bound(remarks, src):
    """Parse the same remarks; raise if a kernel of SGPR_BOUND_KERNELS uses more SGPRs than its bound."""
    name = None
    for ln in remarks.splitlines():
        if "Function Name:" in ln:
            name = ln.split("Function Name:", 1)[1].split("[")[0].strip()
        elif "TotalSGPRs" in ln and name:
            n = int(ln.split(":")[-1].split("[")[0].strip())
            for k, bound in SGPR_BOUND_KERNELS.items():
                if k in name and n > bound:
                    raise RuntimeError(f"{os.path.basename(src)}: {name} uses {n} SGPRs, above {bound}")


def _hip_lib(out, srcs, deps, extra=(), force=False, scratch_check=True):
    """Compile every source to an object in parallel (hipcc, gfx950), then link `out`.
    scratch_check: refuse lean-kernel instances that use scratch, and steady
    instances above their SGPR bound (product builds; the coverage build's hit
    counters cost registers, and it is never timed)."""
    if not (force or _stale(out, deps, extra)):
        return out
    with _locked(out):
        if not (force or _stale(out, deps, extra)):  # built while this worker waited
            return out
        return _hip_lib_locked(out, srcs, deps, extra, scratch_check)


def _hip_lib_locked(out, srcs, deps, extra, scratch_check):
    digest = source_digest(deps)  # before compiling: the record names what was compiled
    odir = out + ".o.d"
    os.makedirs(odir, exist_ok=True)
    # the lean lane's message loop (gr_fast.h: slots x messages, each able to
    # broadcast) must unroll fully, or its per-slot arrays become scratch: the
    # default pragma-unroll size limit (16K) is just below what S = 3 needs
    flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", *extra,
             "-mllvm", "-pragma-unroll-threshold=100000",
             "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = [os.path.join(odir, os.path.basename(s) + ".o") for s in srcs]
    with ThreadPoolExecutor(JOBS) as ex:
        futs = [ex.submit(_run, [HIPCC, *flags, RESOURCE_REMARKS, "-c", s, "-o", o]) for s, o in zip(srcs, objs)]
        for s, f, o in zip(srcs, futs, objs):
            r = f.result()
            with open(o + ".remarks.txt", "w") as fh:  # per-kernel VGPRs/occupancy, for inspection
                fh.write(r)
            if scratch_check:
                check_no_scratch(r, s)
                check_sgpr_bound(r, s)
    _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", *objs, "-o", out])
    write_build_record(out, extra, digest, deps)
    return out


def write_build_record(out, extra=(), digest=None, deps=None):
    """<lib>.build.json beside a built library: the source digest it was built
    from (taken before compiling), when, and by which compiler (bench.py reports
    it with the digest of the tree it runs in, so a stale prebuilt library
    shows). A source edited during the build leaves no record, so the next
    build() compiles again instead of claiming the newer tree."""
    import json
    import time
    try:
        ver = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()
        ver = next((v for v in ver if "HIP version" in v or "clang version" in v), ver[0] if ver else "")
    except OSError:
        ver = ""
    digest = digest or source_digest(deps)
    if source_digest(deps) != digest:
        try:
            os.unlink(out + ".build.json")
        except OSError:
            pass
        return
    rec = {"lib": os.path.basename(out), "source_digest": digest, "built_at": time.strftime("%Y-%m-%dT%H:%M:%S"),
           "compiler": ver.strip(), "arch": ARCH, "flags": list(extra)}
    with open(out + ".build.json", "w") as fh:
        json.dump(rec, fh)


def build_record(lib=None):
    """The build record of a library (default: the engine), or None."""
    import json
    try:
        with open((lib or ENGINE_LIB) + ".build.json") as fh:
            return json.load(fh)
    except (OSError, ValueError):
        return None


def build_engine(force=False):
    return _hip_lib(ENGINE_LIB, ENGINE_SRC, ENGINE_DEPS, force=force)


def build_engine_cover(force=False):
    """libgpuraft_cover.so: the same engine with per-branch hit counters
    (-DGR_COVERAGE, gr_cover.h), for tests/test_coverage.py only."""
    return _hip_lib(COVER_LIB, ENGINE_SRC, ENGINE_DEPS, extra=("-DGR_COVERAGE",), force=force, scratch_check=False)


def build_oracle(force=False):
    odir = os.path.join(ROOT, "oracle")
    os.makedirs(os.path.dirname(ORACLE_LIB), exist_ok=True)
    hdrs = [os.path.join(odir, f) for f in ("raft_oracle.hpp", "oracle_testkit.hpp")] + \
        [os.path.join(ROOT, "include", "gpuraft.h")]
    src = os.path.join(odir, "batch.cpp")
    if force or _stale(ORACLE_LIB, hdrs + [src]):
        _run(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-I" + odir,
              "-I" + os.path.join(ROOT, "include"), src, "-o", ORACLE_LIB, "-lpthread"])
    kat = os.path.join(odir, "kat_tests.cpp")
    if force or _stale(KAT_BIN, hdrs + [kat]):
        _run(["g++", "-std=c++17", "-O1", "-g", "-I" + odir, kat, "-o", KAT_BIN])
    return ORACLE_LIB


def build_hostlane(force=False, out=HOSTLANE_LIB, extra=()):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "hostlane.hip")
    deps = ENGINE_DEPS + [src]
    if not (force or _stale(out, deps)):
        return out
    with _locked(out):
        if not (force or _stale(out, deps)):
            return out
        _run([HIPCC, "--cuda-host-only", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-DGR_COVERAGE", *extra,
              "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dragonboat_amd", "csrc"),
              src, "-o", out])
    return out


def build_hostlane_elect(force=False):
    """libhostlane_elect.so: the same host lane with elections compiled on
    (-DGR_ELECTIONS_FORCE=1; its harness zeroes StepParams, so the run-time
    switch cannot reach it), for tests/test_elections_hostlane.py."""
    return build_hostlane(force, HOSTLANE_ELECT_LIB, ("-DGR_ELECTIONS_FORCE=1",))


def build_quiesce_host(force=False):
    """libquiesce_host.so: gr_quiesce.h (the quiesce manager the device kernel
    runs) compiled by g++ behind a C interface, for tests/test_quiesce.py."""
    os.makedirs(os.path.dirname(QUIESCE_HOST_LIB), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "quiesce_host.cpp")
    deps = [src, os.path.join(CSRC, "gr_quiesce.h"), os.path.join(ROOT, "include", "gpuraft.h")]
    if not (force or _stale(QUIESCE_HOST_LIB, deps)):
        return QUIESCE_HOST_LIB
    with _locked(QUIESCE_HOST_LIB):
        if force or _stale(QUIESCE_HOST_LIB, deps):
            _run(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                  "-I" + CSRC, src, "-o", QUIESCE_HOST_LIB])
    return QUIESCE_HOST_LIB


def build_steady_wu_host(force=False):
    """libsteady_wu_host.so: the steady kernel's wave-uniform addressing and its
    predicate (gr_steady.h WaveAddr, gr_layout.h steady_wu_routes) compiled for
    the host behind a C interface, for tests/test_steady_wu.py."""
    os.makedirs(os.path.dirname(STEADY_WU_HOST_LIB), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "steady_wu_host.hip")
    deps = ENGINE_DEPS + [src]
    if not (force or _stale(STEADY_WU_HOST_LIB, deps)):
        return STEADY_WU_HOST_LIB
    with _locked(STEADY_WU_HOST_LIB):
        if force or _stale(STEADY_WU_HOST_LIB, deps):
            _run([HIPCC, "--cuda-host-only", "-O2", "-g", "-std=c++17", "-fPIC", "-shared",
                  "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, src, "-o", STEADY_WU_HOST_LIB])
    return STEADY_WU_HOST_LIB


def build_config_change_host(force=False):
    """libconfig_change_host.so: gr_config_change.h (what gr_apply_config_change
    runs on the device) compiled for the host over gr_peer records, and the
    reference side (the oracle's raft object driven through its own
    build_peer / export_peer), for tests/test_config_change.py."""
    os.makedirs(os.path.dirname(CONFIG_CHANGE_HOST_LIB), exist_ok=True)
    odir = os.path.join(ROOT, "oracle")
    src = os.path.join(ROOT, "tests", "native", "config_change_host.hip")
    ref = os.path.join(ROOT, "tests", "native", "config_change_ref.cpp")
    deps = [src, ref, os.path.join(ROOT, "include", "gpuraft.h"), os.path.join(odir, "batch.cpp"),
            os.path.join(odir, "raft_oracle.hpp")] + \
        [os.path.join(CSRC, f) for f in ("gr_config_change.h", "gr_host.h", "gr_layout.h", "gr_quiesce.h")]
    if not (force or _stale(CONFIG_CHANGE_HOST_LIB, deps)):
        return CONFIG_CHANGE_HOST_LIB
    with _locked(CONFIG_CHANGE_HOST_LIB):
        if force or _stale(CONFIG_CHANGE_HOST_LIB, deps):
            inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + odir]
            objs = [CONFIG_CHANGE_HOST_LIB + ".host.o", CONFIG_CHANGE_HOST_LIB + ".ref.o"]
            _run([HIPCC, "--cuda-host-only", "-O2", "-g", "-std=c++17", "-fPIC", *inc, "-c", src, "-o", objs[0]])
            _run(["g++", "-std=c++17", "-O2", "-g", "-fPIC", *inc, "-c", ref, "-o", objs[1]])
            _run([HIPCC, "-shared", "-fPIC", *objs, "-o", CONFIG_CHANGE_HOST_LIB, "-lpthread"])
    return CONFIG_CHANGE_HOST_LIB


def _hostlane_with_ref(out, src, ref, macros, force, extra_deps=()):
    """A host-lane build (tests/native/<src>, hipcc host-only with -DGR_COVERAGE
    and `macros`) linked with its reference side (tests/native/<ref>, g++ over
    oracle/batch.cpp and tests/native/ref_pass.h) into `out`."""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    odir = os.path.join(ROOT, "oracle")
    native = os.path.join(ROOT, "tests", "native")
    src, ref = os.path.join(native, src), os.path.join(native, ref)
    deps = ENGINE_DEPS + [src, ref, os.path.join(native, "hostlane.hip"),
                          os.path.join(odir, "batch.cpp"), os.path.join(odir, "raft_oracle.hpp")] + \
        [os.path.join(native, d) for d in extra_deps]
    with open(ref, encoding="utf-8") as fh:  # the shared pass header, where the reference side includes it
        if '#include "ref_pass.h"' in fh.read():
            deps.append(os.path.join(native, "ref_pass.h"))
    if not (force or _stale(out, deps)):
        return out
    with _locked(out):
        if force or _stale(out, deps):
            inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + odir]
            objs = [out + ".host.o", out + ".ref.o"]
            with ThreadPoolExecutor(2) as ex:
                fs = [ex.submit(_run, [HIPCC, "--cuda-host-only", "-O2", "-g", "-std=c++17", "-fPIC", "-DGR_COVERAGE",
                                       *macros, *inc, "-c", src, "-o", objs[0]]),
                      ex.submit(_run, ["g++", "-std=c++17", "-O2", "-g", "-fPIC", *inc, "-c", ref, "-o", objs[1]])]
                for f in fs:
                    f.result()
            _run([HIPCC, "-shared", "-fPIC", *objs, "-o", out, "-lpthread"])
    return out


def build_hostlane_snap(force=False, out=HOSTLANE_SNAP_LIB, extra=()):
    """libhostlane_snap.so: the host lane with snapshots compiled on
    (tests/native/hostlane_snap.hip, -DGR_SNAPSHOTS_FORCE=1: its harness zeroes
    StepParams, so the run-time switch cannot reach it) and the reference side
    (tests/native/snapshot_ref.cpp, the oracle's raft object driven through its
    own build_peer / export_peer), for tests/test_snapshots.py."""
    return _hostlane_with_ref(out, "hostlane_snap.hip", "snapshot_ref.cpp", ("-DGR_SNAPSHOTS_FORCE=1", *extra), force)


def build_hostlane_snap_elect(force=False):
    """libhostlane_snap_elect.so: the same with elections compiled on too, for
    the candidate's InstallSnapshot handler."""
    return build_hostlane_snap(force, HOSTLANE_SNAP_ELECT_LIB, ("-DGR_ELECTIONS_FORCE=1",))


def build_hostlane_cc(force=False, out=HOSTLANE_CC_LIB, extra=()):
    """libhostlane_cc.so: the host lane with config-change entries compiled on
    (tests/native/hostlane_cc.hip, -DGR_CONFIG_ENTRIES_FORCE=1: its harness zeroes
    StepParams, so the run-time switch cannot reach it) and the reference side
    (tests/native/config_entries_ref.cpp, the oracle's raft object with typed
    in-memory entries), for tests/test_config_entries.py."""
    return _hostlane_with_ref(out, "hostlane_cc.hip", "config_entries_ref.cpp",
                              ("-DGR_CONFIG_ENTRIES_FORCE=1", *extra), force)


def build_hostlane_cc_elect(force=False):
    """libhostlane_cc_elect.so: the same with elections compiled on too, for
    promotions over uncommitted entries."""
    return build_hostlane_cc(force, HOSTLANE_CC_ELECT_LIB, ("-DGR_ELECTIONS_FORCE=1",))


def build_hostlane_all(force=False):
    """libhostlane_all.so: the host lane with elections, snapshots and
    config-change entries all compiled on (tests/native/hostlane_all.hip; the
    three _FORCE macros) and the reference side that speaks both message
    conventions over a typed log (tests/native/all_switches_ref.cpp), for
    tests/test_all_switches.py."""
    native = os.path.join(ROOT, "tests", "native")
    own = [os.path.join(native, f) for f in ("hostlane_all.hip", "all_switches_ref.cpp")]
    if not any(os.path.exists(f) for f in own):
        # A tests/ tree from before this target (an older suite run against this
        # engine) has neither of its sources and no test that loads it: nothing to
        # build, and no stale library left behind. One source without the other
        # is a broken tree and fails below like any missing source.
        if os.path.exists(HOSTLANE_ALL_LIB):
            os.unlink(HOSTLANE_ALL_LIB)
        return None
    return _hostlane_with_ref(HOSTLANE_ALL_LIB, "hostlane_all.hip", "all_switches_ref.cpp",
                              ("-DGR_ELECTIONS_FORCE=1", "-DGR_SNAPSHOTS_FORCE=1", "-DGR_CONFIG_ENTRIES_FORCE=1"), force,
                              extra_deps=("hostlane_snap.hip",))


ORACLE_SAN_LIB = os.path.join(ROOT, "oracle", "_build", "liboracle_san.so")
KAT_SAN_BIN = os.path.join(ROOT, "oracle", "_build", "kat_tests_san")
HOSTLANE_SAN_LIB = os.path.join(ROOT, "tests", "_build", "libhostlane_san.so")
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def build_sanitized(force=False):
    """ASAN + UBSAN builds of the host code the CPU tests run:
    the oracle library and KAT binary (g++), and the host build of the lane code
    (hipcc host-only; -fno-gpu-sanitize: host code only). tests/test_sanitizers.py
    runs parity workloads through them with the matching runtime preloaded.
    Test workers call this concurrently: one builds, the others wait on the lock."""
    import fcntl
    os.makedirs(os.path.dirname(HOSTLANE_SAN_LIB), exist_ok=True)
    with open(HOSTLANE_SAN_LIB + ".lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        return _build_sanitized(force)


def _build_sanitized(force):
    odir = os.path.join(ROOT, "oracle")
    hdrs = [os.path.join(odir, f) for f in ("raft_oracle.hpp", "oracle_testkit.hpp")] + \
        [os.path.join(ROOT, "include", "gpuraft.h")]
    src = os.path.join(odir, "batch.cpp")
    os.makedirs(os.path.dirname(ORACLE_SAN_LIB), exist_ok=True)
    os.makedirs(os.path.dirname(HOSTLANE_SAN_LIB), exist_ok=True)
    jobs = []  # independent compiles, side by side
    if force or _stale(ORACLE_SAN_LIB, hdrs + [src]):
        jobs.append(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", *SAN_FLAGS, "-I" + odir,
                     "-I" + os.path.join(ROOT, "include"), src, "-o", ORACLE_SAN_LIB, "-lpthread"])
    kat = os.path.join(odir, "kat_tests.cpp")
    if force or _stale(KAT_SAN_BIN, hdrs + [kat]):
        jobs.append(["g++", "-std=c++17", "-O1", "-g", *SAN_FLAGS, "-I" + odir, kat, "-o", KAT_SAN_BIN])
    hsrc = os.path.join(ROOT, "tests", "native", "hostlane.hip")
    if force or _stale(HOSTLANE_SAN_LIB, ENGINE_DEPS + [hsrc]):
        jobs.append([HIPCC, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-DGR_COVERAGE",
                     "-DGR_HL_SLOTS_35", "-fno-gpu-sanitize", *SAN_FLAGS, "-shared-libsan",
                     "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dragonboat_amd", "csrc"),
                     hsrc, "-o", HOSTLANE_SAN_LIB])
    with ThreadPoolExecutor(3) as ex:
        for f in [ex.submit(_run, j) for j in jobs]:
            f.result()
    return ORACLE_SAN_LIB, HOSTLANE_SAN_LIB


WIRE_OUT_SAN_BIN = os.path.join(ROOT, "tests", "_build", "wire_out_san")


def build_wire_out_san(force=False):
    """tests/_build/wire_out_san: a stand-alone CPU program (its own main) that
    drives gr_wire_out_host's code (gr_host.h) over seeded records under ASAN +
    UBSAN, for tests/test_wire_out_host.py. Host code only; it is run directly."""
    os.makedirs(os.path.dirname(WIRE_OUT_SAN_BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "native", "wire_out_san.hip")
    deps = [src, os.path.join(ROOT, "include", "gpuraft.h"), os.path.join(ROOT, "include", "gpuraft_wire.h")] + \
        [os.path.join(CSRC, f) for f in ("gr_host.h", "gr_layout.h", "gr_quiesce.h")]
    if not (force or _stale(WIRE_OUT_SAN_BIN, deps)):
        return WIRE_OUT_SAN_BIN
    with _locked(WIRE_OUT_SAN_BIN):
        if force or _stale(WIRE_OUT_SAN_BIN, deps):
            _run([HIPCC, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-gpu-sanitize",
                  *[a for f in SAN_FLAGS for a in ("-Xarch_host", f)],
                  "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, src, "-o", WIRE_OUT_SAN_BIN])
    return WIRE_OUT_SAN_BIN


def build_wire(force=False):
    """libgrwire.so: the wire codec (include/gpuraft_wire.h)."""
    os.makedirs(os.path.dirname(WIRE_LIB), exist_ok=True)
    if not (force or _stale(WIRE_LIB, WIRE_DEPS, ())):
        return WIRE_LIB
    with _locked(WIRE_LIB):
        if force or _stale(WIRE_LIB, WIRE_DEPS, ()):
            digest = source_digest(WIRE_DEPS)
            _run([HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared",
                  "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, WIRE_SRC, "-o", WIRE_LIB])
            write_build_record(WIRE_LIB, (), digest, WIRE_DEPS)
    return WIRE_LIB


def build_wire_oracle(force=False):
    """liboraclewire.so: the codec's CPU restatement (test infrastructure)."""
    odir = os.path.join(ROOT, "oracle")
    os.makedirs(os.path.dirname(WIRE_ORACLE_LIB), exist_ok=True)
    deps = [os.path.join(odir, "wire_oracle.hpp"), os.path.join(odir, "wire_capi.cpp"),
            os.path.join(ROOT, "include", "gpuraft_wire.h")]
    if force or _stale(WIRE_ORACLE_LIB, deps):
        _run(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-I" + odir, "-I" + os.path.join(ROOT, "include"),
              os.path.join(odir, "wire_capi.cpp"), "-o", WIRE_ORACLE_LIB, "-lpthread"])
    return WIRE_ORACLE_LIB


def build_tools(force=False):
    """tools/hbm_calib: known-byte-count kernels that calibrate the PMC byte counters."""
    src = HBM_CALIB + ".hip"
    if force or _stale(HBM_CALIB, [src]):
        _run([HIPCC, f"--offload-arch={ARCH}", "-O3", src, "-o", HBM_CALIB])
    return HBM_CALIB


def build_all(force=False):
    # independent targets side by side (each engine build also compiles its units in parallel)
    with ThreadPoolExecutor(10) as ex:
        fs = [ex.submit(f, force) for f in (build_engine, build_engine_cover, build_hostlane, build_hostlane_elect, build_wire,
                                            build_hostlane_snap, build_hostlane_snap_elect,
                                            build_hostlane_cc, build_hostlane_cc_elect, build_hostlane_all)]
        build_oracle(force)
        build_wire_oracle(force)
        build_tools(force)
        build_quiesce_host(force)
        build_steady_wu_host(force)
        build_config_change_host(force)
        for f in fs:
            f.result()
