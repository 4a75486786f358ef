"""In-tree build of the native libraries.

  libredsec_hip.so   the product: HIP kernels + C ABI (include/redsec_hip.h), gfx950 only
  librs_emulate.so   test-only host emulation of one wavefront (csrc/rs_emulate.cpp)

hipcc cross-compiles for gfx950 without a GPU, so `build()` works in the CPU-only container. The
built .so files stay in-tree (git-ignored) so that they travel to the GPU box with the snapshot.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")

HIP_LIB = os.path.join(HERE, "libredsec_hip.so")
EMU_LIB = os.path.join(HERE, "librs_emulate.so")

HIP_SOURCES = ["rs_bootstrap.hip", "rs_general.hip", "rs_kernels.hip", "rs_seeded.hip", "rs_audit.hip", "rs_api.cpp"]
HIP_DEPS = HIP_SOURCES + ["rs_kernels.h", "rs_cohort.h", "rs_diag.h", "rs_lds_plan.h", "rs_ntt.h", "rs_fft.h", "rs_general.h", "rs_keygen.h", "rs_audit.h", "rs_host.h", os.path.join(INCLUDE, "redsec_hip.h")]
# Objects of the product library: (object name, source, extra flags). rs_bootstrap.hip is compiled three times (its RS_BS_PART
# switch): part 1 -- the FFT / exact-NTT blind-rotation kernels and the split duo form -- with LLVM's post-register-allocation
# scheduler off: its in-block reordering of the hand-laid-out LDS / FP64 sequences costs these kernels 1-3 % (same-box A/B,
# profiles/r03/y_ab_compiler_scheduling_*.txt: default-128 +1.3 %, REDsec set +0.9 %, sign1024x1 image 12.36 -> 12.11 ms);
# part 2 -- the split cooperative and split lock-step kernels -- keeps that pass (they lose 6 % / 0.7 % without it) and is
# scheduled with the max-memory-clause strategy: the cooperative kernel streams the key from L2 by itself and gains 6.5 % from
# clustered loads (196-neuron layer 4.33 -> 4.05 ms, split-mode sign1024x1 16.3 -> 15.95 ms; the lock-step kernel -0.5 % / +0.3 %);
# the other files use the default pipeline (the (9, 3) keyswitch in rs_kernels.hip loses 12 % without the post-RA pass).
HIP_OBJECTS = [
    ("rs_bootstrap_1", "rs_bootstrap.hip", ["-DRS_BS_PART=1", "-mllvm", "-enable-post-misched=0"]),
    ("rs_bootstrap_2", "rs_bootstrap.hip", ["-DRS_BS_PART=2", "-mllvm", "-amdgpu-sched-strategy=max-memory-clause"]),
    # part 4 -- blind_rotate_coop8_listed_kernel (round 6) with part 1's flags, in an object of its own: instantiated inside part 1
    # it changed the instructions of 15 other kernels there (tools/codeobj_digest.py), the measured BASELINE-config forms among them
    ("rs_bootstrap_4", "rs_bootstrap.hip", ["-DRS_BS_PART=4", "-mllvm", "-enable-post-misched=0"]),
    ("rs_general", "rs_general.hip", []),
    ("rs_kernels", "rs_kernels.hip", []),
    # seeded ciphertexts (seeded_lwe_kernel) in an object of their own: every kernel of rs_general keeps its instructions
    ("rs_seeded", "rs_seeded.hip", []),
    # device decryption and the key audit (lwe_phase_kernel, audit_bk_kernel, audit_ksk_kernel), likewise in an object of their own
    ("rs_audit", "rs_audit.hip", []),
    ("rs_api", "rs_api.cpp", []),
]
EMU_SOURCES = ["rs_emulate.cpp"]
EMU_DEPS = EMU_SOURCES + ["rs_lds_plan.h", "rs_ntt.h", "rs_fft.h", "rs_general.h", "rs_keygen.h", "rs_audit.h", "rs_host.h"]


def _abs(paths):
    return [p if os.path.isabs(p) else os.path.join(CSRC, p) for p in paths]


def fingerprint(paths, extra=""):
    """sha256 over the CONTENTS of `paths` (and `extra`, e.g. the compiler flags): what a built artefact was made from."""
    import hashlib
    h = hashlib.sha256(extra.encode())
    for p in paths:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def is_stale(target, deps, extra=""):
    """A target is up to date when `<target>.stamp` holds the fingerprint of its present dependencies. Content-based, not
    mtime-based: a snapshot pushed to another machine (the GPU box) never recompiles what was built from the same sources,
    whatever the copy did to the timestamps, and an edited source always does."""
    stamp = target + ".stamp"
    if not (os.path.exists(target) and os.path.exists(stamp)):
        return True
    try:
        return open(stamp).read().strip() != fingerprint(deps, extra)
    except OSError:
        return True


def write_stamp(target, deps, extra=""):
    with open(target + ".stamp", "w") as f:
        f.write(fingerprint(deps, extra) + "\n")


def _stale(target, deps):
    return is_stale(target, _abs(deps) + [os.path.abspath(__file__)])



def find_hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def _locked(name):
    """Exclusive advisory lock for one build target: several ranks of a torch.distributed.run job may import the package at the
    same moment on a tree whose stamp is missing, and must not write the same objects and library side by side."""
    import fcntl
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    f = open(os.path.join(ROOT, "build", "." + name + ".lock"), "w")
    fcntl.flock(f, fcntl.LOCK_EX)
    return f


def _publish(tmp, target, deps):
    """Stamp first (under a temporary name), then both renamed into place: a reader never sees a half-written library."""
    write_stamp(tmp, _abs(deps) + [os.path.abspath(__file__)])
    os.replace(tmp, target)
    os.replace(tmp + ".stamp", target + ".stamp")


def build_hip(force=False, verbose=False):
    if not force and not _stale(HIP_LIB, HIP_DEPS):
        return HIP_LIB
    hipcc = find_hipcc()
    if hipcc is None:
        if os.path.exists(HIP_LIB):
            return HIP_LIB  # prebuilt library shipped with the snapshot
        raise RuntimeError("hipcc not found and no prebuilt libredsec_hip.so present")
    lock = _locked("hip")
    try:
        if not force and not _stale(HIP_LIB, HIP_DEPS):     # another process built it while this one waited for the lock
            return HIP_LIB
        # One object per source (compiled side by side), then one link: the files carry different code-generation flags.
        # Objects and the linked library are written under per-process names and renamed into place.
        objdir = os.path.join(ROOT, "build", "obj.%d" % os.getpid())
        os.makedirs(objdir, exist_ok=True)
        common = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-I" + INCLUDE, "-I" + CSRC]
        jobs, objs = [], []
        for name, src, extra in HIP_OBJECTS:
            obj = os.path.join(objdir, name + ".o")
            cmd = common + extra + ["-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd)))
            objs.append(obj)
        try:
            for cmd, job in jobs:
                if job.wait() != 0:
                    raise subprocess.CalledProcessError(job.returncode, cmd)
            tmp = HIP_LIB + ".tmp.%d" % os.getpid()
            cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", tmp]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            _publish(tmp, HIP_LIB, HIP_DEPS)
        finally:
            for _, job in jobs:
                if job.poll() is None:
                    job.kill()
            shutil.rmtree(objdir, ignore_errors=True)
        return HIP_LIB
    finally:
        lock.close()


def build_emulator(force=False, verbose=False):
    if not force and not _stale(EMU_LIB, EMU_DEPS):
        return EMU_LIB
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("no host C++ compiler for the emulator")
    lock = _locked("emulate")
    try:
        if not force and not _stale(EMU_LIB, EMU_DEPS):      # built by another process while this one waited
            return EMU_LIB
        tmp = EMU_LIB + ".tmp.%d" % os.getpid()
        cmd = [cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-msse4.1", "-fPIC", "-shared",
               "-Wno-unknown-pragmas", "-I" + CSRC] + _abs(EMU_SOURCES) + ["-o", tmp]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        _publish(tmp, EMU_LIB, EMU_DEPS)
        return EMU_LIB
    finally:
        lock.close()


HOST = os.path.join(HERE, "host")
LAYERS_LIB = os.path.join(HERE, "libredsec_layers.so")
LAYERS_SOURCES = [os.path.join(HOST, "tfhe_shim.cpp"), os.path.join(HOST, "layers.cpp")]
LAYERS_DEPS = LAYERS_SOURCES + [os.path.join(HOST, "tfhe", f) for f in ("tfhe.h", "tfhe_io.h", "tfhe_garbage_collector.h")] + \
    [os.path.join(HOST, "lib", f) for f in ("Layer.h", "BinLayer.h", "IntLayer.h", "BinOps_enc.h", "IntOps_enc.h", "BinFunc.h", "IntFunc.h")] + \
    [os.path.join(INCLUDE, "redsec_hip.h"), os.path.join(CSRC, "rs_keygen.h"), os.path.join(CSRC, "rs_ntt.h")]


def build_layers(force=False, verbose=False):
    """C++ host mirror of the reference's layer API + the TFHE-compatible shim (links only the C ABI)."""
    build_hip(force, verbose)
    if not force and not _stale(LAYERS_LIB, LAYERS_DEPS):
        return LAYERS_LIB
    cxx = shutil.which("g++") or shutil.which("c++")
    lock = _locked("layers")
    try:
        if not force and not _stale(LAYERS_LIB, LAYERS_DEPS):
            return LAYERS_LIB
        tmp = LAYERS_LIB + ".tmp.%d" % os.getpid()
        cmd = [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-result", "-Wno-unknown-pragmas", "-I" + HOST, "-I" + INCLUDE, "-I" + CSRC] + LAYERS_SOURCES + \
              ["-L" + HERE, "-lredsec_hip", "-Wl,-rpath,$ORIGIN", "-o", tmp]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        _publish(tmp, LAYERS_LIB, LAYERS_DEPS)
        return LAYERS_LIB
    finally:
        lock.close()


def build_all(force=False, verbose=False):
    return build_hip(force, verbose), build_emulator(force, verbose), build_layers(force, verbose)


if __name__ == "__main__":
    import sys
    print(build_all(force="--force" in sys.argv, verbose=True))
