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

# THE recipe of the product library: what every object is compiled with, then (object name, source under csrc/, extra flags).
# build_tree() below and, through it, tools/build_variant.sh and the ISA tools (--print-flags) read it from here.
HIP_COMMON_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC"]
HIP_OBJECTS = [
    # the FFT / exact-NTT blind-rotation kernels and the split duo form, with LLVM's post-register-allocation scheduler off: its
    # in-block reordering of the hand-laid-out LDS / FP64 sequences costs these kernels 1-3 % (same-box A/B,
    # profiles/r03/y_ab_compiler_scheduling_*.txt: default-128 +1.3 %, REDsec set +0.9 %, sign1024x1 image 12.36 -> 12.11 ms)
    ("rs_bootstrap", "rs_bootstrap.hip", ["-mllvm", "-enable-post-misched=0"]),
    # the split cooperative and split lock-step kernels keep that pass (they lose 6 % / 0.7 % without it) and are scheduled with
    # the max-memory-clause strategy: the cooperative kernel streams the key from L2 by itself and gains 6.5 % from clustered
    # loads (196-neuron layer 4.33 -> 4.05 ms, split-mode sign1024x1 16.3 -> 15.95 ms; the lock-step kernel -0.5 % / +0.3 %)
    ("rs_bootstrap_split", "rs_bootstrap_split.hip", ["-mllvm", "-amdgpu-sched-strategy=max-memory-clause"]),
    # blind_rotate_coop8_listed_kernel (round 6) with the flags of rs_bootstrap, in an object of its own: instantiated beside those
    # kernels it changed the instructions of 15 of them (tools/codeobj_digest.py), the measured BASELINE-config forms among them
    ("rs_bootstrap_listed", "rs_bootstrap_listed.hip", ["-mllvm", "-enable-post-misched=0"]),
    # the other files use the default pipeline (the (9, 3) keyswitch in rs_kernels.hip loses 12 % without the post-RA pass)
    ("rs_general", "rs_general.hip", []),
    ("rs_kernels", "rs_kernels.hip", []),
    # the wide throughput keyswitch (keyswitch_wide_kernel, round 16) in an object of its own: the kernels of rs_kernels keep their
    # instructions. Default pipeline, as rs_kernels
    ("rs_keyswitch_wide", "rs_keyswitch_wide.hip", []),
    # seeded ciphertexts (seeded_lwe_kernel) in an object of their own: every kernel of rs_general keeps its instructions
    ("rs_seeded", "rs_seeded.hip", []),
    # public-key encryption (pk_encrypt_kernel), likewise in an object of its own: no earlier kernel changes an instruction
    ("rs_pubkey", "rs_pubkey.hip", []),
    # compact RLWE public keys (rlwe_pk_encrypt_kernel, rlwe_extract_kernel), likewise in an object of their own
    ("rs_rlwe", "rs_rlwe.hip", []),
    # packed results (pack_init_kernel, pack_kernel), likewise in an object of their own
    ("rs_pack", "rs_pack.hip", []),
    # re-keying (rekey_init_kernel, rekey_kernel), likewise in an object of their own; integer-only sources, as rs_pack
    ("rs_rekey", "rs_rekey.hip", []),
    # ring re-keying (ring_rekey_init_kernel, ring_rekey_kernel), likewise in an object of their own; integer-only sources, as rs_pack
    ("rs_ring_rekey", "rs_ring_rekey.hip", []),
    # encrypted selection (ring_cmux_init_kernel, ring_cmux_kernel), likewise in an object of their own; integer-only sources, as rs_pack
    ("rs_ring_cmux", "rs_ring_cmux.hip", []),
    # the alternating form of the CMUX (ring_cmux_alt_kernel), likewise in an object of its own: ring_cmux_kernel keeps its instructions
    ("rs_ring_cmux_alt", "rs_ring_cmux_alt.hip", []),
    # encrypted rotation (ring_rotate_init_kernel, ring_rotate_kernel, ring_rotate_alt_kernel, ring_heads_kernel), likewise in an
    # object of its own: the CMUX kernels keep their instructions; integer-only sources, as rs_pack
    ("rs_ring_rotate", "rs_ring_rotate.hip", []),
    # batched encrypted lookup (ring_lookup_init_kernel, ring_lookup_level_kernel, ring_lookup_level_alt_kernel), likewise in an
    # object of its own: the CMUX and rotation kernels keep their instructions; integer-only sources, as rs_pack
    ("rs_ring_lookup", "rs_ring_lookup.hip", []),
    # the selector keyswitch of circuit bootstrapping (ring_selector_init_kernel, ring_selector_kernel, circuit_prepare_kernel),
    # likewise in an object of its own; integer-only sources, as rs_pack
    ("rs_ring_selector", "rs_ring_selector.hip", []),
    # its wide form for batches of thousands of rows (ring_selector_wide_kernel), likewise in an object of its own:
    # ring_selector_kernel keeps its instructions
    ("rs_ring_selector_wide", "rs_ring_selector_wide.hip", []),
    # the packing key on the device (pack_keygen_kernel, pack_expand_kernel), likewise; not in rs_pack: its sources stay integer-only
    ("rs_packkey", "rs_packkey.hip", []),
    # device decryption and the key audit (lwe_phase_kernel, audit_bk_kernel, audit_ksk_kernel), likewise in an object of their own
    ("rs_audit", "rs_audit.hip", []),
    # the pre-pass of the indexed gate batches (gate_rows_kernel), likewise in an object of its own
    ("rs_rows", "rs_rows.hip", []),
    # the pre-pass and the MUX fold of the compiled circuits (circuit_rows_kernel, circuit_fold_kernel), likewise
    ("rs_circuit", "rs_circuit.hip", []),
    # the gather, the trivial fill and the scatter of the sparse bootstraps (sparse_*_kernel), likewise
    ("rs_sparse", "rs_sparse.hip", []),
    # the C ABI, host code only, in three units that share rs_api_internal.h: context and the bootstrapped path; the evaluation
    # key (load, generate, expand); key material and client-side calls
    ("rs_api", "rs_api.cpp", []),
    ("rs_api_keys", "rs_api_keys.cpp", []),
    ("rs_api_client", "rs_api_client.cpp", []),
]
HIP_SOURCES = [src for _, src, _ in HIP_OBJECTS]
HIP_DEPS = HIP_SOURCES + ["rs_bootstrap.h", "rs_kernels.h", "rs_cohort.h", "rs_diag.h", "rs_launch_plan.h", "rs_lds_plan.h", "rs_ntt.h", "rs_fft.h", "rs_general.h", "rs_keygen.h", "rs_rlwe.h", "rs_ring_sweep.h", "rs_pack.h", "rs_rekey.h", "rs_ring_rekey.h", "rs_ring_cmux.h", "rs_ring_rotate.h", "rs_ring_lookup.h", "rs_ring_selector.h", "rs_packkey.h", "rs_audit.h", "rs_rows.h", "rs_circuit.h", "rs_sparse.h", "rs_host.h", "rs_api_internal.h", os.path.join(INCLUDE, "redsec_hip.h")]
EMU_SOURCES = ["rs_emulate.cpp"]
EMU_DEPS = EMU_SOURCES + ["rs_launch_plan.h", "rs_lds_plan.h", "rs_ntt.h", "rs_fft.h", "rs_general.h", "rs_keygen.h", "rs_rlwe.h", "rs_ring_sweep.h", "rs_pack.h", "rs_rekey.h", "rs_ring_rekey.h", "rs_ring_cmux.h", "rs_ring_rotate.h", "rs_ring_lookup.h", "rs_ring_selector.h", "rs_packkey.h", "rs_audit.h", "rs_rows.h", "rs_circuit.h", "rs_sparse.h", "rs_host.h"]


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


def _recipe(src_root):
    """(common flags, HIP_OBJECTS) of the tree at `src_root`: this module's own for this tree, else read from THAT tree's
    redsec_amd/build.py, so that a checkout of another commit is built the way that commit builds itself."""
    path = os.path.join(src_root, "redsec_amd", "build.py")
    if os.path.realpath(path) == os.path.realpath(__file__):
        return HIP_COMMON_FLAGS, HIP_OBJECTS
    import importlib.util
    spec = importlib.util.spec_from_file_location("_redsec_build_recipe", path)
    other = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(other)
    return getattr(other, "HIP_COMMON_FLAGS", HIP_COMMON_FLAGS), other.HIP_OBJECTS   # older trees: the same flags, inside build_hip


def object_flags(name, src_root=ROOT):
    """The whole flag list one object of the recipe is compiled with (no input or output file)."""
    common, objects = _recipe(src_root)
    for obj, _, extra in objects:
        if obj == name:
            return common + ["-I" + os.path.join(src_root, "include"), "-I" + os.path.join(src_root, "redsec_amd", "csrc")] + extra
    raise KeyError("no object %r in HIP_OBJECTS (%s)" % (name, ", ".join(o[0] for o in objects)))


def build_tree(src_root, out, extra=(), per_object=None, verbose=False):
    """Compile the HIP_OBJECTS of the tree at `src_root` by that tree's recipe and link them into `out`: one object per entry
    (compiled side by side: the files carry different code-generation flags), then one link. `extra`: flags added to every
    object; `per_object`: {object name: flags added to that object only} (A/B builds). Objects are written under a per-process
    directory, so builds may run side by side."""
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    per_object = per_object or {}
    _, objects = _recipe(src_root)
    unknown = set(per_object) - {o[0] for o in objects}
    if unknown:
        raise KeyError("no object %s in HIP_OBJECTS (%s)" % (sorted(unknown), ", ".join(o[0] for o in objects)))
    objdir = os.path.join(ROOT, "build", "obj.%d" % os.getpid())
    os.makedirs(objdir, exist_ok=True)
    jobs, objs = [], []
    try:
        for name, src, _ in objects:
            obj = os.path.join(objdir, name + ".o")
            cmd = [hipcc] + object_flags(name, src_root) + list(per_object.get(name, ())) + list(extra) + \
                  ["-c", os.path.join(src_root, "redsec_amd", "csrc", src), "-o", obj]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd)))
            objs.append(obj)
        for cmd, job in jobs:
            if job.wait() != 0:
                raise subprocess.CalledProcessError(job.returncode, cmd)
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    finally:
        for _, job in jobs:
            if job.poll() is None:
                job.kill()
        shutil.rmtree(objdir, ignore_errors=True)
    return out


def build_hip(force=False, verbose=False):
    if not force and not _stale(HIP_LIB, HIP_DEPS):
        return HIP_LIB
    if find_hipcc() is None:
        if os.path.exists(HIP_LIB):
            return HIP_LIB  # prebuilt library shipped with the snapshot
        raise RuntimeError("hipcc not found and no prebuilt libredsec_hip.so present")
    lock = _locked("hip")
    try:
        if not force and not _stale(HIP_LIB, HIP_DEPS):     # another process built it while this one waited for the lock
            return HIP_LIB
        tmp = HIP_LIB + ".tmp.%d" % os.getpid()             # linked under a per-process name and renamed into place
        build_tree(ROOT, tmp, verbose=verbose)
        _publish(tmp, HIP_LIB, HIP_DEPS)
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


def main(argv):
    """python -m redsec_amd.build [--force]                 build everything in this tree
       python -m redsec_amd.build --print-flags OBJECT      the flags one object of HIP_OBJECTS is compiled with (ISA tools)
       python -m redsec_amd.build --variant NAME [--src ROOT] [--out PATH] [--object-flags OBJECT="FLAGS"]... [-- FLAGS...]
           libredsec_hip.so of the tree at ROOT (default: this one), by THAT tree's recipe, into PATH (default:
           variants/lib_NAME.so) for same-box A/B runs with REDSEC_HIP_LIB; FLAGS go to every object, --object-flags to one."""
    import argparse
    import shlex
    extra = []
    if "--" in argv:
        k = argv.index("--")
        argv, extra = argv[:k], argv[k + 1:]
    ap = argparse.ArgumentParser(prog="python -m redsec_amd.build", description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--print-flags", metavar="OBJECT")
    ap.add_argument("--variant", metavar="NAME")
    ap.add_argument("--src", default=ROOT)
    ap.add_argument("--out")
    ap.add_argument("--object-flags", action="append", default=[], metavar="OBJECT=FLAGS")
    a = ap.parse_args(argv)
    src = os.path.abspath(a.src)
    if a.print_flags:
        print(" ".join(object_flags(a.print_flags, src)))
    elif a.variant:
        out = os.path.abspath(a.out or os.path.join(ROOT, "variants", "lib_%s.so" % a.variant))
        os.makedirs(os.path.dirname(out), exist_ok=True)
        per_object = {}
        for item in a.object_flags:
            name, _, flags = item.partition("=")
            per_object.setdefault(name, []).extend(shlex.split(flags))
        print(build_tree(src, out, extra, per_object, verbose=True))
    else:
        print(build_all(force=a.force, verbose=True))


if __name__ == "__main__":
    import sys
    main(sys.argv[1:])
