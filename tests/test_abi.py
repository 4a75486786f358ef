"""The C-ABI library loads on a CPU-only machine, exports every symbol include/redsec_hip.h
declares, and refuses to compute without a GPU (no CPU fallback in the product path)."""
import ctypes
import os
import re

import pytest

import redsec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported():
    L = redsec_amd.load_library()
    declared = _declared_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(L, name), "libredsec_hip.so does not export " + name
    assert sorted(redsec_amd.ABI_SYMBOLS) == declared


def test_parameter_sets():
    d = redsec_amd.params("default128")
    assert (d.n, d.N, d.k, d.bk_l, d.bk_Bgbit, d.ks_t, d.ks_basebit) == (630, 1024, 1, 3, 7, 8, 2)
    r = redsec_amd.params("redsec_small_v2")  # client/gen_secure_keyset.cpp:70-91
    assert (r.n, r.N, r.k, r.bk_l, r.bk_Bgbit, r.ks_t, r.ks_basebit) == (350, 1024, 1, 10, 3, 9, 3)


def test_rejects_unsupported_parameters():
    L = redsec_amd.load_library()
    h = ctypes.c_void_p()
    for field, value, why in (("N", 512, b"unsupported ring"), ("N", 3072, b"unsupported ring"), ("N", 16384, b"unsupported ring"),
                              ("k", 2, b"unsupported ring"), ("bk_l", 5, b"bad gadget"), ("ks_t", 16, b"bad keyswitch")):
        p = redsec_amd.params("default128")
        setattr(p, field, value)          # l * Bgbit = 35 > 32; t * basebit = 32 > 31
        assert L.rs_create(ctypes.byref(h), ctypes.byref(p), 0) == -1, field
        assert why in L.rs_last_error(), L.rs_last_error()


def test_reference_parameter_sets_beside_the_shipped_one():
    """client/gen_secure_keyset.cpp:9-68."""
    for name, want in (("redsec_small", (500, 1024, 1, 3, 10, 18, 1)), ("redsec_medium", (3072, 4096, 1, 3, 10, 18, 1)),
                       ("redsec_large", (6144, 8192, 1, 3, 10, 18, 1))):
        r = redsec_amd.params(name)
        assert (r.n, r.N, r.k, r.bk_l, r.bk_Bgbit, r.ks_t, r.ks_basebit) == want


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(redsec_amd.RedsecHipError, match="no HIP device"):
        redsec_amd.Backend(redsec_amd.params("default128"))


def test_product_does_not_reference_oracle():
    """The product package must not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "redsec_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "redsec_oracle" not in src and "oracle_lib" not in src, f


def test_header_is_plain_c99_and_a_c_program_links(tmp_path):
    """The drop-in boundary is a C ABI: include/redsec_hip.h must compile under a C compiler (no C++ in the
    signatures) and a C program must link against libredsec_hip.so. Without a GPU rs_create has to fail with a
    message, never compute."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "cabi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "redsec_hip.h"\n'
        "int main(void) {\n"
        "  rs_params p; rs_ctx* c = NULL;\n"
        "  if (rs_params_default128(&p) != 0 || p.N != 1024 || p.n != 630) return 2;\n"
        "  if (rs_params_redsec_small_v2(&p) != 0 || p.n != 350) return 3;\n"
        "  if (!rs_version() || strlen(rs_version()) == 0) return 4;\n"
        "  if (rs_create(&c, &p, 0) == 0) { puts(\"created\"); rs_destroy(c); return 0; }\n"
        "  printf(\"refused: %s\\n\", rs_last_error());\n"
        "  return 0;\n}\n")
    lib_dir = os.path.join(ROOT, "redsec_amd")
    exe = tmp_path / "cabi"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", lib_dir, "-lredsec_hip", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    import torch
    if not torch.cuda.is_available():
        assert "refused: " in r.stdout and "no HIP device" in r.stdout, r.stdout


def test_kernel_form_names_of_the_binding_follow_the_library_enum():
    """rs_last_launch reports a form id (csrc/rs_launch_plan.h kForm*); backend.Backend.last_launch names it. A form added on one side only
    would index past the list or mislabel a launch."""
    import re
    text = open(os.path.join(ROOT, "redsec_amd", "csrc", "rs_launch_plan.h")).read()
    enum = re.search(r"enum \{ (kFormPerWave = 0[^}]*)\}", text).group(1)
    ids = {name: int(v) for name, v in re.findall(r"(kForm\w+) = (\d+)", enum)}
    assert sorted(ids.values()) == list(range(len(ids)))
    src = open(os.path.join(ROOT, "redsec_amd", "backend.py")).read()
    names = re.search(r'return \{"form": \[([^\]]*)\]\[f\.value\]', src).group(1)
    names = [n.strip().strip('"') for n in names.split(",")]
    assert len(names) == len(ids)
    norm = lambda s: s.replace("_", "").lower()
    for name, v in ids.items():
        assert norm(name[len("kForm"):]) == norm(names[v]), (name, v, names[v])
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    doc = header[header.index("rs_last_launch: what the last blind rotation"):header.index("int rs_last_launch(")]
    for v in ids.values():
        assert re.search(r"\b%d\b" % v, doc), "form id %d is not described in include/redsec_hip.h" % v


def test_kernel_sources_carry_no_experiment_switches():
    """Round 5 deleted the ~70 compile-time experiment switches of rounds 1-4 (RS_T_*, RS_WG_*, RS_GEN_* ...: each measured, none adopted,
    verdicts in MEASUREMENTS.md) together with their code paths. What may still select code in csrc/: RS_DIAG (rs_diag.h: phase stamps
    and the no-key timing probe of diagnostic builds, the ONE guard for everything diagnostic) -- which launchers and kernels an object
    holds is decided by its translation unit (rs_bootstrap.hip, rs_bootstrap_split.hip, rs_bootstrap_listed.hip), not by a switch. This
    test keeps it that way."""
    import glob
    import re
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    allowed = {"RS_DIAG", "RS_STAMPS_ON", "RS_HD"}     # the last two: helper macros, not switches
    seen, conditionals = set(), 0
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        text = open(path).read()
        name = os.path.basename(path)
        if name != "rs_diag.h":
            assert not re.search(r"\bRS_T_[A-Z0-9_]+\b", text), "timing-probe switch outside rs_diag.h: " + name
        for line in text.splitlines():
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                conditionals += 1
                seen |= set(re.findall(r"\bRS_[A-Z0-9_]+\b", line))
            m = re.match(r"\s*#\s*ifndef\s+(RS_[A-Z0-9_]+)", line)     # the `#ifndef X / #define X default` idiom of an A/B switch
            assert not (m and m.group(1) not in allowed), "overridable default in %s: %s" % (name, line.strip())
            code = line.split("//")[0]
            # what a textual macro replacement leaves behind: branches on a literal, `0=1` in prose
            assert not re.search(r"\bif\s*\(\s*[01!]\s*(\)|&&|\|\|)|\b(&&|\|\|)\s*[01]\s*\)", code), "constant condition in %s: %s" % (name, line.strip())
            assert not re.search(r"\b[01]=[01]\b", line), "garbled switch text in %s: %s" % (name, line.strip())
    assert seen <= allowed, sorted(seen - allowed)
    assert conditionals <= 24, conditionals                          # 24 today: __HIP_DEVICE_COMPILE__ / __HIPCC__ and rs_diag.h; may go down, never up


@pytest.mark.parametrize("src,flags", [
    ("rs_bootstrap.hip", ["-DRS_DIAG=253"]),                       # stamps of its three stamped kernels + every timing probe
    ("rs_bootstrap_split.hip", ["-DRS_DIAG=2"]),                   # stamps of the split lock-step kernel: the array lives in its unit
    ("rs_bootstrap.hip", ["-DRS_DIAG=2"]),                         # ... and rs_bootstrap.hip of that build has no stamped kernel and no array
    ("rs_bootstrap_listed.hip", ["-DRS_DIAG=256"]),                # stamps of the listed coop8 kernel: the array lives in its unit
    ("rs_general.hip", ["-DRS_DIAG=144"]),                         # no-key and half-key probes of the general rings
    ("rs_api.cpp", ["-DRS_DIAG=48"]),                              # the probes' switch that turns the exactness gates off
    ("rs_api_keys.cpp", ["-DRS_DIAG=48"]),                         # ... and the other two units of the C ABI: neither reads rs::diag
    ("rs_api_client.cpp", ["-DRS_DIAG=48"]),                       #     today, and the diagnostic build still has to hold all three
])
def test_diagnostic_builds_compile(src, flags):
    """Everything diagnostic sits behind -DRS_DIAG=<bits> (csrc/rs_diag.h) and no product build defines it: nothing but this test would
    notice those paths rotting. Front end only (hipcc -fsyntax-only instantiates every kernel the launchers name): seconds."""
    r = _syntax_only(src, flags)
    assert r.returncode == 0, r.stderr[-3000:]


def _syntax_only(src, flags):
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "redsec_amd", "csrc")
    return subprocess.run([hipcc, "-fsyntax-only", "--offload-arch=gfx950", "-std=c++17", "-Wno-unused-command-line-argument",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + (["-x", "hip"] if src.endswith(".cpp") else []) + flags + [os.path.join(csrc, src)],
                          capture_output=True, text=True, timeout=300)


def test_stamp_bits_of_two_units_in_one_build_are_refused():
    """The stamp array lives in the unit of the stamped kernel and the build has no relocatable device code: -DRS_DIAG=264 (bit 8:
    rs_bootstrap.hip, bit 256: rs_bootstrap_listed.hip) would leave one unit referencing an undefined device symbol. rs_diag.h refuses
    it with an #error."""
    r = _syntax_only("rs_bootstrap.hip", ["-DRS_DIAG=264"])
    assert r.returncode != 0 and "stamp bits of one unit per build" in r.stderr, r.stderr[-3000:]


def test_a_variant_build_of_this_tree_loads_and_exports_the_abi(tmp_path):
    """tools/build_variant.sh (same-box A/B libraries, the stamped builds of tools/stamp_*.py) goes through the recipe of
    redsec_amd/build.py (python -m redsec_amd.build --variant): the library it links must load and resolve every ABI symbol, i.e.
    hold every object of the product library."""
    import shutil
    import subprocess
    import sys
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    out = tmp_path / "lib_variant_test.so"
    r = subprocess.run([sys.executable, "-m", "redsec_amd.build", "--variant", "variant_test", "--src", ROOT, "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = ctypes.CDLL(str(out))
    for name in redsec_amd.ABI_SYMBOLS:
        assert hasattr(lib, name), "the variant library does not export " + name
