"""ctypes binding of libredsec_hip.so (the C ABI in include/redsec_hip.h).

PyTorch is used only as plumbing: device buffers are int32 CUDA (HIP) tensors and launches go on
torch's current stream. All arithmetic happens in the HIP kernels; there is no CPU or eager
fallback -- if the library or a gfx950 device is missing, calls raise RedsecHipError.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)

# every symbol include/redsec_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "rs_last_error", "rs_version", "rs_params_default128", "rs_params_redsec_small_v2", "rs_create", "rs_destroy",
    "rs_load_keys", "rs_reserve", "rs_bootstrap_dev", "rs_bootstrap", "rs_gate_dev", "rs_gate", "rs_mux_dev", "rs_mux",
    "rs_gate_mu_dev", "rs_gather_rows_dev", "rs_bootstrap_wo_ks_dev", "rs_keyswitch_dev", "rs_debug_polymul", "rs_debug_cohort_table", "rs_debug_fp64_rate", "rs_linear_fc_dev", "rs_conv_ternary_dev",
    "rs_sumpool_dev", "rs_lincomb_dev", "rs_dev_alloc", "rs_dev_free", "rs_copy_to_dev", "rs_copy_to_host", "rs_sync",
    "rs_set_timing", "rs_last_kernel_ms", "rs_info", "rs_set_mode", "rs_get_mode", "rs_rounding_certificate", "rs_fft_fallbacks",
    "rs_bootstrap_lut_dev", "rs_set_certificate_limit", "rs_certify", "rs_reserve_stream", "rs_last_kernel_ms_stream", "rs_last_launch", "rs_last_keyswitch", "rs_copy_dev_to_dev",
    "rs_params_redsec_small", "rs_params_redsec_medium", "rs_params_redsec_large", "rs_split_bound",
    "rs_allgather_rows", "rs_release_stream", "rs_load_synthetic_keys", "rs_keygen_dev", "rs_load_keys_dev",
    "rs_keygen_compressed_dev", "rs_expand_keys_dev", "rs_load_compressed_keys", "rs_load_compressed_keys_dev",
    "rs_encrypt_seeded_dev", "rs_expand_ciphertexts_dev", "rs_pk_encrypt_dev", "rs_rlwe_pk_encrypt_dev", "rs_rlwe_extract_dev", "rs_pack_dev",
    "rs_pack_keygen_dev", "rs_pack_expand_dev", "rs_audit_pack_key_dev",
    "rs_phase_dev", "rs_audit_keys_dev", "rs_audit_compressed_keys_dev",
    "rs_gate3_dev", "rs_gate_rows_dev",
    "rs_circuit_create", "rs_circuit_destroy", "rs_circuit_run_dev",
    "rs_bootstrap_sparse_dev",
    "rs_rekey_dev",
    "rs_ring_rekey_dev",
    "rs_ring_cmux_dev", "rs_ring_lookup_dev", "rs_ring_cmux_alt_dev", "rs_ring_lookup_alt_dev",
    "rs_ring_selector_dev", "rs_circuit_bootstrap_dev",
    "rs_ring_rotate_dev", "rs_ring_rotate_alt_dev", "rs_ring_heads_dev",
    "rs_ring_lookup_rows_dev", "rs_ring_lookup_rows_alt_dev",
    "rs_ring_selector_batch_dev", "rs_circuit_bootstrap_batch_dev", "rs_last_selector",
]

GATES = {"NAND": 0, "OR": 1, "AND": 2, "NOR": 3, "XOR": 4, "XNOR": 5, "ANDNY": 6, "ANDYN": 7, "ORNY": 8, "ORYN": 9}

# rs_row_op (include/redsec_hip.h): the two-input gates with their rs_gate_op values, then the three-input ones
ROW_OPS = dict(GATES, MAJ3=10, XOR3=11, MAJ3N=12)

# ops of a circuit cell (rs_cell_op): the row ops with their values, then MUX
CELL_OPS = dict(ROW_OPS, MUX=13)


class RedsecHipError(RuntimeError):
    pass


class RsParams(C.Structure):
    _fields_ = [("n", C.c_int32), ("N", C.c_int32), ("k", C.c_int32), ("bk_l", C.c_int32), ("bk_Bgbit", C.c_int32),
                ("ks_t", C.c_int32), ("ks_basebit", C.c_int32)]


class RsConvShape(C.Structure):
    _fields_ = [(f, C.c_int32) for f in
                ("H", "Wd", "Cin", "Cout", "fh", "fw", "stride_h", "stride_w", "off_h", "off_w", "Ho", "Wo")]


class RsPoolShape(C.Structure):
    _fields_ = [(f, C.c_int32) for f in
                ("H", "Wd", "C", "win_h", "win_w", "stride_h", "stride_w", "off_h", "off_w", "Ho", "Wo")]


class RsKeyAudit(C.Structure):
    _fields_ = [("bk_max_abs", C.c_uint32), ("ksk_max_abs", C.c_uint32), ("bk_over", C.c_uint64), ("ksk_over", C.c_uint64),
                ("ksk_zero_bad", C.c_uint64), ("bk_words", C.c_uint64), ("ksk_words", C.c_uint64)]


class RsPackKeyAudit(C.Structure):
    _fields_ = [("max_abs", C.c_uint32), ("over", C.c_uint64), ("words", C.c_uint64)]


class RsRowGroup(C.Structure):
    _fields_ = [("op", C.c_int32), ("reserved", C.c_int32), ("count", C.c_uint64)]


class RsCell(C.Structure):
    _fields_ = [("src", C.c_int32 * 3), ("op", C.c_uint8), ("neg", C.c_uint8), ("reserved", C.c_uint16)]


# numpy view of an rs_cell table (circuit.Plan.table)
CELL_DTYPE = np.dtype([("src", np.int32, (3,)), ("op", np.uint8), ("neg", np.uint8), ("reserved", np.uint16)])

_lib = None


def load_library(path=None):
    """dlopen libredsec_hip.so (building it in-tree first if the sources are newer)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("REDSEC_HIP_LIB")   # timing experiments may point at a variant build
    so = path or _build.build_hip()
    # torch's HIP runtime must be initialised BEFORE this library's code object registers with its own copy of the runtime in the
    # same process: the other order leaves one of the two without devices ("No HIP GPUs are available" / RS_ERR_NO_DEVICE;
    # measured on the MI355X boxes, ROCm 7.2 + torch 2.10). Loading is the first thing every user of the package does.
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    if not os.path.exists(so):
        raise RedsecHipError("libredsec_hip.so is missing: run `python -m redsec_amd.build`")
    try:
        L = C.CDLL(so)
    except OSError as e:  # pragma: no cover
        raise RedsecHipError("cannot load %s: %s" % (so, e))
    L.rs_last_error.restype = C.c_char_p
    L.rs_version.restype = C.c_char_p
    P = C.POINTER(RsParams)
    vp = C.c_void_p
    L.rs_params_default128.argtypes = [P]
    L.rs_params_redsec_small_v2.argtypes = [P]
    L.rs_params_redsec_small.argtypes = [P]
    L.rs_params_redsec_medium.argtypes = [P]
    L.rs_params_redsec_large.argtypes = [P]
    L.rs_split_bound.argtypes = [vp, C.POINTER(C.c_double)]
    L.rs_create.argtypes = [C.POINTER(vp), P, C.c_int]
    L.rs_destroy.argtypes = [vp]
    L.rs_load_keys.argtypes = [vp, _i32p, _i32p]
    L.rs_load_synthetic_keys.argtypes = [vp, C.c_uint64]
    L.rs_load_keys_dev.argtypes = [vp, vp, vp]
    L.rs_keygen_dev.argtypes = [vp, vp, vp, _i32p, _i32p, C.c_char_p, C.c_double, C.c_double]
    L.rs_keygen_compressed_dev.argtypes = [vp, vp, vp, _i32p, _i32p, C.c_char_p, C.c_char_p, C.c_double, C.c_double]
    L.rs_expand_keys_dev.argtypes = [vp, vp, vp, C.c_char_p, vp, vp]
    L.rs_load_compressed_keys.argtypes = [vp, C.c_char_p, _i32p, _i32p]
    L.rs_load_compressed_keys_dev.argtypes = [vp, C.c_char_p, vp, vp]
    L.rs_encrypt_seeded_dev.argtypes = [vp, vp, vp, vp, C.c_size_t, _i32p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_double]
    L.rs_expand_ciphertexts_dev.argtypes = [vp, vp, C.c_char_p, C.c_uint64, vp, C.c_size_t, vp]
    L.rs_pk_encrypt_dev.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_char_p, C.c_uint64, vp]
    L.rs_rlwe_pk_encrypt_dev.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_char_p, C.c_uint64, C.c_double, vp]
    L.rs_rlwe_extract_dev.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.rs_pack_dev.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_int32, C.c_int32, vp]
    L.rs_rekey_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, vp]
    L.rs_ring_rekey_dev.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_int32, C.c_int32, vp]
    L.rs_ring_cmux_dev.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_int32, C.c_int32, vp]
    L.rs_ring_lookup_dev.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    L.rs_ring_cmux_alt_dev.argtypes = L.rs_ring_cmux_dev.argtypes
    L.rs_ring_lookup_alt_dev.argtypes = L.rs_ring_lookup_dev.argtypes
    L.rs_ring_rotate_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    L.rs_ring_rotate_alt_dev.argtypes = L.rs_ring_rotate_dev.argtypes
    L.rs_ring_heads_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    L.rs_ring_lookup_rows_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    L.rs_ring_lookup_rows_alt_dev.argtypes = L.rs_ring_lookup_rows_dev.argtypes
    L.rs_ring_selector_dev.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp]
    L.rs_circuit_bootstrap_dev.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp]
    L.rs_ring_selector_batch_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp]
    L.rs_circuit_bootstrap_batch_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp]
    L.rs_last_selector.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.rs_pack_keygen_dev.argtypes = [vp, vp, _i32p, _i32p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_double]
    L.rs_pack_expand_dev.argtypes = [vp, vp, C.c_char_p, vp, C.c_int32, vp]
    L.rs_audit_pack_key_dev.argtypes = [vp, C.POINTER(RsPackKeyAudit), vp, vp, C.c_char_p, _i32p, _i32p, C.c_int32, C.c_int32, C.c_uint32]
    L.rs_phase_dev.argtypes = [vp, vp, vp, C.c_size_t, _i32p, C.c_int32]
    L.rs_audit_keys_dev.argtypes = [vp, C.POINTER(RsKeyAudit), vp, vp, vp, vp, _i32p, _i32p, C.c_uint32, C.c_uint32]
    L.rs_audit_compressed_keys_dev.argtypes = [vp, C.POINTER(RsKeyAudit), vp, vp, C.c_char_p, vp, vp, _i32p, _i32p, C.c_uint32, C.c_uint32]
    L.rs_reserve.argtypes = [vp, C.c_size_t]
    L.rs_bootstrap_dev.argtypes = [vp, vp, vp, C.c_int32, C.c_size_t, vp]
    L.rs_bootstrap.argtypes = [vp, _i32p, _i32p, C.c_int32, C.c_size_t]
    L.rs_bootstrap_sparse_dev.argtypes = [vp, vp, vp, C.c_int32, C.c_size_t, vp, C.c_size_t, vp]
    L.rs_gate_dev.argtypes = [vp, C.c_int, vp, vp, vp, C.c_size_t, vp]
    L.rs_gate.argtypes = [vp, C.c_int, _i32p, _i32p, _i32p, C.c_size_t]
    L.rs_gate_mu_dev.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int32, C.c_size_t, vp]
    L.rs_gather_rows_dev.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    L.rs_gate3_dev.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_size_t, vp]
    L.rs_gate_rows_dev.argtypes = [vp, vp, vp, C.c_size_t, vp, C.POINTER(RsRowGroup), C.c_int, C.c_int32, C.c_size_t, vp]
    L.rs_circuit_create.argtypes = [vp, C.POINTER(vp), vp, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t, C.c_size_t]
    L.rs_circuit_destroy.argtypes = [vp, vp]
    L.rs_circuit_run_dev.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.rs_mux_dev.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.rs_mux.argtypes = [vp, _i32p, _i32p, _i32p, _i32p, C.c_size_t]
    L.rs_bootstrap_wo_ks_dev.argtypes = [vp, vp, vp, C.c_int32, C.c_size_t, vp]
    L.rs_keyswitch_dev.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.rs_debug_polymul.argtypes = [vp, _i32p, _i32p, _i32p, C.c_size_t]
    L.rs_debug_cohort_table.argtypes = [vp, vp, _i32p]
    L.rs_debug_fp64_rate.argtypes = [vp, C.POINTER(C.c_double)]
    L.rs_linear_fc_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp]
    L.rs_conv_ternary_dev.argtypes = [vp, vp, vp, vp, vp, C.POINTER(RsConvShape), C.c_int32, C.c_int32, vp, C.c_int32, vp]
    L.rs_sumpool_dev.argtypes = [vp, vp, vp, C.POINTER(RsPoolShape), vp, C.c_int32, vp]
    L.rs_lincomb_dev.argtypes = [vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_size_t, vp]
    L.rs_dev_alloc.argtypes = [vp, C.POINTER(vp), C.c_size_t]
    L.rs_dev_free.argtypes = [vp, vp]
    L.rs_copy_to_dev.argtypes = [vp, vp, vp, C.c_size_t]
    L.rs_copy_to_host.argtypes = [vp, vp, vp, C.c_size_t]
    L.rs_sync.argtypes = [vp]
    L.rs_set_timing.argtypes = [vp, C.c_int]
    L.rs_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rs_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rs_set_mode.argtypes = [vp, C.c_int]
    L.rs_get_mode.argtypes = [vp, C.POINTER(C.c_int)]
    L.rs_rounding_certificate.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    L.rs_fft_fallbacks.argtypes = [vp, C.POINTER(C.c_int64)]
    L.rs_bootstrap_lut_dev.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp]
    L.rs_copy_dev_to_dev.argtypes = [vp, vp, vp, vp, C.c_size_t]
    L.rs_allgather_rows.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_size_t, C.c_size_t]
    L.rs_release_stream.argtypes = [vp, vp]
    L.rs_set_certificate_limit.argtypes = [vp, C.c_double]
    L.rs_certify.argtypes = [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    L.rs_reserve_stream.argtypes = [vp, C.c_size_t, vp]
    L.rs_last_kernel_ms_stream.argtypes = [vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rs_last_launch.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.rs_last_keyswitch.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if path is None:
        _lib = L
    return L


def _check(L, rc):
    if rc != 0:
        raise RedsecHipError("redsec_hip error %d: %s" % (rc, (L.rs_last_error() or b"").decode()))


def params(name, n=None):
    """'default128' | 'redsec_small_v2' | 'redsec_small' | 'redsec_medium' | 'redsec_large'; `n` overrides the LWE
    dimension (reduced-size test keys)."""
    L = load_library()
    p = RsParams()
    if name == "default128":
        _check(L, L.rs_params_default128(C.byref(p)))
    elif name == "redsec_small_v2":
        _check(L, L.rs_params_redsec_small_v2(C.byref(p)))
    elif name in ("redsec_small", "redsec_medium", "redsec_large"):
        _check(L, getattr(L, "rs_params_" + name)(C.byref(p)))
    else:
        raise KeyError(name)
    if n is not None:
        p.n = int(n)
    return p


def _refuse_overlap(name, out, words, others):
    """ValueError where the tensor `out` of a call (its first `words` words) shares memory with an input: others = (name, tensor or
    None, words read). What the ABI refuses with RS_ERR_INVALID (include/redsec_hip.h): these kernels add into out with atomics
    after an init kernel has set it, so an overlap is refused, never computed. Inputs may overlap each other."""
    lo, hi = out.data_ptr(), out.data_ptr() + 4 * words
    for other, t, read in others:
        if t is not None and words and read and t.data_ptr() < hi and lo < t.data_ptr() + 4 * read:
            raise ValueError("%s overlaps %s" % (name, other))


def _np_i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_i32p)


class Backend:
    """One context = one GPU + one evaluation key (mirrors TFheGateBootstrappingCloudKeySet usage,
    /root/reference/lib/BinOps_enc.cpp: every primitive takes `bk` as its last argument)."""

    def __init__(self, p, device=0):
        # torch's HIP runtime must be initialised BEFORE this library initialises its own in the same process: the
        # other order leaves torch with "No HIP GPUs are available" (measured on the MI355X boxes, ROCm 7.2 + torch 2.10)
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        self.L = load_library()
        self.p = p
        self.W = p.n + 1
        self.device = device
        h = C.c_void_p()
        _check(self.L, self.L.rs_create(C.byref(h), C.byref(p), device))
        self.h = h

    @property
    def closed(self):
        """True once rs_destroy has run: every other method would hand the library a null context."""
        return not getattr(self, "h", None)

    def close(self, check=None):
        """rs_destroy; raises if the enforced split-mode certificate of some stream's last call had failed (nothing else would
        look at it any more) -- unless another exception is already on its way out (a close() in a `finally:` block must not
        mask the error that brought the caller there) or check=False says the caller has dealt with the context's state. A
        failure that is not raised is never dropped: it is reported as a RuntimeWarning carrying rs_last_error()."""
        if getattr(self, "h", None):
            h, self.h = self.h, None
            rc = self.L.rs_destroy(h)
            if check is None:
                import sys
                check = sys.exc_info()[0] is None
            if check:
                _check(self.L, rc)
            elif rc != 0:
                import warnings
                warnings.warn("rs_destroy reported error %d while another error was being handled: %s"
                              % (rc, (self.L.rs_last_error() or b"").decode()), RuntimeWarning, stacklevel=2)

    def __del__(self):
        try:
            self.close(check=False)
        except Exception:
            pass

    # ---- keys ----
    def load_keys(self, bk, ksk):
        bk, pbk = _np_i32(bk)
        ksk, pksk = _np_i32(ksk)
        p = self.p
        assert bk.size == p.n * 2 * p.bk_l * 2 * p.N, "bk has the wrong size"
        assert ksk.size == p.N * p.ks_t * (1 << p.ks_basebit) * (p.n + 1), "ksk has the wrong size"
        _check(self.L, self.L.rs_load_keys(self.h, pbk, pksk))

    def _key_sizes(self):
        p = self.p
        return p.n * 2 * p.bk_l * 2 * p.N, p.N * p.ks_t * (1 << p.ks_basebit) * (p.n + 1)

    def load_keys_dev(self, bk, ksk):
        """rs_load_keys from int32 CUDA tensors on this context's device (device-to-device; the tensors are not modified)."""
        nb, nk = self._key_sizes()
        assert bk.numel() == nb, "bk has the wrong size"
        assert ksk.numel() == nk, "ksk has the wrong size"
        _check(self.L, self.L.rs_load_keys_dev(self.h, self._ck_dev(bk), self._ck_dev(ksk)))

    def keygen(self, lwe_key, tlwe_key, seed, bk_stdev, ks_stdev, bk=None, ksk=None):
        """Evaluation key generated on the device (rs_keygen_dev) -> (bk [n][2l][2][N], ksk [N][t][2^basebit][n+1]) int32 CUDA
        tensors (or into the given ones). lwe_key / tlwe_key: 0/1 arrays of length n / N; seed: 32 bytes. Does not load the key."""
        p = self.p
        lwe, plwe = _np_i32(lwe_key)
        tlwe, ptlwe = _np_i32(tlwe_key)
        assert lwe.size == p.n and tlwe.size == p.N, "secret keys have the wrong size"
        seed = bytes(seed)
        assert len(seed) == 32, "seed must be 32 bytes"
        bk = self.empty(p.n, 2 * p.bk_l, 2, p.N) if bk is None else bk
        ksk = self.empty(p.N, p.ks_t, 1 << p.ks_basebit, p.n + 1) if ksk is None else ksk
        nb, nk = self._key_sizes()
        assert bk.numel() == nb and ksk.numel() == nk, "key tensors have the wrong size"
        _check(self.L, self.L.rs_keygen_dev(self.h, self._ck_dev(bk), self._ck_dev(ksk), plwe, ptlwe, seed, float(bk_stdev), float(ks_stdev)))
        return bk, ksk

    def _body_sizes(self):
        p = self.p
        return p.n * 2 * p.bk_l * p.N, p.N * p.ks_t * (1 << p.ks_basebit)

    @staticmethod
    def _seed32(seed, what="seed"):
        seed = bytes(seed)
        assert len(seed) == 32, what + " must be 32 bytes"
        return seed

    def keygen_compressed(self, lwe_key, tlwe_key, mask_seed, noise_seed, bk_stdev, ks_stdev, bk_body=None, ksk_body=None):
        """Bodies of a compressed evaluation key generated on the device (rs_keygen_compressed_dev) -> (bk_body [n][2l][N],
        ksk_body [N][t][2^basebit]) int32 CUDA tensors (or into the given ones). The masks are those of mask_seed (public); the
        noise comes from noise_seed (private, must differ). Does not load the key."""
        p = self.p
        lwe, plwe = _np_i32(lwe_key)
        tlwe, ptlwe = _np_i32(tlwe_key)
        assert lwe.size == p.n and tlwe.size == p.N, "secret keys have the wrong size"
        mask_seed, noise_seed = self._seed32(mask_seed, "mask_seed"), self._seed32(noise_seed, "noise_seed")
        bk_body = self.empty(p.n, 2 * p.bk_l, p.N) if bk_body is None else bk_body
        ksk_body = self.empty(p.N, p.ks_t, 1 << p.ks_basebit) if ksk_body is None else ksk_body
        nb, nk = self._body_sizes()
        assert bk_body.numel() == nb and ksk_body.numel() == nk, "body tensors have the wrong size"
        _check(self.L, self.L.rs_keygen_compressed_dev(self.h, self._ck_dev(bk_body), self._ck_dev(ksk_body), plwe, ptlwe, mask_seed,
                                                       noise_seed, float(bk_stdev), float(ks_stdev)))
        return bk_body, ksk_body

    def expand_keys(self, mask_seed, bk_body, ksk_body, bk=None, ksk=None):
        """The full evaluation key of a compressed one, expanded on the device (rs_expand_keys_dev) -> (bk [n][2l][2][N],
        ksk [N][t][2^basebit][n+1]) int32 CUDA tensors (or into the given ones). Does not load the key."""
        p = self.p
        mask_seed = self._seed32(mask_seed, "mask_seed")
        nb, nk = self._body_sizes()
        assert bk_body.numel() == nb and ksk_body.numel() == nk, "body tensors have the wrong size"
        bk = self.empty(p.n, 2 * p.bk_l, 2, p.N) if bk is None else bk
        ksk = self.empty(p.N, p.ks_t, 1 << p.ks_basebit, p.n + 1) if ksk is None else ksk
        fb, fk = self._key_sizes()
        assert bk.numel() == fb and ksk.numel() == fk, "key tensors have the wrong size"
        _check(self.L, self.L.rs_expand_keys_dev(self.h, self._ck_dev(bk), self._ck_dev(ksk), mask_seed, self._ck_dev(bk_body),
                                                 self._ck_dev(ksk_body)))
        return bk, ksk

    def load_compressed_keys(self, mask_seed, bk_body, ksk_body):
        """Loads a compressed evaluation key, expanded on the device: numpy bodies go through rs_load_compressed_keys (host),
        CUDA tensors through rs_load_compressed_keys_dev. The full key never exists on the host."""
        mask_seed = self._seed32(mask_seed, "mask_seed")
        nb, nk = self._body_sizes()
        if isinstance(bk_body, np.ndarray) or isinstance(ksk_body, np.ndarray):
            bk_body, pbk = _np_i32(bk_body)
            ksk_body, pksk = _np_i32(ksk_body)
            assert bk_body.size == nb and ksk_body.size == nk, "bodies have the wrong size"
            _check(self.L, self.L.rs_load_compressed_keys(self.h, mask_seed, pbk, pksk))
        else:
            assert bk_body.numel() == nb and ksk_body.numel() == nk, "bodies have the wrong size"
            _check(self.L, self.L.rs_load_compressed_keys_dev(self.h, mask_seed, self._ck_dev(bk_body), self._ck_dev(ksk_body)))

    # ---- seeded ciphertexts ----
    def encrypt_seeded(self, lwe_key, mu, mask_seed, noise_seed, first=0, stdev=2.0 ** -15, full=False):
        """Seeded ciphertexts of the torus words mu (int32 CUDA tensor [B]) under lwe_key (host, 0/1) encrypted on the device
        (rs_encrypt_seeded_dev, synchronous) -> the bodies int32 [B], or (bodies, ct [B][n+1]) with full=True. mask_seed is public
        and must not encrypt two messages at one row; noise_seed is private and must differ from it."""
        lwe, plwe = _np_i32(lwe_key)
        assert lwe.size == self.p.n, "lwe_key must have n = %d words" % self.p.n
        B = mu.numel()
        body = self.empty(B)
        ct = self.empty(B, self.W) if full else None
        _check(self.L, self.L.rs_encrypt_seeded_dev(self.h, self._ck_dev(body), self._ck_dev(ct) if full else None, self._ck_dev(mu), B,
                                                    plwe, self._seed32(mask_seed, "mask_seed"), self._seed32(noise_seed, "noise_seed"),
                                                    int(first), float(stdev)))
        return (body, ct) if full else body

    def expand_ciphertexts(self, mask_seed, body, first=0, out=None):
        """The full samples [B][n+1] of seeded ciphertexts with bodies `body` (int32 CUDA tensor [B]), expanded on the device on
        torch's current stream (rs_expand_ciphertexts_dev) -> int32 CUDA tensor, ready for the gates and nets.*.run."""
        B = body.numel()
        out = self.empty(B, self.W) if out is None else out
        assert out.numel() == B * self.W, "out must hold [B][n+1] words"
        _check(self.L, self.L.rs_expand_ciphertexts_dev(self.h, self._ck_dev(out, self.W), self._seed32(mask_seed, "mask_seed"), int(first),
                                                        self._ck_dev(body), B, self._stream()))
        return out

    # ---- public-key encryption ----
    def pk_encrypt(self, pk, mu=None, rand_seed=None, first=0, base=None, out=None):
        """Encryption under a public key without the secret (rs_pk_encrypt_dev, on torch's current stream): out[i] = base[i] + (0, mu[i])
        + a random subset of the rows of pk, the subset of row first + i of rand_seed (32 bytes, PRIVATE; default a fresh os.urandom(32)
        per call: a (rand seed, row) pair must never be used twice). pk: int32 CUDA tensor [m][n+1] of encryptions of zero, or the
        client.SeededCiphertexts of SecretKeySet.public_key (expanded on the device first). mu: int32 CUDA tensor [B] of torus words or
        None; base: int32 CUDA tensor [B][n+1] or None (re-randomisation; out=base works in place). -> int32 CUDA tensor [B][n+1]."""
        if hasattr(pk, "mask_seed"):
            import torch
            body = pk.body if hasattr(pk.body, "is_cuda") else torch.from_numpy(np.ascontiguousarray(pk.body, np.int32)).to("cuda:%d" % self.device)
            pk = self.expand_ciphertexts(pk.mask_seed, body, pk.first)
        m = pk.numel() // self.W
        assert m >= 1 and pk.numel() == m * self.W, "pk must hold [m][n+1] words"
        given = mu if mu is not None else base if base is not None else out
        assert given is not None, "one of mu, base and out must give the batch size"
        B = given.numel() if mu is not None else given.numel() // self.W
        assert base is None or base.numel() == B * self.W, "base must hold [B][n+1] words"
        out = self.empty(B, self.W) if out is None else out
        assert out.numel() == B * self.W, "out must hold [B][n+1] words"
        seed = os.urandom(32) if rand_seed is None else self._seed32(rand_seed, "rand_seed")
        dev = lambda t, cols=None: None if t is None else self._ck_dev(t, cols)
        _check(self.L, self.L.rs_pk_encrypt_dev(self.h, self._ck_dev(out, self.W), self._ck_dev(pk, self.W), m, dev(mu), dev(base, self.W), B,
                                                seed, int(first), self._stream()))
        return out

    def pk_encrypt_bits(self, pk, bits, rand_seed=None, first=0, out=None):
        """pk_encrypt of the bits (host array of 0 / 1) in the gates' +-1/8 encoding -> int32 CUDA tensor [B][n+1]."""
        import torch
        e8 = 1 << 29
        mu = torch.from_numpy(np.where(np.asarray(bits).ravel() != 0, e8, -e8).astype(np.int32)).to("cuda:%d" % self.device)
        return self.pk_encrypt(pk, mu, rand_seed, first, out=out)

    # ---- compact RLWE public keys ----
    def rlwe_pk_encrypt(self, pk, mu, rand_seed=None, first=0, stdev=None, out=None):
        """Encryption under a compact RLWE public key without the secret (rs_rlwe_pk_encrypt_dev, on torch's current stream): ciphertext
        r = (a*u_r + e1, b*u_r + e2 + m_r) carries messages mu[rN .. rN + N - 1], the last one padded with zeros; u_r, e1, e2 are row
        first + r of rand_seed (32 bytes, PRIVATE; default a fresh os.urandom(32) per call: a (rand seed, row) pair must never be used
        twice). pk: int32 CUDA tensor [2][N] (a, then b) or the client.RlwePublicKey (expanded on the host first). mu: int32 CUDA tensor
        [count] of torus words. stdev: deviation of e1, e2; default the set's bk_stdev (ValueError on redsec_medium / redsec_large, where
        it truncates to zero: pass one). -> int32 CUDA tensor [ceil(count / N)][2][N]."""
        from . import keygen
        N = self.p.N
        if hasattr(pk, "mask_seed"):
            import torch
            if pk.name != keygen.set_name(self.p):    # same N is not enough: the default deviation is the set's
                raise ValueError("the public key is of %s, the context of %s" % (pk.name, keygen.set_name(self.p)))
            pk = torch.from_numpy(pk.expand()).to("cuda:%d" % self.device)
        assert pk.numel() == 2 * N, "pk must hold [2][N] words"
        count = mu.numel()
        R = -(-count // N)
        out = self.empty(R, 2, N) if out is None else out
        assert out.numel() == R * 2 * N, "out must hold [ceil(count / N)][2][N] words"
        stdev = keygen.rlwe_default_stdev(keygen.set_name(self.p)) if stdev is None else float(stdev)
        seed = os.urandom(32) if rand_seed is None else self._seed32(rand_seed, "rand_seed")
        _check(self.L, self.L.rs_rlwe_pk_encrypt_dev(self.h, self._ck_dev(out), self._ck_dev(pk), self._ck_dev(mu), count, seed, int(first),
                                                     stdev, self._stream()))
        return out

    def rlwe_extract(self, rlwe, count, out=None):
        """The LWE samples of the first `count` slots of RLWE ciphertexts [R][2][N] (rs_rlwe_extract_dev, on torch's current stream):
        sample rN + c is coefficient c of ciphertext r under the ring key read as an LWE key, the convention of bootstrap_wo_ks
        -> int32 CUDA tensor [count][N+1], ready for keyswitch and phase(dim = N)."""
        N, count = self.p.N, int(count)
        assert 0 <= count and rlwe.numel() == -(-count // N) * 2 * N, "rlwe must hold [ceil(count / N)][2][N] words"
        out = self.empty(count, N + 1) if out is None else out
        assert out.numel() == count * (N + 1), "out must hold [count][N+1] words"
        _check(self.L, self.L.rs_rlwe_extract_dev(self.h, self._ck_dev(out), self._ck_dev(rlwe), count, self._stream()))
        return out

    def rlwe_unpack(self, rlwe, count):
        """rlwe_extract followed by keyswitch (needs the loaded key): the first `count` messages of RLWE ciphertexts as LWE samples
        under the LWE key -> int32 CUDA tensor [count][n+1], ready for the gates and nets.*.run."""
        return self.keyswitch(self.rlwe_extract(rlwe, count))

    def rlwe_pk_encrypt_image(self, pk, pixels, preprocess="sign", rand_seed=None, first=0, stdev=None):
        """rlwe_pk_encrypt of client.SecretKeySet.encrypt_image's messages (2 pixel - 255, or the ReLU nets' pixel / 100 - 1, over
        4096) for the pixels (host array) -> int32 CUDA tensor [ceil(count / N)][2][N]; the server side is rlwe_unpack(., count)."""
        import torch
        px = np.asarray(pixels, dtype=np.int64).ravel()
        v = (px // 100 - 1) if preprocess == "relu" else 2 * px - 255
        mu = torch.from_numpy((v * (1 << 20)).astype(np.int32)).to("cuda:%d" % self.device)
        return self.rlwe_pk_encrypt(pk, mu, rand_seed, first, stdev)

    # ---- packed results ----
    def pack(self, ct, key, basebit=None, t=None, out=None):
        """LWE samples ct (int32 CUDA tensor [count][n+1]) keyswitched into the coefficients of RLWE ciphertexts (rs_pack_dev, on
        torch's current stream): ciphertext r packs samples rN .. rN + N - 1 -> int32 CUDA tensor [ceil(count / N)][2][N], the format
        of section 17 (rlwe_extract, rlwe_unpack, client.SecretKeySet.packed_phase). key: a client.PackingKey (uploaded and
        expanded on the device: keep the tensor of upload_packing_key for repeated calls; ValueError for a key of another set or another n) or
        an int32 CUDA tensor [n][t][2][N] with explicit basebit and t. Needs no loaded key."""
        from . import keygen
        N, n = self.p.N, self.p.n
        if hasattr(key, "mask_seed"):
            basebit, t, key = key.basebit, key.t, self.upload_packing_key(key)
        if basebit is None or t is None:
            raise ValueError("a packing key given as a tensor needs explicit basebit and t")
        basebit, t = keygen._check_digits(basebit, t)
        assert key.numel() == n * t * 2 * N, "key must hold [n][t][2][N] words"
        assert ct.numel() % (n + 1) == 0, "ct must hold [count][n+1] words"
        count = ct.numel() // (n + 1)
        R = -(-count // N)
        out = self.empty(R, 2, N) if out is None else out
        assert out.numel() == R * 2 * N, "out must hold [ceil(count / N)][2][N] words"
        _refuse_overlap("rlwe", out, out.numel(), (("ct", ct, ct.numel()), ("pack_key", key, key.numel())))
        _check(self.L, self.L.rs_pack_dev(self.h, self._ck_dev(out), self._ck_dev(ct), count, self._ck_dev(key), basebit, t, self._stream()))
        return out

    def upload_packing_key(self, key):
        """The expanded client.PackingKey on this context's device -> int32 CUDA tensor [n][t][2][N] (pass it to pack with key.basebit
        and key.t): the bodies are uploaded and the masks regenerated beside them on the device (expand_packing_key), half the bytes
        of the expanded key over the bus. ValueError for a key of another set or another n."""
        import torch
        from . import keygen
        if key.name != keygen.set_name(self.p) or key.n != self.p.n:
            raise ValueError("the packing key is of %s with n = %d, the context of %s with n = %d"
                             % (key.name, key.n, keygen.set_name(self.p), self.p.n))
        return self.expand_packing_key(key.mask_seed, torch.from_numpy(key.body).to("cuda:%d" % self.device), key.t)

    # ---- re-keying ----
    def rekey(self, ct, key, basebit=None, t=None, out=None):
        """LWE samples ct (int32 CUDA tensor [B][n_src+1]) keyswitched to a recipient's key under a caller-supplied key (rs_rekey_dev,
        on torch's current stream) -> int32 CUDA tensor [B][n_dst+1]. key: a client.RekeyKey (uploaded and expanded on this context's
        device, which must be of the destination's n, or ring for the RLWE form: keep the tensor of upload_rekey_key for repeated
        calls) or an int32 CUDA tensor [n_src][t][n_dst+1] with explicit basebit and t. Both dimensions come from the key, not from the
        context: a tensor key works on a context of any set. Needs no loaded key."""
        from . import keygen
        if hasattr(key, "form"):
            basebit, t, key = key.basebit, key.t, self.upload_rekey_key(key)
        if basebit is None or t is None:
            raise ValueError("a re-keying key given as a tensor needs explicit basebit and t")
        basebit, t = keygen._check_digits(basebit, t)
        if key.dim() != 3 or key.shape[1] != t or key.shape[2] < 2:
            raise ValueError("a re-keying key tensor must hold [n_src][t][n_dst+1] words with t = %d, not %s" % (t, tuple(key.shape)))
        n_src, n_dst = key.shape[0], key.shape[2] - 1
        assert ct.numel() % (n_src + 1) == 0, "ct must hold [B][n_src+1] words"
        B = ct.numel() // (n_src + 1)
        out = self.empty(B, n_dst + 1) if out is None else out
        assert out.numel() == B * (n_dst + 1), "out must hold [B][n_dst+1] words"
        _refuse_overlap("out", out, out.numel(), (("ct", ct, ct.numel()), ("rekey_key", key, key.numel())))
        _check(self.L, self.L.rs_rekey_dev(self.h, self._ck_dev(out), self._ck_dev(ct), B, n_src, self._ck_dev(key), n_dst, basebit, t,
                                           self._stream()))
        return out

    def upload_rekey_key(self, key):
        """The expanded client.RekeyKey on this context's device -> int32 CUDA tensor [n_src][t][n_dst+1] (pass it to rekey with
        key.basebit and key.t). Form "seeded": the bodies are uploaded and the masks regenerated beside them
        (rs_expand_ciphertexts_dev), on a context whose n is the key's n_dst; form "rlwe": the ciphertexts are uploaded, their
        rows extracted (rs_rlwe_extract_dev) and the odd ones negated back, on a context whose ring is the key's n_dst. ValueError names the mismatch otherwise."""
        import torch
        dev = "cuda:%d" % self.device
        if key.form == "seeded":
            if self.p.n != key.n_dst:
                raise ValueError("the re-keying key's destination has n = %d (%s), the context n = %d" % (key.n_dst, key.dst_name, self.p.n))
            rows = self.expand_ciphertexts(key.mask_seed, torch.from_numpy(key.body).to(dev), 0)
        else:
            if self.p.N != key.n_dst:
                raise ValueError("the re-keying key's destination is the ring key of N = %d (%s), the context's ring N = %d"
                                 % (key.n_dst, key.dst_name, self.p.N))
            rows = self.rlwe_extract(torch.from_numpy(key.rlwe).to(dev), key.rows)
            rows[1::2].neg_()                                   # keygen.rekey_alternate: the odd rows travel negated
        return rows.reshape(key.n_src, key.t, key.n_dst + 1)

    # ---- ring re-keying ----
    def ring_rekey(self, rlwe, key, basebit=None, t=None, out=None):
        """Packed ciphertexts rlwe (int32 CUDA tensor [R][2][N]) keyswitched to a recipient's ring key under a caller-supplied key
        (rs_ring_rekey_dev, on torch's current stream) -> int32 CUDA tensor [R][2][N] (or into `out`; an `out` that overlaps an input is
        refused with ValueError). key: a client.RingRekeyKey (uploaded on this context's device, whose ring must be the key's: keep the tensor of
        upload_ring_rekey_key for repeated calls) or an int32 CUDA tensor [t+1][2][N] with explicit basebit and t. Needs no loaded
        key."""
        from . import keygen
        N = self.p.N
        if hasattr(key, "form"):
            basebit, t, key = key.basebit, key.t, self.upload_ring_rekey_key(key)
        if basebit is None or t is None:
            raise ValueError("a ring re-keying key given as a tensor needs explicit basebit and t")
        basebit, t = keygen._check_ring_digits(basebit, t)
        assert key.numel() == (t + 1) * 2 * N, "key must hold [t+1][2][N] words"
        assert rlwe.numel() % (2 * N) == 0, "rlwe must hold [R][2][N] words"
        R = rlwe.numel() // (2 * N)
        out = self.empty(R, 2, N) if out is None else out
        assert out.numel() == R * 2 * N, "out must hold [R][2][N] words"
        _refuse_overlap("out", out, out.numel(), (("rlwe", rlwe, rlwe.numel()), ("ring_key", key, key.numel())))
        _check(self.L, self.L.rs_ring_rekey_dev(self.h, self._ck_dev(out), self._ck_dev(rlwe), R, self._ck_dev(key), basebit, t, self._stream()))
        return out

    def upload_ring_rekey_key(self, key):
        """The expanded client.RingRekeyKey on this context's device -> int32 CUDA tensor [t+1][2][N] (pass it to ring_rekey with
        key.basebit and key.t). The key is t + 1 rows, so the masks of the seeded form are regenerated on the host. ValueError for
        a key of another ring."""
        import torch
        if self.p.N != key.N:
            raise ValueError("the ring re-keying key is of N = %d (%s), the context's ring N = %d" % (key.N, key.dst_name, self.p.N))
        return torch.from_numpy(key.expand()).to("cuda:%d" % self.device)

    # ---- encrypted selection ----
    def _ring_selector(self, sel, basebit, l):
        from . import keygen
        depth = None
        if hasattr(sel, "body"):
            basebit, l, depth, sel = sel.basebit, sel.l, sel.depth, self.upload_ring_selector(sel)
        if basebit is None or l is None:
            raise ValueError("a selector given as a tensor needs explicit basebit and l")
        basebit, l = keygen._check_cmux_digits(basebit, l)
        per = 2 * l * 2 * self.p.N
        assert sel.numel() and sel.numel() % per == 0, "sel must hold [depth][2l][2][N] words"
        assert depth is None or sel.numel() == depth * per
        return sel, basebit, l, sel.numel() // per

    def ring_cmux(self, d1, d0, sel, basebit=None, l=None, stride=1, out=None, digits="signed"):
        """out[r] = d1[r stride] where the selector encrypts 1, d0[r stride] where it encrypts 0 (rs_ring_cmux_dev, on torch's
        current stream) -> int32 CUDA tensor [R][2][N], R = ceil(rows of d0 / stride) (or into `out`; an `out` that overlaps an input is
        refused with ValueError). d0, d1: int32 CUDA tensors [rows][2][N] of packed ciphertexts (Backend.pack, rlwe_pk_encrypt) or trivial ones
        (keygen.ring_trivial); d1 = None is the all-zero ciphertext. sel: a client.RingSelector of depth 1 (uploaded on this
        context's device: keep the tensor of upload_ring_selector for repeated calls) or an int32 CUDA tensor [2l][2][N] with
        explicit basebit and l. digits: "signed", or "alternating" (rs_ring_cmux_alt_dev, INTEGRATION.md section 25: the form for
        selectors made by circuit_bootstrap; the same selector serves either); ValueError for anything else. Needs no loaded key."""
        from . import keygen
        N = self.p.N
        call = self.L.rs_ring_cmux_alt_dev if keygen._check_cmux_form(digits) == "alternating" else self.L.rs_ring_cmux_dev
        sel, basebit, l, depth = self._ring_selector(sel, basebit, l)
        assert depth == 1, "ring_cmux takes one selector; ring_lookup takes a tree of them"
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride = %d is below 1" % stride)
        assert d0.numel() % (2 * N) == 0, "d0 must hold [rows][2][N] words"
        R = -(-(d0.numel() // (2 * N)) // stride)
        assert d1 is None or d1.numel() >= ((R - 1) * stride + 1) * 2 * N, "d1 must hold a row for every row read of d0"
        out = self.empty(R, 2, N) if out is None else out
        assert out.numel() == R * 2 * N, "out must hold [R][2][N] words"
        read = ((R - 1) * stride + 1) * 2 * N if R else 0                    # rows 0, stride, .. (R - 1) stride
        _refuse_overlap("out", out, out.numel(), (("d0", d0, read), ("d1", d1, read), ("sel", sel, sel.numel())))
        _check(self.L, call(self.h, self._ck_dev(out), None if d1 is None else self._ck_dev(d1), self._ck_dev(d0),
                            R, stride, self._ck_dev(sel), basebit, l, self._stream()))
        return out

    def ring_lookup(self, table, sel, basebit=None, l=None, out=None, digits="signed"):
        """table[index] for the index encrypted in sel (rs_ring_lookup_dev, on torch's current stream) -> int32 CUDA tensor [2][N]
        (or into `out`). table: int32 CUDA tensor [entries][2][N], entries <= 2^depth; sel: a client.RingSelector (uploaded on this
        context's device) or an int32 CUDA tensor [depth][2l][2][N] with explicit basebit and l. An index at or past `entries`
        gives an encryption of zero. The scratch of the call, ceil(E/2) + ceil(E/4) ciphertexts, is allocated here. digits: as
        ring_cmux ("alternating": rs_ring_lookup_alt_dev). Needs no loaded key."""
        from . import keygen
        N = self.p.N
        call = self.L.rs_ring_lookup_alt_dev if keygen._check_cmux_form(digits) == "alternating" else self.L.rs_ring_lookup_dev
        sel, basebit, l, depth = self._ring_selector(sel, basebit, l)
        assert table.numel() and table.numel() % (2 * N) == 0, "table must hold [entries][2][N] words"
        entries = table.numel() // (2 * N)
        if entries > 1 << depth:
            raise ValueError("%d entries need more than the %d selectors given" % (entries, depth))
        out = self.empty(2, N) if out is None else out
        assert out.numel() == 2 * N, "out must hold [2][N] words"
        _refuse_overlap("out", out, out.numel(), (("table", table, table.numel()), ("sel", sel, sel.numel())))
        first = (entries + 1) // 2
        scratch = self.empty(first + (first + 1) // 2, 2, N) if depth > 1 else None
        _check(self.L, call(self.h, self._ck_dev(out), self._ck_dev(table), entries, self._ck_dev(sel), depth,
                            basebit, l, None if scratch is None else self._ck_dev(scratch), self._stream()))
        return out

    def ring_lookup_rows(self, table, sel, entries=None, R=None, row_stride=0, entry_stride=1, per_row=None, basebit=None, l=None,
                         out=None, digits="signed"):
        """out[q] = table_q[index_q] for R hidden indices in one call (rs_ring_lookup_rows_dev, on torch's current stream;
        INTEGRATION.md section 28) -> int32 CUDA tensor [R][2][N] (or into `out`; an `out` that overlaps an input is refused with
        ValueError). table: int32 CUDA tensor of ciphertexts [..][2][N]; entry e of row q is ciphertext q row_stride + e entry_stride
        of it: (0, 1) one shared table (entries defaults to the table's rows), (entries, 1) R tables one after another, (1, R) the
        layout [entries][R][2][N]. sel: a client.RingSelector (one hidden index for all rows; uploaded on this context's device) or
        an int32 CUDA tensor with explicit basebit and l: [depth][2l][2][N], or [R][depth][2l][2][N] with one index per row; per_row
        is inferred from a 5-D tensor where it is None. R defaults to the number of selector sets. A selector of another ring or
        digit shape raises ValueError. The scratch of the call, R (ceil(E/2) + ceil(E/4)) ciphertexts, is allocated here. digits:
        as ring_cmux ("alternating": rs_ring_lookup_rows_alt_dev). Needs no loaded key."""
        from . import keygen
        N = self.p.N
        call = self.L.rs_ring_lookup_rows_alt_dev if keygen._check_cmux_form(digits) == "alternating" else self.L.rs_ring_lookup_rows_dev
        if hasattr(sel, "body"):
            basebit, l, sel = sel.basebit, sel.l, self.upload_ring_selector(sel)
        if basebit is None or l is None:
            raise ValueError("a selector given as a tensor needs explicit basebit and l")
        basebit, l = keygen._check_cmux_digits(basebit, l)
        per_row = sel.dim() == 5 if per_row is None else bool(per_row)
        if sel.dim() != (5 if per_row else 4) or tuple(sel.shape[-3:]) != (2 * l, 2, N):
            raise ValueError("sel must hold [depth][2l][2][N] words of the context's ring N = %d, or [R][depth][2l][2][N] with one "
                             "index per row; got %s" % (N, tuple(sel.shape)))
        depth = sel.shape[-4]
        if not 1 <= depth <= keygen.RING_LOOKUP_MAX_DEPTH:
            raise ValueError("depth = %d is outside 1 .. %d" % (depth, keygen.RING_LOOKUP_MAX_DEPTH))
        row_stride, entry_stride = int(row_stride), int(entry_stride)
        if row_stride < 0 or entry_stride < 1:
            raise ValueError("row_stride = %d, entry_stride = %d: row_stride must be at least 0 and entry_stride at least 1" % (row_stride, entry_stride))
        assert table.numel() and table.numel() % (2 * N) == 0, "table must hold ciphertexts of [2][N] words"
        held = table.numel() // (2 * N)
        if entries is None:
            if (row_stride, entry_stride) != (0, 1):
                raise ValueError("entries must be given with row_stride = %d, entry_stride = %d" % (row_stride, entry_stride))
            entries = held
        entries = int(entries)
        if not 1 <= entries <= 1 << depth:
            raise ValueError("entries = %d is outside 1 .. 2^%d" % (entries, depth))
        if R is None:
            R = sel.shape[0] if per_row else 1
        R = int(R)
        if R < 0 or (per_row and sel.shape[0] != R):
            raise ValueError("R = %d with %d selector sets" % (R, sel.shape[0] if per_row else 1))
        out = self.empty(R, 2, N) if out is None else out
        assert out.numel() == R * 2 * N, "out must hold [R][2][N] words"
        if R == 0:
            return out
        read = (R - 1) * row_stride + (entries - 1) * entry_stride + 1
        if read > held:
            raise ValueError("the table holds %d ciphertexts, the strides read %d" % (held, read))
        _refuse_overlap("out", out, out.numel(), (("table", table, read * 2 * N), ("sel", sel, sel.numel())))
        first = (entries + 1) // 2
        scratch = self.empty(R * (first + (first + 1) // 2), 2, N) if depth > 1 else None
        _check(self.L, call(self.h, self._ck_dev(out), self._ck_dev(table), entries, row_stride, entry_stride, R, self._ck_dev(sel), depth,
                            int(per_row), basebit, l, None if scratch is None else self._ck_dev(scratch), self._stream()))
        return out

    # ---- encrypted rotation ----
    def ring_rotate(self, rlwe, sel, step=-1, basebit=None, l=None, stride=1, per_row=None, out=None, digits="signed"):
        """out[r] = X^(step index_r) rlwe[r stride] for the index encrypted in sel (rs_ring_rotate_dev, on torch's current stream)
        -> int32 CUDA tensor [R][2][N] (or into `out`; an `out` that overlaps an input is refused with ValueError). step = -1 brings
        slot `index` to coefficient 0, step = -w slots w index .. w index + w - 1 to coefficients 0 .. w - 1. rlwe: int32 CUDA
        tensor [rows][2][N]; stride >= 1 reads every stride-th row, stride = 0 starts every row from rlwe[0] (R is then the number
        of selector sets). sel: a client.RingSelector (one hidden index for all rows; uploaded on this context's device) or an int32
        CUDA tensor with explicit basebit and l: [depth][2l][2][N], or [R][depth][2l][2][N] with one index per row. per_row is
        inferred from a 5-D tensor where it is None. The scratch of the call, R ciphertexts, is allocated here. digits: as
        ring_cmux ("alternating": rs_ring_rotate_alt_dev). Needs no loaded key."""
        from . import keygen
        N = self.p.N
        call = self.L.rs_ring_rotate_alt_dev if keygen._check_cmux_form(digits) == "alternating" else self.L.rs_ring_rotate_dev
        if hasattr(sel, "body"):
            basebit, l, sel = sel.basebit, sel.l, self.upload_ring_selector(sel)
        if basebit is None or l is None:
            raise ValueError("a selector given as a tensor needs explicit basebit and l")
        basebit, l = keygen._check_cmux_digits(basebit, l)
        per_row = sel.dim() == 5 if per_row is None else bool(per_row)
        assert sel.dim() == (5 if per_row else 4) and tuple(sel.shape[-3:]) == (2 * l, 2, N), \
            "sel must hold [depth][2l][2][N] words, or [R][depth][2l][2][N] with one index per row"
        depth = sel.shape[-4]
        if not 1 <= depth <= keygen.RING_LOOKUP_MAX_DEPTH:
            raise ValueError("depth = %d is outside 1 .. %d" % (depth, keygen.RING_LOOKUP_MAX_DEPTH))
        stride = int(stride)
        if stride < 0:
            raise ValueError("stride = %d is below 0" % stride)
        assert rlwe.numel() and rlwe.numel() % (2 * N) == 0, "rlwe must hold [rows][2][N] words"
        rows = rlwe.numel() // (2 * N)
        R = (sel.shape[0] if per_row else 1) if stride == 0 else -(-rows // stride)
        assert not per_row or sel.shape[0] == R, "one selector set per row"
        out = self.empty(R, 2, N) if out is None else out
        assert out.numel() == R * 2 * N, "out must hold [R][2][N] words"
        read = ((R - 1) * stride + 1) * 2 * N
        _refuse_overlap("out", out, out.numel(), (("in", rlwe, read), ("sel", sel, sel.numel())))
        scratch = self.empty(R, 2, N) if depth > 1 else None
        _check(self.L, call(self.h, self._ck_dev(out), self._ck_dev(rlwe), R, stride, self._ck_dev(sel), depth, int(per_row), int(step),
                            basebit, l, None if scratch is None else self._ck_dev(scratch), self._stream()))
        return out

    def ring_heads(self, rlwe, width=1, out=None):
        """The LWE samples of coefficients 0 .. width - 1 of each ciphertext of rlwe [R][2][N] (rs_ring_heads_dev, on torch's current
        stream): sample r width + c is coefficient c of ciphertext r in the convention of rlwe_extract -> int32 CUDA tensor
        [R width][N+1], ready for keyswitch (or into `out`; an `out` that overlaps rlwe is refused with ValueError)."""
        N, width = self.p.N, int(width)
        if not 1 <= width <= N:
            raise ValueError("width = %d is outside 1 .. %d" % (width, N))
        assert rlwe.numel() % (2 * N) == 0, "rlwe must hold [R][2][N] words"
        R = rlwe.numel() // (2 * N)
        out = self.empty(R * width, N + 1) if out is None else out
        assert out.numel() == R * width * (N + 1), "out must hold [R width][N+1] words"
        _refuse_overlap("u", out, out.numel(), (("rlwe", rlwe, rlwe.numel()),))
        _check(self.L, self.L.rs_ring_heads_dev(self.h, self._ck_dev(out), self._ck_dev(rlwe), R, width, self._stream()))
        return out

    def upload_ring_selector(self, sel):
        """The expanded client.RingSelector on this context's device -> int32 CUDA tensor [depth][2l][2][N] (pass it to ring_cmux or
        ring_lookup with sel.basebit and sel.l). The masks of the seeded rows are regenerated on the host. ValueError for a
        selector of another ring."""
        import torch
        if self.p.N != sel.N:
            raise ValueError("the selector is of N = %d (%s), the context's ring N = %d" % (sel.N, sel.name, self.p.N))
        return torch.from_numpy(sel.expand()).to("cuda:%d" % self.device)

    # ---- circuit bootstrapping ----
    def upload_selector_key(self, key):
        """The expanded client.SelectorKey on this context's device -> int32 CUDA tensor [2][n+1][ks_t][2][N] (pass it to
        ring_selector or circuit_bootstrap with key.ks_basebit and key.ks_t). The masks of the seeded rows are regenerated on the
        host. ValueError for a key of another ring."""
        import torch
        if self.p.N != key.N:
            raise ValueError("the selector key is of N = %d (%s), the context's ring N = %d" % (key.N, key.name, self.p.N))
        return torch.from_numpy(key.expand()).to("cuda:%d" % self.device)

    def _selector_key(self, key, ks_basebit, ks_t, n_src):
        from . import keygen
        if hasattr(key, "body"):
            if key.n != n_src:
                raise ValueError("the selector key is of n = %d, the samples of n_src = %d" % (key.n, n_src))
            ks_basebit, ks_t, key = key.ks_basebit, key.ks_t, self.upload_selector_key(key)
        if ks_basebit is None or ks_t is None:
            raise ValueError("a selector key given as a tensor needs explicit ks_basebit and ks_t")
        ks_basebit, ks_t = keygen._check_selector_digits(ks_basebit, ks_t)
        assert key.numel() == 2 * (n_src + 1) * ks_t * 2 * self.p.N, "key must hold [2][n_src+1][ks_t][2][N] words"
        return key, ks_basebit, ks_t

    def ring_selector(self, ct, basebit, l, key, ks_basebit=None, ks_t=None, n_src=None, out=None):
        """The selector keyswitch (rs_ring_selector_dev, on torch's current stream): ct int32 CUDA tensor [depth l][n_src+1], row k l
        + j the bootstrap of bit k at level j with phase +-h_j/2 -> int32 CUDA tensor [depth][2l][2][N], what ring_cmux and
        ring_lookup take (or into `out`; an `out` that overlaps an input is refused with ValueError). key: a client.SelectorKey (uploaded on this context's device:
        keep the tensor of upload_selector_key for repeated calls) or an int32 CUDA tensor [2][n_src+1][ks_t][2][N] with explicit
        ks_basebit and ks_t. n_src defaults to the last dimension of ct less one. Needs no loaded key."""
        from . import keygen
        basebit, l = keygen._check_cmux_digits(basebit, l)
        n_src = ct.shape[-1] - 1 if n_src is None else int(n_src)
        if not 1 <= n_src <= keygen.SELECTOR_MAX_SRC:
            raise ValueError("n_src = %d is outside 1 .. %d" % (n_src, keygen.SELECTOR_MAX_SRC))
        key, ks_basebit, ks_t = self._selector_key(key, ks_basebit, ks_t, n_src)
        assert ct.numel() % ((n_src + 1) * l) == 0, "ct must hold [depth l][n_src+1] words"
        depth = ct.numel() // ((n_src + 1) * l)
        if depth > keygen.RING_LOOKUP_MAX_DEPTH:
            raise ValueError("depth = %d is outside 0 .. %d" % (depth, keygen.RING_LOOKUP_MAX_DEPTH))
        out = self.empty(depth, 2 * l, 2, self.p.N) if out is None else out
        assert out.numel() == depth * 2 * l * 2 * self.p.N, "out must hold [depth][2l][2][N] words"
        _refuse_overlap("sel", out, out.numel(), (("ct", ct, ct.numel()), ("sel_key", key, key.numel())))
        if depth:
            _check(self.L, self.L.rs_ring_selector_dev(self.h, self._ck_dev(out), self._ck_dev(ct), depth, basebit, l, n_src,
                                                       self._ck_dev(key), ks_basebit, ks_t, self._stream()))
        return out

    def circuit_bootstrap(self, bits, basebit, l, key, ks_basebit=None, ks_t=None, out=None):
        """Selectors from bits the server computed (rs_circuit_bootstrap_dev, on torch's current stream): bits int32 CUDA tensor
        [depth][n+1] at +-1/8 under the loaded key -> int32 CUDA tensor [depth][2l][2][N] for ring_cmux / ring_lookup, selector k
        of bit k (or into `out`). key as in ring_selector, of the context's n. The scratch of the call is allocated here. Needs a
        loaded evaluation key."""
        from . import keygen
        basebit, l = keygen._check_cmux_digits(basebit, l)
        key, ks_basebit, ks_t = self._selector_key(key, ks_basebit, ks_t, self.p.n)
        assert bits.numel() % self.W == 0, "bits must hold [depth][n+1] words"
        depth = bits.numel() // self.W
        if depth > keygen.RING_LOOKUP_MAX_DEPTH:
            raise ValueError("depth = %d is outside 0 .. %d" % (depth, keygen.RING_LOOKUP_MAX_DEPTH))
        out = self.empty(depth, 2 * l, 2, self.p.N) if out is None else out
        assert out.numel() == depth * 2 * l * 2 * self.p.N, "out must hold [depth][2l][2][N] words"
        _refuse_overlap("sel", out, out.numel(), (("bits", bits, bits.numel()), ("sel_key", key, key.numel())))
        if depth:
            scratch = self.empty(l * self.p.N + depth * l * (2 * self.W + 1))
            _check(self.L, self.L.rs_circuit_bootstrap_dev(self.h, self._ck_dev(out), self._ck_dev(bits), depth, basebit, l,
                                                           self._ck_dev(key), ks_basebit, ks_t, self._ck_dev(scratch), self._stream()))
        return out

    # ---- batched circuit bootstrapping ----
    def ring_selector_batch(self, ct, basebit, l, key, ks_basebit=None, ks_t=None, n_src=None, out=None):
        """ring_selector for any number of bits in one call (rs_ring_selector_batch_dev, on torch's current stream): ct int32 CUDA
        tensor [count l][n_src+1] -> int32 CUDA tensor [count][2l][2][N] (or into `out`, 16-byte aligned; an `out` that overlaps an
        input is refused with ValueError), the words ring_selector gives for the same rows taken 30 bits at a time. key, ks_basebit,
        ks_t and n_src as in ring_selector. The library picks the kernel from the row count (last_selector tells which)."""
        from . import keygen
        basebit, l = keygen._check_cmux_digits(basebit, l)
        n_src = ct.shape[-1] - 1 if n_src is None else int(n_src)
        if not 1 <= n_src <= keygen.SELECTOR_MAX_SRC:
            raise ValueError("n_src = %d is outside 1 .. %d" % (n_src, keygen.SELECTOR_MAX_SRC))
        key, ks_basebit, ks_t = self._selector_key(key, ks_basebit, ks_t, n_src)
        assert ct.numel() % ((n_src + 1) * l) == 0, "ct must hold [count l][n_src+1] words"
        count = ct.numel() // ((n_src + 1) * l)
        out = self.empty(count, 2 * l, 2, self.p.N) if out is None else out
        assert out.numel() == count * 2 * l * 2 * self.p.N, "out must hold [count][2l][2][N] words"
        _refuse_overlap("sel", out, out.numel(), (("ct", ct, ct.numel()), ("sel_key", key, key.numel())))
        if count:
            _check(self.L, self.L.rs_ring_selector_batch_dev(self.h, self._ck_dev(out), self._ck_dev(ct), count, basebit, l, n_src,
                                                             self._ck_dev(key), ks_basebit, ks_t, self._stream()))
        return out

    def circuit_bootstrap_batch(self, bits, basebit, l, key, ks_basebit=None, ks_t=None, out=None):
        """circuit_bootstrap for any number of bits in one call (rs_circuit_bootstrap_batch_dev, on torch's current stream): bits
        int32 CUDA tensor [count][n+1] at +-1/8 under the loaded key -> int32 CUDA tensor [count][2l][2][N], selector k of bit k (or
        into `out`), the words circuit_bootstrap gives for the same bits taken 30 at a time: ONE bootstrap launch over the count l
        rows, then one selector keyswitch. key as in ring_selector, of the context's n. The scratch of the call is allocated here.
        Needs a loaded evaluation key."""
        from . import keygen
        basebit, l = keygen._check_cmux_digits(basebit, l)
        key, ks_basebit, ks_t = self._selector_key(key, ks_basebit, ks_t, self.p.n)
        assert bits.numel() % self.W == 0, "bits must hold [count][n+1] words"
        count = bits.numel() // self.W
        out = self.empty(count, 2 * l, 2, self.p.N) if out is None else out
        assert out.numel() == count * 2 * l * 2 * self.p.N, "out must hold [count][2l][2][N] words"
        _refuse_overlap("sel", out, out.numel(), (("bits", bits, bits.numel()), ("sel_key", key, key.numel())))
        if count:
            scratch = self.empty(l * self.p.N + count * l * (2 * self.W + 1))
            _check(self.L, self.L.rs_circuit_bootstrap_batch_dev(self.h, self._ck_dev(out), self._ck_dev(bits), count, basebit, l,
                                                                 self._ck_dev(key), ks_basebit, ks_t, self._ck_dev(scratch), self._stream()))
        return out

    def last_selector(self):
        """(form, workgroups) of this context's last selector keyswitch (ring_selector, circuit_bootstrap and their batch forms)."""
        f, n = C.c_int32(), C.c_int64()
        _check(self.L, self.L.rs_last_selector(self.h, C.byref(f), C.byref(n)))
        return {"form": ("chunked", "wide")[f.value], "workgroups": n.value}   # rs_ring_selector.h SeForm

    # ---- the packing key on the device ----
    def _secrets(self, lwe_key, tlwe_key):
        lwe, plwe = _np_i32(lwe_key)
        tlwe, ptlwe = _np_i32(tlwe_key)
        assert lwe.size == self.p.n and tlwe.size == self.p.N, "secret keys have the wrong size"
        return (lwe, tlwe), plwe, ptlwe

    def pack_keygen(self, lwe_key, tlwe_key, mask_seed, noise_seed, basebit, t, stdev, out=None):
        """Bodies of the packing key from lwe_key to tlwe_key (host, 0/1) generated on the device (rs_pack_keygen_dev, synchronous)
        -> int32 CUDA tensor [n][t][N] (or into `out`), the words of keygen.pack_key. stdev is taken as given (any finite value
        >= 0): the policy is client.SecretKeySet.packing_key's."""
        from . import keygen
        basebit, t = keygen._check_digits(basebit, t)
        keep, plwe, ptlwe = self._secrets(lwe_key, tlwe_key)
        out = self.empty(self.p.n, t, self.p.N) if out is None else out
        assert out.numel() == self.p.n * t * self.p.N, "out must hold [n][t][N] words"
        _check(self.L, self.L.rs_pack_keygen_dev(self.h, self._ck_dev(out), plwe, ptlwe, self._seed32(mask_seed, "mask_seed"),
                                                 self._seed32(noise_seed, "noise_seed"), basebit, t, float(stdev)))
        return out

    def expand_packing_key(self, mask_seed, body, t, out=None):
        """The full packing key of the bodies `body` (int32 CUDA tensor [n][t][N]) and the public mask seed, expanded on the device
        on torch's current stream (rs_pack_expand_dev) -> int32 CUDA tensor [n][t][2][N] (or into `out`), what pack takes."""
        t = int(t)
        assert t >= 1 and body.numel() == self.p.n * t * self.p.N, "body must hold [n][t][N] words"
        out = self.empty(self.p.n, t, 2, self.p.N) if out is None else out
        assert out.numel() == 2 * body.numel(), "out must hold [n][t][2][N] words"
        _check(self.L, self.L.rs_pack_expand_dev(self.h, self._ck_dev(out), self._seed32(mask_seed, "mask_seed"), self._ck_dev(body), t,
                                                 self._stream()))
        return out

    def audit_packing_key(self, lwe_key, tlwe_key, key, basebit, t, mask_seed=None, limit=None, noise=False):
        """Exact noise audit of a packing key in device memory under its secret (rs_audit_pack_key_dev, synchronous; CLIENT side): key
        is the full key [n][t][2][N], or with mask_seed= the bodies [n][t][N] (the masks are regenerated, nothing is expanded).
        limit defaults to keygen.pack_noise_limit of the set's default deviation (ValueError where that vanishes: pass one).
        -> a dict of the rs_pack_key_audit fields, plus noise [n][t][N] (int32 CUDA tensor) with noise=True."""
        from . import keygen
        basebit, t = keygen._check_digits(basebit, t)
        keep, plwe, ptlwe = self._secrets(lwe_key, tlwe_key)
        words = self.p.n * t * self.p.N
        assert key.numel() == (words if mask_seed is not None else 2 * words), "key has the wrong size"
        if limit is None:
            limit = keygen.pack_noise_limit(keygen.rlwe_default_stdev(keygen.set_name(self.p)))
        e = self.empty(self.p.n, t, self.p.N) if noise else None
        rep = RsPackKeyAudit()
        _check(self.L, self.L.rs_audit_pack_key_dev(self.h, C.byref(rep), None if e is None else self._ck_dev(e), self._ck_dev(key),
                                                    None if mask_seed is None else self._seed32(mask_seed, "mask_seed"), plwe, ptlwe,
                                                    basebit, t, int(limit)))
        out = {f: int(getattr(rep, f)) for f, _ in RsPackKeyAudit._fields_}
        if noise:
            out["noise"] = e
        return out

    # ---- device decryption and the noise audit of evaluation keys (CLIENT side) ----
    def phase(self, ct, key):
        """Phases b - sum_k a_k key_k of ct (int32 CUDA tensor [B][dim+1]) under the host 0/1 key of dim = len(key) words, taken on
        the device (rs_phase_dev, synchronous; waits for every stream of the device) -> int32 CUDA tensor [B]. dim = n with the LWE
        key, dim = N with the ring key for the output of bootstrap_wo_ks."""
        key, pkey = _np_i32(key)
        dim = key.size
        B = ct.numel() // (dim + 1)
        assert ct.numel() == B * (dim + 1), "ct must hold [B][dim+1] words"
        out = self.empty(B)
        _check(self.L, self.L.rs_phase_dev(self.h, self._ck_dev(out), self._ck_dev(ct), B, pkey, dim))
        return out

    def _audit(self, call, lwe_key, tlwe_key, bk, ksk, limits, noise, shapes, extra=()):
        from . import keygen
        p = self.p
        lwe, plwe = _np_i32(lwe_key)
        tlwe, ptlwe = _np_i32(tlwe_key)
        assert lwe.size == p.n and tlwe.size == p.N, "secret keys have the wrong size"
        assert bk is None or bk.numel() == shapes[0], "bk has the wrong size"
        assert ksk is None or ksk.numel() == shapes[1], "ksk has the wrong size"
        bk_limit, ksk_limit = keygen.noise_limits(keygen.set_name(p)) if limits is None else limits
        bk_noise = self.empty(p.n, 2 * p.bk_l, p.N) if noise and bk is not None else None
        ksk_noise = self.empty(p.N, p.ks_t, 1 << p.ks_basebit) if noise and ksk is not None else None
        dev = lambda t: None if t is None else self._ck_dev(t)
        rep = RsKeyAudit()
        _check(self.L, call(self.h, C.byref(rep), dev(bk_noise), dev(ksk_noise), *extra, dev(bk), dev(ksk), plwe, ptlwe,
                            int(bk_limit), int(ksk_limit)))
        out = {f: int(getattr(rep, f)) for f, _ in RsKeyAudit._fields_}
        if noise:
            out.update(bk_noise=bk_noise, ksk_noise=ksk_noise)
        return out

    def audit_keys(self, lwe_key, tlwe_key, bk=None, ksk=None, limits=None, noise=False):
        """Exact noise audit of a full evaluation key in device memory under its secret (rs_audit_keys_dev, synchronous): bk
        [n][2l][2][N] and ksk [N][t][2^basebit][n+1] int32 CUDA tensors, either may be None (skipped). limits = (bk_limit, ksk_limit),
        default keygen.noise_limits of the set. -> a dict of the rs_key_audit fields, plus bk_noise [n][2l][N] and ksk_noise
        [N][t][2^basebit] (int32 CUDA tensors, None for a skipped half) with noise=True."""
        return self._audit(self.L.rs_audit_keys_dev, lwe_key, tlwe_key, bk, ksk, limits, noise, self._key_sizes())

    def audit_compressed_keys(self, lwe_key, tlwe_key, mask_seed, bk_body, ksk_body, limits=None, noise=False):
        """The same audit of a compressed key, without expanding it (rs_audit_compressed_keys_dev): the masks are regenerated from
        the public mask seed."""
        return self._audit(self.L.rs_audit_compressed_keys_dev, lwe_key, tlwe_key, bk_body, ksk_body, limits, noise, self._body_sizes(),
                           extra=(self._seed32(mask_seed, "mask_seed"),))

    def load_synthetic_keys(self, seed):
        """A key of pseudo-random words generated ON THE DEVICE (rs_load_synthetic_keys; client.synthetic_key_words restates the
        generator): benchmarks and parity tests of the large rings, whose real keys are gigabytes on the host."""
        _check(self.L, self.L.rs_load_synthetic_keys(self.h, C.c_uint64(int(seed) & (2**64 - 1))))

    def release_stream(self, stream):
        _check(self.L, self.L.rs_release_stream(self.h, C.c_void_p(int(stream))))

    def reserve(self, max_batch):
        """Pre-size the workspace of torch's current stream."""
        _check(self.L, self.L.rs_reserve_stream(self.h, int(max_batch), self._stream()))

    # ---- torch plumbing ----
    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _ck_dev(self, t, cols=None):
        import torch
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous(), "need contiguous int32 CUDA tensors"
        assert t.device.index == self.device, "tensor is on another device than the context"
        if cols is not None:
            assert t.shape[-1] == cols, "last dimension must be %d words" % cols
        return C.c_void_p(t.data_ptr())

    def empty(self, *shape):
        import torch
        return torch.empty(*shape, dtype=torch.int32, device="cuda:%d" % self.device)

    # ---- bootstraps on device tensors [B][W] ----
    def bootstrap(self, x, mu, out=None):
        B = x.shape[0]
        out = self.empty(B, self.W) if out is None else out
        _check(self.L, self.L.rs_bootstrap_dev(self.h, self._ck_dev(out, self.W), self._ck_dev(x, self.W), int(mu), B, self._stream()))
        return out

    def bootstrap_sparse(self, rows, mu, live, out=None):
        """bootstrap of a batch whose rows outside `live` are KNOWN trivial samples (rs_bootstrap_sparse_dev; INTEGRATION.md section
        20). rows [B][W]; live: int32 CUDA tensor of the rows that are really bootstrapped (entries outside [0, B) are ignored). An
        unlisted row is read at its last word only and gets the trivial sample the dense call yields for it. out may be rows."""
        import torch
        B = rows.shape[0]
        out = self.empty(B, self.W) if out is None else out
        assert out.numel() == B * self.W, "out must hold [B][n+1] words"
        n_live = int(live.numel())
        assert live.dtype == torch.int32 and (n_live == 0 or (live.is_cuda and live.is_contiguous() and live.device.index == self.device)), \
            "live must be a contiguous int32 CUDA tensor on the context's device"
        _check(self.L, self.L.rs_bootstrap_sparse_dev(self.h, self._ck_dev(out, self.W), self._ck_dev(rows, self.W), int(mu), B,
                                                       C.c_void_p(live.data_ptr()) if n_live else None, n_live, self._stream()))
        return out

    def bootstrap_lut(self, x, lut, out=None, first=0):
        """Programmable bootstrap: ciphertext b uses the test polynomial lut[(first + b) % len(lut)] (int32 CUDA [L][N])."""
        B = x.shape[0]
        out = self.empty(B, self.W) if out is None else out
        _check(self.L, self.L.rs_bootstrap_lut_dev(self.h, self._ck_dev(out, self.W), self._ck_dev(x, self.W),
                                                    self._ck_dev(lut, self.p.N), lut.shape[0], int(first), B, self._stream()))
        return out

    def gate(self, op, a, b, out=None):
        B = a.shape[0]
        out = self.empty(B, self.W) if out is None else out
        _check(self.L, self.L.rs_gate_dev(self.h, GATES[op], self._ck_dev(out, self.W), self._ck_dev(a, self.W),
                                           self._ck_dev(b, self.W), B, self._stream()))
        return out

    def gate_mu(self, op, a, b, mu, out=None):
        B = a.shape[0]
        out = self.empty(B, self.W) if out is None else out
        _check(self.L, self.L.rs_gate_mu_dev(self.h, GATES[op], self._ck_dev(out, self.W), self._ck_dev(a, self.W),
                                              self._ck_dev(b, self.W), int(mu), B, self._stream()))
        return out

    def gather_rows(self, x, index):
        """out[i] = x[index[i]] (index: int32 CUDA tensor; negative -> zero sample)."""
        B = index.numel()
        out = self.empty(B, self.W)
        _check(self.L, self.L.rs_gather_rows_dev(self.h, self._ck_dev(out), self._ck_dev(x, self.W), C.c_void_p(index.data_ptr()), B,
                                                  self._stream()))
        return out

    def gate3(self, op, a, b, c, out=None):
        """out[i] = op(a[i], b[i], c[i]) for op in 'MAJ3' | 'XOR3' | 'MAJ3N' (rs_gate3_dev; +-1/8 in, +-1/8 out)."""
        B = a.shape[0]
        out = self.empty(B, self.W) if out is None else out
        _check(self.L, self.L.rs_gate3_dev(self.h, ROW_OPS[op] if isinstance(op, str) else int(op), self._ck_dev(out, self.W),
                                            self._ck_dev(a, self.W), self._ck_dev(b, self.W), self._ck_dev(c, self.W), B, self._stream()))
        return out

    def gate_rows(self, inp, idx, groups, mu=None, out=None):
        """One bootstrap batch of mixed gates over indexed rows (rs_gate_rows_dev). inp [in_rows][W]; idx int32 CUDA [B][3]: the three
        source rows of every output row (-2: constant TRUE, any other index outside [0, in_rows): constant FALSE); groups: a list of
        (op, count) cutting the B rows into consecutive runs, op a ROW_OPS name or number; mu: the output encoding (default 1/8).
        out [B][W] may be rows of inp, also rows this call reads."""
        B = idx.numel() // 3
        assert idx.numel() == 3 * B, "idx must hold [B][3] indices"
        in_rows = inp.numel() // self.W
        out = self.empty(B, self.W) if out is None else out
        assert out.numel() == B * self.W, "out must hold [B][n+1] words"
        gs = (RsRowGroup * max(1, len(groups)))()
        for g, (op, count) in zip(gs, groups):
            g.op, g.reserved, g.count = (ROW_OPS[op] if isinstance(op, str) else int(op)), 0, int(count)
        _check(self.L, self.L.rs_gate_rows_dev(self.h, self._ck_dev(out, self.W), self._ck_dev(inp, self.W), in_rows, self._ck_dev(idx),
                                                gs, len(groups), (1 << 29) if mu is None else int(mu), B, self._stream()))
        return out

    # ---- compiled circuits (redsec_amd/circuit.py builds the tables) ----
    def circuit_create(self, table, level_end, n_inputs):
        """rs_circuit_create: table = numpy array of CELL_DTYPE sorted by level, level_end = one past the last cell of every level
        -> an opaque handle that lives until circuit_destroy or close()."""
        table = np.ascontiguousarray(table, dtype=CELL_DTYPE)
        level_end = np.ascontiguousarray(level_end, dtype=np.uint32)
        h = C.c_void_p()
        _check(self.L, self.L.rs_circuit_create(self.h, C.byref(h), table.ctypes.data_as(C.c_void_p), len(table),
                                                 level_end.ctypes.data_as(C.POINTER(C.c_uint32)), len(level_end), int(n_inputs)))
        return h

    def circuit_destroy(self, handle):
        _check(self.L, self.L.rs_circuit_destroy(self.h, handle))

    def circuit_run(self, handle, arena, lanes):
        """rs_circuit_run_dev on torch's current stream: arena int32 CUDA [n_inputs + n_cells][lanes][W] with the input rows
        filled; every other row is written. -> arena."""
        assert arena.numel() % (self.W * max(1, int(lanes))) == 0, "arena must hold [wires][lanes][n+1] words"
        _check(self.L, self.L.rs_circuit_run_dev(self.h, handle, self._ck_dev(arena, self.W), int(lanes), self._stream()))
        return arena

    def mux(self, a, b, c, out=None):
        B = a.shape[0]
        out = self.empty(B, self.W) if out is None else out
        _check(self.L, self.L.rs_mux_dev(self.h, self._ck_dev(out, self.W), self._ck_dev(a, self.W), self._ck_dev(b, self.W),
                                          self._ck_dev(c, self.W), B, self._stream()))
        return out

    def bootstrap_wo_ks(self, x, mu):
        B = x.shape[0]
        u = self.empty(B, self.p.N + 1)
        _check(self.L, self.L.rs_bootstrap_wo_ks_dev(self.h, self._ck_dev(u), self._ck_dev(x, self.W), int(mu), B, self._stream()))
        return u

    def keyswitch(self, u):
        B = u.shape[0]
        out = self.empty(B, self.W)
        _check(self.L, self.L.rs_keyswitch_dev(self.h, self._ck_dev(out), self._ck_dev(u, self.p.N + 1), B, self._stream()))
        return out

    # ---- linear stage ----
    def lincomb(self, a, ca, b=None, cb=0, bconst=0):
        B = a.numel() // self.W
        out = self.empty(*a.shape)
        pb = self._ck_dev(b, self.W) if b is not None else None
        _check(self.L, self.L.rs_lincomb_dev(self.h, self._ck_dev(out), self._ck_dev(a, self.W), int(ca), pb, int(cb),
                                              int(bconst), B, self._stream()))
        return out

    def _u8(self, t):
        import torch
        if t is None:
            return None
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
        return C.c_void_p(t.data_ptr())

    def linear_fc(self, x, sign, zero=None, zero_tap_b=0, bias_b=None):
        """x [K][W]; sign/zero uint8 [K][M] -> [M][W]."""
        K = x.shape[0]
        M = sign.shape[1]
        out = self.empty(M, self.W)
        pbias = self._ck_dev(bias_b) if bias_b is not None else None
        depth = int(bias_b.numel()) if bias_b is not None else 0
        _check(self.L, self.L.rs_linear_fc_dev(self.h, self._ck_dev(out), self._ck_dev(x, self.W), self._u8(sign), self._u8(zero),
                                                K, M, int(zero_tap_b), pbias, depth, self._stream()))
        return out

    def conv_ternary(self, x, sign, zero, shape, zero_tap_b=0, pad_tap_b=0, bias_b=None):
        """x [H][Wd][Cin][W] -> [Ho][Wo][Cout][W]; shape: dict of rs_conv_shape fields."""
        s = RsConvShape(**shape)
        out = self.empty(s.Ho, s.Wo, s.Cout, self.W)
        pbias = self._ck_dev(bias_b) if bias_b is not None else None
        depth = int(bias_b.numel()) if bias_b is not None else 0
        _check(self.L, self.L.rs_conv_ternary_dev(self.h, self._ck_dev(out), self._ck_dev(x, self.W), self._u8(sign),
                                                   self._u8(zero), C.byref(s), int(zero_tap_b), int(pad_tap_b), pbias, depth,
                                                   self._stream()))
        return out

    def sumpool(self, x, shape, bias_b=None):
        s = RsPoolShape(**shape)
        out = self.empty(s.Ho, s.Wo, s.C, self.W)
        pbias = self._ck_dev(bias_b) if bias_b is not None else None
        depth = int(bias_b.numel()) if bias_b is not None else 0
        _check(self.L, self.L.rs_sumpool_dev(self.h, self._ck_dev(out), self._ck_dev(x, self.W), C.byref(s), pbias, depth,
                                              self._stream()))
        return out

    # ---- host (numpy) conveniences: synchronous H2D -> kernels -> D2H inside the library ----
    def bootstrap_host(self, x, mu):
        x, px = _np_i32(x)
        out = np.empty_like(x)
        _check(self.L, self.L.rs_bootstrap(self.h, out.ctypes.data_as(_i32p), px, int(mu), x.shape[0]))
        return out

    def gate_host(self, op, a, b):
        a, pa = _np_i32(a)
        b, pb = _np_i32(b)
        out = np.empty_like(a)
        _check(self.L, self.L.rs_gate(self.h, GATES[op], out.ctypes.data_as(_i32p), pa, pb, a.shape[0]))
        return out

    def mux_host(self, a, b, c):
        a, pa = _np_i32(a)
        b, pb = _np_i32(b)
        c, pc = _np_i32(c)
        out = np.empty_like(a)
        _check(self.L, self.L.rs_mux(self.h, out.ctypes.data_as(_i32p), pa, pb, pc, a.shape[0]))
        return out

    def polymul_host(self, a_small, b_torus):
        a, pa = _np_i32(a_small)
        b, pb = _np_i32(b_torus)
        out = np.empty_like(b)
        _check(self.L, self.L.rs_debug_polymul(self.h, out.ctypes.data_as(_i32p), pa, pb, a.size // self.p.N))
        return out

    # ---- arithmetic mode ----
    def set_mode(self, mode):
        """'fft' (default), 'exact' (exact NTT) or 'split' (split-key FFT, exact by an a-priori bound; the only mode of
        the parameter sets outside the specialised N = 1024 kernels)."""
        _check(self.L, self.L.rs_set_mode(self.h, {"exact": 0, "ntt": 0, "fft": 1, "split": 2}[mode]))

    def mode(self):
        m = C.c_int()
        _check(self.L, self.L.rs_get_mode(self.h, C.byref(m)))
        return {0: "exact", 1: "fft", 2: "split"}[m.value]

    def split_bound(self):
        """A-priori bound on the rounding distance of the split-key product for this parameter set."""
        d = C.c_double()
        _check(self.L, self.L.rs_split_bound(self.h, C.byref(d)))
        return d.value

    def rounding_certificate(self, reset=True):
        d = C.c_double()
        _check(self.L, self.L.rs_rounding_certificate(self.h, C.byref(d), 1 if reset else 0))
        return d.value

    def fft_fallbacks(self):
        """Calls (all streams) whose FFT result was recomputed exactly on the device: certificate >= the limit."""
        n = C.c_int64()
        _check(self.L, self.L.rs_fft_fallbacks(self.h, C.byref(n)))
        return n.value

    def set_certificate_limit(self, limit):
        """Rounding distance at which a call is recomputed exactly (default 0.25; 0 forces every call)."""
        _check(self.L, self.L.rs_set_certificate_limit(self.h, float(limit)))

    def certify(self, reset=True):
        """Synchronise torch's current stream -> (largest rounding distance, calls recomputed exactly) on it."""
        d, n = C.c_double(), C.c_int64()
        _check(self.L, self.L.rs_certify(self.h, self._stream(), C.byref(d), C.byref(n), 1 if reset else 0))
        return d.value, n.value

    def last_launch(self):
        """(form, waves per workgroup, ciphertexts per key sweep) of the last blind rotation on the current stream."""
        f, w, r = C.c_int32(), C.c_int32(), C.c_int64()
        _check(self.L, self.L.rs_last_launch(self.h, self._stream(), C.byref(f), C.byref(w), C.byref(r)))
        return {"form": ["per_wave", "workgroup", "duo", "coop2", "coop4", "general", "split_workgroup", "split_coop", "split_duo", "coop8", "coop8_listed"][f.value], "waves_per_block": w.value, "resident": r.value}

    def last_keyswitch(self):
        """(form, slices of the input coefficients) of the last keyswitch on the current stream."""
        f, n = C.c_int32(), C.c_int32()
        _check(self.L, self.L.rs_last_keyswitch(self.h, self._stream(), C.byref(f), C.byref(n)))
        return {"form": ["gather", "tiled", "sliced", "wide"][f.value], "slices": n.value}

    def fp64_rate(self):
        """FP64 FMA lane-operations per second this device sustains right now (box calibration, see include/redsec_hip.h)."""
        v = C.c_double()
        _check(self.L, self.L.rs_debug_fp64_rate(self.h, C.byref(v)))
        return v.value

    def cohort_table(self):
        """Progress table [8 XCDs][64 slots] of the current stream's last lock-step launch with XCD cohorts (debug tap)."""
        out = np.empty((8, 64), dtype=np.int32)
        _check(self.L, self.L.rs_debug_cohort_table(self.h, self._stream(), out.ctypes.data_as(_i32p)))
        return out

    # ---- timing / facts ----
    def set_timing(self, on=True):
        _check(self.L, self.L.rs_set_timing(self.h, 1 if on else 0))

    def last_kernel_ms(self):
        a, b = C.c_float(), C.c_float()
        _check(self.L, self.L.rs_last_kernel_ms_stream(self.h, self._stream(), C.byref(a), C.byref(b)))
        return a.value, b.value

    def info(self):
        bk, ksk, wpb, cus = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        _check(self.L, self.L.rs_info(self.h, C.byref(bk), C.byref(ksk), C.byref(wpb), C.byref(cus)))
        return {"bk_device_bytes": bk.value, "ksk_device_bytes": ksk.value, "waves_per_block": wpb.value, "num_cus": cus.value}

    def sync(self):
        _check(self.L, self.L.rs_sync(self.h))
