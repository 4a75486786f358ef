"""What the key-material and client-side entry points refuse, as a table: for every such call of include/redsec_hip.h the bad
arguments it turns down on the host, with the return code and the exact text of rs_last_error(), rows with two faults at once
(the first check in the call's order wins), and, behind every refused call that takes a secret key, one valid call whose outputs
equal what the same call wrote before the refusal. One toy context (default-128 gadget, reduced n), one item per call. Nothing
here launches a kernel on bad arguments: every row is refused before any launch, and every buffer is large enough for the
arguments of its rows had they been accepted."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID = -1
MASK_SEED = bytes(range(1, 33))
NOISE_SEED = bytes(range(101, 133))
BK_STDEV, KS_STDEV, STDEV = 2.0 ** -25, 2.0 ** -15, 2.0 ** -20
BASEBIT, T = 4, 2                       # digits of the packing key
T_MAX = 33                              # the largest t of a row below
FIRST_MAX = 2 ** 64 - 1
NAN, INF = float("nan"), float("inf")

NULL = "null pointer"
EQUAL = "mask seed and noise seed are equal: the public mask seed would reveal the noise"
ALIGN = "bk must be 16-byte aligned"
BOTH = "both halves of the key are null: nothing to audit"


class Off:
    """a device pointer `by` bytes into a tensor"""
    def __init__(self, tensor, by):
        self.tensor, self.by = tensor, by


# name -> the arguments behind the context, in the order of the C signature
SIGNATURES = {
    "rs_keygen_dev": ("bk", "ksk", "lwe_key", "tlwe_key", "seed", "bk_stdev", "ks_stdev"),
    "rs_keygen_compressed_dev": ("bk", "ksk", "lwe_key", "tlwe_key", "seed", "noise_seed", "bk_stdev", "ks_stdev"),
    "rs_expand_keys_dev": ("bk", "ksk", "seed", "bk_body", "ksk_body"),
    "rs_encrypt_seeded_dev": ("body", "ct", "mu", "B", "lwe_key", "seed", "noise_seed", "first", "stdev"),
    "rs_expand_ciphertexts_dev": ("ct", "seed", "first", "body", "B", "stream"),
    "rs_pk_encrypt_dev": ("ct", "pk", "m", "mu", "base", "B", "seed", "first", "stream"),
    "rs_rlwe_pk_encrypt_dev": ("rlwe", "pk", "mu", "count", "seed", "first", "stdev", "stream"),
    "rs_rlwe_extract_dev": ("u", "rlwe", "count", "stream"),
    "rs_pack_dev": ("rlwe", "ct", "count", "pack_key", "basebit", "t", "stream"),
    "rs_pack_keygen_dev": ("body", "lwe_key", "tlwe_key", "seed", "noise_seed", "basebit", "t", "stdev"),
    "rs_pack_expand_dev": ("pack_key", "seed", "body", "t", "stream"),
    "rs_phase_dev": ("phase", "ct", "B", "key", "dim"),
    "rs_audit_keys_dev": ("report", "bk_noise", "ksk_noise", "bk", "ksk", "lwe_key", "tlwe_key", "bk_limit", "ksk_limit"),
    "rs_audit_compressed_keys_dev": ("report", "bk_noise", "ksk_noise", "seed", "bk", "ksk", "lwe_key", "tlwe_key", "bk_limit",
                                     "ksk_limit"),
    "rs_audit_pack_key_dev": ("report", "noise", "key", "seed", "lwe_key", "tlwe_key", "basebit", "t", "limit"),
}
# the calls that take a secret key, and what a valid call of each writes
SECRET_OUTPUTS = {
    "rs_keygen_dev": ("bk", "ksk"), "rs_keygen_compressed_dev": ("bk", "ksk"), "rs_encrypt_seeded_dev": ("body", "ct"),
    "rs_pack_keygen_dev": ("body",), "rs_phase_dev": ("phase",), "rs_audit_keys_dev": ("report",),
    "rs_audit_compressed_keys_dev": ("report",), "rs_audit_pack_key_dev": ("report",),
}


def _bad(key, at):
    """a marker: the default key of that name with a word of 2 at index `at` (-1: the last)"""
    return ("bad", key, at)


def _deviations(fmt, names):
    """rows for -1, nan and inf in each deviation argument; fmt takes the values of `names` in order"""
    good = {"bk_stdev": BK_STDEV, "ks_stdev": KS_STDEV, "stdev": STDEV}
    rows = []
    for name in names:
        for x in (-1.0, NAN, INF):
            rows.append(({name: x}, fmt % tuple(x if k == name else good[k] for k in names)))
    return rows


def _key_rows(names=("lwe_key", "tlwe_key"), label=None):
    """rows for a word of 2 at index 0 and at the last index of each key; the text names the key and the index"""
    return [({name: _bad(name, at)}, (label or name, at)) for name in names for at in (0, -1)]


def _nulls(names):
    return [({name: None}, NULL) for name in names]


DEV2 = "noise deviations must be finite and non-negative (bk %g, ks %g)"
DEV1 = "noise deviation must be finite and non-negative (%g)"
OVERFLOW_B = "first + B = 18446744073709551615 + 2 passes 2^64"
DIGITS = [({"basebit": 0}, "basebit = 0 is outside 1 .. 8"), ({"basebit": 9}, "basebit = 9 is outside 1 .. 8"),
          ({"t": 0}, "t = 0 is below 1"), ({"t": T_MAX, "basebit": 1}, "t basebit = 33 x 1 passes 32 bits")]
NO_CTX = [({"ctx": None}, "null context")]

# name -> [(overrides of the valid arguments, text of rs_last_error())]; every row returns RS_ERR_INVALID.
# A text given as (key name, index) stands for "<key>[<i>] = 2 is not 0 or 1" with the index resolved against the key's length.
TABLE = {
    "rs_keygen_dev":
        NO_CTX + _nulls(("bk", "ksk", "lwe_key", "tlwe_key", "seed")) + [({"bk": "misaligned"}, ALIGN)] +
        _deviations(DEV2, ("bk_stdev", "ks_stdev")) + _key_rows() + [
            ({"ksk": None, "bk": "misaligned"}, NULL), ({"bk": "misaligned", "bk_stdev": NAN}, ALIGN),
            ({"ks_stdev": -1.0, "lwe_key": _bad("lwe_key", 0)}, DEV2 % (BK_STDEV, -1.0)),
            ({"lwe_key": _bad("lwe_key", -1), "tlwe_key": _bad("tlwe_key", 0)}, ("lwe_key", -1))],
    "rs_keygen_compressed_dev":
        NO_CTX + _nulls(("bk", "ksk", "lwe_key", "tlwe_key", "seed", "noise_seed")) + [({"bk": "misaligned"}, ALIGN)] +
        [({"noise_seed": MASK_SEED}, EQUAL)] + _deviations(DEV2, ("bk_stdev", "ks_stdev")) + _key_rows() + [
            ({"ctx": None, "noise_seed": None}, NULL), ({"noise_seed": None, "bk": "misaligned"}, NULL),
            ({"bk": "misaligned", "noise_seed": MASK_SEED}, ALIGN),
            ({"noise_seed": MASK_SEED, "bk_stdev": INF}, EQUAL),
            ({"bk_stdev": NAN, "tlwe_key": _bad("tlwe_key", 0)}, DEV2 % (NAN, KS_STDEV)),
            ({"lwe_key": _bad("lwe_key", 0), "tlwe_key": _bad("tlwe_key", -1)}, ("lwe_key", 0))],
    "rs_expand_keys_dev":
        NO_CTX + _nulls(("bk", "ksk", "seed", "bk_body", "ksk_body")) + [({"bk": "misaligned"}, ALIGN)] + [
            ({"ksk_body": None, "bk": "misaligned"}, NULL)],
    "rs_encrypt_seeded_dev":
        NO_CTX + _nulls(("body", "mu", "lwe_key", "seed", "noise_seed")) + [({"noise_seed": MASK_SEED}, EQUAL)] +
        _deviations(DEV1, ("stdev",)) + _key_rows(("lwe_key",)) + [({"first": FIRST_MAX, "B": 2}, OVERFLOW_B)] + [
            ({"mu": None, "noise_seed": MASK_SEED}, NULL), ({"noise_seed": MASK_SEED, "stdev": NAN}, EQUAL),
            ({"stdev": -1.0, "lwe_key": _bad("lwe_key", 0)}, DEV1 % -1.0),
            ({"lwe_key": _bad("lwe_key", -1), "first": FIRST_MAX, "B": 2}, ("lwe_key", -1))],
    "rs_expand_ciphertexts_dev":
        NO_CTX + _nulls(("ct", "seed", "body")) + [({"first": FIRST_MAX, "B": 2}, OVERFLOW_B)] + [
            ({"body": None, "first": FIRST_MAX, "B": 2}, NULL)],
    "rs_pk_encrypt_dev":
        NO_CTX + _nulls(("ct", "pk", "seed")) + [({"m": 0}, "m = 0 is outside 1 .. 2^31 - 1")] +
        [({"first": FIRST_MAX, "B": 2}, OVERFLOW_B)] + [
            ({"pk": None, "m": 0}, NULL), ({"m": 0, "first": FIRST_MAX, "B": 2}, "m = 0 is outside 1 .. 2^31 - 1")],
    "rs_rlwe_pk_encrypt_dev":
        NO_CTX + _nulls(("rlwe", "pk", "mu", "seed")) + _deviations(DEV1, ("stdev",)) +
        [({"first": FIRST_MAX, "count": "2N"}, "first + R = 18446744073709551615 + 2 passes 2^64")] + [
            ({"mu": None, "stdev": NAN}, NULL), ({"stdev": INF, "first": FIRST_MAX, "count": "2N"}, DEV1 % INF)],
    "rs_rlwe_extract_dev": NO_CTX + _nulls(("u", "rlwe")),
    "rs_pack_dev":
        NO_CTX + _nulls(("rlwe", "ct", "pack_key")) + DIGITS + [
            ({"ct": None, "basebit": 0}, NULL), ({"basebit": 9, "t": 0}, "basebit = 9 is outside 1 .. 8"),
            ({"t": 0, "basebit": 0}, "basebit = 0 is outside 1 .. 8")],
    "rs_pack_keygen_dev":
        NO_CTX + _nulls(("body", "lwe_key", "tlwe_key", "seed", "noise_seed")) + [({"noise_seed": MASK_SEED}, EQUAL)] +
        _deviations(DEV1, ("stdev",)) + DIGITS + _key_rows() + [
            ({"body": None, "noise_seed": MASK_SEED}, NULL), ({"noise_seed": MASK_SEED, "stdev": -1.0}, EQUAL),
            ({"stdev": NAN, "basebit": 0}, DEV1 % NAN), ({"t": 0, "lwe_key": _bad("lwe_key", 0)}, "t = 0 is below 1"),
            ({"lwe_key": _bad("lwe_key", -1), "tlwe_key": _bad("tlwe_key", -1)}, ("lwe_key", -1))],
    "rs_pack_expand_dev":
        NO_CTX + _nulls(("pack_key", "seed", "body")) + [({"t": 0}, "t = 0 is below 1")] + [({"body": None, "t": 0}, NULL)],
    "rs_phase_dev":
        NO_CTX + _nulls(("phase", "ct", "key")) +
        [({"dim": d}, "dim = %s is neither n = {n} nor k N = {N}" % d) for d in (0, -1, "n-1", "n+1", "2N")] +
        _key_rows(("lwe_key",), "key") + _key_rows(("tlwe_key",), "key") + [
            ({"ct": None, "dim": 0}, NULL), ({"dim": "n+1", "lwe_key": _bad("lwe_key", 0)}, "dim = n+1 is neither n = {n} nor k N = {N}")],
    "rs_audit_keys_dev":
        NO_CTX + _nulls(("report", "lwe_key", "tlwe_key")) + [({"bk": None, "ksk": None}, BOTH)] + _key_rows() + [
            ({"report": None, "bk": None, "ksk": None}, NULL), ({"bk": None, "ksk": None, "lwe_key": _bad("lwe_key", 0)}, BOTH),
            ({"lwe_key": _bad("lwe_key", -1), "tlwe_key": _bad("tlwe_key", 0)}, ("lwe_key", -1))],
    "rs_audit_compressed_keys_dev":
        NO_CTX + _nulls(("report", "seed", "lwe_key", "tlwe_key")) + [({"bk": None, "ksk": None}, BOTH)] + _key_rows() + [
            ({"seed": None, "bk": None, "ksk": None}, NULL), ({"bk": None, "ksk": None, "tlwe_key": _bad("tlwe_key", -1)}, BOTH),
            ({"lwe_key": _bad("lwe_key", 0), "tlwe_key": _bad("tlwe_key", 0)}, ("lwe_key", 0))],
    "rs_audit_pack_key_dev":
        NO_CTX + _nulls(("report", "key", "lwe_key", "tlwe_key")) + DIGITS + _key_rows() + [
            ({"key": None, "basebit": 9}, NULL), ({"basebit": 0, "lwe_key": _bad("lwe_key", 0)}, "basebit = 0 is outside 1 .. 8"),
            ({"t": T_MAX, "basebit": 1, "tlwe_key": _bad("tlwe_key", 0)}, "t basebit = 33 x 1 passes 32 bits"),
            ({"lwe_key": _bad("lwe_key", 0), "tlwe_key": _bad("tlwe_key", 0)}, ("lwe_key", 0))],
}


def _row_id(name, over):
    def show(v):
        return "%s@%d" % (v[1], v[2]) if isinstance(v, tuple) else "seed" if isinstance(v, bytes) else str(v)
    return name + "[" + ",".join("%s=%s" % (k, show(v)) for k, v in over.items()) + "]"


ROWS = [(name, over, text) for name, rows in TABLE.items() for over, text in rows]


class World:
    """the context, the valid arguments of every call, and what the valid secret-key calls wrote before any refusal"""

    def __init__(self, ks):
        import torch
        import redsec_amd
        import redsec_amd.backend as rb
        self.be = be = redsec_amd.Backend(redsec_amd.params("default128", n=ks.p.n), device=0)
        self.L, p = be.L, be.p
        self.n, self.N = n, N = p.n, p.N
        self.keys = {"lwe_key": np.ascontiguousarray(ks.lwe_key, np.int32), "tlwe_key": np.ascontiguousarray(ks.tlwe_key, np.int32)}
        rng = np.random.default_rng(23)

        def words(count, fill=None):
            if fill is None:
                return torch.zeros(count, dtype=torch.int32, device="cuda")
            return torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, count, dtype=np.int64).astype(np.int32)).cuda()
        rows_bk, samples = n * 2 * p.bk_l, N * p.ks_t * (1 << p.ks_basebit)
        bk, ksk = words(rows_bk * 2 * N + 4), words(samples * (n + 1))                 # + 4: the misaligned rows point 4 bytes in
        bk_body, ksk_body = words(rows_bk * N + 4), words(samples)
        pack_body, pack_key = words(n * T_MAX * N), words(n * T_MAX * 2 * N)
        ct, rlwe = words(2 * (N + 2), "random"), words(2 * 2 * N, "random")            # two items of the widest row of a row below
        pk, mu2N = words(2 * 2 * N, "random"), words(2 * N, "random")
        self.structs = {"rs_audit_keys_dev": rb.RsKeyAudit(), "rs_audit_compressed_keys_dev": rb.RsKeyAudit(),
                        "rs_audit_pack_key_dev": rb.RsPackKeyAudit()}
        key_args = dict(lwe_key=self.keys["lwe_key"], tlwe_key=self.keys["tlwe_key"])
        self.valid = {
            "rs_keygen_dev": dict(key_args, bk=bk, ksk=ksk, seed=MASK_SEED, bk_stdev=BK_STDEV, ks_stdev=KS_STDEV),
            "rs_keygen_compressed_dev": dict(key_args, bk=bk_body, ksk=ksk_body, seed=MASK_SEED, noise_seed=NOISE_SEED,
                                             bk_stdev=BK_STDEV, ks_stdev=KS_STDEV),
            "rs_expand_keys_dev": dict(bk=words(rows_bk * 2 * N + 4), ksk=words(samples * (n + 1)), seed=MASK_SEED, bk_body=bk_body,
                                       ksk_body=ksk_body),
            "rs_encrypt_seeded_dev": dict(body=words(2), ct=words(2 * (n + 1)), mu=words(2, "random"), B=1, lwe_key=self.keys["lwe_key"],
                                          seed=MASK_SEED, noise_seed=NOISE_SEED, first=5, stdev=STDEV),
            "rs_expand_ciphertexts_dev": dict(ct=words(2 * (n + 1)), seed=MASK_SEED, first=5, body=words(2, "random"), B=1, stream=None),
            "rs_pk_encrypt_dev": dict(ct=words(2 * (n + 1)), pk=words(4 * (n + 1), "random"), m=4, mu=words(2, "random"), base=None, B=1,
                                      seed=NOISE_SEED, first=5, stream=None),
            "rs_rlwe_pk_encrypt_dev": dict(rlwe=words(2 * 2 * N), pk=pk, mu=mu2N, count=1, seed=NOISE_SEED, first=5, stdev=STDEV,
                                           stream=None),
            "rs_rlwe_extract_dev": dict(u=words(2 * (N + 1)), rlwe=rlwe, count=1, stream=None),
            "rs_pack_dev": dict(rlwe=words(2 * N), ct=ct, count=1, pack_key=pack_key, basebit=BASEBIT, t=T, stream=None),
            "rs_pack_keygen_dev": dict(key_args, body=pack_body, seed=MASK_SEED, noise_seed=NOISE_SEED, basebit=BASEBIT, t=T, stdev=STDEV),
            "rs_pack_expand_dev": dict(pack_key=words(n * T_MAX * 2 * N), seed=MASK_SEED, body=pack_body, t=T, stream=None),
            "rs_phase_dev": dict(phase=words(2), ct=ct, B=1, key=self.keys["lwe_key"], dim=n),
            "rs_audit_keys_dev": dict(key_args, report=self.structs["rs_audit_keys_dev"], bk_noise=None, ksk_noise=None, bk=bk, ksk=ksk,
                                      bk_limit=1, ksk_limit=1),
            "rs_audit_compressed_keys_dev": dict(key_args, report=self.structs["rs_audit_compressed_keys_dev"], bk_noise=None,
                                                 ksk_noise=None, seed=MASK_SEED, bk=bk_body, ksk=ksk_body, bk_limit=1, ksk_limit=1),
            "rs_audit_pack_key_dev": dict(key_args, report=self.structs["rs_audit_pack_key_dev"], noise=None, key=pack_body, seed=MASK_SEED,
                                          basebit=BASEBIT, t=T, limit=1),
        }
        # the valid secret-key calls, once, generators before the audits of what they wrote
        self.before = {name: self.run_valid(name) for name in SECRET_OUTPUTS}
        assert self.before["rs_audit_keys_dev"][0][-2:] == (rows_bk * N, N * p.ks_t * ((1 << p.ks_basebit) - 1))
        assert self.before["rs_audit_pack_key_dev"][0][-1] == n * T * N

    def _resolve(self, name, arg, v):
        n, N = self.n, self.N
        if isinstance(v, tuple):                                       # _bad(key, at)
            key = self.keys[v[1]].copy()
            key[v[2]] = 2
            return key
        if isinstance(v, str) and v == "misaligned":
            return Off(self.valid[name][arg], 4)
        if isinstance(v, str):
            return {"n-1": n - 1, "n+1": n + 1, "2N": 2 * N}[v]
        return v

    def call(self, name, over=()):
        """the call with its valid arguments, `over` laid on top -> return code"""
        args = dict(self.valid[name])
        if name == "rs_phase_dev":                                     # its one key argument is `key`; the rows name which key they spoil
            for k in ("lwe_key", "tlwe_key"):
                if k in dict(over):
                    args["key"], args["dim"] = dict(over)[k], (self.n if k == "lwe_key" else self.N)
        ctx = self.be.h
        for arg, v in dict(over).items():
            if arg == "ctx":
                ctx = v
            elif arg in SIGNATURES[name]:
                args[arg] = v
        args = {k: self._resolve(name, k, v) for k, v in args.items()}
        self.alive = [a for a in args.values() if isinstance(a, np.ndarray)]      # host arrays outlive the call

        def conv(v):
            import torch
            if isinstance(v, torch.Tensor):
                return C.c_void_p(v.data_ptr())
            if isinstance(v, Off):
                return C.c_void_p(v.tensor.data_ptr() + v.by)
            if isinstance(v, np.ndarray):
                return v.ctypes.data_as(C.POINTER(C.c_int32))
            if isinstance(v, C.Structure):
                return C.byref(v)
            return v
        return getattr(self.L, name)(ctx, *[conv(args[a]) for a in SIGNATURES[name]])

    def run_valid(self, name):
        """one valid call -> what it wrote, as host values"""
        import torch
        outputs = [self.valid[name][arg] for arg in SECRET_OUTPUTS[name]]
        for v in outputs:                                              # the call has to write them, whatever they held
            if isinstance(v, C.Structure):
                C.memset(C.byref(v), 0xff, C.sizeof(v))
            else:
                v.fill_(-1)
        torch.cuda.synchronize()
        assert self.call(name) == 0, self.L.rs_last_error()
        torch.cuda.synchronize()
        out = []
        for v in outputs:
            out.append(tuple(getattr(v, f) for f, _ in v._fields_) if isinstance(v, C.Structure) else v.cpu().numpy().copy())
        return out

    def text(self, want, over):
        if isinstance(want, tuple):                                    # (key name, index); rs_phase_dev calls its one key `key`
            label, at = want
            size = self.N if (label == "tlwe_key" or (label == "key" and "tlwe_key" in over)) else self.n
            return "%s[%d] = 2 is not 0 or 1" % (label, at % size)
        return want.replace("n+1", str(self.n + 1)).replace("n-1", str(self.n - 1)).replace("2N", str(2 * self.N)) \
                   .replace("{n}", str(self.n)).replace("{N}", str(self.N))


@pytest.fixture(scope="module")
def world(toy_default):
    import torch
    w = World(toy_default[0])
    yield w
    w.be.close()
    torch.cuda.empty_cache()


def _same(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("name,over,want", ROWS, ids=[_row_id(name, over) for name, over, _ in ROWS])
def test_refusal(world, name, over, want):
    text = world.text(want, over)
    rc = world.call(name, over)
    got = world.L.rs_last_error().decode()
    print(name, over, "->", rc, got)
    assert rc == INVALID and got == text
    if name in SECRET_OUTPUTS:
        assert _same(world.run_valid(name), world.before[name]), name


def test_the_table_covers_every_key_material_and_client_call():
    import redsec_amd
    layer3 = [s for s in redsec_amd.ABI_SYMBOLS if s.endswith("_dev") and any(w in s for w in
              ("keygen", "expand", "encrypt", "rlwe", "pack", "phase", "audit"))]
    assert sorted(layer3) == sorted(TABLE) == sorted(SIGNATURES)
