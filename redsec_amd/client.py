"""Client side of the path: key generation, encryption, decryption (host, numpy).

Mirrors /root/reference/client/gen_secure_keyset.cpp (parameter sets + new_random_gate_bootstrapping_
secret_keyset), client/encrypt_image.cpp:65-85 (v = 2*pixel - 255 -> lweSymEncrypt(v/4096, 2^-15)) and
client/decrypt_image.cpp:37-63 (lweSymDecrypt(., 4096) -> signed -> argmax). None of this is on the
GPU hot path; it produces the inputs the hot path consumes (evaluation key, fresh ciphertexts) in
exactly the layouts include/redsec_hip.h documents.

Everything is vectorised; negacyclic products with the binary TRLWE key are done as two exact
float64 matrix products on 16-bit halves (sums stay below 2^26).
"""
import os

import numpy as np

MSG_SPACE = 4096          # client/decrypt_image.cpp:37 msg_space
SECALPHA = 2.0 ** -15     # client/encrypt_image.cpp:10

PARAM_SETS = {
    # name: (n, N, k, bk_l, bk_Bgbit, ks_t, ks_basebit, ks_stdev, bk_stdev)
    "default128": (630, 1024, 1, 3, 7, 8, 2, 2.0 ** -15, 2.0 ** -25),
    # client/gen_secure_keyset.cpp:70-91
    "redsec_small_v2": (350, 1024, 1, 10, 3, 9, 3, 2.0 ** -25, 2.0 ** -30),
    # client/gen_secure_keyset.cpp:47-68, 28-45, 9-26: the sets the reference defines beside the one it ships
    "redsec_small": (500, 1024, 1, 3, 10, 18, 1, 2.0 ** -25, 2.0 ** -36),
    "redsec_medium": (3072, 4096, 1, 3, 10, 18, 1, 2.0 ** -40, 2.0 ** -45),
    "redsec_large": (6144, 8192, 1, 3, 10, 18, 1, 2.0 ** -41, 2.0 ** -46),
}


def modswitch_to_torus32(mu, msize):
    """TFHE modSwitchToTorus32 (BinOps_enc.cpp:137,184,190; encrypt_image.cpp:77)."""
    interv = ((1 << 63) // int(msize)) * 2
    v = ((np.asarray(mu, dtype=np.int64).astype(object) * interv) >> 32) & 0xFFFFFFFF
    return _wrap32(np.asarray(v, dtype=object))


def _wrap32(x):
    x = np.asarray(x)
    if x.dtype == object:
        x = np.array([int(v) & 0xFFFFFFFF for v in x.ravel()], dtype=np.uint64).reshape(x.shape)
    return (x.astype(np.uint64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _gaussian32(rng, sigma, shape):
    """TFHE gaussian32 with message 0: dtot32(N(0, sigma))."""
    e = rng.normal(0.0, sigma, shape)
    frac = e - np.trunc(e)
    return (frac * 4294967296.0).astype(np.int64).astype(np.uint64).astype(np.uint32).view(np.int32)


def _uniform32(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.int32)


def _negacyclic_matrix(s):
    """T with (a * s)[j] = sum_m a[m] T[m][j] in Z[X]/(X^N+1), s binary."""
    N = len(s)
    idx = (np.arange(N)[None, :] - np.arange(N)[:, None])  # j - m
    T = s[idx % N].astype(np.float64)
    T[idx < 0] *= -1.0
    return T


def _mul_by_binary_poly(A, T):
    """Rows of A (int32 torus) times the binary key polynomial, exact mod 2^32."""
    Au = A.view(np.uint32).astype(np.uint64)
    hi = (Au >> 16).astype(np.float64)
    lo = (Au & 0xFFFF).astype(np.float64)
    ph = (hi @ T).astype(np.int64)
    pl = (lo @ T).astype(np.int64)
    return _wrap32(((ph << 16) + pl).astype(np.uint64))


def _round_phase(ph, msize):
    """client/decrypt_image.cpp:52-58: phases (int32) rounded to multiples of 1/msize, signed."""
    ph = np.asarray(ph, np.int32).view(np.uint32).astype(np.uint64)
    interv = 1 << (32 - int(np.log2(msize)))
    m = ((ph + interv // 2) // interv) % msize
    m = m.astype(np.int64)
    return np.where(m > msize // 2, m - msize, m)


class SecretKeySet:
    """TFheGateBootstrappingSecretKeySet: lwe_key, tlwe_key and the cloud (evaluation) key."""

    def __init__(self, name="redsec_small_v2", seed=0, n=None):
        (n0, N, k, l, Bgbit, t, basebit, ks_stdev, bk_stdev) = PARAM_SETS[name]
        self.name = name
        self.n = int(n) if n is not None else n0
        self.N, self.k, self.l, self.Bgbit, self.t, self.basebit = N, k, l, Bgbit, t, basebit
        self.W = self.n + 1
        rng = np.random.default_rng(seed)
        n = self.n
        self.lwe_key = rng.integers(0, 2, n).astype(np.int32)
        self.tlwe_key = rng.integers(0, 2, N).astype(np.int32)
        # --- bootstrapping key: [n][2l][2][N] ---
        rows = n * 2 * l
        A = _uniform32(rng, (rows, N))
        E = _gaussian32(rng, bk_stdev, (rows, N))
        Bp = _wrap32(E.view(np.uint32).astype(np.uint64) + _mul_by_binary_poly(A, _negacyclic_matrix(self.tlwe_key)).view(np.uint32))
        bk = np.empty((n, 2 * l, 2, N), np.int32)
        bk[:, :, 0, :] = A.reshape(n, 2 * l, N)
        bk[:, :, 1, :] = Bp.reshape(n, 2 * l, N)
        # tGswAddMuIntH: row c*l + j gets s_i * 2^(32-(j+1)Bgbit) on component c, coefficient 0
        for c in range(2):
            for j in range(l):
                h = np.uint32(1 << (32 - (j + 1) * Bgbit))
                cur = bk[:, c * l + j, c, 0].view(np.uint32)
                bk[:, c * l + j, c, 0] = (cur + self.lwe_key.astype(np.uint32) * h).view(np.int32)
        self.bk = np.ascontiguousarray(bk)
        # --- keyswitch key: [N][t][base][n+1], value 0 is the trivial zero sample ---
        base = 1 << basebit
        ksk = np.zeros((N, t, base, n + 1), np.int32)
        Ak = _uniform32(rng, (N, t, base - 1, n))
        Ek = _gaussian32(rng, ks_stdev, (N, t, base - 1))
        dot = (Ak.view(np.uint32).astype(np.uint64) * self.lwe_key.astype(np.uint64)).sum(axis=-1)
        v = np.arange(1, base, dtype=np.uint64)[None, None, :]
        shift = np.array([32 - (j + 1) * basebit for j in range(t)], dtype=np.uint64)[None, :, None]
        mess = (self.tlwe_key.astype(np.uint64)[:, None, None] * v) << shift
        ksk[:, :, 1:, :n] = Ak
        ksk[:, :, 1:, n] = _wrap32(mess + Ek.view(np.uint32).astype(np.uint64) + dot)
        self.ksk = np.ascontiguousarray(ksk)

    @classmethod
    def from_secret(cls, name, lwe_key, tlwe_key):
        """The secret keys alone (encrypt / decrypt / phase / classify), no evaluation key (bk = ksk = None): the client half of
        a key whose evaluation key was generated elsewhere (redsec_amd.keygen, on the device). The LWE dimension is len(lwe_key)."""
        (_, N, k, l, Bgbit, t, basebit, _, _) = PARAM_SETS[name]
        self = cls.__new__(cls)
        self.name = name
        self.lwe_key = np.ascontiguousarray(lwe_key, np.int32)
        self.tlwe_key = np.ascontiguousarray(tlwe_key, np.int32)
        assert self.tlwe_key.size == N, "tlwe_key must have N = %d words" % N
        self.n = int(self.lwe_key.size)
        self.N, self.k, self.l, self.Bgbit, self.t, self.basebit = N, k, l, Bgbit, t, basebit
        self.W = self.n + 1
        self.bk = self.ksk = None
        return self

    # lweSymEncrypt on a batch of torus32 messages -> int32 [B][n+1]
    def encrypt_torus(self, mu, alpha=SECALPHA, seed=1):
        mu = np.asarray(mu).astype(np.int64).ravel()
        rng = np.random.default_rng(seed)
        B = mu.size
        out = np.empty((B, self.W), np.int32)
        a = _uniform32(rng, (B, self.n))
        e = _gaussian32(rng, alpha, (B,))
        dot = (a.view(np.uint32).astype(np.uint64) * self.lwe_key.astype(np.uint64)).sum(axis=-1)
        out[:, :self.n] = a
        out[:, self.n] = _wrap32(mu.astype(np.uint64) + e.view(np.uint32).astype(np.uint64) + dot)
        return out

    def encrypt_bits(self, bits, seed=1):
        """bootsSymEncrypt: +-1/8."""
        e8 = 1 << 29
        return self.encrypt_torus(np.where(np.asarray(bits) != 0, e8, -e8), SECALPHA, seed)

    def encrypt_image(self, pixels, seed=1, preprocess="sign"):
        """client/encrypt_image.cpp:76-77: ptxt = 2*pixel - 255, message ptxt/4096. preprocess="relu": the
        ReLU nets' own input map pixel/100 - 1 (nets/mnist/relu1024x1/main.cpp:203), which the reference's
        client tool does not know about."""
        px = np.asarray(pixels, dtype=np.int64).ravel()
        v = (px // 100 - 1) if preprocess == "relu" else 2 * px - 255
        return self.encrypt_torus(v * (1 << 20), SECALPHA, seed)

    # seeded ciphertexts (include/redsec_hip.h rs_encrypt_seeded_dev): the same messages as the methods
    # above, each sample a body word beside a public mask seed. mask_seed defaults to a fresh os.urandom(32) per call (a (mask seed,
    # row) pair must never encrypt two messages); noise_seed (private) to another.
    def encrypt_torus_seeded(self, mu, alpha=SECALPHA, mask_seed=None, noise_seed=None, first=0):
        """lweSymEncrypt of the torus words mu [B] as seeded ciphertexts (keygen.encrypt_seeded) -> SeededCiphertexts."""
        from . import keygen
        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        noise_seed = os.urandom(32) if noise_seed is None else bytes(noise_seed)
        body = keygen.encrypt_seeded(self.lwe_key, mu, mask_seed, noise_seed, first, alpha)
        return SeededCiphertexts(self.name, self.n, mask_seed, first, body)

    def encrypt_bits_seeded(self, bits, mask_seed=None, noise_seed=None, first=0):
        """bootsSymEncrypt (+-1/8) as seeded ciphertexts."""
        e8 = 1 << 29
        return self.encrypt_torus_seeded(np.where(np.asarray(bits) != 0, e8, -e8), SECALPHA, mask_seed, noise_seed, first)

    def encrypt_image_seeded(self, pixels, preprocess="sign", mask_seed=None, noise_seed=None, first=0):
        """encrypt_image's messages (2 pixel - 255, or the ReLU nets' pixel / 100 - 1, over 4096) as seeded ciphertexts."""
        px = np.asarray(pixels, dtype=np.int64).ravel()
        v = (px // 100 - 1) if preprocess == "relu" else 2 * px - 255
        return self.encrypt_torus_seeded(v * (1 << 20), SECALPHA, mask_seed, noise_seed, first)

    def public_key(self, m=None, mask_seed=None, noise_seed=None, first=0, alpha=SECALPHA):
        """A Regev public key for this secret (include/redsec_hip.h rs_pk_encrypt_dev): m seeded encryptions
        of zero (default keygen.pk_rows(n) = 32 (n + 1) + 256) -> SeededCiphertexts, written and read as an RSC1 file like any other
        seeded batch. Anyone holding it encrypts with Backend.pk_encrypt / keygen.pk_encrypt; only this secret decrypts."""
        from . import keygen
        m = keygen.pk_rows(self.n) if m is None else int(m)
        return self.encrypt_torus_seeded(np.zeros(m, np.int64), alpha, mask_seed, noise_seed, first)

    def rlwe_public_key(self, mask_seed=None, noise_seed=None, stdev=None):
        """The compact RLWE public key of this secret's ring key (include/redsec_hip.h rs_rlwe_pk_encrypt_dev; INTEGRATION.md section
        17): (a, b = a*S + e) with a the domain-10 stream of the public mask seed -> RlwePublicKey (32 bytes + 4N bytes), written and
        read as an RSP1 file. stdev defaults to the set's bk_stdev; on redsec_medium / redsec_large, where that truncates to zero in a
        32-bit torus, it must be given (ValueError otherwise: a noise-free key publishes S). Anyone holding the key encrypts with
        Backend.rlwe_pk_encrypt / keygen.rlwe_pk_encrypt; the server unpacks with the keyswitching key it has loaded."""
        from . import keygen
        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        noise_seed = os.urandom(32) if noise_seed is None else bytes(noise_seed)
        return RlwePublicKey(self.name, mask_seed, keygen.rlwe_public_key(self.name, self.tlwe_key, mask_seed, noise_seed, stdev))

    def packing_key(self, basebit=None, t=None, mask_seed=None, noise_seed=None, stdev=None, backend=None):
        """The packing key from this secret's LWE key to its ring key (include/redsec_hip.h rs_pack_dev)
        -> PackingKey (32 bytes + 4 n t N bytes), written and read as an RSK1 file. basebit, t default to keygen.pack_default(name),
        stdev to the set's bk_stdev (ValueError where that truncates to zero: pass one). A server holding the key packs results with
        Backend.pack; only this secret decrypts them (packed_phase, decrypt_packed_bits, decrypt_packed_ints). With backend= (a
        redsec_amd.Backend of this set and n) the bodies are generated on the device (rs_pack_keygen_dev):
        the same words, the same PackingKey, the same rules for the seeds and the deviation."""
        from . import keygen
        d = keygen.pack_default(self.name)
        basebit, t = keygen._check_digits(d[0] if basebit is None else basebit, d[1] if t is None else t)
        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        noise_seed = os.urandom(32) if noise_seed is None else bytes(noise_seed)
        if backend is None:
            body = keygen.pack_key(self.name, self.lwe_key, self.tlwe_key, mask_seed, noise_seed, basebit, t, stdev)
        else:
            self._check_backend(backend)
            keygen._check_seeds(mask_seed, noise_seed)
            stdev = keygen.rlwe_default_stdev(self.name) if stdev is None else float(stdev)
            body = backend.pack_keygen(self.lwe_key, self.tlwe_key, mask_seed, noise_seed, basebit, t, stdev).cpu().numpy()
        return PackingKey(self.name, self.n, basebit, t, mask_seed, body)

    def _check_backend(self, backend):
        from . import keygen
        if keygen.set_name(backend.p) != self.name or backend.p.n != self.n:
            raise ValueError("the secret is of %s with n = %d, the context of %s with n = %d"
                             % (self.name, self.n, keygen.set_name(backend.p), backend.p.n))

    def audit_packing_key(self, key, backend, limit=None):
        """Exact noise audit of the PackingKey `key` under this secret on the device (rs_audit_pack_key_dev): the bodies are uploaded
        and the masks regenerated from the key's seed, nothing is expanded. limit defaults to keygen.pack_noise_limit of the set's
        default deviation (ValueError where that vanishes: pass one) -> the dict of Backend.audit_packing_key; a key made for this
        secret with a deviation within the limit has over == 0."""
        import torch
        self._check_backend(backend)
        if key.name != self.name or key.n != self.n:
            raise ValueError("the packing key is of %s with n = %d, the secret of %s with n = %d" % (key.name, key.n, self.name, self.n))
        body = torch.from_numpy(key.body).to("cuda:%d" % backend.device)
        return backend.audit_packing_key(self.lwe_key, self.tlwe_key, body, key.basebit, key.t, mask_seed=key.mask_seed, limit=limit)

    def packed_phase(self, rlwe, count, backend=None):
        """Phases of the first `count` slots of packed ciphertexts [R][2][N] under the ring key (slot rN + c is coefficient c of
        ciphertext r) -> int32 [count]; with backend= rlwe is an int32 CUDA tensor and the phase is taken on the device
        (rs_rlwe_extract_dev + rs_phase_dev with dim = N)."""
        from . import keygen
        count = int(count)
        if backend is not None:
            return backend.phase(backend.rlwe_extract(rlwe, count), self.tlwe_key).cpu().numpy()
        ph = keygen.rlwe_phase(rlwe, self.tlwe_key).ravel()
        assert 0 <= count <= ph.size, "count exceeds the slots of the ciphertexts"
        return ph[:count]

    def decrypt_packed_bits(self, rlwe, count, backend=None):
        return (self.packed_phase(rlwe, count, backend) > 0).astype(np.int64)

    def decrypt_packed_ints(self, rlwe, count, msize=MSG_SPACE, backend=None):
        """decrypt_ints of the first `count` slots of packed ciphertexts."""
        return _round_phase(self.packed_phase(rlwe, count, backend), msize)

    def phase(self, ct, backend=None, ring=False):
        """Phases b - sum_k a_k s_k of ct [B][n+1]; with backend= (a redsec_amd.Backend) ct is an int32 CUDA tensor and the phase is
        taken on the device (rs_phase_dev). ring=True: ct holds [B][N+1] samples under the ring key read as an LWE key of dimension
        N (the output of bootstrap_wo_ks, of rlwe_extract, or of a re-keying under this secret's RLWE public key; rs_phase_dev with
        dim = N)."""
        key = self.tlwe_key if ring else self.lwe_key
        if backend is not None:
            return backend.phase(ct.reshape(-1, key.size + 1), key).cpu().numpy()
        ct = np.asarray(ct, np.int32).reshape(-1, key.size + 1)
        dot = (ct[:, :key.size].view(np.uint32).astype(np.uint64) * key.astype(np.uint64)).sum(axis=-1)
        return _wrap32(ct[:, key.size].view(np.uint32).astype(np.uint64) - dot)

    def decrypt_bits(self, ct, backend=None, ring=False):
        return (self.phase(ct, backend, ring) > 0).astype(np.int64)

    def decrypt_ints(self, ct, msize=MSG_SPACE, backend=None, ring=False):
        """client/decrypt_image.cpp:52-58: round the phase to multiples of 1/msize, signed."""
        return _round_phase(self.phase(ct, backend, ring), msize)

    # re-keying (include/redsec_hip.h rs_rekey_dev): keys under which a server turns samples under THIS
    # secret's LWE key into samples under a recipient's key
    def _rekey_digits(self, dst_name, basebit, t):
        from . import keygen
        d = keygen.rekey_default(dst_name)
        return keygen._check_digits(d[0] if basebit is None else basebit, d[1] if t is None else t)

    def _rekey_mu(self, basebit, t, backend, run, alternate=False):
        """run(mu) with mu = keygen.rekey_messages of this secret (alternate: the odd rows negated, keygen.rekey_alternate): a host
        array, or with a backend an int32 CUDA tensor that is zeroed before this returns (it holds the source secret's bits)."""
        from . import keygen
        mu = keygen.rekey_messages(self.lwe_key, basebit, t)
        if alternate:
            mu = keygen.rekey_alternate(mu)
        if backend is None:
            return run(mu)
        import torch
        dev = torch.from_numpy(mu).to("cuda:%d" % backend.device)
        try:
            return run(dev)
        finally:
            dev.zero_()
            torch.cuda.synchronize(backend.device)

    def rekey_to(self, other, basebit=None, t=None, mask_seed=None, noise_seed=None, stdev=None, backend=None):
        """The re-keying key from this secret's LWE key to the LWE key of `other` (a SecretKeySet of any set and n), made by the
        owner of both secrets -> RekeyKey of form "seeded": n_src t seeded encryptions (rows 0 .. n_src t - 1 of the public mask seed,
        domains 7 / 8) of keygen.rekey_messages under other's LWE key, 32 + 4 n_src t bytes. basebit, t default to
        keygen.rekey_default(other.name), stdev to other's ks_stdev (ValueError where that truncates to zero: pass one). Equal seeds
        are refused. With backend= (a redsec_amd.Backend of other's set and n) the bodies are made on the device
        (rs_encrypt_seeded_dev): the same words."""
        from . import keygen
        basebit, t = self._rekey_digits(other.name, basebit, t)
        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        noise_seed = os.urandom(32) if noise_seed is None else bytes(noise_seed)
        keygen._check_seeds(mask_seed, noise_seed)
        stdev = keygen.rekey_row_stdev(other.name) if stdev is None else float(stdev)
        if backend is None:
            body = self._rekey_mu(basebit, t, None, lambda mu: keygen.encrypt_seeded(other.lwe_key, mu, mask_seed, noise_seed, 0, stdev))
        else:
            other._check_backend(backend)
            body = self._rekey_mu(basebit, t, backend, lambda mu: backend.encrypt_seeded(other.lwe_key, mu, mask_seed, noise_seed, 0,
                                                                                         stdev).cpu().numpy())
        return RekeyKey(self.name, other.name, self.n, other.n, basebit, t, mask_seed=mask_seed, body=body)

    def rekey_for(self, rlwe_pk, basebit=None, t=None, rand_seed=None, stdev=None, backend=None):
        """The re-keying key from this secret's LWE key to the RING key behind the recipient's RlwePublicKey, made without any secret of
        the recipient -> RekeyKey of form "rlwe": ceil(n_src t / N) ciphertexts of keygen.rekey_messages, the odd rows negated
        (keygen.rekey_alternate: the rows of one ciphertext share its selector and noise polynomials, and alternating signs keep
        their common part from adding up under the unsigned digits), under rlwe_pk (rows 0 .. of the PRIVATE rand seed, domains
        12 / 13), 8 N bytes each; n_dst = N, and the recipient decrypts what arrives with phase(., ring=True). basebit, t default to keygen.rekey_default(rlwe_pk.name), stdev to the set's bk_stdev (ValueError where that
        truncates to zero: pass one). A rand seed equal to the key's public mask seed is refused. With backend= (a redsec_amd.Backend
        of the recipient's set) the ciphertexts are made on the device (rs_rlwe_pk_encrypt_dev): the same words."""
        from . import keygen
        basebit, t = self._rekey_digits(rlwe_pk.name, basebit, t)
        rand_seed = os.urandom(32) if rand_seed is None else bytes(rand_seed)
        keygen._check_seeds(rlwe_pk.mask_seed, rand_seed)
        stdev = keygen.rlwe_default_stdev(rlwe_pk.name) if stdev is None else float(stdev)
        if backend is None:
            rlwe = self._rekey_mu(basebit, t, None, lambda mu: keygen.rlwe_pk_encrypt(rlwe_pk.expand(), mu, rand_seed, 0, stdev=stdev), True)
        else:
            rlwe = self._rekey_mu(basebit, t, backend, lambda mu: backend.rlwe_pk_encrypt(rlwe_pk, mu, rand_seed, 0, stdev).cpu().numpy(), True)
        return RekeyKey(self.name, rlwe_pk.name, self.n, rlwe_pk.N, basebit, t, rlwe=rlwe)

    # ring re-keying (include/redsec_hip.h rs_ring_rekey_dev): keys under which a server turns PACKED
    # ciphertexts under THIS secret's ring key into packed ciphertexts under a recipient's ring key of the same N
    def _ring_rekey_digits(self, dst_name, form, basebit, t):
        from . import keygen
        if PARAM_SETS[dst_name][1] != self.N:
            raise ValueError("source and destination rings differ: N = %d (%s) and %d (%s); crossing between rings is out of scope"
                             % (self.N, self.name, PARAM_SETS[dst_name][1], dst_name))
        d = keygen.ring_rekey_default(dst_name, form)
        return keygen._check_ring_digits(d[0] if basebit is None else basebit, d[1] if t is None else t)

    def ring_rekey_to(self, other, basebit=None, t=None, mask_seed=None, noise_seed=None, stdev=None):
        """The ring re-keying key from this secret's ring key to the ring key of `other` (a SecretKeySet of the same N), made by the
        owner of both secrets -> RingRekeyKey of form "seeded": t + 1 seeded ring samples (rows 0 .. t of the public mask seed,
        domains 16 / 17) of keygen.ring_rekey_messages under other's ring key, 32 + 4 N (t + 1) bytes. basebit, t default to
        keygen.ring_rekey_default(other.name, "seeded"), stdev to other's bk_stdev (ValueError where that truncates to zero: pass
        one). Equal seeds are refused. The t + 1 products run on the host: there is no device generator."""
        from . import keygen
        basebit, t = self._ring_rekey_digits(other.name, "seeded", basebit, t)
        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        noise_seed = os.urandom(32) if noise_seed is None else bytes(noise_seed)
        keygen._check_seeds(mask_seed, noise_seed)
        stdev = keygen.rlwe_default_stdev(other.name) if stdev is None else float(stdev)
        body = keygen.ring_rekey_key(self.tlwe_key, other.tlwe_key, mask_seed, noise_seed, basebit, t, stdev)
        return RingRekeyKey(self.name, other.name, basebit, t, mask_seed=mask_seed, body=body)

    def ring_rekey_for(self, rlwe_pk, basebit=None, t=None, rand_seed=None, stdev=None, backend=None):
        """The ring re-keying key from this secret's ring key to the ring key behind the recipient's RlwePublicKey, made without any
        secret of the recipient -> RingRekeyKey of form "rlwe": the t + 1 ciphertexts of keygen.ring_rekey_messages under rlwe_pk
        (rows 0 .. t of the PRIVATE rand seed, domains 12 / 13), 8 N bytes each, already the layout rs_ring_rekey_dev takes.
        basebit, t default to keygen.ring_rekey_default(rlwe_pk.name, "rlwe"), stdev to the set's bk_stdev (ValueError where that
        truncates to zero: pass one). A rand seed equal to the key's public mask seed is refused. With backend= (a
        redsec_amd.Backend of the recipient's set) the ciphertexts are made on the device (rs_rlwe_pk_encrypt_dev): the same words.
        The message rows hold this secret's ring key; they are zeroed on the host and on the device before this returns."""
        from . import keygen
        basebit, t = self._ring_rekey_digits(rlwe_pk.name, "rlwe", basebit, t)
        rand_seed = os.urandom(32) if rand_seed is None else bytes(rand_seed)
        keygen._check_seeds(rlwe_pk.mask_seed, rand_seed)
        stdev = keygen.rlwe_default_stdev(rlwe_pk.name) if stdev is None else float(stdev)
        mu = keygen.ring_rekey_messages(self.tlwe_key, basebit, t)
        try:
            if backend is None:
                rlwe = keygen.rlwe_pk_encrypt(rlwe_pk.expand(), mu.ravel(), rand_seed, 0, stdev=stdev)
            else:
                import torch
                dev = torch.from_numpy(mu.ravel()).to("cuda:%d" % backend.device)
                try:
                    rlwe = backend.rlwe_pk_encrypt(rlwe_pk, dev, rand_seed, 0, stdev).cpu().numpy()
                finally:
                    dev.zero_()
                    torch.cuda.synchronize(backend.device)
        finally:
            mu[...] = 0
        return RingRekeyKey(self.name, rlwe_pk.name, basebit, t, rlwe=rlwe)

    # encrypted selection (include/redsec_hip.h rs_ring_cmux_dev / rs_ring_lookup_dev): the bits of an
    # index as RGSW samples under THIS secret's ring key, under which a server picks one packed ciphertext without learning which
    def ring_selector(self, index, depth, basebit=None, l=None, mask_seed=None, noise_seed=None, stdev=None):
        """The selector of table entry `index` for a lookup of `depth` levels (depth = 1: the bit of one CMUX) -> RingSelector: depth
        seeded RGSW samples of 2l rows each (rows k 2l + j of the public mask seed, domains 18 / 19), sample k of bit k of the index,
        32 + 4 N 2l depth bytes. basebit, l default to keygen.ring_cmux_default(name, depth), stdev to the set's bk_stdev (ValueError
        where that truncates to zero: pass one). Equal seeds and an index at or past 2^depth are refused. The 2l depth products run
        on the host: there is no device generator."""
        from . import keygen
        index, depth = int(index), int(depth)
        if not 1 <= depth <= keygen.RING_LOOKUP_MAX_DEPTH:
            raise ValueError("depth = %d is outside 1 .. %d" % (depth, keygen.RING_LOOKUP_MAX_DEPTH))
        if not 0 <= index < 1 << depth:
            raise ValueError("index = %d is outside 0 .. 2^%d - 1" % (index, depth))
        if basebit is None or l is None:
            d = keygen.ring_cmux_default(self.name, depth)
            basebit, l = d[0] if basebit is None else basebit, d[1] if l is None else l
        basebit, l = keygen._check_cmux_digits(basebit, l)
        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        noise_seed = os.urandom(32) if noise_seed is None else bytes(noise_seed)
        keygen._check_seeds(mask_seed, noise_seed)
        stdev = keygen.rlwe_default_stdev(self.name) if stdev is None else float(stdev)
        bits = [(index >> k) & 1 for k in range(depth)]
        body = keygen.ring_selector_rows(bits, self.tlwe_key, mask_seed, noise_seed, basebit, l, stdev)
        return RingSelector(self.name, self.N, depth, basebit, l, mask_seed, body)

    # circuit bootstrapping (include/redsec_hip.h rs_ring_selector_dev / rs_circuit_bootstrap_dev): the key
    # under which a server turns bits it computed under THIS secret's LWE key into selectors under this secret's ring key
    def selector_key(self, ks_basebit=None, ks_t=None, mask_seed=None, noise_seed=None, stdev=None, depth=1):
        """The selector key from this secret's LWE key to its ring key -> SelectorKey: 2 (n + 1) ks_t seeded ring samples (rows (f (n+1)
        + i) ks_t + q of the public mask seed, domains 20 / 21), 32 + 4 N 2 (n + 1) ks_t bytes. ks_basebit, ks_t default to
        keygen.circuit_bootstrap_default(name, depth) (ValueError where no shape works: default-128), stdev to the deviation of
        selector rows (keygen.ring_selector_default_stdev). Equal seeds are refused. The products run on the host: there is no
        device generator. The key encrypts multiples of S and of s S under S: the circular assumption of the bootstrapping key."""
        from . import keygen
        if ks_basebit is None or ks_t is None:
            d = keygen.circuit_bootstrap_default(self.name, depth)
            ks_basebit, ks_t = d[2] if ks_basebit is None else ks_basebit, d[3] if ks_t is None else ks_t
        ks_basebit, ks_t = keygen._check_selector_digits(ks_basebit, ks_t)
        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        noise_seed = os.urandom(32) if noise_seed is None else bytes(noise_seed)
        keygen._check_seeds(mask_seed, noise_seed)
        stdev = keygen.ring_selector_default_stdev(self.name) if stdev is None else float(stdev)
        body = keygen.selector_key(self.lwe_key, self.tlwe_key, mask_seed, noise_seed, ks_basebit, ks_t, stdev)
        return SelectorKey(self.name, len(self.lwe_key), ks_basebit, ks_t, mask_seed, body)

    def classify(self, logits_ct, backend=None):
        """client/decrypt_image.cpp:61-62 argmax."""
        return int(np.argmax(self.decrypt_ints(logits_ct, backend=backend)))


# ---- TFHE v1.1 file formats (the reference's client/*.cpp and nets/*/*/main.cpp exchange these files) -------------
# Same layout as redsec_amd/host/tfhe_shim.cpp writes and reads (see the comment there; [TFHE-recalled]).
TFHE_UID = dict(lwe_sample=42, lwe_key=43, tlwe_key=45, tgsw_sample=47, ks_key=200, bk_key=201)


def _section(title, props):
    body = "".join("%s: %s\n" % (k, v) for k, v in sorted(props.items()))
    return ("-----BEGIN %s-----\n%s-----END %s-----\n" % (title, body, title)).encode()


def _read_section(f, want):
    head = f.readline().decode().rstrip("\n")
    assert head == "-----BEGIN %s-----" % want, (head, want)
    props = {}
    while True:
        line = f.readline().decode().rstrip("\n")
        if line.startswith("-----END "):
            return props
        k, v = line.split(": ", 1)
        props[k] = v


def write_tfhe_keyset(f, sk, secret, ks_stdev, bk_stdev, max_stdev=0.012467):
    """export_tfheGateBootstrapping{Secret,Cloud}KeySet_toFile for a SecretKeySet (binary file object)."""
    i32 = lambda v: np.int32(v).tobytes()
    f.write(_section("GATEBOOTSPARAMS", dict(ks_t=sk.t, ks_basebit=sk.basebit)))
    f.write(_section("LWEPARAMS", dict(n=sk.n, alpha_min=repr(float(ks_stdev)), alpha_max=repr(float(max_stdev)))))
    f.write(_section("TLWEPARAMS", dict(N=sk.N, k=sk.k, alpha_min=repr(float(bk_stdev)), alpha_max=repr(float(max_stdev)))))
    f.write(_section("TGSWPARAMS", dict(l=sk.l, Bgbit=sk.Bgbit)))
    f.write(i32(TFHE_UID["bk_key"]))
    f.write(_section("LWEKSPARAMS", dict(n=sk.k * sk.N, t=sk.t, basebit=sk.basebit)))
    f.write(i32(TFHE_UID["ks_key"]) + np.float64(ks_stdev ** 2).tobytes())
    f.write(np.ascontiguousarray(sk.ksk, np.int32).tobytes())
    for i in range(sk.n):
        f.write(i32(TFHE_UID["tgsw_sample"]) + np.float64(bk_stdev ** 2).tobytes())
        f.write(np.ascontiguousarray(sk.bk[i], np.int32).tobytes())
    if secret:
        f.write(i32(TFHE_UID["lwe_key"]) + np.ascontiguousarray(sk.lwe_key, np.int32).tobytes())
        f.write(i32(TFHE_UID["tlwe_key"]) + np.ascontiguousarray(sk.tlwe_key, np.int32).tobytes())


def read_tfhe_keyset(f, secret):
    """-> dict(params..., bk [n][2l][2][N], ksk [N][t][base][n+1], and for secret files lwe_key, tlwe_key, uids seen)."""
    g = _read_section(f, "GATEBOOTSPARAMS"); lw = _read_section(f, "LWEPARAMS")
    tl = _read_section(f, "TLWEPARAMS"); tg = _read_section(f, "TGSWPARAMS")
    n, N, k, l, Bgbit = int(lw["n"]), int(tl["N"]), int(tl["k"]), int(tg["l"]), int(tg["Bgbit"])
    t, basebit = int(g["ks_t"]), int(g["ks_basebit"])
    rd = lambda count: np.frombuffer(f.read(4 * count), np.int32)
    uids = [int(rd(1)[0])]
    ks = _read_section(f, "LWEKSPARAMS")
    assert (int(ks["n"]), int(ks["t"]), int(ks["basebit"])) == (k * N, t, basebit)
    uids.append(int(rd(1)[0])); f.read(8)
    ksk = rd(k * N * t * (1 << basebit) * (n + 1)).reshape(k * N, t, 1 << basebit, n + 1)
    bk = np.empty((n, (k + 1) * l, k + 1, N), np.int32)
    for i in range(n):
        uids.append(int(rd(1)[0])); f.read(8)
        bk[i] = rd((k + 1) * l * (k + 1) * N).reshape((k + 1) * l, k + 1, N)
    out = dict(n=n, N=N, k=k, l=l, Bgbit=Bgbit, t=t, basebit=basebit, ks_stdev=float(lw["alpha_min"]), bk_stdev=float(tl["alpha_min"]),
               bk=bk, ksk=ksk)
    if secret:
        uids.append(int(rd(1)[0])); out["lwe_key"] = rd(n).copy()
        uids.append(int(rd(1)[0])); out["tlwe_key"] = rd(k * N).copy()
    assert f.read(1) == b"", "trailing bytes in key file"
    out["uids"] = uids
    return out


# The backend's own key-file header ("RSK1" full cloud key, "RSS1" secret key, "RSZ1" compressed cloud key, "RSR1" re-keying key, "RSX1" ring re-keying key, "RSG1" selector; redsec_amd/host/
# tfhe_shim.cpp ParamHeader): magic, int32 n, N, k, l, Bgbit, ks_t, ks_basebit, then double lwe alpha min / max, tlwe alpha min / max.
_RS_HEADER = np.dtype([("magic", "<u4"), ("n", "<i4"), ("N", "<i4"), ("k", "<i4"), ("l", "<i4"), ("Bgbit", "<i4"), ("ks_t", "<i4"),
                       ("ks_basebit", "<i4"), ("lwe_alpha_min", "<f8"), ("lwe_alpha_max", "<f8"), ("tlwe_alpha_min", "<f8"),
                       ("tlwe_alpha_max", "<f8")])
RS_MAGIC = {"RSS1": 0x31535352, "RSK1": 0x314B5352, "RSZ1": 0x315A5352, "RSC1": 0x31435352, "RSP1": 0x31505352,
            "RSR1": 0x31525352, "RSX1": 0x31585352, "RSG1": 0x31475352, "RSB1": 0x31425352}


def write_compressed_cloud_key(f, ck, max_stdev=0.012467):
    """A compressed cloud key file (binary file object): the RSK1 header with magic RSZ1, the 32-byte mask seed, then the raw
    bodies bk_body [n][2l][N] and ksk_body [N][t][2^basebit] (int32). ck: redsec_amd.keygen.CompressedKey."""
    (_, N, k, l, Bgbit, t, basebit, ks_stdev, bk_stdev) = PARAM_SETS[ck.name]
    h = np.zeros((), _RS_HEADER)
    h["magic"], h["n"], h["N"], h["k"], h["l"], h["Bgbit"], h["ks_t"], h["ks_basebit"] = RS_MAGIC["RSZ1"], ck.n, N, k, l, Bgbit, t, basebit
    h["lwe_alpha_min"], h["lwe_alpha_max"], h["tlwe_alpha_min"], h["tlwe_alpha_max"] = ks_stdev, max_stdev, bk_stdev, max_stdev
    host = ck.numpy()
    f.write(h.tobytes())
    f.write(host.mask_seed)
    f.write(np.ascontiguousarray(host.bk_body, np.int32).tobytes())
    f.write(np.ascontiguousarray(host.ksk_body, np.int32).tobytes())


def read_compressed_cloud_key(f):
    """-> redsec_amd.keygen.CompressedKey of an RSZ1 file (numpy bodies)."""
    from . import keygen
    h = np.frombuffer(f.read(_RS_HEADER.itemsize), _RS_HEADER)[0]
    assert int(h["magic"]) == RS_MAGIC["RSZ1"], "not a compressed cloud key file"
    shape = (int(h["N"]), int(h["k"]), int(h["l"]), int(h["Bgbit"]), int(h["ks_t"]), int(h["ks_basebit"]))
    name = next((nm for nm, v in PARAM_SETS.items() if v[1:7] == shape), None)
    assert name is not None, "no parameter set with N, k, l, Bgbit, t, basebit = %s" % (shape,)
    n, N, l, t, basebit = int(h["n"]), shape[0], shape[2], shape[4], shape[5]
    seed = f.read(32)
    rd = lambda count: np.frombuffer(f.read(4 * count), np.int32)
    bk_body = rd(n * 2 * l * N).reshape(n, 2 * l, N)
    ksk_body = rd(N * t * (1 << basebit)).reshape(N, t, 1 << basebit)
    assert f.read(1) == b"", "trailing bytes in compressed key file"
    return keygen.CompressedKey(name, n, seed, bk_body, ksk_body)


class SeededCiphertexts:
    """Seeded LWE ciphertexts (include/redsec_hip.h): the set name, the LWE dimension n, the public 32-byte
    mask seed, the row `first` of the first sample and the bodies (int32 [B], numpy or a CUDA tensor). Sample i has the domain-7
    mask words of row first + i. nbytes: what travels (seed, first, bodies)."""

    def __init__(self, name, n, mask_seed, first, body):
        self.name, self.n, self.mask_seed, self.first = name, int(n), bytes(mask_seed), int(first)
        assert len(self.mask_seed) == 32, "mask seed must be 32 bytes"
        self.body = body
        if not 0 <= self.first <= (1 << 64) - len(self):
            raise ValueError("first + B passes 2^64")

    def __len__(self):
        return int(self.body.numel() if hasattr(self.body, "numel") else np.size(self.body))

    @property
    def nbytes(self):
        return 32 + 8 + 4 * len(self)

    def numpy(self):
        """The same ciphertexts with host bodies."""
        body = self.body if isinstance(self.body, np.ndarray) else self.body.cpu().numpy()
        return SeededCiphertexts(self.name, self.n, self.mask_seed, self.first, np.asarray(body, np.int32).ravel())

    def expand(self):
        """The full samples, expanded on the host (keygen.expand_ciphertexts) -> int32 [B][n+1]."""
        from . import keygen
        return keygen.expand_ciphertexts(self.mask_seed, self.numpy().body, self.n, self.first)


def write_seeded_ciphertexts(f, sc, max_stdev=0.012467):
    """An RSC1 file (binary file object): the RSK1 header with magic RSC1, the 32-byte mask seed, uint64 first, then the int32
    bodies to the end of the file (their count is the file's length). sc: SeededCiphertexts."""
    (_, N, k, l, Bgbit, t, basebit, ks_stdev, bk_stdev) = PARAM_SETS[sc.name]
    h = np.zeros((), _RS_HEADER)
    h["magic"], h["n"], h["N"], h["k"], h["l"], h["Bgbit"], h["ks_t"], h["ks_basebit"] = RS_MAGIC["RSC1"], sc.n, N, k, l, Bgbit, t, basebit
    h["lwe_alpha_min"], h["lwe_alpha_max"], h["tlwe_alpha_min"], h["tlwe_alpha_max"] = ks_stdev, max_stdev, bk_stdev, max_stdev
    host = sc.numpy()
    f.write(h.tobytes())
    f.write(host.mask_seed)
    f.write(np.uint64(host.first).tobytes())
    f.write(np.ascontiguousarray(host.body, np.int32).tobytes())


def read_seeded_ciphertexts(f, n=None):
    """-> SeededCiphertexts of an RSC1 file (numpy bodies). Raises ValueError for a truncated file, another magic, a parameter
    shape no set has, an n outside 1 .. the set's n, or an n other than the given one."""
    raw = f.read(_RS_HEADER.itemsize)
    if len(raw) < 4 or np.frombuffer(raw[:4], "<u4")[0] != RS_MAGIC["RSC1"]:
        raise ValueError("not a seeded ciphertext (RSC1) file")
    if len(raw) < _RS_HEADER.itemsize:
        raise ValueError("truncated seeded ciphertext file: short header")
    h = np.frombuffer(raw, _RS_HEADER)[0]
    shape = (int(h["N"]), int(h["k"]), int(h["l"]), int(h["Bgbit"]), int(h["ks_t"]), int(h["ks_basebit"]))
    name = next((nm for nm, v in PARAM_SETS.items() if v[1:7] == shape), None)
    if name is None:
        raise ValueError("no parameter set with N, k, l, Bgbit, t, basebit = %s" % (shape,))
    hn = int(h["n"])
    if not 0 < hn <= PARAM_SETS[name][0] or (n is not None and hn != int(n)):
        raise ValueError("seeded ciphertexts of n = %d do not fit %s%s" % (hn, name, "" if n is None else " with n = %d" % int(n)))
    seed, first = f.read(32), f.read(8)
    if len(seed) < 32 or len(first) < 8:
        raise ValueError("truncated seeded ciphertext file: short seed or first row")
    rest = f.read()
    if len(rest) % 4:
        raise ValueError("truncated seeded ciphertext file: %d bytes of bodies is not a whole number of words" % len(rest))
    return SeededCiphertexts(name, hn, seed, int(np.frombuffer(first, "<u8")[0]), np.frombuffer(rest, np.int32).copy())


class RlwePublicKey:
    """A compact RLWE public key (include/redsec_hip.h): the set name, the public 32-byte mask seed and the
    body b = a*S + e (int32 [N], numpy). nbytes: what travels (seed + body)."""

    def __init__(self, name, mask_seed, body):
        self.name, self.mask_seed = name, bytes(mask_seed)
        assert len(self.mask_seed) == 32, "mask seed must be 32 bytes"
        self.body = np.ascontiguousarray(body, np.int32).ravel()
        self.N = PARAM_SETS[name][1]
        assert self.body.size == self.N, "body must have N = %d words" % self.N

    @property
    def nbytes(self):
        return 32 + 4 * self.N

    def expand(self):
        """(a, b): the domain-10 mask of the seed, then the body -> int32 [2][N], what rs_rlwe_pk_encrypt_dev takes."""
        from . import keygen
        return np.stack([keygen.rlwe_pk_mask(self.mask_seed, self.N), self.body])


def write_rlwe_public_key(f, pk, max_stdev=0.012467):
    """An RSP1 file (binary file object): the RSK1 header with magic RSP1, the 32-byte mask seed, then the N int32 body words.
    pk: RlwePublicKey."""
    (n, N, k, l, Bgbit, t, basebit, ks_stdev, bk_stdev) = PARAM_SETS[pk.name]
    h = np.zeros((), _RS_HEADER)
    h["magic"], h["n"], h["N"], h["k"], h["l"], h["Bgbit"], h["ks_t"], h["ks_basebit"] = RS_MAGIC["RSP1"], n, N, k, l, Bgbit, t, basebit
    h["lwe_alpha_min"], h["lwe_alpha_max"], h["tlwe_alpha_min"], h["tlwe_alpha_max"] = ks_stdev, max_stdev, bk_stdev, max_stdev
    f.write(h.tobytes())
    f.write(pk.mask_seed)
    f.write(pk.body.tobytes())


def read_rlwe_public_key(f):
    """-> RlwePublicKey of an RSP1 file. Raises ValueError for a truncated file, another magic, a parameter shape no set has, or a
    body that is not exactly N words."""
    raw = f.read(_RS_HEADER.itemsize)
    if len(raw) < 4 or np.frombuffer(raw[:4], "<u4")[0] != RS_MAGIC["RSP1"]:
        raise ValueError("not an RLWE public key (RSP1) file")
    if len(raw) < _RS_HEADER.itemsize:
        raise ValueError("truncated RLWE public key file: short header")
    h = np.frombuffer(raw, _RS_HEADER)[0]
    shape = (int(h["N"]), int(h["k"]), int(h["l"]), int(h["Bgbit"]), int(h["ks_t"]), int(h["ks_basebit"]))
    name = next((nm for nm, v in PARAM_SETS.items() if v[1:7] == shape), None)
    if name is None:
        raise ValueError("no parameter set with N, k, l, Bgbit, t, basebit = %s" % (shape,))
    seed, rest = f.read(32), f.read()
    if len(seed) < 32 or len(rest) != 4 * shape[0]:
        raise ValueError("truncated RLWE public key file: %d bytes after the header, expected 32 + %d" % (len(seed) + len(rest), 4 * shape[0]))
    return RlwePublicKey(name, seed, np.frombuffer(rest, np.int32).copy())


class PackingKey:
    """A packing key (include/redsec_hip.h rs_pack_dev): the set name, the LWE dimension n, the digit
    shape (basebit, t), the public 32-byte mask seed and the bodies b_ij (int32 [n][t][N], numpy). nbytes: what travels (seed +
    bodies); the masks are the domain-14 streams of the seed."""

    def __init__(self, name, n, basebit, t, mask_seed, body):
        self.name, self.n, self.basebit, self.t, self.mask_seed = name, int(n), int(basebit), int(t), bytes(mask_seed)
        assert len(self.mask_seed) == 32, "mask seed must be 32 bytes"
        assert 1 <= self.basebit <= 8 and self.t >= 1 and self.t * self.basebit <= 32, "basebit in 1 .. 8, t >= 1, t basebit <= 32"
        self.N = PARAM_SETS[name][1]
        self.body = np.ascontiguousarray(body, np.int32).reshape(-1)
        assert self.body.size == self.n * self.t * self.N, "body must have n t N = %d words" % (self.n * self.t * self.N)
        self.body = self.body.reshape(self.n, self.t, self.N)

    @property
    def nbytes(self):
        return 32 + 4 * self.n * self.t * self.N

    def expand(self):
        """K[i][j] = (a_ij, b_ij): the domain-14 masks of the seed beside the bodies -> int32 [n][t][2][N], what rs_pack_dev takes."""
        from . import keygen
        out = np.empty((self.n, self.t, 2, self.N), np.int32)
        out[:, :, 0] = keygen.pack_key_mask(self.mask_seed, self.N, np.arange(self.n * self.t)).reshape(self.n, self.t, self.N)
        out[:, :, 1] = self.body
        return out


def write_packing_key(f, key, max_stdev=0.012467):
    """A packing key file (binary file object): the RS header with magic RSK1 -- its n the key's LWE dimension, its ks_t and
    ks_basebit the set's -- then int32 basebit, int32 t of the packing digits, the 32-byte mask seed and the n t N int32 body words.
    key: PackingKey."""
    (_, N, k, l, Bgbit, t, basebit, ks_stdev, bk_stdev) = PARAM_SETS[key.name]
    h = np.zeros((), _RS_HEADER)
    h["magic"], h["n"], h["N"], h["k"], h["l"], h["Bgbit"], h["ks_t"], h["ks_basebit"] = RS_MAGIC["RSK1"], key.n, N, k, l, Bgbit, t, basebit
    h["lwe_alpha_min"], h["lwe_alpha_max"], h["tlwe_alpha_min"], h["tlwe_alpha_max"] = ks_stdev, max_stdev, bk_stdev, max_stdev
    f.write(h.tobytes())
    f.write(np.array([key.basebit, key.t], "<i4").tobytes())
    f.write(key.mask_seed)
    f.write(key.body.tobytes())


def read_packing_key(f):
    """-> PackingKey of a packing key file. Raises ValueError for a truncated file, another magic, a parameter shape no set has, an n
    below 1, digits outside basebit 1 .. 8, t >= 1, t basebit <= 32, or a body that is not exactly n t N words."""
    raw = f.read(_RS_HEADER.itemsize)
    if len(raw) < 4 or np.frombuffer(raw[:4], "<u4")[0] != RS_MAGIC["RSK1"]:
        raise ValueError("not a packing key (RSK1) file")
    if len(raw) < _RS_HEADER.itemsize:
        raise ValueError("truncated packing key file: short header")
    h = np.frombuffer(raw, _RS_HEADER)[0]
    shape = (int(h["N"]), int(h["k"]), int(h["l"]), int(h["Bgbit"]), int(h["ks_t"]), int(h["ks_basebit"]))
    name = next((nm for nm, v in PARAM_SETS.items() if v[1:7] == shape), None)
    if name is None:
        raise ValueError("no parameter set with N, k, l, Bgbit, t, basebit = %s" % (shape,))
    n = int(h["n"])
    digits, seed, rest = f.read(8), f.read(32), f.read()
    if len(digits) < 8 or len(seed) < 32:
        raise ValueError("truncated packing key file: %d bytes after the header" % (len(digits) + len(seed)))
    basebit, t = (int(v) for v in np.frombuffer(digits, "<i4"))
    if n < 1 or not (1 <= basebit <= 8 and t >= 1 and t * basebit <= 32):
        raise ValueError("packing key file with n = %d, basebit = %d, t = %d" % (n, basebit, t))
    if len(rest) != 4 * n * t * shape[0]:
        raise ValueError("truncated packing key file: %d body bytes, expected %d" % (len(rest), 4 * n * t * shape[0]))
    return PackingKey(name, n, basebit, t, seed, np.frombuffer(rest, np.int32).copy())


class RekeyKey:
    """A re-keying key (include/redsec_hip.h rs_rekey_dev) from the LWE key of a secret of set src_name
    and dimension n_src to a recipient's key of dimension n_dst, with the digit shape (basebit, t). Row i t + j encrypts
    s_i 2^(32-(j+1) basebit). One of two payloads:
      form "seeded"  the public 32-byte mask seed and the n_src t body words (int32, numpy) of seeded ciphertexts, rows 0 ..
                     n_src t - 1 of domains 7 / 8, under the recipient's LWE key of set dst_name and dimension n_dst
      form "rlwe"    ceil(n_src t / N) RLWE ciphertexts int32 [R][2][N] under the recipient's compact RLWE public key; n_dst = N and
                     the destination is the recipient's ring key read as an LWE key. Slot r carries row r, negated when r is odd
                     (keygen.rekey_alternate) and negated back on expansion
    nbytes: what travels (seed + bodies, or the ciphertexts)."""

    def __init__(self, src_name, dst_name, n_src, n_dst, basebit, t, mask_seed=None, body=None, rlwe=None):
        self.src_name, self.dst_name, self.n_src, self.n_dst = src_name, dst_name, int(n_src), int(n_dst)
        self.basebit, self.t = int(basebit), int(t)
        assert src_name in PARAM_SETS and dst_name in PARAM_SETS, "unknown parameter set"
        assert 1 <= self.basebit <= 8 and self.t >= 1 and self.t * self.basebit <= 32, "basebit in 1 .. 8, t >= 1, t basebit <= 32"
        assert self.n_src >= 1 and self.n_dst >= 1, "dimensions must be positive"
        assert (rlwe is None) != (body is None), "one payload: seeded bodies or RLWE ciphertexts"
        self.rows = self.n_src * self.t
        if rlwe is None:
            self.form, self.mask_seed, self.rlwe = "seeded", bytes(mask_seed), None
            assert len(self.mask_seed) == 32, "mask seed must be 32 bytes"
            self.body = np.ascontiguousarray(body, np.int32).reshape(-1)
            assert self.body.size == self.rows, "body must have n_src t = %d words" % self.rows
        else:
            N = PARAM_SETS[dst_name][1]
            assert self.n_dst == N, "a key under an RLWE public key has n_dst = N = %d" % N
            self.form, self.mask_seed, self.body = "rlwe", None, None
            self.rlwe = np.ascontiguousarray(rlwe, np.int32).reshape(-1)
            assert self.rlwe.size == -(-self.rows // N) * 2 * N, "rlwe must hold [ceil(n_src t / N)][2][N] words"
            self.rlwe = self.rlwe.reshape(-1, 2, N)

    @property
    def nbytes(self):
        return 32 + 4 * self.rows if self.form == "seeded" else 4 * self.rlwe.size

    def expand(self):
        """K[i][j] = row i t + j: the domain-7 masks of the seed beside the bodies, or the rows extracted from the RLWE ciphertexts
        -> int32 [n_src][t][n_dst+1], what rs_rekey_dev takes (numpy path; Backend.upload_rekey_key does the same on the device)."""
        from . import keygen
        if self.form == "seeded":
            rows = keygen.expand_ciphertexts(self.mask_seed, self.body, self.n_dst, 0)
        else:
            rows = keygen.rekey_alternate(keygen.rlwe_extract(self.rlwe, self.rows))
        return rows.reshape(self.n_src, self.t, self.n_dst + 1)


def _rs_header(magic, name, n, max_stdev=0.012467):
    (_, N, k, l, Bgbit, t, basebit, ks_stdev, bk_stdev) = PARAM_SETS[name]
    h = np.zeros((), _RS_HEADER)
    h["magic"], h["n"], h["N"], h["k"], h["l"], h["Bgbit"], h["ks_t"], h["ks_basebit"] = RS_MAGIC[magic], n, N, k, l, Bgbit, t, basebit
    h["lwe_alpha_min"], h["lwe_alpha_max"], h["tlwe_alpha_min"], h["tlwe_alpha_max"] = ks_stdev, max_stdev, bk_stdev, max_stdev
    return h.tobytes()


def write_rekey_key(f, key):
    """A re-keying key file (binary file object): the RS header with magic RSR1 for the destination (its n the key's n_dst), the
    same header for the source (its n the key's n_src), int32 basebit, int32 t, int32 form (0 seeded, 1 rlwe), then the 32-byte
    mask seed and the n_src t int32 body words, or the ceil(n_src t / N) 2 N int32 words of the RLWE ciphertexts. key: RekeyKey."""
    f.write(_rs_header("RSR1", key.dst_name, key.n_dst))
    f.write(_rs_header("RSR1", key.src_name, key.n_src))
    f.write(np.array([key.basebit, key.t, 0 if key.form == "seeded" else 1], "<i4").tobytes())
    if key.form == "seeded":
        f.write(key.mask_seed)
        f.write(key.body.tobytes())
    else:
        f.write(key.rlwe.tobytes())


def read_rekey_key(f):
    """-> RekeyKey of a re-keying key file. Raises ValueError for a truncated file, another magic, a parameter shape no set has, a
    dimension below 1, digits outside basebit 1 .. 8, t >= 1, t basebit <= 32, an unknown form, an RLWE form whose n_dst is not the
    destination's N, or a payload that is not exactly the words the header promises."""
    names, dims = [], []
    for what in ("destination", "source"):
        raw = f.read(_RS_HEADER.itemsize)
        if len(raw) < 4 or np.frombuffer(raw[:4], "<u4")[0] != RS_MAGIC["RSR1"]:
            raise ValueError("not a re-keying key (RSR1) file: %s header" % what)
        if len(raw) < _RS_HEADER.itemsize:
            raise ValueError("truncated re-keying key file: short %s header" % what)
        h = np.frombuffer(raw, _RS_HEADER)[0]
        shape = (int(h["N"]), int(h["k"]), int(h["l"]), int(h["Bgbit"]), int(h["ks_t"]), int(h["ks_basebit"]))
        name = next((nm for nm, v in PARAM_SETS.items() if v[1:7] == shape), None)
        if name is None:
            raise ValueError("no parameter set with N, k, l, Bgbit, t, basebit = %s (%s)" % (shape, what))
        names.append(name)
        dims.append(int(h["n"]))
    digits, rest = f.read(12), f.read()
    if len(digits) < 12:
        raise ValueError("truncated re-keying key file: %d bytes after the headers" % len(digits))
    basebit, t, form = (int(v) for v in np.frombuffer(digits, "<i4"))
    (dst, src), (n_dst, n_src) = names, dims
    if n_src < 1 or n_dst < 1 or not (1 <= basebit <= 8 and t >= 1 and t * basebit <= 32) or form not in (0, 1):
        raise ValueError("re-keying key file with n_src = %d, n_dst = %d, basebit = %d, t = %d, form = %d" % (n_src, n_dst, basebit, t, form))
    N = PARAM_SETS[dst][1]
    if form == 1 and n_dst != N:
        raise ValueError("re-keying key file of the RLWE form with n_dst = %d, not N = %d" % (n_dst, N))
    want = 32 + 4 * n_src * t if form == 0 else 4 * -(-(n_src * t) // N) * 2 * N
    if len(rest) != want:
        raise ValueError("truncated re-keying key file: %d payload bytes, expected %d" % (len(rest), want))
    if form == 0:
        return RekeyKey(src, dst, n_src, n_dst, basebit, t, mask_seed=rest[:32], body=np.frombuffer(rest[32:], np.int32).copy())
    return RekeyKey(src, dst, n_src, n_dst, basebit, t, rlwe=np.frombuffer(rest, np.int32).copy())


class RingRekeyKey:
    """A ring re-keying key (include/redsec_hip.h rs_ring_rekey_dev) from the ring key of a secret of set
    src_name to a recipient's ring key of set dst_name (the same N), with the digit shape (basebit, t), t basebit <= 31. Row j < t
    encrypts 2^(31-(j+1) basebit) S, row t the constant row. One of two payloads:
      form "seeded"  the public 32-byte mask seed and the bodies int32 [t+1][N] of ring samples, rows 0 .. t of domains 16 / 17,
                     under the recipient's ring key
      form "rlwe"    the t + 1 ciphertexts int32 [t+1][2][N] of the message rows under the recipient's compact RLWE public key:
                     already the layout the call takes
    nbytes: what travels (seed + bodies, or the ciphertexts)."""

    def __init__(self, src_name, dst_name, basebit, t, mask_seed=None, body=None, rlwe=None):
        self.src_name, self.dst_name, self.basebit, self.t = src_name, dst_name, int(basebit), int(t)
        assert src_name in PARAM_SETS and dst_name in PARAM_SETS, "unknown parameter set"
        self.N = PARAM_SETS[dst_name][1]
        assert PARAM_SETS[src_name][1] == self.N, "source and destination share the ring degree N"
        assert 1 <= self.basebit <= 8 and self.t >= 1 and self.t * self.basebit <= 31, "basebit in 1 .. 8, t >= 1, t basebit <= 31"
        assert (rlwe is None) != (body is None), "one payload: seeded bodies or RLWE ciphertexts"
        self.rows = self.t + 1
        if rlwe is None:
            self.form, self.mask_seed, self.rlwe = "seeded", bytes(mask_seed), None
            assert len(self.mask_seed) == 32, "mask seed must be 32 bytes"
            self.body = np.ascontiguousarray(body, np.int32).reshape(-1)
            assert self.body.size == self.rows * self.N, "body must have (t + 1) N = %d words" % (self.rows * self.N)
            self.body = self.body.reshape(self.rows, self.N)
        else:
            self.form, self.mask_seed, self.body = "rlwe", None, None
            self.rlwe = np.ascontiguousarray(rlwe, np.int32).reshape(-1)
            assert self.rlwe.size == self.rows * 2 * self.N, "rlwe must hold [t+1][2][N] words"
            self.rlwe = self.rlwe.reshape(self.rows, 2, self.N)

    @property
    def nbytes(self):
        return 32 + 4 * self.body.size if self.form == "seeded" else 4 * self.rlwe.size

    def expand(self):
        """K[j] = row j: the domain-16 masks of the seed beside the bodies, or the ciphertexts as they are -> int32 [t+1][2][N], what
        rs_ring_rekey_dev takes."""
        from . import keygen
        return keygen.ring_rekey_expand(self.mask_seed, self.body) if self.form == "seeded" else self.rlwe.copy()


def write_ring_rekey_key(f, key):
    """A ring re-keying key file (binary file object): the RS header with magic RSX1 for the destination, the same header for the
    source, int32 basebit, int32 t, int32 form (0 seeded, 1 rlwe), then the 32-byte mask seed and the (t + 1) N int32 body words, or
    the (t + 1) 2 N int32 words of the RLWE ciphertexts. key: RingRekeyKey."""
    f.write(_rs_header("RSX1", key.dst_name, PARAM_SETS[key.dst_name][0]))
    f.write(_rs_header("RSX1", key.src_name, PARAM_SETS[key.src_name][0]))
    f.write(np.array([key.basebit, key.t, 0 if key.form == "seeded" else 1], "<i4").tobytes())
    if key.form == "seeded":
        f.write(key.mask_seed)
        f.write(key.body.tobytes())
    else:
        f.write(key.rlwe.tobytes())


def read_ring_rekey_key(f):
    """-> RingRekeyKey of a ring re-keying key file. Raises ValueError for a truncated file, another magic, a parameter shape no set
    has, rings of different degree, digits outside basebit 1 .. 8, t >= 1, t basebit <= 31, an unknown form, or a payload that is not
    exactly the words the header promises."""
    names = []
    for what in ("destination", "source"):
        raw = f.read(_RS_HEADER.itemsize)
        if len(raw) < 4 or np.frombuffer(raw[:4], "<u4")[0] != RS_MAGIC["RSX1"]:
            raise ValueError("not a ring re-keying key (RSX1) file: %s header" % what)
        if len(raw) < _RS_HEADER.itemsize:
            raise ValueError("truncated ring re-keying key file: short %s header" % what)
        h = np.frombuffer(raw, _RS_HEADER)[0]
        shape = (int(h["N"]), int(h["k"]), int(h["l"]), int(h["Bgbit"]), int(h["ks_t"]), int(h["ks_basebit"]))
        name = next((nm for nm, v in PARAM_SETS.items() if v[1:7] == shape), None)
        if name is None:
            raise ValueError("no parameter set with N, k, l, Bgbit, t, basebit = %s (%s)" % (shape, what))
        names.append(name)
    digits, rest = f.read(12), f.read()
    if len(digits) < 12:
        raise ValueError("truncated ring re-keying key file: %d bytes after the headers" % len(digits))
    basebit, t, form = (int(v) for v in np.frombuffer(digits, "<i4"))
    dst, src = names
    N = PARAM_SETS[dst][1]
    if PARAM_SETS[src][1] != N:
        raise ValueError("ring re-keying key file between rings of N = %d and N = %d" % (PARAM_SETS[src][1], N))
    if not (1 <= basebit <= 8 and t >= 1 and t * basebit <= 31) or form not in (0, 1):
        raise ValueError("ring re-keying key file with basebit = %d, t = %d, form = %d" % (basebit, t, form))
    want = 32 + 4 * (t + 1) * N if form == 0 else 4 * (t + 1) * 2 * N
    if len(rest) != want:
        raise ValueError("truncated ring re-keying key file: %d payload bytes, expected %d" % (len(rest), want))
    if form == 0:
        return RingRekeyKey(src, dst, basebit, t, mask_seed=rest[:32], body=np.frombuffer(rest[32:], np.int32).copy())
    return RingRekeyKey(src, dst, basebit, t, rlwe=np.frombuffer(rest, np.int32).copy())


class RingSelector:
    """The encrypted index of a lookup (include/redsec_hip.h rs_ring_lookup_dev; depth = 1: the bit of rs_ring_cmux_dev;
    INTEGRATION.md section 23) under the ring key of a secret of set `name`: depth seeded RGSW samples of the digit shape
    (basebit, l), l basebit <= 31, sample k of bit k of the index. What travels is the public 32-byte mask seed and the bodies int32
    [depth][2l][N] of the rows k 2l + j of domains 18 / 19; nbytes = 32 + 4 N 2l depth."""

    def __init__(self, name, N, depth, basebit, l, mask_seed, body):
        self.name, self.N, self.depth, self.basebit, self.l = name, int(N), int(depth), int(basebit), int(l)
        assert name in PARAM_SETS and PARAM_SETS[name][1] == self.N, "unknown parameter set or another ring"
        assert 1 <= self.basebit <= 8 and self.l >= 1 and self.l * self.basebit <= 31, "basebit in 1 .. 8, l >= 1, l basebit <= 31"
        assert 1 <= self.depth <= 30, "depth in 1 .. 30"
        self.mask_seed = bytes(mask_seed)
        assert len(self.mask_seed) == 32, "mask seed must be 32 bytes"
        self.body = np.ascontiguousarray(body, np.int32).reshape(-1)
        assert self.body.size == self.depth * 2 * self.l * self.N, "body must have depth 2l N = %d words" % (self.depth * 2 * self.l * self.N)
        self.body = self.body.reshape(self.depth, 2 * self.l, self.N)

    @property
    def nbytes(self):
        return 32 + 4 * self.body.size

    def expand(self):
        """The domain-18 masks of the seed beside the bodies -> int32 [depth][2l][2][N], what rs_ring_lookup_dev takes (and
        rs_ring_cmux_dev for depth = 1)."""
        from . import keygen
        return keygen.ring_selector_expand(self.mask_seed, self.body)


def write_ring_selector(f, sel):
    """A selector file (binary file object): the RS header with magic RSG1 for the set, int32 depth, int32 basebit, int32 l, then the
    32-byte mask seed and the depth 2l N int32 body words. sel: RingSelector."""
    f.write(_rs_header("RSG1", sel.name, PARAM_SETS[sel.name][0]))
    f.write(np.array([sel.depth, sel.basebit, sel.l], "<i4").tobytes())
    f.write(sel.mask_seed)
    f.write(sel.body.tobytes())


def read_ring_selector(f):
    """-> RingSelector of a selector file. Raises ValueError for a truncated file, another magic, a parameter shape no set has, a
    depth outside 1 .. 30, digits outside basebit 1 .. 8, l >= 1, l basebit <= 31, or a payload that is not exactly the words the
    header promises."""
    raw = f.read(_RS_HEADER.itemsize)
    if len(raw) < 4 or np.frombuffer(raw[:4], "<u4")[0] != RS_MAGIC["RSG1"]:
        raise ValueError("not a selector (RSG1) file")
    if len(raw) < _RS_HEADER.itemsize:
        raise ValueError("truncated selector file: short header")
    h = np.frombuffer(raw, _RS_HEADER)[0]
    shape = (int(h["N"]), int(h["k"]), int(h["l"]), int(h["Bgbit"]), int(h["ks_t"]), int(h["ks_basebit"]))
    name = next((nm for nm, v in PARAM_SETS.items() if v[1:7] == shape), None)
    if name is None:
        raise ValueError("no parameter set with N, k, l, Bgbit, t, basebit = %s" % (shape,))
    digits, rest = f.read(12), f.read()
    if len(digits) < 12:
        raise ValueError("truncated selector file: %d bytes after the header" % len(digits))
    depth, basebit, l = (int(v) for v in np.frombuffer(digits, "<i4"))
    if not (1 <= depth <= 30 and 1 <= basebit <= 8 and l >= 1 and l * basebit <= 31):
        raise ValueError("selector file with depth = %d, basebit = %d, l = %d" % (depth, basebit, l))
    N = PARAM_SETS[name][1]
    want = 32 + 4 * depth * 2 * l * N
    if len(rest) != want:
        raise ValueError("truncated selector file: %d payload bytes, expected %d" % (len(rest), want))
    return RingSelector(name, N, depth, basebit, l, rest[:32], np.frombuffer(rest[32:], np.int32).copy())


class SelectorKey:
    """A selector key (include/redsec_hip.h rs_ring_selector_dev) of a secret of set `name` with LWE
    dimension n: 2 (n + 1) ks_t seeded ring samples of the digit shape (ks_basebit, ks_t), ks_t ks_basebit <= 32. What travels is the
    public 32-byte mask seed and the bodies int32 [2][n+1][ks_t][N] of the rows of domains 20 / 21; nbytes = 32 + 4 N 2 (n + 1) ks_t."""

    def __init__(self, name, n, ks_basebit, ks_t, mask_seed, body):
        self.name, self.n, self.ks_basebit, self.ks_t = name, int(n), int(ks_basebit), int(ks_t)
        assert name in PARAM_SETS, "unknown parameter set"
        self.N = PARAM_SETS[name][1]
        assert 1 <= self.n <= 65536, "n in 1 .. 65536"
        assert 1 <= self.ks_basebit <= 8 and self.ks_t >= 1 and self.ks_t * self.ks_basebit <= 32, "ks_basebit in 1 .. 8, ks_t >= 1, ks_t ks_basebit <= 32"
        self.mask_seed = bytes(mask_seed)
        assert len(self.mask_seed) == 32, "mask seed must be 32 bytes"
        self.body = np.ascontiguousarray(body, np.int32).reshape(-1)
        want = 2 * (self.n + 1) * self.ks_t * self.N
        assert self.body.size == want, "body must have 2 (n + 1) ks_t N = %d words" % want
        self.body = self.body.reshape(2, self.n + 1, self.ks_t, self.N)

    @property
    def nbytes(self):
        return 32 + 4 * self.body.size

    def expand(self):
        """The domain-20 masks of the seed beside the bodies -> int32 [2][n+1][ks_t][2][N], what rs_ring_selector_dev takes."""
        from . import keygen
        return keygen.selector_key_expand(self.mask_seed, self.body)


def write_selector_key(f, key):
    """A selector key file (binary file object): the RS header with magic RSB1 for the set (its n the key's n), int32 ks_basebit,
    int32 ks_t, then the 32-byte mask seed and the 2 (n + 1) ks_t N int32 body words. key: SelectorKey."""
    f.write(_rs_header("RSB1", key.name, key.n))
    f.write(np.array([key.ks_basebit, key.ks_t], "<i4").tobytes())
    f.write(key.mask_seed)
    f.write(key.body.tobytes())


def read_selector_key(f):
    """-> SelectorKey of a selector key file. Raises ValueError for a truncated file, another magic, a parameter shape no set has, an
    n outside 1 .. 65536, digits outside ks_basebit 1 .. 8, ks_t >= 1, ks_t ks_basebit <= 32, or a payload that is not exactly the
    words the header promises."""
    raw = f.read(_RS_HEADER.itemsize)
    if len(raw) < 4 or np.frombuffer(raw[:4], "<u4")[0] != RS_MAGIC["RSB1"]:
        raise ValueError("not a selector key (RSB1) file")
    if len(raw) < _RS_HEADER.itemsize:
        raise ValueError("truncated selector key file: short header")
    h = np.frombuffer(raw, _RS_HEADER)[0]
    shape = (int(h["N"]), int(h["k"]), int(h["l"]), int(h["Bgbit"]), int(h["ks_t"]), int(h["ks_basebit"]))
    name = next((nm for nm, v in PARAM_SETS.items() if v[1:7] == shape), None)
    if name is None:
        raise ValueError("no parameter set with N, k, l, Bgbit, t, basebit = %s" % (shape,))
    n = int(h["n"])
    digits, rest = f.read(8), f.read()
    if len(digits) < 8:
        raise ValueError("truncated selector key file: %d bytes after the header" % len(digits))
    ks_basebit, ks_t = (int(v) for v in np.frombuffer(digits, "<i4"))
    if not (1 <= n <= 65536 and 1 <= ks_basebit <= 8 and ks_t >= 1 and ks_t * ks_basebit <= 32):
        raise ValueError("selector key file with n = %d, ks_basebit = %d, ks_t = %d" % (n, ks_basebit, ks_t))
    want = 32 + 4 * 2 * (n + 1) * ks_t * PARAM_SETS[name][1]
    if len(rest) != want:
        raise ValueError("truncated selector key file: %d payload bytes, expected %d" % (len(rest), want))
    return SelectorKey(name, n, ks_basebit, ks_t, rest[:32], np.frombuffer(rest[32:], np.int32).copy())


def write_ciphertexts(f, ct):
    """export_gate_bootstrapping_ciphertext_toFile per row of ct [B][n+1]: uid 42, a[n], b, double variance."""
    ct = np.ascontiguousarray(ct, np.int32)
    for row in ct:
        f.write(np.int32(TFHE_UID["lwe_sample"]).tobytes() + row.tobytes() + np.float64(0.0).tobytes())


def read_ciphertexts(f, n, count):
    rec = 4 + 4 * (n + 1) + 8
    raw = f.read(rec * count)
    assert len(raw) == rec * count
    out = np.empty((count, n + 1), np.int32)
    for i in range(count):
        assert np.frombuffer(raw[i * rec:i * rec + 4], np.int32)[0] == TFHE_UID["lwe_sample"]
        out[i] = np.frombuffer(raw[i * rec + 4:i * rec + 4 + 4 * (n + 1)], np.int32)
    return out


def synthetic_key_words(seed, count, first=0, chunk=1 << 22):
    """Words [first, first + count) of the synthetic key rs_load_synthetic_keys(seed) generates on the device (csrc/rs_ntt.h,
    synthetic_key_word: the high half of splitmix64(seed + k)); the keyswitch key uses seed ^ 0x6b73."""
    out = np.empty(int(count), np.int32)
    seed = np.uint64(int(seed) & (2**64 - 1))
    with np.errstate(over="ignore"):
        for lo in range(0, int(count), chunk):
            hi = min(int(count), lo + chunk)
            k = np.arange(first + lo + 1, first + hi + 1, dtype=np.uint64)
            z = seed + k * np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z ^= z >> np.uint64(31)
            out[lo:hi] = (z >> np.uint64(32)).astype(np.uint32).view(np.int32)
    return out
