"""numpy restatement of the sparse bootstraps (include/redsec_hip.h rs_bootstrap_sparse_dev; csrc/rs_sparse.h), shared by
tests/test_sparse_cpu.py and tests/test_gpu_sparse.py. Test infrastructure: the product never imports it."""
import numpy as np


def directed_b(N):
    """The b words of the directed trivial samples: 0, +-1, the ends of the torus, and every multiple k 2^32 / 2N of the mod-switch
    step +-1 for k in {0, 1, N-1, N, N+1, 2N-1} -- and, beyond that list, the rounding boundaries (k + 1/2) 2^32 / 2N -1, +0 of the
    same k, where the mod-switched word changes."""
    step = (1 << 32) // (2 * N)
    vals = [0, 1, -1, 2**31 - 1, -2**31]
    for k in (0, 1, N - 1, N, N + 1, 2 * N - 1):
        vals += [k * step - 1, k * step + 1, k * step + step // 2 - 1, k * step + step // 2]
    return np.array(vals, np.int64).astype(np.uint64).astype(np.uint32).view(np.int32)


def trivial_word(b, mu, N):
    """b word of bootstrap_mu((0, ..., 0, b)): +mu where b rounds to one of the first N of the 2N mod-switch steps, else -mu."""
    shift = 32 - (2 * N).bit_length() + 1
    barb = ((np.asarray(b, np.int32).view(np.uint32).astype(np.uint64) + (1 << (shift - 1))) >> shift) % (2 * N)
    mu = np.int64(np.int32(mu))
    return np.where(barb < N, mu, -mu).astype(np.uint64).astype(np.uint32).view(np.int32)


def _valid(live, B):
    live = np.asarray(live, np.int64)
    return (live >= 0) & (live < B)


def gather(inp, live):
    """rows[i] = inp[live[i]], the zero sample for an entry outside [0, B)"""
    inp = np.asarray(inp, np.int32)
    ok = _valid(live, inp.shape[0])
    rows = np.zeros((len(live), inp.shape[1]), np.int32)
    rows[ok] = inp[np.asarray(live, np.int64)[ok]]
    return rows


def fill(inp, mu, N):
    inp = np.asarray(inp, np.int32)
    out = np.zeros_like(inp)
    out[:, -1] = trivial_word(inp[:, -1], mu, N)
    return out


def scatter(out, boot, live):
    """out[live[i]] = boot[i] in list order (a repeated entry: the later row stays, as on one wave after another)"""
    out = np.array(out, np.int32)
    for i in np.flatnonzero(_valid(live, out.shape[0])):
        out[int(live[i])] = boot[i]
    return out


def trivial_rows(b, n):
    """the trivial samples (0, ..., 0, b) as int32 [len(b)][n + 1]"""
    x = np.zeros((len(b), n + 1), np.int32)
    x[:, n] = b
    return x
