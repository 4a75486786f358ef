"""Integer arithmetic on bit-sliced ciphertext batches at two bootstraps per bit.

A batch of B encrypted integers of `bits` bits is an int32 tensor [bits][B][W], LSB first, every bit an LWE sample encoding
+-1/8 (what the gates produce and consume). A full adder is two bootstraps of linear combinations of three inputs:
sum = XOR3(a, b, carry), carry' = MAJ3(a, b, carry); with the first input negated the same pair subtracts: difference =
XOR3(a, b, borrow), borrow' = MAJ3N(a, b, borrow) = majority(!a, b, borrow). Each function below issues exactly `bits` calls of
Backend.gate_rows, one per bit, each carrying both gates of all B lanes (2 B rows in two groups). The operands and every result
row live in one arena tensor, addressed through index tables that are built once, on the arena's device; the carry-in of bit 0 is
the index -1, the constant FALSE. Nothing here computes on ciphertext words: torch only lays rows out.

(The C++ layer mirror's BinOps::add keeps the reference's five-gate sequence: it is the drop-in and is tested against it.)

select, maximum, equal and multiply go through compiled circuits instead (redsec_amd/circuit.py): the
generator's netlist is compiled once per (function, bit count) and bound once per backend, and a call is one Backend.circuit_run.

lookup, lookup_rows and evaluate leave the gates for the ring pipeline (INTEGRATION.md sections 24, 26 and 28): the encrypted bits
become selectors by circuit bootstrapping, lookup returns a whole table row under the ring key (lookup_rows: one row per index, R
indices in one call), and evaluate returns f(index) as LWE samples the gates accept again.
"""
import torch

from . import circuit


def _ripple(be, a, b, ops):
    """The ripple chain over the bits of a and b with the row ops `ops` per bit: the LAST op produces the carry (or borrow) the
    next bit reads. -> the result rows as a view [bits][len(ops)][B][W] of the arena."""
    assert a.shape == b.shape and a.dim() == 3, "operands must be [bits][B][W]"
    bits, B, W = a.shape
    k = len(ops)
    base = 2 * bits * B                                           # rows of a, rows of b, then k B result rows per bit
    arena = torch.empty((base + bits * k * B, W), dtype=torch.int32, device=a.device)
    arena[:bits * B] = a.reshape(bits * B, W)
    arena[bits * B:base] = b.reshape(bits * B, W)
    i = torch.arange(bits, dtype=torch.int64, device=a.device)[:, None]
    r = torch.arange(B, dtype=torch.int64, device=a.device)[None, :]
    ia = i * B + r
    carry = base + (i - 1) * k * B + (k - 1) * B + r              # the last result row of the previous bit
    ic = torch.where(i == 0, torch.full_like(carry, -1), carry)
    idx = torch.stack([ia, bits * B + ia, ic], dim=-1).repeat(1, k, 1).to(torch.int32).contiguous()   # [bits][k B][3]
    groups = [(op, B) for op in ops]
    for bit in range(bits):
        lo = base + bit * k * B
        be.gate_rows(arena, idx[bit], groups, out=arena[lo:lo + k * B])
    return arena[base:].view(bits, k, B, W)


def add(be, a, b):
    """a + b -> [bits + 1][B][W]: the sum bits, then the carry out."""
    rows = _ripple(be, a, b, ("XOR3", "MAJ3"))
    return torch.cat([rows[:, 0], rows[-1:, 1]], dim=0)


def sub(be, a, b):
    """a - b mod 2^bits -> (difference [bits][B][W], borrow [B][W]); the borrow is set where a < b."""
    rows = _ripple(be, a, b, ("XOR3", "MAJ3N"))
    return rows[:, 0].contiguous(), rows[-1, 1].contiguous()


def less_than(be, a, b):
    """a < b (unsigned) -> [B][W]: the final borrow of a - b; the difference rows are not computed (B rows per bit)."""
    return _ripple(be, a, b, ("MAJ3N",))[-1, 0].contiguous()


def _plan(be, name, bits):
    """The bound plan of generator `name` at `bits` bits on this backend, made on first use and kept with the backend."""
    cache = be.__dict__.setdefault("_circuit_plans", {})
    if (name, bits) not in cache:
        cache[(name, bits)] = getattr(circuit, name)(bits).compile().bind(be)
    return cache[(name, bits)]


def _pair(a, b):
    assert a.shape == b.shape and a.dim() == 3, "operands must be [bits][B][W]"
    return a.shape[0], torch.cat([a, b], dim=0)


def select(be, cond, x, y):
    """cond ? x : y -> [bits][B][W]; cond [B][W], one MUX cell per bit in one level."""
    assert x.shape == y.shape and x.dim() == 3 and cond.shape == x.shape[1:], "cond must be [B][W], x and y [bits][B][W]"
    return _plan(be, "select", x.shape[0]).run(torch.cat([cond[None], x, y], dim=0))


def maximum(be, a, b):
    """max(a, b) (unsigned) -> [bits][B][W]: the borrow chain of a - b, then one level of MUX cells."""
    bits, inputs = _pair(a, b)
    return _plan(be, "maximum", bits).run(inputs)


def equal(be, a, b):
    """a == b -> [B][W]."""
    bits, inputs = _pair(a, b)
    return _plan(be, "equal", bits).run(inputs)[0]


def multiply(be, a, b):
    """a * b -> [2 bits][B][W]."""
    bits, inputs = _pair(a, b)
    return _plan(be, "multiplier", bits).run(inputs)


def lookup(be, index_bits, table, key, basebit=None, l=None, ks_basebit=None, ks_t=None, digits="signed"):
    """table[index] for an index the server holds as encrypted bits -> int32 CUDA tensor [2][N], a ring
    ciphertext under the ring key of the secret that made `key`. index_bits: [depth][W] (or [depth][1][W], one lane of the
    bit-sliced integers above), LSB first, +-1/8 under the loaded key; table: int32 CUDA tensor [entries][2][N], entries <=
    2^depth (keygen.ring_trivial for plaintext rows); key: a client.SelectorKey, or the tensor of Backend.upload_selector_key with
    explicit ks_basebit and ks_t. basebit, l default to keygen.circuit_bootstrap_default of the backend's set at this depth and
    digit form. digits: "signed", or "alternating" (the CMUX form without the ramp of a produced
    selector's error, which carries finer rows; give it a key of circuit_bootstrap_default(..., digits="alternating")'s ks shape).
    One Backend.circuit_bootstrap over the depth bits, then one Backend.ring_lookup: no round trip to the client."""
    from . import keygen
    keygen._check_cmux_form(digits)
    bits = index_bits.reshape(-1, index_bits.shape[-1]).contiguous()
    if basebit is None or l is None:
        d = keygen.circuit_bootstrap_default(keygen.set_name(be.p), bits.shape[0], digits=digits)
        basebit, l = d[0] if basebit is None else basebit, d[1] if l is None else l
    sel = be.circuit_bootstrap(bits, basebit, l, key, ks_basebit, ks_t)
    return be.ring_lookup(table, sel, basebit, l, digits=digits)


def lookup_rows(be, index_bits, table, key, basebit=None, l=None, ks_basebit=None, ks_t=None, digits="signed"):
    """table[index_r] for R indices the server holds as encrypted bits -> int32 CUDA tensor [R][2][N],
    ring ciphertexts under the ring key of the secret that made `key`. index_bits: [depth][R][W], LSB first, +-1/8 under the loaded
    key; table, key, basebit, l, ks_basebit, ks_t and digits as in lookup; the table is shared by all rows. ONE
    Backend.circuit_bootstrap_batch over the R depth bits (selectors [R][depth][2l][2][N]: bit k of index r is sample r depth + k),
    then ONE Backend.ring_lookup_rows: no round trip to the client and no loop over the indices."""
    from . import keygen
    keygen._check_cmux_form(digits)
    assert index_bits.dim() == 3, "index_bits must be [depth][R][W]"
    depth, R, W = index_bits.shape
    if basebit is None or l is None:
        d = keygen.circuit_bootstrap_default(keygen.set_name(be.p), depth, digits=digits)
        basebit, l = d[0] if basebit is None else basebit, d[1] if l is None else l
    if hasattr(key, "body"):
        ks_basebit, ks_t, key = key.ks_basebit, key.ks_t, be.upload_selector_key(key)
    N = be.p.N
    flat = index_bits.permute(1, 0, 2).contiguous().reshape(R * depth, W)
    sel = be.empty(R, depth, 2 * l, 2, N)
    be.circuit_bootstrap_batch(flat, basebit, l, key, ks_basebit, ks_t, out=sel.view(R * depth, 2 * l, 2, N))
    return be.ring_lookup_rows(table, sel, basebit=basebit, l=l, digits=digits)


CIRCUIT_BOOTSTRAP_BITS = 30   # bits of one Backend.circuit_bootstrap call (rs_circuit_bootstrap_dev: depth <= 30); evaluate itself takes
                              # Backend.circuit_bootstrap_batch, tools/ring_rotate_time.py restates the route of calls of 30 with this


def evaluate(be, index_bits, values, key, width=1, basebit=None, l=None, ks_basebit=None, ks_t=None, digits="signed", keyswitch=True):
    """f(index) for a function given as a table, of an index the server holds as encrypted bits -> int32
    CUDA tensor [R width][W] under the loaded key, what the gates accept: rows r width .. r width + width - 1 are the `width` torus
    words of entry index_r. With keyswitch=False the extracted samples [R width][N+1] under the ring key read as an LWE key.
    index_bits: [depth][W] or [depth][R][W], LSB first, +-1/8 under the loaded key; values: int32 torus words [2^depth width] (a
    tensor or an array), entry i at i width .. i width + width - 1; key: a client.SelectorKey, or the tensor of
    Backend.upload_selector_key with explicit ks_basebit and ks_t. basebit, l default to keygen.circuit_bootstrap_default of the
    backend's set at the total CMUX depth and digit form; a depth or step that search refuses raises its ValueError unchanged.
    Where 2^depth width <= N the table is one trivial row: ONE Backend.circuit_bootstrap_batch over all R depth bits (INTEGRATION.md
    section 27), the row broadcast with stride 0, one Backend.ring_rotate with per-row selectors and step = -width,
    Backend.ring_heads, then Backend.keyswitch: l bootstraps per input bit and none per table entry. A longer table is laid out as
    rows of floor-power-of-two(N / width) entries: the high bits choose the row through ONE Backend.ring_lookup_rows over the shared
    table with per-row selectors (one pair of launches per level for all R indices; R = 1 keeps
    Backend.ring_lookup, which gives the same words), and the low bits rotate the chosen rows as above."""
    from . import keygen
    keygen._check_cmux_form(digits)
    N, W = be.p.N, index_bits.shape[-1]
    depth = index_bits.shape[0]
    bits = index_bits.reshape(depth, -1, W)
    R, width = bits.shape[1], int(width)
    if not 1 <= width <= N:
        raise ValueError("width = %d is outside 1 .. %d" % (width, N))
    if not 1 <= depth <= keygen.RING_LOOKUP_MAX_DEPTH:
        raise ValueError("depth = %d is outside 1 .. %d" % (depth, keygen.RING_LOOKUP_MAX_DEPTH))
    values = torch.as_tensor(values, dtype=torch.int32).to(bits.device).reshape(-1)
    if values.numel() != (width << depth):
        raise ValueError("values holds %d words, 2^%d entries of %d words are %d" % (values.numel(), depth, width, width << depth))
    if basebit is None or l is None:
        d = keygen.circuit_bootstrap_default(keygen.set_name(be.p), depth, digits=digits)
        basebit, l = d[0] if basebit is None else basebit, d[1] if l is None else l
    if hasattr(key, "body"):
        ks_basebit, ks_t, key = key.ks_basebit, key.ks_t, be.upload_selector_key(key)
    # selectors [R][depth][2l][2][N]: bit k of index r is sample r depth + k
    flat = bits.permute(1, 0, 2).contiguous().reshape(R * depth, W)
    sel = be.empty(R, depth, 2 * l, 2, N)
    be.circuit_bootstrap_batch(flat, basebit, l, key, ks_basebit, ks_t, out=sel.view(R * depth, 2 * l, 2, N))
    low = min(depth, (N // width).bit_length() - 1)             # 2^low width <= N
    per = width << low
    table = torch.zeros(1 << (depth - low), 2, N, dtype=torch.int32, device=bits.device)
    table[:, 1, :per] = values.view(-1, per)
    if low == depth:
        chosen, stride = table, 0
    else:
        chosen, stride = be.empty(R, 2, N), 1
        if R == 1:
            be.ring_lookup(table, sel[0, low:], basebit, l, out=chosen[0], digits=digits)
        else:
            be.ring_lookup_rows(table, sel[:, low:].contiguous(), basebit=basebit, l=l, out=chosen, digits=digits)
    if low:
        turned = be.ring_rotate(chosen, sel if low == depth else sel[:, :low].contiguous(), -width, basebit, l, stride=stride,
                                per_row=True, digits=digits)
    else:
        turned = chosen
    u = be.ring_heads(turned, width)
    return be.keyswitch(u) if keyswitch else u
