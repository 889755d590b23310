"""Plain numpy reference of the int8 block wire codec, and the inputs the
codec tests share (a helper module, not a conftest).

Wire block: [f32 scale][f32 0.0][int8 x block]; the last block's payload is
zero past `count`. Per block, all in float32 and in this order:

    scale = m / 127 if m > 0 else 1        (m = max |v| of the block)
    inv   = 1 / scale
    q     = clip(rint(v * inv), -127, 127) (rint: round half to even)
    out   = q * scale
    err   = v - q * scale                  (defined up to fusion, see below)

numpy evaluates every float32 operation correctly rounded, so these are the
bits an IEEE implementation must produce. torch is used for the bf16
conversion only; bf16 arrays are uint16 bit patterns.
"""
import numpy as np
import torch  # at import time: torch has to be loaded before libmlsl_amd.so

HDR = 8
GUARD = 64  # bytes of sentinel after (or around) a buffer under test
F32 = np.float32


def nblocks(count, block):
    return (count + block - 1) // block


def wire_bytes(count, block):
    return nblocks(count, block) * (block + HDR)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def f32_to_bf16(x):
    """float32 -> bf16 bit patterns, round to nearest even."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def decode(a, dtype):
    """Array as the codec sees it: float32 values."""
    return bf16_to_f32(a) if dtype == "bf16" else np.asarray(a, dtype=F32)


def encode(x, dtype):
    return f32_to_bf16(x) if dtype == "bf16" else np.asarray(x, dtype=F32)


def ref_quantize(v_f32, block):
    """(scales[nb] f32, q[nb, block] int8); q is 0 past the end of v."""
    v = np.asarray(v_f32, dtype=F32)
    nb = nblocks(v.size, block)
    vb = np.zeros(nb * block, dtype=F32)
    vb[:v.size] = v
    vb = vb.reshape(nb, block)
    m = np.abs(vb).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        scales = np.where(m > 0, m / F32(127), F32(1)).astype(F32)
    inv = F32(1) / scales
    q = np.clip(np.rint(vb * inv[:, None]), F32(-127), F32(127))
    return scales, q.astype(np.int8)


def ref_wire(scales, q):
    """Wire bytes (uint8, flat) of blocks (scales, q)."""
    nb, block = q.shape
    w = np.zeros((nb, block + HDR), dtype=np.uint8)
    w[:, 0:4] = np.ascontiguousarray(scales, dtype=F32).view(np.uint8).reshape(nb, 4)
    w[:, HDR:] = np.ascontiguousarray(q).view(np.uint8)
    return w.reshape(-1)


def parse_wire(wire, block):
    """(scales[nb] f32, word1[nb] f32, q[nb, block] int8) of wire bytes."""
    w = np.ascontiguousarray(wire, dtype=np.uint8).reshape(-1, block + HDR)
    scales = w[:, 0:4].copy().view(F32).reshape(-1)
    word1 = w[:, 4:8].copy().view(F32).reshape(-1)
    q = w[:, HDR:].copy().view(np.int8)
    return scales, word1, q


def ref_dequantize(scales, q, count, dtype="f32"):
    out = (q.astype(F32) * np.asarray(scales, dtype=F32)[:, None]).reshape(-1)[:count]
    return encode(out, dtype)


def ref_residuals(v_f32, scales, q, dtype="f32"):
    """Both correctly rounded forms of v - q*scale, (unfused, fused): a
    compiler may contract the expression into one fma, and either is right."""
    v = np.asarray(v_f32, dtype=F32)
    n = v.size
    qf = q.reshape(-1)[:n]
    s = np.repeat(np.asarray(scales, dtype=F32), q.shape[1])[:n]
    unfused = (v - qf.astype(F32) * s).astype(F32)
    # int8 x f32 is exact in float64, so one rounding remains: the fma's
    fused = (v.astype(np.float64) - qf.astype(np.float64) * s.astype(np.float64)).astype(F32)
    return encode(unfused, dtype), encode(fused, dtype)


def ref_quant_accum_unfused(acc_wire, wire, count, block):
    """acc += wire with every float32 operation rounded on its own (what a
    target without fma computes); header word 1 and padding keep acc's."""
    sa, w1, qa = parse_wire(acc_wire, block)
    sb, _, qb = parse_wire(wire, block)
    v = (qa.astype(F32) * sa[:, None] + qb.astype(F32) * sb[:, None]).astype(F32)
    v = v.reshape(-1)
    v[count:] = 0
    ns, nq = ref_quantize(v, block)
    nq = nq.reshape(-1)
    nq[count:] = qa.reshape(-1)[count:]
    out = ref_wire(ns, nq.reshape(qa.shape)).reshape(-1, block + HDR)
    out[:, 4:8] = w1.view(np.uint8).reshape(-1, 4)
    return out.reshape(-1)


def exact_sums(acc_wire, wire, count, block):
    """float64 a*as + b*bs per element (both products are exact), and as+bs
    per element."""
    sa, _, qa = parse_wire(acc_wire, block)
    sb, _, qb = parse_wire(wire, block)
    s = qa.astype(np.float64) * sa.astype(np.float64)[:, None] + \
        qb.astype(np.float64) * sb.astype(np.float64)[:, None]
    ssum = np.repeat(sa.astype(np.float64) + sb.astype(np.float64), block)
    return s.reshape(-1)[:count], ssum[:count]


# ---- shared inputs ---------------------------------------------------------

TIE_BLOCK, ZERO_BLOCK = 0, 1


def make_input(count, block, dtype, seed):
    """(inp, err) for one codec case, in `dtype` storage.

    Block 0 is the tie block: its first element is 127 * 2^-3, so the scale
    is exactly 2^-3, and the others are +-(k + 0.5) * 2^-3, every one a
    rounding tie (all exactly representable in bf16 too). Block 1 is all
    zero (scale must be 1.0). The rest is randn * 3. err is randn * 0.01 and
    zero in the two special blocks.
    """
    assert nblocks(count, block) >= 3 and block >= 8
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(count) * 3).astype(F32)
    e = (rng.standard_normal(count) * 0.01).astype(F32)
    k = (np.arange(block) % 127).astype(F32)
    sign = np.where(rng.integers(0, 2, block) == 0, F32(-1), F32(1))
    tie = sign * (k + F32(0.5)) * F32(0.125)
    tie[0] = F32(127 * 0.125)
    v[TIE_BLOCK * block:(TIE_BLOCK + 1) * block] = tie
    v[ZERO_BLOCK * block:(ZERO_BLOCK + 1) * block] = 0
    e[:2 * block] = 0
    return encode(v, dtype), encode(e, dtype)


def codec_expectation(inp, err, count, block, dtype):
    """Everything a quantize + dequantize of (inp, err) must produce:
    dict(wire, out, err_unfused, err_fused); err may be None."""
    v = decode(inp, dtype)
    if err is not None:
        v = (v + decode(err, dtype)).astype(F32)
    scales, q = ref_quantize(v, block)
    r0, r1 = ref_residuals(v, scales, q, dtype)
    return dict(wire=ref_wire(scales, q), out=ref_dequantize(scales, q, count, dtype),
                err_unfused=r0, err_fused=r1, scales=scales, q=q)


def make_exact_wires(count, block, seed):
    """Two hand-built wires whose compressed-domain sum is exact in float32
    whether or not the multiply-adds are fused: power-of-two scales from
    2^-6..2^-3 per block, payload uniform in [-127, 127] and zero past
    `count`, header word 1 = 0.0. Returns (a, b, want): want is the wire of
    the re-quantized exact sum."""
    rng = np.random.default_rng(seed)
    nb = nblocks(count, block)
    wires, sums = [], np.zeros(nb * block, dtype=F32)
    for _ in range(2):
        scales = np.exp2(rng.integers(-6, -2, nb)).astype(F32)
        q = rng.integers(-127, 128, (nb, block)).astype(np.int8)
        q.reshape(-1)[count:] = 0
        wires.append(ref_wire(scales, q))
        # |q| < 2^7 on a grid of 2^-6: every term and the sum fit 24 bits
        sums += (q.astype(F32) * scales[:, None]).reshape(-1)
    want = ref_wire(*ref_quantize(sums[:count], block))
    return wires[0], wires[1], want


def guarded(n, dtype, fill, sentinel=0xCD):
    """(whole, view): `view` is n elements of `dtype` filled with byte
    `fill`, followed in `whole` (uint8) by GUARD sentinel bytes."""
    item = np.dtype(dtype).itemsize
    whole = np.full(n * item + GUARD, sentinel, dtype=np.uint8)
    whole[:n * item] = fill
    return whole, whole[:n * item].view(dtype)
