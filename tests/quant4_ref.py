"""Plain numpy reference of the int4 block wire codec in float32, and the
inputs its tests share (a helper module in the manner of tests/quant_ref.py).

Wire block: [f32 scale][f32 0.0][block / 2 payload bytes]; element i is nibble
i & 1 of payload byte i >> 1, 4-bit two's complement, zero past `count`.
scale = m / 7 if m > 0 else 1 (m = max |v|); q = clip(rint(v * (1 / scale)),
-7, 7); out = q * scale; err = fma(-q, scale, v); a sum is fma(q_r, scale_r,
acc) per wire r in order, from acc = +0.
"""
import numpy as np

from tests import quant_ref as qr

F32, F64, HDR = np.float32, np.float64, 8
TIE_BLOCK, ZERO_BLOCK, NEG_BLOCK = 0, 1, 2


def quantize(v, block):
    """(scales[nb] f32, q[nb, block] int8); q is 0 past the end of v."""
    nb = qr.nblocks(v.size, block)
    vb = np.zeros(nb * block, dtype=F32)
    vb[:v.size] = v
    vb = vb.reshape(nb, block)
    m = np.abs(vb).max(axis=1)
    scales = np.where(m > 0, m / F32(7), F32(1)).astype(F32)
    q = np.clip(np.rint(vb * (F32(1) / scales)[:, None]), F32(-7), F32(7))
    return scales, q.astype(np.int8)


def pack(scales, q):
    nb, block = q.shape
    w = np.zeros((nb, block // 2 + HDR), dtype=np.uint8)
    w[:, 0:4] = np.ascontiguousarray(scales, dtype=F32).view(np.uint8).reshape(nb, 4)
    nib = q.astype(np.uint8) & 0xF
    w[:, HDR:] = nib[:, 0::2] | (nib[:, 1::2] << 4)
    return w.reshape(-1)


def unpack(wire, block):
    """(scales[nb], header word 1 [nb] uint32, q[nb, block] int8)."""
    w = np.ascontiguousarray(wire, dtype=np.uint8).reshape(-1, block // 2 + HDR)
    nib = np.stack([w[:, HDR:] & 0xF, w[:, HDR:] >> 4], axis=2).reshape(w.shape[0], block)
    q = ((nib.astype(np.int16) ^ 8) - 8).astype(np.int8)
    return w[:, 0:4].copy().view(F32).reshape(-1), w[:, 4:8].copy().view(np.uint32), q


def fma(q, s, acc):
    # q * s is exact in float64 (4 x 24 bits) and so is adding a float32 within
    # 2^20 of it: the cast is the fma's one rounding
    return (q.astype(F64) * s.astype(F64) + acc.astype(F64)).astype(F32)


def codec(inp, err, count, block, dtype):
    """dict(wire, out, err) of quantize + dequantize; err may be None."""
    v = qr.decode(inp, dtype)
    if err is not None:
        v = (v + qr.decode(err, dtype)).astype(F32)
    scales, q = quantize(v, block)
    s = np.repeat(scales, block)[:count]
    qf = q.reshape(-1)[:count].astype(F32)
    return dict(wire=pack(scales, q), out=qr.encode(qf * s, dtype),
                err=qr.encode(fma(-qf, s, v), dtype))


def fma_sum(wires, block):
    parsed = [unpack(x, block) for x in wires]
    scales = np.stack([p[0] for p in parsed]).astype(F64)
    assert (scales.max(axis=0) / scales.min(axis=0)).max() < 2.0 ** 16, "reference not exact"
    acc = np.zeros(parsed[0][2].shape, dtype=F32)
    for s, _, q in parsed:
        acc = fma(q, s[:, None], acc)
    return acc


def sum_dequant(wires, count, block, dtype):
    return qr.encode(fma_sum(wires, block).reshape(-1)[:count], dtype)


def sum_requant(wires, block):
    return pack(*quantize(fma_sum(wires, block).reshape(-1), block))


def make_input(count, block, dtype, seed):
    """(inp, err). From three blocks on: block 0 all rounding ties at scale
    2^-3, block 1 zero, block 2 with a negative extreme; err 0 in those."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(count) * 3).astype(F32)
    e = (rng.standard_normal(count) * 0.01).astype(F32)
    if count >= 3 * block:
        sign = np.where(rng.integers(0, 2, block) == 0, F32(-1), F32(1))
        v[:block] = sign * ((np.arange(block) % 7).astype(F32) + F32(0.5)) * F32(0.125)
        v[0] = F32(0.875)
        v[block:2 * block] = 0
        v[2 * block] = -np.abs(v[2 * block:3 * block]).max() - F32(1)
        e[:3 * block] = 0
    return qr.encode(v, dtype), qr.encode(e, dtype)


def make_wires(nwires, count, block, seed):
    """Wires of randn * m, m in [1, 4]. From two wires and three blocks on,
    block 0 sums to ties of the requantize and block 1 is zero in all."""
    rng = np.random.default_rng(seed)
    out = []
    for r, m in enumerate(np.linspace(1.0, 4.0, nwires)):
        scales, q = quantize((rng.standard_normal(count) * m).astype(F32), block)
        if nwires >= 2 and count >= 3 * block:
            sign = np.where(np.arange(block) % 3 == 0, -1, 1).astype(np.int8)
            q[0] = sign if r == 0 else sign * (np.arange(block) % 7) if r == 1 else 0
            q[0, 0] = 7 if r == 1 else 0
            scales[0] = [0.0625, 0.125][r] if r < 2 else 1.0
            q[1], scales[1] = 0, 1.0
        out.append(pack(scales, q))
    return out
