"""Plain numpy reference of the fused AdamW step (ops.adamw_step): every `*`,
`+`, `-`, `/` and sqrt below is one correctly rounded float32 operation, so
these are the bits the kernel and its host twin must produce. bf16 and f16
arrays are uint16 bit patterns (a helper module, not a conftest)."""
import math

import numpy as np

from tests import quant_ref as qr

F32 = np.float32
NP_BITS = {"f32": np.float32, "bf16": np.uint16, "f16": np.uint16}
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
MODES = ("none", "param", "delta")   # what `out` takes


def decode(a, dtype):
    return a.view(np.float16).astype(F32) if dtype == "f16" else qr.decode(a, dtype)


def encode(x, dtype):
    return x.astype(np.float16).view(np.uint16) if dtype == "f16" else qr.encode(x, dtype)


def coef(total, max_norm, grad_scale):
    if total is None:
        return F32(1)
    return F32(min(1.0, float(F32(max_norm)) / (math.sqrt(total) * float(F32(grad_scale)) + 1e-6)))


def step(g, p, m, v, dtype, *, lr, betas, eps, weight_decay, step, grad_scale=1.0, total=None,
         max_norm=None, replica=None, want_out=True):
    """(p, m, v, out) after one step, the inputs left alone; out is the rounded
    p, with `replica` the rounded p - replica, None for want_out=False."""
    b1, b2 = float(betas[0]), float(betas[1])
    gs = (decode(g, dtype) * F32(grad_scale)) * coef(total, max_norm, grad_scale)
    m = m * F32(b1) + gs * F32(1.0 - b1)
    v = v * F32(b2) + (gs * gs) * F32(1.0 - b2)
    den = np.sqrt(v) / F32(math.sqrt(1.0 - b2 ** step)) + F32(eps)
    p = p * F32(1.0 - lr * weight_decay) - (m / den) * F32(lr / (1.0 - b1 ** step))
    assert p.dtype == m.dtype == v.dtype == F32
    out = encode(p if replica is None else p - decode(replica, dtype), dtype) if want_out else None
    return p, m, v, out


def inputs(count, dtype, seed):
    """g, p, m, v and a replica near p; |g| and |p| in [2**-10, 4], so that no
    f32 intermediate is subnormal."""
    rng = np.random.default_rng(seed)
    mag = lambda: (np.exp2(rng.uniform(-10, 2, count))   # noqa: E731
                   * rng.choice([-1.0, 1.0], count)).astype(F32)
    g, p, m, v = encode(mag(), dtype), mag(), mag() * F32(0.1), np.square(mag()) * F32(0.01)
    return g, p, m, v, encode(p * F32(1.001), dtype)
