"""Plain numpy reference of the int8 codec over a LIST of tensors, and what
its tests share (a helper module, not a conftest).

The list's concatenation V is what the codec sees: `quantize_gather` must
write the wire (and the flat residual) that tests/quant_ref.py pins for V, and
`dequantize_scatter` must put

    out = (q * scale) * post_scale

into the tensors, both products rounded to float32 on their own and bf16
rounded once more. With post_scale = 1/3 the two roundings are visible:
(q * scale) * f32(1/3) differs from q * (scale * f32(1/3)) in many elements.
With round_first the kernel rounds q * scale into the dtype before it scales
it (nothing changes for f32): those are the bits of the flat dequantize
followed by a float32 multiplication of the stored elements, which is what
the request over a tensor list has to equal, and for bf16 at 1/3 they differ
from the single rounding in about a quarter of the elements.

Every tensor of a case lies in one sentinel-filled byte arena, at a base that
is 16-byte aligned or exactly one element past such a boundary, with at least
16 sentinel bytes between neighbours and around the whole.
"""
import functools

import numpy as np

from tests import quant_ref as qr

F32 = np.float32
ITEM = {"f32": 4, "bf16": 2}
NP_DT = {"f32": np.float32, "bf16": np.uint16}
BITS = {"f32": np.uint32, "bf16": np.uint16}
SENTINEL = 0xCD
GAP = 16  # sentinel bytes between two tensors, at least

# every count is >= 1; totals are no multiple of 256, so the flat kernels that
# the results are compared with are the generic ones
LAYOUTS = {
    # equals the flat kernels' bytes on the same data
    "one": [1000],
    # boundaries on the first element, exactly on a block edge, one past it
    "edges": [1, 255, 1, 256, 257, 3, 511],
    # more than a hundred segments in a block: the walk crosses many entries
    "tiny700": [1 + i % 3 for i in range(700)],
    # whole-block path, element path, whole-block path again at a start that
    # is not block-aligned in V
    "fastslow": [768, 5, 5, 5, 1024, 7],
    # 2,200,066 elements: more wire blocks than one pass of the grid covers
    # (8192 at four waves in each of 2048 workgroups), so the second trip
    # round the grid-stride loop starts inside a segment
    "big": [100003] * 22,
}
BLOCKS = [256, 128]
POST_SCALES = [1.0, 0.5, 1.0 / 3.0]

# collective shapes: the edge layout, and about 3 MiB of f32 in ragged segments
RAGGED_3MIB = [(i * 7919) % 40000 + 1 for i in range(1, 41)]
COLL_LAYOUTS = {"edges": LAYOUTS["edges"], "ragged3m": RAGGED_3MIB}


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case_input(layout, block, dtype):
    """(V, err0) of a layout in `dtype` storage, read-only: qr.make_input's
    tie block, all-zero block and random rest, with a non-zero residual."""
    count = sum(LAYOUTS[layout])
    v, e = qr.make_input(count, block, dtype, seed=count + block)
    v.setflags(write=False)
    e.setflags(write=False)
    return v, e


@functools.lru_cache(maxsize=None)
def gather_expectation(layout, block, dtype, use_err):
    """qr.codec_expectation of the layout's concatenation, read-only."""
    v, e = case_input(layout, block, dtype)
    want = qr.codec_expectation(v, e if use_err else None, v.size, block, dtype)
    for a in want.values():
        a.setflags(write=False)
    return want


def ref_dequantize_scatter(wire, count, block, dtype, post_scale, round_first=False):
    """The concatenation after the scatter, in `dtype` storage: two float32
    multiplications, then the rounding into the dtype. `round_first` rounds
    q * scale into the dtype before the second one: the flat dequantize's
    stored elements, scaled (the request's finish; f32 does not change)."""
    scales, _, q = qr.parse_wire(wire, block)
    dq = (q.astype(F32) * scales[:, None]).astype(F32).reshape(-1)[:count]
    if round_first:
        dq = qr.decode(qr.encode(dq, dtype), dtype)
    return qr.encode((dq * F32(post_scale)).astype(F32), dtype)


def ref_dequantize_fused_scale(wire, count, block, dtype, post_scale):
    """What ONE rounding would give (q * (scale * post_scale)): the tests show
    that it differs from the reference where the issue says it does."""
    scales, _, q = qr.parse_wire(wire, block)
    s = (scales * F32(post_scale)).astype(F32)
    return qr.encode((q.astype(F32) * s[:, None]).astype(F32).reshape(-1)[:count], dtype)


def residual_ok(got, want):
    """The residual is defined up to the fusion of v - q*scale (quant_ref):
    every element equals one of the two correctly rounded forms."""
    return (got == want["err_unfused"].view(got.dtype)) | \
           (got == want["err_fused"].view(got.dtype))


# ---- arenas ----------------------------------------------------------------

class Arena:
    """Byte layout of a list of tensors in one sentinel-filled allocation.
    `misalign`: every base is one element past a 16-byte boundary; otherwise
    every base is 16-byte aligned (relative to the arena's start, which the
    caller places on a 16-byte boundary)."""

    def __init__(self, counts, dtype, misalign):
        self.counts, self.item = list(counts), ITEM[dtype]
        self.np_dt = NP_DT[dtype]
        self.starts = []
        pos = GAP
        for n in self.counts:
            pos = (pos + 15) // 16 * 16 + (self.item if misalign else 0)
            self.starts.append(pos)
            pos += n * self.item + GAP
        self.nbytes = (pos + 15) // 16 * 16
        mask = np.ones(self.nbytes, dtype=bool)
        for s, n in zip(self.starts, self.counts):
            mask[s:s + n * self.item] = False
        self.guard = mask

    def fill(self, v):
        """uint8 image of the arena holding concatenation `v`."""
        img = np.full(self.nbytes, SENTINEL, dtype=np.uint8)
        raw = np.ascontiguousarray(v).view(np.uint8)
        off = 0
        for s, n in zip(self.starts, self.counts):
            img[s:s + n * self.item] = raw[off:off + n * self.item]
            off += n * self.item
        return img

    def blank(self, byte=0xAB):
        img = np.full(self.nbytes, SENTINEL, dtype=np.uint8)
        img[~self.guard] = byte
        return img

    def gather(self, img):
        """The concatenation held by an arena image."""
        return np.concatenate([img[s:s + n * self.item]
                               for s, n in zip(self.starts, self.counts)]).view(self.np_dt)

    def guards_intact(self, img):
        return bool((img[self.guard] == SENTINEL).all())


def aligned_bytes(nbytes):
    """A uint8 numpy array of nbytes whose first byte is 16-byte aligned."""
    raw = np.empty(nbytes + 16, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 16
    return raw[skip:skip + nbytes]


def guarded_bytes(nbytes, fill):
    """(whole, lo): `whole` is [GUARD sentinels | nbytes of `fill` | GUARD
    sentinels] with the body 16-byte aligned at whole[lo:lo + nbytes]."""
    whole = aligned_bytes(nbytes + 2 * qr.GUARD)
    whole[:] = SENTINEL
    whole[qr.GUARD:qr.GUARD + nbytes] = fill
    return whole, qr.GUARD


def body_intact(whole, nbytes):
    return bool((whole[:qr.GUARD] == SENTINEL).all() and
                (whole[qr.GUARD + nbytes:] == SENTINEL).all())
