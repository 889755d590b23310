"""The int4 wire codec on the GPU (single MI355X): every kernel bit for bit
against the numpy reference and its host twin (both through the helpers of
tests/test_quant4_cpu.py), outputs between sentinels; then the bits=4
collectives and ShardedOptimizer with every rank on one device. `path` names a
launcher's kernel, None leaves it the choice (csrc/hip/kernels.hip)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import quant4_ref as q4  # noqa: E402
from tests import quant_ref as qr  # noqa: E402
from tests import workers_quant4 as w4  # noqa: E402
from tests.test_gpu_kernels_exact import ITEM, _dev_bytes, _intact, _split  # noqa: E402
from tests.test_quant4_cpu import CODEC_CASES, host_codec, host_sums  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


def _trip(path):
    """A count past the grid cap of `path`: its loop takes a second trip."""
    from mlsl_amd import ops
    return (ops.quant4_blocks_per_trip(path == "fast") + 3) * 256


# (count, block, path, offset_elems)
CODEC_PATHS = [(c, b, None, 0) for c, b in CODEC_CASES] + [
    (1280, 256, "fast", 0), (1280, 256, "generic", 0),   # five blocks: an idle half-wave
    (1280, 256, None, 1),       # one element past a 16-byte boundary: generic
    (1 << 16, 256, None, 0),    # 256 KiB of f32: the launcher's own f32 threshold
]


@pytest.mark.parametrize("count,block,path,offset,dtype,use_err", [
    c + (dt, ue) for c in CODEC_PATHS for dt in ("f32", "bf16")
    for ue in ("none", "zero", "rand")] + [
    # a second trip on each path; the generic one ends in a partial block
    ("fast", 256, "fast", 0, "f32", "rand"), ("generic", 256, "generic", 0, "bf16", "rand")],
    ids=str)
def test_codec(count, block, path, offset, dtype, use_err):
    from mlsl_amd import ops
    if isinstance(count, str):
        count = _trip(path) + (0 if path == "fast" else 77)
    torch.cuda.set_device(0)
    inp, err0, want = host_codec(count, block, dtype, use_err)
    off, nbytes, wbytes = offset * ITEM[dtype], count * ITEM[dtype], want["wire"].size
    d_in, d_err = _dev_bytes(off, inp, back=0), _dev_bytes(off, err0)
    d_wire, d_out = _dev_bytes(0, (wbytes, 0xAB)), _dev_bytes(off, (nbytes, 0xAB))
    ops.quantize4(d_in[off:], d_wire[:wbytes], count, block=block, dtype=dtype, path=path,
                  err=None if use_err == "none" else d_err[off:off + nbytes])
    ops.dequantize4(d_wire[:wbytes], d_out[off:off + nbytes], count, block=block, dtype=dtype,
                    path=path)
    torch.cuda.synchronize()
    _, wire, wire_g = _split(d_wire, 0, wbytes)
    out_f, out, out_g = _split(d_out, off, nbytes)
    err_f, err, err_g = _split(d_err, off, nbytes)
    assert np.array_equal(wire, want["wire"])
    assert np.array_equal(out, want["out"].view(np.uint8))
    assert np.array_equal(err, want["err"].view(np.uint8))
    assert _intact(wire_g, out_f, out_g, err_f, err_g), "write outside a buffer"


# (count, block, path, wire_off: every wire that many bytes into its allocation)
SUM_CASES = [
    (1280, 256, "fast", 0), (1280, 256, "generic", 0),
    (1280, 256, "fast", 8),      # wires 8 but not 16 bytes aligned
    (1000, 256, None, 0),        # a partial last block: generic
    (100, 24, None, 4),          # 20-byte wire blocks, 4-byte aligned wires
    (61, 8, None, 0),
]


@pytest.mark.parametrize("count,block,path,wire_off,nwires", [
    c + (n,) for c in SUM_CASES for n in (1, 2, 3, 8)] + [
    ("fast", 256, "fast", 0, 2), ("generic", 256, "generic", 0, 2)], ids=str)
def test_sums(count, block, path, wire_off, nwires):
    """Both N-way kernels; the requantize out of place and into the first and
    the last wire. From three wires on also in reverse order, which changes
    the bits as the reference says."""
    from mlsl_amd import ops
    torch.cuda.set_device(0)
    count = _trip(path) if isinstance(count, str) else count
    wires, outs, want = host_sums(count, block, nwires)
    wb = wires[0].size

    def dev():
        d_w = [_dev_bytes(wire_off, x) for x in wires]
        return d_w, [d[wire_off:wire_off + wb] for d in d_w]

    def wires_kept(d_w, but=None):
        return all(np.array_equal(_split(d, wire_off, wb)[1], x)
                   for k, (d, x) in enumerate(zip(d_w, wires)) if k != but)
    orders = [1, -1] if nwires >= 3 and count >= 1000 else [1]
    for dtype, order in [("f32", o) for o in orders] + [("bf16", 1)]:
        nbytes = count * ITEM[dtype]
        d_w, views = dev()
        d_out = _dev_bytes(16, (nbytes, 0xAB))
        ops.quant_sum_dequant_n4(views[::order], d_out[16:16 + nbytes], count, block=block,
                                 dtype=dtype, path=path)
        torch.cuda.synchronize()
        out_f, out, out_g = _split(d_out, 16, nbytes)
        ref = outs[dtype] if order == 1 else q4.sum_dequant(wires[::-1], count, block, dtype)
        assert np.array_equal(out, ref.view(np.uint8)), (dtype, order)
        assert _intact(out_f, out_g) and wires_kept(d_w)
    for alias in (None, 0, nwires - 1):
        d_w, views = dev()
        d_dst = _dev_bytes(wire_off, (wb, 0xAB)) if alias is None else d_w[alias]
        ops.quant_sum_requant_n4(views, d_dst[wire_off:wire_off + wb], qr.nblocks(count, block),
                                 block=block, path=path)
        torch.cuda.synchronize()
        front, got, back = _split(d_dst, wire_off, wb)
        assert np.array_equal(got, want), f"dst is wire {alias}"
        assert _intact(front, back) and wires_kept(d_w, alias)


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("kind", ["all_reduce", "reduce_scatter"])
def test_collective_one_device(kind, world):
    w4.run_ranks("coll_check", world, device=True, kind=kind)


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_optimizer_one_device(world):
    w4.run_ranks("sharded_optimizer", world, device=True)
