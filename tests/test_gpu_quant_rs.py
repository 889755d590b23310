"""int8-quantized reduce-scatter on one MI355X: the fused sum-dequantize
kernels of csrc/hip/kernels.hip bit for bit, and the collective with every
rank on device 0 (IPC window transport: fused and wait-flag paths, several
sub-messages per segment with slot wrap, the n=1 branch, ShardedOptimizer).

Expectations, cases and rank workers live in tests/workers_quant_rs.py; the
host twin of this file is tests/test_quant_rs_cpu.py.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import quant_ref as qr  # noqa: E402
from tests import workers_quant_rs as w  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

SENTINEL = 0xCD
GUARD = qr.GUARD


def _dev_bytes(front, body, back=GUARD):
    """uint8 device tensor [front sentinel | body | back sentinel]; body is
    a numpy array or (nbytes, fill)."""
    if isinstance(body, tuple):
        body = np.full(body[0], body[1], dtype=np.uint8)
    body = np.ascontiguousarray(body).view(np.uint8).reshape(-1)
    host = np.full(front + body.size + back, SENTINEL, dtype=np.uint8)
    host[front:front + body.size] = body
    return torch.from_numpy(host).cuda()


def _gpu_sum_dequant(a, b, count, block, dtype, offset_elems=0, op=None):
    """ops.quant_sum_dequant into a guarded buffer; returns out's bits.
    The allocation's base is 16-byte aligned and the guard in front is 64
    bytes, so `out` is 16-byte aligned exactly when offset_elems is 0."""
    from mlsl_amd import ops
    op = op or ops.quant_sum_dequant
    front = GUARD + offset_elems * w.ITEM[dtype]
    nbytes = count * w.ITEM[dtype]
    d_a, d_b = _dev_bytes(0, a), _dev_bytes(0, b)
    d_out = _dev_bytes(front, (nbytes, 0xAB))
    assert d_out.data_ptr() % 16 == 0
    op(d_a[:a.size], d_b[:b.size], d_out[front:front + nbytes], count, block=block,
       dtype=dtype)
    torch.cuda.synchronize()
    for d_w, host in ((d_a, a), (d_b, b)):
        h = d_w.cpu().numpy()
        assert np.array_equal(h[:host.size], host), "wire modified"
        assert (h[host.size:] == SENTINEL).all(), "write behind a wire"
    h = d_out.cpu().numpy()
    assert (h[:front] == SENTINEL).all() and (h[front + nbytes:] == SENTINEL).all(), \
        "write outside out"
    return h[front:front + nbytes].view(w.BITS[dtype]).copy()


# offset 0: fast path where block == 256 and the count is whole blocks,
# generic kernel otherwise; offset 1: generic kernel, scalar stores
CASES = [(c, b, 0) for c, b in w.KERNEL_CASES] + [w.OFFSET_CASE + (1,)]


@requires_gpu
class TestSumDequantExact:
    def setup_method(self, _):
        torch.cuda.set_device(0)

    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    @pytest.mark.parametrize("count,block,offset", CASES)
    def test_exact_wires(self, count, block, offset, dtype):
        a, b, _ = qr.make_exact_wires(count, block, seed=count)
        got = _gpu_sum_dequant(a, b, count, block, dtype, offset)
        assert np.array_equal(got, w.exact_wire_sum(a, b, count, block, dtype))

    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    @pytest.mark.parametrize("count,block,offset", CASES)
    def test_random_wires(self, count, block, offset, dtype):
        a, b = w.random_wires(count, block, seed=count)
        got = _gpu_sum_dequant(a, b, count, block, dtype, offset)
        ok = w.matches_a_candidate(got, w.sum_candidates(a, b, count, block, dtype))
        assert ok.all(), f"{(~ok).sum()} elements match no candidate"

    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    def test_wires_at_8_byte_offsets(self, dtype):
        # TMP slots and wire segments start at multiples of 264 bytes: the
        # fast path must take wires that are 8 but not 16 bytes aligned
        from mlsl_amd import ops
        count, block = 1280, 256
        a, b = w.random_wires(count, block, seed=3)
        pad = np.zeros(8, dtype=np.uint8)
        d_a = torch.from_numpy(np.concatenate([pad, a])).cuda()
        d_b = torch.from_numpy(np.concatenate([pad, b])).cuda()
        out = torch.zeros(count * w.ITEM[dtype], dtype=torch.uint8, device="cuda")
        assert d_a.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
        ops.quant_sum_dequant(d_a[8:], d_b[8:], out, count, block=block, dtype=dtype)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(w.BITS[dtype])
        assert w.matches_a_candidate(
            got, w.sum_candidates(a, b, count, block, dtype)).all()

    @pytest.mark.parametrize("dtype", ["f32", "bf16"])
    def test_nt_hook(self, dtype):
        from mlsl_amd import ops
        a, b, _ = qr.make_exact_wires(1280, 256, seed=5)
        got = _gpu_sum_dequant(a, b, 1280, 256, dtype, op=ops.quant_sum_dequant_nt)
        assert np.array_equal(got, w.exact_wire_sum(a, b, 1280, 256, dtype))

    def test_nontemporal_from_128_mib(self):
        # the smallest output that LaunchQuantSumDequant itself stores
        # nontemporally (kSumDequantNtBytes): 32 Mi f32 elements
        count = (128 << 20) // 4
        a, b, _ = qr.make_exact_wires(count, 256, seed=9)
        got = _gpu_sum_dequant(a, b, count, 256, "f32")
        assert np.array_equal(got, w.exact_wire_sum(a, b, count, 256, "f32"))

    def test_rejects_other_dtypes(self):
        from mlsl_amd import ops
        a, b, _ = qr.make_exact_wires(64, 8, seed=1)
        out = torch.zeros(64, dtype=torch.float64, device="cuda")
        with pytest.raises(RuntimeError, match="f32/bf16 only"):
            ops.quant_sum_dequant(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(),
                                  out, 64, block=8, dtype="f64")


# ---- collective, every rank on device 0 ------------------------------------

@requires_gpu
def test_quant_reduce_scatter_world2():
    w.run_ranks("rs_check", 2, device=True)


@requires_gpu
def test_quant_reduce_scatter_world4():
    w.run_ranks("rs_check", 4, device=True)


@requires_gpu
def test_quant_reduce_scatter_unfused_transport():
    # fused kernels off: wait-flag kernel, wide copy, set-flag kernel
    w.run_ranks("rs_check", 2, device=True, extra_env={"MLSL_P2P_FUSED_MAX_KB": "0"})


@requires_gpu
def test_quant_reduce_scatter_multislot():
    # 1 MiB slots against a 3.1 MiB wire segment: several sub-messages per
    # segment, slot wrap, sub-message boundaries on wire-unit boundaries
    w.run_ranks("rs_check", 2, device=True, extra_env={"MLSL_P2P_SLOT_MB": "1"},
                shapes=[(3 << 20, 256)], dtypes=["f32"])


@requires_gpu
def test_quant_reduce_scatter_numpy_buffers():
    # pageable send and recv buffers: staged through HBM around the
    # compressed issue path, the pinned bounce copied out at completion
    w.run_ranks("rs_check", 2, device="numpy", inplace=[False])


@requires_gpu
def test_quant_reduce_scatter_world1():
    w.run_ranks("rs_check", 1, device=True)


@requires_gpu
def test_sharded_optimizer_int8():
    w.run_ranks("rs_sharded_optimizer", 2, device=True)
