"""Exact GPU kernel tests (single MI355X).

The int8 wire codec is compared bit for bit with the numpy reference in
tests/quant_ref.py: wire bytes (header, reserved word, payload, zeroed
padding), dequantized output, residual, and the memory after every buffer.
Reductions, the streaming copy and the benchmark A/B hooks are compared
with exact CPU results at sizes that run every loop of every kernel.

Which case reaches which kernel follows from the dispatch conditions in
csrc/hip/kernels.hip (LaunchQuantize, LaunchDequantize, LaunchQuantAccum,
LaunchReduce, LaunchCopyVariant); each parameter list says it per case.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import quant_ref as qr  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

GUARD = qr.GUARD
SENTINEL = 0xCD
ITEM = {"f32": 4, "bf16": 2}
NP_DT = {"f32": np.float32, "bf16": np.uint16}


def _dev_bytes(front, body, back=GUARD):
    """uint8 device tensor [front sentinel | body | back sentinel]; body is
    a numpy array (any dtype) or (nbytes, fill)."""
    if isinstance(body, tuple):
        body = np.full(body[0], body[1], dtype=np.uint8)
    body = np.ascontiguousarray(body).view(np.uint8).reshape(-1)
    host = np.full(front + body.size + back, SENTINEL, dtype=np.uint8)
    host[front:front + body.size] = body
    return torch.from_numpy(host).cuda()


def _split(t, front, nbytes):
    """(front guard, body, back guard) of a _dev_bytes tensor, on the host."""
    h = t.cpu().numpy()
    return h[:front], h[front:front + nbytes], h[front + nbytes:]


def _intact(*guards):
    return all((g == SENTINEL).all() for g in guards)


def _run_codec(count, block, dtype, use_err, offset_elems=0, quantize=None,
               dequantize=None):
    from mlsl_amd import ops
    quantize = quantize or ops.quantize
    dequantize = dequantize or ops.dequantize
    item, off = ITEM[dtype], offset_elems * ITEM[dtype]
    nbytes, wbytes = count * item, qr.wire_bytes(count, block)
    inp, err0 = qr.make_input(count, block, dtype, seed=count + block)
    want = qr.codec_expectation(inp, err0 if use_err else None, count, block, dtype)

    d_in = _dev_bytes(off, inp, back=0)
    d_err = _dev_bytes(off, err0)
    d_wire = _dev_bytes(0, (wbytes, 0xAB))
    d_out = _dev_bytes(off, (nbytes, 0xAB))
    e_arg = d_err[off:off + nbytes] if use_err else None
    quantize(d_in[off:], d_wire[:wbytes], count, err=e_arg, block=block, dtype=dtype)
    dequantize(d_wire[:wbytes], d_out[off:off + nbytes], count, block=block, dtype=dtype)
    torch.cuda.synchronize()

    _, wire, wire_g = _split(d_wire, 0, wbytes)
    out_f, out, out_g = _split(d_out, off, nbytes)
    err_f, err, err_g = _split(d_err, off, nbytes)
    assert np.array_equal(d_in.cpu().numpy()[off:], inp.view(np.uint8))

    scales, word1, q = qr.parse_wire(wire, block)
    assert np.array_equal(scales.view(np.uint32), want["scales"].view(np.uint32)), \
        "block scales"
    assert not word1.view(np.uint32).any(), "reserved header word"
    assert np.array_equal(q, want["q"]), "payload (padding included)"
    assert np.array_equal(wire, want["wire"])
    assert scales[qr.TIE_BLOCK] == np.float32(0.125) and scales[qr.ZERO_BLOCK] == 1.0
    assert np.array_equal(out, want["out"].view(np.uint8)), "dequantized output"
    bits = {4: np.uint32, 2: np.uint16}[item]
    if use_err:
        got = err.view(bits)
        ok = (got == want["err_unfused"].view(bits)) | (got == want["err_fused"].view(bits))
        assert ok.all(), f"residual: {(~ok).sum()} elements match neither rounding"
    else:
        assert np.array_equal(err, err0.view(np.uint8))
    assert _intact(wire_g, out_f, out_g, err_f, err_g), "write outside a buffer"


def _both(count, block):
    return [(count, block, "f32"), (count, block, "bf16")]


# kernel reached (quantize / dequantize), from X2Eligible and the 16 MiB rule
CODEC_CASES = (
    # QuantizeKernel / DequantizeKernel, fewer elements per block than lanes
    _both(20, 8)
    # generic kernels: tail block of 107 with a scalar tail of 3
    + _both(1003, 128)
    # generic kernels: tail block of 232, padding of 24
    + _both(1000, 256)
    # generic kernels: two vector passes per lane, tail block of 392
    + _both(5000, 512)
    # bf16: QuantizeX2Kernel / DequantizeBf16x2Kernel with 5 blocks (idle
    # half-wave); f32 (< 4 MiB): generic kernels on whole blocks
    + _both(1280, 256)
    # f32 >= 4 MiB: QuantizeX2Kernel<float> / DequantizeF32x2Kernel, odd count
    + [((1 << 20) + 256, 256, "f32")]
    # 16387 blocks > 16384 per pass: second grid-stride pass of the x2 kernels
    + _both(16387 * 256, 256)
    # 8196 blocks > 8192 per pass: second pass of the generic kernels
    + [(8195 * 256 + 77, 256, "f32")]
    # >= 16 MiB, not whole blocks: DequantizeKernel<float, NT>
    + [((1 << 22) + 100, 256, "f32")]
)


@requires_gpu
class TestCodecExact:
    def setup_method(self, _):
        torch.cuda.set_device(0)

    @pytest.mark.parametrize("use_err", [True, False], ids=["err", "noerr"])
    @pytest.mark.parametrize("count,block,dtype", CODEC_CASES)
    def test_quantize_dequantize(self, count, block, dtype, use_err):
        _run_codec(count, block, dtype, use_err)

    @pytest.mark.parametrize("use_err", [True, False], ids=["err", "noerr"])
    def test_bf16_offset_views_take_generic_kernels(self, use_err):
        # input, err and output start one element (2 bytes) into their
        # allocations: not 16-byte aligned, so X2Eligible refuses and the
        # generic kernels (scalar stores in dequantize) must give the same
        # bytes; the element in front of each buffer is guarded too
        _run_codec(1280, 256, "bf16", use_err, offset_elems=1)

    def test_nt_hooks(self):
        # QuantizeX2Kernel<float, true, NT_ST=true> and
        # DequantizeKernel<float, NT=true>, at a whole-block shape
        from mlsl_amd import ops

        def q_nt(inp, wire, count, err, block, dtype):
            ops.quantize_f32_nt(inp, wire, count, err, block=block)

        _run_codec(1280, 256, "f32", True, quantize=q_nt, dequantize=ops.dequantize_nt)


def _accum_on_gpu(a, b, count, block):
    """ops.quant_accum on copies of wires a, b; returns the new acc bytes."""
    from mlsl_amd import ops
    d_a, d_b = _dev_bytes(0, a), _dev_bytes(0, b)
    ops.quant_accum(d_a[:a.size], d_b[:b.size], count, block=block)
    torch.cuda.synchronize()
    _, acc, acc_g = _split(d_a, 0, a.size)
    _, src, src_g = _split(d_b, 0, b.size)
    assert np.array_equal(src, b), "source wire modified"
    assert _intact(acc_g, src_g), "write outside a wire"
    return acc


@requires_gpu
class TestQuantAccumExact:
    def setup_method(self, _):
        torch.cuda.set_device(0)

    @pytest.mark.parametrize("count,block", [
        (1280, 256),        # QuantAccum256Kernel
        (1000, 256),        # QuantAccumKernel: tail block, padding
        (1003, 128),        # QuantAccumKernel: scalar tail
        (8195 * 256, 256),  # QuantAccum256Kernel, second grid-stride pass
    ])
    def test_exact_wires(self, count, block):
        # power-of-two scales: every a*as + b*bs is exact, fused or not, so
        # the whole result wire is determined, reserved word and padding too
        a, b, want = qr.make_exact_wires(count, block, seed=count)
        acc = _accum_on_gpu(a, b, count, block)
        ns, word1, q = qr.parse_wire(acc, block)
        ws, _, wq = qr.parse_wire(want, block)
        assert np.array_equal(ns.view(np.uint32), ws.view(np.uint32)), "block scales"
        assert not word1.view(np.uint32).any(), "reserved header word"
        assert np.array_equal(q, wq), "payload (padding included)"
        assert np.array_equal(acc, want)

    @pytest.mark.parametrize("count,block", [
        (1 << 18, 256),   # QuantAccum256Kernel
        (100003, 128),    # QuantAccumKernel
    ])
    def test_quantized_random_wires(self, count, block):
        """Arbitrary scales: a*as + b*bs may be fused, so a sum within a
        rounding error of a half-integer quotient may round either way.

        With s the exact sum and ns the new scale, q must be
        clip(rint(s/ns)) except where s/ns is within
        delta = 2^-20 * 127 * (as+bs) / ns of a half-integer: |s| <=
        127*(as+bs), so one f32 rounding of the sum moves s/ns by at most
        2^-24*127*(as+bs)/ns, and the roundings of 1/ns and of the product
        add two more of at most 2^-24*127.5 each; delta is sixteen times
        the first and covers all three. The zone may hold 0.1 % of a case.
        The header is f32(max|s|/127) up to one rounding of the largest sum
        and one of the division: 4 ulp."""
        from mlsl_amd import ops
        rng = np.random.default_rng(count)
        wires = []
        for mul in (1.0, 7.0):
            v = (rng.standard_normal(count) * mul).astype(np.float32)
            d_w = _dev_bytes(0, (qr.wire_bytes(count, block), 0xAB))
            ops.quantize(torch.from_numpy(v).cuda(), d_w[:-GUARD], count, block=block,
                         dtype="f32")
            torch.cuda.synchronize()
            w = d_w.cpu().numpy()[:-GUARD]
            assert np.array_equal(w, qr.ref_wire(*qr.ref_quantize(v, block)))
            wires.append(w)
        a, b = wires
        acc = _accum_on_gpu(a, b, count, block)
        ns, word1, q = qr.parse_wire(acc, block)
        _, _, qa = qr.parse_wire(a, block)
        s, ssum = qr.exact_sums(a, b, count, block)

        nb = qr.nblocks(count, block)
        spad = np.zeros(nb * block)
        spad[:count] = s
        m = np.abs(spad).reshape(nb, block).max(axis=1)
        assert (m > 0).all()
        ref_ns = (m / 127.0).astype(np.float32)
        ulps = np.abs(ns.view(np.int32).astype(np.int64) - ref_ns.view(np.int32))
        print(f"header: max {ulps.max()} ulp from f32(max|s|/127)")
        assert ulps.max() <= 4, "block scales"
        assert not word1.view(np.uint32).any(), "reserved header word"
        assert np.array_equal(q.reshape(-1)[count:], qa.reshape(-1)[count:]), "padding"

        ns_e = np.repeat(ns.astype(np.float64), block)[:count]
        t = s / ns_e
        delta = 2.0 ** -20 * 127 * ssum / ns_e
        lo = np.floor(t)
        zone = np.abs(t - lo - 0.5) <= delta
        got = q.reshape(-1)[:count].astype(np.float64)
        exact = np.clip(np.rint(t), -127, 127)
        either = (got == np.clip(lo, -127, 127)) | (got == np.clip(lo + 1, -127, 127))
        bad = np.where(zone, ~either, got != exact)
        print(f"tie zone: {zone.mean() * 100:.4f} % of {count}; mismatches {bad.sum()}")
        assert zone.mean() <= 1e-3
        assert not bad.any(), f"{bad.sum()} payload bytes off"


def _cpu_reduce(a, b, op):
    return {"sum": a + b, "min": torch.minimum(a, b), "max": torch.maximum(a, b)}[op]


@requires_gpu
class TestReduceExact:
    def setup_method(self, _):
        torch.cuda.set_device(0)
        torch.manual_seed(4321)

    @staticmethod
    def _check(fn, a_cpu, b_cpu, want):
        # one guard element after dst: count, not the allocation, bounds it
        n = a_cpu.numel()
        a = torch.cat([a_cpu, a_cpu[:1]]).cuda()
        b = b_cpu.cuda()
        fn(a, b, n)
        torch.cuda.synchronize()
        assert torch.equal(a[:n].cpu(), want)
        assert torch.equal(a[n:].cpu(), a_cpu[:1]) and torch.equal(b.cpu(), b_cpu)

    @pytest.mark.parametrize("op", ["sum", "min", "max"])
    def test_f32_unrolled_loop(self, op):
        # ReduceF32Kernel<op, UNROLL2>: n/4 = 786433 vectors over 524288
        # threads and n*4 < 16 MiB, so the 2-deep loop, the single-vector
        # remainder loop and the scalar tail (1 element) all run
        from mlsl_amd import ops
        n = 3 * (1 << 20) + 5
        a, b = torch.randn(n), torch.randn(n)
        self._check(lambda x, y, k: ops.reduce_(x, y, k, dtype="f32", op=op), a, b,
                    _cpu_reduce(a, b, op))

    # ReduceF32Kernel<SUM, NT>: one block + tail of 3; 2048 blocks, 2 passes
    @pytest.mark.parametrize("n", [4099, (1 << 22) + 3])
    def test_reduce_nt(self, n):
        from mlsl_amd import ops
        a, b = torch.randn(n), torch.randn(n)
        self._check(ops.reduce_nt, a, b, a + b)

    # ReduceF32Kernel<SUM, NT2>: tail of 7; 655360 vector pairs over 524288
    # threads, so more than one grid-stride pass
    @pytest.mark.parametrize("n", [4103, 5 * (1 << 20) + 7])
    def test_reduce_nt2(self, n):
        from mlsl_amd import ops
        a, b = torch.randn(n), torch.randn(n)
        self._check(ops.reduce_nt2, a, b, a + b)

    @pytest.mark.parametrize("op", ["min", "max"])
    @pytest.mark.parametrize("name,dtype", [
        ("f16", torch.float16), ("f64", torch.float64), ("i32", torch.int32),
        ("i64", torch.int64), ("u8", torch.uint8)])
    def test_min_max_scalar_kernels(self, name, dtype, op):
        # ReduceScalarKernel<T, MIN/MAX>
        from mlsl_amd import ops
        n = 1027
        if dtype.is_floating_point:
            a, b = torch.randn(n).to(dtype), torch.randn(n).to(dtype)
        else:
            lo, hi = (0, 256) if dtype == torch.uint8 else (-(1 << 30), 1 << 30)
            a = torch.randint(lo, hi, (n,), dtype=dtype)
            b = torch.randint(lo, hi, (n,), dtype=dtype)
        self._check(lambda x, y, k: ops.reduce_(x, y, k, dtype=name, op=op), a, b,
                    _cpu_reduce(a, b, op))

    def test_u8_sum_wraps(self):
        from mlsl_amd import ops
        n = 1027
        a = torch.randint(0, 256, (n,), dtype=torch.uint8)
        b = torch.randint(0, 256, (n,), dtype=torch.uint8)
        a[:2], b[:2] = 255, torch.tensor([255, 1], dtype=torch.uint8)
        want = a + b  # modulo 256
        assert want[0] == 254 and want[1] == 0
        self._check(lambda x, y, k: ops.reduce_(x, y, k, dtype="u8", op="sum"), a, b, want)


@requires_gpu
class TestCopyExact:
    def setup_method(self, _):
        torch.cuda.set_device(0)

    @pytest.mark.parametrize("variant", ["copy", "plain"])
    @pytest.mark.parametrize("nbytes,offset", [
        (1 << 20, 0),           # CopyNTKernel: n16 == stride, single-pass loop only
        ((12 << 20) + 16, 0),   # CopyNTKernel: pair loop plus remainder loop
        ((1 << 20) + 4, 0),     # not a multiple of 16: hipMemcpyAsync
        (1 << 20, 4),           # both pointers 4 bytes off: hipMemcpyAsync
    ])
    def test_copy(self, nbytes, offset, variant):
        # "copy": LaunchCopy, CopyNTKernel<true>; "plain": CopyNTKernel<false>
        from mlsl_amd import ops
        rng = np.random.default_rng(nbytes + offset)
        data = rng.integers(0, 256, nbytes, dtype=np.uint8)
        front = GUARD + offset
        d_src = _dev_bytes(front, data)
        d_dst = _dev_bytes(front, (nbytes, 0xAB))
        src, dst = d_src[front:front + nbytes], d_dst[front:front + nbytes]
        if variant == "copy":
            ops.copy(dst, src, nbytes)
        else:
            ops.copy_variant(dst, src, nbytes, nt=False)
        torch.cuda.synchronize()
        pre, got, post = _split(d_dst, front, nbytes)
        assert np.array_equal(got, data)
        assert _intact(pre, post), "write outside the destination"
        assert np.array_equal(_split(d_src, front, nbytes)[1], data)
