"""Clipping by the global norm on one device: the kernels and their two consumers."""
import math

import numpy as np
import pytest
import torch

from tests import workers_clip as wc

pytestmark = pytest.mark.gpu
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
BITS = {"f32": torch.int32, "bf16": torch.int16, "f16": torch.int16}
SENT = 77.0


def layouts(dtype):
    """name -> (counts, elements every tensor starts past a 16-byte boundary)."""
    from mlsl_amd import ops
    g = 16 // TORCH_DT[dtype].itemsize          # elements of one 16-byte vector
    tile, trip = 256 * g, ops.list_elems_per_trip(dtype)
    return {"one": ([1], 0), "vec": ([g], 0), "vec-1": ([g - 1], 0), "vec+1": ([g + 1], 0),
            "unaligned": ([3 * g + 2], 1), "tile+1": ([tile + 1], 0),
            "3 workgroups": ([12 * tile + 5], 0), "257 workgroups": ([1028 * tile + 3], 0),
            "second trip": ([trip + 1], 0),
            "tile edges": ([tile, tile + 1, 7], 0), "all unaligned": ([5 * g + 3] * 4, 1),
            "lane walk": (np.random.default_rng(7).integers(1, 4, 700).tolist(), 0),
            "trip inside a segment": ([100, trip + 100], 0)}


def build(dtype, name):
    """(buffer on the device, its tensors as views, their float64 values).
    Around every tensor the buffer holds sentinels: at least a vector each side.
    Magnitudes are uniform in [0.25, 4), so a clipped value stays a normal number
    of f16, which a relative bound presupposes; a tensor's last element is -0.0.
    Layouts of 2**16 elements and more hold quarter integers: their squares add
    up exactly in any order, so the plain float64 sum is what math.fsum gives."""
    counts, off = layouts(dtype)[name]
    g = 16 // TORCH_DT[dtype].itemsize
    gen = torch.Generator().manual_seed(len(counts) + counts[0])
    parts, spans, pos = [], [], 0
    for n in counts:
        x = ((torch.rand(n, generator=gen) * 3.75 + 0.25)
             * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1) if sum(counts) < 2 ** 16
             else torch.randint(-16, 17, (n,), generator=gen) / 4).to(TORCH_DT[dtype])
        x[-1] = -0.0 if n > 1 else x[-1]
        pad = g + (-(off + n)) % g
        parts += [torch.full((g + off,), SENT, dtype=x.dtype), x,
                  torch.full((pad,), SENT, dtype=x.dtype)]
        spans.append((pos + g + off, n))
        pos += g + off + n + pad
    buf = torch.cat(parts).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, [buf[a:a + n] for a, n in spans], torch.cat(parts[1::3]).double().numpy()


@pytest.mark.parametrize("name", list(layouts("f32")))
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_sumsq_and_clip_scale(dtype, name):
    from mlsl_amd import ops   # list forms; one-tensor layouts the flat forms too
    buf, views, vals = build(dtype, name)
    counts, before, max_norm = [v.numel() for v in views], buf.clone(), 1.5
    unchanged = lambda: torch.equal(buf.view(BITS[dtype]), before.view(BITS[dtype]))  # noqa: E731
    ref = math.fsum((vals * vals).tolist()) if vals.size < 2 ** 16 else float((vals * vals).sum())
    sums = [lambda out, acc: ops.sumsq_list(views, counts, out, accumulate=acc),
            lambda out, acc: ops.sumsq(views[0], counts[0], out, accumulate=acc)]
    clips = [lambda tot: ops.clip_scale_list(views, counts, tot, max_norm),
             lambda tot: ops.clip_scale(views[0], counts[0], tot, max_norm)]
    for run in sums[:1 + (len(counts) == 1)]:
        box = torch.tensor([SENT, float("nan"), SENT], dtype=torch.float64).cuda()
        run(box[1:2], False)                     # assigns over the poison
        got = box.cpu().tolist()
        assert abs(got[1] - ref) <= vals.size * 2.0 ** -52 * ref and got[0] == SENT == got[2]
        run(box[1:2], True)                      # the same bits again, onto a non-zero out
        assert box.cpu().tolist() == [SENT, 2 * got[1], SENT] and unchanged()
    for run in clips[:1 + (len(counts) == 1)]:
        for total in (1.0, 0.0, 37.0):
            buf.copy_(before)
            run(torch.tensor([total], dtype=torch.float64).cuda())
            c = wc.coeff(total, max_norm)
            if c == 1.0:                         # nothing moves, -0.0 and sentinels included
                assert unchanged()
                continue
            err = np.abs(torch.cat(views).double().cpu().numpy() - vals * c)
            assert (err <= wc.TOL[dtype] * np.abs(vals * c)).all(), float(err.max())
            for v in views:                      # with the tensors painted over, nothing
                v.fill_(SENT)                    # but sentinels is left: no write outside
            assert (buf == SENT).all()


def test_sumsq_squares_past_f32():
    from mlsl_amd import ops
    x, out = torch.full((1000,), 1e25).cuda(), torch.zeros(1, dtype=torch.float64).cuda()
    ops.sumsq(x, 1000, out)
    ref = 1000 * float(np.float32(1e25)) ** 2   # finite in f64 alone
    assert abs(out.item() - ref) <= 1000 * 2.0 ** -52 * ref


def test_refusals():
    from mlsl_amd import MlslError, ops
    out, x = torch.zeros(1, dtype=torch.float64).cuda(), torch.ones(8).cuda()
    for exc, text, call in (
            (MlslError, "supports f32/bf16/f16 only", lambda: ops.sumsq(x.double(), 8, out)),
            (MlslError, "supports f32/bf16/f16 only",
             lambda: ops.clip_scale_list([x.double()], [8], out, 1.0)),
            (ValueError, "empty", lambda: ops.sumsq_list([], [], out)),
            (ValueError, "at least one element", lambda: ops.clip_scale_list([x], [0], out, 1.0)),
            (MlslError, "at least one element", lambda: ops.sumsq(x, 0, out))):
        with pytest.raises(exc, match=text):
            call()


@pytest.mark.parametrize("world,max_norm,kw", [
    (1, 1.0, {}), (1, 1e6, {}), (2, 1.0, {}), (2, 1e6, {}), (4, 1.0, {}), (4, 1e6, {}),
    (2, 1.0, {"compression": "int8", "grads": "in_place"})])
def test_sharded_optimizer_clips(world, max_norm, kw):
    wc.run_ranks("zero1_clip", world, device=True, max_norm=max_norm, **kw)


@pytest.mark.parametrize("world,grads", [(1, "copy"), (2, "in_place")])
def test_ddp_clip_grad_norm(world, grads):
    wc.run_ranks("ddp_clip", world, device=True, grads=grads)
