"""DistributedData: DDP-style data-parallel wrapper over the mlsl_amd
engine — the "framework integration" role the reference played for
Caffe/Torch (MLSL is the comm library *under* a framework).

Usage (one process per GPU):

    model = Net().cuda()
    dd = DistributedData(model, dist)   # broadcasts initial params
    for batch in loader:
        loss = model(batch).sum()
        loss.backward()                  # hooks start bucketed allreduce
        dd.finish_gradients()            # waits + averages
        opt.step(); opt.zero_grad()

Gradients are bucketed (default 25 MiB) and allreduced non-blocking as
buckets fill during backward — the reference's Backward2/Update overlap
split, driven from torch autograd hooks.

With compression="int8" every f32 or bf16 bucket is one
mx.SegmentedAllReduce: the int8 wire's quantize pass reads the gradients
where they lie and its dequantize pass writes the averaged values back into
them, so there is no torch.cat, no divide and no copy-back, and
finish_gradients() only waits. The average is (q * scale) * (1/world), two
float32 roundings: the bits of a flat quantized allreduce of the bucket
multiplied by float32(1/world). Buckets of any other dtype keep the exact path. Call
close() to release the requests.

compression="int4" is the same on the 4-bit wire (block / 2 + 8 bytes a block
where int8 takes block + 8): the bits of a flat bits=4 request per bucket times
float32(1/world). It runs the two-shot all_reduce only, so ar_algo is None or
"two_shot" and the group has at most 8 ranks.

grads="in_place" (default "copy", the same pair of words as ShardedOptimizer)
gives every f32, bf16 or f16 bucket that has no compressed request one exact
mx.SegmentedAllReduce(compression=None): a kernel gathers the gradients into
the request's own flat buffer, the flat exact all_reduce runs on it, and a
second kernel writes sum * float32(1/world) back into them, so again no
torch.cat, no divide, no per-parameter copy, and finish_gradients() only
waits. Each such bucket keeps a bucket-sized buffer for the wrapper's
lifetime; gradients must be contiguous. The result is the flat request's sum
times float32(1/world), where the default path divides by world.
"""
import torch

import mlsl_amd as mx
from mlsl_amd import ops


class DistributedData:
    def __init__(self, module, dist=None, bucket_mb=25, group="data",
                 average=True, compression=None, ar_algo=None, grads="copy"):
        if compression not in (None, "int8", "int4"):
            raise ValueError(f"compression={compression!r}: expected None, 'int8' or 'int4'")
        if ar_algo is not None and compression is None:
            raise ValueError("ar_algo= selects the quantized all_reduce's algorithm: "
                             "it needs compression='int8' or 'int4'")
        if compression == "int4" and ar_algo == "ring":
            raise ValueError("compression='int4' does not run ar_algo='ring': the ring "
                             "requantizes the partial sum on every hop, which at 4 bits "
                             "loses far more than at 8; name 'two_shot' or nothing")
        if grads not in ("copy", "in_place"):
            raise ValueError(f"grads={grads!r}: expected 'copy' or 'in_place'")
        self.compression = compression
        self.grads = grads
        self.module = module
        self.dist = dist or mx.Distribution(mx.world_size(), 1)
        self.group = group
        self.world = self.dist.process_count(group)
        self.average = average
        self.bucket_bytes = bucket_mb * 1024 * 1024
        self._params = [p for p in module.parameters() if p.requires_grad]
        if torch.cuda.is_available():
            mx.set_compute_stream(torch.cuda.current_stream().cuda_stream)

        # broadcast initial parameters from rank 0 (reference test protocol,
        # mlsl_test.cpp:651-652)
        if self.world > 1:
            for p in self._params:
                flat = p.data.contiguous().view(-1)
                mx.wait(self.dist.bcast(flat, flat.numel(), root=0,
                                        dtype=_dt(p), group=group))
                with torch.no_grad():
                    p.data.copy_(flat.view_as(p.data))

        # bucket assignment in reverse parameter order (grads arrive
        # roughly back-to-front during backward), partitioned by dtype: a
        # bucket must be dtype-uniform because torch.cat would silently
        # promote mixed grads while the allreduce dtype comes from one
        # member param (torch DDP keys its buckets the same way)
        self._buckets = []
        cur, cur_bytes, cur_dtype = [], 0, None
        for p in reversed(self._params):
            if cur and p.dtype != cur_dtype:
                self._buckets.append(cur)
                cur, cur_bytes = [], 0
            cur_dtype = p.dtype
            cur.append(p)
            cur_bytes += p.numel() * p.element_size()
            if cur_bytes >= self.bucket_bytes:
                self._buckets.append(cur)
                cur, cur_bytes = [], 0
        if cur:
            self._buckets.append(cur)
        self._param_bucket = {}
        for bi, ps in enumerate(self._buckets):
            for p in ps:
                self._param_bucket[id(p)] = bi
        self._pending = [0] * len(self._buckets)
        self._reqs = [None] * len(self._buckets)
        self._flat = [None] * len(self._buckets)
        # one request over the bucket's gradient list: compressed for f32/bf16
        # buckets, exact with grads="in_place" for what is left of f32/bf16/f16;
        # None marks a bucket on the cat path
        self._seg = [None] * len(self._buckets)
        if compression is not None and self.world > 1:
            for bi, ps in enumerate(self._buckets):
                if ps[0].dtype in (torch.float32, torch.bfloat16):
                    self._seg[bi] = mx.SegmentedAllReduce(
                        self.dist, [q.numel() for q in ps], dtype=_dt(ps[0]),
                        group=group, ar_algo=ar_algo, compression=compression,
                        post_scale=1.0 / self.world if average else 1.0)
        if grads == "in_place" and self.world > 1:
            for bi, ps in enumerate(self._buckets):
                if self._seg[bi] is None and ps[0].dtype in (torch.float32, torch.bfloat16,
                                                             torch.float16):
                    self._seg[bi] = mx.SegmentedAllReduce(
                        self.dist, [q.numel() for q in ps], dtype=_dt(ps[0]), group=group,
                        compression=None, post_scale=1.0 / self.world if average else 1.0)

        # clip_grad_norm_: the squared norm on the device, and per dtype the
        # device segment tables of the gradients with the addresses they hold
        self._clip_total = None
        self._clip_tables = {}
        self.clip_table_uploads = 0

        for p in self._params:
            p.register_post_accumulate_grad_hook(self._hook)
        self._reset_counts()

    def _reset_counts(self):
        for bi, ps in enumerate(self._buckets):
            self._pending[bi] = len(ps)

    def _hook(self, p):
        if self.world <= 1:
            return
        bi = self._param_bucket[id(p)]
        self._pending[bi] -= 1
        if self._pending[bi] == 0:
            ps = self._buckets[bi]
            if self._seg[bi] is not None:
                grads = [q.grad for q in ps]
                for q, g in zip(ps, grads):
                    if not g.is_contiguous():
                        raise ValueError(
                            f"{self._in_place_why()} reduces gradients in place "
                            f"and needs them contiguous: the gradient of a parameter of shape "
                            f"{tuple(q.shape)} has strides {g.stride()}")
                self._seg[bi].start(grads)
                self._reqs[bi] = self._seg[bi]
                return
            flat = torch.cat([q.grad.detach().reshape(-1) for q in ps])
            self._flat[bi] = flat
            self._reqs[bi] = self.dist.all_reduce(flat, flat, flat.numel(),
                                                  op="sum", dtype=_dt(p),
                                                  group=self.group)

    def _in_place_why(self):
        return f"compression={self.compression!r}" if self.compression is not None \
            else "grads='in_place'"

    def finish_gradients(self):
        """Wait all bucket allreduces and scatter averaged grads back."""
        if self.world <= 1:
            return
        for bi, ps in enumerate(self._buckets):
            if self._reqs[bi] is None:
                continue
            if self._seg[bi] is not None:
                # summed, scaled and written back by the request's finish
                self._seg[bi].wait()
                self._reqs[bi] = None
                continue
            mx.wait(self._reqs[bi])
            flat = self._flat[bi]
            if self.average:
                flat /= self.world
            off = 0
            for q in ps:
                n = q.grad.numel()
                q.grad.copy_(flat[off:off + n].view_as(q.grad))
                off += n
            self._reqs[bi] = None
            self._flat[bi] = None
        self._reset_counts()

    def clip_grad_norm_(self, max_norm):
        """torch.nn.utils.clip_grad_norm_ (L2) for the wrapped module, called
        after finish_gradients(): the reduced gradients are the same on every
        rank, so nothing is exchanged. On the device the gradients are grouped
        by dtype (f32, bf16, f16) and each group is one launch over a segment
        table: ops.sumsq_list adds every group's squares into one float64 scalar,
        ops.clip_scale_list scales each group by min(1, max_norm / (norm +
        1e-6)) read from that scalar. A group's device tables are kept and
        uploaded again only when a gradient's address has changed. Returns the
        norm before clipping as a 0-dim float64 tensor on the gradients' device;
        nothing is read back. Gradients must be contiguous. CPU gradients take
        the same steps as torch operations in float64."""
        max_norm = float(max_norm)
        if not (0.0 < max_norm < float("inf")):
            raise ValueError(f"max_norm={max_norm!r}: expected a positive finite number")
        groups = {}
        for p in self._params:
            g = p.grad
            if g is None or g.numel() == 0:
                continue
            if not g.is_contiguous():
                raise ValueError(
                    f"clip_grad_norm_ scales gradients in place and needs them contiguous: "
                    f"the gradient of a parameter of shape {tuple(p.shape)} has strides "
                    f"{g.stride()}")
            groups.setdefault(g.dtype, []).append(g)
        if not groups:
            return torch.zeros((), dtype=torch.float64)
        first = next(iter(groups.values()))[0]
        if not first.is_cuda:
            total = sum(g.double().square().sum() for gs in groups.values() for g in gs)
            factor = torch.clamp(max_norm / (total.sqrt() + 1e-6), max=1.0).to(torch.float32)
            for gs in groups.values():
                for g in gs:
                    g.mul_(factor)
            return total.sqrt()
        if self._clip_total is None:
            self._clip_total = torch.zeros(1, dtype=torch.float64, device=first.device)
        tabs = [(_dt(gs[0]), self._clip_table(dt, gs)) for dt, gs in groups.items()]
        for i, (dt, (ptrs, offs, nseg, count)) in enumerate(tabs):
            ops.sumsq_list_tables(ptrs, offs, nseg, count, self._clip_total, dtype=dt,
                                  accumulate=i > 0)
        for dt, (ptrs, offs, nseg, count) in tabs:
            ops.clip_scale_list_tables(ptrs, offs, nseg, count, self._clip_total, max_norm,
                                       dtype=dt)
        return self._clip_total.sqrt().reshape(())

    def _clip_table(self, dtype, grads):
        """(device pointers, device prefix offsets, nseg, count) of one dtype's
        gradients, from the cache while their addresses and sizes are the same."""
        key = tuple((g.data_ptr(), g.numel()) for g in grads)
        hit = self._clip_tables.get(dtype)
        if hit is None or hit[0] != key:
            offs = [0]
            for _, n in key:
                offs.append(offs[-1] + n)
            dev = grads[0].device
            hit = (key, (torch.tensor([a for a, _ in key], dtype=torch.int64, device=dev),
                         torch.tensor(offs, dtype=torch.int64, device=dev), len(key), offs[-1]))
            self._clip_tables[dtype] = hit
            self.clip_table_uploads += 1
        return hit[1]

    def close(self):
        """Destroy the buckets' list requests, compressed or exact (none in
        flight)."""
        for bi, r in enumerate(self._seg):
            if r is not None:
                r.destroy()
                self._seg[bi] = None


def _dt(p):
    return {torch.float32: "f32", torch.float64: "f64",
            torch.bfloat16: "bf16", torch.float16: "f16"}[p.dtype]
