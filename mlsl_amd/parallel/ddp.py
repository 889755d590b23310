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
"""
import torch

import mlsl_amd as mx


class DistributedData:
    def __init__(self, module, dist=None, bucket_mb=25, group="data",
                 average=True, compression=None, ar_algo=None):
        if compression not in (None, "int8"):
            raise ValueError(f"compression={compression!r}: expected None or 'int8'")
        if ar_algo is not None and compression is None:
            raise ValueError("ar_algo= selects the quantized all_reduce's algorithm: "
                             "it needs compression='int8'")
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
        # compression="int8": one request over the bucket's gradient list per
        # f32/bf16 bucket; None marks a bucket on the exact path
        self._seg = [None] * len(self._buckets)
        if compression == "int8" and self.world > 1:
            for bi, ps in enumerate(self._buckets):
                if ps[0].dtype in (torch.float32, torch.bfloat16):
                    self._seg[bi] = mx.SegmentedAllReduce(
                        self.dist, [q.numel() for q in ps], dtype=_dt(ps[0]),
                        group=group, ar_algo=ar_algo,
                        post_scale=1.0 / self.world if average else 1.0)

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
                            "compression='int8' reduces gradients in place and needs "
                            f"them contiguous: the gradient of a parameter of shape "
                            f"{tuple(q.shape)} has strides {g.stride()}")
                self._seg[bi].start(grads)
                self._reqs[bi] = self._seg[bi]
                return
            flat = torch.cat([q.grad.detach().reshape(-1) for q in ps])
            self._flat[bi] = flat
            self._reqs[bi] = self.dist.all_reduce(flat, flat, flat.numel(),
                                                  op="sum", dtype=_dt(p),
                                                  group=self.group)

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

    def close(self):
        """Destroy the compressed buckets' requests (none in flight)."""
        for bi, r in enumerate(self._seg):
            if r is not None:
                r.destroy()
                self._seg[bi] = None


def _dt(p):
    return {torch.float32: "f32", torch.float64: "f64",
            torch.bfloat16: "bf16", torch.float16: "f16"}[p.dtype]
