"""ShardedOptimizer: ZeRO-1-style distributed weight update over the
mlsl_amd engine — the torch-level face of the reference's
``distributedUpdate`` ParameterSets (include/mlsl.hpp:306-339,
src/mlsl_impl.cpp:401-435): gradients are reduce-scattered so each data-
parallel rank owns ``1/dp`` of every flat parameter group, the wrapped
optimizer steps only on the owned shard, and the updated shard is
all-gathered back (the reference's StartIncrementComm/WaitIncrementComm
AllGather).

Optimizer state (momentum, Adam moments) therefore lives only for the
owned shard on each rank: state memory scales 1/dp.

Usage (one process per GPU):

    model = Net().cuda()
    dd = DistributedData(model, dist)           # grads stay full-size
    sopt = ShardedOptimizer(model.parameters(), torch.optim.AdamW,
                            dist, lr=1e-3)
    for batch in loader:
        loss = model(batch); loss.backward()
        dd.finish_gradients()                   # averaged full grads
        sopt.step()                             # RS -> shard step -> AG
        sopt.zero_grad()

``ShardedOptimizer`` can also run WITHOUT a DDP wrapper: pass
``reduce="rs"`` and it replaces the gradient allreduce entirely —
reduce_scatter(grad) + sharded step + all_gather(param), one exchange of
each flat buffer per step (the reference's grad RS + increment AG pair).
With ``compression="int8"`` that reduce_scatter travels as int8 wire blocks
with error feedback (one persistent request, so the residual carries over
from step to step). The parameter all_gather is exact unless
``ag_compression="int8"`` is given: see the class.
With ``grads="in_place"`` on top of that the int8 wire is built straight from
the gradients where they lie (one ``mx.SegmentedReduceScatter`` over
``[p.grad ...]``): the flat gradient buffer, as large as the model, and the
copy of every gradient into it are gone.
"""
import torch

import mlsl_amd as mx


def _dt(t):
    return {torch.float32: "f32", torch.float64: "f64",
            torch.bfloat16: "bf16", torch.float16: "f16"}[t.dtype]


class ShardedOptimizer:
    """``ag_compression="int8"`` sends the updated shard back as int8 too.

    Sending int8 *parameters* would cap every weight at 8 bits, so the
    difference between the owner's exact shard and the replica travels
    instead, and is accumulated:

    - The owner keeps ``master``, a clone of its shard in the parameter dtype;
      the wrapped optimizer's parameter and its state live on ``master``.
      ``flat`` and the model's views are the replica on every rank, the owner
      included.
    - After ``opt.step()``, ``delta = master - flat[own]`` goes through one
      persistent ``all_gather(quantized=True, accumulate=True)`` with
      ``recv=flat``. Every rank applies the same fma to every segment, its own
      included, so the replicas stay bit-identical across ranks.
    - What a step's quantization drops (at most half a step of the block,
      ``max|delta| / 254``, per element) is still in ``master - replica`` at
      the next step: the scheme corrects itself, which is why the request
      carries no residual of its own.

    It needs f32 or bf16 parameters, is independent of ``reduce``,
    ``compression`` and ``rs_algo``, and costs one extra shard (``master``)
    and one delta shard per rank. A group of one exchanges nothing and steps
    on ``flat`` as without it. A model checkpoint holds replica values; a
    newly constructed optimizer seeds ``master`` from them.
    """

    def __init__(self, params, opt_cls, dist=None, group="data",
                 reduce="none", average=True, compression="none", rs_algo=None,
                 ag_compression="none", grads="copy", **opt_kwargs):
        """reduce: "none" (grads already reduced, e.g. by DistributedData)
        or "rs" (this wrapper reduce-scatters raw local grads itself).
        compression: "none", or "int8" for the quantized reduce_scatter
        (needs reduce="rs" and f32 or bf16 parameters; block size from
        mx.set_quant_params). A group of one exchanges nothing either way.
        rs_algo: algorithm of that quantized reduce_scatter: None
        (MLSL_QUANT_RS_ALGO, ring unless set), "ring", or "direct" (each shard
        goes straight to its owner and is summed once, nothing requantized;
        at most 8 ranks, N-1 shard-wires of scratch instead of 2).
        ag_compression: "none" (exact parameter all_gather), or "int8": the
        quantized, accumulating all_gather of master - replica described in
        the class docstring (f32 or bf16 parameters).
        grads: "copy" gathers every gradient into one flat buffer as large as
        the parameters (``flat_grad``) before it is reduced. "in_place" (needs
        reduce="rs" and compression="int8"; any rs_algo and ag_compression)
        keeps no such buffer at world > 1: the quantized reduce_scatter reads
        the gradients where they lie and leaves the owned shard in
        ``own_grad``, a tensor of its own. The parameters' bits are those of
        "copy". A parameter without a gradient counts as zeros (one cached
        zeros_like per such parameter) and a non-contiguous gradient goes
        through .contiguous(). On a group of one nothing changes."""
        self.params = [p for p in params if p.requires_grad]
        assert self.params, "no trainable parameters"
        self.dist = dist or mx.Distribution(mx.world_size(), 1)
        self.group = group
        self.world = self.dist.process_count(group)
        self.rank = self.dist.process_idx(group)
        self.average = average
        assert reduce in ("none", "rs")
        self.reduce = reduce
        if compression not in ("none", "int8"):
            raise ValueError(f"compression={compression!r}: expected 'none' or 'int8'")
        if compression == "int8" and reduce != "rs":
            raise ValueError('compression="int8" compresses the gradient '
                             'reduce_scatter: it needs reduce="rs"')
        self.compression = compression
        if rs_algo not in (None, "ring", "direct"):
            raise ValueError(f"rs_algo={rs_algo!r}: expected None, 'ring' or 'direct'")
        if rs_algo is not None and compression != "int8":
            raise ValueError('rs_algo= selects the quantized reduce_scatter\'s '
                             'algorithm: it needs compression="int8"')
        self.rs_algo = rs_algo
        if ag_compression not in ("none", "int8"):
            raise ValueError(f"ag_compression={ag_compression!r}: expected 'none' or 'int8'")
        self.ag_compression = ag_compression
        if grads not in ("copy", "in_place"):
            raise ValueError(f"grads={grads!r}: expected 'copy' or 'in_place'")
        if grads == "in_place" and reduce != "rs":
            raise ValueError('grads="in_place" reads the gradients in the reduce_scatter: '
                             'it needs reduce="rs"')
        if grads == "in_place" and compression != "int8":
            raise ValueError('grads="in_place" builds the int8 wire from the gradients: '
                             'it needs compression="int8"')
        self.grads = grads

        if torch.cuda.is_available() and self.params[0].is_cuda:
            mx.set_compute_stream(torch.cuda.current_stream().cuda_stream)
        dev = self.params[0].device
        dt = self.params[0].dtype
        assert all(p.dtype == dt for p in self.params), \
            "one flat group: uniform dtype required"
        if compression == "int8" and dt not in (torch.float32, torch.bfloat16):
            raise ValueError(f'compression="int8" supports f32/bf16 parameters, not {dt}')
        if ag_compression == "int8" and dt not in (torch.float32, torch.bfloat16):
            raise ValueError(f'ag_compression="int8" supports f32/bf16 parameters, not {dt}')
        total = sum(p.numel() for p in self.params)
        # pad so the shard divides evenly (owned = ceil math in the
        # reference, mlsl_impl.cpp:401-411; padding is the flat analog)
        self.shard = (total + self.world - 1) // self.world
        self.flat = torch.zeros(self.shard * self.world, dtype=dt, device=dev)
        self._in_place = grads == "in_place" and self.world > 1
        if not self._in_place:
            self.flat_grad = torch.zeros_like(self.flat)
        # map parameters onto the flat buffer (they become views)
        off = 0
        with torch.no_grad():
            for p in self.params:
                n = p.numel()
                self.flat[off:off + n].copy_(p.data.reshape(-1))
                p.data = self.flat[off:off + n].view_as(p.data)
                off += n
        lo = self.rank * self.shard
        self.own_param = self.flat[lo:lo + self.shard]
        self.own_grad = (torch.zeros(self.shard, dtype=dt, device=dev) if self._in_place
                         else self.flat_grad[lo:lo + self.shard])
        # int8 all_gather: the optimizer steps on an exact copy of the shard
        # and flat is the replica everywhere; built once, like _qrs
        self.master = self._delta = self._qag = None
        if ag_compression == "int8" and self.world > 1:
            self.master = self.own_param.detach().clone()
            self._delta = torch.zeros_like(self.master)
            self._qag = mx.PersistentRequest(self.dist, "all_gather", self.shard,
                                             dtype=_dt(self.flat), group=group,
                                             quantized=True, accumulate=True)
        # the wrapped optimizer sees ONLY the owned shard (state: 1/dp)
        shard_param = torch.nn.Parameter(
            self.own_param if self.master is None else self.master, requires_grad=False)
        self._shard_holder = shard_param
        self.opt = opt_cls([shard_param], **opt_kwargs)
        # built once: the request owns the error-feedback residual
        self._qrs = None
        self._qrs_seg = None
        self._zero_grads = {}
        if self._in_place:
            self._qrs_seg = mx.SegmentedReduceScatter(
                self.dist, [p.numel() for p in self.params], shard=self.shard,
                dtype=_dt(self.flat), group=group, algo=rs_algo)
        elif compression == "int8" and self.world > 1:
            self._qrs = mx.PersistentRequest(self.dist, "reduce_scatter", self.shard,
                                             dtype=_dt(self.flat), op="sum",
                                             group=group, quantized=True,
                                             algo=rs_algo)

    def _grad_list(self):
        """The gradients as the list request reads them: contiguous, zeros
        where a parameter has none. The list keeps any copy alive until the
        request has been waited for."""
        out = []
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                g = self._zero_grads.get(i)
                if g is None:
                    g = self._zero_grads[i] = torch.zeros_like(
                        p.data, memory_format=torch.contiguous_format)
            else:
                g = g.detach().contiguous()
            out.append(g)
        return out

    def _gather_grads(self):
        off = 0
        for p in self.params:
            n = p.numel()
            g = p.grad
            if g is None:
                self.flat_grad[off:off + n].zero_()
            else:
                self.flat_grad[off:off + n].copy_(g.detach().reshape(-1))
            off += n
        self.flat_grad[off:].zero_()

    def step(self):
        if self._qrs_seg is not None:
            grads = self._grad_list()
            self._qrs_seg.start(grads, self.own_grad)
            self._qrs_seg.wait()
            del grads
            if self.average:
                self.own_grad /= self.world
        elif self.world > 1:
            self._gather_grads()
            if self._qrs is not None:
                # in place: every segment is on the wire before the owned
                # shard is written
                self._qrs.start(self.flat_grad, self.own_grad)
                self._qrs.wait()
            elif self.reduce == "rs":
                # raw local grads -> reduce_scatter into the owned shard
                mx.wait(self.dist.reduce_scatter(
                    self.flat_grad, self.own_grad, self.shard, op="sum",
                    dtype=_dt(self.flat), group=self.group))
            else:
                # grads already reduced everywhere: owned slice is ready
                self.own_grad.copy_(
                    self.flat_grad[self.rank * self.shard:
                                   (self.rank + 1) * self.shard])
            if self.average and self.reduce == "rs":
                self.own_grad /= self.world
        else:
            self._gather_grads()
            self.own_grad.copy_(self.flat_grad[:self.shard])

        self._shard_holder.grad = self.own_grad
        self.opt.step()
        self._shard_holder.grad = None

        if self._qag is not None:
            # what the replica lacks, last step's rounding included, as int8;
            # every rank adds every segment the same way
            torch.sub(self.master, self.own_param, out=self._delta)
            self._qag.start(self._delta, self.flat)
            self._qag.wait()
        elif self.world > 1:
            # increment AllGather (reference StartIncrementComm):
            # every rank's updated shard -> full parameter buffer
            mx.wait(self.dist.all_gather(self.own_param, self.shard,
                                         self.flat, dtype=_dt(self.flat),
                                         group=self.group))

    def zero_grad(self, set_to_none=False):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def state_dict(self):
        return self.opt.state_dict()

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd)
