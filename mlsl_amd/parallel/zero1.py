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
``ag_compression="int8"`` or ``"int4"`` is given: see the class.
With ``grads="in_place"`` on top of that the int8 wire is built straight from
the gradients where they lie (one ``mx.SegmentedReduceScatter`` over
``[p.grad ...]``): the flat gradient buffer, as large as the model, and the
copy of every gradient into it are gone. The int4 wire is built the same way
with ``compression="int4", grads="in_place", rs_algo="direct"``.
"""
import torch

import mlsl_amd as mx
from mlsl_amd import ops


def _dt(t):
    return {torch.float32: "f32", torch.float64: "f64",
            torch.bfloat16: "bf16", torch.float16: "f16"}[t.dtype]


def _np(t):
    """A CPU tensor's memory as the numpy array the host kernels take: 16-bit
    floats as their uint16 bit patterns."""
    return (t if t.dtype == torch.float32 else t.view(torch.int16)).numpy()


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

    ``ag_compression="int4"`` is the same scheme on the 4-bit wire (block/2 + 8
    bytes per block where int8 takes block + 8): ``scale = max|delta| / 7``,
    so a step drops at most ``max|delta| / 14`` per element of a block. With
    no new gradient the replica's distance to ``master`` so shrinks by 14x
    per step where int8's shrinks by 254x, down to the rounding of the
    replica's own dtype. With ``compression="int4"`` both of a step's
    exchanges then travel at 4 bits.

    Either needs f32 or bf16 parameters, is independent of ``reduce``,
    ``compression``, ``rs_algo`` and ``grads``, and costs one extra shard (``master``)
    and one delta shard per rank. A group of one exchanges nothing and steps
    on ``flat`` as without it. A model checkpoint holds replica values; a
    newly constructed optimizer seeds ``master`` from them.

    ``opt_cls="adamw"`` (a string in place of the optimizer class, with ``lr``,
    ``betas``, ``eps``, ``weight_decay``) steps with this project's fused
    kernel, ``ops.adamw_step``, instead of a torch optimizer. The owner keeps
    ``master``, ``exp_avg`` and ``exp_avg_sq`` in float32 whatever the
    parameter dtype, 12 bytes per owned element, and one launch does the
    averaging, the clip's scaling, AdamW and the rounding of the new
    parameter into ``flat`` (or, under ``ag_compression``, of ``master -
    replica`` into the delta). ``lr`` is a plain attribute read at every
    step. For f32 parameters without ``ag_compression`` ``master`` is the
    owned slice of ``flat`` itself where that slice is 16-byte aligned.
    """

    def __init__(self, params, opt_cls, dist=None, group="data",
                 reduce="none", average=True, compression="none", rs_algo=None,
                 ag_compression="none", grads="copy", max_grad_norm=None, **opt_kwargs):
        """reduce: "none" (grads already reduced, e.g. by DistributedData)
        or "rs" (this wrapper reduce-scatters raw local grads itself).
        compression: "none", or "int8" for the quantized reduce_scatter
        (needs reduce="rs" and f32 or bf16 parameters; block size from
        mx.set_quant_params). A group of one exchanges nothing either way.
        "int4" is that reduce_scatter on the 4-bit wire (about half the wire
        bytes, 15 levels per block instead of 255, the error fed back the
        same way): PersistentRequest(..., bits=4) on the grads="copy" path.
        It runs "direct" only: rs_algo may be None or "direct" and "ring" is
        refused; the block size must be a multiple of 8. With
        grads="in_place" the rule is: at 4 bits the in-place path runs direct
        only, and the caller names the algorithm. rs_algo="direct" creates
        SegmentedReduceScatter(compression="int4", algo="direct"), which from
        there behaves as the int8 in-place path does; rs_algo=None is
        refused.
        rs_algo: algorithm of that quantized reduce_scatter: None
        (MLSL_QUANT_RS_ALGO, ring unless set), "ring", or "direct" (each shard
        goes straight to its owner and is summed once, nothing requantized;
        at most 8 ranks, N-1 shard-wires of scratch instead of 2).
        ag_compression: "none" (exact parameter all_gather), or "int8": the
        quantized, accumulating all_gather of master - replica described in
        the class docstring (f32 or bf16 parameters). "int4" is that
        all_gather on the 4-bit wire, PersistentRequest(..., accumulate=True,
        bits=4): about half the wire bytes, any number of ranks, the block
        size a multiple of 8.
        grads: "copy" gathers every gradient into one flat buffer as large as
        the parameters (``flat_grad``) before it is reduced. "in_place" (needs
        reduce="rs" and compression="int8", any rs_algo, or compression="int4"
        with rs_algo="direct"; any ag_compression)
        keeps no such buffer at world > 1: the quantized reduce_scatter reads
        the gradients where they lie and leaves the owned shard in
        ``own_grad``, a tensor of its own. The parameters' bits are those of
        "copy". A parameter without a gradient counts as zeros (one cached
        zeros_like per such parameter) and a non-contiguous gradient goes
        through .contiguous(). On a group of one nothing changes.
        max_grad_norm: None, or a positive finite number: step() clips the
        reduced (and averaged) gradient by its global L2 norm before the
        optimizer sees it, with torch.nn.utils.clip_grad_norm_'s coefficient
        min(1, max_grad_norm / (norm + 1e-6)). Under reduce="rs" no rank holds
        the reduced gradient, so clipping p.grad from outside would clip the
        local, unreduced one; here every rank sums the squares of its own_grad
        shard in float64 on the device (padding is zeros and adds nothing), one
        exact f64 all_reduce of that scalar gives every rank the squared norm,
        and each rank scales its own shard. Nothing is read back: ``grad_norm``
        is a device tensor, the norm before clipping. From three ranks on the
        f64 all_reduce may add in a different order on each rank, so the ranks'
        norms can differ in the last bit; each rank scales only its own shard
        and the parameters travel by all_gather, so the replicas still agree
        bit for bit. Parameters must be f32, bf16 or f16. CPU tensors take the
        same three steps as torch operations in float64."""
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (0.0 < max_grad_norm < float("inf")):
                raise ValueError(f"max_grad_norm={max_grad_norm!r}: expected None or a "
                                 "positive finite number")
        self._fused = isinstance(opt_cls, str)
        if self._fused and opt_cls != "adamw":
            raise ValueError(f"opt_cls={opt_cls!r}: the only built-in optimizer is 'adamw'; "
                             "anything else is passed as a torch optimizer class")
        self.max_grad_norm = max_grad_norm
        self.params = [p for p in params if p.requires_grad]
        assert self.params, "no trainable parameters"
        self.dist = dist or mx.Distribution(mx.world_size(), 1)
        self.group = group
        self.world = self.dist.process_count(group)
        self.rank = self.dist.process_idx(group)
        self.average = average
        assert reduce in ("none", "rs")
        self.reduce = reduce
        if compression not in ("none", "int8", "int4"):
            raise ValueError(f"compression={compression!r}: expected 'none', 'int8' or "
                             "'int4'")
        if compression != "none" and reduce != "rs":
            raise ValueError(f'compression="{compression}" compresses the gradient '
                             'reduce_scatter: it needs reduce="rs"')
        if compression == "int4" and rs_algo == "ring":
            raise ValueError('compression="int4" does not run rs_algo="ring": the ring '
                             'requantizes on every hop, which at 4 bits loses far more than '
                             'at 8; use rs_algo=None or "direct"')
        if compression == "int4" and grads == "in_place" and rs_algo is None:
            raise ValueError('compression="int4" is not wired to grads="in_place" with no '
                             'algorithm named: at 4 bits the in-place path runs direct only, '
                             'and naming rs_algo="direct" runs it')
        self.compression = compression
        if rs_algo not in (None, "ring", "direct"):
            raise ValueError(f"rs_algo={rs_algo!r}: expected None, 'ring' or 'direct'")
        if rs_algo is not None and compression == "none":
            raise ValueError('rs_algo= selects the quantized reduce_scatter\'s '
                             'algorithm: it needs compression="int8"')
        self.rs_algo = rs_algo
        if ag_compression not in ("none", "int8", "int4"):
            raise ValueError(f"ag_compression={ag_compression!r}: expected 'none', 'int8' "
                             "or 'int4'")
        self.ag_compression = ag_compression
        if grads not in ("copy", "in_place"):
            raise ValueError(f"grads={grads!r}: expected 'copy' or 'in_place'")
        if grads == "in_place" and reduce != "rs":
            raise ValueError('grads="in_place" reads the gradients in the reduce_scatter: '
                             'it needs reduce="rs"')
        if grads == "in_place" and compression not in ("int8", "int4"):
            raise ValueError('grads="in_place" builds the quantized wire from the gradients: '
                             'it needs compression="int8" (or "int4" with rs_algo="direct")')
        self.grads = grads

        if torch.cuda.is_available() and self.params[0].is_cuda:
            mx.set_compute_stream(torch.cuda.current_stream().cuda_stream)
        dev = self.params[0].device
        dt = self.params[0].dtype
        assert all(p.dtype == dt for p in self.params), \
            "one flat group: uniform dtype required"
        if compression != "none" and dt not in (torch.float32, torch.bfloat16):
            raise ValueError(f'compression="{compression}" supports f32/bf16 parameters, '
                             f'not {dt}')
        if ag_compression != "none" and dt not in (torch.float32, torch.bfloat16):
            raise ValueError(f'ag_compression="{ag_compression}" supports f32/bf16 '
                             f'parameters, not {dt}')
        if max_grad_norm is not None and dt not in (torch.float32, torch.bfloat16,
                                                    torch.float16):
            raise ValueError(f"max_grad_norm= supports f32/bf16/f16 parameters, not {dt}")
        if self._fused and dt not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f'"adamw" supports f32/bf16/f16 parameters, not {dt}')
        # the squared norm of the reduced gradient, on the device (max_grad_norm)
        self._norm2 = torch.zeros(1, dtype=torch.float64, device=dev)
        self.grad_norm = None
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
        # quantized all_gather: the optimizer steps on an exact copy of the
        # shard and flat is the replica everywhere; built once, like _qrs
        self.master = self._delta = self._qag = None
        if ag_compression != "none" and self.world > 1:
            self.master = self.own_param.detach().clone()
            self._delta = torch.zeros_like(self.master)
            self._qag = mx.PersistentRequest(self.dist, "all_gather", self.shard,
                                             dtype=_dt(self.flat), group=group,
                                             quantized=True, accumulate=True,
                                             bits=4 if ag_compression == "int4" else 8)
        if self._fused:
            self._init_fused(**opt_kwargs)
        else:
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
                dtype=_dt(self.flat), group=group, algo=rs_algo, compression=compression)
        elif compression != "none" and self.world > 1:
            self._qrs = mx.PersistentRequest(self.dist, "reduce_scatter", self.shard,
                                             dtype=_dt(self.flat), op="sum",
                                             group=group, quantized=True,
                                             algo=rs_algo,
                                             bits=4 if compression == "int4" else 8)

    def _init_fused(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        """State of the built-in AdamW: f32 master weights and moments of the
        owned shard. f32 parameters that travel exactly step where they lie,
        unless an odd shard leaves this rank's slice of flat off 16 bytes: the
        kernel's states are vectors, so master is then a buffer of its own and
        the slice takes the new parameter as `out`, the same bits."""
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.step_count = 0
        if (self.flat.dtype == torch.float32 and self._qag is None
                and self.own_param.data_ptr() % 16 == 0):
            self.master = self.own_param
        else:
            self.master = self.own_param.detach().to(torch.float32, copy=True)
        self.exp_avg = torch.zeros_like(self.master)
        self.exp_avg_sq = torch.zeros_like(self.master)

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
            if self.average and not self._fused:
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
            if self.average and self.reduce == "rs" and not self._fused:
                self.own_grad /= self.world
        else:
            self._gather_grads()
            self.own_grad.copy_(self.flat_grad[:self.shard])

        if self._fused:
            self._fused_step()
        else:
            if self.max_grad_norm is not None:
                self._clip_own_grad()
            self._shard_holder.grad = self.own_grad
            self.opt.step()
            self._shard_holder.grad = None

        if self._qag is not None:
            # what the replica lacks, last step's rounding included, quantized;
            # every rank adds every segment the same way
            if not self._fused:
                torch.sub(self.master, self.own_param, out=self._delta)
            self._qag.start(self._delta, self.flat)
            self._qag.wait()
        elif self.world > 1:
            # increment AllGather (reference StartIncrementComm):
            # every rank's updated shard -> full parameter buffer
            mx.wait(self.dist.all_gather(self.own_param, self.shard,
                                         self.flat, dtype=_dt(self.flat),
                                         group=self.group))

    def _fused_step(self):
        """The built-in AdamW on the owned shard, one launch: own_grad is the
        reduced SUM (the kernel averages by grad_scale), _norm2 its squared
        norm, unscaled (the kernel clips from it). The rounded parameter goes
        to own_param, or under ag_compression master - own_param to _delta."""
        g = self.own_grad
        scale = (float(torch.tensor(1.0 / self.world, dtype=torch.float32))
                 if self.average and self.reduce == "rs" else 1.0)
        clip = self.max_grad_norm is not None
        if clip:
            self._sum_squares()
            self.grad_norm = self._norm2.sqrt() * scale
        self.step_count += 1
        kw = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                  step=self.step_count, grad_scale=scale, dtype=_dt(g),
                  max_norm=self.max_grad_norm)
        if self._qag is not None:
            out, replica = self._delta, self.own_param
        else:
            out, replica = (None if self.master is self.own_param else self.own_param), None
        if g.is_cuda:
            ops.adamw_step(g, self.master, self.exp_avg, self.exp_avg_sq, self.shard,
                           total=self._norm2 if clip else None, out=out, replica=replica, **kw)
        else:
            ops.host_adamw_step(_np(g), _np(self.master), _np(self.exp_avg),
                                _np(self.exp_avg_sq), self.shard,
                                total=float(self._norm2) if clip else None,
                                out=None if out is None else _np(out),
                                replica=None if replica is None else _np(replica), **kw)

    def _sum_squares(self):
        """_norm2 = the squared norm of the whole reduced gradient: the shard's
        sum of squares in float64, then one exact scalar all_reduce."""
        g = self.own_grad
        if g.is_cuda:
            ops.sumsq(g, self.shard, self._norm2, dtype=_dt(g))
        else:
            self._norm2.copy_(g.double().square().sum())
        if self.world > 1:
            mx.wait(self.dist.all_reduce(self._norm2, self._norm2, 1, op="sum", dtype="f64",
                                         group=self.group))

    def _clip_own_grad(self):
        """own_grad, final and averaged, scaled by the clip coefficient of the
        whole reduced gradient: shard sum of squares, one scalar all_reduce,
        scale. The shards partition the padded gradient, so their sums add up
        to the full squared norm under reduce="none" as under "rs"."""
        g = self.own_grad
        self._sum_squares()
        if g.is_cuda:
            ops.clip_scale(g, self.shard, self._norm2, self.max_grad_norm, dtype=_dt(g))
        else:
            g.mul_(torch.clamp(self.max_grad_norm / (self._norm2.sqrt() + 1e-6),
                               max=1.0).to(torch.float32))
        self.grad_norm = self._norm2.sqrt()

    def zero_grad(self, set_to_none=False):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def state_dict(self):
        if self._fused:
            return {"step": self.step_count, "master": self.master.clone(),
                    "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone()}
        return self.opt.state_dict()

    def load_state_dict(self, sd):
        if not self._fused:
            return self.opt.load_state_dict(sd)
        self.step_count = int(sd["step"])
        for name in ("master", "exp_avg", "exp_avg_sq"):
            getattr(self, name).copy_(sd[name])
