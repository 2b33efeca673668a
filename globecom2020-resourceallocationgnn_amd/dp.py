"""Batched data parallelism over independent graph instances.

One process per GPU; every rank holds a full replica of the weights and Adam state and a
contiguous shard of B/G whole graphs of the replay minibatch (AggLayer only contracts inside a
sample, BS_brain.py:73, so forward and backward need no communication).  The only collective
is ONE all-reduce (sum) of the flat fp32 gradient buffer per step -- RCCL over xGMI through
`torch.distributed` (backend "nccl" is RCCL on ROCm; "gloo" in the CPU tests).  Each rank
differentiates its shard of the GLOBAL Huber mean (n_global = B), so the sum of the per-rank
gradients is exactly the single-GPU gradient and no rescale is needed.  The target-network
sync stays a local device-to-device copy.
"""
import ctypes as C

import numpy as np

from . import lib as _lib


class DataParallelTrainer(object):
    """`backend` implements forward_backward(batch, y, n_global, want_loss) -> loss tensor,
    grad_tensor() -> flat torch tensor aliasing the gradient buffer, apply_gradients().
    `GnnEngine` is the GPU backend."""

    def __init__(self, backend, process_group=None, force=False, overlap=None, shard_optimizer=None, native=False, comm=None):
        """native: every train_step is ONE library call (GnnEngine.train_step_dp) that runs the forward / backward, the
        collectives of this trainer's form and Adam; the collectives go through `comm` (default, made on the first step: an
        RcclComm on the nccl backend, a TorchComm on any other).  The same launches and collectives as the Python form."""
        import torch.distributed as dist
        self.dist = dist
        self.backend = backend
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        self._grad = None
        self._buckets = None
        self.force = force          # run the collective even with one rank (exercises the RCCL path)
        # overlap: split the step so that the Dense-layer bucket is all-reduced during the graph-layer backward
        # (train_step).  None = the V2X_DP_OVERLAP environment switch, default OFF: the split costs two launches of the
        # slab sums instead of one and two stream hand-overs per step; measured on one MI355X with the RCCL path forced
        # (tools/dp_host_overhead.py, 20 links x 64 features, batch 4096, 3 MB of gradients): 301 us per step split
        # against 271 us unsplit (264 without data parallelism), i.e. the split only pays once hiding the Dense bucket's
        # all-reduce (1.2 MB, latency-bound on xGMI) is worth more than 30 us -- and the models it applies to (feature
        # width <= 64) have at most a few MB of gradients.
        import os
        # Wide models (feat_dim >= 128: one bucket per layer, configs[3]: 207.6 MB of gradients) overlap by default: measured on
        # one MI355X with the RCCL path forced (tools/dp_host_overhead.py --wide) the phased step costs 3.82 ms against 3.65 ms
        # with one all-reduce after the merged weight-gradient launch -- 0.17 ms, which the all-reduce of four of the five
        # buckets behind the remaining backward repays as soon as the collective takes longer than that (8 GPUs over xGMI:
        # ~1 ms for 207.6 MB; unmeasured here, one GPU per box).
        wide = getattr(getattr(backend, "spec", None), "feat_dim", 0) >= 128
        env = os.environ.get("V2X_DP_OVERLAP")
        self.overlap = ((env == "1") if env is not None else wide) if overlap is None else bool(overlap)
        # shard_optimizer: reduce-scatter + Adam on the rank's 1 / G slice of every bucket + all-gather of the parameters
        # (V2X_DP_SHARD_OPTIMIZER=1); see train_step
        self.shard_optimizer = (os.environ.get("V2X_DP_SHARD_OPTIMIZER", "0") == "1") if shard_optimizer is None else bool(shard_optimizer)
        self._has_reduce_scatter = True
        self._bucket_ranges = None
        self._param = None
        self.native = bool(native)
        self._comm = comm

    @property
    def form(self):
        """the v2x_train_step_dp form this trainer's switches select"""
        if self.shard_optimizer:
            return _lib.V2X_DP_SHARDED
        return _lib.V2X_DP_BUCKETS if self.overlap else _lib.V2X_DP_ALLREDUCE

    def comm(self):
        """the collective table of the native step (made on first use: every rank must call it at the same point)"""
        if self._comm is None:
            nccl = self.dist.is_initialized() and self.dist.get_backend(self.group) == "nccl"
            self._comm = (RcclComm if nccl else TorchComm)(self.group, device=getattr(self.backend, "device", None))
            self._own_comm = True
        return self._comm

    def close(self):
        """free the collective table comm() made (an RcclComm holds an RCCL communicator); one handed in stays the caller's"""
        if getattr(self, "_own_comm", False) and self._comm is not None:
            self._comm.close()
            self._comm, self._own_comm = None, False

    def shard(self, batch, y):
        """Contiguous shard of whole graphs for this rank (variable-size batches: balanced by edges + nodes,
        PackedBatch.shard_bounds).  y is [R, C] for the full batch."""
        if self.world == 1:
            return batch, y
        sh, (r0, r1) = batch.shard(self.rank, self.world, with_rows=True)
        return sh, y[r0:r1]

    def _overlapped(self, local_batch):
        """Bucketed collectives overlapped with the backward pass: available when the backend splits its step
        (GnnEngine.forward_backward_phase) and the batch is resident on the device."""
        return ((self.overlap or self.shard_optimizer) and hasattr(self.backend, "forward_backward_phase")
                and (hasattr(local_batch, "device") or getattr(self.backend, "phases_on_host", False)))

    # ---- collectives on one bucket -------------------------------------------------------------------------------------
    def _slice_of(self, n):
        """(first, count) of this rank's slice of an n-float bucket for reduce-scatter / sharded Adam, or None when the bucket
        does not cut into `world` float4-aligned equal slices (it is then all-reduced and updated whole)."""
        if n % (4 * self.world):
            return None
        c = n // self.world
        return self.rank * c, c

    def _reduce_scatter(self, bucket, first, count):
        """Sum over ranks of `bucket`, this rank's slice only, left in place in bucket[first : first + count].  RCCL: a real
        reduce-scatter (half the bytes of an all-reduce); backends without one (gloo in the CPU tests): all-reduce."""
        out = bucket[first:first + count]
        if self._has_reduce_scatter:
            try:
                return self.dist.reduce_scatter_tensor(out, bucket, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
            except (RuntimeError, NotImplementedError):
                self._has_reduce_scatter = False
        return self.dist.all_reduce(bucket, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)

    def train_step(self, local_batch, local_y, n_graphs_global=None, want_loss=True, n_denominator=None):
        """forward+backward on the local shard, reduce the gradient over the ranks, Adam.

        n_denominator (n_graphs_global is its older name): what the GLOBAL Huber mean divides by besides the channel
        count -- the number of graphs of the whole minibatch for fixed-size graphs (one mean per output, BS_brain.py:214),
        the number of NODE ROWS of the whole minibatch for variable_graphs models (one mean over all rows): ragged shards
        hold different numbers of rows, so the caller sums them over the ranks (bench.py does).

        Three forms:
        * default: one replayed graph for forward + backward + slab sums, ONE all-reduce of the flat gradient, Adam on every
          rank -- right for the headline model (3 MB of gradients: latency-bound on xGMI, nothing to hide);
        * `overlap`: the step runs in phases (GnnEngine.forward_backward_phase); bucket k of the gradient is final after phase
          k and its all-reduce is started right away -- asynchronously, RCCL works on its own stream -- while the later
          phases compute.  Wide models have one bucket per layer (configs[3]: 4.6 + 3 x 13.5 + 6.9 M floats = 207.6 MB, whose
          all-reduce is bandwidth-bound and worth hiding behind the ~2.4 ms of backward that follow the first bucket);
          narrow models have two (measured slower than the default at 3 MB: off by default);
        * `shard_optimizer` (implies the phases): reduce-scatter instead of all-reduce, Adam on this rank's 1 / G slice of
          every bucket (v2x_apply_gradients_range: the 28 bytes per parameter of the Adam pass shrink by G), all-gather of
          the updated parameters.  Optimizer moments are then only valid on their owner's slice (gather_optimizer_state)."""
        if n_denominator is not None:
            n_graphs_global = n_denominator
        if n_graphs_global is None:
            raise ValueError("train_step: the global Huber denominator (n_denominator) is required under data parallelism")
        if self.native:
            return self.backend.train_step_dp(local_batch, local_y, self.comm(), self.form, n_graphs_global, want_loss)
        reduce_now = self.world > 1 or self.force
        if reduce_now and self._overlapped(local_batch):
            return self._train_step_phased(local_batch, local_y, n_graphs_global, want_loss)
        if reduce_now and self.shard_optimizer:
            # The phases are not available for this batch (a host-resident batch, a backend without them), but the optimizer
            # state is SHARDED: after any sharded step a rank holds current Adam moments for its own slices only, so a step
            # that ran full-range Adam on every rank would apply different moments on different ranks and the replicas
            # would part without an error.  Stay sharded: whole backward first, then the same per-bucket
            # reduce-scatter / Adam-on-the-slice / all-gather.
            if not hasattr(self.backend, "apply_gradients_range") or not hasattr(self.backend, "grad_buckets"):
                raise RuntimeError("shard_optimizer: the backend has neither phases nor apply_gradients_range; a full-range Adam "
                                   "step would desynchronise the sharded optimizer state")
            return self._train_step_phased(local_batch, local_y, n_graphs_global, want_loss, phased=False)
        loss = self.backend.forward_backward(local_batch, local_y, n_global=n_graphs_global, want_loss=want_loss)
        if reduce_now:
            if self._grad is None:
                self._grad = self.backend.grad_tensor()
            self.dist.all_reduce(self._grad, op=self.dist.ReduceOp.SUM, group=self.group)
            if want_loss and loss is not None:
                loss = self._reduce_loss(loss)
        self.backend.apply_gradients()
        return loss

    def _reduce_loss(self, loss):
        import torch
        if not torch.is_tensor(loss):
            # host-side loss (numpy batches): reduce it on the device the gradient lives on (RCCL has no
            # CPU tensors; gloo takes the CPU tensor as is)
            loss_t = torch.as_tensor(np.asarray(loss, np.float64), device=self._grad.device)
            self.dist.all_reduce(loss_t, op=self.dist.ReduceOp.SUM, group=self.group)
            return loss_t.cpu().numpy()
        self.dist.all_reduce(loss, op=self.dist.ReduceOp.SUM, group=self.group)
        return loss

    def _train_step_phased(self, local_batch, local_y, n_global, want_loss, phased=True):
        """phased=False: the backend's unsplit forward + backward first, then the bucket collectives (nothing overlaps; the
        optimizer step is the sharded one all the same)."""
        if self._grad is None:
            self._grad = self.backend.grad_tensor()
        if self._buckets is None:
            self._bucket_ranges = list(self.backend.grad_buckets())
            self._buckets = [self._grad[o:o + n] for o, n in self._bucket_ranges]
            if self.shard_optimizer:
                self._param = self.backend.param_tensor()
        nb = len(self._buckets)
        works, loss = [], None
        if not phased:
            loss = self.backend.forward_backward(local_batch, local_y, n_global=n_global, want_loss=want_loss)
        for k in range(nb):
            if phased:
                loss = self.backend.forward_backward_phase(local_batch, local_y, k, n_global=n_global, want_loss=want_loss)
            sl = self._slice_of(self._bucket_ranges[k][1]) if self.shard_optimizer else None
            if sl is not None:
                works.append((self._reduce_scatter(self._buckets[k], sl[0], sl[1]), sl))
            else:
                works.append((self.dist.all_reduce(self._buckets[k], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True), None))
        if not self.shard_optimizer:
            for w, _ in works:
                w.wait()
            if want_loss and loss is not None:
                loss = self._reduce_loss(loss)
            self.backend.apply_gradients()
            return loss
        # sharded optimizer step: as each bucket's sum arrives, Adam on the owned slice, then the slice travels to the others
        gathers, first = [], True
        for k, (w, sl) in enumerate(works):
            w.wait()
            off, n = self._bucket_ranges[k]
            if sl is None:                               # bucket not cut: every rank updates all of it
                self.backend.apply_gradients_range(off, n, first)
            else:
                self.backend.apply_gradients_range(off + sl[0], sl[1], first)
                pb = self._param[off:off + n]
                mine = pb[sl[0]:sl[0] + sl[1]]           # RCCL: the in-place form (input = this rank's slice of the output)
                if self.dist.get_backend(self.group) != "nccl":
                    mine = mine.clone()
                gathers.append(self.dist.all_gather_into_tensor(pb, mine, group=self.group, async_op=True))
            first = False
        if want_loss and loss is not None:
            loss = self._reduce_loss(loss)
        for g in gathers:
            g.wait()
        if hasattr(self.backend, "params_changed"):
            self.backend.params_changed()
        return loss

    def gather_optimizer_state(self):
        """shard_optimizer: Adam's moments are only kept up to date on the slice their rank owns.  -> (m, v, iterations) with
        every slice taken from its owner (numpy, on every rank): what a checkpoint of the job has to hold."""
        m, v, it = self.backend.get_optimizer_state()
        if not self.shard_optimizer or self.world == 1:
            return m, v, it
        import torch
        if self._grad is None and self.native:
            self._grad = self.backend.grad_tensor()          # (the device the slices travel through)
        dev = self._grad.device if self._grad is not None else "cpu"
        out = []
        for arr in (m, v):
            t = torch.as_tensor(np.ascontiguousarray(arr), device=dev)
            for off, n in (self._bucket_ranges or self.backend.grad_buckets()):
                sl = self._slice_of(n)
                if sl is None:
                    continue
                b = t[off:off + n]
                self.dist.all_gather_into_tensor(b, b[sl[0]:sl[0] + sl[1]].clone(), group=self.group)
            out.append(t.cpu().numpy())
        return out[0], out[1], it

    def all_reduce_numpy(self, arr):
        """Sum of a small float64 numpy array over the ranks (statistics, not the hot path).  RCCL has no CPU tensors:
        the array travels through the device the gradient lives on; gloo takes the CPU tensor as is."""
        if self.world == 1:
            return np.asarray(arr, np.float64)
        import torch
        if self._grad is None:
            self._grad = self.backend.grad_tensor()
        t = torch.as_tensor(np.asarray(arr, np.float64), device=self._grad.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return t.cpu().numpy()


# ---- collective tables of the native step (v2x_comm, include/v2xgnn.h) -------------------------------------------------------
def _device_view(ptr, n, device):
    """torch view (no copy) of n float32 at device address ptr"""
    import torch

    class _Holder(object):
        pass
    h = _Holder()
    h.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f4", "data": (int(ptr), False), "version": 2, "strides": None}
    return torch.as_tensor(h, device="cuda:%d" % device)


def _group_ranks(group):
    import torch.distributed as dist
    if not dist.is_initialized():
        return 1, 0
    return dist.get_world_size(group), dist.get_rank(group)


class RcclComm(object):
    """The library's RCCL table (v2x_comm_rccl_create) for the ranks of `group`: rank 0's unique id reaches the others over the
    process group.  Creating it is collective over the group.  `comm` is the lib.Comm to hand to the library; close() frees
    the communicator."""

    def __init__(self, group=None, device=None):
        import torch
        import torch.distributed as dist
        self._lib = _lib.load_library()
        self.world, self.rank = _group_ranks(group)
        self.device = torch.cuda.current_device() if device is None else int(device)
        uid = (C.c_uint8 * 128)()
        if self.rank == 0:
            _lib.check(self._lib, self._lib.v2x_comm_rccl_unique_id(uid))
        if self.world > 1:
            box = [bytes(uid)]
            src = dist.get_global_rank(group, 0) if group is not None else 0
            dist.broadcast_object_list(box, src=src, group=group)
            C.memmove(uid, box[0], 128)
        self.comm = _lib.Comm()
        _lib.check(self._lib, self._lib.v2x_comm_rccl_create(uid, self.world, self.rank, self.device, C.byref(self.comm)))

    def close(self):
        if getattr(self, "comm", None) is not None and self.comm.ctx:
            _lib.check(self._lib, self._lib.v2x_comm_rccl_destroy(C.byref(self.comm)))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TorchComm(object):
    """A v2x_comm whose entries are ctypes callbacks into torch.distributed on `group`, for backends the library cannot drive
    itself (gloo: the one-GPU two-rank tests).  Each entry runs its collective on the stream the library hands over and
    blocks the host until it is done.  Reduce-scatter is the whole-bucket all-reduce (gloo has none; the rank's slice then
    holds the sum, as DataParallelTrainer._reduce_scatter does).  An exception inside an entry returns -1 (V2X_ECOMM) and is
    kept in `last_error`."""

    def __init__(self, group=None, device=None):
        import torch
        self.group = group
        self.world, self.rank = _group_ranks(group)
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.last_error = None
        self._fns = [_lib.COLLECTIVE(self._entry(f)) for f in (self._all_reduce, self._reduce_scatter, self._all_gather)]
        self.comm = _lib.Comm(self.world, self.rank, None, *self._fns)

    def _entry(self, body):
        def call(buf, n, stream, ctx):
            try:
                if self.world == 1:
                    return 0                         # the sum over one rank, the gather of one slice: nothing to do
                import torch
                st = torch.cuda.ExternalStream(stream, device=self.device) if stream else torch.cuda.default_stream(self.device)
                with torch.cuda.stream(st):
                    body(_device_view(buf, n, self.device), int(n))
                st.synchronize()
                return 0
            except Exception as exc:                 # (nothing may propagate through the C frames)
                self.last_error = exc
                return -1
        return call

    def _all_reduce(self, t, n):
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)

    _reduce_scatter = _all_reduce

    def _all_gather(self, t, n):
        import torch.distributed as dist
        c = n // self.world
        dist.all_gather_into_tensor(t, t[self.rank * c:(self.rank + 1) * c].clone(), group=self.group)

    def close(self):
        pass
