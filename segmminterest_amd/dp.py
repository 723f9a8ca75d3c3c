"""Data parallelism over the GPUs of one node: the collectives of a data-parallel step (``DPComm``) and the row sharding of a
global batch (``shard_rows``).  How the step uses them is told in trainer.py's module docstring."""
from __future__ import annotations

import torch

from . import hipabi as H
from . import switches


# ------------------------------------------------------------------------------------------------ communication
class DPComm:
    """The three collectives of a data-parallel step (engine-agnostic; works on any torch.distributed
    backend, ``nccl`` = RCCL on the GPU box, ``gloo`` in the CPU tests)."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        # every collective of the step is issued iff ``active``: more than one rank -- or SEGMM_DP_FORCE=1 with an initialised
        # process group of ONE rank, which sends the single-GPU step through the real RCCL calls (tests/test_dp_gpu.py: the
        # only way to execute the nccl code path on a one-GPU box; results must equal the plain step bit for bit)
        self.active = self.world > 1 or (switches.read("comm")["force"] and dist.is_initialized())
        self.pending = []
        # gloo has no device collectives for every op: device tensors are staged through the host.
        # Only the test harness uses that (two ranks sharing one GPU); production is nccl = RCCL.
        self.host_staged = dist.is_initialized() and dist.get_backend(group) == "gloo"

    def _all_reduce(self, t, async_op=False):
        if self.host_staged and t.is_cuda:
            h = t.cpu()
            self.dist.all_reduce(h, op=self.dist.ReduceOp.SUM, group=self.group)
            t.copy_(h)
            return None
        return self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group, async_op=async_op)

    def _pbuf(self, key, shape, dtype, device):
        """Persistent staging buffer of a collective: the SAME tensor every step, so that a recorded step (Trainer.record),
        whose kernels name the results by address, can be replayed around the collectives."""
        bufs = self.__dict__.setdefault("_bufs", {})
        b = bufs.get(key)
        if b is None or tuple(b.shape) != tuple(shape) or b.dtype != dtype or b.device != device:
            b = bufs[key] = torch.empty(shape, dtype=dtype, device=device)
        return b

    def label_stats_buffers(self, B, device):
        """(v, v2, norms) as views of the persistent send record of :meth:`global_label_stats`: the statistics kernel writes where
        the all-gather reads, nothing is packed."""
        mine = self._pbuf("ls_mine", (2 * B + 3,), torch.float32, device)
        return mine[:B], mine[B:2 * B], mine[2 * B:]

    def global_label_stats(self, v, v2, norms):
        """(v_all, v2_all, norms_global): all-gather the per-row view lengths, sum the 3 normalisers.  Returns the triple
        (single process) or a closure that waits for the asynchronous collective and returns it."""
        if not self.active:
            return v, v2, norms
        # ONE collective: [v | v2 | norms] of every rank (every rank holds the same B_local); the three normalisers are
        # summed locally from the gathered copies, in rank order on every rank (identical results everywhere)
        # The collective is ASYNCHRONOUS: the caller gets a closure and calls it right before the loss kernel, so the
        # all-gather (and the rank skew it absorbs) runs under the backbone forward instead of in front of it.
        B, n, dev, G = v.shape[0], 2 * v.shape[0] + 3, v.device, self.world
        mine = self._pbuf("ls_mine", (n,), v.dtype, dev)
        gathered = self._pbuf("ls_gathered", (G * n,), v.dtype, dev)
        v_all, v2_all = self._pbuf("ls_v", (G * B,), v.dtype, dev), self._pbuf("ls_v2", (G * B,), v.dtype, dev)
        norms_g = self._pbuf("ls_norms", (3,), norms.dtype, dev)
        state = {}

        def start():
            # (the statistics kernel normally wrote straight into `mine` -- label_stats_buffers; a caller's own tensors are copied
            # by the library's copy kernel: no torch kernel inside the data-parallel step)
            if v.data_ptr() != mine.data_ptr():
                cp = H.copy_bytes if mine.is_cuda else (lambda d_, s_: d_.copy_(s_))
                cp(mine[:B], v.contiguous())
                cp(mine[B:2 * B], v2.contiguous())
                cp(mine[2 * B:], norms.contiguous())
            if self.host_staged and mine.is_cuda:
                hg = torch.empty((G * n,), dtype=mine.dtype)
                self.dist.all_gather_into_tensor(hg, mine.cpu(), group=self.group)
                gathered.copy_(hg)
                state["work"] = None
            else:
                state["work"] = self.dist.all_gather_into_tensor(gathered, mine, group=self.group, async_op=True)

        def finish():
            work = state.pop("work", None)
            if work is not None:
                work.wait()          # stream-level wait on the communication stream, no host sync
            if gathered.is_cuda:
                H.label_stats_unpack(gathered, G, B, v_all, v2_all, norms_g)          # one launch: split + rank-ordered sum of the counts
            else:
                g = gathered.view(G, n)
                v_all.view(G, B).copy_(g[:, :B])
                v2_all.view(G, B).copy_(g[:, B:2 * B])
                torch.sum(g[:, 2 * B:], 0, out=norms_g)          # counts: exact in fp32 below 2^24
            return v_all, v2_all, norms_g
        H.host_action(start)
        return lambda: H.host_action(finish)

    def gather_rows(self, ids, rows):
        """Sparse exchange of id-table gradients: returns a CLOSURE that yields (ids of all ranks [G*B], rows of all ranks
        [G*B, w]) in rank order (every rank holds the same B, like :meth:`global_label_stats`).

        ONE asynchronous all-gather of ``[rows | id]`` per rank (the int64 id rides in two float lanes of its row) on a process
        group OF ITS OWN: on the gradient group it would queue behind every bucket all-reduce still in flight on that group's
        RCCL stream.  The caller issues it as soon as the compact rows exist and calls the closure right before the segment sum
        (engine._embed_bwd), so the collective and the rank skew it absorbs run under the rest of the embedding backward."""
        if not self.active:
            return lambda: (ids, rows)
        ids, rows = ids.contiguous(), rows.contiguous()
        if ids.dtype != torch.int64:
            ids = ids.to(torch.int64)
        B, w = rows.shape
        G, dev = self.world, rows.device
        seq = self.__dict__.get("_gr_seq", 0)          # (which exchange of the step: reset by Trainer at the head of the backward)
        self._gr_seq = seq + 1
        packed = self._pbuf(("gr_packed", seq), (B, w + 2), torch.float32, dev)
        gathered = self._pbuf(("gr_gathered", seq), (G * B, w + 2), torch.float32, dev)
        ids_all = self._pbuf(("gr_ids", seq), (G * B,), torch.int64, dev)
        rows_all = self._pbuf(("gr_rows", seq), (G * B, w), torch.float32, dev)
        state = {}

        def start():
            packed[:, :w].copy_(rows)
            packed[:, w:].copy_(ids.view(B, 1).view(torch.float32))          # bit pattern of the id, not a conversion
            if self.host_staged and rows.is_cuda:
                hg = torch.empty((G * B, w + 2), dtype=torch.float32)
                self.dist.all_gather_into_tensor(hg, packed.cpu(), group=self.group)
                gathered.copy_(hg)
                state["work"] = None
            else:
                state["work"] = self.dist.all_gather_into_tensor(gathered, packed, group=self._row_group(), async_op=True)

        def finish():
            work = state.pop("work", None)
            if work is not None:
                work.wait()          # stream-level wait on the row group's communication stream, no host sync
            ids_all.copy_(gathered[:, w:].contiguous().view(torch.int64).view(-1))
            rows_all.copy_(gathered[:, :w])
            return ids_all, rows_all
        H.host_action(start)
        return lambda: H.host_action(finish)

    def _row_group(self):
        """Process group of the row exchange (same ranks as the gradient group; created on first use, by every rank at the
        same point of its first data-parallel backward).  A one-rank forced group (tests) shares the gradient group."""
        g = self.__dict__.get("_rowg")
        if g is None:
            if self.world > 1:
                ranks = self.dist.get_process_group_ranks(self.group) if self.group is not None else list(range(self.dist.get_world_size()))
                g = self.dist.new_group(ranks=ranks, backend=self.dist.get_backend(self.group))
            else:
                g = self.group if self.group is not None else self.dist.group.WORLD
            self._rowg = g
        return g

    def gather_ints(self, t):
        """[G*B] int32: the values of every rank in rank order (validation: leave ranks of the global batch)."""
        if not self.active:
            return t
        t = t.contiguous()
        if self.host_staged and t.is_cuda:
            h = torch.empty((self.world * t.shape[0],), dtype=t.dtype)
            self.dist.all_gather_into_tensor(h, t.cpu(), group=self.group)
            return h.to(t.device)
        out = torch.empty((self.world * t.shape[0],), dtype=t.dtype, device=t.device)
        self.dist.all_gather_into_tensor(out, t, group=self.group)
        return out

    def reduce_bucket(self, flat_grad, start, end):
        """Asynchronous SUM all-reduce of one contiguous gradient bucket (gradients are already
        normalised by global counts, so SUM -- not mean -- reproduces the single-process gradient)."""
        if not self.active or end <= start:
            return
        w = self._all_reduce(flat_grad[start:end], async_op=True)
        if w is not None:
            self.pending.append(w)

    def take_pending(self):
        """The outstanding asynchronous all-reduces (issue order); the caller waits for them (``work.wait()`` is a
        stream-level wait on the communication stream, no host sync)."""
        p, self.pending = self.pending, []
        return p

    def finish(self):
        for w in self.take_pending():
            w.wait()

    def sum_scalar(self, t):
        if self.active:
            self._all_reduce(t)
        return t


def shard_rows(n_rows: int, world: int, rank: int):
    """Contiguous row block of ``rank``; the first ``n_rows % world`` ranks get one more."""
    base, rem = divmod(n_rows, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)
