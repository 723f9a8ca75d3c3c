"""Inference -> SegRec bridge.

``inference/save_logits_for_all_leave_SegMM.py:105-150`` runs the interest model over every split and writes
``{"<user_id>-<photo_id>-<time_ms>": [S logits]}`` as JSON (and a torch pickle); SegRec reads that file as
``clip_weight`` and feeds ``feed_dict['c_interest_weight']`` ([batch, item_num, 40]: the TARGET item's slice for every item of
the row, ones when the target's key is missing, own slices for the negatives when a negatives file is given --
SegRec/models/BaseModel.py:228-288), which ``ClipRec.forward`` multiplies into the per-segment predictions
(``sum_seg pred * weight * (seg < duration)``, ClipRec.py:163-181).

``LogitStore`` keeps the same mapping as three int64 key columns + one float32 [n, S] matrix, writes the reference's
JSON byte-for-byte (same key format, ``json.dump`` of python floats converted from fp32 like ``tensor.tolist()``) and a
binary ``.npz`` that loads without parsing 40 floats per row from text; ``weights`` answers a whole batch of lookups
with one vectorised search and ``weighted_head`` is the device kernel for the ClipRec sum.  ``DeviceLogitStore`` is the same store
with the values resident on the device: lookups and the head run as kernels (csrc/storeops.h)."""
from __future__ import annotations

import json
from typing import Optional

import numpy as np
import torch


class LogitStore:
    def __init__(self, S: int = 40):
        self.S = S
        self._keys = []          # list of [n_i, 3] int64 blocks
        self._vals = []          # list of [n_i, S] float32 blocks
        self._index = None

    # ---- writer side (one call per inference batch)
    def add_batch(self, user_id, photo_id, time_ms, logits):
        k = np.stack([np.asarray(torch.as_tensor(v).cpu(), dtype=np.int64).reshape(-1) for v in (user_id, photo_id, time_ms)], 1)
        v = torch.as_tensor(logits).detach().float().cpu().numpy().reshape(k.shape[0], -1)
        if v.shape[1] != self.S:
            raise ValueError("logits have %d segments, store expects %d" % (v.shape[1], self.S))
        self._keys.append(k)
        self._vals.append(v)
        self._index = None

    def _cat(self):
        if len(self._keys) > 1:
            self._keys, self._vals = [np.concatenate(self._keys, 0)], [np.concatenate(self._vals, 0)]
        if not self._keys:
            return np.zeros((0, 3), np.int64), np.zeros((0, self.S), np.float32)
        return self._keys[0], self._vals[0]

    def as_dict(self):
        """The reference's in-memory form; later duplicates of a key overwrite earlier ones, like its dict assignment."""
        k, v = self._cat()
        return {"%d-%d-%d" % (int(a), int(b), int(c)): [float(x) for x in row] for (a, b, c), row in zip(k, v)}

    def save_json(self, path):
        with open(path, "w") as fw:
            json.dump(self.as_dict(), fw)

    def save_binary(self, path):
        k, v = self._cat()
        np.savez(path, keys=k, logits=v, S=np.int64(self.S))

    # ---- reader side
    @classmethod
    def load(cls, path):
        if str(path).endswith(".json"):
            with open(path) as f:
                d = json.load(f)
            st = cls(S=len(next(iter(d.values()))) if d else 40)
            if d:
                keys = np.array([[int(x) for x in key.split("-")] for key in d], dtype=np.int64)
                st._keys, st._vals = [keys], [np.array(list(d.values()), dtype=np.float32)]
            return st
        z = np.load(path)
        st = cls(S=int(z["S"]))
        st._keys, st._vals = [z["keys"]], [z["logits"]]
        return st

    def _build_index(self):
        k, v = self._cat()
        # last occurrence of a key wins (dict semantics): stable sort, keep the last of each run
        order = np.lexsort((np.arange(len(k)), k[:, 2], k[:, 1], k[:, 0]))
        ks = k[order]
        last = np.ones(len(ks), bool)
        if len(ks) > 1:
            last[:-1] = (ks[1:] != ks[:-1]).any(1)
        self._index = (ks[last], order[last])

    def _lookup(self, q):
        """rows of the value matrix for the [n, 3] keys ``q`` (-1 where absent)"""
        if self._index is None:
            self._build_index()
        ks, rows = self._index
        out = np.full((q.shape[0],), -1, dtype=np.int64)
        if len(ks):
            dt = np.dtype([("a", np.int64), ("b", np.int64), ("c", np.int64)])          # lexicographic (user, item, time)
            kv = np.ascontiguousarray(ks).view(dt).reshape(-1)
            qv = np.ascontiguousarray(q).view(dt).reshape(-1)
            pos = np.searchsorted(kv, qv)
            pos_c = np.minimum(pos, len(kv) - 1)
            hit = (pos < len(kv)) & (kv[pos_c] == qv)
            out[hit] = rows[pos_c[hit]]
        return out

    def weights(self, user_id, item_ids, time_ms, neg: "Optional[LogitStore]" = None, id2user=None, id2item=None, device=None):
        """``feed_dict['c_interest_weight']`` of a batch exactly as ``GeneralModel.Dataset._get_feed_dict`` builds it
        (SegRec/models/BaseModel.py:228-288): user_id [B], item_ids [B, I] (column 0 = the target item), time_ms [B] ->
        float32 [B, I, S].  Per row, with key = "<user>-<item 0>-<time>":
          * key absent                      -> ones (the reference appends ONE row of ones, which broadcasts over the items);
          * key present, no negatives file  -> EVERY item of the row gets the TARGET's slice;
          * key present, negatives file ``neg`` and I > 2 -> item 0 the target's slice, item j its own slice from ``neg``
            (KeyError if absent, like the reference).
        ``id2user`` / ``id2item`` (dicts keyed by str): the id mapping the non-KuaiRand branch applies first (:268,275)."""
        u = np.asarray(user_id, np.int64).reshape(-1)
        it = np.asarray(item_ids, np.int64)
        t = np.asarray(time_ms, np.int64).reshape(-1)
        if id2user is not None:
            u = np.asarray([int(id2user[str(int(x))]) for x in u], np.int64)
        if id2item is not None:
            it = np.asarray([[int(id2item[str(int(x))]) for x in r] for r in it], np.int64)
        B, I = it.shape
        _, v = self._cat()
        first = self._lookup(np.stack([u, it[:, 0], t], 1))
        out = np.ones((B, I, self.S), np.float32)
        hit = first >= 0
        if hit.any():
            out[hit] = v[first[hit]][:, None, :]
            if neg is not None and I > 2:
                _, nv = neg._cat()
                q = np.stack([np.broadcast_to(u[:, None], (B, I - 1)), it[:, 1:], np.broadcast_to(t[:, None], (B, I - 1))], -1)
                rows = neg._lookup(q.reshape(-1, 3)).reshape(B, I - 1)
                bad = hit[:, None] & (rows < 0)
                if bad.any():
                    b_, j_ = np.argwhere(bad)[0]
                    raise KeyError("Inference, Key %d-%d-%d not found in clip_weight" % (u[b_], it[b_, j_ + 1], t[b_]))
                out[hit, 1:] = nv[rows[hit]]
        w = torch.from_numpy(out)
        return w.to(device) if device is not None else w


def _dense_map(d, device):
    """A str-keyed id dict of the reference (``id2user`` / ``id2item``) as the dense int64 map of ``segmm_store_lookup``: entry k = the
    value of key str(k), -1 where the dict has none."""
    ks = np.fromiter((int(k) for k in d), np.int64, len(d))
    if len(ks) and ks.min() < 0:
        raise ValueError("DeviceLogitStore: an id map with negative keys has no dense form")
    m = np.full((int(ks.max()) + 1 if len(ks) else 0,), -1, np.int64)
    m[ks] = np.fromiter((int(v) for v in d.values()), np.int64, len(d))
    return torch.from_numpy(m).to(device)


class DeviceLogitStore:
    """``LogitStore`` with the logits resident on the device from the forward that produced them to the head that consumes them.
    ``add_batch`` keeps device tensors and never synchronises; ``finalize`` sorts the three key columns on the host once (the
    values stay where they are) and uploads the index; ``lookup`` / ``weights`` / ``head`` answer the reader's rule
    (``LogitStore.weights``) with ``segmm_store_lookup`` and ``segmm_store_head`` (include/segmm_hip.h).  ``head`` forms no
    [B, I, S] tensor and is differentiable in ``pred``."""

    def __init__(self, S: int = 40, device="cuda", capacity=None):
        """``capacity`` (rows; None = the block list of ``add_batch``): the PREALLOCATED form -- one keys table [capacity, 3], one
        values table [capacity, S] and a host-side row count; ``append`` writes a batch at the count with one ``segmm_store_append``
        and the tables grow geometrically when a batch would not fit (``reserve`` sizes them ahead)."""
        self.S = S
        self.device = torch.device(device)
        self._keys = []          # device [n_i, 3] int64 blocks (the block-list form)
        self._vals = []          # device [n_i, S] float32 blocks
        self._ktab = self._vtab = None          # the preallocated form: tables [capacity, 3] int64 / [capacity, S] float32 ...
        self._n = 0                             # ... and the rows written so far (a host integer: no synchronisation)
        self._index = None       # (keys [n, 3] int64, rows [n] int32) on the device
        self._maps = {}          # id(dict) -> (dict, its length, dense device map): the last MAX_MAPS dicts
        if capacity is not None:
            if int(capacity) < 0:
                raise ValueError("DeviceLogitStore: capacity=%r" % (capacity,))
            self.reserve(int(capacity))

    # ---- writer side
    @property
    def capacity(self):
        """Rows of the preallocated tables; None in the block-list form."""
        return None if self._ktab is None else self._ktab.shape[0]

    def reserve(self, rows):
        """Makes room for ``rows`` rows in all (a block-list store becomes a preallocated one, its blocks the tables' first rows): new
        tables, the rows written so far moved by two ``segmm_copy_bytes`` on the stream.  No synchronisation."""
        from . import hipabi as H
        rows = int(rows)
        if self._ktab is None:
            k, v = self._cat()
            self._keys, self._vals = [], []
            old, self._n = (k, v), k.shape[0]
        else:
            old = (self._ktab, self._vtab)
        if self._ktab is not None and rows <= self._ktab.shape[0]:
            return self
        cap = max(rows, self._n)
        self._ktab = torch.empty((cap, 3), dtype=torch.int64, device=self.device)
        self._vtab = torch.empty((cap, self.S), dtype=torch.float32, device=self.device)
        if self._n:
            H.copy_bytes(self._ktab[:self._n], old[0][:self._n])
            H.copy_bytes(self._vtab[:self._n], old[1][:self._n])
        return self

    def _room(self, B):
        """The tables hold ``B`` more rows behind the count: grown geometrically when they do not."""
        if self._n + B > self._ktab.shape[0]:
            self.reserve(max(2 * self._ktab.shape[0], self._n + B))

    def append(self, user_id, photo_id, time_ms, logits):
        """One batch at the current row count (preallocated form): device int64 [B] key columns, float32 [B, S] logits (any row stride),
        ONE ``segmm_store_append``.  Nothing is converted: anything else is refused by name."""
        from . import hipabi as H
        if self._ktab is None:
            raise RuntimeError("DeviceLogitStore.append: the store has no preallocated tables (DeviceLogitStore(capacity=...) or reserve())")
        if logits.dim() != 2 or logits.shape[1] != self.S:
            raise ValueError("logits have %s segments, store expects %d" % (list(logits.shape[1:]), self.S))
        B = logits.shape[0]
        self._room(B)
        H.store_append(user_id, photo_id, time_ms, logits, self._n, self._ktab, self._vtab)
        self._n += B
        self._index = None

    def add_batch(self, user_id, photo_id, time_ms, logits):
        if self._ktab is not None:
            k = [torch.as_tensor(v).to(self.device, torch.int64).reshape(-1).contiguous() for v in (user_id, photo_id, time_ms)]
            v = torch.as_tensor(logits).detach().to(self.device, torch.float32).reshape(k[0].shape[0], -1)
            if v.shape[1] != self.S:
                raise ValueError("logits have %d segments, store expects %d" % (v.shape[1], self.S))
            return self.append(k[0], k[1], k[2], v.contiguous())
        k = torch.stack([torch.as_tensor(v).to(self.device, torch.int64).reshape(-1) for v in (user_id, photo_id, time_ms)], 1)
        v = torch.as_tensor(logits).detach().to(self.device, torch.float32, copy=True).reshape(k.shape[0], -1)          # a copy: forward buffers are reused
        if v.shape[1] != self.S:
            raise ValueError("logits have %d segments, store expects %d" % (v.shape[1], self.S))
        self._keys.append(k)
        self._vals.append(v)
        self._index = None

    def _cat(self):
        if self._ktab is not None:          # the rows appended so far: views of the tables
            return self._ktab[:self._n], self._vtab[:self._n]
        if len(self._keys) > 1:
            self._keys, self._vals = [torch.cat(self._keys, 0)], [torch.cat(self._vals, 0)]
        if not self._keys:
            self._keys = [torch.zeros((0, 3), dtype=torch.int64, device=self.device)]
            self._vals = [torch.zeros((0, self.S), dtype=torch.float32, device=self.device)]
        return self._keys[0], self._vals[0]

    def __len__(self):
        if self._ktab is not None:
            return self._n
        return sum(k.shape[0] for k in self._keys)

    def finalize(self, on_device=False):
        """Builds the index by ``LogitStore``'s rule (lexicographic order, last occurrence of a key wins): ONE device-to-host copy
        of the key columns, the sort on the host, the sorted keys and their value rows back up.
        ``on_device=True`` (opt-in): the same index from ``segmm_store_index`` -- sort, run flags, scan and compaction as launches on
        the stream, then ONE 8-byte read-back (the number of distinct keys, the pass's only synchronisation) to shape the index
        tensors.  Built for up to ``hipabi.STORE_INDEX_MAX`` keys; beyond, the library refuses by name and this default still works."""
        if self._index is None and on_device:
            from . import hipabi as H
            k, _ = self._cat()
            ok, orows, nu = H.store_index(k)
            m = int(nu.item())
            # (copies when keys repeated: the views would keep the full [n, 3] / [n] outputs alive for the life of the index)
            self._index = (ok, orows) if m == k.shape[0] else (ok[:m].clone(), orows[:m].clone())
        if self._index is None:
            k, _ = self._cat()
            h = LogitStore(self.S)
            h._keys, h._vals = [k.cpu().numpy()], [np.zeros((k.shape[0], 0), np.float32)]
            h._build_index()
            ks, rows = h._index
            self._index = (torch.from_numpy(np.ascontiguousarray(ks)).to(self.device),
                           torch.from_numpy(rows.astype(np.int32)).to(self.device))
        return self

    @classmethod
    def from_store(cls, store: LogitStore, device="cuda"):
        k, v = store._cat()
        st = cls(S=store.S, device=device)
        st._keys, st._vals = [torch.from_numpy(np.ascontiguousarray(k, np.int64)).to(st.device)], [torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(st.device)]
        return st

    def to_store(self) -> LogitStore:
        """The host store of the same batches (one copy of the keys and the values): ``save_json`` / ``save_binary`` of it write the
        bytes a ``LogitStore`` fed the same batches writes."""
        k, v = self._cat()
        st = LogitStore(self.S)
        if k.shape[0]:
            st._keys, st._vals = [k.cpu().numpy()], [v.cpu().numpy()]
        return st

    # ---- reader side
    MAX_MAPS = 4          # id dicts whose dense form is kept (a store sees one id2user and one id2item)

    def _map(self, m):
        """The dense device map of an id dict, converted once and kept while the dict is the same object of the same length (a dict
        that is changed in place without changing its length must not be passed again: its dense form would be stale).  Device
        tensors pass through."""
        if m is None or torch.is_tensor(m):
            return None if m is None else m.to(self.device, torch.int64).contiguous()
        hit = self._maps.get(id(m))
        if hit is None or hit[0] is not m or hit[1] != len(m):
            self._maps.pop(id(m), None)
            while len(self._maps) >= self.MAX_MAPS:
                self._maps.pop(next(iter(self._maps)))          # the oldest entry
            hit = self._maps[id(m)] = (m, len(m), _dense_map(m, self.device))
        return hit[2]

    def _query(self, user_id, item_ids, time_ms):
        q = [torch.as_tensor(x).to(self.device, torch.int64) for x in (user_id, item_ids, time_ms)]
        return q[0].reshape(-1).contiguous(), q[1].contiguous(), q[2].reshape(-1).contiguous()

    def lookup(self, user_id, item_ids, time_ms, neg: "Optional[DeviceLogitStore]" = None, id2user=None, id2item=None, check=True):
        """rowidx int32 [B, I] of the batch (``segmm_store_lookup``: -1 = ones, r >= 0 = this store's value row r, r <= -2 = row
        -2 - r of ``neg``).  ``check=True`` reads the two miss slots once and raises what ``LogitStore.weights`` raises; ``check=False``
        returns (rowidx, miss) and does not synchronise."""
        from . import hipabi as H
        self.finalize()
        u, it, t = self._query(user_id, item_ids, time_ms)
        um, im = self._map(id2user), self._map(id2item)
        nidx = neg.finalize()._index if neg is not None else (None, None)
        rowidx, miss = H.store_lookup(u, it, t, *self._index, neg_keys=nidx[0], neg_rows=nidx[1], user_map=um, item_map=im)
        if not check:
            return rowidx, miss
        m0, m1 = miss.tolist()
        if m1 != H.STORE_MISS_NONE:          # the id maps are applied first, users before items (LogitStore.weights)
            for ids, mp in ((u, um), (it.reshape(-1), im)):
                if mp is not None:
                    bad = (ids < 0) | (ids >= mp.numel())
                    bad = bad | (mp[ids.clamp(0, max(mp.numel() - 1, 0))] < 0) if mp.numel() else torch.ones_like(bad)
                    if bool(bad.any()):
                        raise KeyError(str(int(ids[int(torch.nonzero(bad)[0])])))
        if m0 != H.STORE_MISS_NONE:
            b, j = divmod(m0, it.shape[1])
            uu, ii = (int(u[b]) if um is None else int(um[u[b]])), (int(it[b, j]) if im is None else int(im[it[b, j]]))
            raise KeyError("Inference, Key %d-%d-%d not found in clip_weight" % (uu, ii, int(t[b])))
        return rowidx

    def _neg_vals(self, neg):
        return None if neg is None else neg._cat()[1]

    def weights(self, user_id, item_ids, time_ms, neg: "Optional[DeviceLogitStore]" = None, id2user=None, id2item=None):
        """``LogitStore.weights`` on the device: float32 [B, I, S], a copy of the stored rows."""
        from . import hipabi as H
        rowidx = self.lookup(user_id, item_ids, time_ms, neg=neg, id2user=id2user, id2item=id2item)
        return H.store_head(None, rowidx, self._cat()[1], self._neg_vals(neg))

    def head(self, pred, user_id, item_ids, time_ms, duration=None, neg: "Optional[DeviceLogitStore]" = None, id2user=None, id2item=None,
             check=True):
        """ClipRec's ``(clip_predictions * c_interest_weight * mask).sum(-1)`` for a batch of queries: pred [B, I, S] -> [B, I],
        the weights read from the store's rows by the kernel; differentiable in ``pred`` (the backward keeps rowidx, not weights).
        ``check=False`` does not synchronise and returns (out, miss): a missing negatives key or id counts as ones in ``out``, and
        ``miss`` (``lookup``'s two slots) is how the caller finds out."""
        r = self.lookup(user_id, item_ids, time_ms, neg=neg, id2user=id2user, id2item=id2item, check=check)
        rowidx, miss = (r, None) if check else r
        if duration is not None:
            duration = torch.as_tensor(duration).to(self.device, torch.int64).contiguous()
        out = _StoreHead.apply(pred, rowidx, self._cat()[1], self._neg_vals(neg), duration)
        return out if check else (out, miss)


class _StoreHead(torch.autograd.Function):
    """``segmm_store_head`` / ``segmm_store_head_bwd``: the weights are constants named by rowidx"""

    @staticmethod
    def forward(ctx, pred, rowidx, vals, neg_vals, duration):
        from . import hipabi as H
        ctx.save_for_backward(rowidx, vals, neg_vals, duration)
        ctx.S = pred.shape[-1]
        return H.store_head(pred.detach().contiguous(), rowidx, vals, neg_vals, duration)

    @staticmethod
    def backward(ctx, g):
        from . import hipabi as H
        rowidx, vals, neg_vals, duration = ctx.saved_tensors
        return H.store_head_bwd(g.contiguous(), ctx.S, rowidx=rowidx, vals=vals, neg_vals=neg_vals, duration=duration), None, None, None, None


class _WeightedHead(torch.autograd.Function):
    """``segmm_segment_weighted_sum`` forward; d pred = g * weight * mask (``segmm_store_head_bwd`` with an explicit weight)"""

    @staticmethod
    def forward(ctx, pred, weight, duration):
        from . import hipabi as H
        ctx.save_for_backward(weight, duration)
        ctx.S = pred.shape[-1]
        return H.segment_weighted_sum(pred.detach(), weight, duration)

    @staticmethod
    def backward(ctx, g):
        from . import hipabi as H
        weight, duration = ctx.saved_tensors
        return H.store_head_bwd(g.contiguous(), ctx.S, weight=None if weight is None else weight.contiguous(),
                                duration=None if duration is None else duration.contiguous()), None, None


def weighted_head(pred: torch.Tensor, weight: Optional[torch.Tensor] = None, duration: Optional[torch.Tensor] = None):
    """ClipRec.forward's ``(clip_predictions * interest_weight * mask).sum(-1)`` (ClipRec.py:163-181) on the device; differentiable in
    ``pred`` (``weight`` and ``duration`` are constants)."""
    from . import hipabi as H
    if not pred.requires_grad or not torch.is_grad_enabled():
        return H.segment_weighted_sum(pred, weight, duration)
    return _WeightedHead.apply(pred, weight, duration)
