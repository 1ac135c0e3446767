"""A launch's rows: what a ray-loop launch leaves on the device and how it
reaches a consumer (csrc/launch_rows.h is the device side).

Rows ``[i0, i1)`` come dense (``view[nray, i1-i0, 8]``), with ``tails``
(``engine.Tails``) or as row blocks (``slots``, ``engine.Slots``, with tails).
A sink is called ``sink(i0, i1, view[, tails[, slots]])`` by the engine and
``sink(i0, i1, rows, idx[, tails[, slots]])`` by ``shard.run_sharded`` (``idx``:
the shard's ray indices), ``tails`` / ``slots`` also as keywords; it is given
tails only with ``takes_tails`` and row blocks only with ``takes_slots``
(``deliver``).
"""
import copy

import numpy as np

import _hip as H


def row_args(i0, i1, view, tails=None, slots=None):
    """``(nray, (d_rows, d_row_slot, d_tail_from, d_tail_row))`` of the launch's
    rows ``[i0, i1)`` for a C entry point that reads them."""
    import torch
    if slots is not None and tails is None:
        raise ValueError("row slots need tails")
    if view.ndim != 3 or view.shape[2] != H.NOUT or view.shape[1] != i1 - i0:
        raise ValueError(f"rows must be [n, {i1 - i0}, {H.NOUT}], got {tuple(view.shape)}")
    nray = int(slots.slot.numel() if slots is not None else view.shape[0])
    if tails is not None and tails.frm.numel() != nray:
        raise ValueError(f"tails of {tails.frm.numel()} rays for {nray} rays")
    return nray, (H.dptr(view, torch.float64, "rows"),
                  None if slots is None else H.dptr(slots.slot, torch.int32),
                  None if tails is None else H.dptr(tails.frm, torch.int32),
                  None if tails is None else H.dptr(tails.row, torch.float64))


def one_row(columns, device):
    """Single points as a launch of one row: a ``[n, 1, 8]`` tensor with
    ``columns`` (``{column: values}``, of any shape) set and zeros elsewhere."""
    import torch
    cols = {c: torch.as_tensor(v, dtype=torch.float64).reshape(-1).to(device) for c, v in columns.items()}
    rows = torch.zeros((next(iter(cols.values())).numel(), 1, H.NOUT), dtype=torch.float64, device=device)
    for c, v in cols.items():
        rows[:, 0, c] = v
    return rows


def split_call(rest, tails, slots):
    """A sink's two call forms (above) -> (idx, tails, slots)."""
    import torch
    idx = None
    if rest and (torch.is_tensor(rest[0]) or isinstance(rest[0], np.ndarray)):
        idx, rest = rest[0], rest[1:]
    if len(rest) > 0:
        tails = rest[0]
    if len(rest) > 1:
        slots = rest[1]
    return idx, tails, slots


class RowSink:
    """A sink that hands each launch's rows to ``target.add_rows(i0, i1, view,
    tails, slots, per_ray)`` where they lie: row blocks and tails as they are,
    enqueued on the engine's stream, nothing copied to the host.  ``per_ray``:
    one value per ray of the integration (a device tensor, or None); a
    subclass's ``select(idx)`` gives it for the rays ``idx`` (int64 tensor)."""
    takes_tails = True
    takes_slots = True

    def __init__(self, target, per_ray=None):
        self.target, self.per_ray = target, per_ray
        self._sub = (None, None)   # (idx, per_ray under idx) of the last shard

    def _select(self, idx):
        import torch
        return self.select(torch.as_tensor(idx, device=self.target.device).to(torch.int64))

    def take(self, idx):
        """The sink of the rays ``idx`` (a shard integrated on its own)."""
        sink = copy.copy(self)
        sink.per_ray, sink._sub = self._select(idx), (None, None)
        return sink

    def __call__(self, i0, i1, view, *rest, tails=None, slots=None):
        idx, tails, slots = split_call(rest, tails, slots)
        per_ray = self.per_ray
        if idx is not None:
            if self._sub[0] is not idx:
                sel = self._select(idx)
                self._sub = (idx, None if sel is None else sel.contiguous())
            per_ray = self._sub[1]
        self.target.add_rows(i0, i1, view, tails, slots, per_ray)


def deliver(eng, sink, i0, i1, view, tails, slots=None, idx=None, scratch=None):
    """Hand a launch's rows to ``sink`` (with ``idx``: in the sharded form).
    Row blocks go to a sink that takes them, else they are made dense
    (``Slots.dense``; ``scratch``, a dict, keeps that buffer for the next
    launch); tails go to a sink that takes them, else ``eng.expand`` writes
    them into ``view``."""
    ids = () if idx is None else (idx,)
    if slots is not None:
        if getattr(sink, "takes_slots", False):
            return sink(i0, i1, view, *ids, tails, slots)
        scratch = {} if scratch is None else scratch
        view = scratch["dense"] = slots.dense(view, tails, i0, i1, scratch.get("dense"))
        tails = None
    if tails is not None and getattr(sink, "takes_tails", False):
        return sink(i0, i1, view, *ids, tails)
    if tails is not None:
        eng.expand(view, tails, i0, i1)
    return sink(i0, i1, view, *ids)
