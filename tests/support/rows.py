"""One logical launch and the three row layouts that can hold it.

A launch is a dictionary ``L``: ``i0, i1`` (its rows ``[i0, i1)``), ``rows``
``[nray, i1 - i0, 8]`` (what a dense launch writes), ``tail`` ``[nray, 8]`` and
``tf`` ``[nray]`` (ray j's rows from ``tf[j]`` on repeat ``tail[j]``; ``tf`` may
lie outside the launch) and ``chan`` ``[nray]``.  The layouts: ``dense`` (every
row), ``tails`` (the rows before each ray's tail; the others hold a sentinel
that must never be read) and ``slots`` (those rows in permuted row blocks, the
rays of ``no_block`` without one)."""
import numpy as np

LAYOUTS = ("dense", "tails", "slots")
SENTINEL = {0: 1.0, 1: 0.1, 4: 5.0}   # column -> value: finite, binnable: must never be counted


def no_block(nray):
    """The rays without a row block in the slots layout: every third one, from
    ray 0 (their ``tf`` is at most ``i0``: all tail)."""
    return np.arange(nray) % 3 == 0


def unread(L, sentinel):
    """The launch's row buffer with tails: ray j's rows from ``tf[j]`` on are
    zero with ``sentinel``'s ``{column: value}`` on top."""
    i0, i1 = L["i0"], L["i1"]
    buf = L["rows"].copy()
    cut = np.clip(L["tf"], i0, i1)
    for j in range(buf.shape[0]):
        buf[j, cut[j] - i0:] = 0.0
        for c, v in sentinel.items():
            buf[j, cut[j] - i0:, c] = v
    return buf


def blocks_of(buf, live, seed):
    """``(blocks, slot)``: the rows of the rays ``live`` as row blocks in a
    permuted order, and each ray's block (-1: none)."""
    slot = np.full(buf.shape[0], -1, np.int32)
    slot[live] = np.random.default_rng(seed).permutation(len(live)).astype(np.int32)
    blocks = np.empty((len(live),) + buf.shape[1:])
    blocks[slot[live]] = buf[live]
    return blocks, slot


def layout_text(L, layout, sentinel=SENTINEL, seed=1):
    """The launch in one of the three row layouts, as a host program reads it
    (tests/host/launch_input.h)."""
    i0, i1, tail, tf, chan = (L[k] for k in ("i0", "i1", "tail", "tf", "chan"))
    nray = L["rows"].shape[0]
    hexrow = lambda r: " ".join(float(x).hex() for x in r)       # noqa: E731
    out = []
    buf = L["rows"].copy() if layout == "dense" else unread(L, sentinel)
    slot = None
    if layout == "slots":
        buf, slot = blocks_of(buf, np.where(~no_block(nray))[0], seed)
    out.append(f"{nray} {i0} {i1} {int(layout != 'dense')} {int(layout == 'slots')} {buf.shape[0]}")
    out.append(" ".join(str(int(c)) for c in chan))
    if layout != "dense":
        out.append(" ".join(str(int(t)) for t in tf))
        out += [hexrow(tail[j]) for j in range(nray)]
    if slot is not None:
        out.append(" ".join(str(int(s)) for s in slot))
    out += [hexrow(r) for r in buf.reshape(-1, 8)]
    return out


def layout_device(L, sentinel, seed=1, device="cuda", live=None):
    """``name -> (view, Tails, Slots)`` device objects of the launch's logical
    rows.  ``live``: the rays with a row block (default: all but ``no_block``)."""
    import torch
    from engine import Slots, Tails
    rows = L["rows"]
    nray = rows.shape[0]
    out = {"dense": (torch.as_tensor(rows, device=device).contiguous(), None, None)}
    buf = unread(L, sentinel)
    t = Tails(nray, device)
    t.frm.copy_(torch.as_tensor(L["tf"]))
    t.row.copy_(torch.as_tensor(L["tail"]))
    out["tails"] = (torch.as_tensor(buf, device=device).contiguous(), t, None)
    blocks, slot = blocks_of(buf, np.where(~no_block(nray))[0] if live is None else live, seed)
    s = Slots(nray, device)
    s.slot.copy_(torch.as_tensor(slot))
    out["slots"] = (torch.as_tensor(blocks, device=device).contiguous(), t, s)
    return out
