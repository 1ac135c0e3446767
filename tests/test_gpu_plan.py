"""``rwrt_launch_plan`` (csrc/plan.hip) against the torch expressions it
replaces in ``RayEngine.advance``: the work per ray, ``prev_work``, the live
count, the row slots of ``rwrt_row_slots`` and the queue order of
``RayEngine.cost_order``, element for element; and an ``advance`` with and
without it.

Shapes: one ray; one less and one more than a 256-thread block; 70 001 rays
(18 tiles of 4 096, several blocks of the radix sort).  Counts below 2^20 with
many ties (the order of equal work is part of the contract)."""
import numpy as np
import pytest
import torch

import _hip as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def case(n, frozen, seed):
    """A state, counters and an earlier ``prev_work`` for ``n`` rays of which
    the fraction ``frozen`` has a NaN somewhere in y."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((12, n))
    dead = rng.random(n) < frozen if 0.0 < frozen < 1.0 else np.full(n, frozen >= 1.0)
    s[rng.integers(0, 5, n)[dead], np.nonzero(dead)[0]] = np.nan
    # few distinct values (ties), and some up to 2^20
    since = np.where(rng.random(n) < 0.9, rng.integers(0, 40, n), rng.integers(0, 1 << 20, n))
    prev = rng.integers(0, 1000, n)
    acc = rng.integers(0, since + prev + 1)
    count = np.stack([acc, since + prev - acc], 1).astype(np.int64)
    st = dict(state=torch.as_tensor(s, device=DEV), count=torch.as_tensor(count, device=DEV), nray=n)
    return st, torch.as_tensor(prev.astype(np.int64), device=DEV)


def plan(ctx, st, prev, total):
    from engine import Slots
    n = st["nray"]
    work = torch.full((n,), -5, dtype=torch.int64, device=DEV)
    order = torch.full((n,), -5, dtype=torch.int64, device=DEV)
    sl = Slots(n, DEV)
    sl.slot.fill_(-9)
    n_live = ctx.launch_plan(n, total, st["state"], st["count"], prev, work, order, sl.slot, sl.n_dev)
    return work, order, sl, n_live


def check(ctx, st, prev, total):
    from engine import RayEngine, Slots
    n = st["nray"]
    state0, count0 = st["state"].clone(), st["count"].clone()
    want_work = st["count"].sum(1) - (0 if total else prev)
    want_prev = st["count"].sum(1)
    want_order = RayEngine.cost_order(st, want_work)
    want_live = int((~torch.isnan(st["state"][:5].sum(0))).sum().item())
    ref = Slots(n, DEV).compute(st, torch.cuda.current_stream().cuda_stream)
    work, order, sl, n_live = plan(ctx, st, prev, total)
    assert n_live == want_live == ref.count() == int(sl.n_dev.item())
    assert torch.equal(work, want_work)
    assert torch.equal(prev, want_prev)
    assert torch.equal(sl.slot, ref.slot)
    assert torch.equal(order, want_order)
    # (the inputs are read only)
    assert torch.equal(st["count"], count0)
    assert np.array_equal(state0.cpu().numpy().view(np.int64), st["state"].cpu().numpy().view(np.int64))


@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_plan_equals_the_torch_expressions(n):
    ctx = H.Context(DEV)
    for k, frozen in enumerate((1.0 / 3.0, 1.0, 0.0)):
        for total in (False, True):
            st, prev = case(n, frozen, 100 * n + k)
            check(ctx, st, prev, total)


def test_plan_scratch_regrows_with_n():
    """One context, a growing ray count: the scratch is grown on demand, and a
    smaller set afterwards runs in the larger scratch."""
    ctx = H.Context(DEV)
    sizes = []
    for n in (257, 70001, 1000):
        st, prev = case(n, 0.3, n)
        check(ctx, st, prev, False)
        sizes.append(ctx._plan_scratch.numel())
    assert sizes[0] < sizes[1] == sizes[2]


def test_plan_work_of_all_the_key_bits():
    """Work above 2^32 (more bits than a 32-bit key) still orders the rays."""
    st, prev = case(257, 0.3, 7)
    st["count"][::5, 0] += 1 << 40
    check(H.Context(DEV), st, prev, True)


class Dense:
    """A sink of dense rows: keeps every launch's."""

    def __init__(self):
        self.chunks = {}

    def __call__(self, i0, i1, view):
        self.chunks[i0] = (i1, view.clone())


class Blocks(Dense):
    """A sink of row blocks: keeps every launch's rows made dense."""
    takes_slots = True

    def __call__(self, i0, i1, view, tails, slots):
        self.chunks[i0] = (i1, slots.dense(view, tails, i0, i1).clone())


@pytest.fixture(scope="module")
def c3_257():
    from bench import make_bs
    from conftest import golden
    from engine import RayEngine
    from support.cases import c3_sample_y0
    bs, _ = make_bs("zonal")
    eng = RayEngine.from_bs(bs)
    y0 = c3_sample_y0(eng, n_dead=64)
    n_live = len(golden("c3_sample.npz")["idx"])
    # 193 live rays from across the cost strata, then the 64 dead slots
    sel = torch.cat([torch.arange(0, n_live, n_live // 193, device=eng.device)[:193],
                     torch.arange(n_live, n_live + 64, device=eng.device)])
    assert sel.numel() == 257
    return eng, y0[:, sel].contiguous()


def test_sharded_step_with_and_without_the_switches(c3_257, monkeypatch):
    """``shard.run_sharded`` with one rank (the bench's step): the endpoints
    that the launches store themselves (``Tails.row``), with the plan, equal
    those gathered from the rows (RWRT_LAST_ROWS=0) and those without the
    plan (RWRT_PLAN=0), bit for bit; so do the counters."""
    import engine
    import shard
    eng, y0 = c3_257
    nt = 29
    got = []
    for rows_stored, use in ((True, True), (False, True), (True, False), (False, False)):
        monkeypatch.setattr(engine, "LAST_ROWS", rows_stored)
        monkeypatch.setattr(eng, "use_plan", use, raising=False)
        r = shard.run_sharded(eng, y0, nt, 7200.0, rank=0, world=1, probe=2, lead=[6], chunk=12,
                              ttotal=(nt - 1) * 7200.0, team=[4, 64, 0])
        e = r.endpoints.cpu().numpy().copy()
        e[np.isnan(e)] = np.nan
        got.append((e.view(np.int64), r.counts.cpu().numpy(), list(eng.launch_log)))
    assert len(got[0][2]) == 3 and got[0][2][0]["n_heavy"] == 4
    # (both kinds of last row: the 64 dead slots' tails and live rays' stored rows)
    frozen_end = np.isnan(got[0][0].view(np.float64)[:, :5]).any(1)
    assert 64 <= frozen_end.sum() < y0.shape[1]
    for e, c, log in got[1:]:
        assert np.array_equal(e, got[0][0]) and np.array_equal(c, got[0][1]) and log == got[0][2]


@pytest.mark.parametrize("sink", [Dense, Blocks])
@pytest.mark.parametrize("policy", ["priority", "total"])
def test_advance_with_and_without_the_plan(c3_257, sink, policy, monkeypatch):
    """29 rows of 257 rays in four launches (the first orders live rays first,
    the others by work, two of them with rays in latency mode: team 4 and 64): the same
    rows, counters, state and launch log with RWRT_PLAN 1 and 0."""
    eng, y0 = c3_257
    nt = 29
    got = {}
    for use in (True, False):
        monkeypatch.setattr(eng, "use_plan", use, raising=False)
        rec = sink()
        res = eng.integrate(y0, nt, 7200.0, ttotal=(nt - 1) * 7200.0, chunk=12, first_chunk=[2, 6], sink=rec,
                            order_policy=policy, team=[0, 4, 64, 0])
        got[use] = (rec.chunks, res, list(eng.launch_log))
    (ca, ra, la), (cb, rb, lb) = got[True], got[False]
    assert la == lb and len(la) == 4 and la[1]["n_heavy"] == 4 and la[2]["n_heavy"] > 4
    assert sorted(ca) == sorted(cb)
    for i0 in ca:
        assert ca[i0][0] == cb[i0][0]
        assert np.array_equal(ca[i0][1].cpu().numpy().view(np.int64), cb[i0][1].cpu().numpy().view(np.int64)), i0
    for name in ("nacc", "nrej", "nanrow"):
        assert torch.equal(getattr(ra, name), getattr(rb, name)), name
    assert np.array_equal(ra.state["state"].cpu().numpy().view(np.int64),
                          rb.state["state"].cpu().numpy().view(np.int64))
