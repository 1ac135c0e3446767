"""Every ray's last row of a tails launch is in ``Tails.row``.

``rwrt_rk45_run_tails`` / ``_slots`` and their time-varying twins store ray
j's row ``it_end - 1`` into ``d_tail_row[j]`` where they write its state back
(a ray frozen at the launch's start has it from ``frozen_tail_kernel``), so
``Tails.last_row`` / ``Slots.last_row`` are ``tails.row`` itself.  Checked
after each of two launches, rows [1, 5) then [5, 29), against the dense rows
of ``rwrt_rk45_run`` on the same rays, bit for bit (NaN equal to NaN), with
``tails.frm`` what it was (the launch's start for a ray frozen there, its end
for every other ray):

* ``nray`` 1, 63, 65 (one more than a wave) and 257 (one more than a block),
  live C3 sample rays, dead root slots and rays that the jump mask freezes
  inside the second launch; a set that is frozen entirely;
* the ordinary ray loop with the drain-time hand-off off, the quad latency
  mode (``n_heavy`` 4 and 64), and the hand-off at its largest threshold, 16
  rays per wave (the quad layout holds 16 rays: every drained wave hands off);
* dense rows with tails and row blocks;
* the time-varying loops on small level sets: fp64 at 32 and 64 lanes, fp32
  storage, latency waves (one ray per wave).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = 7.25
NT = 29
BOUNDS = ((1, 5), (5, 29))


def bits(t):
    a = t.detach().cpu().numpy().astype(np.float64, copy=True)
    a[np.isnan(a)] = np.nan
    return a.view(np.int64)


def frozen_of(st):
    return torch.isnan(st["state"][:5].sum(0))


def check_launches(eng, y0, nt, bounds, n_heavy=0, per_wave=16, slots=False):
    """Both launches, dense and with tails, from the same initial state; the
    rays handed off by the tails launches."""
    from engine import Slots, Tails, t_eval_of
    n = y0.shape[1]
    p = eng.params(nt, 7200.0)
    tb = torch.as_tensor(t_eval_of(nt, 7200.0, (nt - 1) * 7200.0), dtype=torch.float64, device=eng.device)
    sd, st = eng.init(y0, p), eng.init(y0, p)
    moved = 0
    for i0, i1 in bounds:
        frozen0 = frozen_of(st)
        assert torch.equal(frozen0, frozen_of(sd))
        order = eng.live_first_order_of(st)
        nh = min(n_heavy, int((~frozen0).sum().item()))
        dense = torch.full((n, i1 - i0, 8), SENTINEL, dtype=torch.float64, device=eng.device)
        eng.run(sd, p, tb, i0, i1, dense, order, nh, per_wave)
        tails = Tails(n, eng.device)
        tails.row.fill_(SENTINEL)
        sl = Slots(n, eng.device).compute(st, eng._stream()) if slots else None
        rows = torch.full((max(1, sl.count()) if slots else n, i1 - i0, 8), SENTINEL, dtype=torch.float64,
                          device=eng.device)
        eng.run(st, p, tb, i0, i1, rows, order, nh, per_wave, tails, sl)
        moved += int(eng.work[0].item())
        assert np.array_equal(bits(tails.row), bits(dense[:, -1])), f"launch [{i0}, {i1}): last rows differ"
        want_frm = torch.where(frozen0, i0, i1).to(torch.int32)
        assert torch.equal(tails.frm, want_frm), f"launch [{i0}, {i1}): tail_from changed"
        assert tails.last_row(rows, i1) is tails.row
        if slots:
            assert sl.last_row(rows, tails, i1) is tails.row
        assert np.array_equal(bits(st["state"]), bits(sd["state"]))
        assert torch.equal(st["count"], sd["count"]) and torch.equal(st["nanrow"], sd["nanrow"])
    return moved


@pytest.fixture(scope="module", params=["zonal", "nonzonal"])
def c3(request):
    """The engine, the C3 sample with 128 dead slots, and for every ray the
    first row at which it is frozen (from one dense launch; NT: never)."""
    from bench import make_bs
    from engine import RayEngine, t_eval_of
    from support.cases import c3_sample_y0
    bs, _ = make_bs(request.param)
    eng = RayEngine.from_bs(bs)
    y0 = c3_sample_y0(eng, n_dead=128)
    p = eng.params(NT, 7200.0)
    tb = torch.as_tensor(t_eval_of(NT, 7200.0, (NT - 1) * 7200.0), dtype=torch.float64, device=eng.device)
    st = eng.init(y0, p)
    out = torch.empty((y0.shape[1], NT - 1, 8), dtype=torch.float64, device=eng.device)
    eng.run(st, p, tb, 1, NT, out, eng.live_first_order_of(st))
    nan = torch.isnan(out[:, :, :5].sum(2)).cpu().numpy()
    first = np.where(nan.any(1), nan.argmax(1) + 1, NT)
    yield eng, y0, first
    eng.handoff = 16


def pick(first, n):
    """``n`` rays: up to two that freeze inside the second launch, a quarter
    dead slots, the rest live to the end (cost-stratified: the sample's order)."""
    mid = np.nonzero((first > BOUNDS[1][0]) & (first < NT))[0][: min(2, n // 8)]
    dead = np.nonzero(first == 1)[0][-(n // 4):] if n >= 4 else np.zeros(0, np.int64)
    live = np.nonzero(first == NT)[0]
    live = live[:: max(1, len(live) // n)][: n - len(mid) - len(dead)]
    sel = np.sort(np.concatenate([mid, dead, live]))
    assert len(sel) == n
    return sel, len(mid)


@pytest.mark.parametrize("nray", [1, 63, 65, 257])
def test_static_last_rows(c3, nray):
    eng, y0, first = c3
    sel, n_mid = pick(first, nray)
    assert n_mid > 0 or nray < 8      # (a ray that the jump mask freezes inside the second launch)
    y = y0[:, torch.as_tensor(sel, device=eng.device)].contiguous()
    for slots in (False, True):
        eng.handoff = 0               # (a) the ordinary loop
        assert check_launches(eng, y, NT, BOUNDS, slots=slots) == 0
        for n_heavy in (4, 64):       # (b) the quad latency mode
            check_launches(eng, y, NT, BOUNDS, n_heavy=n_heavy, slots=slots)
        eng.handoff = 16              # (c) every drained wave hands its rays off
        assert check_launches(eng, y, NT, BOUNDS, slots=slots) > 0


def test_static_last_rows_of_a_frozen_set(c3):
    eng, y0, first = c3
    dead = np.nonzero(first == 1)[0][:65]
    y = y0[:, torch.as_tensor(dead, device=eng.device)].contiguous()
    for slots in (False, True):
        check_launches(eng, y, NT, BOUNDS, slots=slots)
        check_launches(eng, y, NT, BOUNDS, n_heavy=4, slots=slots)


@pytest.fixture(scope="module")
def levels_y0():
    import rwrt_oracle as O
    import synthetic as S
    from engine import RayEngine
    from levels import Levels
    nlev = 9
    bl = [S.background_level(j, res=0.25) for j in range(nlev)]
    made = {}

    def make(fp32):
        if fp32 not in made:
            lv = Levels(bl[0]["lat"], bl[0]["lon"], nlev, t0=0.0, dt=6 * 3600.0, fp32=fp32)
            for j, b in enumerate(bl):
                lv.set_level(j, b["u"], b["v"])
            eng = RayEngine.from_levels(lv)
            cfg = S.config("C5")
            slon, slat = O.source_matrix(cfg.SW_lon, cfg.SW_lat, cfg.dlon, cfg.dlat, cfg.nnx, cfg.nny)
            rows = eng.initial_rows(slon, slat, cfg.zwn, S.c3_freq(S.C5_PERIODS_DAYS[-1])).cpu().numpy()
            y0 = rows[:5].reshape(5, -1)
            sel = np.sort(np.random.default_rng(5).choice(y0.shape[1], size=257, replace=False))
            y0 = y0[:, sel].copy()
            y0[2, ::9] = np.nan          # dead slots among them
            made[fp32] = (eng, torch.as_tensor(y0, device=eng.device))
        return made[fp32]
    return make


@pytest.mark.parametrize("fp32,lanes,n_heavy", [(False, 32, 0), (False, 64, 0), (True, 64, 0), (False, 32, 4)])
def test_time_varying_last_rows(levels_y0, fp32, lanes, n_heavy):
    """fp64 levels at 32 and 64 lanes, fp32 storage, and latency waves (four
    rays, one per wave)."""
    eng, y0 = levels_y0(fp32)
    eng.tv_lanes = lanes
    for slots in (False, True):
        check_launches(eng, y0, 13, ((1, 5), (5, 13)), n_heavy=n_heavy, per_wave=1, slots=slots)
