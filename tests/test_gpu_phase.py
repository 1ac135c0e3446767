"""The WKB phase along rays and wave-field maps on the GPU (``rwrt_ray_phase``,
phase.py): ``cnt``, ``nseg`` and ``dropped`` equal the definition
``phase.reference_phase`` exactly, ``theta`` agrees within ``1e-12 max(S, 1)``
(``S`` the sum of ``|dk| + |dl|`` along the ray: theta itself cancels), and
per box ``re`` and ``im`` within ``(1e-12 max(S_max, 1) + 2 (n + 1) 2^-53)
wabs`` and ``wabs`` within the rounding bound of a sum taken in any order --
for crafted rows in every row layout (dense, tails, row blocks), in chunks,
across shards, after a restart, through ``WR.ray_phase`` forward and backward
on real rays, next to a ``DensitySink`` in one ``Tee`` and through
``EnsembleWR.reduce`` over a member stack.

Fixture of the real rays: the zonal and the non-zonal state at 2.5 degrees,
4 x 4 sources x 4 wavenumbers x 3 roots = 192 slots, 181 rows of 2 h
(tests/support/backward.py); each history, reference and map is computed once
per module."""
import math

import numpy as np
import pytest
import torch

import phase as P
from density import DensityMap, DensitySink, DensitySpec, with_channels
from engine import Tails
from phase import PhaseMap, PhaseSink, PhaseSpec, reference_phase
from summary import Tee
from support.backward import KINDS, NT, TSTEP, cfg
from support.cases import bs_of
from support.cases_phase import (NRAY, VARIANTS, assert_phase, assert_same_run, crafted_history, crafted_spec,
                                 device_layouts, numpy_with_carry, start, sum_bound, wabs_ref)
from support.dist import one_rank
from support.rows import LAYOUTS

pytestmark = pytest.mark.gpu
DEV = "cuda"
NT_CRAFTED = 24
CHUNKS = [(1, 9), (9, 10), (10, 24)]


# ------------------------------------------------- crafted rows, entry point
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_crafted_rows_every_layout(name):
    """Row 0 and the launch [1, 24) of the host tests (41 rays: a partial
    wave), every layout, sentinel rows where nothing may be read, a theta0 per
    ray: the bars of the module's docstring; row 0 alone deposits and leaves
    theta at theta0."""
    spec = crafted_spec(name)
    h = crafted_history(NT_CRAFTED, seed=3)
    assert {-1, 1, 23, 24, 27} <= set(h["tf"].tolist()) and {-1, 3} <= set(h["chan"].tolist())
    theta0 = np.linspace(-1.0, 1.0, NRAY)
    want = reference_phase(h["rows"], h["chan"], spec, theta0)
    assert want["nseg"].sum() > 200 and want["cnt"].sum() > 200 and np.count_nonzero(want["cnt"]) > 20
    row0 = reference_phase(h["rows"][:, :1], h["chan"], spec, theta0)
    for layout, (view, tails, slots) in device_layouts(h, 1, NT_CRAFTED).items():
        m = start(PhaseMap(spec, NRAY, DEV, h["chan"], theta0), h["rows"][:, 0])
        assert_phase(m.numpy(), row0, (name, layout, "row 0"))
        assert row0["cnt"].sum() > 10 and np.array_equal(m.numpy()["theta"], theta0)
        m.add_rows(1, NT_CRAFTED, view, tails, slots)
        assert_phase(m.numpy(), want, (name, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["7x5-amp", "36x18-unweighted-omega"])
def test_chunks_give_what_one_launch_gives(name, layout):
    """The launches [1, 9), [9, 10) and [10, 24) against one launch [1, 24):
    theta, nseg, the carried rows and cnt bit for bit, the sums within the
    bound; a second row 0 (it_begin == 0) starts over whatever is carried."""
    spec = crafted_spec(name)
    h = crafted_history(NT_CRAFTED, seed=4)
    want = reference_phase(h["rows"], h["chan"], spec)
    one = start(PhaseMap(spec, NRAY, DEV, h["chan"]), h["rows"][:, 0])
    one.add_rows(1, NT_CRAFTED, *device_layouts(h, 1, NT_CRAFTED)[layout])
    three = start(PhaseMap(spec, NRAY, DEV, h["chan"]), h["rows"][:, 0])
    for i0, i1 in CHUNKS:
        three.add_rows(i0, i1, *device_layouts(h, i0, i1)[layout])
    a, b = numpy_with_carry(one), numpy_with_carry(three)
    assert_phase(a, want, (name, layout))
    assert_phase(b, want, (name, layout, "chunks"))
    assert_same_run(a, b, want, (name, layout))
    live = P.phase_valid(h["rows"], spec)[:, -1] & (h["chan"] >= 0) & (h["chan"] < 3)
    assert live.sum() > 5 and np.array_equal(a["carry"][:3, live], h["rows"][live, -1, :3].T)
    assert np.isnan(a["carry"][0, ~live]).all()
    # row 0 again without a restart: the carried rows are not joined to it
    before = one.numpy()
    start(one, h["rows"][:, 0])
    after = one.numpy()
    row0 = reference_phase(h["rows"][:, :1], h["chan"], spec)
    assert np.array_equal(after["nseg"], before["nseg"]) and np.array_equal(after["theta"], before["theta"])
    assert np.array_equal(after["cnt"], before["cnt"] + row0["cnt"])


def test_restart_forgets_the_carry_and_keeps_the_sums():
    """[1, 9), restart(), [9, 24): the segment into row 9 is not joined -- the
    history with an invalid row put between rows 8 and 9 (omega_dt == 0: the
    row numbers do not matter)."""
    spec = crafted_spec("7x5-amp")
    h = crafted_history(NT_CRAFTED, seed=4)
    m = start(PhaseMap(spec, NRAY, DEV, h["chan"]), h["rows"][:, 0])
    m.add_rows(1, 9, *device_layouts(h, 1, 9)["tails"])
    kept = m.numpy()
    assert m.restart() is m and torch.isnan(m.prev).all() and tuple(m.prev.shape) == (4, NRAY)
    again = m.numpy()
    for k in ("cnt", "re", "im", "wabs", "theta", "nseg"):
        assert np.array_equal(kept[k], again[k]), k
    m.add_rows(9, NT_CRAFTED, *device_layouts(h, 9, NT_CRAFTED)["tails"])
    holed = np.concatenate([h["rows"][:, :9], np.full((NRAY, 1, 8), np.nan), h["rows"][:, 9:]], axis=1)
    want = reference_phase(holed, h["chan"], spec)
    whole = reference_phase(h["rows"], h["chan"], spec)
    assert want["nseg"].sum() < whole["nseg"].sum() and np.array_equal(want["cnt"], whole["cnt"])
    assert_phase(m.numpy(), want, "restart")


def test_shards_add_up():
    """Two maps fed disjoint ray subsets through ``ray`` columns, then added,
    and one map fed the two subsets one after the other, against one map of
    all rays."""
    spec = crafted_spec("36x18-ug-no-need")
    h = crafted_history(NT_CRAFTED, seed=5, tf=np.full(NRAY, NT_CRAFTED))
    theta0 = np.linspace(0.5, -0.5, NRAY)
    want = reference_phase(h["rows"], h["chan"], spec, theta0)
    perm = np.random.default_rng(1).permutation(NRAY)
    parts = [np.sort(perm[:17]), perm[17:]]                     # (the second one not in column order)
    rows = torch.as_tensor(h["rows"], device=DEV)
    maps = [PhaseMap(spec, NRAY, DEV, h["chan"], theta0) for _ in parts]
    both = PhaseMap(spec, NRAY, DEV, h["chan"], theta0)
    for m, idx in zip(maps, parts):
        ray = torch.as_tensor(idx, device=DEV)
        for t in (m, both):
            t.add_rows(0, 1, rows[ray, :1].contiguous(), ray=ray)
            t.add_rows(1, NT_CRAFTED, rows[ray, 1:].contiguous(), ray=ray)
    assert_phase(both.numpy(), want, "one map, two shards")
    a, b = (m.numpy() for m in maps)
    added = {k: a[k] + b[k] for k in ("cnt", "re", "im", "wabs", "nseg", "dropped")}
    added["theta"] = theta0 + ((a["theta"] - theta0) + (b["theta"] - theta0))
    other = np.setdiff1d(np.arange(NRAY), parts[0])
    assert np.array_equal(a["theta"][other], theta0[other]) and a["nseg"][other].sum() == 0
    assert_phase(added, want, "two maps added")
    with pytest.raises(ValueError):
        both.add_rows(1, 2, rows[:5, 1:2].contiguous())          # 5 rays for 41 columns and no ray
    with pytest.raises(ValueError):
        PhaseMap(spec, NRAY, DEV).start(h["rows"][:, 0, 0], h["rows"][:, 0, 1], v=h["rows"][:, 0, 5])   # no k, l


def test_a_psi_that_is_not_finite_is_dropped():
    """k0 + k1 overflows: theta is infinite from row 1 on and every binned row
    is counted in dropped, the rows of a tail too; next to it a finite ray
    whose tail of 3 rows is 3 deposits and 2 more segments."""
    spec = PhaseSpec(8, 4, weight="amp")
    rows = np.zeros((2, 6, 8))
    rows[:, :, 0] = 0.25 * np.arange(6)
    rows[:, :, 4] = 1.5
    rows[0, :, 2] = 1e308
    rows[1, :, 2] = 2.0
    rows[:, 3:] = rows[:, 3:4]
    want = reference_phase(rows, None, spec)
    assert want["dropped"] == 5 and want["cnt"].sum() == 7 and want["nseg"].tolist() == [5, 5]
    for tailed in (False, True):
        m = start(PhaseMap(spec, 2, DEV), rows[:, 0])
        if tailed:
            tails = Tails(2, DEV)
            tails.frm.fill_(3)
            tails.row.copy_(torch.as_tensor(rows[:, 3]))
            buf = rows[:, 1:].copy()
            buf[:, 2:, 0] = 3.0                                   # sentinel rows: never read
            m.add_rows(1, 6, torch.as_tensor(buf, device=DEV), tails)
        else:
            m.add_rows(1, 6, torch.as_tensor(rows[:, 1:], device=DEV))
        got = m.numpy()
        assert_phase(got, want, ("dropped", tailed))
        assert got["theta"][1] == 1.5 and not np.isfinite(got["theta"][0])


def test_contention_one_box():
    """4 160 rays into the same box at every row, with k = l = 0 and a dyadic
    amplitude (psi == 0: every term is w itself): re == n w and im == 0
    exactly, in any order."""
    nray = 4160
    rows = np.zeros((nray, 3, 8))
    rows[:, :, 0], rows[:, :, 1] = [0.1, 0.2, 0.3], 0.05
    rows[:, :, 4] = 0.75
    spec = PhaseSpec(36, 18)
    m = start(PhaseMap(spec, nray, DEV), rows[:, 0])
    m.add_rows(1, 3, torch.as_tensor(rows[:, 1:], device=DEV))
    got = m.numpy()
    assert_phase(got, reference_phase(rows, None, spec), "contention")
    assert np.count_nonzero(got["cnt"]) == 2 and got["cnt"].sum() == 3 * nray
    assert got["re"].sum() == 0.75 * 3 * nray == got["wabs"].sum() and got["im"].sum() == 0.0


# ------------------------------------------------------------- real rays
SPEC = PhaseSpec(36, 18)
_REAL = {}


def _wr(kind, backward=False):
    from wr import WR
    c = cfg()
    bs = bs_of(kind)
    w = WR(c.nzwn, c.nsource, TSTEP, (NT - 1) * TSTEP, 0.0, nx=bs.nlon, ny=bs.nlat, backward=backward)
    w.bs = bs
    w.set_zwn(c.zwn)
    w.set_source_matrix(c.SW_lon, c.SW_lat, c.dlon, c.dlat, c.nnx, c.nny)
    return w


def real(kind, backward=False):
    """``ray_run``'s history ``[192, 181, 8]``, its reference and the map of
    ``WR.ray_phase`` -- computed once."""
    key = (kind, backward)
    if key not in _REAL:
        with np.errstate(all="ignore"):
            hist = _wr(kind, backward)._history_rows("rk45", "numpy", None)
            want = reference_phase(hist, None, SPEC)
            w = _wr(kind, backward)
            m = w.ray_phase(SPEC)
        assert np.isnan(w.rlon[1:]).all() and not np.isnan(w.rlon[0]).any()
        for a in [hist] + [v for v in want.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _REAL[key] = dict(hist=hist, want=want, map=m, got=m.numpy())
    return _REAL[key]


def _is_rich(f, kind):
    """What the comparisons need to see (else they could pass vacuously)."""
    hist, want = f["hist"], f["want"]
    ok = P.phase_valid(hist, SPEC)
    live0 = ok[:, 0]
    ends = live0 & ~ok.all(axis=1)
    fin = np.isfinite(want["theta"])
    print(f"{kind}: {int(live0.sum())} live rays, {int(ends.sum())} going invalid mid-run, "
          f"max |theta| {np.abs(want['theta'][fin]).max():.4g}, max S {want['S'][fin].max():.4g}, "
          f"{int(want['nseg'].sum())} segments, {int(want['cnt'].sum())} deposits, dropped {want['dropped']}")
    assert live0.sum() >= 30, (kind, int(live0.sum()))
    if kind == "nonzonal":
        assert ends.sum() >= 3, (kind, int(ends.sum()))
    assert np.abs(want["theta"][fin]).max() >= 10.0
    coh = f["map"].coherence().cpu().numpy()
    mixed = (want["cnt"] >= 2) & (coh < 0.9)
    print(f"{kind}: {int(mixed.sum())} boxes with cnt >= 2 and coherence < 0.9")
    assert mixed.sum() >= 20, (kind, int(mixed.sum()))


@pytest.mark.parametrize("kind", KINDS)
def test_ray_phase_equals_the_reference_on_the_history(kind):
    """WR.ray_phase forward against reference_phase of ray_run's history, and
    cnt against WR.ray_density's count on the same grid."""
    f = real(kind)
    _is_rich(f, kind)
    assert_phase(f["got"], f["want"], kind)
    with np.errstate(all="ignore"):
        dens = _wr(kind).ray_density(DensitySpec(36, 18, weight="amp"))
    assert np.array_equal(f["got"]["cnt"], dens.count.cpu().numpy())
    assert f["got"]["theta"].reshape(3, cfg().nsource, cfg().nzwn).shape == (3, 16, 4)


def test_ray_phase_modes_channels_and_frequency():
    """mode='numpy' is the reference on the delivered history; by='zwn' splits
    the same deposits into one map per wavenumber; a frequency turns into
    omega_dt = freq * tstep, negated for a backward run."""
    f = real("zonal")
    with np.errstate(all="ignore"):
        host = _wr("zonal").ray_phase(SPEC, mode="numpy")
        m = _wr("zonal").ray_phase(SPEC, by="zwn")
    for k in ("cnt", "nseg", "theta", "re", "im", "wabs"):
        assert np.array_equal(host[k], f["want"][k], equal_nan=True), k
    assert m.spec.nchan == 4 and np.array_equal(m.cnt.sum(dim=0).cpu().numpy(), f["want"]["cnt"][0])
    assert np.array_equal(m.theta.cpu().numpy(), f["got"]["theta"], equal_nan=True)
    with pytest.raises(ValueError):
        _wr("zonal").ray_phase(SPEC, by="source")
    seen = {}

    def spy(reference, Map, Sink, spec, *a, **kw):
        seen["omega_dt"] = spec.omega_dt

    for backward, freq, given, want in ((False, 2e-6, 0.0, 2e-6 * TSTEP), (True, 2e-6, 0.0, -2e-6 * TSTEP),
                                        (False, 2e-6, 0.25, 0.25), (True, 0.0, 0.0, 0.0)):
        w = _wr("zonal", backward)
        w.set_freq(freq)
        w._ray_segments = spy
        w.ray_phase(PhaseSpec(36, 18, omega_dt=given))
        assert seen["omega_dt"] == want, (backward, freq, given)


def test_derived_fields_and_output(tmp_path):
    import ncio
    f = real("nonzonal")
    m, got = f["map"], f["got"]
    cnt, hit = got["cnt"], got["cnt"] > 0
    amp = np.hypot(got["re"], got["im"])
    for name, want in (("field", got["re"]), ("amplitude", amp), ("mean_phase", np.arctan2(got["im"], got["re"])),
                       ("coherence", amp / np.where(hit, got["wabs"], 1.0))):
        a = getattr(m, name)().cpu().numpy()
        assert np.array_equal(np.isnan(a), ~hit), name
        assert np.allclose(a[hit], want[hit], rtol=1e-14, atol=0.0), name
    coh = m.coherence().cpu().numpy()[hit]
    assert coh.max() <= 1.0 + 1e-12 and coh.min() >= 0.0 and (cnt[hit] == 1).any()
    assert np.allclose(coh[cnt[hit] == 1], 1.0, rtol=1e-14)            # one deposit agrees with itself
    # (a device division by a constant may be a product with its reciprocal: one more rounding)
    assert np.allclose(m.cycles().cpu().numpy(), got["theta"] / (2 * math.pi), rtol=2.0 ** -51, atol=0.0, equal_nan=True)
    # without a weight the coherence is over cnt
    rows = np.zeros((2, 1, 8))
    rows[:, 0, 0], rows[1, 0, 2] = 0.1, 0.0
    u = PhaseMap(PhaseSpec(4, 2, weight=None, need=None), 2, DEV, theta0=[0.0, math.pi])
    start(u, rows[:, 0])
    assert u.wabs is None and abs(float(np.nanmax(u.coherence().cpu().numpy()))) < 1e-15      # two rays cancel
    for name in ("map.nc", "map.npz"):
        path = str(tmp_path / name)
        m.output(path)
        d = ncio.read(path)
        assert d["cnt"].shape == (1, 18, 36) and np.array_equal(d["cnt"], cnt)
        assert d["cnt"].dtype.kind == ("i" if name.endswith(".npz") else "f")
        for k in ("re", "im", "wabs", "theta"):
            assert np.array_equal(d[k], got[k], equal_nan=True), k
        assert np.array_equal(d["nseg"], got["nseg"]) and d["dropped"].tolist() == [float(got["dropped"])]
        assert d["lon_edges"].shape == (37,) and d["lat_edges"].tolist() == np.linspace(-90.0, 90.0, 19).tolist()


# --------------------------------------------------- sinks and directions
def test_tee_with_a_density_sink():
    """One integration into Tee(DensitySink, PhaseSink), with omega_dt != 0:
    the phase map as the reference has it, the density map as WR.ray_density's."""
    kind = "nonzonal"
    f = real(kind)
    spec = PhaseSpec(36, 18, omega_dt=0.375)
    w = _wr(kind)
    eng = w.bs.engine()
    rows0 = eng.initial_rows(w.source_lon, w.source_lat, w.zwn, w.freq)            # [7, 3, ns, nz]
    r0 = rows0.reshape(7, -1).cpu().numpy()
    y0 = rows0[:5].reshape(5, -1).contiguous()
    apart = start(PhaseMap(spec, 192, eng.device), r0.T)
    eng.integrate(y0.clone(), NT, TSTEP, ttotal=(NT - 1) * TSTEP, sink=PhaseSink(apart), chunk=37)
    dspec = DensitySpec(36, 18, weight="amp")
    dens = DensityMap(dspec, eng.device)
    eng.integrate(y0.clone(), NT, TSTEP, ttotal=(NT - 1) * TSTEP, sink=DensitySink(dens))
    m = start(PhaseMap(spec, 192, eng.device), r0.T)
    dm = DensityMap(dspec, eng.device)
    eng.integrate(y0.clone(), NT, TSTEP, ttotal=(NT - 1) * TSTEP, sink=Tee(DensitySink(dm), PhaseSink(m)))
    with np.errstate(all="ignore"):
        want = reference_phase(f["hist"], None, spec)
    assert_phase(m.numpy(), want, "tee")
    assert_same_run(numpy_with_carry(m), numpy_with_carry(apart), want, "tee against apart")
    assert np.array_equal(dm.count.cpu().numpy(), dens.count.cpu().numpy())
    assert np.allclose(dm.wsum.cpu().numpy(), dens.wsum.cpu().numpy(), rtol=1e-12, atol=0.0)
    # the same rays, the same theta: only psi turns with the row
    assert np.array_equal(m.numpy()["theta"], f["got"]["theta"], equal_nan=True)
    assert not np.array_equal(m.numpy()["re"], f["got"]["re"])


@pytest.mark.parametrize("kind", KINDS)
def test_backward_ray_phase(kind):
    """WR(backward=True).ray_phase against the reference on that history; the
    backward rays are not the forward ones."""
    f = real(kind, backward=True)
    assert_phase(f["got"], f["want"], (kind, "backward"))
    fwd = real(kind)
    assert f["want"]["nseg"].sum() > 1000 and not np.array_equal(f["want"]["cnt"], fwd["want"]["cnt"])
    dens = DensitySpec(36, 18, weight="amp")
    with np.errstate(all="ignore"):
        count = _wr(kind, True).ray_density(dens).count.cpu().numpy()
    assert np.array_equal(f["got"]["cnt"], count)


def test_ensemble_reduce_by_member():
    """EnsembleWR.reduce with a PhaseMap over a 2-member stack, by='member':
    channel m is WR.ray_phase on member m alone -- integers and theta exactly,
    the sums within the bound."""
    import synthetic as S
    from ensemble import EnsembleWR
    from levels import Levels
    bgs = [S.background(k) for k in KINDS]
    lv = Levels(bgs[0]["lat"], bgs[0]["lon"], 2)
    lv.set_levels(np.stack([b["u"] for b in bgs]), np.stack([b["v"] for b in bgs]))
    c = cfg()
    ew = EnsembleWR(lv, c.nzwn, c.nsource, TSTEP, (NT - 1) * TSTEP)
    ew.set_zwn(c.zwn)
    ew.set_source_matrix(c.SW_lon, c.SW_lat, c.dlon, c.dlat, c.nnx, c.nny)

    def make(device, chan, nray):
        m = PhaseMap(with_channels(SPEC, ew.nmember), nray, device, chan)
        m.start(ew.rlon[0], ew.rlat[0], ew.ramp[0], ew.ramp[0], k=ew.rzwn[0], l=ew.rmwn[0])
        return m, PhaseSink(m)

    with np.errstate(all="ignore"):
        got = ew.reduce(make, by="member").numpy()
    assert got["cnt"].shape == (2, 18, 36) and got["theta"].shape == (2 * 192,)
    for mem, kind in enumerate(KINDS):
        f = real(kind)
        alone, want = f["got"], f["want"]
        sel = slice(mem * 192, (mem + 1) * 192)
        assert np.array_equal(got["cnt"][mem], alone["cnt"][0]), kind
        assert np.array_equal(got["nseg"][sel], alone["nseg"]), kind
        assert np.array_equal(got["theta"][sel], alone["theta"], equal_nan=True), kind
        bound = sum_bound(want["cnt"], wabs_ref(want))[0]
        for k in ("re", "im", "wabs"):
            assert np.all(np.abs(got[k][mem] - alone[k][0]) <= bound), (kind, k)
    assert got["dropped"] == sum(real(k)["got"]["dropped"] for k in KINDS)


# ------------------------------------------------------------- allreduce
def _allreduce_body(dist, ops):
    spec = crafted_spec("7x5-amp")
    h = crafted_history(NT_CRAFTED, seed=3)
    theta0 = np.linspace(-1.0, 1.0, NRAY)
    m = start(PhaseMap(spec, NRAY, "cuda:0", h["chan"], theta0), h["rows"][:, 0])
    m.add_rows(1, NT_CRAFTED, torch.as_tensor(h["rows"][:, 1:], device="cuda:0"))
    before, prev = m.numpy(), m.prev.clone()
    m.allreduce(dist.group.WORLD)
    after = m.numpy()
    same_prev = bool(torch.equal(torch.nan_to_num(prev, nan=-7.0), torch.nan_to_num(m.prev, nan=-7.0)))
    kinds = [str(o) for o in ops]
    # WR.ray_phase with a group, through the N-rank branches on one rank
    # (shard.COLLECTIVE_MIN_WORLD = 1, as tests/test_gpu_multirank.py does)
    import shard
    with np.errstate(all="ignore"):
        alone = _wr("nonzonal").ray_phase(SPEC, by="zwn").numpy()
        shard.COLLECTIVE_MIN_WORLD = 1
        grouped = _wr("nonzonal").ray_phase(SPEC, by="zwn", group=dist.group.WORLD).numpy()
    return dist.get_backend(), kinds, same_prev, before, after, alone, grouped, len(ops) - len(kinds)


def test_allreduce_one_rank_group_leaves_the_map_unchanged():
    backend, kinds, same_prev, before, after, alone, grouped, nops_wr = one_rank(_allreduce_body)
    assert backend == "nccl" and same_prev
    # cnt re im wabs dropped nseg | theta of the owner, the owners
    assert len(kinds) == 8 and all("SUM" in k for k in kinds)
    assert before["nseg"].sum() > 200 and np.abs(before["theta"]).max() > 10.0
    for k in ("cnt", "re", "im", "wabs", "theta", "nseg"):
        assert np.array_equal(after[k], before[k], equal_nan=True), k
    assert after["dropped"] == before["dropped"]
    # the grouped drop-in: the same map as the run without a group, all-reduced
    assert alone["cnt"].shape == (4, 18, 36) and alone["nseg"].sum() > 10000
    for k in ("cnt", "theta", "nseg"):
        assert np.array_equal(grouped[k], alone[k], equal_nan=True), k
    for k in ("re", "im", "wabs"):
        assert np.allclose(grouped[k], alone[k], rtol=1e-12, atol=1e-9), k
    assert nops_wr >= 8
