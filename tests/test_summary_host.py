"""Per-ray path summaries, host side (no GPU): the NumPy definition
``summary.reference_summary`` against a plain scalar loop and on the
reference's own C1 history, the shared row update csrc/summary_rows.h in a
stand-alone program under the sanitizers (chunked, with constant tails, the
tail's closed form against row by row), and the argument checks of
``rwrt_ray_summary``."""
import ctypes
import math
import os

import numpy as np
import pytest

import _hip as H
from summary import R_EARTH, Tee, reference_summary, regions_rad
from support import hostprog
from support.bits import bitwise
from support.cases_summary import C1_BOX, FLOAT_FIELDS, REGIONS8, assert_summary, c1_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_PI = 2 * math.pi
INF, NAN = math.inf, math.nan


def random_rows(nray=40, nt=23, seed=0):
    """Rows with NaN prefixes, NaN holes, all-NaN rays, non-finite values in
    single columns, ``l == 0`` rows, repeated points and constant tails."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-3.0, 3.0, (nray, nt, 8))
    rows[..., 0] = rng.uniform(-70.0, 70.0, (nray, nt))
    rows[..., 1] = rng.uniform(-1.6, 1.6, (nray, nt))
    rows[..., 3] = rng.choice([-2.0, -0.5, 0.0, 0.5, 2.0], (nray, nt))
    for j in range(nray):
        kind = j % 8
        if kind == 1:
            rows[j, :rng.integers(1, nt)] = NAN                        # a NaN prefix
        elif kind == 2:
            a = rng.integers(1, nt - 2)
            rows[j, a:a + rng.integers(1, 4)] = NAN                    # a hole
        elif kind == 3:
            rows[j] = NAN                                              # no valid row
        elif kind == 4:
            rows[j, rng.integers(0, nt), 0] = INF                      # one invalid row: lon only
            rows[j, rng.integers(0, nt), 1] = NAN
            rows[j, rng.integers(0, nt), 4] = NAN                      # valid rows with a non-finite amp
            rows[j, rng.integers(0, nt), 4] = -INF
        elif kind == 5:
            rows[j, rng.integers(2, nt):] = rows[j, 1]                 # a constant tail (frozen ray)
        elif kind == 6:
            a = rng.integers(1, nt)
            rows[j, a:] = NAN                                          # a NaN tail
            rows[j, a - 1, 3] = NAN                                    # l is NaN on a valid row
        elif kind == 7:
            rows[j, 5:9, :2] = rows[j, 4, :2]                          # equal points, other l
    return rows


def scalar_summary(rows, regions):
    """The definition of the issue, ray by ray and row by row in Python floats."""
    boxes = [[math.pi * (float(v) / 180.0) for v in b] for b in regions]
    nray, nt = rows.shape[:2]
    out = {k: [] for k in FLOAT_FIELDS + ("path", "n_valid", "last_row", "n_turn")}
    first_row = np.full((len(boxes), nray), -1, np.int32)
    rows_inside = np.zeros((len(boxes), nray), np.int32)
    for j in range(nray):
        a = dict(lon_first=NAN, lat_first=NAN, lon_last=NAN, lat_last=NAN, l_last=NAN, lat_min=INF, lat_max=-INF,
                 amp_max=-INF, path=0.0, n_valid=0, last_row=-1, n_turn=0)
        prev = None
        for i in range(nt):
            lon, lat, l, amp = (float(rows[j, i, c]) for c in (0, 1, 3, 4))
            if not (math.isfinite(lon) and math.isfinite(lat)):
                prev = None
                continue
            if prev is not None:
                plon, plat, pl = prev
                if (pl > 0 and l < 0) or (pl < 0 and l > 0):
                    a["n_turn"] += 1
                dlon, dlat = lon - plon, lat - plat
                h = math.sin(dlat / 2.0) ** 2 + math.cos(plat) * math.cos(lat) * math.sin(dlon / 2.0) ** 2
                a["path"] += abs(2 * math.atan2(math.sqrt(h), math.sqrt(1.0 - h)))
            if a["n_valid"] == 0:
                a["lon_first"], a["lat_first"] = lon, lat
            a["n_valid"] += 1
            a["last_row"] = i
            a["lon_last"], a["lat_last"], a["l_last"] = lon, lat, l
            a["lat_min"], a["lat_max"] = min(a["lat_min"], lat), max(a["lat_max"], lat)
            if math.isfinite(amp):
                a["amp_max"] = max(a["amp_max"], abs(amp))
            lam = (lon % TWO_PI) % TWO_PI
            for r, (w, e, s, n) in enumerate(boxes):
                in_lon = (w <= lam < e) if w < e else (lam >= w or lam < e)
                if in_lon and s <= lat < n:
                    if first_row[r, j] < 0:
                        first_row[r, j] = i
                    rows_inside[r, j] += 1
            prev = (lon, lat, l)
        for k, v in a.items():
            out[k].append(v)
    out = {k: np.array(v) for k, v in out.items()}
    out["first_row"], out["rows_inside"] = first_row, rows_inside
    return out


@pytest.mark.parametrize("nreg", [0, 1, 8])
def test_reference_summary_against_the_scalar_definition(nreg):
    rows = random_rows(seed=nreg)
    regions = REGIONS8[:nreg]
    got, want = reference_summary(rows, regions), scalar_summary(rows, regions)
    assert got["first_row"].shape == (nreg, rows.shape[0]) and got["n_valid"].dtype == np.int32
    # (math.sin / cos / atan2 are this host's libm, NumPy's may be its own: path by tolerance)
    assert_summary(got, want, f"nreg {nreg}")
    assert np.array_equal(got["path_m"], got["path"] * 6.3712e6) and R_EARTH == 6.3712e6
    # what the rows were made to hold
    assert got["n_valid"][3] == 0 and got["last_row"][3] == -1 and np.isnan(got["lon_last"][3])
    assert got["lat_min"][3] == INF and got["lat_max"][3] == -INF and got["amp_max"][3] == -INF
    assert got["path"][3] == 0.0 and got["n_turn"][3] == 0
    assert 0 < got["n_valid"][1] < rows.shape[1] and got["last_row"][1] == rows.shape[1] - 1
    assert got["last_row"][6] < rows.shape[1] - 1 and np.isnan(got["l_last"][6])
    assert got["n_turn"].max() > 0
    if nreg:
        assert 0 < (got["first_row"][0] >= 0).sum() < rows.shape[0]


def test_reference_summary_small_cases_by_hand():
    """Three rows written out: a reflection, a hole that breaks the path, and
    a box across 0 degrees."""
    q = math.pi / 2
    rows = np.zeros((3, 3, 8))
    # along the equator 0 -> 90 -> 180 degrees, l changes sign once (through 0 does not count)
    rows[0, :, 0], rows[0, :, 3], rows[0, :, 4] = [0.0, q, 2 * q], [1.0, 0.0, -1.0], [1.0, -3.0, NAN]
    # the same with the middle row missing: no segment, no turn
    rows[1] = rows[0]
    rows[1, 1, :2] = NAN
    rows[1, :, 3] = [1.0, 5.0, -1.0]
    # along a meridian through -1 degree longitude: 0 -> 45 N -> 0, reflected once
    rows[2, :, 0], rows[2, :, 1], rows[2, :, 3] = -math.pi / 180, [0.0, q / 2, 0.0], [2.0, 0.5, -0.5]
    s = reference_summary(rows, [(350, 20, 20, 60), (350, 20, -10, 10)])
    assert s["n_valid"].tolist() == [3, 2, 3] and s["last_row"].tolist() == [2, 2, 2]
    assert s["n_turn"].tolist() == [0, 0, 1]
    assert np.allclose(s["path"], [math.pi, 0.0, q], rtol=1e-14, atol=0) and s["path"][1] == 0.0
    assert s["amp_max"].tolist() == [3.0, 1.0, 0.0]
    assert s["lat_max"][2] == q / 2 and s["lat_min"][2] == 0.0
    assert s["first_row"].tolist() == [[-1, -1, 1], [0, 0, 0]]
    assert s["rows_inside"].tolist() == [[0, 0, 1], [1, 1, 2]]
    assert s["lon_last"][0] == 2 * q and s["l_last"].tolist() == [-1.0, -1.0, -0.5]
    with pytest.raises(ValueError):
        reference_summary(rows, [C1_BOX] * 9)
    assert regions_rad([(0, 360, -90, 90)])[0].tolist() == [0.0, TWO_PI, -q, q]


def test_reference_summary_c1_history():
    """The reference's own 90-day C1 history (3 rays x 1 081 rows): the
    literals pin the definition to reference data."""
    s = reference_summary(c1_rows(), [C1_BOX])
    assert s["n_valid"].tolist() == [1081, 1081, 1081]
    assert s["n_turn"].tolist() == [0, 155, 111]
    assert s["path"][0] == 0.0                       # the dead root slot never moves
    assert s["first_row"].tolist() == [[-1, 97, 93]]
    assert s["rows_inside"].tolist() == [[0, 88, 93]]
    assert s["last_row"].tolist() == [1080] * 3 and s["amp_max"][0] == -INF
    assert 50.0 < s["path"][2] < s["path"][1] < 70.0   # several times round the globe in 90 days


# ------------------------------------------------ csrc/summary_rows.h on the host
def chunk_bounds(nt, nchunk):
    """``nchunk`` chunks of ``[0, nt)``; the first is row 0 alone when there is more than one."""
    if nchunk == 1:
        return [0, nt]
    return [0] + [int(v) for v in np.linspace(1, nt, nchunk).round()]


def tail_from(rows, b0, b1):
    """Per ray the start of the chunk's longest constant suffix (bit patterns:
    NaN rows repeat too) -- what a launch stores once as the ray's tail."""
    bits = np.ascontiguousarray(rows[:, b0:b1, :5]).view(np.int64)
    tf = np.full(rows.shape[0], b1 - 1)
    for i in range(b1 - 2, b0 - 1, -1):
        same = (bits[:, i - b0] == bits[:, b1 - 1 - b0]).all(axis=1) & (tf == i + 1)
        tf = np.where(same, i, tf)
    return tf


def run_host_program(exe, rows, regions, nchunk, tails=True):
    nray, nt = rows.shape[:2]
    boxes = regions_rad(regions)
    bounds = chunk_bounds(nt, nchunk)
    tfs = np.stack([tail_from(rows, a, b) if tails else np.full(nray, b) for a, b in zip(bounds[:-1], bounds[1:])], 1)
    lines = [str(len(boxes))] + [" ".join(float(v).hex() for v in b) for b in boxes]
    lines += [f"{nray} {nt} {len(bounds) - 1}", " ".join(map(str, bounds))]
    for j in range(nray):
        lines.append(" ".join(str(int(v)) for v in tfs[j]))
        lines += [" ".join(float(rows[j, i, c]).hex() for c in (0, 1, 3, 4)) for i in range(nt)]
    out = [ln.split() for ln in hostprog.run(exe, lines)]
    assert len(out) == nray
    f = np.array([[int(x, 16) for x in ln[:9]] for ln in out], np.uint64).view(np.float64)
    i = np.array([[int(x) for x in ln[9:]] for ln in out], np.int32).reshape(nray, 4 + 2 * len(boxes))
    got = {k: f[:, c] for c, k in enumerate(FLOAT_FIELDS + ("path",))}
    got.update(n_valid=i[:, 0], last_row=i[:, 1], n_turn=i[:, 2], prev_valid=i[:, 3],
               first_row=i[:, 4:4 + len(boxes)].T, rows_inside=i[:, 4 + len(boxes):].T)
    return got, tfs


def test_row_update_host_program_under_sanitizers(tmp_path):
    """csrc/summary_rows.h (what the kernel calls) in a stand-alone program
    built with ASan + UBSan and run directly: crafted rows and the C1 history,
    fed in 1, 2 and 7 chunks with each chunk's constant suffix as a tail,
    equal reference_summary -- integers equal, selections bitwise, path within
    1e-12 -- and chunking changes no bit, path included; the program itself
    checks the tail's closed form against the row-by-row update."""
    exe = hostprog.build("summary_rows", tmp_path)
    for name, rows, regions in (("crafted", random_rows(seed=5), REGIONS8), ("crafted-1", random_rows(seed=6), [C1_BOX]),
                                ("crafted-0", random_rows(seed=7), []), ("c1", c1_rows(), [C1_BOX])):
        want = reference_summary(rows, regions)
        first = None
        for nchunk in (1, 2, 7):
            got, tfs = run_host_program(exe, rows, regions, nchunk)
            assert_summary(got, want, (name, nchunk))
            valid_last = np.isfinite(rows[:, -1, 0]) & np.isfinite(rows[:, -1, 1])
            assert np.array_equal(got["prev_valid"], valid_last.astype(np.int32))
            if name.startswith("crafted"):
                assert (tfs[:, -1] < rows.shape[1] - 1).any()          # some tails are longer than one row
            first = first or got
            assert bitwise(got["path"], first["path"]), (name, nchunk)
        dense, _ = run_host_program(exe, rows, regions, 2, tails=False)
        assert bitwise(dense["path"], first["path"]), name
        if name == "c1":
            assert got["n_turn"].tolist() == [0, 155, 111] and got["path"][0] == 0.0
            assert got["first_row"].tolist() == [[-1, 97, 93]] and got["rows_inside"].tolist() == [[0, 88, 93]]


# ----------------------------------------------------------- C entry point
def _call(lib, nray=16, i0=1, i1=5, rows=64, slot=None, tfrom=None, trow=None, ray=None, ncol=16, reg=None,
          f64=64, i32=64):
    """rwrt_ray_summary with fake (never dereferenced) device pointers."""
    return lib.rwrt_ray_summary(nray, i0, i1, rows, slot, tfrom, trow, ray, ncol,
                                None if reg is None else ctypes.byref(reg), f64, i32, None)


def test_summary_argument_errors_without_a_gpu():
    """Every check happens before any HIP call and names the argument."""
    lib = H.load()
    assert ctypes.sizeof(H.SummaryRegions) == 264
    assert (H.SUMMARY_MAXREG, H.SUMMARY_NF64, H.SUMMARY_NI32) == (8, 9, 4)
    hdr = open(os.path.join(ROOT, "include", "rwrt.h")).read()
    for name, v in (("MAXREG", 8), ("NF64", 9), ("NI32", 4)):
        assert f"#define RWRT_SUMMARY_{name} {v}\n" in hdr
    assert "abi 5" in H.version()                      # an additive member: the version stays

    def reg(nreg=1, **edge):
        c = H.SummaryRegions()
        c.nreg = nreg
        for r in range(min(max(nreg, 0), 8)):
            c.box[r][0], c.box[r][1], c.box[r][2], c.box[r][3] = 0.1, 0.2, -0.5, 0.5
        for k, v in edge.items():
            c.box[0][int(k[1:])] = v
        return c

    cases = [
        (dict(f64=None), b"d_f64"), (dict(i32=None), b"d_i32"),
        (dict(reg=reg(9)), b"nreg"), (dict(reg=reg(-1)), b"nreg"),
        (dict(reg=reg(1, e0=NAN)), b"box"), (dict(reg=reg(1, e3=INF)), b"box"),
        (dict(slot=64), b"d_row_slot"),
        (dict(tfrom=64), b"d_tail_row"), (dict(trow=64), b"d_tail_from"),
        (dict(i0=5, i1=5), b"it_begin"), (dict(i0=6, i1=5), b"it_begin"), (dict(i0=-1, i1=5), b"it_begin"),
        (dict(rows=None), b"d_rows"),
        (dict(rows=72), b"16-byte"), (dict(tfrom=64, trow=72), b"16-byte"),
        (dict(nray=-1), b"nray"), (dict(nray=1 << 31), b"nray"),
        (dict(ncol=15), b"nacc_cols"), (dict(ncol=-1, ray=64), b"nacc_cols"),
    ]
    for kw, word in cases:
        assert _call(lib, **kw) == H.RWRT_ERR_ARG, kw
        assert word in lib.rwrt_last_error(), (kw, lib.rwrt_last_error())
        assert lib.rwrt_last_error().startswith(b"rwrt_ray_summary: ")
    # no rays: a no-op (no device is touched; there is none on the build host)
    assert _call(lib, nray=0, rows=None) == H.RWRT_OK
    assert _call(lib, nray=0, rows=None, reg=reg(8), ncol=0) == H.RWRT_OK


def test_tee_advertises_what_every_member_takes():
    calls = []

    class Full:
        takes_tails = takes_slots = True

        def __init__(self, tag):
            self.tag = tag

        def take(self, idx):
            return Full((self.tag, tuple(idx)))

        def __call__(self, *a, **k):
            calls.append((self.tag, a, k))

    def plain(i0, i1, view):
        calls.append(("plain", (i0, i1, view), {}))

    t = Tee(Full("a"), Full("b"))
    assert t.takes_tails and t.takes_slots
    t(1, 5, "rows", "tails", "slots")
    assert calls == [("a", (1, 5, "rows", "tails", "slots"), {}), ("b", (1, 5, "rows", "tails", "slots"), {})]
    assert [s.tag for s in t.take([3, 4]).sinks] == [("a", (3, 4)), ("b", (3, 4))]
    mixed = Tee(Full("a"), plain)
    assert not mixed.takes_tails and not mixed.takes_slots
    with pytest.raises(TypeError):
        mixed.take([3, 4])                         # (plain cannot follow a shard's ray numbering)
    del calls[:]
    mixed(1, 5, "rows")
    assert [c[0] for c in calls] == ["a", "plain"]
    with pytest.raises(ValueError):
        Tee()
