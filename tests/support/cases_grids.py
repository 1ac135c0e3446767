"""The grids the ray loop is held to besides 144 x 73, their seed set, and the
conditions the reference's records on them (tests/golden/grid_<name>.npz) meet.

Each grid reaches arithmetic the 2.5-degree global cyclic state cannot:

``g1``    181 x 360  the clamped seam cell (``x0 == x1 == W-1`` at
                     ``nextafter(2 pi, 0)``), a top row that is NOT clamped,
                     1 021 cache-image tiles
``g10``   19 x 36    11 tiles, almost no cell changes, ``W*H % 64 == 63``
``g127``  33 x 127   ``W*H = 66*64``: no partial tile; odd ``nlon``, ``dlon``
                     not a round number
``nc``    73 x 144   non-cyclic (``W = nlon``): longitudes past the last column
                     read the clamped column
``q``     721 x 1440 16 234 tiles, offsets near 2^27, ~4 cell changes per row
``g30``   7 x 12     time-varying only: ``H = 7`` is below the block cache's
                     8 x 8 (5 levels of ``background_level(j, res=30)``)

This module needs neither a GPU nor the reference.
"""
import os

import numpy as np

import rwrt_oracle as O
import synthetic as S

PI = O.PI
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")

#        name: (nlat, nlon, xcyclic)
GRIDS = {"g1": (181, 360, True),
         "g10": (19, 36, True),
         "g127": (33, 127, True),
         "nc": (73, 144, False),
         "q": (721, 1440, True)}
STATIC = tuple(GRIDS)
TV_SMALL = {"g30": 30.0, "g10": 10.0}       # background_level(j, res=...)
TV_NLEV, TV_NT = 5, 13

# the seed set: 32 sources on both sides of the 0/360 seam x 3 wavenumbers x 3 roots
SEEDS = dict(SW_lon=340, SW_lat=15, dlon=5, dlat=10, nnx=8, nny=4)
ZWN = np.array([2.0, 4.0, 6.0])
FREQ, TSTEP, NT = 0.0, 7200.0, 41
NRAY = 3 * SEEDS["nnx"] * SEEDS["nny"] * len(ZWN)

# what every grid's records must contain (asserted by the generator and, on
# the committed files, by tests/test_grids_oracle.py)
MIN_LIVE0, MIN_DIED, MIN_REJECTED, MIN_SEAM = 150, 1, 100, 50
MIN_NC_CLAMPED_ROWS = 200


def axes(name):
    """``(lat, lon)`` in degrees, float32."""
    nlat, nlon, _ = GRIDS[name]
    lat = np.linspace(-90.0, 90.0, nlat).astype(np.float32)
    lon = (np.arange(nlon) * (360.0 / nlon)).astype(np.float32)
    return lat, lon


def state(name, kind="nonzonal"):
    """``dict(u, v, lat, lon)`` of a synthetic basic state on the grid's axes."""
    lat, lon = axes(name)
    return S.background_on(kind, lat, lon)


def xcyclic(name):
    return GRIDS[name][2]


def golden(name):
    return np.load(os.path.join(GOLDEN, f"grid_{name}.npz"), allow_pickle=False)


def sources():
    s = SEEDS
    return O.source_matrix(s["SW_lon"], s["SW_lat"], s["dlon"], s["dlat"], s["nnx"], s["nny"])


_BG = {}


def background(name, kind="nonzonal"):
    """The oracle's ``Background`` of the grid (built once)."""
    if (name, kind) not in _BG:
        _BG[(name, kind)] = O.Background(**state(name, kind), xcyclic=xcyclic(name))
    return _BG[(name, kind)]


def tv_levels(name):
    """The ``TV_NLEV`` levels ``dict(u, v, lat, lon)`` of a small time-varying grid."""
    return [S.background_level(j, res=TV_SMALL[name]) for j in range(TV_NLEV)]


def cell_xy(lon_axis, lat_axis, lon, lat):
    """``floor`` of the fractional cell coordinates of interpolation.py:78-82 for
    radian axes (the float32-rounded ones of ``BS``): ``(ix, iy)`` as float64,
    NaN where ``|lat| > pi/2``."""
    with np.errstate(invalid="ignore"):
        xs = (np.asarray(lon, np.float64) % (2 * PI)) % (2 * np.pi)
        fx = np.floor((xs - lon_axis[0]) / (lon_axis[1] - lon_axis[0]))
        fy = np.floor((np.asarray(lat, np.float64) - lat_axis[0]) / (lat_axis[1] - lat_axis[0]))
        out = np.abs(lat) > 0.5 * PI
    fx[out], fy[out] = np.nan, np.nan
    return fx, fy


def events(name, g):
    """What the records ``g`` of grid ``name`` contain: a dict of counts."""
    nlat, nlon, cyc = GRIDS[name]
    W, H = nlon + (1 if cyc else 0), nlat
    lon, lat = g["track"]                                # [NT, nray]: every row
    live = ~np.isnan(lon)
    live0 = ~np.isnan(g["row0"][3])
    both = live[1:] & live[:-1]
    with np.errstate(invalid="ignore"):
        turn = np.floor(lon / (2 * PI))
        seam = int((both & (turn[1:] != turn[:-1])).sum())
    died = int((live[1] & ~live[-1]).sum())
    ix, _ = cell_xy(g["lon"], g["lat"], lon, lat)
    mx, my = cell_xy(g["lon"], g["lat"], g["merc_lon"], g["merc_lat"])
    return dict(live0=int(live0.sum()), died=died,
                rejected=int(g["attempts"]) - int(g["nacc"].sum()), seam=seam,
                clamped_rows=int((live & (ix >= W - 1)).sum()),
                merc_seam_clamped=int((mx == W - 1).sum()),
                merc_seam_at_last_ulp=bool(cell_xy(g["lon"], g["lat"], np.array([np.nextafter(2 * PI, 0)]),
                                                   np.array([0.3]))[0][0] == W - 1),
                merc_top_clamped=int((my >= H - 1).sum()),
                top_reaches=bool((0.5 * PI - g["lat"][0]) / (g["lat"][1] - g["lat"][0]) >= H - 1))


def check_events(name, g):
    """The conditions the records of grid ``name`` must meet; returns the counts."""
    e = events(name, g)
    assert e["live0"] >= MIN_LIVE0, e
    assert e["died"] >= MIN_DIED, e
    assert e["rejected"] >= MIN_REJECTED, e
    assert e["seam"] >= MIN_SEAM, e
    if name == "nc":
        assert e["clamped_rows"] >= MIN_NC_CLAMPED_ROWS, e
    if name in ("g1", "q"):
        assert e["merc_seam_at_last_ulp"] and e["merc_seam_clamped"] >= 1, e
    # the top row is clamped (y0 == y1 == H-1) exactly where the axis reaches it
    assert (e["merc_top_clamped"] > 0) == e["top_reaches"], e
    return e
