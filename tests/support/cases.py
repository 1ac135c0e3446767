"""Basic states, engines and reference runs that the GPU tests of several
products share; each is built once per process."""
import numpy as np
import torch

import rwrt_oracle as O
import synthetic as S
from conftest import golden
from density import DensitySpec, reference_bins

NAN = np.nan
NT_C2 = 121          # 10 days
DT = 6 * 3600.0      # between the levels of a time-varying background


_ENG = {}


def bs_of(kind):
    from bs import BS
    bg = S.background(kind)
    bs = BS(len(bg["lon"]), len(bg["lat"]))
    bs.load_arrays(**bg)
    bs.ready(xcyclic=True)
    return bs


def engine(kind):
    if kind not in _ENG:
        from engine import RayEngine
        _ENG[kind] = RayEngine.from_bs(bs_of(kind))
    return _ENG[kind]


def run_c2(kind, nt, chunk=None, order=None, eng=None, **kw):
    from engine import t_eval_of
    g = golden(f"init_C2_{kind}.npz")
    eng = eng or engine(kind)
    y0 = torch.as_tensor(g["rows"][:5].reshape(5, -1))
    rows = {}

    def sink(i0, i1, out):
        rows[(i0, i1)] = out.cpu().numpy().copy()

    res = eng.integrate(y0, nt, 7200.0, ttotal=(nt - 1) * 7200.0, chunk=chunk, sink=sink, **kw)
    nray = y0.shape[1]
    hist = np.full((nray, nt, 8), np.nan)
    hist[:, 0, :7] = g["rows"].reshape(7, -1).T
    for (i0, i1), r in rows.items():
        hist[:, i0:i1] = r
    return hist, res


def run_wr(kind, cfg_name, nt, inte_method):
    from wr import WR
    cfg = S.config(cfg_name)
    bs = bs_of(kind)
    w = WR(cfg.nzwn, cfg.nsource, 7200.0, (nt - 1) * 7200.0, cfg.freq, nx=bs.nlon, ny=bs.nlat)
    w.bs = bs
    w.set_zwn(cfg.zwn)
    w.set_source_matrix(cfg.SW_lon, cfg.SW_lat, cfg.dlon, cfg.dlat, cfg.nnx, cfg.nny)
    with np.errstate(all="ignore"):
        w.ray_run(mode="hip", inte_method=inte_method)
    return np.array([w.rlon, w.rlat, w.rzwn, w.rmwn, w.ramp, w.rug, w.rvg]).reshape(7, nt, -1)


C2_SPEC = DensitySpec(360, 180, nchan=4, weight="amp")
_C2 = {}


def c2_chan():
    return (np.arange(3 * 256 * 4) % 4).astype(np.int32)      # slot (root, source, zwn) -> zwn


def c2_ref(method="rk45"):
    """Dense rows of the 10-day C2 zonal run collected by a plain sink, and
    their reference map (computed once)."""
    if method not in _C2:
        if method == "rk45":
            hist, _ = run_c2("zonal", NT_C2)
        else:
            g = golden("init_C2_zonal.npz")
            got = {}
            engine("zonal").integrate_rk4(torch.as_tensor(g["rows"][:5].reshape(5, -1)), NT_C2, 7200.0,
                                          sink=lambda a, b, o: got.__setitem__(a, o.cpu().numpy().copy()))
            hist = np.concatenate([np.full((3072, 1, 8), np.nan)] + [got[k] for k in sorted(got)], axis=1)
        pts = hist[:, 1:]
        ref = reference_bins(pts[..., 0], pts[..., 1], pts[..., 4], c2_chan()[:, None], C2_SPEC)
        _C2[method] = (pts, ref)
    return _C2[method]


def c1_wr():
    from wr import WR
    cfg = S.config("C1")
    bs = bs_of("zonal")
    wr = WR(cfg.nzwn, cfg.nsource, 7200.0, 90 * 86400.0, 0.0, nx=bs.nlon, ny=bs.nlat)
    wr.bs = bs
    wr.set_zwn(cfg.zwn)
    wr.set_source_matrix(cfg.SW_lon, cfg.SW_lat, cfg.dlon, cfg.dlat, cfg.nnx, cfg.nny)
    return wr


_TV = {}


def tv_engine(fp32, nlev=5):
    if fp32 not in _TV:
        from engine import RayEngine
        from levels import Levels
        bl = [S.background_level(j) for j in range(nlev)]
        lv = Levels(bl[0]["lat"], bl[0]["lon"], nlev, t0=0.0, dt=6 * 3600.0, fp32=fp32)
        for j, b in enumerate(bl):
            lv.set_level(j, b["u"], b["v"])
        _TV[fp32] = RayEngine.from_levels(lv)
    return _TV[fp32]


def c2_wr(nt=61):
    from wr import WR
    cfg = S.config("C2")
    bs = bs_of("nonzonal")
    w = WR(cfg.nzwn, cfg.nsource, 7200.0, (nt - 1) * 7200.0, cfg.freq, nx=bs.nlon, ny=bs.nlat, chunk_rows=20)
    w.bs = bs
    w.set_zwn(cfg.zwn)
    w.set_source_matrix(cfg.SW_lon, cfg.SW_lat, cfg.dlon, cfg.dlat, cfg.nnx, cfg.nny)
    return w


_C2_HIST = {}


def c2_y0(kind):
    g = golden(f"init_C2_{kind}.npz")
    return g["rows"].reshape(7, -1), torch.as_tensor(g["rows"][:5].reshape(5, -1))


def c2_hist(kind, method="rk45"):
    """The logical history ``[3072, 121, 8]`` of the 10-day C2 run as a plain
    sink receives it (dense rows), computed once."""
    if (kind, method) not in _C2_HIST:
        if method == "rk45":
            hist, _ = run_c2(kind, NT_C2)
        else:
            row0, y0 = c2_y0(kind)
            got = {}
            engine(kind).integrate_rk4(y0, NT_C2, 7200.0,
                                       sink=lambda a, b, o: got.__setitem__(a, o.cpu().numpy().copy()))
            hist = np.full((3072, NT_C2, 8), NAN)
            hist[:, 0, :7] = row0.T
            hist[:, 1:] = np.concatenate([got[k] for k in sorted(got)], axis=1)
        hist.setflags(write=False)
        _C2_HIST[(kind, method)] = hist
    return _C2_HIST[(kind, method)]


def c3_sample_y0(eng, n_dead=2048):
    from bench import c3_sources
    src, zcs = c3_sources(eng)
    y0 = torch.cat([eng.initial_rows_dev(src, zc)[0][:5].reshape(5, -1) for zc in zcs], dim=1)
    g = golden("c3_sample.npz")
    dead = torch.nonzero(torch.isnan(y0.sum(0))).squeeze(1)[:: 397][:n_dead]
    sel = torch.cat([torch.as_tensor(g["idx"], device=eng.device), dead])
    return y0[:, sel].contiguous()


_TV_ORACLE = {}


def tv(fp32, nlev=5):
    key = (fp32, nlev)
    if key not in _TV_ORACLE:
        from engine import RayEngine
        from levels import Levels
        bl = [S.background_level(j) for j in range(nlev)]
        lv = Levels(bl[0]["lat"], bl[0]["lon"], nlev, t0=0.0, dt=DT, fp32=fp32)
        for j, b in enumerate(bl):
            lv.set_level(j, b["u"], b["v"])
        ob = O.TimeVaryingBackground([O.Background(**b) for b in bl], 0.0, DT, fp32=fp32)
        _TV_ORACLE[key] = (RayEngine.from_levels(lv), ob, O.Background(**bl[0]))
    return _TV_ORACLE[key]
