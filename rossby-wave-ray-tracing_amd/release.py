"""Rays released at N times into one evolving flow, in one launch: ``ReleaseWR``.

A time-varying run (``RayEngine.from_levels`` on a ``levels.Levels`` with
several levels) starts every ray at ray time 0, i.e. at the first level.
``ReleaseWR`` traces the same sources and wavenumbers once per release time --
every day of a season, or the start, middle and end of a regime transition --
as ONE ray run (``RayEngine.integrate(release=)``, the ``rwrt_rk45_*_rel``
entry points): every ray carries its own level origin ``levels.t0 - release``,
its time still starts at 0, and release ``i`` ends exactly as a separate
time-varying run on the same levels with ``t0 = levels.t0 - releases[i]``
would, bit for bit.

Ray slot of (release, root, source, zwn): ``((i*3 + root)*nsource + s)*nzwn + iz``
-- the history arrays ``rlon .. rvg`` are ``[nt, nrelease, 3, nsource, nzwn]``.
Row ``k`` of a ray is its state ``k * tstep`` AFTER ITS RELEASE: the row axis
is lead time, not calendar time, in the histories and in every product reduced
from them -- an ``arrival.ArrivalMap`` over a release stack maps the lead time
after release at which a cell is first reached.

Row 0 of release ``r`` holds the roots of the dispersion relation on the state
valid at ``r`` (``Levels.state_at``: the two bracketing levels blended as
packed records, the level's own record at a level time).  Between two levels
row 0's ``ug, vg`` come from that blended state, while the run's RHS blends the
two levels after the bilinear lookup in each: the two agree to rounding, not
bit for bit.

The reference's two global outcomes are decided per release
(``ensemble.member_outcomes`` with the release index): a failed release's rays
are frozen before the first launch, and ``ray_run`` NaNs the rows from
``break_row[i]`` on for that release only.
"""
import numpy as np

from constants import day, hour
from ensemble import EnsembleWR, member_outcomes   # noqa: F401  (member_outcomes: per release here)
from levels import level_origin, time_index        # noqa: F401  (re-exported: the release -> t0 conversion)


def reference_state_at(packed, r, dt, t0=0.0):
    """NumPy definition of ``Levels.state_at``: the packed state valid ``r``
    seconds after the first of the levels ``packed[nlev, ncol, nrow, 12]``
    (fp64, ``dt`` apart).  ``s, j, w`` are the kernels' at ray time 0 of a ray
    whose level origin is ``t0 - r`` (``levels.time_index``); the result is
    ``packed[j] * (1 - w) + packed[j + 1] * w`` as three array operations, and
    ``packed[j]`` / ``packed[j + 1]`` themselves (no copy) for ``w == 0`` /
    ``w == 1``.  One level is blended with itself, as the kernels do."""
    packed = np.asarray(packed)
    nlev = packed.shape[0]
    j, w = time_index(0.0, level_origin(t0, r), dt, nlev)
    up = j + 1 if nlev > 1 else j
    if w == 0.0:
        return packed[j]
    if w == 1.0:
        return packed[up]
    a = packed[j] * (1.0 - w)
    b = packed[up] * w
    return a + b


class ReleaseWR(EnsembleWR):
    """``WR`` over release times into one time-varying ``levels.Levels`` (fp64,
    levels at ``levels.t0 + j * levels.dt``): one launch for all releases.
    ``releases``: seconds after the first level, one per release.  Same source
    and wavenumber setters as ``WR``; the leading axis of every array is the
    release, and rows count steps since release (lead time)."""

    axis = "release"

    def __init__(self, levels, releases, nzwn, nsource, tstep=1. * hour, ttotal=20. * day, freq=0, rtol=1e-6,
                 atol=1e-6, cut_off=0.1, MinStepFactor=1e-3, chunk_rows=None):
        rel = np.asarray(releases, dtype=np.float64).reshape(-1)
        if rel.size < 1:
            raise ValueError("a release stack needs at least one release time")
        if not np.isfinite(rel).all():
            raise ValueError("release times must be finite (seconds after the first level)")
        if getattr(levels, "fp32", False):
            raise NotImplementedError("release stacks need fp64 level storage")
        super().__init__(levels, nzwn, nsource, tstep, ttotal, freq, rtol, atol, cut_off, MinStepFactor, chunk_rows)
        self.releases = rel
        self.nrelease = self.nmember = int(rel.size)   # (the leading axis EnsembleWR's code runs over)

    def engine(self):
        """The time-varying ``RayEngine`` of the levels (built on first use; one
        level goes through the time-varying kernels too)."""
        if self._engine is None:
            from engine import RayEngine
            self._engine = RayEngine.from_levels(self.levels, time_varying=True)
        return self._engine

    def _initial_rows(self):
        """Row 0 of every release ``[nrelease, 7, 3, nsource, nzwn]``: per distinct
        release time ``Levels.state_at`` and one ``rwrt_ray_initial`` call on it."""
        import torch
        eng = self.engine()
        src = eng.sources(self.source_lon, self.source_lat)
        zc = eng.zwn_tensor(self.zwn, self.freq)
        rows, infos = {}, []
        for r in map(float, self.releases):
            if r not in rows:
                rows[r], info = eng.initial_rows_dev(src, zc, packed=self.levels.state_at(r).contiguous())
                infos.append(info)
        eng.check_initial(torch.stack(infos).sum())
        return torch.stack([rows[r] for r in map(float, self.releases)]).cpu().numpy()

    def _init(self, eng, y0, p):
        import torch
        index = torch.as_tensor(self.members())
        st = eng.init(torch.as_tensor(y0), p, release=self.releases[index.numpy()])
        return st, index.to(eng.device)

    def reduce(self, make, by="release"):
        """As ``EnsembleWR.reduce``; ``by``: None, 'zwn', 'root' or 'release'.
        The rows a product sees are steps since each ray's release."""
        return super().reduce(make, by)

    def _output_extra(self):
        """``output`` gains ``release_time`` (seconds after the first level) on the
        ``release`` dimension; ``time`` counts steps since release."""
        return {"release_time": (("release",), self.releases, "s")}
