/*
 * rwrt.h -- C ABI of the MI355X batched Rossby-wave ray integrator.
 *
 * The reference (yinan-codes/Rossby-wave-ray-tracing) has no FFI: its ray loop
 * is selected by Python method dispatch, WR.ray_run -> WR.core_ray_run
 * ('numpy_rk45') -> WR.core_ray_run_rk45 (wr.py:889-911, 767-887).  The
 * entry points below are what that dispatch binds instead (ctypes, see
 * INTEGRATION.md); each cites the reference function it replaces.
 *
 * Conventions
 *  - Every pointer named d_* is DEVICE memory owned by the caller (the Python
 *    host keeps it in PyTorch-ROCm tensors).  The library never allocates or
 *    frees caller memory.
 *  - All calls are asynchronous and ordered on `stream` (a hipStream_t; NULL =
 *    the default stream).  Status codes report argument and launch errors;
 *    per-ray failure is data (NaN), exactly as in the reference.
 *  - fp64 throughout; the fields are the reference's 18-field stack.
 *  - The ray-loop entry points (rwrt_rk45_run, rwrt_rk45_run_tv, rwrt_rk4_run)
 *    take an execution context, rwrt_ctx, that owns the library's own scratch
 *    (a per-ray frozen flag, a side stream and its events).  Nothing else in
 *    the library holds state between calls: calls through DISTINCT contexts
 *    are reentrant and may run concurrently on different streams or threads.
 *    One context may be shared by threads (its calls are serialised on the
 *    host) and used on several streams (a call waits on the device for the
 *    context's previous call before reusing its scratch).
 */
#ifndef RWRT_H
#define RWRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RWRT_ABI_VERSION 5  /* 3: constant row tails (rwrt_rk45_run_tails, rwrt_expand_tails);
                               4: row blocks for the live rays only (rwrt_rk45_run_slots);
                               5: ray-density maps binned on the device (rwrt_ray_density);
                                  per-ray path summaries (rwrt_ray_summary) and the wavenumber
                                  map (rwrt_wn_map, rwrt_wn_fill) joined ABI 5 later as additive
                                  members, and so did the spherical-harmonic filter
                                  (rwrt_sh_filter), the arrival-time maps
                                  (rwrt_ray_arrival), the basic-state diagnostics
                                  (rwrt_bs_diag), the wave-ray flux maps
                                  (rwrt_ray_flux), the residence-time maps along ray
                                  segments (rwrt_ray_track), the gate-crossing maps
                                  (rwrt_ray_cross), the WKB phase along rays with its
                                  wave-field maps (rwrt_ray_phase), the ray-tube maps
                                  (rwrt_ray_tube), the Helmholtz decomposition with
                                  the Rossby-wave source (rwrt_sh_helmholtz,
                                  rwrt_sh_rws) and the caustic-aware wave-field maps
                                  (rwrt_ray_wave): no earlier signature or layout changed */
#define RWRT_NFIELD_REF 18  /* BS.fields[..., 18]            (bs.py:349-368) */
#define RWRT_NFIELD_PACK 12 /* 11 hot fields + 1 pad per grid point           */
#define RWRT_NVAR 5         /* y = (lon, lat, k, l, amp)     (wr.py:768-776)  */
#define RWRT_NMERC 12       /* fmu .. fmqyy                  (bs.py:885-887)  */
#define RWRT_NOUT 8         /* per output row: lon lat k l amp ug vg nacc     */
#define RWRT_NSTATE 12      /* per ray: y[5] f[5] t h_abs                     */

typedef enum {
  RWRT_OK = 0,
  RWRT_ERR_ARG = 1,        /* bad argument (message in rwrt_last_error)     */
  RWRT_ERR_HIP = 2,        /* HIP launch / runtime error                     */
  RWRT_SOLVER_FAILED = 3   /* rkf45.py:423-425 "All nan" (set by the host)   */
} rwrt_status;

/* Grid of BS.fields: W = nlon (+1 cyclic pad column, bs.py:370-372) columns,
 * H = nlat rows.  lon0/dlon, lat0/dlat are bs.lon[0], bs.lon[1]-bs.lon[0],
 * bs.lat[0], bs.lat[1]-bs.lat[0] of the float32-rounded grid
 * (bs.py:225-236, interpolation.py:78-82). */
typedef struct {
  int32_t ncol;
  int32_t nrow;
  double lon0, dlon;
  double lat0, dlat;
} rwrt_grid;

/* Solver parameters of WR.core_ray_run_rk45 / RK45 (wr.py:792-794). */
typedef struct {
  double rtol;      /* max(rtol, 100 eps)          rkf45.py:21-26  */
  double atol;
  double min_step;  /* Global_Minstep              rkf45.py:362    */
  double cut_off;   /* jump mask threshold, rad    wr.py:170       */
  int32_t nt;       /* rows of the history         wr.py:157       */
  int32_t flags;    /* RWRT_PARAMS_*; 0: the reference's forward loop */
  double tstep;     /* output interval = RK4 step  wr.py:147       */
} rwrt_params;      /* 48 bytes */

/* rwrt_params.flags (the former `reserved` word: same offset, same size).
 *
 * RWRT_PARAMS_BACKWARD: backward ray tracing -- the reference's DP5(4) loop
 * (WR.core_ray_run_rk45 over RK45) with direction = -1 (rkf45.py:207,
 * 426-429).  Output row i is the ray's state at time -d_tbound[i]: d_tbound
 * stays the non-negative elapsed times, the loop steps to their negatives.
 * Everything else is the forward loop's: the step control (h_abs, the
 * min_step clamp -- min_step is positive --, the accept and reject factors),
 * the pole and jump masks against the previous row, ug and vg of a row as the
 * true group velocity there (not negated), the nacc column, frozen rays
 * repeating their row, and the three row layouts (dense, tails, slots), the
 * queue order, n_heavy and time chunking.  The RHS is autonomous and IEEE
 * negation is exact, so the rows equal the forward integration of -f bit for
 * bit.
 * Honoured by rwrt_rk45_init (h_abs depends on the direction through
 * select_initial_step's trial point y0 + h0 * direction * f0) and by
 * rwrt_rk45_run, rwrt_rk45_run_tails and rwrt_rk45_run_slots; init and every
 * run call of one integration carry the same flag.  Between calls d_state
 * holds, besides y and h_abs, f = the RHS at y (not negated) and t = minus
 * the elapsed time (the last row's -d_tbound; a ray frozen at a call's start
 * gets the positive value from the fill kernels: its t is never read again).
 * The diagnostic trace (rwrt_ctx_set_trace) is not recorded by backward calls.
 * Every other entry with an rwrt_params argument -- rwrt_rk4_run, the _tv
 * entries, the _stack entries -- returns RWRT_ERR_ARG before any HIP call when the flag
 * is set, and every entry returns RWRT_ERR_ARG for any other non-zero bit;
 * the message starts with the entry point's name.  (rwrt_kat_rk45 takes no
 * rwrt_params: it has no way to be asked for a backward run.) */
#define RWRT_PARAMS_BACKWARD 1

/* A time-varying basic state (this framework's extension for BASELINE
 * configs[4]; the reference's fun ignores t, wr.py:784-789): nlev packed
 * levels [nlev][ncol][nrow][12] (fp64, or fp32 when fp32 != 0; fp32 == 2
 * also computes the RHS in fp32 -- not the reference's arithmetic) valid at
 * t0 + j*dt seconds of ray time.  The RHS interpolates each level bilinearly
 * exactly like the static state and then linearly in time:
 * s = (t - t0)/dt, j = clip(floor(s), 0, nlev-2), w = clip(s - j, 0, 1),
 * field = f_j (1 - w) + f_{j+1} w. */
typedef struct {
  const void* d_levels;
  int32_t nlev;
  int32_t fp32;
  double t0;
  double dt;
} rwrt_background;
const char* rwrt_version(void);

/* Execution context of the ray-loop entry points: created
 * for one HIP device, destroyed when no call through it is pending (destroy
 * waits for the last call's kernels before freeing its scratch). */
typedef struct rwrt_ctx rwrt_ctx;
rwrt_status rwrt_ctx_create(int32_t device, rwrt_ctx** out);
rwrt_status rwrt_ctx_destroy(rwrt_ctx* ctx);
/* Rays per wavefront in the latency mode of rwrt_rk45_run (n_heavy > 0) on
 * this context: 1..16 (default 16 = 64 rays per CU).  Fewer rays per wave
 * make each heavy ray's attempts faster (its wave stalls less often on the
 * other rays' cell refills and interval ends) at more CUs per heavy ray.
 * Schedule only: results do not depend on it. */
rwrt_status rwrt_ctx_set_latency_density(rwrt_ctx* ctx, int32_t rays_per_wave);
/* Rays per wavefront of this context's fp64 time-varying ray loops
 * (rwrt_rk45_run_tv*, levels with fp32 == 0): 64 (default; the lower
 * bracketing level cached per lane in LDS, the upper one gathered) or 32
 * (lane pairs: lanes L and L + 32 run the same ray, each caching and blending
 * one bracketing level, exchanged by v_permlane32_swap -- no HBM gathers
 * while a ray stays in its cell and level pair, half the LDS-DMA per refill;
 * RayEngine's default, C5 fp64 1.21 -> 1.61e9 with the other round-5 changes).
 * Schedule only: results do not depend on it (ABI 3).  The release-stack
 * entry (rwrt_rk45_run_rel, below) honours it too; it reads the setting itself
 * when it launches, where the time-varying entries read it before. */
rwrt_status rwrt_ctx_set_tv_lanes(rwrt_ctx* ctx, int32_t lanes);
/* The work-queue grid of this context's last DP5(4) ray-loop launch (additive
 * within ABI 5; diagnostic): the persistent blocks that pulled rays from the
 * queue (0 before any launch, and for a launch whose rays all ran in latency
 * mode) and the rays a block holds at once (256; 128 at 32 rays per wave), so
 * blocks * rays_per_block rays are in flight and any further live ray is a
 * lane's second.  Host bookkeeping only: no HIP call. */
rwrt_status rwrt_ctx_last_grid(rwrt_ctx* ctx, int32_t* blocks, int32_t* rays_per_block);
/* Drain-time hand-off of this context's static-state ray loops (ABI 4): once
 * a call's work queue is drained, a wavefront with at most max_rays rays left
 * (0 = off, at most 16; default 16) continues them four lanes per ray, in the
 * latency mode's layout, from exactly where they stopped (between two
 * attempts).  Schedule only: results do not depend on it.  A call's d_work[0]
 * counts the rays it handed off (diagnostic). */
rwrt_status rwrt_ctx_set_handoff(rwrt_ctx* ctx, int32_t max_rays);
/* Diagnostic ray trace of the context's rwrt_rk45_run calls (NULL / 0: off):
 * for queue positions w < capacity of the order, the ray's lane records
 * d_trace[w * 10 + 0..9] = {ray, hardware id (HW_REG_HW_ID: wave, SIMD, CU,
 * SE fields), XCC id, start and end of the ray's integration in the launch
 * (s_memrealtime, 100 MHz), attempts made, 1 if in latency mode else 0,
 * block index, start and end in shader clocks (s_memtime)} -- where, how long
 * and at what clock the heaviest rays run (the makespan of a launch is
 * theirs).  Costs one compare per ray when off. */
rwrt_status rwrt_ctx_set_trace(rwrt_ctx* ctx, int64_t* d_trace, int64_t capacity);
/* Last error message of the calling thread ("" if none). */
const char* rwrt_last_error(void);

/* Device layout of BS.fields (bs.py:349-372): d_fields is the reference stack
 * [ncol][nrow][18] fp64; d_packed receives [ncol][nrow][12] (the 11 fields the
 * hot path reads -- u v ux uy vx vy qx qy qxx qxy qyy -- plus a zero pad). */
rwrt_status rwrt_pack_fields(const rwrt_grid* g, const double* d_fields,
                             double* d_packed, void* stream);

/* BS.cal_bs_mercator_point(lon, lat, mode='numpy') (bs.py:513-519,781-887):
 * d_out[12][n] = fmu fmv fmux fmuy fmvx fmvy fmqx fmqy fmqxx fmqxy fmqyx fmqyy. */
rwrt_status rwrt_mercator_point(const rwrt_grid* g, const double* d_packed,
                                int64_t n, const double* d_lon,
                                const double* d_lat, double* d_out,
                                void* stream);

/* WR.diffun_numpy(y)[0][0:5] (wr.py:492-556 with core_diffun wr.py:44-82 and
 * cal_ugvg 'extent' wn.py:266-294): d_y[5][n] -> d_dydt[5][n]. */
rwrt_status rwrt_rhs(const rwrt_grid* g, const double* d_packed, int64_t n,
                     const double* d_y, double* d_dydt, void* stream);

/* One Dormand-Prince 5(4) attempt: rk_step (rkf45.py:259-321) followed by
 * _estimate_error_norm (rkf45.py:368-373, scale rkf45.py:442-445).
 * d_y, d_f: [5][n]; d_h: [n] (signed step).  Outputs d_K[7][5][n],
 * d_ynew[5][n], d_err[n] (NaN kept, as the reference returns it). */
rwrt_status rwrt_dp54_attempt(const rwrt_grid* g, const double* d_packed,
                              int64_t n, const double* d_y, const double* d_f,
                              const double* d_h, double rtol, double atol,
                              double* d_K, double* d_ynew, double* d_err,
                              void* stream);

/* Initial rays WR.ray_initial_numpy (wr.py:344-395) on the device, per
 * (source, zonal wavenumber): the Mercator point at the source
 * (cal_bs_mercator_point, bs.py:781-887), the meridional wavenumbers of the
 * t = 0 dispersion relation (cal_ky_numpy, bs.py:985-1040 -- np.roots
 * restated operation for operation: companion matrix, LAPACK zgeev's
 * zgebal + zlahqr, csrc/nproots.h), change_roots_order (bs.py:942-982) and
 * the t = 0 group velocity (cal_ugvg_numpy, wn.py:209-259).
 *  d_src_lon, d_src_lat, d_src_cos [nsource]: source position (radians, as
 *    set_source_matrix makes it, wr.py:236-258) and np.cos(lat) from the
 *    host libm -- the one transcendental of this path, so that it is the
 *    reference's own value.
 *  d_zwn[4][nzwn] = {k, k**2, k**3, freq / k * R} as NumPy evaluates them
 *    (bs.py:1005-1012).
 *  d_rows[7][3][nsource][nzwn] = lon lat k l amp ug vg (wr.py:160-167
 *    layout of row 0; NaN where a slot has no real root).
 *  d_info[1] (int32, zeroed by this call) counts polynomials with
 *    non-finite coefficients -- np.linalg.eigvals raises LinAlgError there;
 *    the host raises too when it is non-zero. */
rwrt_status rwrt_ray_initial(const rwrt_grid* g, const double* d_packed,
                             int64_t nsource, const double* d_src_lon,
                             const double* d_src_lat, const double* d_src_cos,
                             int32_t nzwn, const double* d_zwn, double* d_rows,
                             int32_t* d_info, void* stream);

/* The wavenumber map (ABI 5, additive): the reference's WN (wn.py) on every
 * grid node of nlev packed fp64 levels and for every zonal wavenumber -- the
 * meridional wavenumbers the t = 0 dispersion relation admits, how many there
 * are, and their group velocities.
 *  d_packed [nlev][g->ncol][g->nrow][12] fp64; level_stride, in doubles, is
 *    the distance between two levels (ignored when nlev == 1).
 *  nlon <= g->ncol map columns (the cyclic pad column is no map column);
 *    d_lon[nlon], d_lat[g->nrow]: the BS radian axes themselves (bs.lon,
 *    bs.lat: float32-rounded, not lon0 + i*dlon); d_cos[g->nrow] = np.cos of
 *    d_lat from the host libm; d_zwn[4][nzwn] as for the initial rays.
 *  d_mwn, d_ug, d_vg [nlev][nlon][nrow][nzwn][3], d_rootnum
 *    [nlev][nlon][nrow][nzwn] (int32).
 * The entry (lev, i, j, iz, slot) is, bit for bit, what the initial-ray call
 * above writes on level lev for a source at (d_lon[i], d_lat[j]): d_rows[3],
 * [5], [6] at [slot][s][iz] -- the same device functions (csrc/ray_point.h)
 * serve both, the field lookup included (the bilinear lookup at the node, not
 * a read of the node's record).  rootnum counts the non-NaN slots of mwn (after the |m| > 100
 * filter); ug, vg are NaN where a slot has no root; k == 0 gives rootnum 0 and
 * ug = vg = 0.  d_info[1] (int32, zeroed by this call) counts polynomials with
 * non-finite coefficients or a failed solve; rootnum is -1 and the nine values
 * are NaN there (the pole rows of a lat-lon grid), and nothing raises.
 * One thread per (level, node, k).  Asynchronous and ordered on `stream`;
 * needs no rwrt_ctx. */
rwrt_status rwrt_wn_map(const rwrt_grid* g, const double* d_packed, int32_t nlev,
                        int64_t level_stride, int32_t nlon, const double* d_lon,
                        const double* d_lat, const double* d_cos, int32_t nzwn,
                        const double* d_zwn, double* d_mwn, double* d_ug,
                        double* d_vg, int32_t* d_rootnum, int32_t* d_info,
                        void* stream);

/* NaN fill of one level of a map (the reference WN's postprocess, defined in
 * csrc/wn_fill.h): d_in, d_out [nlon][nlat][nplane], nplane = nzwn * 3.  A
 * non-NaN entry is copied; a NaN entry becomes the mean of the non-NaN ones
 * among its eight neighbours in the same plane of d_in (i +- 1 wraps when
 * cyclic, is skipped at the edge otherwise; j +- 1 is skipped at the edge;
 * summed with di = -1, 0, 1 outer, dj = -1, 0, 1 inner; infinities count), and
 * stays NaN when there is none.  d_out == d_in is an argument error. */
rwrt_status rwrt_wn_fill(int32_t nlon, int32_t nlat, int32_t nplane, int32_t cyclic,
                         const double* d_in, double* d_out, void* stream);

/* Triangular spherical-harmonic truncation of a batch of fields (the
 * reference's SHSF.py, NCL's shaec -> tri_trunc -> shsec; the definition is
 * shsf.reference_filter, the weights and Legendre recurrence are
 * csrc/shsf_legendre.h).  Grid: nlat odd, latitudes equally spaced from -pi/2
 * to +pi/2 with both poles, ascending; nlon even, longitudes 2 pi i / nlon.
 *  d_in [nfield][nlat][nlon] float32, file layout.
 *  d_w [nlat]: the Clenshaw-Curtis weights in x = sin(lat) (they sum to 2).
 *  d_x [2][nlat]: sin(lat), then cos(lat) (exactly 0 at the poles), from the host.
 *  d_spec [nfield][trunc+1][trunc+1][2]: the coefficients a_lm (re, im) at
 *    [l][m], a_lm = sum_j w_j p_lm(x_j) F_m(j) with F_m the unnormalised
 *    longitude DFT and int p_lm^2 dx = 1; zero for l < m and for orders above
 *    min(trunc, nlon/2 - 1).  Always written.
 *  d_out32, d_out64 [nfield][nlat][nlon] or NULL: the field rebuilt from the
 *    degrees l <= trunc, fp64 and/or that value rounded to float32; both NULL:
 *    coefficients only.
 *  d_scratch: 2*nfield*(trunc+1)*nlat*2 doubles.
 * RWRT_ERR_ARG: nlat even or < 3, nlon odd, trunc < 0 or > (nlat-1)/2,
 * nfield < 0 (or > 65535), any two of d_in, d_out32, d_out64 overlapping, a
 * NULL buffer, or a row (nlon) or an order (trunc) too large for LDS.
 * nfield == 0 is a no-op.  Every sum has a fixed order (no atomics): a call's
 * output is bit-identical from call to call, and a field's result does not
 * depend on the batch it is in.  Four kernels, asynchronous and ordered on
 * `stream`; needs no rwrt_ctx. */
rwrt_status rwrt_sh_filter(int32_t nlon, int32_t nlat, int32_t nfield, int32_t trunc,
                           const float* d_in, const double* d_w, const double* d_x,
                           double* d_spec, float* d_out32, double* d_out64,
                           double* d_scratch, void* stream);

/* Helmholtz decomposition of a batch of winds (u, v) on the filter's grid (the
 * grid, d_w and d_x of rwrt_sh_filter): vorticity and divergence, the
 * streamfunction and the velocity potential, the rotational and the divergent
 * wind and the vorticity gradient, all truncated triangularly at `trunc`.
 * The definition is helmholtz.reference_helmholtz; the vector basis
 * (b_lm = m p_lm / cos(lat) and d_lm = dp_lm/dlat, finite at the pole nodes) is
 * csrc/sh_vector.h.  The planes of a call are a mask of the bits below; they
 * are written in bit order.  vrt_x = (1 / (a cos(lat))) d vrt / d lon,
 * vrt_y = (1 / a) d vrt / d lat, a = 6.3712e6 m. */
#define RWRT_SHV_VRT   0x001u  /* relative vorticity                     */
#define RWRT_SHV_DIV   0x002u  /* divergence                             */
#define RWRT_SHV_PSI   0x004u  /* streamfunction                         */
#define RWRT_SHV_CHI   0x008u  /* velocity potential                     */
#define RWRT_SHV_UROT  0x010u  /* rotational wind, zonal component       */
#define RWRT_SHV_VROT  0x020u  /*                  meridional component  */
#define RWRT_SHV_UDIV  0x040u  /* divergent wind, zonal component        */
#define RWRT_SHV_VDIV  0x080u  /*                 meridional component   */
#define RWRT_SHV_VRTX  0x100u  /* vorticity gradient, zonal component    */
#define RWRT_SHV_VRTY  0x200u  /*                     meridional component */
#define RWRT_SHV_NPLANE 10
/*  d_u, d_v [npair][nlat][nlon] float32, file layout, latitude ascending.
 *  d_spec [npair][2][trunc+1][trunc+1][2]: vrt_lm, then div_lm (re, im) at
 *    [l][m]; zero for l < m, for l = 0 and for orders above
 *    min(trunc, nlon/2 - 1).  Always written.
 *  d_out64 [npair][popcount(planes)][nlat][nlon]: the planes, in bit order.
 *  d_rot32 [npair][2][nlat][nlon] or NULL: u_rot, v_rot of d_out64 rounded to
 *    float32 (what rwrt_bs_ready reads); needs both bits in `planes`.
 *  d_out64 NULL: with d_rot32 NULL coefficients only; with d_rot32 only for
 *    planes == RWRT_SHV_UROT | RWRT_SHV_VROT (nothing but the float32 pair).
 *  d_scratch: npair*(4 + popcount(planes))*(trunc+1)*nlat*2 doubles.
 * RWRT_ERR_ARG: nlat even or < 3, nlon odd, trunc < 1 or > (nlat-1)/2, an empty
 * mask or unknown bits, npair < 0 or npair * max(2, popcount) > 65535, d_u, d_v,
 * d_out64, d_rot32 overlapping, a NULL buffer, or a row (nlon) or an order
 * (trunc) too large for LDS.  npair == 0 is a no-op.  Every sum has a fixed
 * order (no atomics): a call's output is bit-identical from call to call, and
 * a pair's result does not depend on the batch it is in, nor a plane's on the
 * other planes asked for.  Asynchronous and ordered on `stream`; needs no
 * rwrt_ctx. */
rwrt_status rwrt_sh_helmholtz(int32_t nlon, int32_t nlat, int32_t npair, int32_t trunc, uint32_t planes,
                              const float* d_u, const float* d_v, const double* d_w, const double* d_x,
                              double* d_spec, double* d_out64, float* d_rot32,
                              double* d_scratch, void* stream);

/* The Rossby-wave source of Sardeshmukh & Hoskins (1988), pointwise from planes
 * of two decompositions A and B, each [nfield][nlat][nlon] fp64 (the
 * definition is helmholtz.reference_rws):
 *   S = -(vrt_B + f) div_A - (udiv_A vrtx_B + vdiv_A (vrty_B + beta)),
 *   f = 2 Omega sin(lat), beta = 2 Omega cos(lat) / a; planetary == 0: f = beta = 0.
 * d_x as in rwrt_sh_filter.  RWRT_ERR_ARG: the grid, nfield < 0 (or > 65535),
 * planetary not 0 or 1, a NULL buffer, d_out overlapping a plane.  nfield == 0
 * is a no-op.  One kernel, asynchronous on `stream`; needs no rwrt_ctx. */
rwrt_status rwrt_sh_rws(int32_t nlon, int32_t nlat, int32_t nfield, int32_t planetary, const double* d_x,
                        const double* d_div_a, const double* d_udiv_a, const double* d_vdiv_a,
                        const double* d_vrt_b, const double* d_vrtx_b, const double* d_vrty_b,
                        double* d_out, void* stream);

/* Solver construction: RungeKutta.__init__ (rkf45.py:335-366) with
 * select_initial_step (rkf45.py:34-99) on d_y0[5][nray].
 * Writes d_state[12][nray] = y f t(=0) h_abs, zeroes d_count[nray][2]
 * (accepted, rejected), sets d_nanrow[nray] = nt and d_live[nray] (1 if the
 * ray's state has a finite mean, rkf45.py:400-403).  d_summary[2] (int64,
 * zeroed here) accumulates {live rays, live rays with a finite h_abs}: the
 * host raises RWRT_SOLVER_FAILED when the first is > 0 and the second is 0
 * (the only way rkf45.py:423-425 can trigger). */
rwrt_status rwrt_rk45_init(const rwrt_grid* g, const double* d_packed,
                           int64_t nray, const double* d_y0,
                           const rwrt_params* p, double* d_state,
                           int64_t* d_count, int32_t* d_nanrow,
                           int32_t* d_live, int64_t* d_summary, void* stream);

/* The ray loop WR.core_ray_run_rk45 (wr.py:767-887) for output rows
 * it_begin <= i < it_end (1 <= it_begin < it_end <= nt): every ray is stepped
 * to d_tbound[i] (t_eval, wr.py:798-801) with the reference's step control
 * (rkf45.py:222-253,375-514), then masked (wr.py:838-850) and its group
 * velocity recomputed (wr.py:856-865).  Rays are taken from device work
 * queues in the order d_order[nray] (NULL = 0..nray-1); the first n_heavy
 * entries (live rays, at most 4 x rays-per-wave per CU on half the CUs) run
 * in latency mode -- four lanes of a wave per ray, in the first blocks of the
 * same grid (pass the rays expected to be slowest; 0 = none).
 * Output row r of
 * ray j is d_out[(j*(it_end-it_begin) + r)*8 + {lon,lat,k,l,amp,ug,vg,nacc}].
 * d_state / d_count / d_nanrow carry the per-ray solver state across calls
 * (time chunking).  d_work: >= 2 int32 of scratch (queue heads), reset by
 * this call on `stream`.  Results do not depend on the order or n_heavy.
 * Rays frozen at the call's start (NaN in their state) are flagged in the
 * context's scratch (1 byte per ray, grown on demand) and their rows written
 * by a kernel on the context's side stream; `stream` waits for it, so the
 * call remains one stream-ordered operation (also for rwrt_rk45_run_tv and
 * rwrt_rk4_run). */
rwrt_status rwrt_rk45_run(rwrt_ctx* ctx, const rwrt_grid* g, const double* d_packed,
                          int64_t nray, const rwrt_params* p,
                          const double* d_tbound, int32_t it_begin,
                          int32_t it_end, const int64_t* d_order,
                          int64_t n_heavy, double* d_state, int64_t* d_count,
                          int32_t* d_nanrow, double* d_out, int32_t* d_work,
                          void* stream);

/* rwrt_rk45_run with constant row tails (ABI 3).  A ray frozen at the call's
 * start (a NaN in its state, rkf45.py:400-403: dead root slots, rays masked
 * by wr.py:838-850 in an earlier call) repeats one row for the whole call
 * (wr.py:868-876 stores the unchanged state).  Instead of writing that row
 * into d_out for every row, the call stores it once:
 *  d_tail_from[nray] (int32): the first row i (it_begin <= i <= it_end) from
 *    which ray j's rows of this call all equal d_tail_row[j] and are NOT
 *    written to d_out; it_end when the ray has no constant tail (every row of
 *    it is in d_out).  This build gives the rays frozen at the call's start
 *    it_begin and every other ray it_end (a ray that freezes during the call
 *    writes its remaining rows, as rwrt_rk45_run does).
 *  d_tail_row[nray][8] (16-byte aligned): ray j's last row of the call, row
 *    it_end - 1 -- its tail row where d_tail_from[j] < it_end, and for every
 *    other ray the row the call wrote last into d_out (stored where the ray's
 *    state is written back), so a caller that wants the end points of a call
 *    reads them here whatever the layout of d_out.
 * rwrt_expand_tails writes the tails into d_out for a consumer that wants the
 * rows dense: then d_out equals rwrt_rk45_run's bit for bit, as do the state,
 * counters and nanrow after every call.  NULL d_tail_from and d_tail_row:
 * rwrt_rk45_run itself.  (C3: 116 GB of constant rows per 90-day step that
 * are never written.) */
rwrt_status rwrt_rk45_run_tails(rwrt_ctx* ctx, const rwrt_grid* g, const double* d_packed,
                                int64_t nray, const rwrt_params* p,
                                const double* d_tbound, int32_t it_begin,
                                int32_t it_end, const int64_t* d_order,
                                int64_t n_heavy, double* d_state, int64_t* d_count,
                                int32_t* d_nanrow, double* d_out, int32_t* d_tail_from,
                                double* d_tail_row, int32_t* d_work, void* stream);
/* d_out[(j*(it_end-it_begin) + r)*8 + 0..7] := d_tail_row[j][0..7] for every
 * ray j and row it_begin + r >= d_tail_from[j] (the dense rows of a tails
 * call); other rows are not touched. */
rwrt_status rwrt_expand_tails(int64_t nray, int32_t it_begin, int32_t it_end,
                              const int32_t* d_tail_from, const double* d_tail_row,
                              double* d_out, void* stream);

/* ABI 4: rows only for the rays live at the call's start.  rwrt_row_slots
 * numbers the rays whose state has a finite mean (rkf45.py:400-403: the rays
 * a call steps; every other ray repeats one row, its tail) in ray order:
 *  d_row_slot[nray] (int32) := j's index among them, -1 for a frozen ray;
 *  d_nslot[0] (int64) := their number.
 * rwrt_rk45_run_slots is rwrt_rk45_run_tails with ray j's rows at
 * d_out[(d_row_slot[j]*(it_end-it_begin) + r)*8 + 0..7]: d_out holds
 * nslot x rows x 8 doubles instead of nray x rows x 8 (C3: the 716 400 live
 * rays of 2.40 M slots, 49.5 GB instead of 166 GB for a 1 080-row call).
 * d_row_slot must come from rwrt_row_slots on the call's own d_state (after
 * the previous call); tails are required.  rwrt_expand_slots writes the dense
 * rows d_out[nray][rows][8] of such a call from its row blocks d_rows and its
 * tails: equal bit for bit to rwrt_rk45_run's d_out. */
rwrt_status rwrt_row_slots(int64_t nray, const double* d_state, int32_t* d_row_slot, int64_t* d_nslot,
                           void* stream);
rwrt_status rwrt_rk45_run_slots(rwrt_ctx* ctx, const rwrt_grid* g, const double* d_packed,
                                int64_t nray, const rwrt_params* p,
                                const double* d_tbound, int32_t it_begin,
                                int32_t it_end, const int64_t* d_order,
                                int64_t n_heavy, double* d_state, int64_t* d_count,
                                int32_t* d_nanrow, double* d_out, const int32_t* d_row_slot,
                                int32_t* d_tail_from, double* d_tail_row, int32_t* d_work,
                                void* stream);
rwrt_status rwrt_expand_slots(int64_t nray, int32_t it_begin, int32_t it_end, const int32_t* d_row_slot,
                              const int32_t* d_tail_from, const double* d_tail_row, const double* d_rows,
                              double* d_out, void* stream);

/* ABI 5, additive: what orders a ray-loop call, decided in one call.  From the
 * state and counters a previous call left, for every ray j:
 *  d_work[j] (int64) := d_count[j][0] + d_count[j][1] - d_prev_work[j], the
 *    attempts since the call d_prev_work was taken before (RWRT_PLAN_SINCE),
 *    or every attempt so far (RWRT_PLAN_TOTAL); then
 *  d_prev_work[j] := d_count[j][0] + d_count[j][1] (in and out; it must not
 *    exceed the counters on entry: work is not negative);
 *  d_row_slot[nray], d_nslot[0]: exactly what rwrt_row_slots gives on d_state;
 *  d_order[nray] (int64): the rays live now (rwrt_row_slots' test) by
 *    descending d_work, equal work in ascending ray index, then the frozen
 *    rays in ascending ray index -- the d_order of a rwrt_rk45_run* call that
 *    starts its longest rays first;
 *  h_nlive[0] (int64, HOST memory) := the number of live rays (= d_nslot[0]).
 * The call runs a fixed number of small kernels and a radix sort of the live
 * rays over the bits of the largest d_work on `stream`, and waits on the
 * stream once (for h_nlive).  d_scratch: rwrt_launch_plan_bytes(nray) bytes
 * of device memory, 256-byte aligned, the caller's (contents do not matter;
 * a larger buffer serves a smaller nray). */
#define RWRT_PLAN_SINCE 0
#define RWRT_PLAN_TOTAL 1
rwrt_status rwrt_launch_plan_bytes(int64_t nray, int64_t* bytes);
rwrt_status rwrt_launch_plan(int64_t nray, int32_t policy, const double* d_state,
                             const int64_t* d_count, int64_t* d_prev_work, int64_t* d_work,
                             int64_t* d_order, int32_t* d_row_slot, int64_t* d_nslot,
                             int64_t* h_nlive, void* d_scratch, int64_t scratch_bytes, void* stream);

/* ABI 5: ray-density maps.  The output rows of a ray-loop call are binned
 * where they lie instead of being shipped to the host: how many ray points
 * fall into each box of a regular lon-lat map, optionally with the sum of one
 * row column (the amplitude), in nchan maps selected per ray.  The definition
 * is density.reference_bins (NumPy); csrc/density_bins.h restates it and the
 * counts equal NumPy's exactly.  For a row point (lon, lat, w) of a ray with
 * channel c:
 *   lam = (lon % 2 pi) % 2 pi          (Python float %, as every lookup of the
 *                                       ray loops wraps its longitude)
 *   ix  = min(floor(lam * inv_dlon), nx - 1)
 *   iy  = floor((lat - lat0) * inv_dlat)
 * binned iff lon and lat are finite, 0 <= iy < ny, 0 <= c < nchan and, when
 * wcol >= 0, w is finite: count[c][iy][ix] += 1 and wsum[c][iy][ix] += w.
 * inv_dlon and inv_dlat are computed once by the caller (fp64) and never
 * recomputed on the device. */
typedef struct {
  int32_t nx, ny, nchan, wcol;   /* wcol: -1 counts only, 2..6 also sum that row column */
  double inv_dlon;               /* nx / (2 pi)          */
  double lat0, inv_dlat;         /* rad; ny / (lat1-lat0) */
} rwrt_density_map;              /* 40 bytes */

/* Bins rows it_begin <= i < it_end of nray rays and ACCUMULATES into
 * d_count[nchan][ny][nx] (int64) and, with wcol >= 0, d_wsum (fp64): the
 * caller zeroes them once, so time chunks and shards add up.  Row layouts are
 * those of the run entry points:
 *  d_row_slot == NULL: dense rows d_rows[nray][rows][8];
 *  otherwise row blocks d_rows[nslot][rows][8] with ray j in block
 *    d_row_slot[j], -1: the ray has no block and all its rows are its tail
 *    (tails are required with slots);
 *  d_tail_from / d_tail_row non-NULL: rows i >= d_tail_from[j] (any value in
 *    [it_begin, it_end]) are d_tail_row[j][8] and are not read from d_rows; a
 *    finite tail adds its row count to one bin at once (the weight as
 *    w * rows).
 * d_chan[nray] (int32) is each ray's map, NULL: map 0 for every ray; a ray
 * with a channel outside [0, nchan) is skipped.  Equal-bin runs of a ray's
 * consecutive rows are combined before the atomic.  Counts are exact; the
 * weighted sums depend on the arrival order in their last bits.  Asynchronous
 * and ordered on `stream`; needs no rwrt_ctx.  nray == 0 is a no-op. */
rwrt_status rwrt_ray_density(const rwrt_density_map* m, int64_t nray,
                             int32_t it_begin, int32_t it_end,
                             const double* d_rows, const int32_t* d_row_slot,
                             const int32_t* d_tail_from, const double* d_tail_row,
                             const int32_t* d_chan, int64_t* d_count, double* d_wsum,
                             void* stream);

/* ABI 5, additive: per-ray path summaries.  The same rows reduced per ray
 * instead of per map box: how far the ray travelled, how often it was
 * reflected, which latitudes it reached, where and when it stopped, and when
 * and for how long it was inside up to RWRT_SUMMARY_MAXREG lon-lat boxes.  The
 * definition is summary.reference_summary (NumPy); csrc/summary_rows.h restates
 * it.  A row is valid iff lon and lat are finite; a path segment (the
 * haversine angle of the reference's cal_dis) and a sign change of l are
 * counted for row i iff rows i-1 and i are both valid.
 *
 * Accumulators are struct-of-arrays, one column per ray.
 *  d_f64[RWRT_SUMMARY_NF64][nacc_cols], rows in this order:
 *    lon_first lat_first   first valid row             (NaN: none yet)
 *    lon_last lat_last l_last   last valid row         (NaN: none yet)
 *    lat_min lat_max       over valid rows             (+inf / -inf)
 *    amp_max               max |amp|, finite amp only  (-inf)
 *    path                  radians, summed in row order (0)
 *  d_i32[RWRT_SUMMARY_NI32 + 2 nreg][nacc_cols]:
 *    n_valid (0)  last_row (-1)  n_turn (0)  prev_valid (0)
 *    first_row[nreg]       first valid row inside box r (-1: never)
 *    rows_inside[nreg]     valid rows inside box r      (0)
 * The caller writes the initial values (in brackets) once; every call loads a
 * ray's column, updates it with rows it_begin <= i < it_end and stores it, so
 * a ray's rows may arrive in several calls.  The accumulators are a running
 * state, not a sum: the calls for one ray must deliver CONSECUTIVE rows in
 * order -- each call's it_begin equals the previous call's it_end (row 0, the
 * initial row, is a call of its own with it_begin = 0) -- because prev_valid
 * and lon_last, lat_last, l_last are the carried previous row.  Nothing
 * checks that on the device.  Two rays must not share a column in one call. */
#define RWRT_SUMMARY_MAXREG 8
#define RWRT_SUMMARY_NF64 9
#define RWRT_SUMMARY_NI32 4
typedef struct {
  int32_t nreg, reserved;                  /* 0 .. RWRT_SUMMARY_MAXREG boxes */
  double box[RWRT_SUMMARY_MAXREG][4];      /* radians: lon_w lon_e lat_s lat_n; inside: lat_s <= lat < lat_n and,
                                              lam = (lon % 2 pi) % 2 pi, lon_w <= lam < lon_e -- or, when
                                              lon_w >= lon_e (a box across 0), lam >= lon_w or lam < lon_e */
} rwrt_summary_regions;                    /* 264 bytes */

/* Row layouts (dense, tails, row blocks) and their argument rules are those
 * of rwrt_ray_density.  d_ray[nray] (int64): ray j of the call accumulates
 * into column d_ray[j] (a shard's rays in the whole set's arrays), NULL:
 * column j; a ray whose column is outside [0, nacc_cols) is skipped.  reg
 * NULL: no boxes.  One lane walks one ray; no atomics.  Asynchronous and
 * ordered on `stream`; needs no rwrt_ctx.  nray == 0 is a no-op. */
rwrt_status rwrt_ray_summary(int64_t nray, int32_t it_begin, int32_t it_end,
                             const double* d_rows, const int32_t* d_row_slot,
                             const int32_t* d_tail_from, const double* d_tail_row,
                             const int64_t* d_ray, int64_t nacc_cols,
                             const rwrt_summary_regions* reg,
                             double* d_f64, int32_t* d_i32, void* stream);

/* ABI 5, additive: arrival-time maps.  The same rows reduced per map box to
 * WHEN ray points fall into it: the first and the last output row with a point
 * in the box and, per time window of window_rows rows, how many points.  The
 * definition is arrival.reference_arrival (NumPy); csrc/arrival_rows.h
 * restates it and every output equals NumPy's exactly.  A point is binned as
 * by rwrt_ray_density (`bins`), with bins.wcol read as "the row column that
 * must be finite" (-1: none): nothing is summed.  Row i lies in window
 * i / window_rows. */
typedef struct {
  rwrt_density_map bins;
  int32_t window_rows;           /* 0: no counts (d_count is not used) */
  int32_t nwin;                  /* windows of d_count; it_end <= nwin * window_rows */
} rwrt_arrival_map;              /* 48 bytes */

/* Reduces rows it_begin <= i < it_end of nray rays and ACCUMULATES into
 * d_first[nchan][ny][nx] (int32, min of the row index), d_last (int32, max)
 * and, with window_rows > 0, d_count[nwin][nchan][ny][nx] (int64, add;
 * nwin*nchan*ny*nx < 2^31): the caller writes INT32_MAX, -1 and 0 once, so
 * time chunks and shards combine.  Row layouts, d_chan and their argument
 * rules are those of rwrt_ray_density.  Equal-bin runs of a ray's consecutive
 * rows are combined before the atomics (one min, one max, one add per run and
 * one more add per window the run enters); a constant tail is one run and
 * costs one add per window it touches.  Asynchronous and ordered on `stream`;
 * needs no rwrt_ctx.  nray == 0 is a no-op. */
rwrt_status rwrt_ray_arrival(const rwrt_arrival_map* m, int64_t nray,
                             int32_t it_begin, int32_t it_end,
                             const double* d_rows, const int32_t* d_row_slot,
                             const int32_t* d_tail_from, const double* d_tail_row,
                             const int32_t* d_chan, int32_t* d_first, int32_t* d_last,
                             int64_t* d_count, void* stream);

/* ABI 5, additive: wave-ray flux maps.  The same rows reduced per map box to
 * a vector: the sum of the group velocities (or of their directions) of the
 * ray points in the box, with their number, the sum of their row indices and
 * the sum of their speeds -- the magnitude and direction of wave activity, the
 * mean propagation time and the mean speed per box.  The definition is
 * flux.reference_flux (NumPy); csrc/flux_rows.h restates it.
 *
 * A row (lon lat k l amp ug vg) at row index i of a ray with channel c is
 * accepted iff 0 <= c < nchan; lon, lat, ug, vg are finite; |k| <= wn_max and
 * |l| <= wn_max (false for NaN); s2 = ug*ug + vg*vg (two rounded products, one
 * rounded sum, no FMA) is finite and s2_min <= s2 <= s2_max; with unit vectors
 * s2 > 0; and the point falls in a bin.  The latitude index is
 * rwrt_ray_density's.  The longitude index is rwrt_ray_density's too (wrapped,
 * nx bins over [0, 2 pi), lon0 = 0), or, with mode bit 1, that of the
 * UNWRAPPED window: fx = floor((lon - lon0) * inv_dlon), binned iff
 * 0 <= fx < nx compared in fp64 -- the ray loops never wrap lon, so eastward
 * and westward routes around the globe stay apart.  With speed = sqrt(s2) an
 * accepted point adds 1 and i to the bin's integers and (ug, vg, speed) -- with
 * mode bit 0 (ug / speed, vg / speed, speed) -- to its sums.  The amplitude is
 * no criterion. */
typedef struct {
  int32_t nx, ny, nchan;
  int32_t mode;             /* bit 0: unit vectors; bit 1: unwrapped longitude window */
  double lon0, inv_dlon;    /* rad; nx / (lon1 - lon0).  wrapped: 0 and nx / (2 pi) */
  double lat0, inv_dlat;    /* rad; ny / (lat1 - lat0) */
  double s2_min, s2_max;    /* squares of the speed bounds, computed once by the caller */
  double wn_max;
} rwrt_flux_map;            /* 72 bytes */

/* Reduces rows it_begin <= i < it_end of nray rays and ACCUMULATES into
 * d_cnt[nchan][ny][nx][2] (int64: count, rowsum) and d_sum[nchan][ny][nx][3]
 * (fp64: fx, fy, fs): the caller zeroes them once, so time chunks and shards
 * add up.  A bin's accumulators are interleaved so that one update touches
 * neighbouring addresses.  Row layouts, d_chan and their argument rules are
 * those of rwrt_ray_density.  Equal-bin runs of a ray's consecutive rows are
 * summed in row order before the atomics (two integer and three fp64 adds per
 * run); a constant tail of n rows from row tf on is one run: count += n,
 * rowsum += n tf + n (n - 1) / 2, each sum += v * n.  count and rowsum are
 * exact; the sums depend on the arrival order in their last bits.
 * RWRT_ERR_ARG before any HIP call: a NULL map, d_cnt or d_sum; nx, ny or
 * nchan not positive; nchan*ny*nx >= 2^31; mode bits >= 4; inv_dlon or
 * inv_dlat not finite and positive; lon0 or lat0 not finite; wrapped with
 * lon0 != 0; s2_min NaN or negative, s2_max NaN or below s2_min; wn_max NaN or
 * negative; the row arguments as for rwrt_ray_density.  Asynchronous and
 * ordered on `stream`; needs no rwrt_ctx.  nray == 0 is a no-op. */
rwrt_status rwrt_ray_flux(const rwrt_flux_map* m, int64_t nray,
                          int32_t it_begin, int32_t it_end,
                          const double* d_rows, const int32_t* d_row_slot,
                          const int32_t* d_tail_from, const double* d_tail_row,
                          const int32_t* d_chan, int64_t* d_cnt, double* d_sum,
                          void* stream);

/* ABI 5, additive: residence-time maps along ray segments.  The point maps
 * above bin one point per ray per row; here the straight segment (in lon-lat)
 * between two consecutive valid rows of a ray is deposited into every map box
 * it passes through, each box receiving the fraction of the segment inside it,
 * so that a map does not depend on the output interval, has no gaps and
 * conserves the total: every live segment deposits exactly one row interval.
 * The definition is track.reference_track (Python); csrc/track_cells.h
 * restates it.
 *
 * Grid coordinates of a row: X = (lon - lon0) * inv_dlon and
 * Y = (lat - lat0) * inv_dlat (one rounded subtraction, one rounded product,
 * no FMA); lon is never wrapped (wrapped maps have lon0 = 0), so X may be
 * negative or above nx.  A row is valid iff lon and lat are finite and, when
 * need >= 0 / wcol >= 0, its columns `need` / `wcol` are finite.  Segment i
 * joins rows i-1 and i of a ray and is considered iff both are valid and the
 * ray's channel is in [0, nchan).  With fx0 fy0 fx1 fy1 the floors of its end
 * points (fp64) it is DROPPED -- d_dropped += 1 and nothing else -- if any
 * |f| > 2^30 or ncx + ncy + 1 > max_cells, ncx = |fx1 - fx0|, ncy =
 * |fy1 - fy0|, both compared in fp64 before any conversion.  Otherwise it
 * starts in cell (fx0, fy0) at t = 0 and crosses ncx x-lines and ncy y-lines,
 * line g at t = (g - X0) / (X1 - X0) resp. (g - Y0) / (Y1 - Y0) (IEEE
 * division), taken in ascending t, a tie going to x; the cell left at t_next
 * is emitted with weight t_next - t, the last cell with 1.0 - t, a segment
 * inside one cell with exactly 1.0.  An emitted cell (ix, iy, w) is deposited
 * iff 0 <= iy < ny and, wrapped, into column ix mod nx (non-negative) or, with
 * mode bit 1 (the unwrapped window of rwrt_flux_map), iff 0 <= ix < nx:
 * cnt += 1, time += w and, with wcol >= 0, wsum += w * (0.5 * (v0 + v1)), v
 * the column wcol at the two ends. */
typedef struct {
  int32_t nx, ny, nchan;
  int32_t mode;             /* bit 1: unwrapped longitude window; no other bit */
  int32_t need, wcol;       /* row columns, -1 (none) or 2..6: must be finite / is integrated */
  int32_t max_cells;        /* >= 1: the most cells one segment may pass through */
  int32_t reserved;
  double lon0, inv_dlon;    /* rad; nx / (lon1 - lon0).  wrapped: 0 and nx / (2 pi) */
  double lat0, inv_dlat;    /* rad; ny / (lat1 - lat0) */
} rwrt_track_map;           /* 64 bytes */

/* Deposits the segments that end on rows it_begin <= i < it_end of nray rays
 * and ACCUMULATES into d_cnt (int64), d_time and d_wsum (fp64; NULL iff
 * wcol < 0), each [nchan][ny][nx], and d_dropped[1] (int64): the caller zeroes
 * them once, so time chunks and shards add up.  Row layouts and their argument
 * rules are those of rwrt_ray_density.  d_ray[nray] (int64): ray j of the call
 * is column d_ray[j] (a shard's rays in the whole set's arrays), NULL: column
 * j; a ray whose column is outside [0, nacc_cols) is skipped.  d_chan
 * [nacc_cols] (int32) is indexed by that column, NULL: channel 0.
 *  d_prev[3][nacc_cols] (fp64): the carried previous row of every ray -- lon
 *    (NaN: no valid previous row), lat, and the value of column wcol (0
 *    without one).  The caller writes NaN once; every call loads a ray's
 *    column, walks its rows and stores the last row, with lon = NaN if that
 *    row was invalid.  It is a running state, not a sum: the calls for one ray
 *    must deliver CONSECUTIVE rows in order -- each call's it_begin equals the
 *    previous call's it_end (row 0, the initial row, is a call of its own with
 *    it_begin = 0, which deposits nothing).  Nothing checks that on the
 *    device.  Two rays must not share a column in one call.  A ray whose
 *    channel is outside [0, nchan) is not walked and its column stays.
 * One lane walks one ray and keeps the current cell's visits and sums in
 * registers across segments (a ray ends a segment in the cell in which it
 * starts the next), adding them to the map only when the cell changes: one
 * 64-bit integer add and one or two hardware fp64 adds, no compare-exchange
 * loop.  A constant tail of n rows is its first segment plus one update for
 * the n - 1 segments of length zero.  cnt and dropped are exact; time and
 * wsum depend on the arrival order in their last bits.
 * RWRT_ERR_ARG before any HIP call: a NULL map, d_prev, d_cnt, d_time or
 * d_dropped; d_wsum present without wcol or missing with it; nx, ny or nchan
 * not positive; nchan*ny*nx >= 2^31; mode other than 0 or 2; max_cells < 1;
 * need or wcol outside {-1, 2..6}; inv_dlon or inv_dlat not finite and
 * positive; lon0 or lat0 not finite; wrapped with lon0 != 0; it_begin < 0;
 * nacc_cols not covering the rays; the row arguments as for rwrt_ray_density.
 * Asynchronous and ordered on `stream`; needs no rwrt_ctx.  nray == 0 is a
 * no-op. */
rwrt_status rwrt_ray_track(const rwrt_track_map* m, int64_t nray,
                           int32_t it_begin, int32_t it_end,
                           const double* d_rows, const int32_t* d_row_slot,
                           const int32_t* d_tail_from, const double* d_tail_row,
                           const int64_t* d_ray, int64_t nacc_cols, const int32_t* d_chan,
                           double* d_prev, int64_t* d_cnt, double* d_time,
                           double* d_wsum, int64_t* d_dropped, void* stream);

/* ABI 5, additive: gate-crossing maps.  The maps above reduce per lon-lat
 * box; a line has no area.  Here every passage of a ray's segment (two
 * consecutive valid rows) through a GATE -- a latitude circle or a meridian --
 * is counted by direction, binned along the gate, timed, and recorded per ray.
 * The definition is cross.reference_cross (Python); csrc/cross_lines.h
 * restates it.  Every operation is one rounded fp64 + - * / or a floor, no
 * FMA, IEEE division.
 *
 * kind 0, latitude circle lat = pos: s(lat) = (lat >= pos); the segment
 *   crosses iff s0 != s1, in direction 0 (northward) iff s1, else 1;
 *   t = (pos - lat0) / (lat1 - lat0); lon_c = lon0 + t * (lon1 - lon0); bin
 *   min(floor(lam * inv_d), nbin - 1), lam = (lon_c % 2 pi) % 2 pi (Python's
 *   float %, as rwrt_ray_density wraps); org is 0.
 * kind 1, meridian lon = pos + 2 pi n, 0 <= pos < 2 pi: u = lon - pos,
 *   m = floor(u * (1 / (2 pi))) -- lon is never wrapped; the segment crosses iff
 *   m0 != m1, in direction 0 (eastward) iff m1 > m0, else 1.  It is DROPPED
 *   for that gate -- d_dropped += 1 and nothing else -- iff |m0| > 2^30,
 *   |m1| > 2^30 or |m1 - m0| > 1, compared in fp64.  Otherwise
 *   G = max(m0, m1) * (2 pi), t = (G - u0) / (u1 - u0) clamped to [0, 1],
 *   lat_c = lat0 + t * (lat1 - lat0), bin floor((lat_c - org) * inv_d), in
 *   the map iff 0 <= bin < nbin.
 * A row is valid as for rwrt_ray_track: lon, lat and the columns need / wcol
 * finite; segment i joins rows i-1 and i and is considered iff both are valid
 * and the ray's channel c is in [0, nchan).  A crossing of gate g in direction
 * d on segment i happens at tc = (double)(i - 1) + t rows, in the window
 * w = (i - 1) / window_rows (0 without windows).  Per ray, always:
 * ncross[g][d] += 1, tfirst[g][d] = tc if it was NaN.  Per bin, when the
 * crossing is in the map: cnt[w][g][d][c][bin] += 1, tsum += tc and, with
 * wcol >= 0, wsum += v0 + t * (v1 - v0). */
#define RWRT_CROSS_MAXGATE 8
typedef struct {
  int32_t kind, reserved;   /* 0: latitude circle, 1: meridian */
  double pos;               /* rad; a meridian's in [0, 2 pi) */
  double org, inv_d;        /* the bins along the gate: nbin over longitude (org 0, nbin / (2 pi))
                               resp. over latitude (lat0, nbin / (lat1 - lat0)) */
} rwrt_cross_gate;          /* 32 bytes */

typedef struct {
  int32_t ngate, nbin, nchan;
  int32_t need, wcol;       /* row columns, -1 (none) or 2..6: must be finite / is interpolated */
  int32_t window_rows, nwin;   /* 0 and 1: no time windows */
  int32_t reserved;
  rwrt_cross_gate gate[RWRT_CROSS_MAXGATE];
} rwrt_cross_map;           /* 288 bytes */

/* Finds the crossings of the segments that end on rows it_begin <= i < it_end
 * of nray rays and ACCUMULATES into d_cnt (int64), d_tsum and d_wsum (fp64;
 * NULL iff wcol < 0), each [nwin][ngate][2][nchan][nbin], d_dropped[1] (int64)
 * and, unless both are NULL (maps only), d_ncross (int32) and d_tfirst (fp64),
 * each [ngate][2][nacc_cols]: the caller zeroes the maps, d_dropped and
 * d_ncross and writes NaN into d_tfirst and d_prev once, so time chunks and
 * shards add up.  Row layouts, d_ray, d_chan (indexed by column) and d_prev
 * [3][nacc_cols] -- the carried previous row, a running state fed CONSECUTIVE
 * rows, row 0 in a call of its own -- are those of rwrt_ray_track; a ray whose
 * channel is outside [0, nchan) is not walked and its columns stay.
 * One lane walks one ray; a row's side of every gate (s, or m) is computed
 * once and carried to the next row, and only where two sides differ are the
 * division, the interpolation and the atomics made: one 64-bit integer add and
 * one or two hardware fp64 adds, no compare-exchange loop; the ray's own
 * column of d_ncross / d_tfirst takes plain loads and stores.  A constant tail
 * is its first row: segments of length zero cross nothing.  cnt, ncross and
 * dropped are exact, tfirst is written in row order and equals the definition
 * bit for bit; tsum and wsum depend on the arrival order in their last bits.
 * RWRT_ERR_ARG before any HIP call: a NULL map, d_prev, d_cnt, d_tsum or
 * d_dropped; d_wsum present without wcol or missing with it; exactly one of
 * d_ncross and d_tfirst; ngate outside 1..8; nbin or nchan not positive;
 * nwin*ngate*2*nchan*nbin >= 2^31; kind other than 0 or 1; pos or org not
 * finite; inv_d not finite and positive; a latitude circle with org != 0; a
 * meridian's pos outside [0, 2 pi); need or wcol outside {-1, 2..6};
 * window_rows < 0, nwin < 1, window_rows == 0 with nwin != 1, or it_end - 1 >
 * nwin * window_rows with windows; it_begin < 0; nacc_cols not covering the
 * rays; the row arguments as for rwrt_ray_density.  Asynchronous and ordered
 * on `stream`; needs no rwrt_ctx.  nray == 0 is a no-op. */
rwrt_status rwrt_ray_cross(const rwrt_cross_map* m, int64_t nray,
                           int32_t it_begin, int32_t it_end,
                           const double* d_rows, const int32_t* d_row_slot,
                           const int32_t* d_tail_from, const double* d_tail_row,
                           const int64_t* d_ray, int64_t nacc_cols, const int32_t* d_chan,
                           double* d_prev, int64_t* d_cnt, double* d_tsum,
                           double* d_wsum, int64_t* d_dropped,
                           int32_t* d_ncross, double* d_tfirst, void* stream);

/* ABI 5, additive: the WKB phase along rays and wave-field maps.  A WKB wave
 * is A exp(i theta); the ray loops integrate A (the amp column) and the local
 * wavenumbers k, l, this integrates the phase theta = int k dlon + l dY along
 * every ray, dY = dlat / cos(lat) (k, l: the Mercator wavenumbers times the
 * earth's radius, as the rows carry them), and superposes the rays' waves per
 * map box.  The definition is phase.reference_phase (NumPy);
 * csrc/phase_rows.h restates it.
 *
 * A row is valid iff lon, lat, k and l are finite, |lat| < pi/2 (the double
 * nearest pi/2, compared in fp64) and the columns need / wcol, where named,
 * are finite; for a valid row a = l / cos(lat).  Segment i joins rows i-1 and
 * i and is joined iff both are valid and the ray's channel c is in
 * [0, nchan); then, one rounding per operation, in this order, no FMA:
 *   dk = (0.5 * (k0 + k1)) * (lon1 - lon0)
 *   dl = (0.5 * (a0 + a1)) * (lat1 - lat0)
 *   theta_i = theta_{i-1} + (dk + dl);  nseg += 1
 * else theta_i = theta_{i-1}.  Every valid row i (row 0 too) of a ray whose
 * channel is in range has psi = theta_i - omega_dt * (double)i and is binned
 * as rwrt_ray_density bins it (lam = (lon % 2 pi) % 2 pi, wrapped axis); a
 * binned row with a finite psi adds cnt += 1, re += w cos(psi), im += w
 * sin(psi), wabs += |w| (w: the column wcol, 1 without one, and then there is
 * no wabs); a binned row whose psi is not finite adds 1 to dropped and nothing
 * else. */
typedef struct {
  int32_t nx, ny, nchan;
  int32_t need, wcol;       /* row columns, -1 (none) or 2..6: must be finite / weighs the deposit */
  int32_t reserved;
  double lat0, inv_dlat;    /* rad; ny / (lat1 - lat0) */
  double inv_dlon;          /* nx / (2 pi) */
  double omega_dt;          /* the wave's frequency times the row interval, rad per row */
} rwrt_phase_map;           /* 56 bytes */

/* Integrates the phase over the segments that end on rows it_begin <= i <
 * it_end of nray rays and deposits those rows: ACCUMULATES into d_cnt (int64),
 * d_re, d_im and d_wabs (fp64; d_wabs NULL iff wcol < 0), each
 * [nchan][ny][nx], d_dropped[1] (int64) and, per ray column, d_theta (fp64)
 * and d_nseg (int32), each [nacc_cols].  The caller zeroes the maps, d_nseg
 * and d_dropped and writes theta_0 into d_theta and NaN into d_carry once, so
 * time chunks and shards add up.  Row layouts, d_ray and d_chan (indexed by
 * column) are those of rwrt_ray_track; a ray whose channel is outside
 * [0, nchan) is not walked and its columns stay.
 *  d_carry[4][nacc_cols] (fp64): the carried previous row of every ray -- lon
 *    (NaN: no valid previous row), lat, k and a.  A running state, like
 *    d_prev of rwrt_ray_track: the calls for one ray deliver CONSECUTIVE rows
 *    in order, once.  A call with it_begin == 0 treats its first row as row 0
 *    whatever d_carry holds: it sets the carry, deposits, and leaves theta as
 *    given.
 * One lane walks one ray: one cos per valid row (a is carried, not
 * recomputed), one sincos per deposit (the device library's), one 64-bit
 * integer add and two or three hardware fp64 adds per deposit, no
 * compare-exchange loop; the ray's own columns of d_theta, d_nseg and d_carry
 * take plain loads and stores.  A constant tail of n rows is its first row
 * plus n - 1 segments of length zero: nseg += n - 1, theta takes the one sum
 * (dk + dl) of such a segment (+0, or NaN where an average overflows), and the
 * n - 1 equal deposits are made as ONE product (double)(n - 1) * term per sum
 * when omega_dt == 0, row by row otherwise.  cnt, nseg and dropped are exact;
 * theta follows the definition's order of operations and differs from it only
 * through cos; re, im and wabs depend on the arrival order in their last bits.
 * RWRT_ERR_ARG before any HIP call: a NULL map, d_carry, d_theta, d_nseg,
 * d_cnt, d_re, d_im or d_dropped; d_wabs present without wcol or missing with
 * it; nx, ny or nchan not positive; nchan*ny*nx >= 2^31; need or wcol outside
 * {-1, 2..6}; inv_dlon or inv_dlat not finite and positive; lat0 or omega_dt
 * not finite; it_begin < 0; nacc_cols not covering the rays; the row
 * arguments as for rwrt_ray_density.  Asynchronous and ordered on `stream`;
 * needs no rwrt_ctx.  nray == 0 is a no-op. */
rwrt_status rwrt_ray_phase(const rwrt_phase_map* m, int64_t nray,
                           int32_t it_begin, int32_t it_end,
                           const double* d_rows, const int32_t* d_row_slot,
                           const int32_t* d_tail_from, const double* d_tail_row,
                           const int64_t* d_ray, int64_t nacc_cols, const int32_t* d_chan,
                           double* d_carry, double* d_theta, int32_t* d_nseg,
                           int64_t* d_cnt, double* d_re, double* d_im, double* d_wabs,
                           int64_t* d_dropped, void* stream);

/* ABI 5, additive: ray-tube maps -- geometric spreading, caustics and the
 * Maslov index per ray.  The first consumer that reads more than one ray's
 * rows per lane: ray j's tube is spanned by the difference vectors between its
 * neighbours in the source lattice, west to east (pair a) and south to north
 * (pair b).  The definition is tube.reference_tube (NumPy); csrc/tube_rows.h
 * restates it.
 *
 * A point is valid iff lon and lat are finite, |lat| < pi/2 (the double
 * nearest pi/2) and the column need, where named, is finite.  The stencil is
 * fixed at row 0: the pair (p, q) of direction a is (W, E) if both are valid
 * there, else (j, E), else (W, j), else none; direction b likewise.  A ray
 * invalid at row 0, without a pair in either direction, with a channel outside
 * [0, nchan) or with jac_0 == 0 has no tube.  At row i, one rounding per
 * operation, no FMA:
 *   dla = wrap(lon_q - lon_p), dpa = lat_q - lat_p       (dlb, dpb: pair b)
 *   jac = dla * dpb - dlb * dpa;  A = jac * cos(lat_j);  D = A / A_0
 * with wrap(d) = ((d + pi) % 2 pi) % 2 pi - pi (Python's %).  Row i is open iff
 * j and its stencil rays are valid there, max(|dla|, |dpa|, |dlb|, |dpb|) <=
 * max_sep and every earlier row was open; the first row that is not closes the
 * tube for good.  An open row i >= 1 whose (jac < 0) differs from the previous
 * row's is a caustic.  Every open row in the map adds cnt += 1, slog +=
 * log|D| in ray j's box (binned as rwrt_ray_density bins it), a caustic
 * ncaus += 1; an open row with jac == 0 adds 1 to dropped instead. */
typedef struct {
  int32_t nx, ny, nchan;
  int32_t need;             /* row column, -1 (none) or 2..6: must be finite */
  double lat0, inv_dlat;    /* rad; ny / (lat1 - lat0) */
  double inv_dlon;          /* nx / (2 pi) */
  double max_sep;           /* rad, positive; +inf: no limit */
} rwrt_tube_map;            /* 48 bytes */

#define RWRT_TUBE_NI 5      /* rows of d_state_i */
#define RWRT_TUBE_NF 13     /* rows of d_state_f */

/* Walks the tubes of all nray rays over rows it_begin <= i < it_end: ray j is
 * column j of every per-ray array, and every ray of the run is in the launch
 * (a ray reads its neighbours' rows).  ACCUMULATES into d_cnt, d_ncaus (int64)
 * and d_slog (fp64), each [nchan][ny][nx], and d_dropped[1] (int64).  Row
 * layouts and d_chan are those of rwrt_ray_density.
 *  d_nbr[4][nray] (int32): the W, E, S, N neighbour of every ray, -1 for
 *    none.  An index outside [-1, nray) is never followed: the ray counts as
 *    closed and bit 0 of d_err[0] (int32) is set.
 *  d_state_i[RWRT_TUBE_NI][nray] (int32): flags (bits 0-1 and 2-3: the pair of
 *    direction a and b -- 0 none, 1 (lo, hi), 2 (j, hi), 3 (lo, j); bit 4:
 *    open), mu, first (-1: none), nrow, close_row (-1: never).
 *  d_state_f[RWRT_TUBE_NF][nray] (fp64): jac_prev, jac_0, cos_0, dmin, dlast
 *    (signed), f0[4] and flast[4]: (dla cos, dpa, dlb cos, dpb) at row 0 and
 *    at the last open row.
 *    Both are a running state and the per-ray result at once: the calls
 *    deliver CONSECUTIVE rows in order, once.  A call with it_begin == 0
 *    fixes every stencil from its first row and starts the per-ray arrays
 *    over; before one, flags 0 (no tube) makes every other call a no-op.
 * One lane walks one ray and resolves its stencil rays' row blocks once per
 * call; where a ray and its whole stencil are in their constant tails, the n
 * remaining rows are the first of them plus ONE product (double)(n - 1) *
 * log|D|.  64-bit integer adds and hardware fp64 adds, no compare-exchange
 * loop.  Every integer rests on the sign of jac and is exact; D, f0 and flast
 * differ from the definition only through cos, slog also through log and the
 * arrival order.
 * RWRT_ERR_ARG before any HIP call: a NULL map, d_nbr, d_state_i, d_state_f,
 * d_cnt, d_slog, d_ncaus, d_dropped or d_err; nx, ny or nchan not positive;
 * nchan*ny*nx >= 2^31; need outside {-1, 2..6}; inv_dlon or inv_dlat not
 * finite and positive; lat0 not finite; max_sep not positive (NaN included);
 * it_begin < 0; the row arguments as for rwrt_ray_density.  Asynchronous and
 * ordered on `stream`; needs no rwrt_ctx.  nray == 0 is a no-op. */
rwrt_status rwrt_ray_tube(const rwrt_tube_map* m, int64_t nray,
                          int32_t it_begin, int32_t it_end,
                          const double* d_rows, const int32_t* d_row_slot,
                          const int32_t* d_tail_from, const double* d_tail_row,
                          const int32_t* d_chan, const int32_t* d_nbr,
                          int32_t* d_state_i, double* d_state_f,
                          int64_t* d_cnt, double* d_slog, int64_t* d_ncaus,
                          int64_t* d_dropped, int32_t* d_err, void* stream);

/* ABI 5, additive: caustic-aware wave-field maps.  The WKB wave of a ray is
 * A |D|^(-1/2) exp(i (theta - mu pi / 2)): rwrt_ray_phase integrates theta and
 * knows no caustic, rwrt_ray_tube finds D and the Maslov index mu and keeps
 * only the last of each.  Here one lane walks both, so that every row deposits
 * with the mu and the D it has there.  The definition is wave.reference_wave
 * (NumPy), a composition of the two definitions above; csrc/wave_rows.h
 * composes csrc/tube_rows.h and csrc/phase_rows.h in the same way.
 *
 * Per row i of ray j: open_i, jac_i, D_i and the running mu_i (a caustic at
 * row i counted) are rwrt_ray_tube's, with need and max_sep; theta_i, nseg and
 * the validity of the row are rwrt_ray_phase's, with need, wcol and omega_dt.
 * theta runs over every phase-valid row whether the tube is open or not.  Row
 * i deposits iff it is phase-valid, the tube is open there and the point lies
 * in the map, binned by position alone as rwrt_ray_tube bins it.  Then, in
 * this order, one rounding per operation, no FMA:
 *   jac_i == 0                      dropped += 1, nothing else
 *   |jac_i| < d_floor * |jac_0|     clipped += 1, nothing else
 *   w = wv (the column wcol, 1.0 without one); spread: w = wv / sqrt(|D_i|)
 *   psi = (theta_i - omega_dt * (double)i) - (double)mu_i * HALF_PI
 *   psi or w not finite             dropped += 1, nothing else
 *   cnt += 1, re += w cos(psi), im += w sin(psi), wabs += |w|
 * with HALF_PI the double nearest pi / 2. */
typedef struct {
  int32_t nx, ny, nchan;
  int32_t need, wcol;       /* row columns, -1 (none) or 2..6: must be finite / weighs the deposit */
  int32_t spread;           /* 1: divide the weight by sqrt(|D|); 0: the Maslov phase alone */
  double lat0, inv_dlat;    /* rad; ny / (lat1 - lat0) */
  double inv_dlon;          /* nx / (2 pi) */
  double max_sep;           /* rad, positive; +inf: no limit */
  double omega_dt;          /* the wave's frequency times the row interval, rad per row */
  double d_floor;           /* finite, >= 0: a deposit with |jac| below d_floor |jac_0| is clipped */
} rwrt_wave_map;            /* 72 bytes */

#define RWRT_WAVE_NI 6      /* rows of d_state_i */
#define RWRT_WAVE_NF 9      /* rows of d_state_f */

/* Walks the tube and the phase of all nray rays over rows it_begin <= i <
 * it_end: ray j is column j of every per-ray array, and every ray of the run
 * is in the launch (a ray reads its neighbours' rows).  ACCUMULATES into d_cnt
 * (int64), d_re, d_im and d_wabs (fp64), each [nchan][ny][nx], and into
 * d_dropped[1] and d_clipped[1] (int64).  Row layouts, d_chan, d_nbr and d_err
 * are those of rwrt_ray_tube; a ray whose channel is outside [0, nchan) is not
 * walked and its columns stay.
 *  d_state_i[RWRT_WAVE_NI][nray] (int32): flags, mu, first, nrow, close_row as
 *    in rwrt_ray_tube, and nseg.
 *  d_state_f[RWRT_WAVE_NF][nray] (fp64): the carried previous row lon (NaN:
 *    none), lat, k, a = l / cos(lat); theta; jac_prev, jac_0, cos_0 and dlast
 *    (signed).
 *    Both are a running state and the per-ray result at once: the calls
 *    deliver CONSECUTIVE rows in order, once.  The caller writes theta_0 into
 *    theta and zeroes nseg.  A call with it_begin == 0 treats its first row as
 *    row 0: it fixes every stencil and starts the tube's per-ray arrays over,
 *    forgets the carried row and leaves theta and nseg as given.
 * One lane walks one ray; while its tube is open it gathers its stencil rays'
 * rows per row, and a ray whose tube has closed goes on integrating theta
 * without them.  Where a ray and its whole stencil are in their constant
 * tails, the n remaining rows are the first of them plus ONE product
 * (double)(n - 1) * term per sum when omega_dt == 0, row by row otherwise.  One
 * 64-bit integer add and three hardware fp64 adds per deposit, no
 * compare-exchange loop.  Every integer, dropped and clipped rest on jac alone
 * and are exact; theta, mu, first, nrow, close_row and dlast are bit for bit
 * what rwrt_ray_phase and rwrt_ray_tube give for the same rows; re, im and
 * wabs depend on cos, sqrt, sincos and the arrival order in their last bits.
 * RWRT_ERR_ARG before any HIP call: a NULL map, d_nbr, d_state_i, d_state_f,
 * d_cnt, d_re, d_im, d_wabs, d_dropped, d_clipped or d_err; nx, ny or nchan
 * not positive; nchan*ny*nx >= 2^31; need or wcol outside {-1, 2..6}; spread
 * not 0 or 1; inv_dlon or inv_dlat not finite and positive; lat0 or omega_dt
 * not finite; max_sep not positive (NaN included); d_floor negative or not
 * finite; it_begin < 0; the row arguments as for rwrt_ray_density.
 * Asynchronous and ordered on `stream`; needs no rwrt_ctx.  nray == 0 is a
 * no-op. */
rwrt_status rwrt_ray_wave(const rwrt_wave_map* m, int64_t nray,
                          int32_t it_begin, int32_t it_end,
                          const double* d_rows, const int32_t* d_row_slot,
                          const int32_t* d_tail_from, const double* d_tail_row,
                          const int32_t* d_chan, const int32_t* d_nbr,
                          int32_t* d_state_i, double* d_state_f,
                          int64_t* d_cnt, double* d_re, double* d_im, double* d_wabs,
                          int64_t* d_dropped, int64_t* d_clipped, int32_t* d_err,
                          void* stream);

/* Fixed-step RK4 ray loop, the reference's default integrator:
 * WR.core_ray_run_numpy (wr.py:702-765) with rk4_step_numpy (wr.py:583-622)
 * and core_rk4_step (wr.py:89-95), for rows it_begin <= i < it_end, dt =
 * p->tstep.  A ray whose stage input is masked (|lat| >= pi/2 or |l| >= 100)
 * keeps its state for that step.  d_state rows 0..4 hold y (set them to the
 * initial rows before the first call); d_count[nray][2] = {steps taken, steps
 * held} -- held by a masked stage 2-4, or by a masked first stage, which
 * holds the ray for every remaining step (the step of a state with a NaN in
 * lon/lat/k/l is counted in neither); d_nanrow / d_out / d_work as for
 * rwrt_rk45_run (nacc column = steps taken); rays with such a NaN at the
 * call's start are written from the context's side stream as in
 * rwrt_rk45_run. */
rwrt_status rwrt_rk4_run(rwrt_ctx* ctx, const rwrt_grid* g, const double* d_packed,
                         int64_t nray, const rwrt_params* p, int32_t it_begin,
                         int32_t it_end, const int64_t* d_order,
                         double* d_state, int64_t* d_count, int32_t* d_nanrow,
                         double* d_out, int32_t* d_work, void* stream);

/* BS.ready on the device (bs.py:264-279 vorticity, bs.py:121-200 finite
 * differences, bs.py:291-305 smth9, bs.py:318-372 the stack): writes the
 * packed record [nlon+1][nlat][12] of one basic state (fp64, or fp32 when
 * fp32 != 0) -- the 11 hot fields bit-identical to BS.fields.
 *  d_u, d_v [nlat][nlon] float32 as read from the file (ascending latitude;
 *    the host flips a descending file like bs.py:251-256).
 *  d_trig[3][nlat]: np.cos(lat) (for u cos(lat)), then np.cos and np.sin of
 *    lat[1:-1] at indices 1..nlat-2 (host libm, the reference's values).
 *  dx, dy: BS.dx, BS.dy (bs.py:77-78).  d_scratch: 4*nlon*nlat doubles. */
rwrt_status rwrt_bs_ready(int32_t nlon, int32_t nlat, const float* d_u,
                          const float* d_v, const double* d_trig, double dx,
                          double dy, double* d_scratch, void* d_packed,
                          int32_t fp32, void* stream);

/* The basic-state diagnostics (ABI 5, additive): the 23 fields that BS.output
 * writes (bs.py:461-511) after BS.ready(xcyclic=True) (bs.py:318-407), for a
 * batch of nlev levels.  Plane ids, in BS.output's order (bs.py:481-505):
 *   0 u  1 v  2 q  3 ux  4 uxx  5 uy  6 vx  7 vxx  8 vy  9 qx  10 qy  11 qxx
 *   12 qxy  13 qyx  14 qyy  15 qxxx  16 qxxy  17 qxyy  18 qyyy  19 qyxx
 *   20 qyyx  21 betam  22 KS
 * Plane p of a level is bit for bit (NaN for NaN) the attribute of that name:
 * qxx, qxy, qyy after smth9, qyx the copy taken before it, the third
 * derivatives from the unsmoothed second derivatives.  On rows 1..nlat-2
 *   betam = ((2 Omega)(c c) + (((-c) uyy + s uy) + u / c) / R) / R
 *   KS    = sqrt((betam c) / u) R   where betam > 0 and u > 0, NaN elsewhere
 * with c, s = d_trig[1], d_trig[2], u the float32 value widened and uyy =
 * gradient_yy(u); rows 0 and nlat-1 of both are NaN.  Every operation is
 * + - * / sqrt in fp64 in NumPy's evaluation order.
 *  d_u, d_v [nlev][nlat][nlon] float32, file layout, ascending latitude;
 *    d_trig, dx, dy exactly rwrt_bs_ready's.
 *  select: bit p set = plane p is written.  d_out
 *    [nlev][popcount(select)][nlon][nlat], the selected planes in ascending id.
 *  d_scratch: needed only when select has a plane derived from q (ids 2,
 *    9..20): 4*nlon*nlat*scratch_levels doubles (rwrt_bs_ready's q, qxx, qyy,
 *    qxy of every level in flight); the call then works through the levels in
 *    groups of scratch_levels, one set of launches per group.  Without such a
 *    plane d_scratch may be NULL, scratch_levels is ignored and the call is one
 *    launch.  Results depend neither on scratch_levels nor on the batch a level
 *    is in; no atomics.
 * RWRT_ERR_ARG before any HIP call: nlon < 3, nlat < 4, nlev < 0, select == 0
 * or with bits >= RWRT_NDIAG, a NULL d_u, d_v, d_trig or d_out, scratch needed
 * but NULL or scratch_levels < 1, d_out (or the scratch) overlapping an input.
 * nlev == 0 is a no-op.  Asynchronous, ordered on stream; needs no rwrt_ctx. */
#define RWRT_NDIAG 23
rwrt_status rwrt_bs_diag(int32_t nlon, int32_t nlat, int32_t nlev,
                         const float* d_u, const float* d_v,
                         const double* d_trig, double dx, double dy,
                         uint32_t select, double* d_out, double* d_scratch,
                         int32_t scratch_levels, void* stream);

/* rwrt_rk45_init / rwrt_rk45_run on a time-varying background (same state,
 * queue and output conventions).  Steps reuse K6 = fun(t + h, y_new) as the
 * next f (FSAL, scipy's RK45 convention); the per-row group velocity is
 * evaluated at the row time t_bound. */
rwrt_status rwrt_rk45_init_tv(const rwrt_grid* g, const rwrt_background* b,
                              int64_t nray, const double* d_y0,
                              const rwrt_params* p, double* d_state,
                              int64_t* d_count, int32_t* d_nanrow,
                              int32_t* d_live, int64_t* d_summary, void* stream);
rwrt_status rwrt_rk45_run_tv(rwrt_ctx* ctx, const rwrt_grid* g, const rwrt_background* b,
                             int64_t nray, const rwrt_params* p,
                             const double* d_tbound, int32_t it_begin,
                             int32_t it_end, const int64_t* d_order,
                             int64_t n_heavy, double* d_state, int64_t* d_count,
                             int32_t* d_nanrow, double* d_out, int32_t* d_work,
                             void* stream);
/* n_heavy > 0 on a time-varying background (fp64 or fp32 levels; not with
 * fp32 arithmetic, fp32 == 2): the first n_heavy rays of d_order (at most 4
 * per CU on half the CUs) run one per wavefront, replicated on its 64 lanes,
 * their lookups served from an 8 x 8-point block of both bracketing levels in
 * the wave's LDS (reloaded by all 64 lanes at once) -- a schedule, results
 * are unchanged (ABI 3). */
/* rwrt_rk45_run_tv with constant row tails (as rwrt_rk45_run_tails). */
rwrt_status rwrt_rk45_run_tv_tails(rwrt_ctx* ctx, const rwrt_grid* g, const rwrt_background* b,
                                   int64_t nray, const rwrt_params* p,
                                   const double* d_tbound, int32_t it_begin,
                                   int32_t it_end, const int64_t* d_order,
                                   int64_t n_heavy, double* d_state, int64_t* d_count,
                                   int32_t* d_nanrow, double* d_out, int32_t* d_tail_from,
                                   double* d_tail_row, int32_t* d_work, void* stream);
/* rwrt_rk45_run_tv with row blocks for the live rays only (as rwrt_rk45_run_slots). */
rwrt_status rwrt_rk45_run_tv_slots(rwrt_ctx* ctx, const rwrt_grid* g, const rwrt_background* b,
                                   int64_t nray, const rwrt_params* p,
                                   const double* d_tbound, int32_t it_begin,
                                   int32_t it_end, const int64_t* d_order,
                                   int64_t n_heavy, double* d_state, int64_t* d_count,
                                   int32_t* d_nanrow, double* d_out, const int32_t* d_row_slot,
                                   int32_t* d_tail_from, double* d_tail_row, int32_t* d_work,
                                   void* stream);
/* The time-varying RHS at per-point times: d_t[n], d_y[5][n] -> d_dydt[5][n]. */
rwrt_status rwrt_rhs_tv(const rwrt_grid* g, const rwrt_background* b, int64_t n,
                        const double* d_t, const double* d_y, double* d_dydt,
                        void* stream);
/* Member stacks (additive members of ABI 5): rays through nmember STATIC basic
 * states on one grid in one launch -- forty winters, the members of an
 * ensemble, three pressure levels, one flow at several truncations.  Every
 * ray lives in one member for its whole life (d_member[ray]); nothing is
 * interpolated between members, and a ray's rows, counters and state are bit
 * for bit what rwrt_rk45_init / rwrt_rk45_run{,_tails,_slots} give for that
 * ray on that member alone, whatever the other rays, the queue order or the
 * chunking.
 *
 * Layout: d_packed[nmember][ncol][nrow][12] fp64, member m at d_packed +
 * m * member_stride doubles (16-byte aligned: member_stride even, at least
 * ncol*nrow*12) -- a levels stack whose t0 / dt are ignored.  d_member[nray]
 * (int32, device): 0 <= member < nmember is the caller's duty; the kernels
 * clamp the index wherever it addresses memory, so a bad one reads a wrong
 * member, never outside the stack.
 *
 * Limit: the ray loop keeps one cache image per member (6 KiB per 64 grid
 * points, rebuilt per call in the context's scratch) and addresses all of them
 * by 32-bit offsets from one base:
 *   nmember * ceil(ncol*nrow / 64) * 6 KiB + 8 KiB <= 2^32
 * (about 43 members at 0.25 degrees, thousands at 2.5 degrees); a larger
 * stack is RWRT_ERR_ARG.
 *
 * What stacks do not have: the latency mode (there is no n_heavy), the
 * drain-time hand-off (rwrt_ctx_set_handoff is ignored), the lean RHS tier
 * (every launch runs the full tier; the results are the same bits), fp32
 * member storage, time-varying members, RK4.
 *
 * The one run entry covers the three row layouts: d_row_slot, d_tail_from and
 * d_tail_row may be NULL under the rules of rwrt_rk45_run, _tails and _slots
 * (tails need both tail buffers; row slots need tails).  Every other argument
 * is as in rwrt_rk45_init / rwrt_rk45_run.  RWRT_ERR_ARG, with a message and
 * before any HIP call: a NULL grid or stack, nmember < 1, a member_stride too
 * small or odd, the limit above, NULL d_packed or d_member with nray > 0, and
 * every check of rwrt_rk45_run (NULL ctx, params, row window, buffers,
 * alignment, slots without tails). */
typedef struct {
  const double* d_packed;    /* [nmember][ncol][nrow][12] fp64 */
  int32_t nmember, reserved;
  int64_t member_stride;     /* doubles between two members, >= ncol*nrow*12 */
  const int32_t* d_member;   /* [nray]: 0 <= member < nmember, the caller's duty */
} rwrt_stack;                /* 32 bytes */
rwrt_status rwrt_rk45_init_stack(const rwrt_grid* g, const rwrt_stack* stack, int64_t nray,
                                 const double* d_y0, const rwrt_params* p, double* d_state,
                                 int64_t* d_count, int32_t* d_nanrow, int32_t* d_live,
                                 int64_t* d_summary, void* stream);
rwrt_status rwrt_rk45_run_stack(rwrt_ctx* ctx, const rwrt_grid* g, const rwrt_stack* stack,
                                int64_t nray, const rwrt_params* p, const double* d_tbound,
                                int32_t it_begin, int32_t it_end, const int64_t* d_order,
                                double* d_state, int64_t* d_count, int32_t* d_nanrow, double* d_out,
                                const int32_t* d_row_slot, int32_t* d_tail_from, double* d_tail_row,
                                int32_t* d_work, void* stream);
/* Release stacks (additive members of ABI 5): rays released at different
 * times into ONE time-varying background in one launch -- the same sources
 * every day of a season, or at the start, middle and end of a regime
 * transition.  The background is rwrt_background's (nlev fp64 levels at
 * t0 + j * dt); d_t0[ray] is that ray's own value of rwrt_background.t0, and
 * b->t0 is ignored.  A ray's time starts at 0 as in every time-varying call,
 * so a ray released r seconds after the first level has d_t0[ray] =
 * (time of the first level) - r, and its row i is its state i * tstep after
 * its release.  Past the last level the last level persists, before the first
 * the first.
 *
 * The level index and weight of an evaluation at ray time t are those of
 * rwrt_rk45_run_tv with t0 = d_t0[ray]: s = (t - d_t0[ray]) / dt and the same
 * clamps.  Nothing else differs, so a ray's rows, counters and state are bit
 * for bit what rwrt_rk45_init_tv / rwrt_rk45_run_tv{,_tails,_slots} of the
 * same build give for that ray alone with b->t0 = d_t0[ray], whatever the
 * other rays, the queue order, the row layout, the chunking or
 * rwrt_ctx_set_tv_lanes.
 *
 * What release stacks do not have: the latency mode (there is no n_heavy),
 * fp32 level storage and the fp32 RHS (b->fp32 must be 0), the backward
 * direction, RK4.
 *
 * The one run entry covers the three row layouts: d_row_slot, d_tail_from and
 * d_tail_row may be NULL under the rules of rwrt_rk45_run_stack.  Every other
 * argument is as in rwrt_rk45_init_tv / rwrt_rk45_run_tv_slots.  RWRT_ERR_ARG
 * before any HIP call, with a message that starts with the entry's name: a
 * NULL grid or background, nlev < 1, dt <= 0, b->fp32 != 0, NULL d_t0 with
 * nray > 0, RWRT_PARAMS_BACKWARD or any other flag bit; and, with the
 * messages they have there, every check of rwrt_rk45_run_tv_slots (NULL ctx,
 * params, levels, row window, buffers, alignment, slots without tails).
 * nray == 0 launches nothing. */
rwrt_status rwrt_rk45_init_rel(const rwrt_grid* g, const rwrt_background* b, const double* d_t0,
                               int64_t nray, const double* d_y0, const rwrt_params* p, double* d_state,
                               int64_t* d_count, int32_t* d_nanrow, int32_t* d_live, int64_t* d_summary,
                               void* stream);
rwrt_status rwrt_rk45_run_rel(rwrt_ctx* ctx, const rwrt_grid* g, const rwrt_background* b, const double* d_t0,
                              int64_t nray, const rwrt_params* p, const double* d_tbound, int32_t it_begin,
                              int32_t it_end, const int64_t* d_order, double* d_state, int64_t* d_count,
                              int32_t* d_nanrow, double* d_out, const int32_t* d_row_slot, int32_t* d_tail_from,
                              double* d_tail_row, int32_t* d_work, void* stream);
/* Stepper known-answer tests: the same device stepper on the analytic ODEs of
 * the rkf45.py demos (rkf45.py:839-882), driven like rk45_simple_current
 * (rkf45.py:672-724).  kind: 0 dx/dt = 2t, 1 dx/dt = e^(0.1 t), 2 Lorenz
 * (nvar 1, 1, 3).  d_y0[nvar][ncol]; d_teval[nt]; d_out[ncol][nt][nvar]. */
rwrt_status rwrt_kat_rk45(int32_t kind, int64_t ncol, const double* d_y0,
                          int32_t nt, const double* d_teval, double rtol,
                          double atol, double min_step, double* d_out,
                          void* stream);

/* Device math self-test: d_out[i] = f(d_x[i], d_y[i]) with the exact device
 * routines the kernels use.  kind: 0 sin(x), 1 cos(x), 2 tan(x), 3 pow(x, y),
 * 4 atan2(x, y), 5 Python x % y (fmod-based), 6 sqrt(x), 7 x / y, 8 floor(x),
 * 9/10 sin/cos through sincos(x), 11 x / 6.3712e6 (the kernels' exact division
 * by the earth radius), 12 fmod(x, y) for y > 0 (the kernels' exact fmod),
 * 13 x % (2 pi) and 14 (x % (2 pi)) % (2 pi) as the kernels evaluate them,
 * 15 x / y by a shared reciprocal, 16 np.floor(x).astype(int32),
 * (17-22: retired device-libm restatements), 23/24 x / y through the interleaved
 * division pair (as its first / second quotient), 25/26/27/28 the reference
 * NumPy's sin/cos/tan/power as restated in csrc/np_math.h, 29 the restated
 * VRCP14PD, 30/31/32 sin/cos/tan and 33 pow exactly as the kernels evaluate
 * them, 34 x / y by the RHS's shared-reciprocal division (qdiv), 35 1.0
 * where that division is inside its exact range (DivGuard), else 0.0, and
 * 36/37 the jump mask's verdict (wr.py:844-850; 1.0: a jump) for a step of
 * (dlat, dlon) = (x, y) from (lon, lat) = (1.0, 0.6) rad at cut_off 0.05 rad,
 * 36 with the kernels' polynomial "no jump" shortcut, 37 without it
 * (38/39: unassigned, refused), 40 the lean RHS tail's leaf guard: 1.0 where
 * the value x is admitted as leaf y (0 lons - lon0, 1 lat - lat0, 2 lat, 3 k,
 * 4 l, 5 amp; the other leaves physical), else 0.0, 41 the shared reciprocal
 * rcp2(x) itself, 42 the literal the kernels hold for rcp2(6.3712e6) and
 * 43 1.0 where a packed background value x is inside the lean tier's window
 * (0, or finite with an admitted exponent), else 0.0.
 * Lets the tests prove which operations are bit-exact on the GPU (IEEE
 * division, sqrt, fmod) and measure the last-bit agreement of the rest. */
rwrt_status rwrt_selftest_math(int32_t kind, int64_t n, const double* d_x,
                               const double* d_y, double* d_out, void* stream);

/* HOST routine (no device call; the drop-in's delivery into the reference
 * arrays, wr.py:868-876): rows [0, nrows) of a host block dst[nrows][ncol]
 * (row stride ld doubles) become prev[ncol] -- the row before the block --
 * except the nsrc columns cols[] (strictly ascending, < ncol), which take
 * src[nrows][nsrc] (row stride ld_src).  A ray whose rows in a launch are all
 * bitwise equal to its previous row (a frozen ray: rkf45.py:400-403) is then
 * never shipped over PCIe; the block equals what a full copy would give, bit
 * for bit.  Reentrant (callers split the rows over threads). */
rwrt_status rwrt_host_fill_rows(double* dst, int64_t nrows, int64_t ncol, int64_t ld,
                                const double* prev, const double* src, int64_t nsrc,
                                int64_t ld_src, const int64_t* cols);

#ifdef __cplusplus
}
#endif

#endif /* RWRT_H */
