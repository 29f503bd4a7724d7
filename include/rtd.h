/*
 * rtd.h -- C ABI of the MI355X discrete-ordinate radiative-transfer engine (librtd.so).
 *
 * This is the drop-in boundary for the hot path of LDEO-CREW/Pythonic-DISORT:
 *
 *   _assemble_intensity_and_fluxes   src/PythonicDISORT/_assemble_intensity_and_fluxes.py:8-32
 *     -> _solve_for_gen_and_part_sols   src/PythonicDISORT/_solve_for_gen_and_part_sols.py:5-16
 *     -> _solve_for_coeffs              src/PythonicDISORT/_solve_for_coeffs.py:8-29
 *     -> closures u / u0 / flux_up / flux_down   _assemble_intensity_and_fluxes.py:170,334,446,527
 *
 * The reference has no FFI of its own (it is pure Python over NumPy/SciPy); the entry points
 * below are what a ctypes binding of that path binds.  They take the *prepared* arguments of
 * `_assemble_intensity_and_fluxes` (delta-M scaled, source-rescaled; pydisort.py:184-372), with a
 * leading column axis C added to every per-atmosphere array so that many independent
 * atmospheric columns are solved in one call.  C = 1 reproduces one `pydisort()` call.
 *
 * Conventions: plain C, all arrays contiguous row-major float64, caller-allocated HOST memory
 * unless a name says "dev"; sizes are int32; every function returns 0 on success or a nonzero
 * status (rtd_last_error() gives the text).  No exceptions cross the boundary.  A plan owns its
 * device buffers and one HIP stream; plans are independent and may be used from different host
 * threads (one thread per plan).
 */
#ifndef RTD_H
#define RTD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtd_plan rtd_plan; /* opaque */

typedef struct {
  int32_t ncols;    /* C : independent atmospheric columns                                  */
  int32_t nlayers;  /* NLayers                                                              */
  int32_t nquad;    /* NQuad (streams, even, 2 ... 128; N = NQuad/2 per hemisphere)         */
  int32_t nleg;     /* NLeg  (phase-function moments used, <= NQuad)                        */
  int32_t nfourier; /* NFourier (1 when only fluxes are wanted)                             */
  int32_t nscoeffs; /* Nscoeffs: polynomial order+1 of the isotropic source (0 = none)      */
  int32_t nbdrf;    /* NBDRF: number of tabulated BDRF Fourier modes (0 = black surface)    */
  int32_t beam;     /* there_is_beam_source (any I0 > 0)                                    */
} rtd_dims;

/* --- library / device ------------------------------------------------------------------- */
int rtd_version(void);
const char* rtd_last_error(void);
int rtd_device_count(int32_t* count);
/* free and total memory of a device right now (hipMemGetInfo; either pointer may be NULL): what a caller sizes a retention
 * budget or a pool limit against */
int rtd_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes);

/* --- plan life cycle ---------------------------------------------------------------------- */
/* Allocates every device buffer the path needs for `dims` on HIP device `device`.
 * Inputs and results are held for all `ncols` columns; the intermediates of the solve (eigenvector blocks, BC workspace:
 * ~8 MB per 20-layer 32-stream column) are held for one *window* of columns at a time and the kernels run window after
 * window on the plan's stream, so ncols is bounded by the inputs and results only (10^5 columns of BASELINE.json's
 * configs[3] need 2.3 GB).  rtd_plan_create sizes the window itself (environment RTD_WORK_BYTES, default 24 GiB of
 * intermediates); rtd_plan_create_windowed takes it from the caller (work_columns <= 0: automatic).
 * A plan of more than one window pipelines them: it keeps the eigen stage's hand-off buffers twice and runs the eigen
 * stage of window w + 1 on a second HIP stream beside the boundary-condition and evaluation stage of window w (events
 * order the two; RTD_NO_PIPELINE=1 in the environment runs the windows one after the other).  Nothing of this is visible
 * at the ABI: every call below is ordered on the plan's stream as before, rtd_plan_synchronize covers both. */
int rtd_plan_create(const rtd_dims* dims, int32_t device, rtd_plan** plan);
int rtd_plan_create_windowed(const rtd_dims* dims, int32_t device, int32_t work_columns, rtd_plan** plan);
/* A plan whose evaluators can be called again after a solve WITHOUT solving again, whatever its window count -- the contract
 * of the reference's closures, which keep GC_collect, K_collect, B_collect of the solve and evaluate any (tau, phi) from them
 * (_assemble_intensity_and_fluxes.py:170-262).  Everything rtd_plan_evaluate / rtd_plan_get_tensors read of a solve (the
 * eigenvector blocks Y, A, the eigenvalues, particular solutions and boundary-condition coefficients: 3.1 of the 8.4 MB of
 * intermediates of a 20-layer 32-stream column) is then held for ALL columns; only the boundary-condition workspace stays
 * windowed.  retain_bytes: budget for that state in bytes; < 0: three tenths of the device memory that is free at creation;
 * 0: never (= rtd_plan_create_windowed).
 * A batch whose full state does not fit the budget is created in the LEAN retained form when that fits (10 streams and up): only
 * what cannot be recomputed cheaply is held for all columns -- the boundary-condition coefficients, k, E = exp(-k dtau), the beam
 * and thermal particular solutions: 0.5 MB per 20-layer 32-stream column, 50 GB for BASELINE's 10^5-column batch -- and
 * rtd_plan_evaluate re-runs the EIGEN stage (never the boundary-condition solve) for the layers its points touch, window by window,
 * in the wavefront composition the solve had them in: results bit-identical to the full form; an evaluation at one depth per column
 * costs about a tenth of a solve.  Else the plan is a plain windowed one, whose rtd_plan_evaluate solves the windows again.
 * rtd_plan_retained tells which it is: 1 full (one-window plans: always), 2 lean, 0 neither.
 * rtd_plan_create_retained_form: form 0 = as above (full, else lean, else neither), 1 = full or neither, 2 = lean or neither. */
int rtd_plan_create_retained(const rtd_dims* dims, int32_t device, int32_t work_columns, int64_t retain_bytes, rtd_plan** plan);
int rtd_plan_create_retained_form(const rtd_dims* dims, int32_t device, int32_t work_columns, int64_t retain_bytes, int32_t form,
                                  rtd_plan** plan);
int rtd_plan_retained(rtd_plan* plan, int32_t* retained);
/* columns per window and number of windows of a plan */
int rtd_plan_windows(rtd_plan* plan, int32_t* work_columns, int32_t* nwindows);
int rtd_plan_destroy(rtd_plan* plan);
int rtd_plan_synchronize(rtd_plan* plan);
/* bytes of device memory held by the plan */
int rtd_plan_device_bytes(rtd_plan* plan, int64_t* bytes);
/* Device memory of destroyed plans.  Small arenas (blocks up to 64 MB, 512 MB in all) are always kept for the next plan of about
 * the same size: one-column calls create and destroy a plan per call.  LARGE blocks are kept only when the caller asks for it --
 * rtd_pool_set_limit, or RTD_POOL_BYTES in the environment; the default limit is 0: a library imported under someone else's
 * process must not sit on gigabytes of a GPU it shares with that process's allocator.  With a limit (bytes PER DEVICE; < 0: an
 * eighth of that device's memory; oldest blocks of the same device out first), creating and destroying a plan of gigabytes per call
 * costs neither hipMalloc nor the seconds-long stalls the runtime's lazy reclaim of freed gigabytes puts on later allocations
 * (profiles/r05_alloc_outliers.txt: 4 of 40 creations of a 14 GB plan stalled for 1.8 ... 4.7 s without, none with) -- a serving
 * loop opts in once.  No counterpart in the reference (NumPy's allocator).
 * rtd_pool_set_limit: the new limit (previous may be NULL; lowering it frees what no longer fits); rtd_pool_bytes: what is held
 * right now; rtd_pool_trim: give it back to the runtime (device -1: every device; released may be NULL).  An allocation of the
 * library that fails with out-of-memory trims the pool and is tried again by itself. */
int rtd_pool_set_limit(int64_t bytes, int32_t device, int64_t* previous);
int rtd_pool_bytes(int64_t* cached);
int rtd_pool_trim(int32_t device, int64_t* released);
/* Which columns of the batch failed numerically in the last solve: status[ncols], 0 = fine.  Bits 1..4 of the low byte:
 * 2 eigen-iteration not converged, 4 non-positive Cholesky pivot / non-finite eigenvalue, 8 singular boundary-condition
 * system, 16 non-finite beam particular solution -- raised by Fourier mode 0; the same bits shifted left by 8: raised by
 * a mode m > 0 (the fluxes and u0 of such a column are still valid: they come from mode 0; the reference returns NaN
 * intensities and valid fluxes there, _solve_for_gen_and_part_sols.py:186).  A column's failure does not touch the other
 * columns' results; rtd_plan_fetch / _evaluate report RTD_ERR_NUMERIC when any column they return has failed. */
int rtd_plan_get_column_status(rtd_plan* plan, int32_t* status);

/* --- inputs (host -> device) -------------------------------------------------------------- */
/* Quadrature of one hemisphere: mu_arr_pos[N], W[N]  (pydisort.py:304-306). */
int rtd_plan_set_quadrature(rtd_plan* plan, const double* mu_pos, const double* weights);

/* Per-column prepared arguments of _assemble_intensity_and_fluxes (_assemble.py:8-32):
 *   scaled_omega      [C][L]        scaled_omega_arr
 *   tau               [C][L]        tau_arr (unscaled lower boundaries, for layer lookup)
 *   scaled_tau_with_0 [C][L+1]      scaled_tau_arr_with_0
 *   scale_tau         [C][L]        scale_tau
 *   wleg              [C][L][NLeg]  weighted_scaled_Leg_coeffs
 *   mu0, I0, phi0, rescale [C]      beam parameters (I0 already divided by rescale_factor)
 *   b_pos, b_neg      [C][M][N]     Dirichlet BCs per Fourier mode (NULL = 0); _coeffs.py:142-158
 *   s_poly            [C][L][Ns]    scaled_s_poly_coeffs (NULL when Ns = 0)
 *   bdrf_q            [C][NBDRF][N][N]  q^m(mu_i, mu_j)     } BDRF_Fourier_modes evaluated on the
 *   bdrf_q0           [C][NBDRF][N]     q^m(mu_i, mu0)      } quadrature grid; _coeffs.py:121-134
 */
int rtd_plan_set_columns(rtd_plan* plan, const double* scaled_omega, const double* tau,
                         const double* scaled_tau_with_0, const double* scale_tau, const double* wleg,
                         const double* mu0, const double* I0, const double* phi0, const double* rescale,
                         const double* b_pos, const double* b_neg, const double* s_poly,
                         const double* bdrf_q, const double* bdrf_q0);

/* Thermal source polynomials about the top of their own layer, on the host (no device, no plan).  s_poly [C][L][Ns] are the
 * user's s_poly_coeffs -- coefficients in the ABSOLUTE, UNSCALED optical depth -- and tau_arr, omega_arr, f_arr [C][L] as
 * pydisort()'s arguments; s_local [C][L][Ns] receives, per layer, the coefficients in x = scale_tau (tau - top of the layer),
 * times (1 - omega) / scale_tau, NOT yet divided by the rescale factor: what rtd_plan_set_columns_raw forms on the device, by the
 * same routine (csrc/rtd_dd.h: one double-double Taylor shift).  The float64 coefficients in the absolute SCALED depth that
 * rtd_plan_set_columns takes cannot hold a deep polynomial of degree >= 5 (the substitution alone loses 1e-8 of the source at
 * degree 9 and optical depth 90); a front end that has the user's polynomials goes this way and through
 * rtd_plan_set_columns_local, which is rtd_plan_set_columns except that its polynomials ARE in this local form (divided by
 * rescale) and are uploaded as given. */
int rtd_source_polynomials_local(int64_t ncolumns, int32_t nlayers, int32_t nscoeffs, const double* tau_arr,
                                 const double* omega_arr, const double* f_arr, const double* s_poly, double* s_local);
int rtd_plan_set_columns_local(rtd_plan* plan, const double* scaled_omega, const double* tau,
                               const double* scaled_tau_with_0, const double* scale_tau, const double* wleg,
                               const double* mu0, const double* I0, const double* phi0, const double* rescale,
                               const double* b_pos, const double* b_neg, const double* s_local,
                               const double* bdrf_q, const double* bdrf_q0);

/* The same batch from RAW inputs: the preparation of pydisort.py:316-372 (delta-M scaling of tau, omega and the moments,
 * the thermal source polynomial in the scaled optical depth, the rescaling of every source by the largest one) runs on
 * the device.  For throughput batches: the host hands over what the user gave, nothing is computed per column on the CPU.
 *   tau_arr, omega_arr, f_arr [C][L]   as pydisort()'s arguments (f_arr = 0: no delta-M scaling)
 *   leg_all   [C][L][nleg_all]         Leg_coeffs_all (nleg_all >= nleg; the first nleg moments are used)
 *   mu0, I0, phi0 [C]                  I0 NOT rescaled
 *   b_pos, b_neg  [C][M][N]            Dirichlet BCs per Fourier mode, NOT rescaled (NULL = 0)
 *   s_poly    [C][L][Ns]               s_poly_coeffs as given by the user (NULL when Ns = 0)
 *   bdrf_q, bdrf_q0                    as in rtd_plan_set_columns */
int rtd_plan_set_columns_raw(rtd_plan* plan, const double* tau_arr, const double* omega_arr, const double* leg_all,
                             int32_t nleg_all, const double* f_arr, const double* mu0, const double* I0,
                             const double* phi0, const double* b_pos, const double* b_neg, const double* s_poly,
                             const double* bdrf_q, const double* bdrf_q0);

/* Thermal sources from temperatures, integrated on the device.  DISORT describes a thermal problem by TEMPER, BTEMP, TTEMP,
 * TEMIS and the band WVNMLO ... WVNMHI; the reference turns them into s_poly_coeffs, b_pos and b_neg on the host with
 * generate_s_poly_coeffs, blackbody_contrib_to_BCs and generate_emissivity_from_BDRF (subroutines.py:413-454, :354-377,
 * :459-486; SciPy quadrature of the Planck function).  Here one device thread integrates one (temperature, band) in closed
 * form (csrc/rtd_planck.h: Gauss-Legendre panels of x^3 / (e^x - 1), float64 accurate from the Rayleigh-Jeans end to the Wien
 * tail); E(T) below is that integral in W / m^2, with the reference's formula and units (subroutines.py:322-350).
 *
 * The plan-free form: out[i] = E(T[i]) over wvnmlo[i] ... wvnmhi[i] (cm^-1), i < n; host arrays in, host array out,
 * synchronous.  T = 0 and wvnmlo = wvnmhi give 0. */
int rtd_planck_band(int32_t device, int64_t n, const double* T, const double* wvnmlo, const double* wvnmhi, double* out);

/* The thermal description of a batch (host arrays):
 *   temper   [C][L+1]   level temperatures, top first (TEMPER)
 *   wvnmlo, wvnmhi [C]  the band of each column
 *   btemp, ttemp [C]    temperatures of the bottom and top boundaries; NULL: that boundary does not emit
 *   temis    [C]        emissivity of the top boundary; NULL: 1
 *   emissivity [C][N]   directional emissivity of the surface; NULL: Kirchhoff's law on the zeroth BDRF mode of the plan,
 *                       1 - 2 sum_j q^0(mu_i, mu_j) mu_j w_j  (1 when nbdrf = 0) */
typedef struct {
  const double *temper, *wvnmlo, *wvnmhi, *btemp, *ttemp, *temis, *emissivity;
} rtd_thermal;

/* rtd_plan_set_columns_raw with the isotropic source formed on the device from `th` instead of given as s_poly; the plan must
 * have nscoeffs = 2.  Per column: the level emissions E(temper[l]); the source polynomial of layer l = (intercept, slope) of
 * the line through (tau_{l-1}, E_l), (tau_l, E_{l+1}) in the unscaled optical depth (linear_spline_coefficients,
 * subroutines.py:381-409), which the device preparation then treats as a user-given s_poly;
 *   b_pos[c][0][i] += emissivity[c][i] E(btemp[c]),   b_neg[c][0][i] += temis[c] E(ttemp[c])
 * on top of what the caller passed (NULL = 0).  With emissivity = NULL and nbdrf > 0 the quadrature must have been set, and
 * bdrf_q must be the final table (not with rtd_plan_set_bdrf_samples, which forms it later).  Everything else as in
 * rtd_plan_set_columns_raw. */
int rtd_plan_set_columns_thermal(rtd_plan* plan, const double* tau_arr, const double* omega_arr, const double* leg_all,
                                 int32_t nleg_all, const double* f_arr, const double* mu0, const double* I0,
                                 const double* phi0, const double* b_pos, const double* b_neg, const double* bdrf_q,
                                 const double* bdrf_q0, const rtd_thermal* th);

/* k-distribution bands: the optical properties of P profiles x G spectral points mixed on the device.  Within a band (the
 * g-points of a correlated-k band, the wavelengths of an instrument channel) every column of a profile shares its scatterers,
 * its geometry and its surface; only the gas absorption per layer and the solar weight change from point to point.  The caller
 * states the band as it has it -- G + 2 S doubles per profile and layer instead of the 3 + nleg per column and layer of
 * rtd_plan_set_columns_raw -- and the device forms tau_arr, omega_arr, f_arr and the moments of every column c = p G + g:
 *   sca   = sum_s omega_spec[p][l][s] dtau_spec[p][l][s]
 *   dtau  = sum_s dtau_spec[p][l][s] + dtau_abs[p][g][l]
 *   tau_arr[c][l] = dtau[c][0] + ... + dtau[c][l],   omega_arr[c][l] = sca / dtau
 *   leg_all[c][l][k] = sum_s omega_spec dtau_spec leg_spec[s][k] / sca  (k >= 1; 1 for k = 0),   k < nleg
 *   f_arr[c][l] = the same expression at k = nleg when delta_m is set (needs nleg_all > nleg), else 0
 * with s and l ascending and one thread per output element: the bits do not depend on the launch geometry.  A layer without a
 * scatterer (sca = 0) gets the moments (1, 0, ...) and f = 0.  The mixed leg_all has nleg moments per layer ([C][L][nleg]): those
 * the solver uses. */
typedef struct {
  int32_t nprofiles, ngpoints, nspecies, nleg_all, delta_m;
  const double *dtau_abs;   /* [P][G][L] absorption optical thickness of each layer at each spectral point (>= 0) */
  const double *dtau_spec;  /* [P][L][S] extinction optical thickness of each species in each layer (>= 0)        */
  const double *omega_spec; /* [P][L][S] single-scattering albedo of each species (0 ... 1)                       */
  const double *leg_spec;   /* [S][nleg_all] Legendre coefficients of each species' phase function, [s][0] = 1    */
} rtd_band;

/* The plan-free form, like rtd_planck_band: host arrays in, the four mixed arrays out (tau_arr, omega_arr, f_arr [P G][L],
 * leg_all [P G][L][nleg]), synchronous.  RTD_ERR_ARG for a null pointer, P, G, S or nlayers < 1, nleg < 1, or
 * nleg_all < nleg + (delta_m ? 1 : 0). */
int rtd_band_mix(int32_t device, int32_t nlayers, int32_t nleg, const rtd_band* band, double* tau_arr, double* omega_arr,
                 double* f_arr, double* leg_all);

/* rtd_plan_set_columns_raw with tau_arr, omega_arr, f_arr and leg_all formed on the device from `band`; the plan must have
 * ncols = P G.  mu0, I0, phi0 [C] and the boundary and BDRF arrays as there (per column).  th may be NULL; given, the isotropic
 * source is formed as by rtd_plan_set_columns_thermal (plan with nscoeffs = 2, else no isotropic source: nscoeffs = 0) -- its
 * slopes use the mixed tau.  tau_out [C][L] (may be NULL) receives the mixed tau_arr as the device formed it: the optical depths
 * of the levels, which the caller needs to name an evaluation point.  Not combined with rtd_plan_set_mode_shard or a
 * communicator (RTD_ERR_STATE). */
int rtd_plan_set_columns_band(rtd_plan* plan, const rtd_band* band, const double* mu0, const double* I0, const double* phi0,
                              const double* b_pos, const double* b_neg, const double* bdrf_q, const double* bdrf_q0,
                              const rtd_thermal* th, double* tau_out);

/* BDRF Fourier modes formed on the device.  The reference takes the surface as callables
 * BDRF_Fourier_modes[m](mu, -mu') evaluated on the quadrature grid (_solve_for_coeffs.py:121-134); for a reflectance
 * rho(mu, mu', dphi) its tests integrate every mode on the host (pydisotest/6_test.py:194-201).  Here the caller passes
 * rho sampled at dphi_p = 2 pi p / nphi, p < nphi, and the device forms the plan's NBDRF modes
 *   q^m = (2 - delta_m0)/nphi  sum_p rho_p cos(m dphi_p)      (trapezoid rule of 1/((1+delta_m0) pi) Int rho cos(m dphi))
 *   rho_qq [C][N][N][nphi]   rho(mu_i, mu_j, dphi_p)
 *   rho_q0 [C][N][nphi]      rho(mu_i, mu0, dphi_p)   (NULL when there is no beam)
 * Call after rtd_plan_set_columns (whose bdrf_q / bdrf_q0 may then be NULL) and before rtd_plan_solve. */
int rtd_plan_set_bdrf_samples(rtd_plan* plan, int32_t nphi, const double* rho_qq, const double* rho_q0);

/* Parametric surface models: the samples themselves formed on the device, from the three or four numbers per pixel a land or ocean
 * retrieval holds (csrc/rtd_surface.h has the formulas and their conditioning).  rho(mu, mu', dphi): mu the REFLECTED cosine, mu'
 * the INCIDENT one, both in (0, 1]; dphi the difference of the PROPAGATION azimuths, as the reference's BDRF callables take it
 * (pydisotest/6_test.py:11-24): backscatter -- the hot spot -- is at dphi = pi.  params is [rows][4], unused entries 0:
 *   RTD_SURFACE_LAMBERT  albedo in [0, 1]                    no sampling: q^0 = albedo, q^m = 0 for m > 0 (nphi is only range-checked)
 *   RTD_SURFACE_HAPKE    B0 >= 0, HH > 0, 0 < W <= 1         Hapke's soil as in DISORT's test problem 6
 *   RTD_SURFACE_ROSSLI   f_iso, f_vol, f_geo >= 0            Ross-Thick / Li-Sparse-Reciprocal (h/b = 2, b/r = 1), CLAMPED at 0: the
 *                                                            kernels are unbounded below at grazing angles (rho = -1.8 at the smallest
 *                                                            node of 16 streams for the weights 0.3, 0.1, 0.05) and a negative
 *                                                            reflectance is not a surface
 *   RTD_SURFACE_RPV      rho0 >= 0, k > 0, |Theta| < 1, rho_c  Rahman-Pinty-Verstraete; Theta < 0 is backscattering
 *   RTD_SURFACE_OCEAN    U >= 0, n > 1, rho_w >= 0           the wind-roughened ocean, Cox-Munk glint with isotropic slopes: wind speed U in
 *                                                            m/s (sigma^2 = 0.003 + 0.00512 U), real refractive index n (unpolarized
 *                                                            Fresnel), rho_w a Lambertian addition for underlight and foam.  The glint
 *                                                            is at dphi = 0.  Shadowing (S = 1 / (1 + L(mu) + L(mu'))) is ALWAYS ON:
 *                                                            without it the albedo at the smallest node exceeds 1 from 16 streams
 *                                                            upward (4.8 at 34 streams, U = 5 m/s); with it the worst is 0.74
 * every parameter finite.  All five are reciprocal and even in dphi: the cosine series of rtd_plan_set_bdrf_samples is complete.
 * rows: 1 (one surface for all columns), C (one per column) or -- for rtd_plan_set_columns_band -- P (one per profile).
 * The ocean does not take the uniform-grid route of the other models in a plan: the glint's azimuthal width at a grazing pair of 34
 * or 64 streams is 1e-3 rad.  rtd_surface_ocean_kernel forms its modes in one pass per pair of cosines on the clustered periodic grid
 * dphi = psi - a sin psi, psi_p = 2 pi p / nphi, weights (1 - a cos psi_p) / nphi, a per pair (csrc/rtd_surface.h defines it), straight
 * into the tables: no samples in memory, no scratch block, no chunk, no RTD_SURFACE_BYTES.  For this model nphi is the number of
 * psi nodes: even, >= 4 NBDRF (Nyquist on the coarsest spacing), <= 16384; 512 leaves <= 1.7e-9 of a pair's largest mode at 64
 * streams (profiles/surface_ocean.json).  rtd_surface_samples keeps its uniform dphi grid for every model. */
enum { RTD_SURFACE_LAMBERT = 0, RTD_SURFACE_HAPKE = 1, RTD_SURFACE_ROSSLI = 2, RTD_SURFACE_RPV = 3, RTD_SURFACE_OCEAN = 4 };
typedef struct { int32_t model, nphi, rows; const double* params; } rtd_surface;

/* Sticky, in the manner of rtd_plan_request_nt; the parameters are copied.  NULL or model < 0 withdraws the request.  RTD_ERR_ARG
 * for a plan with nbdrf = 0, for inadmissible parameters (the message names the first bad row), or unless
 * 2 (NBDRF - 1) < nphi <= 16384 (RTD_SURFACE_OCEAN: nphi even and 4 NBDRF <= nphi <= 16384).  While a request is set, rtd_plan_set_columns_raw, _thermal and _band form bdrf_q and bdrf_q0 on the
 * device where they otherwise upload them -- AHEAD of the thermal kernels, so Kirchhoff's law with emissivity = NULL reads the
 * device-formed zeroth mode -- by rtd_surface_samples_kernel, one thread per sample at dphi_p = 2 pi p / nphi with mu' the nodes and
 * the column's raw mu0, and rtd_bdrf_modes_kernel, in chunks of columns whose samples fit a scratch block from the pool (RTD_SURFACE_BYTES,
 * default 256 MiB; one column at least); the tables do not depend on the chunk size.  Those calls then take bdrf_q = bdrf_q0 = NULL
 * (a table: RTD_ERR_ARG), return RTD_ERR_STATE before rtd_plan_set_quadrature, RTD_ERR_ARG when rows fits neither 1, C nor (a band) P
 * or when a plan with a beam meets a mu0 outside (0, 1]; a plan without a beam skips the mu0 column (bdrf_q0 stays 0).  The
 * host-prepared rtd_plan_set_columns / _local return RTD_ERR_STATE while a request is set.  A later rtd_plan_set_bdrf_samples still
 * overwrites the tables.  A plan that never requests allocates and launches nothing for this. */
int rtd_plan_request_surface(rtd_plan* plan, const rtd_surface* surface);
/* The plan-free form, like rtd_planck_band: rho[r][p] = rho(mu[r], mup[r], 2 pi p / nphi) with params[r][4], r < n, by the kernel
 * the plans use (the same bits); host arrays in, host array out, synchronous.  RTD_ERR_ARG for an unknown model, inadmissible
 * parameters, a cosine outside (0, 1] or nphi outside 1 ... 16384. */
int rtd_surface_samples(int32_t device, int32_t model, int64_t n, const double* params, const double* mu, const double* mup,
                        int32_t nphi, double* rho);
/* Diagnostic, in the spirit of rtd_plan_get_nt: the BDRF tables as the plan holds them, uploaded or device-formed, unpadded:
 * q [C][NBDRF][N][N], q0 [C][NBDRF][N]; either pointer may be NULL.  RTD_ERR_STATE before the columns.  Synchronous. */
int rtd_plan_get_bdrf(rtd_plan* plan, double* q, double* q0);

/* Fourier-mode shard (the partition for fewer columns than GPUs): the plan's nfourier local modes
 * stand for the modes first, first + stride, ... of `total` (the reference's NFourier; modes are independent through
 * the eigen stage and the boundary-condition solve, _gen_part.py:91, _coeffs.py:111, and meet only in the Fourier sum,
 * _assemble.py:256-260).  b_pos / b_neg of rtd_plan_set_columns are then those of the local modes.  The evaluators
 * return the shard's partial sums (u0, fluxes and the thermal terms from the shard that owns mode 0 only); summing the
 * shards gives the full result: rtd_comm_allreduce_results.  Default: first 0, stride 1, total = nfourier. */
int rtd_plan_set_mode_shard(rtd_plan* plan, int32_t first, int32_t stride, int32_t total);

/* Declares the uploaded inputs NEW without uploading them again: the next solve recomputes everything that depends on
 * them -- the per-column associated-Legendre tables at -mu0 and the beam attenuations, which a plan otherwise keeps from run
 * to run while its inputs are unchanged (the reference recomputes them in every call, _solve_for_gen_and_part_sols.py:96-109)
 * -- and starts behind everything queued on the plan's stream, as after rtd_plan_set_columns.  For measurements of the
 * fresh-input rate with inputs resident in HBM (bench.py: `value`; repeated inputs: `value_cached_tables`). */
int rtd_plan_invalidate_tables(rtd_plan* plan);

/* --- solve: _solve_for_gen_and_part_sols + _solve_for_coeffs on the device ---------------- */
/* Asynchronous on the plan's stream. */
int rtd_plan_solve(rtd_plan* plan);

/* --- evaluators: the closures of _assemble_intensity_and_fluxes --------------------------- */
/* tau: [C][ntau] optical depths (0 <= tau <= tau_arr[-1]); phi: [nphi].
 * u      [C][NQuad][ntau][nphi]   (axes mu, tau, phi as the reference's u(tau, phi))
 * u0     [C][NQuad][ntau]
 * fluxes [C][ntau]: flux_up, flux_down diffuse, flux_down direct
 * ulast  [C][NQuad][ntau]: last Fourier mode u^{M-1} (for return_Fourier_error), may be NULL
 * antiderivative bit 0 switches every output to the tau-antiderivative (is_antiderivative_wrt_tau);
 * bit 1 evaluates u without the Nakajima-Tanaka corrections even when rtd_plan_set_nt is active;
 * bit 2 (value 4) switches every output -- u with its Nakajima-Tanaka corrections, u0, ulast and the three fluxes -- to its
 * derivative with respect to tau, the caller's UNSCALED optical depth (inside layer l the delta-M scaled depth moves at
 * d tau* / d tau = scale_tau[l]).  The solution is closed-form per layer, so this is exact and costs what a value costs; the
 * reference leaves it to the autograd package (pydisort(..., autograd_compatible=True)).  The layer of a point is found as for
 * the values, argmax(tau <= tau_arr): at an interface tau = tau_arr[l] the result is the one-sided derivative from ABOVE, i.e.
 * of layer l, which ends there; at tau = 0 it is the right derivative.  Derivatives are generally discontinuous across
 * interfaces.  d(flux_down_direct)/d tau = -flux_down_direct / mu0.  Bits 0 and 2 together: RTD_ERR_ARG.
 * Bit 3 (value 8) forms u on the device although the u pointer is NULL (nothing of it is copied): for rtd_plan_fetch_view behind
 * the call.  rtd_plan_evaluate_band reads the same bit.
 * Any output pointer may be NULL.  Synchronous (returns when the host arrays are filled).
 * Returns RTD_ERR_TAU_RANGE if some tau lies outside its column (the reference raises ValueError). */
int rtd_plan_evaluate(rtd_plan* plan, int32_t ntau, const double* tau, int32_t nphi, const double* phi,
                      int32_t antiderivative, double* u, double* u0, double* flux_up,
                      double* flux_down_diffuse, double* flux_down_direct, double* ulast);

/* Nakajima-Tanaka intensity corrections (TMS + IMS; reference pydisort.py:375-698), applied on the device to the
 * `u` output of rtd_plan_evaluate once set (the reference returns u_corrected in place of u).
 *   weighted_leg_all [C][L][nleg_all]  (2l+1) g_l of the FULL phase function (weighted_Leg_coeffs_all)
 *   f_arr            [C][L]            delta-M truncation fractions
 *   ims_coef         [C][nleg_all]     (2l+1)(2 g~_l - g~_l^2), g~ the tau-omega weighted residual moments (:601-611)
 *   ims_par          [C][2]            scaled_mu0 = mu0/(1 - omega_avg f_avg), amplitude I0/(4pi) (omega_avg f_avg)^2/(1 - omega_avg f_avg)
 * nleg_all <= 0 switches the corrections off. */
int rtd_plan_set_nt(rtd_plan* plan, int32_t nleg_all, const double* weighted_leg_all, const double* f_arr,
                    const double* ims_coef, const double* ims_par);
/* The same four inputs formed ON THE DEVICE, for the plans whose columns arrive unprepared: while nleg_all > 0 is requested (sticky;
 * 0 withdraws the request), rtd_plan_set_columns_raw, _thermal and _band also form weighted_leg_all, ims_coef and ims_par from the
 * arrays they stage (arithmetic of csrc/rtd_nt_prep.h), keep f_arr, and switch the corrections on.
 *   raw columns: nleg_all must equal the nleg_all passed there and exceed nleg; weighted_leg_all is [C][L][nleg_all].
 *   a band:      nleg_all must equal band->nleg_all (> nleg) and band->delta_m must be set.  The mixture's moments do not depend
 *                on the spectral point: weighted_leg_all is [P][L][nleg_all], one row per profile shared by its G columns, formed
 *                by the expression behind rtd_band_mix's moments (the same bits); only the IMS constants are per column.
 *   otherwise RTD_ERR_ARG from those calls; likewise for a plan without a beam, as rtd_plan_set_nt.
 * The IMS weights are omega_l tau_arr[l] with the CUMULATIVE tau_arr, the reference's convention (:601-610); I0 in the amplitude
 * is the plan's rescaled beam.  Each column's sums run over l ascending in one chain per moment (one wavefront per column, lanes
 * over the moments, no atomics, no cross-lane reduction): the bits depend on the inputs alone.  A column with
 * sum_l f_l omega_l tau_arr[l] = 0 gets ims_coef = 0, amplitude 0 and scaled_mu0 = mu0 -- its IMS term is exactly 0, where the
 * formulas (and the host-prepared path) give 0 / 0.
 * While a request is set the host-prepared rtd_plan_set_columns returns RTD_ERR_STATE.  rtd_plan_set_nt(nleg_all <= 0) still
 * switches the corrections off (until the next columns).  A plan that never requests allocates and launches nothing for this. */
int rtd_plan_request_nt(rtd_plan* plan, int32_t nleg_all_or_0);
/* Diagnostic, in the spirit of rtd_plan_get_tensors: what the plan holds of the four inputs, uploaded or device-formed.  wfull
 * [rows][L][nleg_all] with *rows = C, or P for a band; f [C][L]; ims_coef [C][nleg_all]; ims_par [C][2].  Any pointer may be NULL.
 * RTD_ERR_STATE when no corrections are set.  Synchronous. */
int rtd_plan_get_nt(rtd_plan* plan, double* wfull, double* f, double* ims_coef, double* ims_par, int32_t* rows);

/* Throughput form: evaluation points are uploaded once, results stay in HBM. */
int rtd_plan_set_eval_points(rtd_plan* plan, int32_t ntau, const double* tau, int32_t nphi, const double* phi);
/* What rtd_plan_run / rtd_plan_run_fetch evaluate at the stored points (and rtd_plan_fetch then returns): order 0 the values
 * (default), -1 the tau-antiderivatives (bit 0 of rtd_plan_evaluate's flag word), +1 the tau-derivatives (its bit 2, same
 * one-sided convention at the interfaces).  A streamed batch too large to retain thus returns derivatives host to host through
 * the window pipeline.  Any order other than 0 takes the evaluation kernel: the fused interface evaluation is value-only.
 * RTD_ERR_ARG for any other order. */
int rtd_plan_set_eval_order(rtd_plan* plan, int32_t order);
/* solve + evaluate at the stored points, asynchronous on the plan's stream */
int rtd_plan_run(rtd_plan* plan);
/* copy the results of the last rtd_plan_run to the host (any pointer may be NULL) */
int rtd_plan_fetch(rtd_plan* plan, double* u, double* u0, double* flux_up, double* flux_down_diffuse,
                   double* flux_down_direct);
/* rtd_plan_run + rtd_plan_fetch as one host-to-host pipeline: window w's results travel to the host (device -> pinned
 * staging on a copy stream -> the caller's arrays) while window w+1 is being solved.  Synchronous; any pointer may be NULL. */
int rtd_plan_run_fetch(rtd_plan* plan, double* u, double* u0, double* flux_up, double* flux_down_diffuse,
                       double* flux_down_direct);
/* Spectral integration of the results on the device: with weights set, consecutive groups of G columns are the spectral points
 * of one profile (column c = p G + g, P = ncols / G), and
 *   out[p][k][e] = sum_g w[k][g] X[p G + g][e]
 * for each of K >= 1 weight sets (k-distribution weights, several channels' response functions, photolysis cross sections) and
 * every element e of a column's result X.  The t-th evaluation point of each of a profile's columns must be the same physical
 * level: that is the caller's contract.  The sum is accumulated in double-double (exact products, g ascending) and rounded once:
 * it is the correctly rounded sum to within 2^-90 sum_g |w x|, whatever the window size.  w [K][G]; ncols % G == 0 and K >= 1,
 * else RTD_ERR_ARG; G <= 0 switches the stage off.  Not combined with rtd_plan_set_mode_shard or a communicator (RTD_ERR_STATE:
 * multi-GPU band runs shard by profile and need no collective over g). */
int rtd_plan_set_band_weights(rtd_plan* plan, int32_t ngpoints, int32_t nsets, const double* w);
/* After rtd_plan_run: reduces the plan's result buffers on the plan's stream and copies out u [P][K][NQuad][ntau][nphi],
 * u0 [P][K][NQuad][ntau] and the fluxes [P][K][ntau]; a NULL output is neither reduced nor copied.  Status as rtd_plan_fetch: when
 * any of a profile's G columns has failed numerically (mode 0 for u0 and the fluxes, any mode for u) that profile's outputs are NaN,
 * every other profile keeps its result, and the call returns RTD_ERR_NUMERIC.  rtd_plan_fetch still returns the unreduced fields. */
int rtd_plan_fetch_band(rtd_plan* plan, double* u, double* u0, double* flux_up, double* flux_down_diffuse,
                        double* flux_down_direct);
/* rtd_plan_evaluate (solved or retained plan, the same flag word, the same tau-range error; tau [C][ntau]) without copying the
 * unreduced fields out: evaluates into the device buffers, reduces, returns the reduced arrays of rtd_plan_fetch_band. */
int rtd_plan_evaluate_band(rtd_plan* plan, int32_t ntau, const double* tau, int32_t nphi, const double* phi, int32_t flags,
                           double* u, double* u0, double* flux_up, double* flux_down_diffuse, double* flux_down_direct);
/* Actinic fluxes (4 pi x the mean intensity: what a photolysis rate integrates) of the results the plan holds, formed on the
 * device from the resident u0 (rtd_actinic_kernel, one thread per column and point, the streams summed in ascending order: the
 * bits depend on neither the launch geometry nor the window size).  The reference has them for one column on the host
 * (generate_diff_act_flux_funcs, subroutines.py:258-318; _assemble_intensity_and_fluxes.py:353-371).  With x = u0, w the
 * quadrature weights, l, tau* and sc = scale_tau[l] of the point as in rtd_plan_evaluate, and I0 the CALLER's beam
 * (rescale x the prepared I0):
 *   act_up           = 2 pi sum_{i<N} w_i x_i
 *   act_down_diffuse = 2 pi sum_{i<N} w_i x_{N+i} + R,   R = I0 e^(-tau* / mu0) - I0 e^(-tau / mu0)
 *   act_down_direct  = D = I0 e^(-tau / mu0)             (flux_down_direct / mu0; no counterpart in the reference)
 * in the order (value, tau-antiderivative, tau-derivative) the results were evaluated in -- rtd_plan_set_eval_order for
 * rtd_plan_run / _run_fetch, the flag word for rtd_plan_evaluate / _evaluate_band:
 *   antiderivative: R = I0 e^(-tau* / mu0) / (-sc / mu0) - I0 e^(-tau / mu0) (-mu0),   D = I0 e^(-tau / mu0) (-mu0)
 *   derivative:     R = I0 e^(-tau* / mu0) (-sc / mu0) - I0 e^(-tau / mu0) / (-mu0),   D = I0 e^(-tau / mu0) / (-mu0)
 * R is the part of the direct beam that delta-M scaling reclassifies as diffuse: act_down_diffuse + act_down_direct is the
 * physical downward actinic flux.  R = D = 0 for a plan without a beam and for a column with I0 = 0; a mode shard that does not
 * own mode 0 returns zeros, like the fluxes.  (The reference forms R with the I0 it has divided by its rescale factor and does
 * not multiply back: its flux_act_down_diffuse is low by R (1 - 1 / rescale) whenever another source exceeds the beam.)
 * [C][ntau] each, ntau that of the LATEST evaluation (rtd_plan_evaluate / _evaluate_band replace the stored points, whatever
 * outputs they were asked for; flux_bytes of rtd_plan_result_dev_ptrs = 3 C ntau 8 tells it); any pointer may be NULL.
 * RTD_ERR_STATE when the plan holds no evaluated results (nothing solved, or new evaluation points, new inputs, a new mode shard
 * or a new solve -- rtd_plan_solve or the layer-shard pair -- since); RTD_ERR_NUMERIC as rtd_plan_fetch reports it for u0.
 * The buffers behind these calls are allocated at the first of them: a plan that never asks holds what it held before.  The
 * gathered-results collectives (rtd_comm_*) do not carry actinic fluxes. */
int rtd_plan_fetch_actinic(rtd_plan* plan, double* act_up, double* act_down_diffuse, double* act_down_direct);
/* The same summed over the spectral points with every weight set (rtd_plan_set_band_weights; rtd_band_reduce_kernel with the
 * mode-0 mask), [P][K][ntau]: with w[k][g] = cross section x quantum yield x the point's k-weight, up + diffuse + direct is the
 * photolysis rate per level.  RTD_ERR_STATE without weights; a profile with a failed column is NaN and the call returns
 * RTD_ERR_NUMERIC, as rtd_plan_fetch_band. */
int rtd_plan_fetch_band_actinic(rtd_plan* plan, double* act_up, double* act_down_diffuse, double* act_down_direct);
/* Radiances at user polar angles: the reference's subroutines.interpolate (subroutines.py:614-705) -- barycentric polynomial
 * interpolation in mu of the evaluated u and u0, each hemisphere on its own -- applied on the device to the results the plan holds
 * (rtd_view_basis_kernel, rtd_view_apply_kernel).  It is polynomial interpolation of u as evaluated (with its Nakajima-Tanaka
 * corrections when they are on), NOT an integration of the source function.  With x_j, j < N, the positive nodes and the rows of u
 * ordered [x_0 .. x_{N-1}, -x_0 .. -x_{N-1}]: mu > 0 reads the rows 0 .. N-1, every other mu the rows N .. 2N-1 -- +0.0 and -0.0
 * included (the reference's mask is `mu > 0`): mu = 0 is the DOWNWARD hemisphere's polynomial at its end.  With a = |mu|
 *   l_j(a) = (b_j / (a - x_j)) / sum_k (b_k / (a - x_k)),  b_j = 1 / prod_{k != j} (x_j - x_k),  out = sum_j l_j u_row(j);
 * a == x_j returns that row bit for bit.  b is formed on the host once per request in long double and rounded once; the sum is one
 * chain, j ascending, without atomics: the bits depend on neither the launch geometry nor the window size.  The operator is linear
 * and acts on mu alone, so it applies to whatever the result buffers hold: values, tau-antiderivatives or tau-derivatives, the
 * partial sums of a mode shard (the shards' results add up).  A per-column relative azimuth needs nothing new: phi0[c].
 * mu: [nmu], or [C][nmu] when per_column != 0, every |mu| <= 1 (else, or for a NaN or a null pointer, RTD_ERR_ARG); nmu <= 0
 * withdraws the request.  RTD_ERR_STATE before rtd_plan_set_quadrature.  Sticky across solves and evaluations, like the band
 * weights; the call itself touches the host only.  Under band weights per-column angles must be identical within a profile
 * (RTD_ERR_ARG here when the weights are present, else from rtd_plan_fetch_band_view). */
int rtd_plan_set_view_mu(rtd_plan* plan, int32_t nmu, const double* mu, int32_t per_column);
/* Where the Nakajima-Tanaka corrections of the view of u come from.  mode 0 (default): from the interpolation, as above -- the
 * corrected u of the nodes is interpolated.  That is right for the smooth delta-M solution and wrong in kind for the corrections: TMS
 * is the single-scattering term of the full, untruncated phase function, whose forward peak a polynomial through the nodes cannot
 * carry.  mode 1: the corrections are closed forms of the inputs and of (mu, tau, phi), so they are evaluated AT the angles
 * (csrc/rtd_nt_view.hip, arithmetic csrc/rtd_nt_view.h):
 *   u_mu(c, mu, tau, phi) = sum_j l_j(|mu|) u_uncorrected(c, j, tau, phi) + rescale_c [TMS + IMS](c, mu, tau, phi)
 * TMS for both hemispheres, IMS for mu < 0 only, as at the nodes; in all three tau-orders.  The formulas are written so that they stay
 * finite and keep their digits where the node formulas are infinity times zero: |mu| = mu0 (an almucantar has mu = -mu0 exactly),
 * |mu| = the IMS scaled mu0 (ims_par[0]) and their neighbourhoods, and mu = +-1.  mu = +-0.0 is REFUSED in this mode (RTD_ERR_ARG, from
 * this call when the held angles contain it, from rtd_plan_set_view_mu afterwards): the limit differs by hemisphere; mode 0 keeps
 * accepting it.  u0_mu is untouched (the corrections never touched u0), and so are u, u0 and the fluxes themselves.
 * The view of u is then formed BY THE EVALUATION (run, run_fetch, evaluate, evaluate_band), window by window, and the two fetches copy
 * or reduce it as it is: angles or a mode set AFTER an evaluation leave the view of u unavailable until the next one (RTD_ERR_STATE
 * from the fetches; u0_mu is still served).  Each output is one chain of additions in a fixed order, without atomics: the bits depend on
 * neither the launch geometry nor the window size.  A plan without corrections, and an evaluation that skips them (bit 1 of the flag
 * word), ignore the mode: their u is interpolated at the fetch.  Mode shards follow the node corrections' rule: the corrections are
 * applied by whichever shard's plan has them switched on (the front end switches them on in the shard that owns mode 0 only), that
 * shard's view carries them whole, and the shards' views add up.  With mode 0 every result of every entry point keeps its bits, and a
 * plan that never asks for mode 1 allocates and launches nothing more.  RTD_ERR_ARG for any other mode.  Host only, sticky. */
int rtd_plan_set_view_nt(rtd_plan* plan, int32_t mode);
/* u_mu [C][nmu][ntau][nphi], u0_mu [C][nmu][ntau] of the LATEST evaluation (run, run_fetch, evaluate, evaluate_band), interpolated
 * on the plan's stream and copied out; either pointer may be NULL.  RTD_ERR_STATE when no angles are set, when the plan holds no
 * evaluated results (as rtd_plan_fetch_actinic), or when u_mu is asked for but the latest evaluation formed no u (nphi = 0, or an
 * evaluation whose u pointer was NULL without bit 3 of its flag word); RTD_ERR_NUMERIC as rtd_plan_fetch reports it: any mode for
 * u_mu, mode 0 for u0_mu.  The buffers behind these calls are allocated at the first of them: a plan that never asks holds what it
 * held before.  The gathered-results collectives (rtd_comm_*) do not carry these arrays. */
int rtd_plan_fetch_view(rtd_plan* plan, double* u_mu, double* u0_mu);
/* The same summed over the spectral points with every weight set (rtd_band_reduce_kernel; masks: any mode for u_mu, mode 0 for
 * u0_mu): u_mu [P][K][nmu][ntau][nphi], u0_mu [P][K][nmu][ntau].  RTD_ERR_STATE without weights; a profile with a failed column
 * is NaN and the call returns RTD_ERR_NUMERIC, as rtd_plan_fetch_band. */
int rtd_plan_fetch_band_view(rtd_plan* plan, double* u_mu, double* u0_mu);
/* Lambertian albedo sweeps from one solve.  For a Lambertian surface of albedo A that emits (1 - A) E below the layers, every field
 * x of the solution -- u, u0, flux_up, the diffuse flux_down, a view of u or u0, in any tau-order -- is, exactly in the
 * discrete-ordinate system (the adding formula of 6S, MODTRAN and DISORT's albedo / transmissivity mode),
 *   x(A) = x_black + kappa(A) x_below,   kappa(A) = (A F / pi + (1 - A) E) / (1 - A s)
 * x_black: the caller's problem over a BLACK, non-emitting surface (the primary: nbdrf = 0, b_pos = 0; beam, b_neg, thermal sources,
 * delta-M and Nakajima-Tanaka corrections as it likes -- the corrections do not see the surface); x_below: the same layers without
 * any source, lit from below by unit isotropic intensity (the companion: b_pos = 1, nfourier 1, beam 0, nscoeffs 0, nbdrf 0);
 * F = flux_down (diffuse + direct, VALUE order) of the primary at the bottom, s = flux_down of the companion at the bottom over pi,
 * the spherical albedo.  kappa does not depend on tau: the formula holds for values, tau-antiderivatives and tau-derivatives alike.
 * The direct flux does not change.  K albedos cost the two solves -- 1 + 1 / nfourier of one -- and an elementwise kernel.
 * rtd_plan_couple_lambert couples the LATEST evaluations the two plans hold (run, run_fetch, evaluate, evaluate_band), on the device
 * (rtd_lambert_kappa_kernel, rtd_lambert_couple_kernel; arithmetic and rounding bound csrc/rtd_lambert.h; one fma per output, no
 * atomics: the bits depend on neither the launch geometry nor the window or chunk size):
 *   albedo        [A] (albedo_rows = 1) or [C][A] (albedo_rows = C), every value in [0, 1]
 *   fdown_bottom, sph_albedo [C]   F and s, caller-supplied (the caller evaluates both plans at the bottom once)
 *   emission      [C] or NULL (= 0): E >= 0, the surface's black-body emission
 *   u [C][A][NQuad][ntau][nphi], u0 [C][A][NQuad][ntau], flux_up, flux_down_diffuse [C][A][ntau]
 *   u_mu [C][A][nmu][ntau][nphi], u0_mu [C][A][nmu][ntau]   with viewing angles set on BOTH plans (rtd_plan_set_view_mu): the
 *                 primary's view of u as its evaluation or rtd_plan_fetch_view would return it (interpolated or at the angles), the
 *                 companion's view of u0 beside it
 * Any output pointer may be NULL; nothing is formed for it.  The coupled arrays are formed chunk of columns after chunk in a scratch
 * block from the pool (RTD_LAMBERT_BYTES, default 256 MiB -- not a tuned number; one column at least) and copied out; nothing stays
 * with either plan (the view outputs go through the plans' own view buffers, as rtd_plan_fetch_view does), and a plan that never asks
 * allocates and launches nothing for this.  Synchronous.
 * A column with 1 - A s <= 0 (or a non-finite factor) for one of its albedos is NaN in every output.
 * RTD_ERR_ARG: a null plan, nalb < 1, an albedo outside [0, 1] or not finite, an emission negative or not finite, albedo_rows neither
 * 1 nor C, a null albedo, fdown_bottom or sph_albedo.  RTD_ERR_STATE: the plans differ in ncols, nlayers, nquad or device; the
 * companion's dims are not (nfourier 1, beam 0, nscoeffs 0, nbdrf 0); the primary has nbdrf != 0; either plan holds no evaluated
 * results (as rtd_plan_fetch_actinic); the resident ntau or tau-order of the two differ; u is wanted but the primary's latest
 * evaluation formed none; view outputs are wanted but angles are not set on both plans or nmu differs; a mode shard or a communicator
 * is active.  RTD_ERR_NUMERIC as rtd_plan_fetch reports it, over both plans: the failed columns are NaN (u and u_mu: any mode of the
 * primary; the others: mode 0 of either plan), the others keep their results. */
int rtd_plan_couple_lambert(rtd_plan* primary, rtd_plan* companion, int32_t nalb, const double* albedo, int32_t albedo_rows,
                            const double* fdown_bottom, const double* sph_albedo, const double* emission, double* u, double* u0,
                            double* flux_up, double* flux_down_diffuse, double* u_mu, double* u0_mu);
/* The same for a band: kappa differs per spectral point (F, s and possibly A depend on g), so the columns are coupled BEFORE the
 * weighted sum over g, which rtd_band_reduce_kernel then forms with the primary's band weights, chunk of profiles after chunk.
 * albedo_rows: 1, P (one list per profile) or C = P G (a spectral albedo).  u [P][K][A][NQuad][ntau][nphi], u0 [P][K][A][NQuad][ntau],
 * the fluxes [P][K][A][ntau], the views [P][K][A][nmu][...].  RTD_ERR_STATE without weights on the primary.  A profile with a failed
 * column in either plan is NaN, the others are kept, and the call returns RTD_ERR_NUMERIC.  Per-column angles must be identical
 * within a profile (RTD_ERR_ARG, as rtd_plan_fetch_band_view). */
int rtd_plan_couple_lambert_band(rtd_plan* primary, rtd_plan* companion, int32_t nalb, const double* albedo, int32_t albedo_rows,
                                 const double* fdown_bottom, const double* sph_albedo, const double* emission, double* u, double* u0,
                                 double* flux_up, double* flux_down_diffuse, double* u_mu, double* u0_mu);
/* The plan-free form, like rtd_planck_band: kappa [ncols][A] by the kernel the plans use (the same bits), and flag [ncols] (may be
 * NULL): 1 where 1 - A s <= 0 or a factor is not finite for one of the column's albedos.  albedo_rows 1 or ncols; host arrays in,
 * host arrays out, synchronous; the argument errors of rtd_plan_couple_lambert. */
int rtd_lambert_kappa(int32_t device, int64_t ncols, int32_t nalb, const double* albedo, int32_t albedo_rows,
                      const double* fdown_bottom, const double* sph_albedo, const double* emission, double* kappa, int32_t* flag);
/* device pointers of the result buffers of rtd_plan_run (for a device-side collective); any pointer may be NULL */
int rtd_plan_result_dev_ptrs(rtd_plan* plan, void** u_dev, int64_t* u_bytes, void** flux_dev, int64_t* flux_bytes);

/* --- the reference's tensors for one column (layout of the reference) ---------------------- */
/* GC [M][L][Q][Q], K [M][L][Q], B [M][L][Q], G_inv_mu_inv [L][Q], G [M][L][Q][Q]; any may be NULL.
 * These are what _solve_for_coeffs returns (_coeffs.py:390) and what the closures capture. */
int rtd_plan_get_tensors(rtd_plan* plan, int32_t column, double* GC, double* K, double* B,
                         double* G_inv_mu_inv, double* G);

/* --- one-call forms (rtd_solve_batch / rtd_solve_tensors) -------------------------------- */
/* A struct of the prepared arguments of _assemble_intensity_and_fluxes (_assemble.py:8-32) with the column axis; the
 * field meanings are those of rtd_plan_set_quadrature / rtd_plan_set_columns.  NULL optional fields as there. */
typedef struct {
  const double *mu_pos, *weights;                                         /* [N] */
  const double *scaled_omega, *tau, *scaled_tau_with_0, *scale_tau, *wleg; /* per column and layer */
  const double *mu0, *I0, *phi0, *rescale;                                /* [C] */
  const double *b_pos, *b_neg, *s_poly, *bdrf_q, *bdrf_q0;                /* optional */
} rtd_inputs;

/* create plan -> upload -> solve -> evaluate at (tau [C][ntau], phi [nphi]) -> destroy, in one call: what one batched
 * call of the reference's _assemble_intensity_and_fluxes + closures would return.  Output pointers may be NULL. */
int rtd_solve_batch(const rtd_dims* dims, int32_t device, const rtd_inputs* in, int32_t ntau, const double* tau,
                    int32_t nphi, const double* phi, double* u, double* u0, double* flux_up,
                    double* flux_down_diffuse, double* flux_down_direct);

/* the same up to the solve, returning the tensors the reference's closures capture for column `column`
 * (GC, K, B, G_inv_mu_inv, G in the reference layout; _solve_for_coeffs.py:390). */
int rtd_solve_tensors(const rtd_dims* dims, int32_t device, const rtd_inputs* in, int32_t column, double* GC, double* K,
                      double* B, double* G_inv_mu_inv, double* G);

/* --- measurement --------------------------------------------------------------------------- */
/* When enabled, rtd_plan_run/solve bracket each kernel with HIP events on the plan's stream. */
int rtd_plan_enable_timing(rtd_plan* plan, int32_t enable);
/* accumulated milliseconds per kernel slot since the last reset (slot names as returned by the Python wrapper):
 * [0] "tables" Legendre tables; [2] "jacobi" the fused rtd_eigen_kernel; [1] "asm" and [3] "post" are the empty slots of
 * the earlier three-kernel eigen stage; [4] "iface" the interface kernel of 66 ... 128 streams -- or, at 64 streams, the tiled fused
 * rtd_bc_tile2_kernel; [5] "sweep" the sweep kernel of 66 ... 128 streams -- or the fused rtd_bc_small_kernel / rtd_bc_mfma_kernel
 * when NQuad <= 32 (slot 4 is then empty) -- or, at 64 streams, the pivoted kernels' pass over the chains the tiled kernel flagged; [6] "eval"
 * rtd_eval_kernel or, with the fused interface evaluation, rtd_fourier_kernel, plus the NT corrections.  Launches counted in nlaunch[7] (one per window of columns).  Synchronises; with timing
 * enabled every window starts with a stream synchronisation: a measurement mode, not the throughput path. */
int rtd_plan_get_timing(rtd_plan* plan, double ms[7], int64_t nlaunch[7], int32_t reset);
/* number of (column, mode) chains of the last window solved whose speculative (diagonal-pivot) elimination failed in
 * the tiled fused boundary-condition kernel (64 streams) and that the pivoted row-per-lane kernels solved instead
 * (diagnostic; 0 for other stream counts) */
int rtd_plan_pivoted_chains(rtd_plan* plan, int32_t* chains);
/* maximum Jacobi sweeps used by any eigenproblem of the last solve (diagnostic) */
int rtd_plan_max_sweeps(rtd_plan* plan, int32_t* sweeps);

/* --- multi-GPU: RCCL over xGMI, one communicator rank per plan (one process per GPU) -------- */
/* The path shards by atmospheric column with no exchange during the solve (the reference's
 * independent loops are _solve_for_gen_and_part_sols.py:88-91 and _solve_for_coeffs.py:110-111, the meeting point is
 * the Fourier sum _assemble_intensity_and_fluxes.py:256-260); the one collective stitches the evaluated results of
 * every rank -- u [C][NQuad][ntau][nphi] and the fluxes [3][C][ntau] -- with ncclAllGather.  rank 0 creates the id
 * (ncclGetUniqueId) and hands the 128 bytes to the other ranks by any host channel. */
/* Load RCCL now (call before anything else in the process loads another RCCL/HIP runtime, e.g. PyTorch). */
int rtd_comm_preload(void);
int rtd_comm_unique_id(char id[128]);
int rtd_comm_init(rtd_plan* plan, const char id[128], int32_t rank, int32_t nranks);
/* RCCL's own statement about the plan's communicator: ncclCommCount, ncclCommUserRank, ncclCommCuDevice (any pointer may be
 * null).  RTD_ERR_STATE when they disagree with the arguments of rtd_comm_init. */
int rtd_comm_size(rtd_plan* plan, int32_t* nranks, int32_t* rank, int32_t* device);
/* Which transport carries the collectives, as text: "rccl", or "stub:ipc" / "stub:shm" when RTD_RCCL_STUB named the tests'
 * stand-in (plan may be null: "stub" without the communicator's mode).  Never a rate through the stub. */
int rtd_comm_transport(rtd_plan* plan, char* buf, int32_t nbuf);
int rtd_comm_allgather_fluxes(rtd_plan* plan);               /* asynchronous on the plan's stream */
int rtd_comm_fetch_gathered(rtd_plan* plan, double* out);    /* host [nranks][3][C][ntau] */
/* u AND fluxes of the last rtd_plan_run: the rank's results are snapshot into its own slot of the gathered arrays (device
 * copy on the plan's stream), then two IN-PLACE ncclAllGather run from there on the plan's communication stream, ordered
 * after the copy by an event: the next rtd_plan_run overlaps them completely (nothing of it waits for the collective; the
 * next gather's snapshot does, a whole step later).  rtd_plan_synchronize waits for both streams. */
int rtd_comm_allgather_results(rtd_plan* plan);
/* The same results gathered on ONE rank only ("if only rank 0 needs results"): the other ranks
 * ncclSend their u and fluxes, `root` ncclRecv's them into the layout of rtd_comm_allgather_results (one group call on
 * the communication stream, overlapped with the next run like the all-gather).  Every rank of the communicator calls
 * it; rtd_comm_fetch_gathered_results is then valid on the root. */
int rtd_comm_gather_results(rtd_plan* plan, int32_t root);
/* host copies of the gathered results: u [nranks][C][NQuad][ntau][nphi] (= all nranks * C columns in rank order),
 * fluxes [nranks][3][C][ntau]; either may be NULL */
int rtd_comm_fetch_gathered_results(rtd_plan* plan, double* u, double* fluxes);
/* A slice of the gathered results: the columns [first, first + count) of rank `rank`'s shard -- u [count][NQuad][ntau][nphi],
 * fluxes [3][count][ntau]; either may be NULL.  What a consumer (or a verification: bench.py checks every rank's slot
 * against a local solve of the same columns) reads without copying all nranks * C columns to the host. */
int rtd_comm_fetch_gathered_columns(rtd_plan* plan, int32_t rank, int32_t first, int32_t count, double* u, double* fluxes);
/* Layer shards (the north star's variant "(layer x mode x column) instances sharded, a single
 * all-gather to stitch the boundary-condition system"): the eigen stage is independent per layer
 * (_solve_for_gen_and_part_sols.py:114), the boundary-condition solve couples the layers (_solve_for_coeffs.py:296-323).
 * Rank r decomposes the layers [r * count, (r + 1) * count) of every (column, mode) with rtd_plan_solve_layers; ONE
 * ncclAllGather (rtd_comm_allgather_layers: pack, gather, unpack on the plan's stream) gives every rank the eigen-stage
 * results of all layers -- Y, A, k, E, B per (column, mode, layer) and the thermal-source vectors per (column, layer):
 * 8 Lloc [C M (2 NP^2 + 2 NP + 2 NP) + C (2 NP Ns + NP)] bytes per rank (cfg4, one column, 4 ranks: 737 KB per rank) --
 * and rtd_plan_solve_bc finishes the solve on each rank (or on the one that wants the result).  Worth it only for few
 * columns with very large nlayers x nfourier; plans of one window only. */
int rtd_plan_solve_layers(rtd_plan* plan, int32_t first_layer, int32_t count);
int rtd_comm_allgather_layers(rtd_plan* plan, int32_t count_per_rank);
int rtd_plan_solve_bc(rtd_plan* plan);

/* mode shards: ncclAllReduce(sum) of the u, u0 and flux results of rtd_plan_run over the ranks, in place, asynchronous
 * on the plan's stream (rtd_plan_fetch then returns the complete fields on every rank) */
int rtd_comm_allreduce_results(rtd_plan* plan);
int rtd_comm_destroy(rtd_plan* plan);

enum {
  RTD_OK = 0,
  RTD_ERR_ARG = 1,        /* bad argument / unsupported size */
  RTD_ERR_HIP = 2,        /* HIP runtime failure             */
  RTD_ERR_TAU_RANGE = 3,  /* tau outside [0, tau_arr[-1]]    */
  RTD_ERR_STATE = 4,      /* call order (e.g. evaluate before solve) */
  RTD_ERR_NUMERIC = 5     /* numerical failure on the device: non-positive Cholesky pivot (phase function not positive
                             definite after delta-M scaling), Jacobi iteration not converged, singular boundary-condition
                             system or 1/mu0 on an eigenvalue (non-finite result).  The reference raises LinAlgError from
                             np.linalg.solve / returns NaN in these cases (_solve_for_gen_and_part_sols.py:186, :226-231) */
};

/* --- environment read by the library (the complete list; tests/test_host_logic.py greps the sources against it) ---------
 * None of these changes a result beyond rounding: they select between implementations that the test suite holds to the same
 * parity (tests/test_gpu_parity.py runs the suite under each), size buffers, or print diagnostics.  A timing experiment whose
 * results are NOT valid (such as round 3's aliased hand-off reads, HISTORY.md section 7a) is never an environment switch.
 *   RTD_WORK_BYTES        bytes of solve intermediates per plan (default 24 GiB): sizes the automatic column window
 *   RTD_POOL_BYTES        bytes of device memory (per device) of destroyed plans kept for the next plan in blocks above 64 MB
 *                         (default 0: large blocks go straight back to the runtime); the same as rtd_pool_set_limit
 *   RTD_SURFACE_BYTES     bytes of the scratch block in which the surface models' samples are formed, chunk of columns after chunk
 *                         (default 256 MiB; one column at least): rtd_plan_request_surface, rtd_surface_samples
 *   RTD_LAMBERT_BYTES     bytes of the scratch block in which the coupled arrays of a Lambertian sweep are formed, chunk of columns
 *                         after chunk (default 256 MiB; one column, or one band profile, at least): rtd_plan_couple_lambert, _band
 *   RTD_NO_PIPELINE       windows one after the other on one stream (no second hand-off slot, no eigen stream)
 *   RTD_BC_FORCE_PIVOT    fused boundary-condition kernels: =1 every elimination is redone by the column-pivoted LDS path (the
 *                         path of a failed speculation); =2 every chain of the 32-stream kernel takes the register-resident
 *                         column-pivoted elimination throughout (the path of near-conservative mode-0 chains)
 *   RTD_BC_FORCE_HANDOVER tiled (64-stream) kernel: every third chain goes to the pivoted row-per-lane kernels
 *   RTD_EIG_MFMA          eigen stage with its assembly GEMMs on the matrix cores (measured slower; a tested variant)
 *   RTD_RCCL_STUB         TESTS ONLY: path of a stand-in for the RCCL entry points (tests/stub/librccl_stub.so) for rank processes
 *                         that share one GPU, where RCCL itself refuses a second rank; rtd_comm_transport() then says "stub"
 *   RTD_DEBUG             diagnostics on stderr
 */
#ifdef __cplusplus
}
#endif
#endif /* RTD_H */
