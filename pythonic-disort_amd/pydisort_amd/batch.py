"""Column-batched entry point: many independent atmospheres per call (no reference equivalent -- the
reference solves one column per ``pydisort`` call)."""
import numpy as np

from ._engine import Plan, lambert_kappa, planck_band, view_angles, view_corrections as _view_corrections
from . import _nt
from ._prepare import double_gauss, prepare_columns
from ._surface import surface_request


DEFAULT_RETAIN_BYTES = 16 << 30  # pydisort_batch(retain=..., retain_bytes=None): what a call may keep on the device for its evaluators


def _thermal_inputs(thermal, C, L, N, with_bdrf_samples):
    """``pydisort_batch(thermal=...)``: the dict checked and broadcast to what ``Plan.set_columns_thermal`` takes.  Every error a
    user can make is raised here, before anything touches the device."""
    known = ("TEMPER", "WVNMLO", "WVNMHI", "BTEMP", "TTEMP", "TEMIS", "emissivity")
    unknown = set(thermal) - set(known)
    if unknown:
        raise ValueError(f"thermal: unknown entries {sorted(unknown)} (known: {', '.join(known)}).")
    for k in known[:3]:
        if thermal.get(k) is None:
            raise ValueError(f"thermal: {k} is required.")
    T = np.asarray(thermal["TEMPER"], float)
    if T.ndim not in (1, 2) or T.shape[-1] != L + 1:
        raise ValueError("Missing temperature specification at some boundaries / interfaces.")
    if T.ndim == 2 and T.shape[0] != C:
        raise ValueError("thermal: TEMPER must be [C, L + 1] or [L + 1].")

    def per_column(k):
        v = thermal.get(k)
        if v is None:
            return None
        v = np.asarray(v, float)
        if v.ndim > 1 or (v.ndim == 1 and v.shape != (C,)):
            raise ValueError(f"thermal: {k} must be a scalar or [C].")
        return np.ascontiguousarray(np.broadcast_to(v, (C,)))

    out = dict(TEMPER=np.ascontiguousarray(np.broadcast_to(T, (C, L + 1))))
    for k in known[1:6]:
        out[k] = per_column(k)
    for k in ("TEMPER", "BTEMP", "TTEMP"):
        if out[k] is not None and not np.all(out[k] >= 0):
            raise ValueError(f"thermal: {k} must not be negative.")
    if not (np.all(out["WVNMLO"] >= 0) and np.all(out["WVNMLO"] <= out["WVNMHI"])):
        raise ValueError("thermal: need 0 <= WVNMLO <= WVNMHI.")
    em = thermal.get("emissivity")
    if em is None:
        if with_bdrf_samples:
            raise ValueError("thermal: give `emissivity` with bdrf_samples -- the BDRF modes that Kirchhoff's law would use are "
                             "formed on the device after the sources.")
    else:
        em = np.asarray(em, float)
        if em.ndim == 0 or em.shape == (C,):
            em = np.broadcast_to(em.reshape(-1, 1), (C, N))
        elif em.shape != (C, N):
            raise ValueError("thermal: emissivity must be a scalar, [C] or [C, N].")
        em = np.ascontiguousarray(em)
    out["emissivity"] = em
    return out


def _nt_checks(I0, mu0, N, NLeg, nleg_all):
    """What the device-formed Nakajima-Tanaka corrections need of a batch, checked on the small arrays before a plan exists."""
    if not (np.all(I0 > 0) and NLeg < nleg_all):
        raise ValueError("NT_cor needs a beam source in every column and NLeg < number of Legendre coefficients.")
    if np.any(np.abs(double_gauss(N)[0][None, :] - np.asarray(mu0, float).reshape(-1, 1)) < 1e-8):
        raise ValueError("Some quadrature angles come too close to `mu0`. Perturb `NQuad` or `mu0` to rectify this error.")


def _stream_counts(NQuad, NLeg, NFourier, only_flux, nleg_all):
    """The defaults and rules of NQuad, NLeg and NFourier that ``pydisort_batch`` and ``pydisort_band`` share; nleg_all: the number
    of Legendre coefficients provided -> (N, NLeg, NFourier)."""
    NLeg = NQuad if NLeg is None else NLeg
    NFourier = 1 if only_flux else (NQuad if NFourier is None else NFourier)
    if NQuad % 2 or NQuad < 2 or NQuad > 128:
        raise ValueError("NQuad must be even and between 2 and 128.")
    if not (0 < NFourier <= NLeg <= NQuad and NLeg <= nleg_all):
        raise ValueError("Need 0 < NFourier <= NLeg <= NQuad and NLeg <= number of Legendre coefficients provided.")
    return NQuad // 2, NLeg, NFourier


def _check_numeric_errors(numeric_errors):
    if numeric_errors not in ("raise", "nan"):
        raise ValueError('numeric_errors must be "raise" or "nan".')


def _default_window(only_flux, NFourier, NLeg, NQuad):
    """Columns per window of the streamed forms when the caller names none: windows of ~8 192 (column, mode) chains -- the two-stream
    window pipeline of the library does best there (256 cfg4 columns: +4 % over windows of 2 048); the library
    shrinks a window that does not fit the device (RTD_WORK_BYTES when set, else 80 % of the free device memory: rtd_api.hip
    plan_build)."""
    modes = 1 if only_flux else int(NFourier or NLeg or NQuad)
    return max(64, 8192 // max(modes, 1))


def _retention(retain, retain_bytes, defer_solve, C, N, NFourier, L, device):
    """``retain`` / ``retain_bytes`` of ``pydisort_batch`` -> (form, budget in bytes) for ``Plan``."""
    form = {"auto": 0, True: 0, "full": 1, "lean": 2}.get(retain if isinstance(retain, (str, bool)) else "auto")
    if retain is False or retain is None or (retain == "auto" and defer_solve):
        budget = 0  # (the throughput callers drive plan.run() themselves: nothing to keep)
    elif form is None:
        raise ValueError('retain must be "auto", "full", "lean", False or a number of bytes.')
    elif isinstance(retain, (int, np.integer)) and not isinstance(retain, bool):
        budget = int(retain)  # (an int: that many bytes, the round-5 spelling of retain_bytes)
    else:
        budget = DEFAULT_RETAIN_BYTES if retain_bytes is None else int(retain_bytes)
        if budget > 0 and retain_bytes is None:
            # the default never takes more than three tenths of what is free -- asked of the runtime only when the batch is large
            # enough for it to matter (hipMemGetInfo costs a small call a noticeable fraction of its time)
            NP = 4
            while NP < N:
                NP *= 2
            if C * NFourier * L * (2 * NP * NP + 8 * NP) * 8 > (256 << 20):
                budget = max(1, min(budget, int(0.3 * Plan.free_device_bytes(device))))
    return form, budget


class BatchSolution:
    """Evaluators over all columns; arrays carry a leading column axis.

    ``is_derivative_wrt_tau=True`` (keyword-only) returns the derivative with respect to the unscaled ``tau`` of what the
    evaluator returns otherwise -- exact, from the closed form, for the whole batch in one device pass; at an interface it is the
    one-sided derivative from above (of the layer that ends there), at ``tau = 0`` the right derivative.  It excludes
    ``is_antiderivative_wrt_tau`` (``ValueError``)."""

    def __init__(self, plan, prep):
        self.plan, self.prep = plan, prep
        self.mu_arr = np.concatenate((prep["mu"], -prep["mu"]))

    def _tau(self, tau):
        tau = np.asarray(tau, dtype=float)
        if tau.ndim == 1:
            tau = np.broadcast_to(tau, (self.prep["C"], len(tau)))
        if np.any(tau < 0) or np.any(tau > self.prep["tau"][:, -1:]):
            raise ValueError("tau input outside the tau range specified for the atmosphere (check `tau_arr`).")
        return np.ascontiguousarray(tau)

    @staticmethod
    def _order(is_antiderivative_wrt_tau, is_derivative_wrt_tau):
        if is_derivative_wrt_tau and is_antiderivative_wrt_tau:
            raise ValueError("`is_derivative_wrt_tau` and `is_antiderivative_wrt_tau` cannot both be set.")
        return bool(is_derivative_wrt_tau)

    def _eval(self, want, tau, phi, is_antiderivative_wrt_tau, is_derivative_wrt_tau, mu=None, corrections="interpolated"):
        """One device evaluation of `want` for an evaluator: the order's check, then the view angles `mu` (``u_at`` / ``u0_at``), then
        the range check of tau -> the dict of ``Plan.evaluate``."""
        deriv = self._order(is_antiderivative_wrt_tau, is_derivative_wrt_tau)
        if mu is not None:
            self.plan.set_view(mu, corrections=corrections)
        return self.plan.evaluate(self._tau(tau), phi, is_antiderivative_wrt_tau, want=(want,), derivative=deriv)

    def u(self, tau, phi, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """-> [C, NQuad, ntau, nphi]"""
        return self._eval("u", tau, phi, is_antiderivative_wrt_tau, is_derivative_wrt_tau)["u"]

    def u0(self, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """-> [C, NQuad, ntau]"""
        return self._eval("u0", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau)["u0"]

    def flux_up(self, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """-> [C, ntau]"""
        return self._eval("flux", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau)["flux_up"]

    def flux_down(self, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """-> (diffuse [C, ntau], direct [C, ntau])"""
        r = self._eval("flux", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau)
        return r["flux_down_diffuse"], r["flux_down_direct"]

    def flux_act_up(self, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """Upward actinic flux 2 pi sum_i w_i u0_i, formed on the device -> [C, ntau]"""
        return self._eval("act", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau)["flux_act_up"]

    def flux_act_down(self, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """Downward actinic flux -> (diffuse [C, ntau], direct [C, ntau]).  The diffuse part carries the reference's delta-M
        reclassification term I0 e^(-tau* / mu0) - I0 e^(-tau / mu0) with the caller's I0 (``generate_diff_act_flux_funcs``); the
        direct part is flux_down_direct / mu0; their sum is the physical downward actinic flux."""
        r = self._eval("act", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau)
        return r["flux_act_down_diffuse"], r["flux_act_down_direct"]

    def u_at(self, mu, tau, phi, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False, corrections="interpolated"):
        """u at the polar-angle cosines mu [nmu] or [C, nmu] -> [C, nmu, ntau, nphi]: the reference's ``subroutines.interpolate(u)``
        for the whole batch on the device -- barycentric polynomial interpolation in mu of the evaluated (Nakajima-Tanaka corrected)
        u, each hemisphere on its own; mu > 0 looks up, every other mu, 0 included, down (``Plan.set_view``).  Only u_mu leaves the
        device.  corrections="at_angles" (keyword-only) interpolates the uncorrected u and evaluates the Nakajima-Tanaka corrections
        at mu itself instead of interpolating them -- the choice near the sun's direction, where the full phase function's forward
        peak is narrower than the node spacing; mu = 0 is then a ValueError.  Without NT_cor the two are the same."""
        return self._eval("view_u", tau, phi, is_antiderivative_wrt_tau, is_derivative_wrt_tau, mu, corrections)["u_mu"]

    def u0_at(self, mu, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """The azimuthal mean u0 at the polar-angle cosines mu [nmu] or [C, nmu] -> [C, nmu, ntau] (``u_at``)."""
        return self._eval("view_u0", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau, mu)["u0_mu"]


    # ---- Lambertian albedo sweeps (pydisort_batch(..., lambert_sweep=True)) ----
    lit_from_below = None  # the companion BatchSolution: the same layers without a source, lit from below by unit isotropic intensity;
    #                        its u0_at(mu, 0) is the upward total transmittance
    _lambert = None        # dict(flux_down_bottom [C], spherical_albedo [C]), held on the host for every coupling call
    _thermal_band = None   # (WVNMLO, WVNMHI) of thermal=, for lambert(BTEMP=)

    def _lambert_state(self, caller):
        if self._lambert is None:
            raise ValueError(f"{caller} needs a solution made with lambert_sweep=True.")
        return self._lambert

    def lambert_terms(self):
        """The atmospheric-correction terms of the sweep -> dict(flux_down_bottom [C]: the downward flux, diffuse + direct, at the
        bottom over a black surface; spherical_albedo [C]: flux_down of ``lit_from_below`` at the bottom over pi)."""
        return dict(self._lambert_state("lambert_terms"))

    def _lambert_emission(self, emission, BTEMP):
        """emission / BTEMP of ``lambert`` -> [C] or None (``planck_band`` over the band of thermal=)."""
        if BTEMP is None:
            return emission
        if emission is not None:
            raise ValueError("Give either emission or BTEMP, not both.")
        if self._thermal_band is None:
            raise ValueError("BTEMP needs the band of thermal= (WVNMLO, WVNMHI).")
        T = np.broadcast_to(np.asarray(BTEMP, float), (self.prep["C"],))
        if T.ndim != 1 or not np.all(T >= 0):
            raise ValueError("BTEMP must be a scalar or [C] and not negative.")
        return planck_band(np.ascontiguousarray(T), *self._thermal_band, device=self.plan.device)

    def lambert(self, albedo, emission=None, BTEMP=None):
        """The same atmosphere over the Lambertian albedos `albedo` [A] or [C, A], emitting (1 - A) x `emission` (scalar or [C];
        or BTEMP: the Planck function over the band of thermal=) -> ``LambertSweep``, whose evaluators carry an albedo axis after the
        column axis.  Exact in the discrete-ordinate system: x(A) = x_black + kappa(A) x_below, coupled on the device
        (``Plan.couple_lambert``); no solve is made."""
        self._lambert_state("lambert")
        return LambertSweep(self, albedo, self._lambert_emission(emission, BTEMP))


class LambertSweep:
    """Evaluators of a ``lambert_sweep=True`` solution over a list of Lambertian albedos: what ``BatchSolution`` returns with an
    albedo axis after the column axis, and the same two tau-order keywords.  Each call evaluates the primary and ``lit_from_below``
    at the points (an evaluation each, no solve on a retained plan) and couples them on the device.

    kappa : [C, A] the coupling factor as the device formed it (csrc/rtd_lambert.h)."""

    def __init__(self, sol, albedo, emission):
        self.sol, self.albedo, self.emission = sol, np.asarray(albedo, float), emission
        t = sol._lambert
        self.kappa, self.kappa_flag = lambert_kappa(self._column_albedo(), t["flux_down_bottom"], t["spherical_albedo"], emission, sol.plan.device)

    def _column_albedo(self):
        """The albedo as the coupling calls take it: [A] or [C, A]."""
        return self.albedo

    def _couple(self, want):
        t = self.sol._lambert
        return self.sol.plan.couple_lambert(self.sol.lit_from_below.plan, self._column_albedo(), t["flux_down_bottom"], t["spherical_albedo"],
                                            self.emission, want=want)

    def _eval(self, want, tau, phi, is_antiderivative_wrt_tau, is_derivative_wrt_tau, mu=None, corrections="interpolated"):
        a, b = self.sol, self.sol.lit_from_below
        deriv = a._order(is_antiderivative_wrt_tau, is_derivative_wrt_tau)
        if mu is not None:
            a.plan.set_view(mu, corrections=corrections)
            b.plan.set_view(mu)
        tau = a._tau(tau)
        if want == "flux":  # (the one field the surface does not touch travels as the primary evaluates it)
            self._direct = a.plan.evaluate(tau, None, is_antiderivative_wrt_tau, want=("flux",), derivative=deriv)["flux_down_direct"]
        else:
            a.plan.evaluate_resident(tau, phi, is_antiderivative_wrt_tau, deriv, keep_u=want in ("u", "view_u"))
        b.plan.evaluate_resident(tau, None, is_antiderivative_wrt_tau, deriv)
        return self._couple((want,))

    def u(self, tau, phi, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """-> [C, A, NQuad, ntau, nphi]"""
        return self._eval("u", tau, phi, is_antiderivative_wrt_tau, is_derivative_wrt_tau)["u"]

    def u0(self, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """-> [C, A, NQuad, ntau]"""
        return self._eval("u0", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau)["u0"]

    def flux_up(self, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """-> [C, A, ntau]"""
        return self._eval("flux", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau)["flux_up"]

    def flux_down(self, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """-> (diffuse [C, A, ntau], direct [C, A, ntau]); the direct flux does not see the surface: the primary's, broadcast."""
        diffuse = self._eval("flux", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau)["flux_down_diffuse"]
        return diffuse, np.ascontiguousarray(np.broadcast_to(self._direct[:, None, :], diffuse.shape))

    def u_at(self, mu, tau, phi, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False, corrections="interpolated"):
        """-> [C, A, nmu, ntau, nphi] (``BatchSolution.u_at``: the primary's view of u, interpolated or with its corrections at the
        angles, coupled with the companion's view of u0)."""
        return self._eval("view_u", tau, phi, is_antiderivative_wrt_tau, is_derivative_wrt_tau, mu, corrections)["u_mu"]

    def u0_at(self, mu, tau, is_antiderivative_wrt_tau=False, *, is_derivative_wrt_tau=False):
        """-> [C, A, nmu, ntau]"""
        return self._eval("view_u0", tau, None, is_antiderivative_wrt_tau, is_derivative_wrt_tau, mu)["u0_mu"]


def _lambert_refusals(bdrf_q, bdrf_q0, bdrf_samples, surface, mode_shard, b_pos, thermal, defer_solve):
    """What ``lambert_sweep=True`` excludes: the primary is solved over a black, non-emitting surface; the surface belongs to the sweep."""
    for name, v in (("bdrf_q", bdrf_q), ("bdrf_q0", bdrf_q0), ("bdrf_samples", bdrf_samples), ("surface", surface), ("mode_shard", mode_shard)):
        if v is not None:
            raise ValueError(f"lambert_sweep cannot be combined with {name}: the primary is solved over a black surface.")
    if np.any(np.asarray(b_pos, float) != 0):
        raise ValueError("lambert_sweep needs b_pos = 0: the surface's emission is given to lambert(emission=...).")
    if thermal is not None and (thermal.get("BTEMP") is not None or thermal.get("emissivity") is not None):
        raise ValueError("lambert_sweep: BTEMP and emissivity belong to lambert(BTEMP=...), not to thermal=.")
    if defer_solve:
        raise ValueError("lambert_sweep is not available in the streamed forms.")


def _lambert_companion(sol, prep_c, device, work_columns, budget, form, bottom):
    """The companion plan of a sweep, solved, and the two host-held terms: both plans evaluated at each column's bottom, in value
    order, fluxes only.  sol: the primary's solution, which receives ``lit_from_below`` and the terms."""
    plan_c = Plan(prep_c, device=device, work_columns=work_columns, retain_bytes=budget, retain_form=form or 0)
    plan_c.numeric_errors = sol.plan.numeric_errors
    plan_c.solve()
    sol.lit_from_below = BatchSolution(plan_c, plan_c.prep)
    bottom = np.ascontiguousarray(bottom)
    ra, rb = sol.plan.evaluate(bottom, want=("flux",)), plan_c.evaluate(bottom, want=("flux",))
    sol._lambert = dict(flux_down_bottom=np.ascontiguousarray(ra["flux_down_diffuse"][:, 0] + ra["flux_down_direct"][:, 0]),
                        spherical_albedo=np.ascontiguousarray((rb["flux_down_diffuse"][:, 0] + rb["flux_down_direct"][:, 0]) / np.pi))


def pydisort_batch(tau_arr, omega_arr, NQuad, Leg_coeffs_all, mu0, I0, phi0, NLeg=None, NFourier=None,
                   b_pos=0, b_neg=0, only_flux=False, f_arr=0, NT_cor=False, bdrf_q=None, bdrf_q0=None,
                   s_poly_coeffs=None, device=0, bdrf_samples=None, NBDRF=None, mode_shard=None, work_columns=0,
                   device_prepare=False, numeric_errors="raise", retain="auto", retain_bytes=None, _defer_solve=False,
                   thermal=None, surface=None, lambert_sweep=False):
    """Like ``pydisort`` with a leading column axis on every atmospheric input:
    tau_arr, omega_arr, f_arr [C, L]; Leg_coeffs_all [C, L, NLeg_all]; mu0, I0, phi0 [C];
    b_pos / b_neg: scalar, [C], [C, N] or [C, N, NFourier]; s_poly_coeffs [C, L, Ns];
    bdrf_q [C, NBDRF, N, N] and bdrf_q0 [C, NBDRF, N]: BDRF Fourier modes tabulated on the quadrature grid.
    bdrf_samples=(rho_qq [C, N, N, nphi], rho_q0 [C, N, nphi] or None) instead: the reflectance itself sampled at
    dphi_p = 2 pi p / nphi; its first NBDRF (default NFourier) Fourier modes are then formed on the device
    (``subroutines.sample_BDRF`` builds the samples from a function rho(mu, mu', dphi)).
    surface=dict(model="lambert" | "hapke" | "rossli" | "rpv" | "ocean", params=[npar] or [C, npar], nphi=256 (ocean: 512)) instead: a parametric surface
    model, stated in the few numbers a retrieval holds per pixel -- albedo; Hapke's B0, HH, W; the Ross-Li kernel weights f_iso, f_vol,
    f_geo (clamped at 0: the kernels go negative at grazing angles); RPV's rho0, k, Theta, rho_c.  The device samples the reflectance
    at the quadrature nodes and mu0 and forms its first NBDRF (default NFourier) modes (``Plan.request_surface``); no table or sample
    array exists on the host.  rho(mu, mu', dphi) takes dphi as the reference's BDRF callables do: the hot spot is at dphi = pi.
    Implies device_prepare=True; excludes bdrf_q, bdrf_samples and mode_shard.  With ``thermal`` and no emissivity, Kirchhoff's law
    uses the device-formed zeroth mode.
    NT_cor=True adds the Nakajima-Tanaka corrections to ``u`` on the device (needs a beam in every column,
    f_arr > 0 and more Legendre coefficients than NLeg).
    mode_shard=(r, G): solve only the Fourier modes r, r + G, r + 2G, ... (the partition for
    fewer columns than GPUs); the evaluators then return this shard's partial sums -- the shards add up to the full
    result (u0, fluxes and NT corrections come from shard 0 only; ``Plan.allreduce_results`` sums across RCCL ranks).
    device_prepare=True: the delta-M scaling and the source rescaling of pydisort.py:316-372 run on the device from the raw
    inputs (``rtd_plan_set_columns_raw``) instead of in NumPy -- for throughput batches; not with mode_shard.  With NT_cor=True the corrections' inputs are formed on the
    device as well (``Plan.request_nt``: no [C, L, NLeg_all] host array); a column without truncation (f_arr = 0) then gets the TMS
    term alone, its IMS term is exactly 0.
    thermal=dict(TEMPER=..., WVNMLO=..., WVNMHI=..., BTEMP=None, TTEMP=None, TEMIS=1.0, emissivity=None): the thermal problem as
    DISORT states it -- level temperatures TEMPER [C, L + 1] or [L + 1], the wavenumber band (cm^-1), the temperatures of the bottom
    and top boundaries and the top's emissivity (scalars or [C]; None: that boundary does not emit).  The device integrates the
    Planck function per level and boundary and forms what the reference's host helpers ``generate_s_poly_coeffs``,
    ``blackbody_contrib_to_BCs`` and ``generate_emissivity_from_BDRF`` return: the linear-in-tau source of every layer, and
    emissivity x E(BTEMP), TEMIS x E(TTEMP) ADDED to b_pos, b_neg (include/rtd.h: rtd_plan_set_columns_thermal).  emissivity: scalar,
    [C] or [C, N]; None: Kirchhoff's law on the zeroth mode of ``bdrf_q`` (1 without a BDRF; not with ``bdrf_samples``).  Implies
    device_prepare=True; excludes ``s_poly_coeffs``.
    numeric_errors: "raise" (a column whose solve fails numerically -- e.g. a phase function whose truncation is not
    positive -- raises NumericalError from the evaluators; ``sol.plan.column_status()`` tells which) or "nan" (the failed
    columns are NaN in the returned arrays, every other column keeps its result: one bad column does not cost the batch).
    work_columns: columns whose intermediates are resident on the device at a time (0: sized by the library); batches
    larger than that are solved window by window (include/rtd.h: rtd_plan_create_windowed).
    retain: the returned evaluators keep what they need of the solve for EVERY column -- as the reference's closures keep
    GC_collect, K_collect, B_collect (_assemble_intensity_and_fluxes.py:170-262) -- so that calling them again costs an
    evaluation, not a solve, also for a batch of several windows (include/rtd.h: rtd_plan_create_retained).  Two forms: "full"
    (3.1 MB per 20-layer 32-stream column: an evaluator call only evaluates) and "lean" (0.5 MB per such column: coefficients,
    eigenvalues and particular solutions stay, an evaluator call re-runs the eigen stage -- not the boundary-condition solve -- for
    the layers its points touch; same bits, about a tenth of a solve for one depth per column; 10 streams and up).  "auto"
    (default): full while it fits the budget, else lean while that fits, else neither; "full" / "lean": that form or neither;
    False: never (every call of an evaluator on a batch of several windows then solves them again).
    retain_bytes: the budget in bytes.  None (default): DEFAULT_RETAIN_BYTES = 16 GiB, and never more than three tenths of the
    free device memory -- the library is a guest on the GPU; a caller that wants BASELINE's 10^5-column batch retained passes what
    it is willing to give (50 GB lean).
    lambert_sweep=True: the problem is solved as stated over a BLACK, non-emitting surface, and beside it a companion -- the same
    layers without any source, lit from below by unit isotropic intensity, one Fourier mode: 1 / NFourier of a solve -- so that
    ``sol.lambert(albedo)`` returns the solution over any list of Lambertian albedos without another solve (the adding formula, exact
    in the discrete-ordinate system; include/rtd.h: rtd_plan_couple_lambert).  Right after the two solves both are evaluated at each
    column's bottom (fluxes only): ``sol.lambert_terms()`` holds the downward flux over the black surface and the spherical albedo,
    ``sol.lit_from_below`` is the companion's ``BatchSolution``.  On a plan of several windows that is not retained that evaluation,
    like every evaluator call, solves the windows again.  Excludes bdrf_q, bdrf_q0, bdrf_samples, surface, mode_shard, a non-zero
    b_pos, and BTEMP or emissivity inside thermal= (the surface's emission belongs to ``lambert(emission=...)``): ``ValueError``.
    All columns share NQuad, NLeg, NFourier and the layer count.  Returns (mu_arr, BatchSolution)."""
    if lambert_sweep:
        _lambert_refusals(bdrf_q, bdrf_q0, bdrf_samples, surface, mode_shard, b_pos, thermal, _defer_solve)
    tau_arr = np.atleast_2d(np.asarray(tau_arr, float))
    C, L = tau_arr.shape
    omega_arr = np.broadcast_to(np.asarray(omega_arr, float), (C, L))
    Leg = np.asarray(Leg_coeffs_all, float)
    if Leg.ndim == 2:
        Leg = np.broadcast_to(Leg[None], (C,) + Leg.shape)
    N, NLeg, NFourier = _stream_counts(NQuad, NLeg, NFourier, only_flux, Leg.shape[2])
    if not (np.all(tau_arr > 0) and np.all(np.diff(tau_arr, axis=1) > 0)):
        raise ValueError("tau values must be positive and increasing.")
    if not (np.all(omega_arr >= 0) and np.all(omega_arr < 1)):
        raise ValueError("Single-scattering albedo must be between 0 and 1, excluding 1.")
    mu0 = np.broadcast_to(np.asarray(mu0, float), (C,))
    I0 = np.broadcast_to(np.asarray(I0, float), (C,))
    phi0 = np.broadcast_to(np.asarray(phi0, float), (C,))
    if np.any(I0 < 0) or (np.any(I0 > 0) and not np.all((mu0 > 0) & (mu0 <= 1))):
        raise ValueError("Need I0 >= 0 and 0 < mu0 <= 1 for every column when there is a beam source.")

    def bc(b):
        b = np.asarray(b, float)
        if b.ndim == 0 and b == 0:
            return None  # all zero: nothing to allocate or upload
        out = np.zeros((C, N, NFourier))
        if b.ndim == 0 or b.shape == (C,):
            out[:, :, 0] = np.broadcast_to(b, (C,))[:, None]
        elif b.shape == (C, N):
            out[:, :, 0] = b
        elif b.shape == (C, N, NFourier):
            out[:] = b
        else:
            raise ValueError("The shape of a boundary condition is incorrect.")
        return out

    sf = None
    if surface is not None:
        if bdrf_q is not None or bdrf_q0 is not None or bdrf_samples is not None:
            raise ValueError("Give either surface or bdrf_q / bdrf_q0 / bdrf_samples, not both.")
        if mode_shard is not None:
            raise ValueError("surface cannot be combined with mode_shard.")
        sf = surface_request(surface, ((), (C,)), f"one surface, or one per column: C = {C}", NFourier, NBDRF)
        device_prepare = True
    th = None
    if thermal is not None:
        if s_poly_coeffs is not None:
            raise ValueError("Give either s_poly_coeffs or thermal, not both.")
        th = _thermal_inputs(thermal, C, L, N, bdrf_samples is not None)
        device_prepare = True
    f_arr = np.broadcast_to(np.asarray(f_arr, float), (C, L))
    sp = np.zeros((C, L, 0)) if s_poly_coeffs is None or np.all(np.asarray(s_poly_coeffs) == 0) \
        else np.asarray(s_poly_coeffs, float).reshape(C, L, -1)
    bq = np.zeros((C, 0, N, N)) if bdrf_q is None else np.asarray(bdrf_q, float)
    bq0 = np.zeros((C, 0, N)) if bdrf_q0 is None else np.asarray(bdrf_q0, float)
    if bdrf_samples is not None:
        if bdrf_q is not None:
            raise ValueError("Give either bdrf_q / bdrf_q0 or bdrf_samples, not both.")
        nb = NFourier if NBDRF is None else int(NBDRF)
        if not 0 < nb <= NFourier:
            raise ValueError("Need 0 < NBDRF <= NFourier.")
        bq, bq0 = np.zeros((C, nb, N, N)), np.zeros((C, nb, N))  # placeholders: the device fills the tables
    nt_device = 0
    if device_prepare:
        if mode_shard is not None or (NT_cor and th is not None):
            raise ValueError("device_prepare cannot be combined with mode_shard, nor thermal with NT_cor.")
        if NT_cor and not only_flux:  # the corrections' inputs are formed on the device too (Plan.request_nt); checks on the small arrays
            _nt_checks(I0, mu0, N, NLeg, Leg.shape[2])
            nt_device = Leg.shape[2]
        bp, bn = bc(b_pos), bc(b_neg)
        raw = dict(tau_arr=tau_arr, omega_arr=omega_arr, leg=Leg, f_arr=f_arr, mu0=mu0, I0=I0, phi0=phi0,
                   b_pos=None if bp is None else np.ascontiguousarray(bp.transpose(0, 2, 1)),
                   b_neg=None if bn is None else np.ascontiguousarray(bn.transpose(0, 2, 1)),
                   s_poly=sp if sp.shape[2] > 0 else None,
                   bdrf_q=bq if bq.shape[1] > 0 else None, bdrf_q0=bq0 if bq.shape[1] > 0 else None)
        mu, W = double_gauss(N)
        prep = dict(C=C, L=L, N=N, P=NLeg, M=NFourier, Ns=2 if th is not None else sp.shape[2],
                    NBDRF=bq.shape[1] if sf is None else sf["NBDRF"],
                    beam=bool(np.any(I0 > 0)), mu=mu, W=W, tau=tau_arr, raw=raw, thermal=th, nt=nt_device, surface=sf)
    else:
        prep = prepare_columns(tau_arr, omega_arr, NQuad, Leg, mu0, I0, phi0, NLeg, NFourier, bc(b_pos), bc(b_neg),
                               f_arr, sp, bq, bq0)
    if mode_shard is not None:
        r, G = int(mode_shard[0]), int(mode_shard[1])
        if not (0 <= r < G <= NFourier):
            raise ValueError("mode_shard=(r, G) needs 0 <= r < G <= NFourier.")
        modes = np.arange(r, NFourier, G)
        for k in ("b_pos", "b_neg"):  # the source rescale above saw every mode
            if prep[k] is not None:
                prep[k] = np.ascontiguousarray(prep[k][:, modes, :])
        prep["M"] = len(modes)
        prep["mode_shard"] = (r, G, NFourier)
        NT_cor = NT_cor and r == 0
    _check_numeric_errors(numeric_errors)
    form, budget = _retention(retain, retain_bytes, _defer_solve, C, N, NFourier, L, device)
    plan = Plan(prep, device=device, work_columns=work_columns, retain_bytes=budget, retain_form=form or 0)
    plan.numeric_errors = numeric_errors
    if bdrf_samples is not None:
        plan.set_bdrf_samples(bdrf_samples[0], bdrf_samples[1] if np.any(I0 > 0) else None)
    if not _defer_solve:
        plan.solve()
    if NT_cor and not only_flux and not nt_device:
        if not (np.all(I0 > 0) and np.any(f_arr > 0) and NLeg < Leg.shape[2]):
            raise ValueError("NT_cor needs a beam source in every column, f_arr > 0 and NLeg < number of Legendre coefficients.")
        if np.any(np.abs(prep["mu"][None, :] - mu0[:, None]) < 1e-8):
            raise ValueError("Some quadrature angles come too close to `mu0`. Perturb `NQuad` or `mu0` to rectify this error.")
        plan.set_nt(*_nt.nt_inputs(prep, omega_arr, f_arr, Leg, NLeg, mu0))
    sol = BatchSolution(plan, prep)
    if lambert_sweep:
        if th is not None:
            sol._thermal_band = (th["WVNMLO"], th["WVNMHI"])
        # the companion needs no corrections: the first NLeg moments, through the raw device-prepared entry
        raw_c = dict(tau_arr=tau_arr, omega_arr=omega_arr, leg=np.ascontiguousarray(Leg[..., :NLeg]), f_arr=f_arr, mu0=np.ones(C),
                     I0=np.zeros(C), phi0=np.zeros(C), b_pos=np.ones((C, 1, N)), b_neg=None, s_poly=None, bdrf_q=None, bdrf_q0=None)
        mu_c, W_c = double_gauss(N)
        prep_c = dict(C=C, L=L, N=N, P=NLeg, M=1, Ns=0, NBDRF=0, beam=False, mu=mu_c, W=W_c, tau=tau_arr, raw=raw_c, thermal=None, nt=0,
                      surface=None)
        _lambert_companion(sol, prep_c, device, work_columns, budget, form, tau_arr[:, -1:])
    return sol.mu_arr, sol


def solve_columns_streamed(cfg, tau, phi, chunk_columns=0, device=0, only_flux=False, out=None, numeric_errors="raise",
                           *, tau_order=0, actinic=False, mu=None, view_corrections="interpolated"):
    """Throughput form for large column counts: ONE plan holds the inputs and the results of all columns, the
    intermediates of the solve (~8 MB per cfg4 column) live for `chunk_columns` columns at a time (0: ~8 192 (column,
    mode) chains per window) and the device-to-host copies of a window overlap the kernels of the next (``Plan.run_fetch``).
    Source terms are taken from the whole batch (a beam or a thermal source in any column switches it on for all).

    cfg : dict of ``pydisort_batch`` keyword arguments with a leading column axis (tau_arr, omega_arr, Leg_coeffs_all,
          mu0, I0, phi0, optional f_arr, b_pos, b_neg, s_poly_coeffs, bdrf_q, bdrf_q0, NLeg, NFourier); NQuad scalar.
          surface=dict(model=..., params=[npar] or [C, npar], nphi=256) in cfg (with NBDRF) forms the BDRF modes of all columns on
          the device from a parametric model, as in ``pydisort_batch``.
          NT_cor=True in cfg adds the Nakajima-Tanaka corrections to u, their inputs formed on the device (ignored with only_flux).
    tau : [C, ntau] evaluation depths; phi : [nphi].
    out : optional dict of preallocated C-contiguous float64 result arrays to fill (the same keys and shapes).  Without `actinic`
          every key of the result is required.  With actinic=True the contract differs in two places: u0 may be absent (it then
          stays on the device and is not in the result), and an actinic array that is absent is allocated and ADDED to the
          caller's dict; one that is present is checked like the others and filled in place.
    numeric_errors : as in ``pydisort_batch`` ("nan": failed columns come back as NaN, the rest of the batch is kept).
    tau_order : 0 the values (default), +1 their derivatives with respect to the unscaled tau (as ``is_derivative_wrt_tau`` of the
          evaluators: one-sided from above at an interface), -1 their tau-antiderivatives (``is_antiderivative_wrt_tau``): a
          batch too large to retain gets them host to host through the same window pipeline (``Plan.set_eval_order``).
    actinic : True adds flux_act_up, flux_act_down_diffuse, flux_act_down_direct [C, ntau] (``Plan.fetch_actinic``), formed on the
          device from the resident u0 in the same `tau_order`; u0 itself may then be left out of `out` (it is not copied).
    mu : polar-angle cosines [nmu] or [C, nmu] (``Plan.set_view``): adds u_mu [C, nmu, ntau, nphi] (not with only_flux) and u0_mu
          [C, nmu, ntau], interpolated on the device in the same `tau_order` (``Plan.fetch_view``).  u may then be left out of `out`:
          it stays on the device and is neither copied nor returned.  A view array that is absent from `out` is allocated and ADDED
          to the caller's dict; one that is present is checked like the others and filled in place.
    view_corrections : "interpolated" (default) or "at_angles", the `corrections` of ``Plan.set_view`` for u_mu: with NT_cor in cfg the
          corrections are evaluated at mu itself, window by window, instead of being interpolated (mu = 0 is then a ValueError).
    Returns dict(u [C, NQuad, ntau, nphi] (absent when only_flux), u0, flux_up, flux_down_diffuse, flux_down_direct)."""
    if tau_order not in (-1, 0, 1):
        raise ValueError("tau_order must be -1, 0 or +1.")
    tau = np.ascontiguousarray(np.asarray(tau, float))
    C, ntau = tau.shape
    if mu is not None:
        mu = view_angles(mu, C)
    at_angles = bool(_view_corrections(view_corrections, mu))
    if chunk_columns <= 0:
        chunk_columns = _default_window(only_flux, cfg.get("NFourier"), cfg.get("NLeg"), int(cfg["NQuad"]))
    _, sol = pydisort_batch(only_flux=only_flux, device=device, work_columns=chunk_columns, device_prepare=True,
                            numeric_errors=numeric_errors, _defer_solve=True, **cfg)
    plan = sol.plan
    try:
        sol._tau(tau)  # range check on the host, with the reference's message
        phi = np.array([0.0]) if only_flux else np.atleast_1d(np.asarray(phi, float))
        plan.set_eval_points(tau, phi)
        if tau_order != 0:
            plan.set_eval_order(tau_order)
        Q = plan.Q
        shapes = dict(u0=(C, Q, ntau), flux_up=(C, ntau), flux_down_diffuse=(C, ntau), flux_down_direct=(C, ntau))
        if not only_flux:
            shapes["u"] = (C, Q, ntau, len(phi))
        act = {k: (C, ntau) for k in Plan._ACT} if actinic else {}
        view = {}
        if mu is not None:
            plan.set_view(mu, **(dict(corrections=view_corrections) if at_angles else {}))
            view["u0_mu"] = (C, mu.shape[-1], ntau)
            if not only_flux:
                view["u_mu"] = (C, mu.shape[-1], ntau, len(phi))
        if out is None:
            out = {k: np.empty(shp) for k, shp in shapes.items()}
        else:
            for k, shp in list(shapes.items()) + list(act.items()) + list(view.items()):
                a = out.get(k)
                if a is None and actinic and (k == "u0" or k in act):
                    continue  # (with actinic=True the caller may leave u0 on the device; actinic arrays not given are allocated)
                if a is None and view and (k == "u" or k in view):
                    continue  # (with mu the caller may leave u on the device; view arrays not given are allocated)
                if a is None or a.shape != shp or a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
                    raise ValueError(f"out[{k!r}] must be a C-contiguous float64 array of shape {shp}.")
        plan.run_fetch(out)
        if actinic:
            out.update(plan.fetch_actinic(out))
        if view:
            out.update({k: v for k, v in plan.fetch_view(("u0",) if only_flux else ("u", "u0"), out).items() if v is not None})
    finally:
        plan.close()
    return out
