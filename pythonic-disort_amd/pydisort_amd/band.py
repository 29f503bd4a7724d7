"""k-distribution bands: P profiles x G spectral points per call, mixed and spectrally integrated on the device (no reference
equivalent -- the reference solves one monochromatic column per ``pydisort`` call).

Within a band every column of a profile shares its scatterers, its geometry and its surface; only the gas absorption per layer and
the solar weight change from point to point, and what is wanted back is P band results, not P G monochromatic ones.  The band is
stated as the user has it -- G + 2 S numbers per profile and layer -- and the device forms tau_arr, omega_arr, f_arr and the
Legendre moments of the P G columns (include/rtd.h: rtd_plan_set_columns_band) and sums the results over g with the band's
weights (rtd_plan_set_band_weights).  Column p G + g throughout."""
import numpy as np

from ._engine import Plan, lambert_kappa, view_angles, view_corrections as _view_corrections
from ._prepare import double_gauss
from .batch import (BatchSolution, _check_numeric_errors, _default_window, _lambert_companion, _lambert_refusals, _nt_checks, _retention,
                    _stream_counts, _thermal_inputs)
from ._surface import surface_request


def level_tau(tau_arr, levels=None):
    """The optical depth of the interfaces `levels` (indices 0 ... L, None: all of them) of every column: tau_arr [C, L] ->
    [C, nlev].  A level is the only coordinate the spectral points of a profile share: each column is evaluated at its OWN
    optical depth of that level."""
    tau_arr = np.asarray(tau_arr, float)
    C, L = tau_arr.shape
    table = np.concatenate((np.zeros((C, 1)), tau_arr), axis=1)
    if levels is None:
        return table
    lv = np.atleast_1d(np.asarray(levels))
    if lv.ndim != 1 or lv.size < 1 or not np.issubdtype(lv.dtype, np.integer):
        raise ValueError("levels must be interface indices (integers), a scalar or a one-dimensional sequence.")
    if np.any(lv < 0) or np.any(lv > L):
        raise ValueError(f"levels must lie between 0 and the number of layers ({L}).")
    return np.ascontiguousarray(table[:, lv])


def net_flux_convergence(flux_up, flux_down_diffuse, flux_down_direct):
    """F_net[l] - F_net[l + 1] with F_net = down_diffuse + down_direct - up at ALL levels [..., L + 1] -> [..., L]: the power
    each layer absorbs, the heating rate up to the caller's units."""
    net = np.asarray(flux_down_diffuse, float) + np.asarray(flux_down_direct, float) - np.asarray(flux_up, float)
    return net[..., :-1] - net[..., 1:]


def _per_column(v, name, P, G, tail=()):
    """A boundary / surface / thermal array given per profile [P, ...] or per column [P G, ...] -> per column."""
    v = np.asarray(v, float)
    C = P * G
    if v.shape == (C,) + tail:
        return v
    if v.shape == (P,) + tail:
        return np.repeat(v, G, axis=0)
    raise ValueError(f"{name} must be given per profile {(P,) + tail} or per column {(C,) + tail}; got {v.shape}.")


def _band_inputs(dtau_abs, dtau_spec, omega_spec, Leg_spec, NQuad, mu0, I0, phi0, weights, NLeg, NFourier, delta_M, only_flux,
                 b_pos, b_neg, bdrf_q, bdrf_q0, thermal, surface=None, NBDRF=None):
    """Everything a user can get wrong is raised here, on the small arrays, before anything touches the device.
    -> (prep for ``Plan``, weights [K, G], whether the K axis is dropped)."""
    a, ds, om, leg = (np.asarray(v, float) for v in (dtau_abs, dtau_spec, omega_spec, Leg_spec))
    if a.ndim != 3:
        raise ValueError("dtau_abs must have the shape [P, G, L].")
    P, G, L = a.shape
    if ds.ndim != 3 or ds.shape[:2] != (P, L) or ds.shape[2] < 1:
        raise ValueError(f"dtau_spec must have the shape [P = {P}, L = {L}, S] with at least one species.")
    S = ds.shape[2]
    if om.shape != (P, L, S):
        raise ValueError(f"omega_spec must have the shape of dtau_spec {(P, L, S)}.")
    if leg.ndim != 2 or leg.shape[0] != S:
        raise ValueError(f"Leg_spec must have the shape [S = {S}, NLeg_all].")
    N, NLeg, NFourier = _stream_counts(NQuad, NLeg, NFourier, only_flux, leg.shape[1])
    if delta_M and leg.shape[1] <= NLeg:
        raise ValueError("delta_M needs more Legendre coefficients per species than NLeg (the truncation fraction is moment NLeg).")
    if not (np.all(a >= 0) and np.all(ds >= 0)):
        raise ValueError("Optical thicknesses (dtau_abs, dtau_spec) must not be negative.")
    if not (np.all(om >= 0) and np.all(om <= 1)):
        raise ValueError("Single-scattering albedo of every species must be between 0 and 1.")
    if not np.all(leg[:, 0] == 1):
        raise ValueError("The zeroth Legendre coefficient of every species must be 1.")
    # every (p, g, l) through the spectral point of least absorption: never by forming the columns
    least = ds.sum(axis=2) + a.min(axis=1)
    if not np.all(least > 0):
        raise ValueError("Every layer must have a positive optical thickness at every spectral point.")
    if not np.all((om * ds).sum(axis=2) < least):
        raise ValueError("Single-scattering albedo of the mixture must be between 0 and 1, excluding 1.")
    w = np.asarray(weights, float)
    squeeze = w.ndim == 1
    if w.ndim not in (1, 2) or w.shape[-1] != G or w.size == 0:
        raise ValueError(f"weights must have the shape [G = {G}] or [K, G].")
    w = np.ascontiguousarray(np.atleast_2d(w))
    C = P * G

    def per_profile(v, name):
        v = np.asarray(v, float)
        if v.ndim == 0 or v.shape == (P,):
            return np.repeat(np.broadcast_to(v, (P,)), G)
        raise ValueError(f"{name} must be a scalar or [P = {P}].")

    mu0c, phi0c = per_profile(mu0, "mu0"), per_profile(phi0, "phi0")
    I0 = np.asarray(I0, float)
    if I0.ndim == 0 or I0.shape == (G,) or I0.shape == (P, G):  # (P = G: a vector is taken per spectral point)
        I0c = np.ascontiguousarray(np.broadcast_to(I0, (P, G))).reshape(C)
    elif I0.shape == (P,):
        I0c = np.repeat(I0, G)
    else:
        raise ValueError(f"I0 must be a scalar, [G = {G}], [P = {P}] or [P, G].")
    if np.any(I0c < 0) or (np.any(I0c > 0) and not np.all((mu0c > 0) & (mu0c <= 1))):
        raise ValueError("Need I0 >= 0 and 0 < mu0 <= 1 for every column when there is a beam source.")

    def bc(b, name):
        b = np.asarray(b, float)
        if b.ndim == 0:
            if b == 0:
                return None  # all zero: nothing to allocate or upload
            b = np.broadcast_to(b, (P,))
        out = np.zeros((C, NFourier, N))
        if b.ndim == 1:
            out[:, 0, :] = _per_column(b, name, P, G)[:, None]
        elif b.ndim == 2:
            out[:, 0, :] = _per_column(b, name, P, G, (N,))
        elif b.ndim == 3:
            out[:] = _per_column(b, name, P, G, (N, NFourier)).transpose(0, 2, 1)
        else:
            raise ValueError("The shape of a boundary condition is incorrect.")
        return out

    bp, bn = bc(b_pos, "b_pos"), bc(b_neg, "b_neg")
    if (bdrf_q is None) != (bdrf_q0 is None):
        raise ValueError("Give bdrf_q and bdrf_q0 together.")
    NB, bq, bq0 = 0, None, None
    if bdrf_q is not None:
        bq = np.asarray(bdrf_q, float)
        if bq.ndim != 4 or bq.shape[2:] != (N, N) or not 0 < bq.shape[1] <= NFourier:
            raise ValueError("bdrf_q must have the shape [P or P G, NBDRF <= NFourier, N, N].")
        NB = bq.shape[1]
        bq = np.ascontiguousarray(_per_column(bq, "bdrf_q", P, G, (NB, N, N)))
        bq0 = np.ascontiguousarray(_per_column(bdrf_q0, "bdrf_q0", P, G, (NB, N)))
    sf = None
    if surface is not None:
        if bdrf_q is not None:
            raise ValueError("Give either surface or bdrf_q / bdrf_q0, not both.")
        sf = surface_request(surface, ((), (P,), (P, G)), f"one surface, one per profile or one per column: P = {P}, G = {G}", NFourier, NBDRF)
        NB = sf["NBDRF"]
    th = None
    if thermal is not None:
        t = dict(thermal)
        for k, v in list(t.items()):
            if v is None or np.ndim(v) == 0 or (k == "TEMPER" and np.ndim(v) == 1):
                continue
            tail = (L + 1,) if k == "TEMPER" else (N,) if (k == "emissivity" and np.ndim(v) == 2) else ()
            t[k] = _per_column(v, "thermal: " + k, P, G, tail)
        th = _thermal_inputs(t, C, L, N, False)
    mu, W = double_gauss(N)
    band = dict(dtau_abs=a, dtau_spec=ds, omega_spec=om, leg_spec=leg, delta_m=bool(delta_M))
    cols = dict(mu0=mu0c, I0=I0c, phi0=phi0c, b_pos=bp, b_neg=bn, bdrf_q=bq, bdrf_q0=bq0)
    prep = dict(C=C, L=L, N=N, P=NLeg, M=NFourier, Ns=2 if th is not None else 0, NBDRF=NB, beam=bool(np.any(I0c > 0)), mu=mu, W=W,
                tau=None, raw=None, band=band, cols=cols, thermal=th, surface=sf)
    return prep, w, squeeze


class BandSolution:
    """Band results of P profiles: every evaluator returns [P, K, ...], summed over the G spectral points with each of the K
    weight sets on the device (the K axis is dropped when ``weights`` was [G]).  ``levels`` are interface indices 0 ... L (None:
    all of them); each column is evaluated at its own optical depth of the level.

    columns : the ordinary ``BatchSolution`` over the P G columns (unreduced evaluators in tau, column p G + g).
    tau_arr : [P, G, L] the mixed optical depths of the lower layer boundaries, as the device formed them."""

    def __init__(self, plan, P, G, squeeze):
        self.plan, self.P, self.G, self._squeeze = plan, P, G, squeeze
        self.columns = BatchSolution(plan, plan.prep)
        self.mu_arr = self.columns.mu_arr
        self.tau_arr = plan.prep["tau"].reshape(P, G, -1)

    def _out(self, a):
        return a[:, 0] if self._squeeze else a

    def _eval(self, levels, phi, want):
        return self.plan.evaluate_band(level_tau(self.plan.prep["tau"], levels), phi, want=want)

    def flux_up(self, levels=None):
        """-> [P, K, nlev]"""
        return self._out(self._eval(levels, None, ("flux",))["flux_up"])

    def flux_down(self, levels=None):
        """-> (diffuse [P, K, nlev], direct [P, K, nlev])"""
        r = self._eval(levels, None, ("flux",))
        return self._out(r["flux_down_diffuse"]), self._out(r["flux_down_direct"])

    def u0(self, levels=None):
        """-> [P, K, NQuad, nlev]"""
        return self._out(self._eval(levels, None, ("u0",))["u0"])

    def u(self, levels, phi):
        """-> [P, K, NQuad, nlev, nphi]"""
        return self._out(self._eval(levels, phi, ("u",))["u"])

    def flux_act_up(self, levels=None):
        """Upward actinic flux of the band -> [P, K, nlev]"""
        return self._out(self._eval(levels, None, ("act",))["flux_act_up"])

    def flux_act_down(self, levels=None):
        """Downward actinic flux of the band -> (diffuse [P, K, nlev], direct [P, K, nlev]); the delta-M reclassification term is
        applied per column, before the sum over the spectral points (``BatchSolution.flux_act_down``)."""
        r = self._eval(levels, None, ("act",))
        return self._out(r["flux_act_down_diffuse"]), self._out(r["flux_act_down_direct"])

    def actinic_flux(self, levels=None):
        """Total actinic flux up + down diffuse + down direct -> [P, K, nlev].  With weights[k][g] = cross section x quantum yield x
        the point's k-weight this is the photolysis rate per level."""
        r = self._eval(levels, None, ("act",))
        return self._out(r["flux_act_up"] + r["flux_act_down_diffuse"] + r["flux_act_down_direct"])

    def _set_view(self, mu, corrections="interpolated"):
        mu = view_angles(mu, self.P, "P")
        self.plan.set_view(np.repeat(mu, self.G, axis=0) if mu.ndim == 2 else mu, corrections=corrections)

    def u_at(self, mu, levels, phi, *, corrections="interpolated"):
        """Band radiance at the polar-angle cosines mu [nmu] or [P, nmu] -> [P, K, nmu, nlev, nphi]: every column's u is
        interpolated in mu on the device (``BatchSolution.u_at``), then summed over the spectral points.  corrections="at_angles"
        (keyword-only): the Nakajima-Tanaka corrections of every column are evaluated at mu itself before the sum."""
        self._set_view(mu, corrections)
        return self._out(self._eval(levels, phi, ("view_u",))["u_mu"])

    def u0_at(self, mu, levels=None):
        """-> [P, K, nmu, nlev] (``u_at``)"""
        self._set_view(mu)
        return self._out(self._eval(levels, None, ("view_u0",))["u0_mu"])

    def net_flux_convergence(self):
        """-> [P, K, L]: F_net[l] - F_net[l + 1], F_net = down_diffuse + down_direct - up: the layers' absorbed power (host
        arithmetic on the reduced level fluxes)."""
        r = self._eval(None, None, ("flux",))
        return self._out(net_flux_convergence(r["flux_up"], r["flux_down_diffuse"], r["flux_down_direct"]))

    # ---- Lambertian albedo sweeps (pydisort_band(..., lambert_sweep=True)) ----
    def lambert_terms(self):
        """The UNREDUCED terms of the sweep -> dict(flux_down_bottom, spherical_albedo [P, G]) (``BatchSolution.lambert_terms``):
        they differ per spectral point, which is why the coupling happens before the sum over g."""
        return {k: v.reshape(self.P, self.G) for k, v in self.columns.lambert_terms().items()}

    def lambert(self, albedo, emission=None, BTEMP=None):
        """The band over the Lambertian albedos `albedo` [A], [P, A] or [P, G, A] (a spectral albedo), emitting (1 - A) x `emission`
        (scalar, [P] or [P G]; or BTEMP likewise: the Planck function over the band of thermal=) -> ``BandLambertSweep``, whose
        evaluators take levels and return [P, K, A, ...].  Every column is coupled on the device BEFORE the weighted sum over g
        (``Plan.couple_lambert_band``)."""
        self.columns._lambert_state("lambert")
        per_col = [None if v is None or np.ndim(v) == 0 else _per_column(v, name, self.P, self.G) for v, name in ((emission, "emission"), (BTEMP, "BTEMP"))]
        return BandLambertSweep(self, albedo, self.columns._lambert_emission(emission if per_col[0] is None else per_col[0],
                                                                          BTEMP if per_col[1] is None else per_col[1]))


class BandLambertSweep:
    """Evaluators of a ``lambert_sweep=True`` band over a list of Lambertian albedos: what ``BandSolution`` returns with an albedo
    axis after the K axis.  Each call evaluates the primary and the companion at the levels and couples every column on the device
    before the spectral sum.

    kappa : [P, G, A] the coupling factor of every column as the device formed it."""

    def __init__(self, band, albedo, emission):
        alb = np.asarray(albedo, float)
        if alb.ndim == 3:
            if alb.shape[:2] != (band.P, band.G):
                raise ValueError(f"albedo must have the shape [A], [P = {band.P}, A] or [P, G = {band.G}, A].")
            alb = alb.reshape(band.P * band.G, -1)
        elif alb.ndim == 2 and alb.shape[0] != band.P:
            raise ValueError(f"albedo must have the shape [A], [P = {band.P}, A] or [P, G = {band.G}, A].")
        self.band, self.albedo, self.emission = band, alb, emission
        t = band.columns._lambert
        per_column = np.repeat(alb, band.G, axis=0) if (alb.ndim == 2 and alb.shape[0] == band.P and band.G > 1) else alb
        kappa, self.kappa_flag = lambert_kappa(per_column, t["flux_down_bottom"], t["spherical_albedo"], emission, band.plan.device)
        self.kappa = kappa.reshape(band.P, band.G, -1)

    def _eval(self, levels, phi, want, mu=None, corrections="interpolated"):
        band, a, b = self.band, self.band.plan, self.band.columns.lit_from_below.plan
        if mu is not None:
            band._set_view(mu, corrections)
            mu = view_angles(mu, band.P, "P")
            b.set_view(np.repeat(mu, band.G, axis=0) if mu.ndim == 2 else mu)
        tau = level_tau(a.prep["tau"], levels)
        direct = None
        if want == "flux":
            direct = a.evaluate_band(tau, None, want=("flux",))["flux_down_direct"]
        else:
            a.evaluate_resident(tau, phi, keep_u=want in ("u", "view_u"))
        b.evaluate_resident(tau, None)
        t = band.columns._lambert
        out = a.couple_lambert_band(b, self.albedo, t["flux_down_bottom"], t["spherical_albedo"], self.emission, want=(want,))
        out["flux_down_direct"] = direct
        return {k: None if v is None else band._out(v) for k, v in out.items()}

    def flux_up(self, levels=None):
        """-> [P, K, A, nlev]"""
        return self._eval(levels, None, "flux")["flux_up"]

    def flux_down(self, levels=None):
        """-> (diffuse [P, K, A, nlev], direct [P, K, A, nlev]: the primary's, broadcast)"""
        r = self._eval(levels, None, "flux")
        d = r["flux_down_diffuse"]
        return d, np.ascontiguousarray(np.broadcast_to(np.expand_dims(r["flux_down_direct"], -2), d.shape))

    def u0(self, levels=None):
        """-> [P, K, A, NQuad, nlev]"""
        return self._eval(levels, None, "u0")["u0"]

    def u(self, levels, phi):
        """-> [P, K, A, NQuad, nlev, nphi]"""
        return self._eval(levels, phi, "u")["u"]

    def u_at(self, mu, levels, phi, *, corrections="interpolated"):
        """-> [P, K, A, nmu, nlev, nphi] (``BandSolution.u_at``)"""
        return self._eval(levels, phi, "view_u", mu, corrections)["u_mu"]

    def u0_at(self, mu, levels=None):
        """-> [P, K, A, nmu, nlev]"""
        return self._eval(levels, None, "view_u0", mu)["u0_mu"]


def pydisort_band(dtau_abs, dtau_spec, omega_spec, Leg_spec, NQuad, mu0, I0, phi0, weights, NLeg=None, NFourier=None,
                  delta_M=True, only_flux=False, b_pos=0, b_neg=0, bdrf_q=None, bdrf_q0=None, thermal=None, device=0,
                  work_columns=0, numeric_errors="raise", retain="auto", retain_bytes=None, _defer_solve=False, surface=None,
                  NBDRF=None, lambert_sweep=False, NT_cor=False):
    """P profiles x G spectral points of a band in one call.

    dtau_abs [P, G, L]: absorption optical thickness of each layer at each spectral point; dtau_spec, omega_spec [P, L, S]:
    extinction optical thickness and single-scattering albedo of each of S scatterer species; Leg_spec [S, NLeg_all]: the species'
    Legendre coefficients.  The device mixes them into the P G columns (column p G + g):
    dtau = sum_s dtau_s + dtau_abs, omega = sum_s omega_s dtau_s / dtau, moments weighted by omega_s dtau_s; with delta_M the
    truncation fraction f is the mixture's moment NLeg (Leg_spec then needs more than NLeg moments).  A layer without a scatterer
    gets the moments (1, 0, ...).
    mu0, phi0: scalar or [P]; I0: scalar, [G] (the solar weight of each spectral point), [P] or [P, G].
    weights: [G] or [K, G] -- k-distribution weights, several channels' response functions, photolysis cross sections.
    b_pos / b_neg (scalar, [.], [., N] or [., N, NFourier]), bdrf_q [., NBDRF, N, N], bdrf_q0 [., NBDRF, N] and the arrays of
    ``thermal`` (as in ``pydisort_batch``) are per profile, or per column where they differ by g.
    surface=dict(model=..., params=[npar], [P, npar] or [P, G, npar], nphi=256) with NBDRF (default NFourier) instead of bdrf_q /
    bdrf_q0: a parametric surface model whose modes the device forms, as in ``pydisort_batch``; parameters per profile are shared by
    the profile's G columns on the device.
    NT_cor=True adds the Nakajima-Tanaka corrections to ``u`` before the spectral sum, their inputs formed on the device
    (``Plan.request_nt``): the mixture's full weighted phase function once per PROFILE ([P, L, NLeg_all] -- it does not depend on
    the spectral point), the IMS constants per column.  Needs delta_M, more moments in Leg_spec than NLeg, I0 > 0 in every column
    and mu0 away from the quadrature nodes (``ValueError``); not with ``thermal``; ignored with only_flux.
    lambert_sweep=True: as in ``pydisort_batch`` -- the band is solved over a black, non-emitting surface with a lit-from-below
    companion beside it (built through the same band mixture), and ``sol.lambert(albedo)`` returns the band over any list of
    Lambertian albedos, also one that follows the spectral point; the same exclusions (``ValueError``).
    Everything else as in ``pydisort_batch``.  Not combined with mode shards or communicators.
    Returns (mu_arr, BandSolution)."""
    if lambert_sweep:
        _lambert_refusals(bdrf_q, bdrf_q0, None, surface, None, b_pos, thermal, _defer_solve)
    prep, w, squeeze = _band_inputs(dtau_abs, dtau_spec, omega_spec, Leg_spec, NQuad, mu0, I0, phi0, weights, NLeg, NFourier, delta_M,
                                    only_flux, b_pos, b_neg, bdrf_q, bdrf_q0, thermal, surface, NBDRF)
    _check_numeric_errors(numeric_errors)
    if NT_cor and not only_flux:
        if not delta_M:
            raise ValueError("NT_cor needs delta_M: the corrections restore what the truncation removes.")
        if thermal is not None:
            raise ValueError("NT_cor is not combined with thermal in a band.")
        _nt_checks(prep["cols"]["I0"], prep["cols"]["mu0"], prep["N"], prep["P"], prep["band"]["leg_spec"].shape[1])
        prep["nt"] = prep["band"]["leg_spec"].shape[1]
    form, budget = _retention(retain, retain_bytes, _defer_solve, prep["C"], prep["N"], prep["M"], prep["L"], device)
    plan = Plan(prep, device=device, work_columns=work_columns, retain_bytes=budget, retain_form=form or 0)
    plan.numeric_errors = numeric_errors
    plan.set_band_weights(w)
    if not _defer_solve:
        plan.solve()
    G = w.shape[1]
    sol = BandSolution(plan, prep["C"] // G, G, squeeze)
    if lambert_sweep:
        if prep["thermal"] is not None:
            sol.columns._thermal_band = (prep["thermal"]["WVNMLO"], prep["thermal"]["WVNMHI"])
        Cn, N = prep["C"], prep["N"]
        cols_c = dict(mu0=np.ones(Cn), I0=np.zeros(Cn), phi0=np.zeros(Cn), b_pos=np.ones((Cn, 1, N)), b_neg=None, bdrf_q=None, bdrf_q0=None)
        prep_c = dict(prep, M=1, Ns=0, NBDRF=0, beam=False, cols=cols_c, thermal=None, surface=None, nt=0)
        _lambert_companion(sol.columns, prep_c, device, work_columns, budget, form, plan.prep["tau"][:, -1:])
    return sol.mu_arr, sol


def solve_band_streamed(dtau_abs, dtau_spec, omega_spec, Leg_spec, NQuad, mu0, I0, phi0, weights, levels=None, phi=None,
                        chunk_columns=0, NLeg=None, NFourier=None, delta_M=True, only_flux=False, b_pos=0, b_neg=0, bdrf_q=None,
                        bdrf_q0=None, thermal=None, device=0, numeric_errors="raise", *, actinic=False, mu=None,
                        view_corrections="interpolated", surface=None, NBDRF=None, NT_cor=False):
    """Throughput form of ``pydisort_band`` (as ``solve_columns_streamed`` is of ``pydisort_batch``): ONE plan holds the inputs
    and the results of all P G columns, the intermediates of the solve live for `chunk_columns` columns at a time, the results at
    `levels` (None: all L + 1) and `phi` are reduced on the device and only the P band results travel to the host -- 1 / G of what
    ``Plan.run_fetch`` moves, so no window-overlapped copy is needed.
    Returns dict(u [P, K, NQuad, nlev, nphi] (absent when only_flux), u0 [P, K, NQuad, nlev], flux_up, flux_down_diffuse,
    flux_down_direct [P, K, nlev], tau_arr [P, G, L]); the K axis is dropped when ``weights`` was [G].  actinic=True adds
    flux_act_up, flux_act_down_diffuse, flux_act_down_direct [P, K, nlev] (``Plan.fetch_band_actinic``).  NT_cor as in
    ``pydisort_band``: u is corrected per column on the device before it is reduced.  mu [nmu] or [P, nmu]: adds the band
    radiances at those polar-angle cosines, u_mu [P, K, nmu, nlev, nphi] (not with only_flux) and u0_mu [P, K, nmu, nlev]
    (``BandSolution.u_at``, ``Plan.fetch_band_view``); view_corrections="at_angles" evaluates the Nakajima-Tanaka corrections of u_mu
    at mu itself (``Plan.set_view``; the angles are then set before the run, which forms the view).  surface, NBDRF as in
    ``pydisort_band``."""
    if mu is not None:
        mu = view_angles(mu, np.shape(dtau_abs)[0] if np.ndim(dtau_abs) == 3 else 0, "P")
    at_angles = bool(_view_corrections(view_corrections, mu)) and mu is not None
    if chunk_columns <= 0:
        chunk_columns = _default_window(only_flux, NFourier, NLeg, NQuad)
    _, sol = pydisort_band(dtau_abs, dtau_spec, omega_spec, Leg_spec, NQuad, mu0, I0, phi0, weights, NLeg=NLeg, NFourier=NFourier,
                           delta_M=delta_M, only_flux=only_flux, b_pos=b_pos, b_neg=b_neg, bdrf_q=bdrf_q, bdrf_q0=bdrf_q0,
                           thermal=thermal, device=device, work_columns=chunk_columns, numeric_errors=numeric_errors, retain=False,
                           _defer_solve=True, NT_cor=NT_cor, surface=surface, NBDRF=NBDRF)
    plan = sol.plan
    try:
        phi = np.array([0.0]) if (only_flux or phi is None) else np.atleast_1d(np.asarray(phi, float))
        plan.set_eval_points(level_tau(plan.prep["tau"], levels), phi)
        if at_angles:
            sol._set_view(mu, view_corrections)
        plan.run()
        out = plan.fetch_band(want=("u0", "flux") if only_flux else ("u", "u0", "flux"))
        if actinic:
            out.update(plan.fetch_band_actinic())
        if mu is not None:
            if not at_angles:
                sol._set_view(mu)
            out.update(plan.fetch_band_view(("u0",) if only_flux else ("u", "u0")))
    finally:
        plan.close()
    out = {k: sol._out(v) for k, v in out.items() if v is not None}
    out["tau_arr"] = sol.tau_arr
    return out
