"""Thin object wrapper over a device plan (include/rtd.h): uploads prepared columns, launches the HIP
path, evaluates at (tau, phi).  Host arrays are NumPy float64; nothing here computes on the CPU."""
import ctypes as C

import numpy as np

from . import _lib


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def view_angles(mu, rows, axis="C"):
    """The polar-angle cosines of ``Plan.set_view`` checked on the host: [nmu] or [rows, nmu], every |mu| <= 1 (the reference's
    ``interpolate`` raises the same text) -> C-contiguous float64."""
    mu = _f64(np.atleast_1d(np.asarray(mu, dtype=np.float64)))
    if mu.ndim not in (1, 2) or mu.shape[-1] < 1 or (mu.ndim == 2 and mu.shape[0] != rows):
        raise ValueError(f"mu must have the shape [nmu] or [{axis} = {rows}, nmu] with nmu >= 1.")
    if not np.all(np.abs(mu) <= 1):
        raise ValueError("mu values must be between -1 and 1.")
    return mu


def view_corrections(corrections, mu=None):
    """The `corrections` keyword of ``Plan.set_view`` and of everything that passes it on -> the mode of rtd_plan_set_view_nt:
    "interpolated" 0, "at_angles" 1.  With mu (already through ``view_angles``) the one refusal of "at_angles" is made here, before
    the plan is touched: mu = 0 has no corrections of its own."""
    if corrections not in ("interpolated", "at_angles"):
        raise ValueError(f'corrections must be "interpolated" or "at_angles", not {corrections!r}.')
    mode = int(corrections == "at_angles")
    if mode and mu is not None and np.any(mu == 0):
        raise ValueError('mu = 0 is not accepted with corrections="at_angles": the limit differs by hemisphere.')
    return mode


_RESULT = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct")  # the C ABI's order of the result pointers
_THERMAL = ("TEMPER", "WVNMLO", "WVNMHI", "BTEMP", "TTEMP", "TEMIS", "emissivity")  # the fields of rtd_thermal, in their order


def _result_arrays(lead, Q, ntau, nphi, want=None):
    """The result dictionary of the fetches and evaluations: u `lead` + [Q, ntau, nphi], u0 `lead` + [Q, ntau], the three fluxes
    `lead` + [ntau].  want: what is allocated of ("u", "u0", "flux"), the rest is None, and so is u without azimuths; None: all of
    it, as the fetches of the stored points return it.  (``Plan.evaluate`` alone spells its arrays out: it is timed per call.)"""
    every = want is None
    field, level = lead + (Q, ntau), lead + (ntau,)
    fl = [np.empty(level) if every or "flux" in want else None for _ in range(3)]
    return {"u": np.empty(field + (nphi,)) if every or ("u" in want and nphi > 0) else None,
            "u0": np.empty(field) if every or "u0" in want else None, "flux_up": fl[0], "flux_down_diffuse": fl[1], "flux_down_direct": fl[2]}


def _out_int(fn, *args, ctype=C.c_int64):
    """The integer that a C entry point returns through its last argument."""
    b = ctype()
    _lib.check(fn(*args, C.byref(b)))
    return b.value


def _result_ptrs(out):
    """The five result pointers of the C ABI, in its order, from a result dictionary (a missing or None entry: NULL)."""
    return [_lib.dptr(out.get(k)) for k in _RESULT]


def _out_arrays(given, shapes):
    """name -> array of the shape `shapes` gives it: the caller's own of `given` (dict or None), checked and to be filled in place,
    else freshly allocated."""
    out = {}
    for k, shape in shapes.items():
        a = given.get(k) if given else None
        if a is None:
            a = np.empty(shape)
        elif not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable and a.shape == shape):
            raise ValueError(f"out[{k!r}] must be a writeable C-contiguous float64 array of the shape {shape}.")
        out[k] = a
    return out


def lambert_arrays(albedo, rows_ok, fdown_bottom, sph_albedo, emission, Cn):
    """The small arrays of a Lambertian sweep checked on the host, before the library sees them: albedo [A] or [rows, A] with rows in
    `rows_ok` and every value in [0, 1]; fdown_bottom, sph_albedo [C]; emission a scalar or [C], finite and not negative, or None
    -> (albedo, F, s, E) as C-contiguous float64 (E None: no emission)."""
    alb = _f64(np.atleast_1d(np.asarray(albedo, dtype=np.float64)))
    if alb.ndim not in (1, 2) or alb.shape[-1] < 1 or (alb.ndim == 2 and alb.shape[0] not in rows_ok):
        raise ValueError(f"albedo must have the shape [A] or [rows, A] with rows in {sorted(set(rows_ok))} and A >= 1.")
    if not np.all((alb >= 0) & (alb <= 1)):
        raise ValueError("albedo values must be between 0 and 1.")
    F, s = _f64(fdown_bottom), _f64(sph_albedo)
    if F is None or s is None or F.shape != (Cn,) or s.shape != (Cn,):
        raise ValueError(f"fdown_bottom and sph_albedo must have the shape [C = {Cn}].")
    E = None
    if emission is not None:
        E = np.asarray(emission, dtype=np.float64)
        if E.ndim > 1 or (E.ndim == 1 and E.shape != (Cn,)):
            raise ValueError(f"emission must be a scalar or [C = {Cn}].")
        E = _f64(np.broadcast_to(E, (Cn,)))
        if not np.all((E >= 0) & np.isfinite(E)):
            raise ValueError("emission must be finite and not negative.")
    return alb, F, s, E


def _thermal_struct(thermal, Cn, L, N):
    """The thermal dict of ``Plan.set_columns_thermal`` checked against the plan's (C, L, N) -> (rtd_thermal, the arrays it points
    into: they must outlive the call that takes the struct)."""
    shapes = dict(zip(_THERMAL, ((Cn, L + 1), (Cn,), (Cn,), (Cn,), (Cn,), (Cn,), (Cn, N))))
    t = {k: _f64(thermal.get(k)) for k in _THERMAL}
    for k, shape in shapes.items():
        if t[k] is None:
            if k in _THERMAL[:3]:
                raise ValueError(f"thermal batch does not match the plan: {k} is required")
        elif t[k].shape != shape:
            raise ValueError(f"thermal batch does not match the plan: {k} has the shape {t[k].shape}, expected {shape}")
    return _lib.rtd_thermal(*[_lib.dptr(t[k]) for k in _THERMAL]), t


class Plan:
    def __init__(self, prep, device=0, work_columns=0, retain_bytes=0, retain_form=0):
        """prep: dict from _prepare.prepare_columns.  work_columns: columns whose intermediates are resident at a time
        (0: sized by the library, include/rtd.h: rtd_plan_create_windowed).  retain_bytes: budget for keeping what the
        evaluators need of a solve for ALL columns of a plan of several windows, so that evaluate() does not solve again
        (include/rtd.h: rtd_plan_create_retained; -1: three tenths of the free device memory, 0: never -- the throughput form).
        retain_form: 0 the full state, else the lean one (coefficients, k, E, B; Y, A recomputed per evaluation), 1 full only,
        2 lean (rtd_plan_create_retained_form)."""
        lib = _lib.load()
        self._lib = lib
        self.device = int(device)
        # What later calls read, with its "nothing yet" value (the uploads below set some of it, so it comes first).
        self.solved = False        # solve / run / run_fetch / solve_bc; every upload and shard call clears it
        self._ev_shape = None      # (ntau, nphi) of the stored points: set_eval_points, evaluate_band
        self._band = None          # (P, K): set_band_weights
        self._view = None          # nmu: set_view
        self._view_nt = 0          # set_view(corrections=): the mode of rtd_plan_set_view_nt the plan is in
        self._surface = None       # (model id, nphi, rows): request_surface
        self._sharded = False      # set_mode_shard
        self._nranks = None        # comm_init
        self._nt_request = 0       # request_nt
        self._nt_nleg_all = 0      # set_nt, or the set_columns_raw / _thermal / _band that met a request
        self._nt_on = False        # pydisort.py: the corrections are switched on for the closures of the current call
        self._idle_key = None      # pydisort.py: _plan_for, the shape under which the plan waits for a next call
        self.prep = prep
        self.C, self.L, self.N, self.Q = prep["C"], prep["L"], prep["N"], 2 * prep["N"]
        self.M = prep["M"]
        dims = _lib.rtd_dims(prep["C"], prep["L"], 2 * prep["N"], prep["P"], prep["M"], prep["Ns"],
                             prep["NBDRF"], int(prep["beam"]))
        h = C.c_void_p()
        _lib.check(lib.rtd_plan_create_retained_form(C.byref(dims), device, int(work_columns), int(retain_bytes), int(retain_form), C.byref(h)))
        self._h = h
        mu, w = _f64(prep["mu"]), _f64(prep["W"])
        _lib.check(lib.rtd_plan_set_quadrature(h, _lib.dptr(mu), _lib.dptr(w)))
        if prep.get("nt"):
            self.request_nt(prep["nt"])
        if prep.get("surface") is not None:
            self.request_surface(prep["surface"]["model"], prep["surface"]["params"], prep["surface"]["nphi"])
        if prep.get("band") is not None:
            self.set_columns_band(prep["band"], prep["cols"], prep.get("thermal"))
        elif prep.get("raw") is not None and prep.get("thermal") is not None:
            self.set_columns_thermal(prep["raw"], prep["thermal"])
        elif prep.get("raw") is not None:
            self.set_columns_raw(prep["raw"])
        else:
            self.set_columns(prep)
        if prep.get("mode_shard") is not None:
            self.set_mode_shard(*prep["mode_shard"])

    def set_mode_shard(self, first, stride, total):
        """The plan's M local Fourier modes stand for the modes first, first + stride, ... of `total`
        (include/rtd.h: rtd_plan_set_mode_shard); evaluators then return this shard's partial sums."""
        if self._band_active() and (int(first), int(stride), int(total)) != (0, 1, self.M):
            raise ValueError("a mode shard is not combined with band inputs or band weights.")
        _lib.check(self._lib.rtd_plan_set_mode_shard(self._h, int(first), int(stride), int(total)))
        self._sharded = (int(first), int(stride), int(total)) != (0, 1, self.M)
        self.solved = False

    def _band_active(self):
        return self.prep.get("band") is not None or self._band is not None

    def _band_allowed(self):
        if self._sharded or self._nranks is not None:
            raise ValueError("band inputs and band weights are not combined with a mode shard or a communicator.")

    def allreduce_results(self):
        """RCCL all-reduce (sum) of the results of run() over the ranks of the communicator (mode shards)."""
        _lib.check(self._lib.rtd_comm_allreduce_results(self._h))

    def set_columns(self, prep):
        """Upload the prepared per-column inputs (same dimensions as the plan): a plan can be reused for many batches.
        A plan created without a beam source skips the beam terms on the device, so a batch that has one is refused
        (and a batch without one for a plan with one is fine: its beam terms are zero)."""
        for k in ("C", "L", "N", "P", "M", "Ns", "NBDRF"):
            if prep[k] != self.prep[k]:
                raise ValueError(f"prepared batch does not match the plan: {k} = {prep[k]} vs {self.prep[k]}")
        if prep["beam"] and not self.prep["beam"]:
            raise ValueError("prepared batch has a beam source but the plan was created without one")
        keys = ["omega_s", "tau", "tau_s0", "scale_tau", "wleg", "mu0", "I0", "phi0", "rescale",
                "b_pos", "b_neg", "s_s", "bdrf_q", "bdrf_q0"]
        local = prep.get("s_local") is not None  # the thermal polynomials about their layers' tops (_prepare.py)
        if local:
            keys[keys.index("s_s")] = "s_local"
        arrs = [_f64(prep[k]) for k in keys]
        setter = self._lib.rtd_plan_set_columns_local if local else self._lib.rtd_plan_set_columns
        _lib.check(setter(self._h, *[_lib.dptr(a) for a in arrs]))
        self.prep = prep
        self.solved = False

    def set_columns_thermal(self, raw, thermal):
        """``set_columns_raw`` with the isotropic source and the boundary emissions formed on the device from temperatures
        (include/rtd.h: rtd_plan_set_columns_thermal; the plan needs Ns = 2).  raw: as there, without s_poly.  thermal:
        dict(TEMPER [C, L + 1], WVNMLO, WVNMHI [C], BTEMP, TTEMP, TEMIS [C] or None, emissivity [C, N] or None)."""
        self.set_columns_raw(raw, thermal)

    def set_columns_raw(self, raw, _thermal=None):
        """Upload a batch as the user gave it; delta-M scaling and source rescaling run on the device
        (include/rtd.h: rtd_plan_set_columns_raw).  raw: dict(tau_arr, omega_arr, f_arr [C, L], leg [C, L, nleg_all],
        mu0, I0, phi0 [C], b_pos / b_neg [C, M, N] or None, s_poly [C, L, Ns] or None, bdrf_q [C, NBDRF, N, N],
        bdrf_q0 [C, NBDRF, N] or None).  The C ABI takes bare pointers whose extents the plan implies, so every
        array's shape is checked here."""
        names = ("tau_arr", "omega_arr", "leg", "f_arr", "mu0", "I0", "phi0", "b_pos", "b_neg", "s_poly", "bdrf_q", "bdrf_q0")
        a = {k: _f64(raw.get(k)) for k in names}
        p = self.prep
        self._check_columns(a, {"tau_arr", "omega_arr", "f_arr", "mu0", "I0", "phi0"} | ({"s_poly"} if p["Ns"] > 0 and _thermal is None else set()), "raw")
        if _thermal is None:
            _lib.check(self._lib.rtd_plan_set_columns_raw(
                self._h, _lib.dptr(a["tau_arr"]), _lib.dptr(a["omega_arr"]), _lib.dptr(a["leg"]), a["leg"].shape[2],
                *[_lib.dptr(a[k]) for k in ("f_arr", "mu0", "I0", "phi0", "b_pos", "b_neg", "s_poly", "bdrf_q", "bdrf_q0")]))
        else:
            if p["Ns"] != 2 or a["s_poly"] is not None:
                raise ValueError("thermal batch does not match the plan: it needs Ns = 2 and no s_poly")
            th, keep = _thermal_struct(_thermal, p["C"], p["L"], p["N"])
            _lib.check(self._lib.rtd_plan_set_columns_thermal(
                self._h, _lib.dptr(a["tau_arr"]), _lib.dptr(a["omega_arr"]), _lib.dptr(a["leg"]), a["leg"].shape[2],
                *[_lib.dptr(a[k]) for k in ("f_arr", "mu0", "I0", "phi0", "b_pos", "b_neg", "bdrf_q", "bdrf_q0")], C.byref(th)))
        # what later checks (set_columns, the closures' tau range, beam terms) compare against follows the new batch
        self.prep = dict(p, tau=a["tau_arr"], mu0=a["mu0"], phi0=a["phi0"], raw=raw, thermal=_thermal, band=None)
        if self._nt_request:
            self._nt_nleg_all = self._nt_request
        self.solved = False

    def _check_columns(self, a, required, label):
        """The per-column arrays `a` of a raw or band upload (name -> array, None: not given) against the shapes the plan implies;
        `label`: "raw" or "band".  `required`: what must be given besides the BDRF tables, which are required when the plan has BDRF
        modes and no surface is requested, and refused when one is.  An array of a term the plan does not have becomes None in `a`
        (the library ignores the pointer).  "leg", where `a` has it, is [C, L, nleg_all >= NLeg]."""
        p = self.prep
        Cn, L, N, M, Ns, NB = p["C"], p["L"], p["N"], p["M"], p["Ns"], p["NBDRF"]
        shapes = {"tau_arr": (Cn, L), "omega_arr": (Cn, L), "f_arr": (Cn, L), "mu0": (Cn,), "I0": (Cn,), "phi0": (Cn,),
                  "b_pos": (Cn, M, N), "b_neg": (Cn, M, N), "s_poly": (Cn, L, Ns), "bdrf_q": (Cn, NB, N, N), "bdrf_q0": (Cn, NB, N)}
        requested = self._surface is not None
        if requested and (a["bdrf_q"] is not None or a["bdrf_q0"] is not None):
            raise ValueError(f"{label} batch does not match the plan: a surface is requested, bdrf_q and bdrf_q0 must be None")
        if "leg" in a and (a["leg"] is None or a["leg"].ndim != 3 or a["leg"].shape[:2] != (Cn, L) or a["leg"].shape[2] < p["P"]):
            raise ValueError(f"{label} batch does not match the plan: leg must be [C = {Cn}, L = {L}, nleg_all >= {p['P']}]")
        if NB > 0 and not requested:
            required = required | {"bdrf_q", "bdrf_q0"}
        for k, shape in shapes.items():
            if k not in a:
                continue
            if a[k] is None:
                if k in required:
                    raise ValueError(f"{label} batch does not match the plan: {k} is required")
            elif (k == "s_poly" and Ns == 0) or (k.startswith("bdrf") and NB == 0):
                a[k] = None
            elif a[k].shape != shape:
                raise ValueError(f"{label} batch does not match the plan: {k} has the shape {a[k].shape}, expected {shape}")
        if not p["beam"] and np.any(a["I0"] > 0):
            raise ValueError(f"{label} batch has a beam source but the plan was created without one")

    def set_columns_band(self, band, cols, thermal=None):
        """Upload a batch of P profiles x G spectral points as a k-distribution band; tau_arr, omega_arr, f_arr and the moments of
        the P G columns (column p G + g) are mixed on the device (include/rtd.h: rtd_plan_set_columns_band).
        band: dict(dtau_abs [P, G, L], dtau_spec [P, L, S], omega_spec [P, L, S], leg_spec [S, nleg_all], delta_m).
        cols: dict(mu0, I0, phi0 [C], b_pos / b_neg [C, M, N] or None, bdrf_q [C, NBDRF, N, N], bdrf_q0 [C, NBDRF, N] or None).
        thermal: as in ``set_columns_thermal`` (the plan then needs Ns = 2).  Returns the mixed tau_arr [C, L] as the device formed
        it.  The C ABI takes bare pointers whose extents the plan implies, so every array's shape is checked here."""
        self._band_allowed()
        p = self.prep
        Cn, L, Ns = p["C"], p["L"], p["Ns"]
        b = {k: _f64(band.get(k)) for k in ("dtau_abs", "dtau_spec", "omega_spec", "leg_spec")}
        if any(v is None for v in b.values()) or b["dtau_abs"].ndim != 3 or b["dtau_spec"].ndim != 3 or b["leg_spec"].ndim != 2:
            raise ValueError("band does not match the plan: dtau_abs [P, G, L], dtau_spec and omega_spec [P, L, S] and leg_spec "
                             "[S, nleg_all] are required")
        P, G, _ = b["dtau_abs"].shape
        S, nleg_all = b["leg_spec"].shape
        delta_m = bool(band.get("delta_m"))
        if P * G != Cn or b["dtau_abs"].shape != (P, G, L):
            raise ValueError(f"band does not match the plan: dtau_abs has the shape {b['dtau_abs'].shape}, expected [P, G, {L}] with P G = {Cn}")
        for k in ("dtau_spec", "omega_spec"):
            if b[k].shape != (P, L, S) or S < 1:
                raise ValueError(f"band does not match the plan: {k} has the shape {b[k].shape}, expected {(P, L, S)} with S >= 1")
        if nleg_all < p["P"] + int(delta_m):
            raise ValueError(f"band does not match the plan: leg_spec needs {p['P'] + int(delta_m)} moments per species, has {nleg_all}")
        a = {k: _f64(cols.get(k)) for k in ("mu0", "I0", "phi0", "b_pos", "b_neg", "bdrf_q", "bdrf_q0")}
        self._check_columns(a, {"mu0", "I0", "phi0"}, "band")
        th, keep = None, None
        if thermal is not None:
            if Ns != 2:
                raise ValueError("thermal batch does not match the plan: it needs Ns = 2")
            ts, keep = _thermal_struct(thermal, Cn, L, p["N"])
            th = C.byref(ts)
        elif Ns != 0:
            raise ValueError("band batch does not match the plan: a plan with Ns > 0 needs thermal")
        bs = _lib.rtd_band(P, G, S, nleg_all, int(delta_m), *[_lib.dptr(b[k]) for k in ("dtau_abs", "dtau_spec", "omega_spec", "leg_spec")])
        tau = np.empty((Cn, L))
        _lib.check(self._lib.rtd_plan_set_columns_band(
            self._h, C.byref(bs), *[_lib.dptr(a[k]) for k in ("mu0", "I0", "phi0", "b_pos", "b_neg", "bdrf_q", "bdrf_q0")], th, _lib.dptr(tau)))
        self.prep = dict(p, tau=tau, mu0=a["mu0"], phi0=a["phi0"], band=band, cols=cols, thermal=thermal, raw=None)
        if self._nt_request:
            self._nt_nleg_all = self._nt_request
        self.solved = False
        return tau

    def set_band_weights(self, weights):
        """Spectral integration of the results on the device (include/rtd.h: rtd_plan_set_band_weights): weights [K, G], the
        columns p G ... p G + G - 1 are the spectral points of profile p.  None switches it off."""
        if weights is None:
            _lib.check(self._lib.rtd_plan_set_band_weights(self._h, 0, 0, None))
            self._band = None
            return
        self._band_allowed()
        w = _f64(weights)
        if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] < 1 or self.C % w.shape[1] != 0:
            raise ValueError(f"weights must be [K, G] with K >= 1 and G dividing the {self.C} columns of the plan.")
        _lib.check(self._lib.rtd_plan_set_band_weights(self._h, w.shape[1], w.shape[0], _lib.dptr(w)))
        self._band = (self.C // w.shape[1], w.shape[0])

    @staticmethod
    def _after(state, setter, caller):
        """What `setter` left in the plan's `state`, for a `caller` that needs it; the refusal of one that came before it."""
        if state is None:
            raise ValueError(f"{setter} must precede {caller}.")
        return state

    def _stored_points(self, caller):
        return self._after(self._ev_shape, "set_eval_points", caller)

    def _band_shape(self, caller):
        return self._after(self._band, "set_band_weights", caller)

    def _checked_band(self, rc):
        """The device has already written NaN into every profile with a failed column: numeric_errors == "nan" only has to keep
        the status from being raised."""
        if not (rc == _lib.RTD_ERR_NUMERIC and self.numeric_errors == "nan"):
            _lib.check(rc)

    def fetch_band(self, want=("u", "u0", "flux")):
        """After run(): the results at the stored points summed over the spectral points with every weight set, on the device
        (include/rtd.h: rtd_plan_fetch_band) -> dict(u [P, K, Q, ntau, nphi], u0 [P, K, Q, ntau], flux_up / flux_down_diffuse /
        flux_down_direct [P, K, ntau]); what `want` leaves out is neither reduced nor copied (None).  A profile with a failed
        column is NaN (numeric_errors == "nan") or raises NumericalError."""
        ntau, nphi = self._stored_points("fetch_band")
        out = _result_arrays(self._band_shape("fetch_band / evaluate_band"), self.Q, ntau, nphi, want)
        self._checked_band(self._lib.rtd_plan_fetch_band(self._h, *_result_ptrs(out)))
        return out

    def evaluate_band(self, tau, phi=None, antiderivative=False, want=("u", "u0", "flux"), skip_nt=False, derivative=False):
        """``evaluate`` without copying the unreduced fields out: tau [C, ntau] (the t-th point of each of a profile's columns must
        be the same physical level), phi [nphi] or None -> the dict of ``fetch_band`` (include/rtd.h: rtd_plan_evaluate_band);
        "act" in `want` adds the reduced actinic fluxes of ``fetch_band_actinic``, "view" the reduced radiances at the angles of
        ``set_view`` (``fetch_band_view``; "view_u" / "view_u0": one of the two)."""
        tau, ntau, phi, nphi, flags, view = self._eval_args(tau, phi, antiderivative, derivative, skip_nt, want)
        out = _result_arrays(self._band_shape("fetch_band / evaluate_band"), self.Q, ntau, nphi, want)
        self._ev_shape = (ntau, nphi)
        self._checked_band(self._lib.rtd_plan_evaluate_band(self._h, ntau, _lib.dptr(tau), nphi, _lib.dptr(phi), flags, *_result_ptrs(out)))
        if "act" in want:
            out.update(self.fetch_band_actinic())
        if view:
            out.update(self.fetch_band_view(view))
        return out

    _ACT = ("flux_act_up", "flux_act_down_diffuse", "flux_act_down_direct")

    def _resident_ntau(self):
        """Points per column of the results the plan holds now, as the plan itself reports it (include/rtd.h:
        rtd_plan_result_dev_ptrs, flux_bytes = 3 C ntau 8).  The host arrays of the actinic fetches are sized from this and from
        nothing this object remembers: evaluate() moves the plan's points without a fetch of the stored ones in mind."""
        return self._resident_shape()[0]

    def fetch_actinic(self, out=None):
        """Actinic fluxes (4 pi x the mean intensity) of the results the plan holds -- after run(), run_fetch(), evaluate() or
        evaluate_band(), whatever their `want`, at the points and in the order (value, antiderivative, derivative) of the latest
        of them -- formed on the device from the resident u0 (include/rtd.h: rtd_plan_fetch_actinic) -> dict(flux_act_up,
        flux_act_down_diffuse, flux_act_down_direct [C, ntau]); diffuse + direct is the physical downward actinic flux.  `out`:
        dict whose arrays of those names are filled in place (C-contiguous float64 [C, ntau], anything else is a ValueError);
        the others are allocated."""
        out = _out_arrays(out, dict.fromkeys(self._ACT, (self.C, self._resident_ntau())))
        self._checked(self._lib.rtd_plan_fetch_actinic(self._h, *[_lib.dptr(out[k]) for k in self._ACT]), out)
        return out

    def fetch_band_actinic(self):
        """``fetch_actinic`` summed over the spectral points with every weight set on the device (include/rtd.h:
        rtd_plan_fetch_band_actinic) -> the same keys, [P, K, ntau].  With weights = cross section x quantum yield x k-weight the sum
        of the three is the photolysis rate per level."""
        shape = self._band_shape("fetch_band_actinic") + (self._resident_ntau(),)
        out = {k: np.empty(shape) for k in self._ACT}
        self._checked_band(self._lib.rtd_plan_fetch_band_actinic(self._h, *[_lib.dptr(out[k]) for k in self._ACT]))
        return out

    _VIEW = ("u_mu", "u0_mu")

    def set_view(self, mu, *, corrections="interpolated"):
        """Polar-angle cosines at which ``fetch_view`` / ``fetch_band_view`` (and "view" in the `want` of ``evaluate`` /
        ``evaluate_band``) return the radiances: mu [nmu] shared by the columns, or [C, nmu]; None withdraws the request
        (include/rtd.h: rtd_plan_set_view_mu).  mu > 0 is interpolated among the upward rows of u, every other mu -- 0 included --
        among the downward rows, as the reference's ``subroutines.interpolate`` does.  Sticky across solves and evaluations.
        Under band weights, angles given per column must be the same for the columns of a profile.
        corrections (keyword-only; include/rtd.h: rtd_plan_set_view_nt): "interpolated" (default) -- the Nakajima-Tanaka corrected u
        of the nodes is interpolated; "at_angles" -- the uncorrected u is interpolated and TMS + IMS are evaluated at the angles
        themselves, which is what resolves the solar aureole and glint geometry.  Then mu = 0 is a ValueError, and the view of u is
        formed by the NEXT evaluation: ``fetch_view`` for u_mu before it is an error.  Ignored by a plan without corrections."""
        if mu is not None:
            mu = view_angles(mu, self.C)
        mode = view_corrections(corrections, mu)
        if mode == 0:
            self._set_view_nt(0)  # (before the angles: a zero among them is refused while the plan is in the other mode)
        if mu is None:
            _lib.check(self._lib.rtd_plan_set_view_mu(self._h, 0, None, 0))
            self._view = None
            return
        if mu.ndim == 2 and self._band is not None:
            per_profile = mu.reshape(self._band[0], self.C // self._band[0], -1)
            if not np.array_equal(per_profile, np.broadcast_to(per_profile[:, :1], per_profile.shape)):
                raise ValueError("mu must be the same for the columns of a band profile.")
        _lib.check(self._lib.rtd_plan_set_view_mu(self._h, mu.shape[-1], _lib.dptr(mu), int(mu.ndim == 2)))
        self._view = mu.shape[-1]
        self._set_view_nt(mode)

    def _set_view_nt(self, mode):
        """The plan's mode of rtd_plan_set_view_nt, changed only when it differs: a plan that never asks makes no call for it."""
        if mode != self._view_nt:
            _lib.check(self._lib.rtd_plan_set_view_nt(self._h, mode))
            self._view_nt = mode

    def _resident_shape(self):
        """(ntau, nphi) of the results the plan holds now, as the plan itself reports them (``_resident_ntau``; u_bytes =
        C Q ntau nphi 8)."""
        ub, fb = C.c_int64(), C.c_int64()
        _lib.check(self._lib.rtd_plan_result_dev_ptrs(self._h, None, C.byref(ub), None, C.byref(fb)))
        ntau = int(fb.value // (24 * self.C))
        return ntau, (int(ub.value // (8 * self.C * self.Q * ntau)) if ntau > 0 else 0)

    def _view_arrays(self, lead, want, out):
        """The host arrays of the two view fetches: `lead` + (nmu, ntau[, nphi]).  u_mu is None when "u" is not wanted or the
        resident results have no azimuths; arrays of `out` are checked and filled in place, the others allocated."""
        nmu = self._after(self._view, "set_view", "fetch_view / fetch_band_view")
        ntau, nphi = self._resident_shape()
        shapes = {}
        if "u" in want and nphi > 0:
            shapes["u_mu"] = lead + (nmu, ntau, nphi)
        if "u0" in want:
            shapes["u0_mu"] = lead + (nmu, ntau)
        return dict(dict(u_mu=None, u0_mu=None), **_out_arrays(out, shapes))

    def fetch_view(self, want=("u", "u0"), out=None):
        """Radiances at the angles of ``set_view`` of the results the plan holds -- after run(), run_fetch(), evaluate() or
        evaluate_band(), at the points and in the order (value, antiderivative, derivative) of the latest of them -- interpolated
        on the device from the resident u and u0 (include/rtd.h: rtd_plan_fetch_view) -> dict(u_mu [C, nmu, ntau, nphi],
        u0_mu [C, nmu, ntau]); what `want` leaves out is None, and so is u_mu when the results have no azimuths.  `out`: dict whose
        arrays of those names are filled in place (C-contiguous float64 of those shapes, anything else is a ValueError)."""
        arrays = self._view_arrays((self.C,), want, out)
        self._checked(self._lib.rtd_plan_fetch_view(self._h, _lib.dptr(arrays["u_mu"]), _lib.dptr(arrays["u0_mu"])), arrays)
        return arrays

    def fetch_band_view(self, want=("u", "u0")):
        """``fetch_view`` summed over the spectral points with every weight set on the device (include/rtd.h:
        rtd_plan_fetch_band_view) -> dict(u_mu [P, K, nmu, ntau, nphi], u0_mu [P, K, nmu, ntau])."""
        arrays = self._view_arrays(self._band_shape("fetch_band_view"), want, None)
        self._checked_band(self._lib.rtd_plan_fetch_band_view(self._h, _lib.dptr(arrays["u_mu"]), _lib.dptr(arrays["u0_mu"])))
        return arrays

    def evaluate_resident(self, tau, phi=None, antiderivative=False, derivative=False, keep_u=False):
        """``evaluate`` into the plan's device buffers with nothing copied out: for ``couple_lambert`` behind it.  keep_u: u is formed
        on the device (bit 3 of the flag word; needs azimuths).  A numerical failure is raised, or left to the call that reads the
        buffers under numeric_errors == "nan"."""
        tau, ntau, phi, nphi, flags, _ = self._eval_args(tau, phi, antiderivative, derivative, False, ())
        self._checked_band(self._lib.rtd_plan_evaluate(self._h, ntau, _lib.dptr(tau), nphi, _lib.dptr(phi),
                                                       flags | (8 if keep_u and nphi > 0 else 0), *[None] * 6))

    def _couple_lambert(self, fn, lead, rows_ok, companion, albedo, fdown_bottom, sph_albedo, emission, want):
        """What ``couple_lambert`` and ``couple_lambert_band`` share: the checks of the small arrays, the host arrays `lead` +
        (A, ...) of what `want` names, the call."""
        if not isinstance(companion, Plan) or (companion.C, companion.L, companion.N) != (self.C, self.L, self.N):
            raise ValueError("couple_lambert: the companion must be a Plan of the same columns, layers and streams.")
        alb, F, s, E = lambert_arrays(albedo, rows_ok, fdown_bottom, sph_albedo, emission, self.C)
        ntau, nphi = self._resident_shape()
        A = alb.shape[-1]
        view = self._view_want(want)
        nmu = self._after(self._view, "set_view", "couple_lambert with a view") if view else 0
        shapes = {"u": (self.Q, ntau, nphi) if "u" in want and nphi > 0 else None, "u0": (self.Q, ntau) if "u0" in want else None,
                  "flux_up": (ntau,) if "flux" in want else None, "flux_down_diffuse": (ntau,) if "flux" in want else None,
                  "u_mu": (nmu, ntau, nphi) if "u" in view and nphi > 0 else None, "u0_mu": (nmu, ntau) if "u0" in view else None}
        out = {k: None if shp is None else np.empty(lead + (A,) + shp) for k, shp in shapes.items()}
        self._checked_band(fn(self._h, companion._h, A, _lib.dptr(alb), alb.shape[0] if alb.ndim == 2 else 1, _lib.dptr(F), _lib.dptr(s),
                              _lib.dptr(E), *[_lib.dptr(out[k]) for k in shapes]))
        return out

    def couple_lambert(self, companion, albedo, fdown_bottom, sph_albedo, emission=None, want=("u", "u0", "flux")):
        """Lambertian albedo sweep (include/rtd.h: rtd_plan_couple_lambert): this plan solved over a BLACK surface, `companion` the
        same layers without a source lit from below by unit isotropic intensity (M = 1, no beam), both evaluated at the same points
        in the same tau-order; the LATEST evaluations the two hold are coupled on the device, x_black + kappa(A) x_below.
        albedo [A] or [C, A]; fdown_bottom, sph_albedo [C]: flux_down (diffuse + direct, value order) of this plan at the bottom and
        flux_down of the companion there over pi; emission: scalar or [C] or None.  want: "u", "u0", "flux", and "view" / "view_u" /
        "view_u0" with ``set_view`` on both plans -> dict(u [C, A, Q, ntau, nphi], u0 [C, A, Q, ntau], flux_up, flux_down_diffuse
        [C, A, ntau], u_mu [C, A, nmu, ntau, nphi], u0_mu [C, A, nmu, ntau]); what `want` leaves out is None.  A failed column (of
        either plan) is NaN (numeric_errors == "nan") or raises NumericalError."""
        return self._couple_lambert(self._lib.rtd_plan_couple_lambert, (self.C,), (self.C,), companion, albedo, fdown_bottom, sph_albedo,
                                    emission, want)

    def couple_lambert_band(self, companion, albedo, fdown_bottom, sph_albedo, emission=None, want=("u", "u0", "flux")):
        """``couple_lambert`` before the sum over the spectral points with every weight set of this plan (include/rtd.h:
        rtd_plan_couple_lambert_band): albedo [A], [P, A] or [C = P G, A] (a spectral albedo) -> the same keys, [P, K, A, ...]."""
        P, K = self._band_shape("couple_lambert_band")
        return self._couple_lambert(self._lib.rtd_plan_couple_lambert_band, (P, K), (P, self.C), companion, albedo, fdown_bottom,
                                    sph_albedo, emission, want)

    @staticmethod
    def _view_want(want):
        """"view" in `want` asks for both u_mu and u0_mu, "view_u" / "view_u0" for one -> the `want` of the view fetches."""
        return tuple(k for k, names in (("u", ("view", "view_u")), ("u0", ("view", "view_u0"))) if any(n in want for n in names))

    def close(self):
        # (probed, like nothing else of the plan's: __init__ can fail before the handle exists, and __del__ still comes here)
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rtd_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_bdrf_samples(self, rho_qq, rho_q0=None):
        """Form the plan's NBDRF BDRF Fourier modes on the device from samples of the reflectance on a uniform grid
        of relative azimuths dphi_p = 2 pi p / nphi:  rho_qq [C, N, N, nphi] = rho(mu_i, mu_j, dphi_p) and, with a
        beam, rho_q0 [C, N, nphi] = rho(mu_i, mu0, dphi_p).  Replaces the tables given to ``set_columns``."""
        Cn, N = self.prep["C"], self.prep["N"]
        rho_qq = _f64(rho_qq)
        if rho_qq.ndim != 4 or rho_qq.shape[:3] != (Cn, N, N):
            raise ValueError("rho_qq must have the shape [C, N, N, nphi].")
        nphi = rho_qq.shape[3]
        q0 = None
        if rho_q0 is not None:
            q0 = _f64(rho_q0)
            if q0.shape != (Cn, N, nphi):
                raise ValueError("rho_q0 must have the shape [C, N, nphi].")
        _lib.check(self._lib.rtd_plan_set_bdrf_samples(self._h, nphi, _lib.dptr(rho_qq), _lib.dptr(q0) if q0 is not None else None))
        self.solved = False

    def set_nt(self, weighted_leg_all, f_arr, ims_coef, ims_par):
        """Enable device-side Nakajima-Tanaka corrections of `u` (arrays with a leading column axis)."""
        a = [_f64(v) for v in (weighted_leg_all, f_arr, ims_coef, ims_par)]
        _lib.check(self._lib.rtd_plan_set_nt(self._h, a[0].shape[-1], *[_lib.dptr(v) for v in a]))
        self._nt_nleg_all = a[0].shape[-1]

    def clear_nt(self):
        _lib.check(self._lib.rtd_plan_set_nt(self._h, 0, None, None, None, None))

    def request_nt(self, nleg_all):
        """While nleg_all > 0 is requested, ``set_columns_raw`` / ``_thermal`` / ``_band`` also form the inputs of the
        Nakajima-Tanaka corrections on the device and switch them on (include/rtd.h: rtd_plan_request_nt); nleg_all is the number
        of moments of the raw batch, or of the band's species.  0 withdraws the request."""
        _lib.check(self._lib.rtd_plan_request_nt(self._h, int(nleg_all)))
        self._nt_request = max(int(nleg_all), 0)

    def request_surface(self, model, params=None, nphi=256):
        """While a surface is requested, ``set_columns_raw`` / ``_thermal`` / ``_band`` form the plan's BDRF Fourier modes on the
        device from a parametric model instead of taking ``bdrf_q`` / ``bdrf_q0`` (include/rtd.h: rtd_plan_request_surface; the
        plan needs NBDRF > 0).  model: "lambert" | "hapke" | "rossli" | "rpv" | "ocean", or the id of include/rtd.h; params [npar] or
        [rows, npar] (padded to 4 with zeros) with rows = 1, C or -- for a band -- P; nphi: azimuth samples per pair of cosines.
        model=None withdraws the request.  The host-prepared ``set_columns`` is refused while a request is set."""
        from . import _surface
        if model is None:
            _lib.check(self._lib.rtd_plan_request_surface(self._h, None))
            self._surface = None
            return
        if isinstance(model, str):
            if model.lower() not in _surface.MODELS:
                raise ValueError(f"surface: unknown model {model!r} (known: {', '.join(_surface.MODELS)}).")
            model = _surface.MODELS[model.lower()][0]
        p = np.atleast_2d(np.asarray(params, dtype=np.float64))
        if p.ndim != 2 or not 1 <= p.shape[1] <= 4:
            raise ValueError("surface: params must be [npar] or [rows, npar] with npar <= 4.")
        p4 = np.zeros((p.shape[0], 4))
        p4[:, :p.shape[1]] = p
        sf = _lib.rtd_surface(int(model), int(nphi), p4.shape[0], _lib.dptr(p4))
        _lib.check(self._lib.rtd_plan_request_surface(self._h, C.byref(sf)))
        self._surface = (int(model), int(nphi), p4.shape[0])

    def get_bdrf(self):
        """The BDRF tables as the plan holds them, uploaded or device-formed (include/rtd.h: rtd_plan_get_bdrf) ->
        (q [C, NBDRF, N, N], q0 [C, NBDRF, N])."""
        NB = self.prep["NBDRF"]
        q, q0 = np.zeros((self.C, NB, self.N, self.N)), np.zeros((self.C, NB, self.N))
        _lib.check(self._lib.rtd_plan_get_bdrf(self._h, _lib.dptr(q), _lib.dptr(q0)))
        return q, q0

    def get_nt(self):
        """What the plan holds of the corrections' inputs, uploaded or device-formed (include/rtd.h: rtd_plan_get_nt) ->
        dict(wfull [rows, L, nleg_all] with rows = C, or P for a band; f [C, L]; ims_coef [C, nleg_all]; ims_par [C, 2])."""
        rows = C.c_int32()
        _lib.check(self._lib.rtd_plan_get_nt(self._h, None, None, None, None, C.byref(rows)))  # (RTD_ERR_STATE without NT)
        nall = self._nt_nleg_all  # (the call does not report it: that of the last upload, or of the request the columns met)
        if not nall:
            raise ValueError("set_nt or request_nt must precede get_nt.")
        out = dict(wfull=np.empty((rows.value, self.L, nall)), f=np.empty((self.C, self.L)), ims_coef=np.empty((self.C, nall)),
                   ims_par=np.empty((self.C, 2)))
        _lib.check(self._lib.rtd_plan_get_nt(self._h, *[_lib.dptr(out[k]) for k in ("wfull", "f", "ims_coef", "ims_par")], None))
        return out

    def solve(self):
        _lib.check(self._lib.rtd_plan_solve(self._h))
        self.solved = True

    def synchronize(self):
        _lib.check(self._lib.rtd_plan_synchronize(self._h))

    def device_bytes(self):
        return _out_int(self._lib.rtd_plan_device_bytes, self._h)

    @staticmethod
    def pool_bytes():
        """Device memory of closed plans that the library keeps for the next plan (include/rtd.h: rtd_pool_bytes)."""
        return _out_int(_lib.load().rtd_pool_bytes)

    @staticmethod
    def pool_trim(device=-1):
        """Gives that memory back to the runtime (include/rtd.h: rtd_pool_trim); returns the bytes released."""
        return _out_int(_lib.load().rtd_pool_trim, int(device))

    @staticmethod
    def free_device_bytes(device=0):
        """Free memory of the device right now (include/rtd.h: rtd_device_memory)."""
        b = C.c_int64()
        _lib.check(_lib.load().rtd_device_memory(int(device), C.byref(b), None))
        return b.value

    @staticmethod
    def pool_set_limit(nbytes=-1, device=0):
        """Opt in to (or out of) keeping the LARGE device blocks of closed plans for the next plan: nbytes per device, < 0 = an
        eighth of the device's memory, 0 = off (the default).  Returns the previous limit (include/rtd.h: rtd_pool_set_limit)."""
        return _out_int(_lib.load().rtd_pool_set_limit, int(nbytes), int(device))

    def evaluate(self, tau, phi=None, antiderivative=False, want=("u", "u0", "flux"), skip_nt=False, derivative=False):
        """tau [C, ntau]; phi [nphi] or None -> dict of arrays (u [C,Q,ntau,nphi], u0 [C,Q,ntau],
        flux_up / flux_down_diffuse / flux_down_direct [C,ntau], ulast [C,Q,ntau]; "act" in `want` adds the actinic fluxes of
        ``fetch_actinic`` at the same points, in the same order, "view" the radiances u_mu [C,nmu,ntau,nphi] and u0_mu [C,nmu,ntau]
        of ``fetch_view`` at the angles of ``set_view`` -- "view_u" / "view_u0": one of the two; u itself then stays on the device
        unless "u" is wanted too).  derivative: every output is its
        derivative with respect to the unscaled tau (include/rtd.h: bit 2 of rtd_plan_evaluate's flag word; one-sided from above
        at an interface); not together with antiderivative."""
        tau, ntau, phi, nphi, flags, view = self._eval_args(tau, phi, antiderivative, derivative, skip_nt, want)
        # The arrays and their pointers are spelled out here, not taken from _result_arrays / _result_ptrs: this is the one call of
        # the class that bench.py times per call (a whole one-column pydisort() with one closure), and through the helpers that
        # call measured 5 to 7 us slower (HISTORY.md).
        field, level, dptr = (self.C, self.Q, ntau), (self.C, ntau), _lib.dptr
        u = np.empty(field + (nphi,)) if ("u" in want and nphi > 0) else None
        u0 = np.empty(field) if "u0" in want else None
        ul = np.empty(field) if "ulast" in want else None
        fu, fd, fb = (np.empty(level), np.empty(level), np.empty(level)) if "flux" in want else (None, None, None)
        out = dict(u=u, u0=u0, ulast=ul, flux_up=fu, flux_down_diffuse=fd, flux_down_direct=fb)
        self._checked(self._lib.rtd_plan_evaluate(self._h, ntau, dptr(tau), nphi, dptr(phi), flags, dptr(u), dptr(u0), dptr(fu), dptr(fd),
                                                  dptr(fb), dptr(ul)), out)
        if "act" in want:
            out.update(self.fetch_actinic())
        if view:
            out.update(self.fetch_view(view))
        return out

    def _eval_args(self, tau, phi, antiderivative, derivative, skip_nt, want):
        """The arguments ``evaluate`` and ``evaluate_band`` share -> (tau [C, ntau], ntau, phi [nphi] or None, nphi, the flag word of
        include/rtd.h: bit 0 antiderivative | 2 skip_nt | 4 derivative | 8 keep u on the device for the view, the `want` of the view
        fetch)."""
        if antiderivative and derivative:
            raise ValueError("antiderivative and derivative exclude each other.")
        tau = _f64(np.atleast_2d(tau))
        assert tau.shape[0] == self.C
        phi = _f64(np.atleast_1d(phi)) if phi is not None else None
        nphi = 0 if phi is None else len(phi)
        view = self._view_want(want)
        keep_u = 8 if ("u" in view and nphi > 0) else 0  # (u is formed on the device although nothing of it is copied)
        return tau, tau.shape[1], phi, nphi, int(bool(antiderivative)) | (2 if skip_nt else 0) | (4 if derivative else 0) | keep_u, view

    # ---- throughput form (results stay in HBM until fetch) ----
    def set_eval_points(self, tau, phi):
        tau = _f64(np.atleast_2d(tau))
        phi = _f64(np.atleast_1d(phi))
        self._ev_shape = (tau.shape[1], len(phi))
        _lib.check(self._lib.rtd_plan_set_eval_points(self._h, tau.shape[1], _lib.dptr(tau), len(phi),
                                                      _lib.dptr(phi)))

    def set_eval_order(self, order):
        """What run() / run_fetch() evaluate at the stored points: 0 the values (default), -1 their tau-antiderivatives, +1 their
        tau-derivatives (include/rtd.h: rtd_plan_set_eval_order)."""
        if order not in (-1, 0, 1):
            raise ValueError("order must be -1, 0 or +1.")
        _lib.check(self._lib.rtd_plan_set_eval_order(self._h, int(order)))

    def run(self):
        _lib.check(self._lib.rtd_plan_run(self._h))
        self.solved = True

    def invalidate_tables(self):
        """Treat the resident inputs as new: the next solve recomputes the per-column Legendre tables at -mu0 and the beam
        attenuations it would otherwise keep from run to run (include/rtd.h: rtd_plan_invalidate_tables)."""
        _lib.check(self._lib.rtd_plan_invalidate_tables(self._h))

    def retained(self):
        """True when evaluate() after a solve only evaluates (one window, or the evaluator state of every column is resident)."""
        return self.retained_form() is not None

    def retained_form(self):
        """"full" (one window, or everything the evaluators read is resident for every column), "lean" (coefficients, k, E, B
        resident; evaluate() re-runs the eigen stage for the layers its points touch, never the boundary-condition solve) or
        None (evaluate() solves the windows again)."""
        return {0: None, 1: "full", 2: "lean"}[_out_int(self._lib.rtd_plan_retained, self._h, ctype=C.c_int32)]

    def windows(self):
        """(columns per window, number of windows) of the plan's work arena."""
        a, b = C.c_int32(), C.c_int32()
        _lib.check(self._lib.rtd_plan_windows(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def run_fetch(self, out=None):
        """run() and fetch() as one host-to-host pipeline (device-to-host copies of a window overlap the next window's
        kernels; include/rtd.h: rtd_plan_run_fetch).  `out`: dict of preallocated arrays to fill (u, u0, flux_up,
        flux_down_diffuse, flux_down_direct; missing keys are not fetched), default: all of them, freshly allocated."""
        ntau, nphi = self._stored_points("run_fetch")
        if out is None:
            out = _result_arrays((self.C,), self.Q, ntau, nphi)
        self._checked(self._lib.rtd_plan_run_fetch(self._h, *_result_ptrs(out)), out)
        self.solved = True
        return out

    def fetch(self):
        out = _result_arrays((self.C,), self.Q, *self._stored_points("fetch"))
        self._checked(self._lib.rtd_plan_fetch(self._h, *_result_ptrs(out)), out)
        return out

    def result_dev_ptrs(self):
        up, fp = C.c_void_p(), C.c_void_p()
        ub, fb = C.c_int64(), C.c_int64()
        _lib.check(self._lib.rtd_plan_result_dev_ptrs(self._h, C.byref(up), C.byref(ub), C.byref(fp), C.byref(fb)))
        return (up.value, ub.value), (fp.value, fb.value)

    def tensors(self, column=0):
        """The reference's tensors for one column: GC, K, B, G_inv_mu_inv, G."""
        M, L, Q = self.M, self.L, self.Q
        GC, G = np.empty((M, L, Q, Q)), np.empty((M, L, Q, Q))
        K, B, Z = np.empty((M, L, Q)), np.empty((M, L, Q)), np.zeros((L, Q))
        _lib.check(self._lib.rtd_plan_get_tensors(self._h, column, _lib.dptr(GC), _lib.dptr(K), _lib.dptr(B),
                                                  _lib.dptr(Z), _lib.dptr(G)))
        return dict(GC=GC, K=K, B=B, G_inv_mu_inv=Z, G=G)

    # ---- RCCL over xGMI (one rank per plan) ----
    @staticmethod
    def comm_preload():
        _lib.check(_lib.load().rtd_comm_preload())

    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().rtd_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid, rank, nranks):
        if self._band_active():
            raise ValueError("a communicator is not combined with band inputs or band weights.")
        _lib.check(self._lib.rtd_comm_init(self._h, uid, rank, nranks))
        self._nranks = nranks

    def comm_size(self):
        """(nranks, rank, device) as RCCL itself reports them for the plan's communicator (ncclCommCount,
        ncclCommUserRank, ncclCommCuDevice; include/rtd.h: rtd_comm_size)."""
        n, r, d = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        _lib.check(self._lib.rtd_comm_size(self._h, C.byref(n), C.byref(r), C.byref(d)))
        return int(n.value), int(r.value), int(d.value)

    def comm_transport(self):
        """Which transport carries the collectives: "rccl", or "stub:ipc" / "stub:shm" when the environment named the tests'
        stand-in (include/rtd.h: rtd_comm_transport)."""
        buf = C.create_string_buffer(32)
        _lib.check(self._lib.rtd_comm_transport(self._h, buf, 32))
        return buf.value.decode()

    def allgather_fluxes(self):
        _lib.check(self._lib.rtd_comm_allgather_fluxes(self._h))

    def solve_layers(self, first, count):
        """Eigen stage of the layers [first, first + count) only (layer shards; include/rtd.h: rtd_plan_solve_layers)."""
        _lib.check(self._lib.rtd_plan_solve_layers(self._h, int(first), int(count)))
        self.solved = False

    def allgather_layers(self, count_per_rank):
        """ONE RCCL all-gather of the eigen-stage results of every rank's layers (rtd_comm_allgather_layers)."""
        _lib.check(self._lib.rtd_comm_allgather_layers(self._h, int(count_per_rank)))

    def solve_bc(self):
        """Boundary-condition solve over all layers, after solve_layers / allgather_layers."""
        _lib.check(self._lib.rtd_plan_solve_bc(self._h))
        self.solved = True

    def allgather_results(self):
        """RCCL all-gather of u and the fluxes of the last run() over the ranks, on the plan's communication stream
        (overlaps the next run(); include/rtd.h: rtd_comm_allgather_results)."""
        _lib.check(self._lib.rtd_comm_allgather_results(self._h))

    def gather_results(self, root=0):
        """The results of the last run() gathered on rank `root` only (ncclSend / ncclRecv; include/rtd.h:
        rtd_comm_gather_results); every rank calls it."""
        _lib.check(self._lib.rtd_comm_gather_results(self._h, int(root)))

    def fetch_gathered_results(self, want_u=True):
        """-> (u [nranks * C, Q, ntau, nphi] or None, fluxes [nranks, 3, C, ntau]) of the last allgather_results()."""
        (ntau, nphi), nranks = self._stored_points("fetch_gathered_results"), self._after(self._nranks, "comm_init", "fetch_gathered_results")
        u = np.empty((nranks * self.C, self.Q, ntau, nphi)) if want_u else None
        fl = np.empty((nranks, 3, self.C, ntau))
        _lib.check(self._lib.rtd_comm_fetch_gathered_results(self._h, _lib.dptr(u), _lib.dptr(fl)))
        return u, fl

    def fetch_gathered_columns(self, rank, first, count, want_u=True):
        """-> (u [count, Q, ntau, nphi] or None, fluxes [3, count, ntau]): the columns [first, first + count) of rank
        `rank`'s shard in the gathered arrays of the last allgather_results() / gather_results()."""
        ntau, nphi = self._stored_points("fetch_gathered_columns")
        u = np.empty((count, self.Q, ntau, nphi)) if want_u else None
        fl = np.empty((3, count, ntau))
        _lib.check(self._lib.rtd_comm_fetch_gathered_columns(self._h, int(rank), int(first), int(count), _lib.dptr(u), _lib.dptr(fl)))
        return u, fl

    def fetch_gathered(self):
        out = np.empty((self._after(self._nranks, "comm_init", "fetch_gathered"), 3, self.C, self._stored_points("fetch_gathered")[0]))
        _lib.check(self._lib.rtd_comm_fetch_gathered(self._h, _lib.dptr(out)))
        return out

    def enable_timing(self, on=True):
        _lib.check(self._lib.rtd_plan_enable_timing(self._h, int(on)))

    def timing(self, reset=True):
        ms = (C.c_double * 7)()
        n = (C.c_int64 * 7)()
        _lib.check(self._lib.rtd_plan_get_timing(self._h, ms, n, int(reset)))
        names = ("tables", "asm", "jacobi", "post", "iface", "sweep", "eval")
        return {k: (ms[i], n[i]) for i, k in enumerate(names)}

    def pivoted_chains(self):
        """(column, mode) chains of the last window that the tiled 64-stream BC kernel handed to the pivoted kernels."""
        return _out_int(self._lib.rtd_plan_pivoted_chains, self._h, ctype=C.c_int32)

    # ---- a failed column in a batch: raise (default) or mark ----
    numeric_errors = "raise"  # or "nan": fill the failed columns of the returned arrays with NaN instead of raising

    def _checked(self, rc, arrays):
        """Maps the status of a call that returns results.  numeric_errors == "nan": a numerical failure (rc 5) is not raised;
        the columns it belongs to are NaN in `arrays` (u: any failed mode; u0 and fluxes: a failed mode 0 -- the others
        keep their values: they come from mode 0 alone), every other column keeps its result."""
        if rc == _lib.RTD_ERR_NUMERIC and self.numeric_errors == "nan":
            st = self.column_status()
            for k, a in arrays.items():
                if a is not None:
                    a[(st & (0xFFFF if k in ("u", "ulast", "u_mu") else 0xFF)) != 0] = np.nan
            return
        _lib.check(rc)

    def column_status(self):
        """int32 [C]: 0 for a column that solved cleanly, else the numerical-failure bits of include/rtd.h
        (rtd_plan_get_column_status): low byte raised by Fourier mode 0, next byte by modes m > 0 (fluxes and u0 of such a
        column are still valid).  After a NumericalError from a batch this tells which columns to drop."""
        out = np.zeros(self.C, dtype=np.int32)
        _lib.check(self._lib.rtd_plan_get_column_status(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def max_sweeps(self):
        return _out_int(self._lib.rtd_plan_max_sweeps, self._h, ctype=C.c_int32)


def planck_band(T, WVNMLO, WVNMHI, device=0):
    """Planck function integrated over the band WVNMLO ... WVNMHI (cm^-1) at temperature(s) T (K), in W / m^2 -- what the
    reference's ``blackbody_contrib_to_BCs`` integrates with SciPy on the host, on the device in closed form and for a band per
    element (include/rtd.h: rtd_planck_band).  The arguments broadcast; the result has the shape of ``T``."""
    T = np.asarray(T, dtype=np.float64)
    lo, hi = np.asarray(WVNMLO, dtype=np.float64), np.asarray(WVNMHI, dtype=np.float64)
    t, lo, hi = (np.ascontiguousarray(np.broadcast_to(a, T.shape)) for a in (T, lo, hi))
    out = np.empty(T.shape)
    _lib.check(_lib.load().rtd_planck_band(int(device), out.size, _lib.dptr(t), _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(out)))
    return out[()]


def band_mix(dtau_abs, dtau_spec, omega_spec, Leg_spec, NLeg, delta_M=True, device=0):
    """The effective optical properties of a k-distribution band, mixed on the device as ``pydisort_band`` mixes them
    (include/rtd.h: rtd_band_mix): dtau_abs [P, G, L], dtau_spec and omega_spec [P, L, S], Leg_spec [S, nleg_all] ->
    (tau_arr, omega_arr, f_arr [P G, L], Leg_coeffs [P G, L, NLeg]), column p G + g.  f_arr is the mixture's moment NLeg with
    delta_M, else 0; a layer without a scatterer has the moments (1, 0, ...)."""
    a, ds, om, leg = (_f64(v) for v in (dtau_abs, dtau_spec, omega_spec, Leg_spec))
    if a.ndim != 3 or ds.ndim != 3 or leg.ndim != 2:
        raise ValueError("band_mix: need dtau_abs [P, G, L], dtau_spec and omega_spec [P, L, S] and Leg_spec [S, nleg_all].")
    P, G, L = a.shape
    S, nleg_all = leg.shape
    if ds.shape != (P, L, S) or om.shape != (P, L, S):
        raise ValueError(f"band_mix: dtau_spec and omega_spec must have the shape {(P, L, S)}.")
    NLeg = int(NLeg)
    if NLeg < 1 or nleg_all < NLeg + int(bool(delta_M)):
        raise ValueError("band_mix: Leg_spec needs NLeg moments per species, and one more with delta_M.")
    bs = _lib.rtd_band(P, G, S, nleg_all, int(bool(delta_M)), *[_lib.dptr(v) for v in (a, ds, om, leg)])
    out = [np.empty((P * G, L)) for _ in range(3)] + [np.empty((P * G, L, NLeg))]
    _lib.check(_lib.load().rtd_band_mix(int(device), L, NLeg, C.byref(bs), *[_lib.dptr(v) for v in out]))
    return tuple(out)


def lambert_kappa(albedo, fdown_bottom, sph_albedo, emission=None, device=0):
    """The factor kappa(A) = (A F / pi + (1 - A) E) / (1 - A s) of a Lambertian albedo sweep as the device forms it, by the kernel
    behind ``Plan.couple_lambert`` (include/rtd.h: rtd_lambert_kappa): albedo [A] or [C, A], fdown_bottom and sph_albedo [C],
    emission scalar, [C] or None -> (kappa [C, A], flag [C]: 1 where 1 - A s <= 0 or a factor is not finite)."""
    Cn = int(np.size(fdown_bottom))
    alb, F, s, E = lambert_arrays(albedo, (Cn,), np.reshape(fdown_bottom, -1), np.reshape(sph_albedo, -1), emission, Cn)
    kappa, flag = np.empty((Cn, alb.shape[-1])), np.zeros(Cn, dtype=np.int32)
    _lib.check(_lib.load().rtd_lambert_kappa(int(device), Cn, alb.shape[-1], _lib.dptr(alb), Cn if alb.ndim == 2 else 1, _lib.dptr(F),
                                             _lib.dptr(s), _lib.dptr(E), _lib.dptr(kappa), flag.ctypes.data_as(C.POINTER(C.c_int32))))
    return kappa, flag


def device_count():
    n = C.c_int32()
    lib = _lib.load()
    rc = lib.rtd_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _inputs_struct(prep):
    """(rtd_inputs, keep-alive list) for the one-call entry points of include/rtd.h."""
    keys = [("mu_pos", "mu"), ("weights", "W"), ("scaled_omega", "omega_s"), ("tau", "tau"),
            ("scaled_tau_with_0", "tau_s0"), ("scale_tau", "scale_tau"), ("wleg", "wleg"), ("mu0", "mu0"), ("I0", "I0"),
            ("phi0", "phi0"), ("rescale", "rescale"), ("b_pos", "b_pos"), ("b_neg", "b_neg"), ("s_poly", "s_s"),
            ("bdrf_q", "bdrf_q"), ("bdrf_q0", "bdrf_q0")]
    keep, s = [], _lib.rtd_inputs()
    for field, k in keys:
        a = _f64(prep[k])
        keep.append(a)
        setattr(s, field, _lib.dptr(a))
    return s, keep


def _dims(prep):
    return _lib.rtd_dims(prep["C"], prep["L"], 2 * prep["N"], prep["P"], prep["M"], prep["Ns"], prep["NBDRF"],
                         1 if prep["beam"] else 0)


def solve_batch_once(prep, tau, phi, device=0):
    """One call of the C ABI's ``rtd_solve_batch``: plan creation, upload, solve, evaluation and teardown inside the
    library.  tau [C, ntau], phi [nphi] -> dict(u, u0, flux_up, flux_down_diffuse, flux_down_direct)."""
    lib = _lib.load()
    s, keep = _inputs_struct(prep)
    dims = _dims(prep)
    tau, phi = _f64(np.atleast_2d(tau)), _f64(np.atleast_1d(phi))
    nt, nph = tau.shape[1], phi.shape[0]
    out = _result_arrays((prep["C"],), 2 * prep["N"], nt, nph)
    _lib.check(lib.rtd_solve_batch(C.byref(dims), device, C.byref(s), nt, _lib.dptr(tau), nph, _lib.dptr(phi), *_result_ptrs(out)))
    return out


def solve_tensors_once(prep, column=0, device=0):
    """One call of ``rtd_solve_tensors``: the tensors the reference's closures capture for one column."""
    lib = _lib.load()
    s, keep = _inputs_struct(prep)
    dims = _dims(prep)
    M, L, Q = prep["M"], prep["L"], 2 * prep["N"]
    out = dict(GC=np.empty((M, L, Q, Q)), K=np.empty((M, L, Q)), B=np.empty((M, L, Q)), G_inv_mu_inv=np.empty((L, Q)),
               G=np.empty((M, L, Q, Q)))
    _lib.check(lib.rtd_solve_tensors(C.byref(dims), device, C.byref(s), column,
                                     *[_lib.dptr(out[k]) for k in ("GC", "K", "B", "G_inv_mu_inv", "G")]))
    return out
