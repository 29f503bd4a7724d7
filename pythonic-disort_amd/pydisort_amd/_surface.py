"""Parametric surface models (include/rtd.h: rtd_surface; csrc/rtd_surface.h has the formulas): what ``surface=`` of the batch and
band entry points takes, checked on the host before a plan exists, and the plan-free ``surface_reflectance``.

rho(mu, mu', dphi): mu is the reflected cosine, mu' the incident one, dphi the difference of the propagation azimuths as the
reference's BDRF callables take it -- backscatter (the hot spot) is at dphi = pi.  Ross-Li is clamped at 0: its kernels are unbounded
below at grazing angles (rho = -1.8 at the smallest node of 16 streams for the weights 0.3, 0.1, 0.05).

"ocean" is the wind-roughened sea (Cox-Munk glint, isotropic slopes): U the wind speed in m/s, n the real refractive index, rho_w a
Lambertian addition for underlight and foam; the glint is at dphi = 0.  Its shadowing is always on: without it the albedo at the
smallest node exceeds 1 from 16 streams upward.  In a plan its modes are formed on a clustered azimuth grid of nphi nodes (even,
>= 4 NBDRF; default 512, which leaves <= 1.7e-9 of a pair's largest mode at 64 streams: profiles/surface_ocean.json), because the
glint at a grazing pair of cosines is 1e-3 rad wide; ``surface_reflectance`` keeps the uniform grid for it as for the others."""
import numpy as np

from . import _lib

# name -> (model id of include/rtd.h, number of parameters)
MODELS = {"lambert": (0, 1), "hapke": (1, 3), "rossli": (2, 3), "rpv": (3, 4), "ocean": (4, 3)}
PARAMETERS = {"lambert": "albedo", "hapke": "B0, HH, W", "rossli": "f_iso, f_vol, f_geo", "rpv": "rho0, k, Theta, rho_c",
              "ocean": "U, n, rho_w"}
NPHI_DEFAULT = {"ocean": 512}  # (every other model: 256)
NPHI_MAX = 16384


def _model(name):
    if not isinstance(name, str) or name.lower() not in MODELS:
        raise ValueError(f"surface: unknown model {name!r} (known: {', '.join(MODELS)}).")
    return name.lower()


def check_params(name, p4):
    """p4 [rows, 4] against the ranges of include/rtd.h; the message names the first bad row."""
    ok = np.all(np.isfinite(p4), axis=1)
    a, b, c = p4[:, 0], p4[:, 1], p4[:, 2]
    with np.errstate(invalid="ignore"):
        if name == "lambert":
            ok &= (a >= 0) & (a <= 1)
            need = "finite, 0 <= albedo <= 1"
        elif name == "hapke":
            ok &= (a >= 0) & (b > 0) & (c > 0) & (c <= 1)
            need = "finite, B0 >= 0, HH > 0, 0 < W <= 1"
        elif name == "rossli":
            ok &= (a >= 0) & (b >= 0) & (c >= 0)
            need = "finite, f_iso, f_vol, f_geo >= 0"
        elif name == "rpv":
            ok &= (a >= 0) & (b > 0) & (np.abs(c) < 1)
            need = "finite, rho0 >= 0, k > 0, |Theta| < 1"
        else:
            ok &= (a >= 0) & (b > 1) & (c >= 0)
            need = "finite, U >= 0, n > 1, rho_w >= 0"
    if not np.all(ok):
        r = int(np.argmin(ok))
        raise ValueError(f"surface: {name} parameters ({PARAMETERS[name]}) of row {r} are {p4[r, :MODELS[name][1]].tolist()}; need {need}.")


def _pad4(name, params, lead_ok, what):
    """params [..., npar] with the leading shape one of `lead_ok` -> ([rows, 4] padded with 0, leading shape)."""
    npar = MODELS[name][1]
    p = np.asarray(params, dtype=np.float64)
    if npar == 1 and (p.ndim == 0 or (p.shape in lead_ok and p.shape != (1,))):
        p = p[..., None]  # (a bare albedo, or one per row)
    if p.ndim < 1 or p.shape[-1] != npar or p.shape[:-1] not in lead_ok:
        shapes = " or ".join(str(list(s) + [npar]) for s in lead_ok)
        raise ValueError(f"surface: params of {name} ({PARAMETERS[name]}) must have the shape {shapes} ({what}); got {list(p.shape)}.")
    lead = p.shape[:-1]
    p4 = np.zeros((int(np.prod(lead, dtype=np.int64)), 4))
    p4[:, :npar] = p.reshape(-1, npar)
    check_params(name, p4)
    return p4, lead


def surface_request(surface, lead_ok, what, NFourier, NBDRF):
    """``surface=dict(model=..., params=..., nphi=256)`` of an entry point -> dict(model=id, name, nphi, params [rows, 4], NBDRF) for
    ``Plan.request_surface``.  nphi defaults to 512 for "ocean".  lead_ok: the admissible leading shapes of params, e.g. ((), (C,)).  Every error is a ValueError raised
    here, before anything touches the device."""
    if not isinstance(surface, dict):
        raise ValueError("surface must be a dict(model=..., params=..., nphi=256).")
    unknown = set(surface) - {"model", "params", "nphi"}
    if unknown:
        raise ValueError(f"surface: unknown entries {sorted(unknown)} (known: model, params, nphi).")
    if surface.get("params") is None:
        raise ValueError("surface: params is required.")
    name = _model(surface.get("model"))
    p4, _ = _pad4(name, surface["params"], lead_ok, what)
    nb = NFourier if NBDRF is None else int(NBDRF)
    if not 0 < nb <= NFourier:
        raise ValueError("Need 0 < NBDRF <= NFourier.")
    nphi = surface.get("nphi", NPHI_DEFAULT.get(name, 256))
    if not isinstance(nphi, (int, np.integer)) or isinstance(nphi, bool) or not 2 * (nb - 1) < nphi <= NPHI_MAX:
        raise ValueError(f"surface: nphi must be an integer with 2 (NBDRF - 1) < nphi <= {NPHI_MAX} (NBDRF = {nb}).")
    if name == "ocean" and (nphi % 2 or nphi < 4 * nb):
        raise ValueError(f"surface: nphi of ocean (the nodes of its clustered azimuth grid) must be even with 4 NBDRF <= nphi <= {NPHI_MAX} "
                         f"(NBDRF = {nb}).")
    return dict(model=MODELS[name][0], name=name, nphi=int(nphi), params=np.ascontiguousarray(p4), NBDRF=nb)


def surface_reflectance(model, params, mu, mu_p, nphi, device=0):
    """rho(mu, mu_p, 2 pi p / nphi), p < nphi, of a parametric surface model, formed on the device by the kernel the plans use
    (include/rtd.h: rtd_surface_samples): model "lambert" | "hapke" | "rossli" | "rpv" | "ocean"; params [..., npar]; mu (reflected) and mu_p
    (incident) cosines in (0, 1].  The leading axes of params, mu and mu_p broadcast; the result has their shape plus [nphi].
    rho_qq [C, N, N, nphi] of ``sample_BDRF`` is ``surface_reflectance(m, params[:, None, None, :], mu[:, None], mu[None, :], nphi)``."""
    name = _model(model)
    npar = MODELS[name][1]
    p = np.asarray(params, dtype=np.float64)
    if npar == 1 and p.ndim == 0:
        p = p[None]
    if p.ndim < 1 or p.shape[-1] != npar:
        raise ValueError(f"surface_reflectance: params of {name} ({PARAMETERS[name]}) must have the shape [..., {npar}]; got {list(p.shape)}.")
    mu, mu_p = np.asarray(mu, dtype=np.float64), np.asarray(mu_p, dtype=np.float64)
    if not isinstance(nphi, (int, np.integer)) or isinstance(nphi, bool) or not 1 <= nphi <= NPHI_MAX:
        raise ValueError(f"surface_reflectance: nphi must be an integer between 1 and {NPHI_MAX}.")
    if not (np.all((mu > 0) & (mu <= 1)) and np.all((mu_p > 0) & (mu_p <= 1))):
        raise ValueError("surface_reflectance: mu and mu_p must lie in (0, 1].")
    try:
        shape = np.broadcast_shapes(p.shape[:-1], mu.shape, mu_p.shape)
    except ValueError:
        raise ValueError(f"surface_reflectance: params {list(p.shape)}, mu {list(mu.shape)} and mu_p {list(mu_p.shape)} do not broadcast.") from None
    n = int(np.prod(shape, dtype=np.int64))
    p4 = np.zeros((n, 4))
    p4[:, :npar] = np.broadcast_to(p, shape + (npar,)).reshape(n, npar)
    check_params(name, p4)
    m = np.ascontiguousarray(np.broadcast_to(mu, shape)).reshape(n)
    mp = np.ascontiguousarray(np.broadcast_to(mu_p, shape)).reshape(n)
    out = np.empty((n, int(nphi)))
    _lib.check(_lib.load().rtd_surface_samples(int(device), MODELS[name][0], n, _lib.dptr(p4), _lib.dptr(m), _lib.dptr(mp), int(nphi),
                                               _lib.dptr(out)))
    return out.reshape(shape + (int(nphi),))
