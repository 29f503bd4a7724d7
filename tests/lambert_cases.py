"""Shared by the Lambertian-sweep tests: the fixture cases of tests/golden/lambert/, a NumPy / fractions.Fraction model of
csrc/rtd_lambert.h that reproduces its roundings operation by operation, the exact rational value of what it computes, and the
rounding bounds stated in that header.

The model: every operation of the header is one correctly rounded float64 operation, so each is formed exactly in
fractions.Fraction and rounded once by float() (which rounds a Fraction to nearest-even):
  g = F / PI_D;  e = fma(-A, E, E);  n = fma(A, g, e);  d = fma(-A, s, 1);  kappa = n / d;  out = fma(kappa, b, a) (a when kappa == 0).
Exact values use PI as a 60-digit rational: its distance from pi is far below everything compared here."""
import os
from fractions import Fraction as Fr

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "lambert")

U = Fr(1, 2 ** 53)
PI_D = 3.14159265358979323846  # the float64 nearest pi: RTD_LAMBERT_PI
PI = Fr("3.14159265358979323846264338327950288419716939937510582097494")
KAPPA_ULPS, COUPLE_ULPS = 6, 8  # RTD_LAMBERT_KAPPA_ULPS, RTD_LAMBERT_COUPLE_ULPS

ALBEDOS = (0.0, 0.3, 0.95, 1.0)
PHI = np.array([0.0, 2.0])
ORDERS = ("value", "antider")  # what the reference evaluates; the tau-derivative is the oracle's and the device's alone
VALUE_ONLY = ("q16_l3_thermal",)  # the reference's antiderivative of a thermal particular solution needs ntau == NLayers


FIELDS = ("u", "u0", "flux_up", "flux_down_diffuse", "u_mu", "u0_mu")  # what the surface changes


def orders_of(name):
    return ORDERS[:1] if name in VALUE_ONLY else ORDERS


def fields_of(order):
    """The fields a fixture holds in a tau-order: the reference's u0 and u return the VALUE for the antiderivative of a solve
    without a beam -- the lit-from-below solve -- so only the fluxes are stored there (tests/golden/make_lambert_goldens.py)."""
    return FIELDS if order == "value" else ("flux_up", "flux_down_diffuse")


def _fma(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))  # (inf or nan either way)
    try:
        return float(Fr(a) * Fr(b) + Fr(c))
    except OverflowError:
        return float(np.copysign(np.inf, Fr(a) * Fr(b) + Fr(c)))


def kappa_model(A, F, s, E):
    """rtd_lambert_kappa, rounding by rounding -> (kappa, bad)."""
    A, F, s, E = float(A), float(F), float(s), float(E)
    g = F / PI_D
    e = _fma(-A, E, E)
    n = _fma(A, g, e)
    d = _fma(-A, s, 1.0)
    bad = int(not (d > 0.0) or not np.isfinite(d) or not np.isfinite(n))
    with np.errstate(all="ignore"):
        return float(np.float64(n) / np.float64(d)), bad


def couple_model(a, b, kappa):
    """rtd_lambert_couple over arrays a, b (b broadcast against a) -> the array of a's shape."""
    a = np.asarray(a, float)
    b = np.broadcast_to(np.asarray(b, float), a.shape)
    if kappa == 0.0:
        return a.copy()
    out = np.empty(a.size)
    for i, (x, y) in enumerate(zip(a.ravel(), b.ravel())):
        out[i] = _fma(kappa, y, x)
    return out.reshape(a.shape)


def kappa_exact(A, F, s, E):
    """(kappa of the float64 inputs as a Fraction (pi the 60-digit rational), the magnitude the header's bound is relative to)."""
    A, F, s, E = Fr(float(A)), Fr(float(F)), Fr(float(s)), Fr(float(E))
    d = 1 - A * s
    return (A * F / PI + (1 - A) * E) / d, (A * abs(F) / PI + (1 - A) * E) / d


def kappa_ratio(got, A, F, s, E):
    """|got - exact| over the header's bound KAPPA_ULPS u (A |F| / pi + (1 - A) E) / (1 - A s); 0 when both vanish."""
    want, size = kappa_exact(A, F, s, E)
    err = abs(Fr(float(got)) - want)
    return 0.0 if err == 0 else float(err / (KAPPA_ULPS * U * size)) if size != 0 else float("inf")


def couple_ratio(got, a, b, A, F, s, E):
    """The worst of |got - (a + kappa_exact b)| over the header's bound COUPLE_ULPS u (|a| + |kappa_exact b|), elementwise over arrays
    (b broadcast against a)."""
    k = kappa_exact(A, F, s, E)[0]
    got, a = np.asarray(got, float), np.asarray(a, float)
    b = np.broadcast_to(np.asarray(b, float), a.shape)
    worst = 0.0
    for g, x, y in zip(got.ravel(), a.ravel(), b.ravel()):
        want, size = Fr(float(x)) + k * Fr(float(y)), abs(Fr(float(x))) + abs(k * Fr(float(y)))
        err = abs(Fr(float(g)) - want)
        if err != 0:
            worst = max(worst, float(err / (COUPLE_ULPS * U * size)) if size != 0 else float("inf"))
    return worst


# ---- the fixture cases: keyword arguments of the reference's pydisort() over a BLACK surface; E the surface's black-body emission ----
def _hg(g, n):
    return g ** np.arange(n)


def cases():
    three = dict(tau_arr=np.array([0.3, 1.1, 2.0]), omega_arr=np.array([0.95, 0.8, 0.9]), mu0=0.6, I0=np.pi, phi0=0.5)
    leg3 = np.stack([_hg(0.75, 64), _hg(0.6, 64), _hg(0.8, 64)])
    out = {
        "q6_l1": (dict(tau_arr=np.array([0.8]), omega_arr=np.array([0.9]), NQuad=6, Leg_coeffs_all=_hg(0.7, 6)[None, :], mu0=0.6, I0=np.pi,
                       phi0=0.5), 1.7),
        "q16_l3_nt": (dict(three, NQuad=16, Leg_coeffs_all=leg3, NLeg=16, f_arr=leg3[:, 16], NT_cor=True, b_neg=0.2), 0.0),
        "q16_l3_thermal": (dict(three, NQuad=16, Leg_coeffs_all=leg3[:, :16], b_neg=0.2,
                                s_poly_coeffs=np.array([[0.6, 0.3], [0.5, 0.4], [0.2, 0.55]])), 1.7),
        "q34_l3": (dict(three, NQuad=34, Leg_coeffs_all=leg3[:, :34]), 0.0),
        "q16_l3_nodm": (dict(three, NQuad=16, Leg_coeffs_all=leg3[:, :16], b_neg=0.2), 0.0),
        "q16_thick": (dict(tau_arr=np.array([2.0, 12.0, 30.0]), omega_arr=np.array([0.9999, 0.99999, 0.9999]), NQuad=16,
                           Leg_coeffs_all=np.tile(_hg(0.7, 16), (3, 1)), mu0=0.6, I0=np.pi, phi0=0.5), 0.0),
    }
    return out


def points(kw):
    """Four depths: the top, an interior point, an interface (the bottom of a one-layer column's upper half), the bottom."""
    tau_arr = np.asarray(kw["tau_arr"], float)
    mid = tau_arr[0] if len(tau_arr) > 1 else 0.5 * tau_arr[0]
    return np.array([0.0, 0.37 * tau_arr[-1], mid, tau_arr[-1]])


def view_mu(NQuad):
    """Three angles: upward, downward, and a quadrature node looking down."""
    from numpy.polynomial.legendre import leggauss
    x = leggauss(NQuad // 2)[0]
    return np.array([0.83, -0.41, -0.5 * (x[1] + 1.0)])


def below_kwargs(kw):
    """The lit-from-below companion of a case: the same layers, no source, b_pos = 1, one azimuth-independent mode."""
    keep = {k: kw[k] for k in ("tau_arr", "omega_arr", "NQuad", "mu0", "phi0") if k in kw}
    NLeg = kw.get("NLeg", kw["NQuad"])
    extra = {"f_arr": kw["f_arr"]} if "f_arr" in kw else {}
    return dict(keep, Leg_coeffs_all=np.asarray(kw["Leg_coeffs_all"])[:, :NLeg], NLeg=NLeg, I0=0.0, b_pos=1.0, only_flux=True, **extra)


def load(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


SOLVES = ("black", "below") + tuple(f"direct{i}" for i in range(len(ALBEDOS)))  # the leading axis of every stored field


def get(store, solve, order, field):
    """One solve's field of a fixture (or of a dict laid out like one): "<order>.<field>"[SOLVES.index(solve)]."""
    return store[f"{order}.{field}"][SOLVES.index(solve)]


def terms(store):
    """(F, s) of a fixture or of any dict with the same keys: flux_down (diffuse + direct, value order) of the black solve and of
    the lit-from-below solve at the bottom, the last of the stored depths; s over pi."""
    F = get(store, "black", "value", "flux_down_diffuse")[-1] + get(store, "black", "value", "flux_down_direct")[-1]
    s = (get(store, "below", "value", "flux_down_diffuse")[-1] + get(store, "below", "value", "flux_down_direct")[-1]) / np.pi
    return float(F), float(s)


def coupled(store, order, field, A, E):
    """The model of csrc/rtd_lambert.h applied to a store's black and below arrays -> (the coupled field, kappa, 1 / (1 - A s))."""
    F, s = terms(store)
    k, bad = kappa_model(A, F, s, E)
    assert not bad
    a, b = get(store, "black", order, field), get(store, "below", order, field)
    return couple_model(a, b, k), k, 1.0 / (1.0 - A * s)
