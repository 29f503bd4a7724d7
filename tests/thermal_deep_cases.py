"""Deep thermal source polynomials (plain NumPy; shared by tools/hp_truth_case.py, which writes the 40-digit fixtures
tests/golden/hp/thermal_<NQuad>_<name>.npz, by tests/test_thermal_deep_cpu.py and by tests/test_gpu_thermal_deep.py).

A thermal source arrives as s_poly_coeffs [L, Ns]: one polynomial per layer in the ABSOLUTE, unscaled optical depth.  Deep in an
atmosphere that form cancels, and every road from it to the coefficients about the layer's top that the kernels use has to keep
what float64 cannot (csrc/rtd_dd.h).  These columns state their polynomials per layer in the LOCAL variable xi = (tau - top) /
thickness, s_l = sum_i c_i xi^i with

    c_i = r_i (0.8 k_min dtau*)^i / i!,   r_i in [0.5, 1] (seeded),

an e^(0.8 k x)-like source (k_min the layer's smallest eigenvalue, dtau* its delta-M-scaled thickness) whose particular solution
sum_q b_q(K) x^q does not cancel; convert them to absolute-tau coefficients in exact rational arithmetic and round those to float64.
The floats are the user's input, and the truth's.

Columns (thermal only: I0 = 0, NFourier = 1; Lambertian surface 0.3; b_neg = 0.3, b_pos = 0.5; omega alternates 0.9 / 0.8):
  d<deg>   delta-M on, chi_l = f + (1 - f) g^l with f_arr = f = 0.5, g = 0.7: the scaled moments are g^l -- a phase function at every
           stream count -- and scale_tau = 0.55 / 0.6 whatever NQuad is.  deg = 1, 3, 5, 9, 13, 19 (Ns = 2 ... 20); d16 (Ns = 17) at 16
           and 32 streams
  n<deg>   the twin without delta-M (f = 0, chi_l = g^l)
  thin     d1 with the eighth (fourth, where L = 10) layer 1e-3 thin: a LINEAR source only (the thin-layer floor of higher degrees
           is a separate matter)
Layers: thicknesses 6, 3, 6, 3 ... (L = 20, tau_L = 90) up to 64 streams; 12, 7, ... (L = 10, tau_L = 95) at 96 and 128 streams.
Stream counts: 6, 16, 30, 32, 64, 96, 128 -- every implementation of the thermal stage and its padding.
"""
import os
from fractions import Fraction
from functools import lru_cache
from math import comb, factorial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HP_DIR = os.path.join(HERE, "golden", "hp")

STREAMS = (6, 16, 30, 32, 64, 96, 128)
DEGREES = (1, 3, 5, 9, 13, 19)
NS17_STREAMS = (16, 32)  # d16: Ns = 17, the first length past the 16 double-doubles of a thread's stack
ONE_COLUMN_STREAMS = (6, 16, 32)  # pydisort() column by column
F, G = 0.5, 0.7
OMEGA = (0.9, 0.8)
SURFACE, B_NEG, B_POS = 0.3, 0.3, 0.5
THIN = 1e-3
DEEP = ("d13", "d16", "d19")  # fixtures that must record a float64-substitution loss >= 1e-6; Ns = 17, 20 a Horner loss >= 1e-7


def layer_count(NQuad):
    return 20 if NQuad <= 64 else 10


def thicknesses(NQuad, thin=False):
    L = layer_count(NQuad)
    d = np.tile([6.0, 3.0] if L == 20 else [12.0, 7.0], L // 2)
    if thin:
        d[7 if L == 20 else 3] = THIN
    return d


def names(NQuad):
    out = [f"{p}{d}" for d in DEGREES for p in "dn"] + ["thin"]
    if NQuad in NS17_STREAMS:
        out.append("d16")
    return out


def keys():
    return [f"{q}_{n}" for q in STREAMS for n in names(q)]


def degree(name):
    return 1 if name == "thin" else int(name[1:])


@lru_cache(maxsize=None)
def k_min(NQuad, omega, delta_m):
    """Smallest eigenvalue of a layer in the (scaled) optical depth: mode 0 of the discrete-ordinates problem with the scaled
    moments g^l and the scaled albedo (1 - f) omega / (1 - omega f)."""
    N = NQuad // 2
    x, w = np.polynomial.legendre.leggauss(N)
    mu, W = 0.5 * (x + 1.0), 0.5 * w
    om = (1.0 - F) * omega / (1.0 - omega * F) if delta_m else omega
    ell = np.arange(NQuad)
    P = np.polynomial.legendre.legvander(mu, NQuad - 1)  # [N, NQuad]
    wl = 0.5 * om * (2 * ell + 1) * G**ell
    Dp = (P * wl) @ P.T
    Dm = (P * wl * (-1.0) ** ell) @ P.T
    al = (Dp * W[None, :] - np.eye(N)) / mu[:, None]
    be = Dm * W[None, :] / mu[:, None]
    return float(np.sqrt(np.min(np.linalg.eigvals((al - be) @ (al + be)).real)))


def local_coefficients(key):
    """c [L, deg + 1]: the layer polynomials in xi = (tau - top) / thickness, by the rule above."""
    q, name = key.split("_")
    NQuad, deg = int(q), degree(name)
    delta_m = name[0] != "n"
    d = thicknesses(NQuad, name == "thin")
    rng = np.random.default_rng([NQuad, deg, int(delta_m)])
    c = np.empty((len(d), deg + 1))
    for l, dt in enumerate(d):
        om = OMEGA[l % 2]
        a = 0.8 * k_min(NQuad, om, delta_m) * dt * ((1.0 - om * F) if delta_m else 1.0)
        c[l] = rng.uniform(0.5, 1.0, deg + 1) * np.array([a**i / factorial(i) for i in range(deg + 1)])
    return c


def absolute_exact(c, tau_arr):
    """The local polynomials c [L, n] as EXACT rational coefficients in the absolute optical depth: [L][n] Fractions."""
    top = [Fraction(0)] + [Fraction(float(t)) for t in tau_arr[:-1]]
    out = []
    for l, row in enumerate(c):
        dt = Fraction(float(tau_arr[l])) - top[l]
        n = len(row)
        loc = [Fraction(float(v)) / dt**i for i, v in enumerate(row)]  # in (tau - top)
        out.append([sum(loc[i] * comb(i, j) * (-top[l]) ** (i - j) for i in range(j, n)) for j in range(n)])
    return out


def local_exact(a_row, top):
    """EXACT coefficients about `top` of the polynomial with the float64 absolute coefficients a_row: Fractions."""
    a = [Fraction(float(v)) for v in a_row]
    t = Fraction(float(top))
    return [sum(a[j] * comb(j, i) * t ** (j - i) for j in range(i, len(a))) for i in range(len(a))]


def exact_local_scaled(kw):
    """What the kernels are to work from, in exact arithmetic on the float64 inputs: per layer the coefficients of the scaled source
    (1 - omega) / sc s(tau) in x = sc (tau - top), sc = fl(1 - omega f) -- b_i = (exact shift of a by the layer's top)_i / sc^i
    (1 - omega) / sc.  -> ([L][Ns] Fractions, the layers' scaled thicknesses [L] Fractions)."""
    tau = np.atleast_1d(np.asarray(kw["tau_arr"], float))
    L = len(tau)
    om = np.broadcast_to(np.atleast_1d(np.asarray(kw["omega_arr"], float)), (L,))
    f = np.broadcast_to(np.atleast_1d(np.asarray(kw.get("f_arr", 0.0), float)), (L,))
    a = np.atleast_2d(np.asarray(kw["s_poly_coeffs"], float))
    top = np.concatenate(([0.0], tau[:-1]))
    out, width = [], []
    for l in range(L):
        sc = Fraction(float(1.0 - om[l] * f[l]))
        k = (1 - Fraction(float(om[l]))) / sc
        out.append([b / sc**i * k for i, b in enumerate(local_exact(a[l], top[l]))])
        width.append(sc * (Fraction(float(tau[l])) - Fraction(float(top[l]))))
    return out, width


def source_error(got, exact, width, npoints=9):
    """Largest error of the local polynomials got [L][Ns] (floats or Fractions) against exact [L][Ns] over npoints per layer, in
    units of the layer's largest source value; and the same error over the bound unit sum_i |exact_i| x^i (for arithmetic bounds).
    Exact rational evaluation.  -> (of the source, of the sum of the absolute local terms)."""
    worst, worst_terms = 0.0, 0.0
    for g, e, w in zip(got, exact, width):
        d = [Fraction(float(a)) - b if not isinstance(a, Fraction) else a - b for a, b in zip(g, e)]
        xs = [w * j / (npoints - 1) for j in range(npoints)]
        big = max(abs(sum(c * x**i for i, c in enumerate(e))) for x in xs)
        for x in xs:
            err = abs(sum(c * x**i for i, c in enumerate(d)))
            terms = sum(abs(c) * x**i for i, c in enumerate(e))
            worst = max(worst, float(err / big))
            worst_terms = max(worst_terms, float(err / terms) if terms else 0.0)
    return worst, worst_terms


def horner_shift(a_row, t):
    """The Taylor shift in plain float64 (Horner / Ruffini, fused multiply-adds left aside): what rtd_taylor_shift did beyond 16
    coefficients."""
    c = [float(v) for v in a_row]
    n = len(c)
    for k in range(n - 1):
        for j in range(n - 2, k - 1, -1):
            c[j] = c[j + 1] * t + c[j]
    return c


@lru_cache(maxsize=None)
def case(key):
    """Keyword arguments of the one-column ``pydisort`` for "<NQuad>_<name>"."""
    q, name = key.split("_")
    NQuad = int(q)
    delta_m = name[0] != "n"
    tau_arr = np.cumsum(thicknesses(NQuad, name == "thin"))
    L = len(tau_arr)
    chi = G ** np.arange(NQuad + 1)
    if delta_m:
        chi = F + (1.0 - F) * chi
    s = np.array([[float(v) for v in row] for row in absolute_exact(local_coefficients(key), tau_arr)])
    return dict(tau_arr=tau_arr, omega_arr=np.tile(OMEGA, L // 2), NQuad=NQuad, NFourier=1, Leg_coeffs_all=np.tile(chi, (L, 1)),
                mu0=0.6, I0=0.0, phi0=0.0, f_arr=np.full(L, F if delta_m else 0.0), s_poly_coeffs=s, b_neg=B_NEG, b_pos=B_POS,
                BDRF_Fourier_modes=[SURFACE])


def points(kw):
    """tau = 0, every interface, the bottom and one interior point per layer."""
    edges = np.concatenate(([0.0], np.atleast_1d(kw["tau_arr"])))
    return np.sort(np.concatenate((edges, edges[:-1] + 0.4 * np.diff(edges))))


def fixture_path(key):
    return os.path.join(HP_DIR, f"thermal_{key}.npz")


def batches(NQuad):
    """{Ns: [names]}: the columns of one coefficient count, which stack into one batch."""
    out = {}
    for n in names(NQuad):
        out.setdefault(degree(n) + 1, []).append(n)
    return out


def batch_kwargs(NQuad, column_names):
    """Columns of one stream count and ONE coefficient count stacked for ``pydisort_batch`` -> (kwargs, tau [C, ntau])."""
    N = NQuad // 2
    cols = [case(f"{NQuad}_{n}") for n in column_names]
    C = len(cols)
    st = lambda k: np.stack([kw[k] for kw in cols])  # noqa: E731
    out = dict(tau_arr=st("tau_arr"), omega_arr=st("omega_arr"), NQuad=NQuad, Leg_coeffs_all=st("Leg_coeffs_all"), mu0=np.full(C, 0.6),
               I0=np.zeros(C), phi0=np.zeros(C), NFourier=1, b_pos=np.full((C, N), B_POS), b_neg=np.full(C, B_NEG), f_arr=st("f_arr"),
               bdrf_q=np.full((C, 1, N, N), SURFACE), bdrf_q0=np.full((C, 1, N), SURFACE), s_poly_coeffs=st("s_poly_coeffs"))
    return out, np.stack([points(kw) for kw in cols])
