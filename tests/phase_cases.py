"""Inputs beyond Henyey-Greenstein with 0 <= g < 1: phase-function classes with structural zeros, negative moments and
tabulated Mie moments, as six columns per stream count (plain NumPy; shared by tools/hp_truth_case.py, which writes the 40-digit
fixtures tests/golden/hp/phase_<NQuad>_<column>.npz, by tests/test_phase_truth_cpu.py and by tests/test_gpu_phase_truth.py).

Columns (all NFourier = 3, NLeg = NQuad, NQuad + 1 moments given, the same layer count: they stack into one batch):
  c0  Rayleigh in every layer, two omega = 1 - 1e-6 layers, beam, Lambertian surface, no thermal source
  c1  isotropic, omega = [0.5, 1 - 1e-6, 0.0] (a non-scattering layer under a near-conservative one), beam + b_neg, no thermal source
  c2  backscattering Henyey-Greenstein (g < 0), omega <= 0.99, no beam, linear thermal source, b_pos vector
  c3  double Henyey-Greenstein b g1^l + (1 - b) g2^l (g1 > 0 > g2) with delta-M (f = chi_NQuad), omega <= 0.99, beam, quadratic
      thermal source
  c4  short expansion (five non-zero moments, then zeros up to NLeg = NQuad), beam, a two-mode non-symmetric tabulated BDRF
  c5  layered mix: Rayleigh over cloud C1 with delta-M and omega = 1 - 1e-6 over isotropic, beam, Lambertian, no thermal source
No column with an omega > 1 - 1e-5 layer has a thermal source (tests/test_gpu_random_parity.py:
test_thermal_polynomial_in_a_near_conservative_thin_layer_is_as_good_as_the_reference says why no tolerance exists there).

Stream counts: 6, 14, 30, 62, 126 (one pair short of the padded widths 4 / 8 / 16 / 32 / 64 per hemisphere) carry all six columns;
8, 16, 32, 64, 128 carry c5 only.  PADDED carries all six as well: 10, 18, 34, 98 are the most-padded ends of the widths 8 / 16 / 32 /
64 (one pair past the next smaller width), and 66, 94, 96 the 48-lane class of the wide boundary-condition kernels (66 ... 96 streams)
at its most-padded end, one pair short and full; each takes the g, g1, g2, b of the next smaller count of FULL.  2 and 4 streams are
left out: c3 and c4 cannot be stated there.
Three layers up to 64 streams, two beyond, where c1 drops its last layer and c5 its first.

The one column with another layer count, at 94 and 126 streams ("94_deep", "126_deep"; in no batch): six layers, the recursion of
the wide kernels across five interfaces on ill-conditioned layers --
  deep  Rayleigh 0.95 (0.3 thick) / cloud C1 with delta-M, omega = 1 - 1e-6 (0.8) / isotropic 0.5 (1e-3: a thin layer) / Rayleigh,
        omega = 1 - 1e-6 (0.9) / cloud C1 with delta-M, 0.9 (9.0: the Stamnes-Conklin scaling at work) / non-scattering (2.0);
        beam, Lambertian 0.3, no thermal source.
g, g1, g2 and b shrink with the stream count so that every truncation  sum_{l < NQuad} (2l + 1) chi*_l P_l  (delta-M-scaled where
f > 0) is a phase function: non-negative over 4001 angles (tests/test_phase_truth_cpu.py asserts it).

NEGATIVE is the one case deliberately outside that rule: 8 streams, Rayleigh / 0.8 0.8^l + 0.2 (-0.5)^l / isotropic, whose
truncation dips to -0.25.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HP_DIR = os.path.join(HERE, "golden", "hp")

FULL = (6, 14, 30, 62, 126)  # all six columns
MIX_ONLY = (8, 16, 32, 64, 128)  # c5 only
PADDED = (10, 18, 34, 66, 94, 96, 98)  # all six columns: the most-padded ends of the widths, and the 48-lane class (66 ... 96)
DEEP = (94, 126)  # the six-layer column "deep"
COLUMNS = ("c0", "c1", "c2", "c3", "c4", "c5")
NEAR_CONSERVATIVE = ("c0", "c1", "c5", "deep")
NFOURIER = 3
PHI = np.array([0.0, 0.7, 3.0])
NEGATIVE = "8_neg"
MU0, I0, PHI0 = 0.6, 2.0, 0.5

#  NQuad: (g of c2, (b, g1, g2) of c3): the largest round figures whose NQuad-term truncation stays non-negative
HG_PARAMETERS = {6: (-0.5, (0.8, 0.6, -0.4)), 14: (-0.65, (0.8, 0.8, -0.5)), 30: (-0.75, (0.8, 0.9, -0.7)),
                 62: (-0.85, (0.8, 0.92, -0.8)), 126: (-0.9, (0.8, 0.95, -0.85))}
# the PADDED stream counts take the entry of the next smaller count of FULL
HG_PARAMETERS.update({10: HG_PARAMETERS[6], 18: HG_PARAMETERS[14], 34: HG_PARAMETERS[30],
                      66: HG_PARAMETERS[62], 94: HG_PARAMETERS[62], 96: HG_PARAMETERS[62], 98: HG_PARAMETERS[62]})
# Cloud C1 itself admits no such choice, and at 6 streams its delta-M-scaled truncation dips to -0.0078: there, and only there, the
# cloud layer of c5 is 95 % cloud C1 + 5 % Rayleigh (a cloud with molecular scattering between the droplets; minimum +0.074), still
# a tabulated Mie sequence and no geometric one.  Every other stream count takes the C1 moments as they are (minima 0.0076 ... 0.030).
CLOUD_FRACTION = {6: 0.95}
SHORT = np.array([1.0, 0.6, 0.35, 0.1, 0.02])


def pad(a, n):
    out = np.zeros(n)
    out[:len(a)] = a
    return out


def isotropic(n):
    return pad([1.0], n)


def rayleigh(n):
    return pad([1.0, 0.0, 0.1], n)


def henyey_greenstein(g, n):
    return float(g) ** np.arange(n)


def double_henyey_greenstein(b, g1, g2, n):
    return b * henyey_greenstein(g1, n) + (1.0 - b) * henyey_greenstein(g2, n)


def short_expansion(n):
    return pad(SHORT, n)


def cloud_c1(n):
    """The first n Legendre moments of the cloud C1 phase function (DISORT's test problem 5), from the fixture of the literal
    cfg2 column the repository already carries."""
    z = np.load(os.path.join(HERE, "golden", "synth", "cfg2_q32_cloud_a.npz"))
    return np.array(z["Leg_coeffs_all"][0, :n], float)


def layer_count(NQuad):
    return 3 if NQuad <= 64 else 2


def _surface_mode(m):
    """Fourier mode m of a BDRF that is not symmetric in (mu, mu'): a callable f(mu, -mu') as ``pydisort`` takes it."""
    if m == 0:
        return lambda mu, mup: 0.2 * (1.0 + 0.8 * np.outer(mu, np.asarray(mup) ** 2))
    return lambda mu, mup: 0.06 * np.outer(np.sqrt(1.0 - mu**2) * (1.0 + 0.5 * mu), np.sqrt(1.0 - np.asarray(mup) ** 2))


def keys():
    return ([f"{q}_{c}" for q in FULL for c in COLUMNS] + [f"{q}_c5" for q in MIX_ONLY]
            + [f"{q}_{c}" for q in PADDED for c in COLUMNS] + [f"{q}_deep" for q in DEEP])


def case(key):
    """Keyword arguments of the one-column ``pydisort`` for "<NQuad>_<column>" (or NEGATIVE)."""
    if key == NEGATIVE:
        n = 9
        return dict(tau_arr=np.array([0.3, 1.1, 2.0]), omega_arr=np.array([1 - 1e-6, 0.9, 0.5]), NQuad=8,
                    Leg_coeffs_all=np.stack([rayleigh(n), double_henyey_greenstein(0.8, 0.8, -0.5, n), isotropic(n)]),
                    mu0=MU0, I0=I0, phi0=PHI0, b_neg=0.1, BDRF_Fourier_modes=[0.3], s_poly_coeffs=np.array([[0.2, 0.05]] * 3))
    q, col = key.split("_")
    NQuad = int(q)
    N, n, L = NQuad // 2, NQuad + 1, layer_count(NQuad)
    last = slice(None, L)  # two layers: the first two ...
    kw = dict(tau_arr=np.array([0.3, 1.1, 2.0])[:L], NQuad=NQuad, NFourier=NFOURIER, mu0=MU0, I0=I0, phi0=PHI0)
    if col == "deep":
        c1 = cloud_c1(n)
        kw.update(tau_arr=np.cumsum([0.3, 0.8, 1e-3, 0.9, 9.0, 2.0]), omega_arr=np.array([0.95, 1 - 1e-6, 0.5, 1 - 1e-6, 0.9, 0.0]),
                  Leg_coeffs_all=np.stack([rayleigh(n), c1, isotropic(n), rayleigh(n), c1, isotropic(n)]),
                  f_arr=np.array([0.0, c1[NQuad], 0.0, 0.0, c1[NQuad], 0.0]), BDRF_Fourier_modes=[0.3])
    elif col == "c0":
        kw.update(omega_arr=np.array([1 - 1e-6, 0.7, 1 - 1e-6])[[0, 2] if L == 2 else [0, 1, 2]],
                  Leg_coeffs_all=np.tile(rayleigh(n), (L, 1)), BDRF_Fourier_modes=[0.3])
    elif col == "c1":
        kw.update(omega_arr=np.array([0.5, 1 - 1e-6, 0.0])[last], Leg_coeffs_all=np.tile(isotropic(n), (L, 1)), b_neg=0.1)
    elif col == "c2":
        g = HG_PARAMETERS[NQuad][0]
        kw.update(omega_arr=np.array([0.99, 0.6, 0.9])[last], Leg_coeffs_all=np.tile(henyey_greenstein(g, n), (L, 1)), I0=0.0,
                  s_poly_coeffs=np.array([[0.2, 0.05], [0.1, 0.0], [0.3, -0.02]])[last], b_pos=0.1 + 0.4 * np.linspace(0.0, 1.0, N) ** 2)
    elif col == "c3":
        leg = double_henyey_greenstein(*HG_PARAMETERS[NQuad][1], n)
        kw.update(omega_arr=np.array([0.9, 0.99, 0.8])[last], Leg_coeffs_all=np.tile(leg, (L, 1)), f_arr=np.full(L, leg[NQuad]),
                  s_poly_coeffs=np.array([[0.2, 0.05, -0.01], [0.1, 0.0, 0.02], [0.3, -0.02, 0.005]])[last])
    elif col == "c4":
        kw.update(omega_arr=np.array([0.95, 0.3, 0.8])[last], Leg_coeffs_all=np.tile(short_expansion(n), (L, 1)), NLeg=NQuad,
                  BDRF_Fourier_modes=[_surface_mode(0), _surface_mode(1)])
    elif col == "c5":
        a = CLOUD_FRACTION.get(NQuad, 1.0)
        c1 = a * cloud_c1(n) + (1.0 - a) * rayleigh(n)
        mix = slice(3 - L, 3)  # ... except the mix, which keeps its last two
        kw.update(omega_arr=np.array([0.95, 1 - 1e-6, 0.5])[mix], Leg_coeffs_all=np.stack([rayleigh(n), c1, isotropic(n)])[mix],
                  f_arr=np.array([0.0, c1[NQuad], 0.0])[mix], BDRF_Fourier_modes=[0.3])
    else:
        raise KeyError(key)
    return kw


def points(kw):
    """tau = 0, every interface, the bottom and one interior point per layer; the three azimuths."""
    edges = np.concatenate(([0.0], np.atleast_1d(kw["tau_arr"])))
    return np.sort(np.concatenate((edges, edges[:-1] + 0.4 * np.diff(edges)))), PHI


def fixture_path(key):
    return os.path.join(HP_DIR, f"phase_{key}.npz")


def truncation_minimum(kw, nangles=4001):
    """Per layer the minimum over nangles cosines of the phase function the solver sees: the first NQuad moments, delta-M-scaled
    (chi - f) / (1 - f) where f > 0."""
    x = np.linspace(-1.0, 1.0, nangles)
    NQuad = kw["NQuad"]
    leg = np.atleast_2d(kw["Leg_coeffs_all"])[:, :NQuad]
    f = np.broadcast_to(np.atleast_1d(kw.get("f_arr", 0.0)), (leg.shape[0],))
    out = []
    for chi, fl in zip(leg, f):
        scaled = (chi - fl) / (1.0 - fl)
        out.append(float(np.polynomial.legendre.legval(x, (2 * np.arange(NQuad) + 1) * scaled).min()))
    return np.array(out)


def batch_kwargs(NQuad):
    """The six columns of a stream count stacked for ``pydisort_batch``: per-column f_arr (zeros without delta-M), bdrf_q tables (zeros
    without a surface), a zero thermal polynomial for the columns without a source.  -> (kwargs, tau [6, ntau])."""
    from pydisort_amd._prepare import double_gauss
    N, L = NQuad // 2, layer_count(NQuad)
    mu, _ = double_gauss(N)
    cols = [case(f"{NQuad}_{c}") for c in COLUMNS]
    C = len(cols)
    bq, bq0 = np.zeros((C, 2, N, N)), np.zeros((C, 2, N))
    sp, b_pos, b_neg, f = np.zeros((C, L, 3)), np.zeros((C, N)), np.zeros(C), np.zeros((C, L))
    for c, kw in enumerate(cols):
        for m, mode in enumerate(kw.get("BDRF_Fourier_modes", [])):
            if np.isscalar(mode):
                bq[c, m], bq0[c, m] = mode, mode
            else:
                bq[c, m], bq0[c, m] = mode(mu, mu), mode(mu, np.array([kw["mu0"]]))[:, 0]
        if "s_poly_coeffs" in kw:
            sp[c, :, :kw["s_poly_coeffs"].shape[1]] = kw["s_poly_coeffs"]
        b_pos[c] = kw.get("b_pos", 0.0)
        b_neg[c] = kw.get("b_neg", 0.0)
        f[c] = kw.get("f_arr", 0.0)
    out = dict(tau_arr=np.stack([kw["tau_arr"] for kw in cols]), omega_arr=np.stack([kw["omega_arr"] for kw in cols]), NQuad=NQuad,
               Leg_coeffs_all=np.stack([kw["Leg_coeffs_all"] for kw in cols]), mu0=np.full(C, MU0),
               I0=np.array([kw["I0"] for kw in cols]), phi0=np.full(C, PHI0), NFourier=NFOURIER, b_pos=b_pos, b_neg=b_neg, f_arr=f,
               bdrf_q=bq, bdrf_q0=bq0, s_poly_coeffs=sp)
    return out, np.stack([points(kw)[0] for kw in cols])
