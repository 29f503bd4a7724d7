"""Deep ill-conditioned chains: one five-layer pattern repeated down a column of up to 41 layers, so that near-conservative,
non-scattering, thin and delta-M-scaled layers meet every depth-dependent mechanism of the boundary-condition and eigen kernels (plain
NumPy; shared by tools/hp_truth_case.py, which writes the 40-digit fixtures tests/golden/hp/chain_<key>.npz, by
tests/test_chain_truth_cpu.py and by tests/test_gpu_chain_truth.py).  The phase functions, the azimuths and the beam are those of
tests/phase_cases.py.

Layer l of a chain with offset s has type t = (l + s) % 5:
  t  thickness  omega     moments    delta-M
  0  0.3        1 - 1e-6  Rayleigh   -
  1  0.8        0.9       cloud C1   f = chi_NQuad
  2  1e-3       0.5       isotropic  -
  3  2.5        1 - 1e-6  Rayleigh   -
  4  0.05       0.0       isotropic  -
Beam (mu0 = 0.6, I0 = 2, phi0 = 0.5), Lambertian surface 0.3, NFourier = 3, NQuad + 1 moments given, no thermal source (the rule of
phase_cases.py: none beside an omega > 1 - 1e-5 layer).  Points: phase_cases.points (the top, every interface, the bottom, one
interior point per layer at 0.4 of its thickness).

Keys: "<NQuad>_L<L>" for offset 0, "<NQuad>_L<L>_s<k>" for offsets 1 ... 4.  The offsets exist at 16_L21, 32_L21, 64_L25 and 96_L9:
with s = 0 they form a five-column batch in which unlike layers share eigen wavefronts (4 layers per wavefront of
rtd_eigen_kernel<16,2>, 2 problems of <32,2>; L is no multiple of either) and unlike chains share a wavefront of
rtd_bc_small_kernel.

The depths: rtd_bc_mfma_kernel (18 ... 32 streams) keeps RTD_BCF_WIN = 20 layers of a chain resident in LDS and refills the window in
both sweeps.  With s = 0 layer 19, the last of the window, is non-scattering and layer 20, the first refilled, is near-conservative
Rayleigh.  32_L19 / 32_L20 / 32_L21 / 32_L41 are one short of the window, the window, one past it and one past twice it; 18_L21 and
30_L21 cross it at the most-padded and at one pair short of the width.  No other boundary-condition kernel keeps a resident window of
layers (rtd_bc_small, rtd_bc_tile2, rtd_bc_wide and rtd_bc_rows stream every layer; RTD_BCF_WIN is the only such constant in csrc/),
so no second triple exists.  L = 21 at 10 ... 16 streams runs the two-layers-ahead operand pipeline of rtd_bc_small_kernel far beyond
8 layers; L = 25 at 34 ... 64 streams the tiled kernel and its hand-over to the row-per-lane pair on a deep chain; L = 9 at 66 ... 128
streams the wide kernels' recursion over eight interfaces.
"""
import os

import numpy as np

import phase_cases as P
from phase_cases import PHI, MU0, I0, PHI0, rayleigh, isotropic, cloud_c1  # noqa: F401  (PHI, MU0, ... are part of this module)

HP_DIR = P.HP_DIR
NFOURIER = 3
PERIOD = 5
THICKNESS = (0.3, 0.8, 1e-3, 2.5, 0.05)
OMEGA = (1 - 1e-6, 0.9, 0.5, 1 - 1e-6, 0.0)
CLOUD = 1  # the one type with delta-M
SURFACE = 0.3
WINDOW = 20  # RTD_BCF_WIN of csrc/rtd_bc.hip

#  (NQuad, L) of the offset-0 cases
SINGLE = ((8, 9), (10, 21), (14, 21), (16, 21),
          (18, 21), (30, 21), (32, 19), (32, 20), (32, 21), (32, 41),
          (34, 25), (62, 25), (64, 25),
          (66, 9), (96, 9), (98, 9), (128, 9))
BATCHES = ((16, 21), (32, 21), (64, 25), (96, 9))  # these carry the offsets 1 ... 4 as well
OFFSETS = (0, 1, 2, 3, 4)


def key_of(NQuad, L, s=0):
    return f"{NQuad}_L{L}" + (f"_s{s}" if s else "")


def parse(key):
    """-> (NQuad, L, offset)"""
    parts = key.split("_")
    return int(parts[0]), int(parts[1][1:]), int(parts[2][1:]) if len(parts) > 2 else 0


def keys():
    return [key_of(q, L) for q, L in SINGLE] + [key_of(q, L, s) for q, L in BATCHES for s in OFFSETS[1:]]


def layer_types(L, s=0):
    return (np.arange(L) + s) % PERIOD


def case(key):
    """Keyword arguments of the one-column ``pydisort`` for "<NQuad>_L<L>" or "<NQuad>_L<L>_s<k>"."""
    NQuad, L, s = parse(key)
    n = NQuad + 1
    t = layer_types(L, s)
    c1 = cloud_c1(n)
    moments = np.stack([rayleigh(n), c1, isotropic(n), rayleigh(n), isotropic(n)])
    return dict(tau_arr=np.cumsum(np.array(THICKNESS)[t]), omega_arr=np.array(OMEGA)[t], NQuad=NQuad, NFourier=NFOURIER,
                Leg_coeffs_all=moments[t], f_arr=np.where(t == CLOUD, c1[NQuad], 0.0), mu0=MU0, I0=I0, phi0=PHI0,
                BDRF_Fourier_modes=[SURFACE])


def points(kw):
    return P.points(kw)


def interfaces(kw):
    """The top, every interface and the bottom: the points of the run path's fused interface evaluation (a subset of ``points``)."""
    return np.concatenate(([0.0], np.atleast_1d(kw["tau_arr"])))


def fixture_path(key):
    return os.path.join(HP_DIR, f"chain_{key}.npz")


def batch_kwargs(NQuad, L):
    """The five offsets of (NQuad, L) stacked for ``pydisort_batch``, in the layout of phase_cases.batch_kwargs.
    -> (kwargs, tau [5, ntau])."""
    N = NQuad // 2
    cols = [case(key_of(NQuad, L, s)) for s in OFFSETS]
    C = len(cols)
    bq, bq0 = np.zeros((C, 1, N, N)), np.zeros((C, 1, N))
    bq[:], bq0[:] = SURFACE, SURFACE
    out = dict(tau_arr=np.stack([kw["tau_arr"] for kw in cols]), omega_arr=np.stack([kw["omega_arr"] for kw in cols]), NQuad=NQuad,
               Leg_coeffs_all=np.stack([kw["Leg_coeffs_all"] for kw in cols]), mu0=np.full(C, MU0), I0=np.full(C, I0),
               phi0=np.full(C, PHI0), NFourier=NFOURIER, b_pos=np.zeros((C, N)), b_neg=np.zeros(C),
               f_arr=np.stack([kw["f_arr"] for kw in cols]), bdrf_q=bq, bdrf_q0=bq0)
    return out, np.stack([points(kw)[0] for kw in cols])
