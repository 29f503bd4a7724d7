"""The cases of the viewing-angle fixtures (tests/golden/view/*.npz) and a NumPy model of the device's interpolation in mu, shared by
the maker (tests/golden/make_view_goldens.py), the CPU test that pins the model to the reference (tests/test_view_cpu.py) and the
GPU tests (tests/test_gpu_view.py).

The model follows csrc/rtd_api.hip operation by operation (rtd_view_basis_kernel, rtd_view_apply_kernel, view_weights):

    b_j    = 1 / prod_{k != j} (x_j - x_k)      long double, k ascending, divided by max |b|, rounded once   (host)
    a      = |mu|;  rows 0 .. N-1 when mu > 0, else rows N .. 2N-1 (+0.0 and -0.0 included)
    a == x_j:  the result is row j, copied
    else   t_j = b_j / (a - x_j);  s = t_0 + t_1 + ... (j ascending);  l_j = t_j / s
           out = l_0 X_0, then += l_j X_j for j = 1 .. N-1

in float64, without fused multiply-adds (the device compiler may contract the chain's products into its additions: fewer roundings,
inside the same bound)."""
import os
import warnings
from fractions import Fraction

import numpy as np

import actinic_cases as A

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "view")
PHI = np.array([0.0, 2.1])
TOL = 1e-9


def cases():
    """name -> keyword arguments of the one-column ``pydisort`` (the reference's, the oracle's and this project's alike): 6, 16 and
    34 streams over three layers; Nakajima-Tanaka corrections; a thermal source; no delta-M scaling."""
    full = dict(only_flux=False)
    return {
        "L3_q6": A.hg_column(3, 6, g=0.6, **full),
        "L3_q16": A.hg_column(3, 16, **full),
        "L3_q34": A.hg_column(3, 34, **full),
        "L3_q16_nt": A.hg_column(3, 16, seed=5, NT_cor=True, **full),
        "L3_q16_thermal": A.hg_column(3, 16, seed=1, s_poly_coeffs=np.array([[0.30, 0.10], [0.42, 0.05], [0.20, 0.12]]), **full),
        "L3_q16_no_deltam": A.hg_column(3, 16, delta_m=False, **full),
    }


# the reference's own tau-antiderivative of the thermal particular solution is not one (tests/actinic_cases.py: VALUE_ONLY)
VALUE_ONLY = ("L3_q16_thermal",)


def nodes(NQuad):
    """The positive quadrature cosines as the project's plans hold them."""
    import sys
    pkg = os.path.join(os.path.dirname(HERE), "pythonic-disort_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from pydisort_amd._prepare import double_gauss
    return np.asarray(double_gauss(NQuad // 2)[0], float)


def mu_list(x):
    """1, a node exactly, the float next above a node, an interior point, +0.0, an interior point below, a negated node, -1."""
    x = np.asarray(x, float)
    return np.array([1.0, x[1], np.nextafter(x[1], 2.0), 0.37, 0.0, -0.62, -x[len(x) // 2], -1.0])


def points(kw):
    """tau = 0, every interface (the last is the bottom) and two interior depths."""
    t = np.asarray(kw["tau_arr"], float)
    return np.concatenate(([0.0], t, [0.4 * t[0], t[0] + 0.6 * (t[1] - t[0])]))


def weights(x):
    """The barycentric weights as the host forms them (view_weights): long double, rounded once."""
    x = np.asarray(x, np.longdouble)
    b = np.empty(len(x), np.longdouble)
    for j in range(len(x)):
        prod = np.longdouble(1.0)
        for k in range(len(x)):
            if k != j:
                prod = prod * (x[j] - x[k])
        b[j] = np.longdouble(1.0) / prod
    return np.asarray(b / np.max(np.abs(b)), np.float64)


def basis(mu, x, b=None):
    """mu [nmu] -> (l [nmu, N], lower [nmu] bool: the rows N .. 2N-1, node [nmu]: j at a node, else -1), as rtd_view_basis_kernel."""
    mu, x = np.atleast_1d(np.asarray(mu, np.float64)), np.asarray(x, np.float64)
    b = weights(x) if b is None else b
    N = len(x)
    l = np.zeros((len(mu), N))
    node = np.full(len(mu), -1)
    for m, v in enumerate(mu):
        a = abs(v)
        hit = np.nonzero(a == x)[0]
        if len(hit):
            node[m] = hit[-1]
            l[m, hit[-1]] = 1.0
            continue
        t = np.array([b[j] / (a - x[j]) for j in range(N)])
        s = np.float64(0.0)
        for j in range(N):
            s = s + t[j]
        l[m] = t / s
    return l, ~(mu > 0), node


def interpolate(mu, x, X, b=None):
    """X [2N, ...] -> [nmu, ...], as rtd_view_apply_kernel: the node's row copied, else one chain, j ascending."""
    X = np.asarray(X, np.float64)
    N = len(x)
    l, lower, node = basis(mu, x, b)
    out = np.empty((len(l),) + X.shape[1:])
    for m in range(len(l)):
        rows = X[N:] if lower[m] else X[:N]
        if node[m] >= 0:
            out[m] = rows[node[m]]
            continue
        acc = l[m, 0] * rows[0]
        for j in range(1, N):
            acc = acc + l[m, j] * rows[j]
        out[m] = acc
    return out


def exact_basis(mu, x):
    """The exact basis of the float64 nodes at the float64 mu (fractions.Fraction): [nmu][N]."""
    xs = [Fraction(float(v)) for v in x]
    N = len(xs)
    w = []
    for j in range(N):
        prod = Fraction(1)
        for k in range(N):
            if k != j:
                prod *= xs[j] - xs[k]
        w.append(1 / prod)
    out = []
    for v in np.atleast_1d(mu):
        a = abs(Fraction(float(v)))
        if a in xs:
            out.append([Fraction(int(xs[j] == a)) for j in range(N)])
            continue
        t = [w[j] / (a - xs[j]) for j in range(N)]
        s = sum(t)
        out.append([v / s for v in t])
    return out


def lebesgue(mu, x):
    """Lambda(mu) = sum_j |l_j(|mu|)| [nmu]: by how much interpolation can amplify an error of the node values."""
    return np.array([float(sum(abs(v) for v in row)) for row in exact_basis(mu, x)])


def oracle(kw):
    """The CPU oracle's (u, u0) closures of one column; u carries the Nakajima-Tanaka corrections when kw asks for them."""
    from oracle import disort_oracle as O
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = O.pydisort(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    return res[4], res[3]


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
