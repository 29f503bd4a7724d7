"""The interpolation in mu that the device applies (csrc/rtd_api.hip: rtd_view_basis_kernel, rtd_view_apply_kernel), as the NumPy
model of tests/view_cases.py, held against the REFERENCE's ``subroutines.interpolate`` (fixtures tests/golden/view/*.npz, made by
tests/golden/make_view_goldens.py) off the nodes as well as on them.

Tolerance: the model is applied to the CPU oracle's u / u0 at the nodes.  Those are held to the reference at the project's standing
1e-9 of the field's scale, and interpolation amplifies an error of the node values by at most Lambda(mu) = sum_j |l_j(|mu|)|: 1e-9
Lambda(mu) of the scale (the largest magnitude of the reference's array), point by point.  The model's own rounding (test 3's bound,
~1e-14) is far inside.

Figures seen (CPU): worst ratio to that tolerance 5.6e-4 (L3_q34, u_mu, at the node mu = 0.0247 where Lambda = 1: the oracle's own
distance from the reference at a node); off the nodes at worst 5.2e-5 (L3_q16, u0_mu at mu = 0, Lambda = 4.5).  Polynomials: at worst
0.18 of the rounding bound."""
from fractions import Fraction

import numpy as np
import pytest

import view_cases as V

U = Fraction(1, 2 ** 53)


@pytest.mark.parametrize("name", sorted(V.cases()))
def test_model_on_the_oracles_nodes_matches_the_references_interpolate(name):
    kw = V.cases()[name]
    g = V.load(name)
    x = V.nodes(kw["NQuad"])
    mu, tau, phi = g["mu"], g["tau"], g["phi"]
    assert np.array_equal(mu, V.mu_list(x)) and np.array_equal(tau, V.points(kw)) and np.array_equal(g["tau_arr"], kw["tau_arr"])
    u, u0 = V.oracle(kw)
    lam = V.lebesgue(mu, x)
    worst = 0.0
    for suffix, antider in (("", False), (".antider", True)):
        if antider and name in V.VALUE_ONLY:
            continue
        for key, nodes_arr in (("u_mu", np.asarray(u(tau, phi, antider))), ("u0_mu", np.asarray(u0(tau, antider)))):
            want = g[key + suffix]
            got = V.interpolate(mu, x, nodes_arr)
            assert got.shape == want.shape
            scale = np.max(np.abs(want))
            ratio = np.abs(got - want) / (V.TOL * lam.reshape((-1,) + (1,) * (want.ndim - 1)) * scale)
            m = int(np.argmax(np.max(ratio.reshape(len(mu), -1), axis=1)))
            print(f"VIEW CPU {name} {key}{suffix}: worst {np.max(ratio):.2e} of 1e-9 Lambda (at mu = {mu[m]!r}, Lambda = {lam[m]:.2f})")
            assert np.max(ratio) <= 1.0, (name, key, suffix, float(np.max(ratio)))
            worst = max(worst, float(np.max(ratio)))
    print(f"VIEW CPU {name}: worst {worst:.2e}")


@pytest.mark.parametrize("NQuad", [6, 16, 34, 128])
def test_nodes_zero_and_hemispheres(NQuad):
    """A node returns its row bit for bit; +0.0 and -0.0 read the downward rows; mu > 0 the upward ones."""
    x = V.nodes(NQuad)
    N = len(x)
    rng = np.random.default_rng(NQuad)
    X = rng.standard_normal((2 * N, 3, 2))
    X[1, 0, 0] = -0.0
    got = V.interpolate(np.concatenate((x, -x)), x, X)
    assert got.tobytes() == X.tobytes()
    l, lower, node = V.basis([0.0, -0.0, 1e-300, -1e-300, 1.0, -1.0], x)
    assert list(lower) == [True, True, False, True, False, True] and np.all(node == -1)
    assert np.array_equal(l[0], l[1]) and np.array_equal(l[2], l[3])
    zero = V.interpolate([0.0, -0.0], x, X)
    assert np.array_equal(zero[0], zero[1])
    up_only = X.copy()
    up_only[N:] = 0.0
    assert np.all(V.interpolate([0.0, -0.0, -0.3], x, up_only) == 0.0) and np.all(V.interpolate([0.3], x, up_only) != 0.0)
    b = V.weights(x)
    assert np.max(np.abs(b)) == 1.0 and np.all(b != 0.0) and np.all(np.isfinite(b))


@pytest.mark.parametrize("NQuad", [6, 16, 34])
def test_model_reproduces_polynomials_within_its_rounding_bound(NQuad):
    """Polynomials of degree < N in mu with float64 coefficients, evaluated exactly (fractions.Fraction) at the float64 nodes and
    rounded once (upward rows: p(x_j), downward rows: p(-x_j)), come back within gamma_k sum_j |l_j X_j| of the exact interpolant of
    the SAMPLES (k as tests/test_gpu_view.py derives it), and within gamma_(k+1) sum_j |l_j X_j| of the polynomial itself: the
    samples' one rounding is one more unit."""
    x = V.nodes(NQuad)
    N = len(x)
    mu = np.concatenate((V.mu_list(x), np.linspace(-0.99, 0.99, 23)))
    rng = np.random.default_rng(7 + NQuad)
    coef = [[Fraction(float(c)) for c in row] for row in rng.standard_normal((4, N))]

    def poly(c, t):
        acc = Fraction(0)
        for v in c:
            acc = acc * t + v
        return acc

    xs = [Fraction(float(v)) for v in x]
    X = np.array([[float(poly(c, t)) for c in coef] for t in xs + [-t for t in xs]])  # [2N, 4]
    got = V.interpolate(mu, x, X)
    exact = V.exact_basis(mu, x)
    worst = 0.0
    for m, v in enumerate(mu):
        lam = sum(abs(t) for t in exact[m])
        k = N + 4 + 2 * (N + 2) * lam
        gam, gam1 = k * U / (1 - k * U), (k + 1) * U / (1 - (k + 1) * U)
        half = N if not v > 0 else 0
        for e in range(X.shape[1]):
            terms = [exact[m][j] * Fraction(float(X[half + j, e])) for j in range(N)]
            want, size = sum(terms), sum(abs(t) for t in terms)
            err = abs(Fraction(float(got[m, e])) - want)
            assert err <= gam * size, (NQuad, float(v), e, float(err), float(gam * size))
            worst = max(worst, float(err / (gam * size)))
            assert abs(Fraction(float(got[m, e])) - poly(coef[e], Fraction(float(v)))) <= gam1 * size, (NQuad, float(v), e)
    print(f"VIEW CPU polynomials NQuad {NQuad}: worst {worst:.3f} of the rounding bound")
