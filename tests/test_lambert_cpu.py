"""The adding formula of a Lambertian surface as csrc/rtd_lambert.h computes it, on the host: a model of the header that
reproduces its roundings operation by operation (tests/lambert_cases.py) is applied to the REFERENCE's black and lit-from-below
arrays of tests/golden/lambert/ and compared with the reference's own direct solves (``BDRF_Fourier_modes=[A]``,
``b_pos=(1 - A) E``); then the same against the oracle's own three solves on the same inputs, in all three tau-orders.

Cases (lambert_cases.cases): 6 streams x 1 layer with surface emission; 16 x 3 with NT_cor, delta-M and b_neg; 16 x 3 with a linear
thermal source, b_neg and surface emission E = 1.7; 34 x 3; 16 x 3 without delta-M; the thick near-conservative column tau = (2, 12,
30), omega = (0.9999, 0.99999, 0.9999), g = 0.7, where s = 0.869 and 1 / (1 - s) = 7.6.  A in (0, 0.3, 0.95, 1) for each.  The
reference fixtures hold values of every field and antiderivatives of the fluxes (what the reference evaluates correctly without a
beam, see the maker); the oracle covers u, u0, flux_up, flux_down_diffuse and the views of u and u0 in all three orders.

Distance: max |coupled - direct| over the field's largest value, the field one (case, order, field, albedo) array.  Both sides
are float64 solves of different linear systems, so the distance is their conditioning, not the coupling's rounding (which
tests/test_lambert_arith_cpu.py bounds at 8 ulp).  MEASURED (x86-64, this build's NumPy and LAPACK), worst over fields and albedos:
  case            reference: value  antider (fluxes) | oracle: value   antider   deriv
  q6_l1                      7.5e-16   1.0e-15       |         7.0e-16  1.2e-15  4.7e-16
  q16_l3_nt                  2.3e-15   8.6e-16       |         2.9e-15  1.0e-15  1.1e-15
  q16_l3_thermal             2.9e-15   -             |         3.1e-15  1.6e-15  3.0e-15
  q34_l3                     6.6e-15   1.3e-15       |         4.2e-15  1.5e-15  9.8e-16
  q16_l3_nodm                1.8e-15   4.8e-16       |         3.3e-15  7.9e-16  1.5e-15
  q16_thick                  5.2e-15   1.1e-13       |         5.2e-15  1.4e-13  1.6e-15
The antiderivative of the thick near-conservative column stands apart: it divides every homogeneous term by its eigenvalue, and the
diffusion eigenvalue of omega = 0.99999, g = 0.7 is about 0.003, so the two solves' eigenvalue roundings are amplified some 300 times there.  HELD at
ten times the worst figure measured: 7e-14, and 1.4e-12 for the thick column's antiderivatives -- both under the project's
end-to-end ceiling of 1e-9 of the field scale times 1 / (1 - A s), which the assertion checks too."""
import warnings

import numpy as np
import pytest
import scipy.interpolate

import lambert_cases as LC
from oracle import disort_oracle as O

CEILING = 1e-9


def _held(name, order):
    return 1.4e-12 if (name, order) == ("q16_thick", "antider") else 7e-14


def _distance(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_model_of_the_header_couples_the_references_parts_into_its_direct_solves(name):
    kw, E = LC.cases()[name]
    store = LC.load(name)
    assert float(store["E"]) == E and tuple(store["albedos"]) == LC.ALBEDOS
    worst = 0.0
    for order in LC.orders_of(name):
        for field in LC.fields_of(order):
            for i, A in enumerate(LC.ALBEDOS):
                got, _, amp = LC.coupled(store, order, field, A, E)
                d = _distance(got, LC.get(store, f"direct{i}", order, field))
                assert d <= _held(name, order) <= CEILING * amp, (order, field, A, d)
                worst = max(worst, d)
    got0 = LC.coupled(store, "value", "u", 0.0, 0.0)[0]  # A = 0 without emission: the black solve itself, bit for bit
    assert np.array_equal(got0, LC.get(store, "black", "value", "u"))
    print(f"LAMBERT model vs reference {name}: worst {worst:.2e} of the field's largest value")


def _view(x, mu):
    """The reference's ``subroutines.interpolate`` of x [NQuad, ...] at the angles mu: barycentric interpolation in mu, each
    hemisphere on its own, mu > 0 among the upward rows."""
    N = x.shape[0] // 2
    nodes = O.gauss_legendre_01(N)[0]
    out = np.empty((len(mu),) + x.shape[1:])
    out[mu > 0] = scipy.interpolate.BarycentricInterpolator(nodes, x[:N])(mu[mu > 0])
    out[~(mu > 0)] = scipy.interpolate.BarycentricInterpolator(-nodes, x[N:])(mu[~(mu > 0)])
    return out


def _oracle_store(kw, E):
    """The oracle's own black, lit-from-below and direct solves laid out like a fixture, in all three tau-orders."""
    tau, mu = LC.points(kw), LC.view_mu(kw["NQuad"])
    solves = [kw, LC.below_kwargs(kw)] + [dict(kw, BDRF_Fourier_modes=[A], b_pos=(1.0 - A) * E) for A in LC.ALBEDOS]
    store = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        results = [O.pydisort(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}) for s in solves]
    for order, flags in (("value", {}), ("antider", dict(is_antiderivative_wrt_tau=True)), ("deriv", dict(is_derivative_wrt_tau=True))):
        per = {f: [] for f in LC.FIELDS + ("flux_down_direct",)}
        for r in results:
            u0 = np.asarray(r[3](tau, **flags), float).reshape(-1, len(tau))
            u = np.asarray(r[4](tau, LC.PHI, **flags), float).reshape(-1, len(tau), len(LC.PHI)) if len(r) > 4 else np.repeat(u0[..., None], len(LC.PHI), -1)
            down = r[2](tau, **flags)
            per["u"].append(u)
            per["u0"].append(u0)
            per["flux_up"].append(np.asarray(r[1](tau, **flags), float).reshape(len(tau)))
            per["flux_down_diffuse"].append(np.asarray(down[0], float).reshape(len(tau)))
            per["flux_down_direct"].append(np.broadcast_to(np.asarray(down[1], float), (len(tau),)).copy())
            per["u0_mu"].append(_view(u0, mu))
            per["u_mu"].append(_view(u, mu))
        for f, arrays in per.items():
            store[f"{order}.{f}"] = np.stack(arrays)
    return store


@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_model_of_the_header_couples_the_oracles_parts_into_its_direct_solves(name):
    kw, E = LC.cases()[name]
    store = _oracle_store(kw, E)
    worst = 0.0
    for order in ("value", "antider", "deriv"):
        for field in LC.FIELDS:
            for i, A in enumerate(LC.ALBEDOS):
                got, _, amp = LC.coupled(store, order, field, A, E)
                d = _distance(got, LC.get(store, f"direct{i}", order, field))
                assert d <= _held(name, order) <= CEILING * amp, (order, field, A, d)
                worst = max(worst, d)
    print(f"LAMBERT model vs oracle {name}: worst {worst:.2e} of the field's largest value")
