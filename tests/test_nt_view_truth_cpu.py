"""tools/nt_view_truth.py -- the 40-digit arbiter of the Nakajima-Tanaka corrections at viewing angles -- checked on its own, on the CPU:

1. With the quadrature nodes as angles its divided-difference form agrees with the plain form (the reference's quotients as they
   stand, which is tools/nt_truth.py's arithmetic) to 1e-30 of the largest term before rounding, and after rounding it reproduces the
   ``truth_*`` arrays of tests/golden/nt bit for bit -- all fixtures of one column, the two near-node ones among them.
2. At mu = -mu0, where the plain form divides by zero (asserted), the divided form agrees to 1e-25 with the mean of the plain form at
   -mu0 (1 +- 2^-60) evaluated in 80 digits (the mean cancels the first-order term in the offset; the second is 2^-120).  The same at
   minus the IMS scaled mu0, where chi is 0 / 0.
3. The fixtures of tests/golden/nt_view regenerate bit for bit from tests/golden/make_nt_view_goldens.py."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import goldens
import nt_truth_cases as NC
import nt_view_cases as VC

mp = pytest.importorskip("mpmath")
sys.path.insert(0, os.path.join(goldens.HERE, "..", "tools"))
import nt_truth  # noqa: E402
import nt_view_truth as VT  # noqa: E402


def flat(t):
    return [v for plane in t for row in plane for v in row]


@pytest.mark.parametrize("name", NC.SINGLE)
def test_nodes_as_angles_reproduce_the_node_fixtures(name):
    case = NC.load(name)
    kw = case.columns[0]
    nodes = nt_truth.quadrature_nodes(kw["NQuad"] // 2)
    mu = np.concatenate((nodes, -nodes))
    divided = VT.terms(kw, mu, case.tau, case.phi, "divided")
    plain = VT.terms(kw, mu, case.tau, case.phi, "plain")
    for o in VT.ORDERS:
        d, p = flat(divided[o]), flat(plain[o])
        rel = max(abs(a - b) for a, b in zip(d, p)) / max(abs(b) for b in p)
        assert rel <= mp.mpf("1e-30"), (o, mp.nstr(rel, 3))
        got = np.array([float(v) for v in d]).reshape(case.truth[o].shape)
        assert got.tobytes() == case.truth[o].tobytes(), o


def _mean_of_plain(kw, centre, tau, phi):
    with mp.workdps(80):
        dl = mp.mpf(2) ** -60
        a = VT.terms(kw, [-centre * (1 + dl)], tau, phi, "plain", dps=80)
        b = VT.terms(kw, [-centre * (1 - dl)], tau, phi, "plain", dps=80)
        return {o: [(x + y) / 2 for x, y in zip(flat(a[o]), flat(b[o]))] for o in VT.ORDERS}


@pytest.mark.parametrize("name", ["q18_L3", "q16_L7_mixed", "q32_L20_thick"])
def test_the_limit_at_minus_mu0(name):
    case = NC.load(name)
    kw = case.columns[0]
    with pytest.raises(ZeroDivisionError):
        VT.terms(kw, [-kw["mu0"]], case.tau, case.phi, "plain")
    got = VT.terms(kw, [-kw["mu0"]], case.tau, case.phi, "divided")
    want = _mean_of_plain(kw, mp.mpf(kw["mu0"]), case.tau, case.phi)
    for o in VT.ORDERS:
        rel = max(abs(x - y) for x, y in zip(flat(got[o]), want[o])) / max(abs(y) for y in want[o])
        print(f"{name} {o}: divided at -mu0 against the plain form around it: {mp.nstr(rel, 3)}")
        assert rel <= mp.mpf("1e-25")


def test_the_limit_at_minus_the_scaled_mu0():
    """|mu| = the scaled mu0 as a float64: chi's x is then ~1e-17 -- the series branch of psi2 -- and the plain form, though finite,
    has spent 34 of its 40 digits; against 80 digits around the point the divided form keeps 1e-25."""
    import make_nt_view_goldens as G
    case = NC.load("q18_L3")
    kw = case.columns[0]
    s = G.scaled_mu0(kw)
    assert 0 < s < 1
    got = VT.terms(kw, [-s], case.tau, case.phi, "divided")
    want = _mean_of_plain(kw, mp.mpf(s), case.tau, case.phi)
    for o in VT.ORDERS:
        rel = max(abs(x - y) for x, y in zip(flat(got[o]), want[o])) / max(abs(y) for y in want[o])
        assert rel <= mp.mpf("1e-25"), (o, mp.nstr(rel, 3))


sys.path.insert(0, os.path.join(goldens.HERE, "golden"))


@pytest.mark.parametrize("name", VC.NAMES)
def test_fixtures_regenerate_bit_for_bit(name):
    spec = importlib.util.spec_from_file_location("make_nt_view_goldens", os.path.join(goldens.HERE, "golden", "make_nt_view_goldens.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert sorted(gen.CASES) == sorted(VC.NAMES) == sorted(f[:-4] for f in os.listdir(VC.DIR) if f.endswith(".npz"))
    res = gen.build(name)
    z = np.load(os.path.join(VC.DIR, name + ".npz"))
    assert sorted(z.files) == sorted(res)
    for k in z.files:
        a = np.asarray(res[k])
        assert a.shape == z[k].shape and a.astype(z[k].dtype).tobytes() == z[k].tobytes(), k
