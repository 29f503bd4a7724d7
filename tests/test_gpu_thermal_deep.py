"""Deep thermal source polynomials against 40-digit truth of the USER's inputs (tests/thermal_deep_cases.py; fixtures
tests/golden/hp/thermal_<NQuad>_<name>.npz from tools/hp_truth_case.py thermal ..., checked on the CPU by
tests/test_thermal_deep_cpu.py): polynomials of degree 1 ... 19 per layer, stated in the absolute optical depth down to tau = 90,
through every implementation of the thermal stage (6, 16, 30, 32, 64, 96, 128 streams) and all three entries -- ``pydisort()``
column by column, ``pydisort_batch`` prepared on the host, and prepared on the device.  The truth forms the source about each
layer's top from the raw float64 coefficients in exact arithmetic; the float64 oracle (= the reference's algorithm) is up to 2e-2
of the scale away from it under delta-M at degree 19 and further without (the fixtures record it), so it is no party here.

Held, per column and entry: u0, flux_up and both parts of flux_down -- the value, d/dtau and the antiderivative in tau -- at
tau = 0, every interface, the bottom and one interior point per layer.  The tolerances are the project's ceilings, not measurements
of this code: values 1e-9 of the field's scale and 1e-6 pointwise (tests/test_gpu_random_parity.py: arbitrated), derivative 1e-7 and
antiderivative 2e-8 of their own scale (tests/test_gpu_random_orders.py); the column with a 1e-3-thin layer (linear source) is held to
the same.  Host- and device-prepared batches agree to 1e-12 of the scale in every value and derivative.  Columns of one coefficient
count form one small batch and a plan of their own: Ns = 2, 4, 6, 10, 14, 20 everywhere, Ns = 17 at 16 and 32 streams.

Measured on one MI355X, the worst over all columns, entries and quantities (the oracle's u0 beside it: 2e-2 of the scale at d19,
1.5 ... 5 at n19): values 4.7e-14 of the scale (64_d13), derivative 1.3e-14 (96_n19), antiderivative 4.9e-10 (64_d19).  Before
the double-double routines of csrc/rtd_dd.h switched contraction off, the device-prepared batches were 2e-8 (degree 9), 1e-5
(degree 13) and 2.5e-3 (degree 19) of the scale away: fused multiply-adds inside the error-free transformations.
"""
import warnings

import numpy as np
import pytest

import goldens
import thermal_deep_cases as TD

pytestmark = pytest.mark.gpu

VALUE_TOL = (1e-9, 1e-6)
ORDER_TOL = {"derivative": 1e-7, "antiderivative": 2e-8}
HOST_VS_DEVICE = 1e-12
ORDERS = {"": {}, "derivative.": dict(is_derivative_wrt_tau=True), "antiderivative.": dict(is_antiderivative_wrt_tau=True)}
BATCHES = [(q, ns) for q in TD.STREAMS for ns in sorted(TD.batches(q))]
ONE_COLUMN = [f"{q}_{n}" for q in TD.ONE_COLUMN_STREAMS for n in TD.names(q)]


@pytest.fixture(scope="module")
def amd():
    import pydisort_amd
    from pydisort_amd import _engine
    assert _engine.device_count() >= 1, "no HIP device visible"
    return pydisort_amd


_SOLVED = {}


def batch(amd, NQuad, Ns, device_prepare):
    """{column name: {quantity: array}} of the columns of one coefficient count, solved once as one batch and plan."""
    k = (NQuad, Ns, device_prepare)
    if k not in _SOLVED:
        names = TD.batches(NQuad)[Ns]
        cfg, tau = TD.batch_kwargs(NQuad, names)
        assert cfg["s_poly_coeffs"].shape[2] == Ns
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, sol = amd.pydisort_batch(device_prepare=device_prepare, **cfg)
            out = {n: {} for n in names}
            for prefix, flag in ORDERS.items():
                u0, fup, fd = sol.u0(tau, **flag), sol.flux_up(tau, **flag), sol.flux_down(tau, **flag)
                for c, n in enumerate(names):
                    out[n].update({prefix + "u0": u0[c], prefix + "flux_up": fup[c], prefix + "flux_down_diffuse": fd[0][c],
                                   prefix + "flux_down_direct": fd[1][c]})
        assert not np.any(sol.plan.column_status())
        sol.plan.close()
        _SOLVED[k] = out
    return _SOLVED[k]


def one_column(amd, key):
    import deriv_cases as D
    kw = dict(TD.case(key))
    tau = TD.points(kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = amd.pydisort(only_flux=True, **kw)
        out = {}
        for prefix, flag in ORDERS.items():
            out.update({prefix + q: v for q, v in D.evaluate(res, tau, None, **flag).items()})
    return out


def held(label, key, fields):
    """Every quantity and order of one column against its fixture; all are measured and recorded before the test fails."""
    from conftest import record_parity
    z = np.load(TD.fixture_path(key))
    assert np.array_equal(z["tau"], TD.points(TD.case(key)))
    failures = []
    for prefix in ORDERS:
        order = prefix.rstrip(".")
        for q in ("u0", "flux_up", "flux_down_diffuse"):
            got = np.asarray(fields[prefix + q], float)
            assert got.shape == z[prefix + q].shape and np.all(np.isfinite(got)), (label, prefix + q)
            a, b = goldens.max_rel_err(got, z[prefix + q])
            tol = VALUE_TOL if not order else (ORDER_TOL[order], None)
            print(f"thermal-deep {label} {prefix + q}: {a:.3e} of the scale, {b:.3e} pointwise (oracle's u0 {float(z['oracle_u0_scale_rel']):.1e})")
            try:
                record_parity(f"thermal_deep/{label}/{prefix + q}", a, b, tol[0], tol[1], against="40-digit truth",
                              oracle_vs_truth_scale_rel=float(z["oracle_u0_scale_rel"]))
            except AssertionError as e:
                failures.append(str(e))
        direct = np.asarray(fields[prefix + "flux_down_direct"], float)
        assert not np.any(direct), (label, prefix, "a direct beam without a beam")
    assert not failures, failures


@pytest.mark.parametrize("device_prepare", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("NQuad,Ns", BATCHES)
def test_batch_of_one_coefficient_count_against_truth(amd, NQuad, Ns, device_prepare):
    got = batch(amd, NQuad, Ns, device_prepare)
    failures = []
    for name, fields in got.items():
        try:
            held(f"{'device' if device_prepare else 'host'} {NQuad}_{name}", f"{NQuad}_{name}", fields)
        except AssertionError as e:  # every column is measured before the test fails
            failures.append((name, str(e)))
    assert not failures, failures


@pytest.mark.parametrize("key", ONE_COLUMN)
def test_one_column_against_truth(amd, key):
    held(f"pydisort {key}", key, one_column(amd, key))


@pytest.mark.parametrize("NQuad,Ns", BATCHES)
def test_host_and_device_prepared_batches_agree(amd, NQuad, Ns):
    """Both preparations run ONE routine on the user's polynomials (csrc/rtd_dd.h: rtd_source_local) for three and more coefficients;
    what is left between them is the rounding of the rescale factor (a division here, a product with the reciprocal there) and of
    the linear road: 1e-12 of the scale for every value and tau-derivative.  The antiderivative is the reference's, of the ABSOLUTE
    form: the evaluator re-expands the local coefficients about tau* = 0 (rtd_eval.hip), which multiplies a last-bit difference of
    the coefficients by the cancellation of that form -- 1e5 at 20 coefficients -- in both batches alike.  There the two are held
    to the ceiling each of them is held to against the truth."""
    from conftest import record_parity
    host, dev = batch(amd, NQuad, Ns, False), batch(amd, NQuad, Ns, True)
    worst = {"": 0.0, "antiderivative": 0.0}
    for name in host:
        for q, a in host[name].items():
            b = dev[name][q]
            scale = float(np.max(np.abs(a)))
            d = float(np.max(np.abs(a - b))) / scale if scale > 0 else float(np.max(np.abs(b)))
            k = "antiderivative" if q.startswith("antiderivative.") else ""
            worst[k] = max(worst[k], d)
    print(f"thermal-deep host vs device {NQuad} streams, Ns = {Ns}: {worst['']:.3e} of the scale; antiderivative {worst['antiderivative']:.3e}")
    record_parity(f"thermal_deep/host_vs_device/{NQuad}_Ns{Ns}/antiderivative", worst["antiderivative"], 0.0, ORDER_TOL["antiderivative"],
                  None, against="device-prepared batch")
    record_parity(f"thermal_deep/host_vs_device/{NQuad}_Ns{Ns}", worst[""], 0.0, HOST_VS_DEVICE, None, against="device-prepared batch")
