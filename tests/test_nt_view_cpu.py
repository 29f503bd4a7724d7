"""csrc/rtd_nt_view.hip on the host: rtd_nt_view_tables_kernel and rtd_nt_view_apply_kernel, with the routines of csrc/rtd_nt_view.h they
run, compiled over tests/cpu/fake_hip into the stand-alone program tests/cpu/nt_view_host_main.cpp with g++ -fsanitize=address,undefined
and run directly -- the kernels thread by thread on heap blocks of exactly the documented extents, nothing preloaded.

The prepared inputs are the host preparation's (pydisort_amd._prepare / _nt: NumPy, no device).  Held against the 40-digit fixtures of
tests/golden/nt_view on all three tau-orders: max|out - truth| <= tol max|truth| per column, tol by tests/nt_view_cases.py (ten times
the node kernels' figure of the class, the coincidence angles included), everything finite.  Windows of 4 and per-column angles must
give the bits of one window and a shared list.

Seen with g++ on x86-64 (no contraction), worst of the three orders, of max|truth|: q6_L1 1.7e-15, batch6_q16_L3 2.3e-14,
q34_L3 1.1e-13, q16_L4_mu0_near_node 7.9e-15, q16_L4_smu0_near_node 1.1e-14, q32_L20_cloud 1.4e-14.  The worst point of a value or
an antiderivative is as a rule the coincidence angle mu = -mu0 at phi = phi0 itself -- that is the forward direction, where the series is
largest -- and it is no worse than elsewhere (the node formulas lose 1.3e-10 and 1.3e-7 near a node: tests/test_nt_truth_cpu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nt_view_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hexes(a):
    return " ".join(float(v).hex() for v in np.asarray(a, float).ravel())


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("nt_view") / "nt_view_host")
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", "-I", os.path.join(ROOT, "tests", "cpu", "fake_hip"), "-x", "c++",
                    os.path.join(ROOT, "tests", "cpu", "nt_view_host_main.cpp"), "-o", out], check=True)
    return out


def prepared(case):
    from pydisort_amd import _nt
    from pydisort_amd._prepare import prepare_columns
    kw = case.kw
    C = case.C
    N = kw["NQuad"] // 2
    prep = prepare_columns(kw["tau_arr"], kw["omega_arr"], kw["NQuad"], kw["Leg_coeffs_all"], kw["mu0"], kw["I0"], kw["phi0"], kw["NLeg"],
                           kw["NFourier"], None, None, kw["f_arr"], np.zeros((C, kw["tau_arr"].shape[1], 0)), np.zeros((C, 0, N, N)),
                           np.zeros((C, 0, N)))
    return prep, _nt.nt_inputs(prep, kw["omega_arr"], kw["f_arr"], kw["Leg_coeffs_all"], kw["NLeg"], kw["mu0"])


def run(exe, tmp_path, case, order, mu, window, group=1):
    prep, (wfull, f, coef, par) = prepared(case)
    wfull = wfull[::group]
    C, L = case.C, prep["L"]
    nmu, ntau, nphi = mu.shape[-1], case.tau.shape[1], len(case.phi)
    head = f"{C} {L} {prep['P']} {wfull.shape[2]} {nmu} {ntau} {nphi} {int(mu.ndim == 2)} {window} {VC.ORDER_INT[order]} {group}\n"
    arrays = [prep["omega_s"], prep["tau"], prep["tau_s0"], prep["scale_tau"], prep["wleg"], prep["mu0"], prep["I0"], prep["phi0"], prep["rescale"],
              wfull, f, coef, par, mu, case.tau, case.phi]
    path = tmp_path / "in.txt"
    path.write_text(head + "\n".join(hexes(a) for a in arrays) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    rows = [[float.fromhex(v) for v in line.split()] for line in r.stdout.strip().splitlines()]
    return np.array(rows).reshape(C, nmu, ntau, nphi)


@pytest.mark.parametrize("order", VC.ORDERS)
@pytest.mark.parametrize("name", VC.NAMES)
def test_kernels_against_truth(exe, tmp_path, name, order):
    case = VC.load(name)
    got = run(exe, tmp_path, case, order, case.mu, window=case.C)
    assert np.all(np.isfinite(got))
    tol = VC.tolerance(case.kw["NQuad"], order)
    err = VC.worst(got, case.truth[order])
    hot = VC.coincidence(case)
    assert hot.any() or name == "q6_L1"  # (mu0 = 1: the neighbours lie beyond -1 and were dropped; -mu0 = -1 itself is there)
    err_hot = max(float(np.max(np.abs(got[c] - case.truth[order][c])[hot[c]]) / np.max(np.abs(case.truth[order][c])))
                  for c in range(case.C) if hot[c].any())
    print(f"nt-view host {name} {order}: {err:.2e} of max|truth| (coincidence angles {err_hot:.2e}), tol {tol:.2e}")
    assert err <= tol and err_hot <= tol


@pytest.mark.parametrize("order", VC.ORDERS)
def test_windows_and_per_column_angles_keep_the_bits(exe, tmp_path, order):
    """Six columns: one window against windows of 4 (the second one short), the fixture's per-column angles; then one column's list
    shared by all against the same list repeated per column."""
    case = VC.load(VC.BATCH)
    one = run(exe, tmp_path, case, order, case.mu, window=case.C)
    assert np.array_equal(one, run(exe, tmp_path, case, order, case.mu, window=4))
    shared = case.mu[2]
    a = run(exe, tmp_path, case, order, shared, window=4)
    b = run(exe, tmp_path, case, order, np.repeat(shared[None], case.C, axis=0), window=case.C)
    assert np.array_equal(a, b) and np.all(np.isfinite(a))
    assert np.array_equal(a[2], one[2])


def test_columns_that_share_a_row_of_the_full_phase_function(exe, tmp_path):
    """A band's spectral points read one row of wfull per profile, by (c0 + c) / group with windows that are not aligned to the group:
    pairs of columns given the moments of the pair's first column, once as three shared rows (group 2; windows of 4, of 3 -- the
    second one starts in the middle of a pair -- and of 6) and once as six rows of their own -- the same bits."""
    case = VC.load(VC.BATCH)
    for k in ("Leg_coeffs_all", "f_arr"):
        case.kw[k] = np.repeat(case.kw[k][::2], 2, axis=0)
    for window in (4, 3, 6):
        a = run(exe, tmp_path, case, "value", case.mu, window=window, group=2)
        b = run(exe, tmp_path, case, "value", case.mu, window=window)
        assert np.array_equal(a, b) and np.all(np.isfinite(a))
