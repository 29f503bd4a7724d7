"""Every kernel class against 40-digit truth on deep ill-conditioned chains (tests/chain_cases.py: a five-layer pattern of
near-conservative Rayleigh, cloud C1 with delta-M, a thin isotropic layer, a thick near-conservative Rayleigh layer and a
non-scattering layer, repeated down to 41 layers).  The fixtures are tests/golden/hp/chain_<key>.npz (tools/hp_truth_case.py chain
...); tests/test_chain_truth_cpu.py checks them on the CPU.  On these chains the float64 oracle (= the reference's algorithm) is 1.6e-7
of the scale off at 32 streams and up to 2.5e-5 beyond, two to four orders past the class ceilings: only the truth can hold the kernels.

What the depths are for ("Deep chains"):
  * 32_L19 / L20 / L21 / L41, 18_L21, 30_L21: the refill of the LDS window of rtd_bc_mfma_kernel (RTD_BCF_WIN = 20) in both sweeps,
    with a non-scattering layer last in the window and a near-conservative one first refilled; the GjPiv path meeting that refill;
  * 10_L21 ... 16_L21: the two-layers-ahead operand pipeline of rtd_bc_small_kernel far beyond 8 layers;
  * 34_L25 ... 64_L25: the tiled kernel, and its hand-over to rtd_iface_kernel<32> / rtd_sweep_kernel<32>, on a deep chain;
  * 66_L9 ... 128_L9: the wide kernels' recursion over eight interfaces and their distribution over the XCDs;
  * the five-offset batches at 16, 32, 64 and 96 streams: unlike layers in one eigen wavefront with L no multiple of the pack factor,
    unlike chains in one wavefront of rtd_bc_small_kernel.

Held, per case and path: u, u0, flux_up and both parts of flux_down within  min(10 x MEASURED, outer)  of the truth, in both metrics
of goldens.max_rel_err.  outer is the class ceiling (1e-9 / 1e-6 up to 32 streams, 2e-9 / 1e-6 at 34 ... 64, 2e-8 / 1e-7 beyond); for
the forced fallbacks the project's budget for omega = 1 - 1e-6 problems, 1e-7 / 1e-6.  Per batch in addition: every column within
1e-12 of the scale of its one-column solve.

The run path (set_eval_points at the interfaces, run, fetch) evaluates u^m inside the boundary-condition kernel's backward sweep;
tests/test_gpu_parity.py compares it with the evaluation kernel, which reads the same coefficients.  Here it is held to the truth's
rows at the interfaces (every second point of a fixture).

MEASURED: the worst of the five quantities on one MI355X, per label as the parity report prints it (chain/<label>); beside it the
float64 oracle's distance from the same truth for u, as the fixture records it.  Every batch column was bit-equal to its one-column
solve.  No figure of the scale is within three orders of its ceiling and none grows with depth (32 streams, L = 19 / 20 / 21 / 41:
1.1e-13, 1.0e-13, 1.0e-13, 9.3e-14).  Pointwise, the chains beyond 64 streams stand out (5.0e-8 ... 2.0e-7, two above the class's
1e-7): see FLOAT64_COST.  10_L21 (8.0e-13) is the resonance of 10_c0 (tests/test_gpu_phase_truth.py) on a deep chain.
"""
import warnings

import numpy as np
import pytest

import chain_cases as C
import goldens

pytestmark = pytest.mark.gpu

QUANTITIES = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct")
BATCH_VS_ONE_COLUMN = 1e-12
FORCED_BUDGET = (1e-7, 1e-6)

RUN_PATH = ("16_L21", "32_L21", "32_L41", "64_L25")
PIVOT_KEYS = ("18_L21", "32_L21", "32_L41")
HANDOVER_KEYS = ("34_L25", "64_L25")
HANDOVER_BATCH = (64, 25)
FORCED = ([("RTD_BC_FORCE_PIVOT", v, k) for v in ("1", "2") for k in PIVOT_KEYS]
          + [("RTD_BC_FORCE_HANDOVER", "1", k) for k in HANDOVER_KEYS])

#   label: (of the scale, pointwise)                                          oracle's u: of the scale / pointwise
MEASURED = {
    "8_L9": (4.0e-14, 9.6e-14),                                               # 1.2e-10 / 8.0e-10
    "10_L21": (8.0e-13, 2.2e-12),                                             # 5.4e-10 / 2.4e-09
    "14_L21": (4.3e-14, 1.8e-13),                                             # 1.9e-09 / 8.9e-09
    "16_L21": (4.5e-14, 2.4e-13),                                             # 7.2e-09 / 3.2e-08
    "18_L21": (6.4e-14, 4.4e-13),                                             # 1.0e-08 / 5.0e-08
    "30_L21": (6.8e-14, 1.9e-10),                                             # 3.1e-09 / 2.8e-08
    "32_L19": (1.1e-13, 7.4e-11),                                             # 1.6e-07 / 1.0e-06
    "32_L20": (1.0e-13, 1.1e-09),                                             # 1.6e-07 / 1.2e-06
    "32_L21": (1.0e-13, 2.0e-10),                                             # 1.6e-07 / 1.1e-06
    "32_L41": (9.3e-14, 4.0e-10),                                             # 1.6e-07 / 1.0e-06
    "34_L25": (5.6e-14, 3.6e-09),                                             # 1.1e-07 / 1.0e-06
    "62_L25": (2.1e-13, 4.3e-11),                                             # 1.4e-06 / 2.5e-05
    "64_L25": (2.6e-13, 6.4e-11),                                             # 1.6e-06 / 2.6e-05
    "66_L9": (3.6e-13, 1.2e-11),                                              # 2.0e-06 / 3.4e-05
    "96_L9": (2.7e-13, 5.0e-08),                                              # 5.2e-06 / 1.1e-04
    "98_L9": (4.7e-13, 9.1e-08),                                              # 3.5e-06 / 8.2e-05
    "128_L9": (3.4e-13, 3.0e-10),                                             # 1.2e-05 / 3.1e-04
    "16_L21_s1": (1.8e-14, 1.6e-13),                                          # 2.9e-09 / 3.5e-08
    "16_L21_s2": (3.3e-14, 2.1e-12),                                          # 8.2e-09 / 3.5e-08
    "16_L21_s3": (3.5e-14, 2.4e-13),                                          # 8.2e-09 / 3.1e-08
    "16_L21_s4": (2.5e-14, 6.5e-13),                                          # 7.2e-09 / 3.5e-08
    "32_L21_s1": (2.8e-14, 5.0e-10),                                          # 5.6e-08 / 1.1e-06
    "32_L21_s2": (9.8e-14, 2.1e-10),                                          # 2.5e-07 / 1.1e-06
    "32_L21_s3": (9.7e-14, 3.7e-10),                                          # 2.5e-07 / 1.0e-06
    "32_L21_s4": (9.5e-14, 1.0e-09),                                          # 1.6e-07 / 1.2e-06
    "64_L25_s1": (4.4e-14, 3.7e-11),                                          # 5.1e-07 / 2.3e-05
    "64_L25_s2": (2.3e-13, 2.4e-11),                                          # 5.1e-06 / 2.5e-05
    "64_L25_s3": (2.7e-13, 3.9e-11),                                          # 5.1e-06 / 2.5e-05
    "64_L25_s4": (3.1e-13, 1.6e-11),                                          # 1.6e-06 / 2.3e-05
    "96_L9_s1": (1.1e-13, 8.1e-08),                                           # 1.7e-06 / 1.3e-04
    "96_L9_s2": (2.8e-13, 2.0e-07),                                           # 2.5e-05 / 1.1e-04
    "96_L9_s3": (2.0e-13, 1.2e-07),                                           # 2.5e-05 / 1.2e-04
    "96_L9_s4": (2.2e-13, 5.8e-08),                                           # 5.4e-06 / 1.2e-04
    "run 16_L21": (3.5e-14, 6.5e-13),                                         # 7.2e-09 / 3.2e-08
    "run 32_L21": (8.5e-14, 6.4e-10),                                         # 1.6e-07 / 1.1e-06
    "run 32_L41": (9.1e-14, 5.2e-10),                                         # 1.6e-07 / 1.0e-06
    "run 64_L25": (2.6e-13, 6.2e-11),                                         # 1.6e-06 / 2.6e-05
    "batch 16_L21": (4.5e-14, 2.4e-13),                                       # 7.2e-09 / 3.2e-08
    "batch 16_L21_s1": (1.8e-14, 1.6e-13),                                    # 2.9e-09 / 3.5e-08
    "batch 16_L21_s2": (3.3e-14, 2.1e-12),                                    # 8.2e-09 / 3.5e-08
    "batch 16_L21_s3": (3.5e-14, 2.4e-13),                                    # 8.2e-09 / 3.1e-08
    "batch 16_L21_s4": (2.5e-14, 6.5e-13),                                    # 7.2e-09 / 3.5e-08
    "batch 32_L21": (1.0e-13, 2.0e-10),                                       # 1.6e-07 / 1.1e-06
    "batch 32_L21_s1": (2.8e-14, 5.0e-10),                                    # 5.6e-08 / 1.1e-06
    "batch 32_L21_s2": (9.8e-14, 2.1e-10),                                    # 2.5e-07 / 1.1e-06
    "batch 32_L21_s3": (9.7e-14, 3.7e-10),                                    # 2.5e-07 / 1.0e-06
    "batch 32_L21_s4": (9.5e-14, 1.0e-09),                                    # 1.6e-07 / 1.2e-06
    "batch 64_L25": (2.6e-13, 6.4e-11),                                       # 1.6e-06 / 2.6e-05
    "batch 64_L25_s1": (4.4e-14, 3.7e-11),                                    # 5.1e-07 / 2.3e-05
    "batch 64_L25_s2": (2.3e-13, 2.4e-11),                                    # 5.1e-06 / 2.5e-05
    "batch 64_L25_s3": (2.7e-13, 3.9e-11),                                    # 5.1e-06 / 2.5e-05
    "batch 64_L25_s4": (3.1e-13, 1.6e-11),                                    # 1.6e-06 / 2.3e-05
    "batch 96_L9": (2.7e-13, 5.0e-08),                                        # 5.2e-06 / 1.1e-04
    "batch 96_L9_s1": (1.1e-13, 8.1e-08),                                     # 1.7e-06 / 1.3e-04
    "batch 96_L9_s2": (2.8e-13, 2.0e-07),                                     # 2.5e-05 / 1.1e-04
    "batch 96_L9_s3": (2.0e-13, 1.2e-07),                                     # 2.5e-05 / 1.2e-04
    "batch 96_L9_s4": (2.2e-13, 5.8e-08),                                     # 5.4e-06 / 1.2e-04
    "run batch 16_L21": (3.5e-14, 6.5e-13),                                   # 7.2e-09 / 3.2e-08
    "run batch 16_L21_s1": (3.9e-14, 4.8e-13),                                # 2.9e-09 / 3.5e-08
    "run batch 16_L21_s2": (6.2e-14, 1.3e-10),                                # 8.2e-09 / 3.5e-08
    "run batch 16_L21_s3": (3.0e-14, 1.8e-13),                                # 8.2e-09 / 3.1e-08
    "run batch 16_L21_s4": (2.5e-14, 3.0e-13),                                # 7.2e-09 / 3.5e-08
    "run batch 32_L21": (8.5e-14, 6.4e-10),                                   # 1.6e-07 / 1.1e-06
    "run batch 32_L21_s1": (2.7e-14, 1.0e-09),                                # 5.6e-08 / 1.1e-06
    "run batch 32_L21_s2": (9.9e-14, 5.9e-10),                                # 2.5e-07 / 1.1e-06
    "run batch 32_L21_s3": (1.0e-13, 6.1e-10),                                # 2.5e-07 / 1.0e-06
    "run batch 32_L21_s4": (9.5e-14, 6.0e-10),                                # 1.6e-07 / 1.2e-06
    "run batch 32_L41": (9.1e-14, 5.2e-10),                                   # 1.6e-07 / 1.0e-06
    "run batch 64_L25": (2.6e-13, 6.2e-11),                                   # 1.6e-06 / 2.6e-05
    "run batch 64_L25_s1": (4.4e-14, 9.1e-11),                                # 5.1e-07 / 2.3e-05
    "run batch 64_L25_s2": (2.3e-13, 1.4e-10),                                # 5.1e-06 / 2.5e-05
    "run batch 64_L25_s3": (2.7e-13, 1.1e-10),                                # 5.1e-06 / 2.5e-05
    "run batch 64_L25_s4": (3.5e-13, 7.4e-11),                                # 1.6e-06 / 2.3e-05
    "forced RTD_BC_FORCE_PIVOT=1 18_L21": (6.4e-14, 4.4e-13),                 # 1.0e-08 / 5.0e-08
    "forced RTD_BC_FORCE_PIVOT=1 32_L21": (1.0e-13, 2.0e-10),                 # 1.6e-07 / 1.1e-06
    "forced RTD_BC_FORCE_PIVOT=1 32_L41": (9.3e-14, 4.0e-10),                 # 1.6e-07 / 1.0e-06
    "forced RTD_BC_FORCE_PIVOT=2 18_L21": (6.4e-14, 4.4e-13),                 # 1.0e-08 / 5.0e-08
    "forced RTD_BC_FORCE_PIVOT=2 32_L21": (1.0e-13, 2.0e-10),                 # 1.6e-07 / 1.1e-06
    "forced RTD_BC_FORCE_PIVOT=2 32_L41": (9.3e-14, 4.0e-10),                 # 1.6e-07 / 1.0e-06
    "forced RTD_BC_FORCE_HANDOVER=1 34_L25": (1.1e-13, 8.5e-09),              # 1.1e-07 / 1.0e-06
    "forced RTD_BC_FORCE_HANDOVER=1 64_L25": (2.8e-13, 4.2e-11),              # 1.6e-06 / 2.6e-05
    "forced RTD_BC_FORCE_HANDOVER=1 batch 64_L25": (2.8e-13, 4.2e-11),        # 1.6e-06 / 2.6e-05
    "forced RTD_BC_FORCE_HANDOVER=1 batch 64_L25_s1": (4.3e-14, 2.5e-11),     # 5.1e-07 / 2.3e-05
    "forced RTD_BC_FORCE_HANDOVER=1 batch 64_L25_s2": (2.4e-13, 2.6e-11),     # 5.1e-06 / 2.5e-05
    "forced RTD_BC_FORCE_HANDOVER=1 batch 64_L25_s3": (2.3e-13, 2.3e-11),     # 5.1e-06 / 2.5e-05
    "forced RTD_BC_FORCE_HANDOVER=1 batch 64_L25_s4": (2.5e-13, 2.4e-11),     # 1.6e-06 / 2.3e-05
}


def ceiling(NQuad):
    return (1e-9, 1e-6) if NQuad <= 32 else (2e-9, 1e-6) if NQuad <= 64 else (2e-8, 1e-7)


# Unforced chains whose POINTWISE figure lands above the ceiling of its class (1e-7 beyond 64 streams), explained in DESIGN section 7
# ("Deep chains") with the 40-digit boundary-condition solve and evaluation fed with the device's exported G, K, B: at the interface
# on top of a non-scattering layer the two most grazing upward streams are 2e-8 of the field's scale (just past the metric's
# threshold of 1e-8), and the point is evaluated -- by the reference's rule -- from the near-conservative layer above, as a sum of
# 96 terms of 0.1 of the scale each: the device's absolute error there is 3.9e-15 of the scale (35 ulp of the scale; 1e-14 at the
# neighbouring points, where nothing cancels), the device's tensors cost 6e-18, and the oracle is 1.1e-4 pointwise off on the same
# input.  A float64 cost of the formulation, not a defect: these keep the project's budget for omega = 1 - 1e-6 problems pointwise,
# 1e-6, and the ceiling of their class of the scale; no other bound changes.
FLOAT64_COST = ("96_L9_s2", "96_L9_s3", "batch 96_L9_s2", "batch 96_L9_s3")


def tolerance(label, key, forced=False):
    assert label in MEASURED, f"no measured distance recorded for {label}"
    outer = FORCED_BUDGET if forced else ceiling(C.parse(key)[0])
    if label in FLOAT64_COST:
        outer = (outer[0], FORCED_BUDGET[1])
    return min(10 * MEASURED[label][0], outer[0]), min(10 * MEASURED[label][1], outer[1])


@pytest.fixture(scope="module")
def amd():
    import pydisort_amd
    from pydisort_amd import _engine
    assert _engine.device_count() >= 1, "no HIP device visible"
    return pydisort_amd


def solve_one(amd, key, run_path=False):
    """(the five quantities at the case's points, with run_path the same at the interfaces through the run path, pivoted_chains())
    of a one-column solve; the plan's status is clean.  The plan is closed by hand: an idle one-column plan waits for the next
    call of its shape, and the RTD_BC_FORCE_* switches are read when a plan is built -- a plan left behind here would serve the
    next solve of its shape under the switches of THIS one."""
    kw = C.case(key)
    tau, phi = C.points(kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = amd.pydisort(**kw)
        fd = got[2](tau)
        fields = dict(u=got[4](tau, phi), u0=got[3](tau), flux_up=got[1](tau), flux_down_diffuse=fd[0], flux_down_direct=fd[1])
    plan = got[1].__self__.plan
    assert not np.any(plan.column_status()), (key, plan.column_status())
    chains = plan.pivoted_chains()
    fused = None
    if run_path:
        plan.set_eval_points(C.interfaces(kw)[None], phi)
        plan.run()
        fused = {k: v[0] for k, v in plan.fetch().items()}
        assert not np.any(plan.column_status()), (key, plan.column_status())
    plan.close()
    return fields, fused, chains


_ONE = {}


def one_column(amd, key):
    """``solve_one`` without a switch: solved once and shared with the batch and the forced tests."""
    if key not in _ONE:
        _ONE[key] = solve_one(amd, key, key in RUN_PATH)
    return _ONE[key]


def at_interfaces(z):
    """The truth's rows at the top, the interfaces and the bottom: every second point of the fixture."""
    return {k: (z[k][:, ::2] if k in ("u", "u0") else z[k][::2]) for k in QUANTITIES}


def held(label, key, fields, interfaces_only=False, forced=False):
    from conftest import record_parity
    z = np.load(C.fixture_path(key))
    kw = C.case(key)
    tau, phi = C.points(kw)
    assert np.array_equal(z["tau"], tau) and np.array_equal(z["phi"], phi) and np.array_equal(tau[::2], C.interfaces(kw))
    want = at_interfaces(z) if interfaces_only else z
    worst = [0.0, 0.0]
    for k in QUANTITIES:
        assert np.shape(fields[k]) == np.shape(want[k]) and np.all(np.isfinite(fields[k])), (label, k)
        a, b = goldens.max_rel_err(fields[k], want[k])
        print(f"    {k}: {a:.3e} of the scale, {b:.3e} pointwise")
        worst = [max(worst[0], a), max(worst[1], b)]
    print(f"chain-truth {label}: worst {worst[0]:.3e} of the scale, {worst[1]:.3e} pointwise; oracle u "
          f"{float(z['oracle_u_scale_rel']):.3e} / {float(z['oracle_u_pointwise_rel']):.3e}")
    tol = tolerance(label, key, forced)
    record_parity(f"chain/{label}", worst[0], worst[1], tol[0], tol[1], against="40-digit truth",
                  oracle_vs_truth_scale_rel=float(z["oracle_u_scale_rel"]), oracle_vs_truth_pointwise_rel=float(z["oracle_u_pointwise_rel"]))


@pytest.mark.parametrize("key", C.keys())
def test_one_column_against_truth(amd, key):
    held(key, key, one_column(amd, key)[0])


@pytest.mark.parametrize("key", RUN_PATH)
def test_one_column_run_path_against_truth_at_the_interfaces(amd, key):
    held(f"run {key}", key, one_column(amd, key)[1], interfaces_only=True)


def solve_batch(amd, NQuad, L, run_path):
    cfg, tau = C.batch_kwargs(NQuad, L)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, sol = amd.pydisort_batch(**cfg)
        fd = sol.flux_down(tau)
        out = dict(u=sol.u(tau, C.PHI), u0=sol.u0(tau), flux_up=sol.flux_up(tau), flux_down_diffuse=fd[0], flux_down_direct=fd[1])
    plan = sol.plan
    assert not np.any(plan.column_status()), plan.column_status()
    out["pivoted_chains"] = plan.pivoted_chains()
    if run_path:
        plan.set_eval_points(tau[:, ::2], C.PHI)
        plan.run()
        out["fused"] = plan.fetch()
        assert not np.any(plan.column_status()), plan.column_status()
    plan.close()
    return out


_BATCH = {}


def unforced_batch(amd, NQuad, L):
    if (NQuad, L) not in _BATCH:
        _BATCH[NQuad, L] = solve_batch(amd, NQuad, L, C.key_of(NQuad, L) in RUN_PATH)
    return _BATCH[NQuad, L]


def batch_held(amd, NQuad, L, got, prefix, offsets=C.OFFSETS, interfaces_only=False, forced=False):
    """The columns of a five-offset batch held to the truth and, unforced at the case's points, within BATCH_VS_ONE_COLUMN of their
    one-column solves; every column is measured before the test fails."""
    failures = []
    for s in offsets:
        key = C.key_of(NQuad, L, s)
        fields = {k: got[k][s] for k in QUANTITIES}
        if not (interfaces_only or forced):  # (a forced path is another elimination: not compared with the unforced solve)
            one = one_column(amd, key)[0]
            for k in QUANTITIES:
                d = float(np.max(np.abs(fields[k] - one[k])) / np.max(np.abs(one[k])))
                print(f"chain-truth batch {key} {k}: {d:.3e} of the scale from the one-column solve")
                if not d <= BATCH_VS_ONE_COLUMN:
                    failures.append((key, k, "batch vs one column", d))
        try:
            held(f"{prefix} {key}", key, fields, interfaces_only, forced)
        except AssertionError as e:
            failures.append((key, str(e)))
    assert not failures, failures


@pytest.mark.parametrize("NQuad,L", C.BATCHES)
def test_five_offsets_in_one_batch_against_truth(amd, NQuad, L):
    """Unlike layers side by side in the eigen wavefronts (L = 21, 25, 9: no multiple of 4 or 2, so the last wavefront of a column
    is shared with the next column's first layers) and unlike chains in one wavefront of rtd_bc_small_kernel."""
    batch_held(amd, NQuad, L, unforced_batch(amd, NQuad, L), "batch")


@pytest.mark.parametrize("key", RUN_PATH)
def test_batch_run_path_against_truth_at_the_interfaces(amd, key):
    """The fused interface evaluation of a five-offset batch.  32_L41 has a fixture for offset 0 only: its four other columns ride
    along in the batch and column 0 is held."""
    NQuad, L, _ = C.parse(key)
    got = unforced_batch(amd, NQuad, L)
    batch_held(amd, NQuad, L, got["fused"], "run batch", offsets=C.OFFSETS if (NQuad, L) in C.BATCHES else (0,), interfaces_only=True)


@pytest.mark.parametrize("switch,value,key", FORCED, ids=[f"{s}={v}-{k}" for s, v, k in FORCED])
def test_forced_fallback_against_truth(amd, monkeypatch, switch, value, key):
    """RTD_BC_FORCE_PIVOT=1 (the LDS redo) and =2 (GjPiv) of rtd_bc_mfma_kernel across the window's refill; RTD_BC_FORCE_HANDOVER=1:
    mode 0 of the three leaves rtd_bc_tile2_kernel for the row-per-lane pair on a 25-layer chain -- one chain per column under the
    switch, none without."""
    handover = switch == "RTD_BC_FORCE_HANDOVER"
    if handover:
        assert one_column(amd, key)[2] == 0
    monkeypatch.setenv(switch, value)
    fields, _, chains = solve_one(amd, key)
    print(f"chain-truth forced {switch}={value} {key}: pivoted_chains {chains}")
    assert chains == (sum(m % 3 == 0 for m in range(C.NFOURIER)) if handover else 0)
    held(f"forced {switch}={value} {key}", key, fields, forced=True)


def test_no_solve_runs_under_the_switch_of_another(amd, monkeypatch):
    """``solve_one`` leaves no plan behind: the same chain without, with and again without the hand-over switch is solved by plans
    built under the environment of each call (pivoted_chains() 0, 1, 0)."""
    key = HANDOVER_KEYS[0]
    assert solve_one(amd, key)[2] == 0
    monkeypatch.setenv("RTD_BC_FORCE_HANDOVER", "1")
    assert solve_one(amd, key)[2] == 1
    monkeypatch.delenv("RTD_BC_FORCE_HANDOVER")
    assert solve_one(amd, key)[2] == 0


def test_forced_handover_batch_against_truth(amd, monkeypatch):
    """The five offsets of 64_L25 under RTD_BC_FORCE_HANDOVER=1: the five mode-0 chains go to the row-per-lane pair, the ten
    others stay in the tiled kernel."""
    NQuad, L = HANDOVER_BATCH
    assert unforced_batch(amd, NQuad, L)["pivoted_chains"] == 0
    monkeypatch.setenv("RTD_BC_FORCE_HANDOVER", "1")
    got = solve_batch(amd, NQuad, L, False)
    print(f"chain-truth forced RTD_BC_FORCE_HANDOVER=1 batch {NQuad}_L{L}: pivoted_chains {got['pivoted_chains']}")
    assert got["pivoted_chains"] == len(C.OFFSETS) * sum(m % 3 == 0 for m in range(C.NFOURIER))
    batch_held(amd, NQuad, L, got, "forced RTD_BC_FORCE_HANDOVER=1 batch", forced=True)
