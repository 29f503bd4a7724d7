"""The host side of the viewing-angle entry points under the address / undefined-behaviour sanitizers, as a stand-alone program.

tests/cpu/view_host_main.cpp is compiled together with csrc/rtd_api.hip (as it is) and the shadow launchers of
tests/cpu/host_asan_shadow.cpp against the stand-in runtime of tests/cpu/fake_hip, with the sanitizer runtimes linked in
statically, and run directly: no preloaded library, no Python.  rtd_view_basis_kernel, rtd_view_apply_kernel and
rtd_band_reduce_kernel are rtd_api.hip's own, so the stand-in runtime runs them thread by thread on heap memory:
rtd_plan_set_view_mu, rtd_plan_fetch_view and rtd_plan_fetch_band_view after run, run_fetch, evaluate and evaluate_band, in all
three tau-orders, with shared and per-column angles, each output NULL in turn, windows of 4 over 15 columns in groups of 5,
nphi = 0, the lazily grown buffers, withdrawal by nmu = 0, a new quadrature, and every RTD_ERR_STATE / RTD_ERR_ARG case of
include/rtd.h including unequal angles inside a band profile -- all bounds-checked on the CPU, and every element recomputed in
long double from the u / u0 fetched from the same plan, before any of it runs on a GPU."""
import host_program


def test_view_entry_points_are_clean_under_the_sanitizers(tmp_path):
    r = host_program.build_and_run(tmp_path, "view_host_main.cpp", "view_host")
    assert r.returncode == 0 and "VIEW HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
