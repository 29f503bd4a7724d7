"""The host side of the parametric surface models under the address / undefined-behaviour sanitizers, as a stand-alone program.

tests/cpu/surface_host_main.cpp is compiled together with csrc/rtd_api.hip (as it is) and the shadow launchers of
tests/cpu/host_asan_shadow.cpp against the stand-in runtime of tests/cpu/fake_hip, with the sanitizer runtimes linked in
statically, and run directly: no preloaded library, no Python.  rtd_surface_samples_kernel and rtd_surface_lambert_kernel are
rtd_api.hip's own, so the stand-in runtime runs them thread by thread on heap memory: rtd_plan_request_surface followed by
rtd_plan_set_columns_raw, _thermal (Kirchhoff emissivity from the device-formed zeroth mode) and _band, 7 columns with rows = 1, C and
P (and bands of 2 x 3 and 3 x 2 columns whose profiles share a row), RTD_SURFACE_BYTES forcing chunks of 1 and of 3 columns, plans
without a beam, withdrawal of the request, rtd_plan_set_bdrf_samples on top, and every RTD_ERR_ARG / RTD_ERR_STATE case of
include/rtd.h -- all bounds-checked on the CPU; Lambert's tables are checked by value, and every sample the plan-free
rtd_surface_samples returns is recomputed in long double (held to 1e-13 of the row's max |rho|: long double carries 64 bits, the
bound is that of double arithmetic with room for a few ulp per libm call; measured 8.2e-16)."""
import host_program


def test_surface_entry_points_are_clean_under_the_sanitizers(tmp_path):
    r = host_program.build_and_run(tmp_path, "surface_host_main.cpp", "surface_host")
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SURFACE HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
