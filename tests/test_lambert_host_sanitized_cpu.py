"""The host side of the Lambertian-sweep entry points under the address / undefined-behaviour sanitizers, as a stand-alone program.

tests/cpu/lambert_host_main.cpp is compiled together with csrc/rtd_api.hip (as it is; a host compiler takes csrc/rtd_lambert.hip
into its unit) and the shadow launchers of tests/cpu/host_asan_shadow.cpp against the stand-in runtime of tests/cpu/fake_hip, with
the sanitizer runtimes linked in statically, and run directly: no preloaded library, no Python.  rtd_lambert_kappa_kernel,
rtd_lambert_couple_kernel, rtd_band_reduce_kernel and the view kernels RUN there thread by thread on heap memory:
rtd_plan_couple_lambert and rtd_plan_couple_lambert_band after run, run_fetch, evaluate and evaluate_band, in all three
tau-orders, with shared, per-column and per-profile albedos, with and without emission, each output NULL in turn, nphi = 0,
windows of 4 over 15 columns in groups of 5, scratch blocks small enough for several chunks (the same bits as one chunk), view
outputs with shared and per-column angles, a column whose 1 - A s is not positive, rtd_lambert_kappa, and every RTD_ERR_ARG /
RTD_ERR_STATE case of include/rtd.h -- all bounds-checked on the CPU, and every element recomputed in long double from the arrays
fetched from the same two plans within the bound of csrc/rtd_lambert.h, before any of it runs on a GPU."""
import host_program


def test_lambert_entry_points_are_clean_under_the_sanitizers(tmp_path):
    r = host_program.build_and_run(tmp_path, "lambert_host_main.cpp", "lambert_host")
    assert r.returncode == 0 and "LAMBERT HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
