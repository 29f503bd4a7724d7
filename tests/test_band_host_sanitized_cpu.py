"""The host side of the k-distribution band entry points under the address / undefined-behaviour sanitizers, as a stand-alone
program.

tests/cpu/band_host_main.cpp is compiled together with csrc/rtd_api.hip (as it is) and the shadow launchers of
tests/cpu/host_asan_shadow.cpp against the stand-in runtime of tests/cpu/fake_hip, with the sanitizer runtimes linked in
statically, and run directly.  The mix and reduction kernels are rtd_api.hip's own, so the stand-in runtime runs them thread by
thread on heap memory: the carve of the staging block with and without the thermal description, every optional pointer NULL in
turn, windows that are no multiple of the spectral points, one and two register chunks of weight sets -- all bounds-checked on
the CPU, and every mixed and every reduced element recomputed in long double, before any of it runs on a GPU."""
import host_program


def test_band_entry_points_are_clean_under_the_sanitizers(tmp_path):
    r = host_program.build_and_run(tmp_path, "band_host_main.cpp", "band_host")
    assert r.returncode == 0 and "BAND HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
