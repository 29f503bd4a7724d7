"""The host side of the thermal entry points under the address / undefined-behaviour sanitizers, as a stand-alone program.

tests/cpu/thermal_host_main.cpp is compiled together with csrc/rtd_api.hip (as it is) and the shadow launchers of
tests/cpu/host_asan_shadow.cpp against the stand-in runtime of tests/cpu/fake_hip, with the sanitizer runtimes linked in
statically, and run directly.  The thermal kernels are rtd_api.hip's own, so the stand-in runtime runs them thread by thread on heap memory: the carve of the staging block, every
NULL combination of rtd_thermal, the padded BDRF rows of the Kirchhoff sum and the tail of rtd_planck_band's grid are all
bounds-checked on the CPU before they ever run on a GPU."""
import host_program


def test_thermal_entry_points_are_clean_under_the_sanitizers(tmp_path):
    r = host_program.build_and_run(tmp_path, "thermal_host_main.cpp", "thermal_host")
    assert r.returncode == 0 and "THERMAL HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
