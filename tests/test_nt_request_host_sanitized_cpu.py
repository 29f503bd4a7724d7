"""The host side of rtd_plan_request_nt / rtd_plan_get_nt under the address / undefined-behaviour sanitizers, as a stand-alone
program.

tests/cpu/nt_request_host_main.cpp is compiled together with csrc/rtd_api.hip (as it is) and the shadow launchers of
tests/cpu/host_asan_shadow.cpp against the stand-in runtime of tests/cpu/fake_hip, with the sanitizer runtimes linked in
statically, and run directly.  Raw, thermal and band uploads with and without a request, on plans of one window, of windows of 4
and retained.  The preparation kernels of the corrections' inputs are rtd_api.hip's own, so the stand-in runtime runs them thread
by thread on heap memory: the carve of a band's unweighted moments in the staging block, the plan's buffers with one row of the
weighted phase function per profile, what rtd_plan_get_nt copies out (by value), the refusals and their order before any
allocation, and the windows of an evaluation of raw columns -- all bounds-checked on the CPU before any of it runs on a GPU."""
import host_program


def test_request_entry_points_are_clean_under_the_sanitizers(tmp_path):
    r = host_program.build_and_run(tmp_path, "nt_request_host_main.cpp", "nt_request_host")
    assert r.returncode == 0 and "NT REQUEST HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
