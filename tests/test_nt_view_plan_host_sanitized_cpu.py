"""The host side of rtd_plan_set_view_nt under the address / undefined-behaviour sanitizers, as a stand-alone program.

tests/cpu/nt_view_plan_host_main.cpp is compiled together with csrc/rtd_api.hip (as it is; a host compiler takes csrc/rtd_nt_view.hip
into that unit) and the shadow launchers of tests/cpu/host_asan_shadow.cpp against the stand-in runtime of tests/cpu/fake_hip, with the
sanitizer runtimes linked in statically, and run directly.  Plans of one window, of windows of 4, retained in full and lean, with
shared and per-column angles, with and without corrections: the mode's refusals (an unknown mode, mu = 0 in either order of the two
calls), the view of u formed inside the window loop by evaluate, run and run_fetch in all three tau-orders -- the two kernels of
rtd_nt_view.hip RUN there on heap memory, so the window's slice of the view buffer, the one-window table and the per-column angles are
bounds-checked -- the fetch that is refused after a late request and served again after the next evaluation, and what the plan
allocates: nothing until the mode is used."""
import host_program


def test_view_nt_entry_point_is_clean_under_the_sanitizers(tmp_path):
    r = host_program.build_and_run(tmp_path, "nt_view_plan_host_main.cpp", "nt_view_plan_host")
    assert r.returncode == 0 and "NT VIEW PLAN HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
