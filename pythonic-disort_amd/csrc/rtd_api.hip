// rtd_api.hip -- host side of the C ABI declared in include/rtd.h (plan life cycle, uploads, launches).
#include <algorithm>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <type_traits>
#include <vector>

#include "../../include/rtd.h"
#include "rtd_device.h"
#include "rtd_dd.h"
#include "rtd_planck.h"
#include "rtd_nt_prep.h"
#include "rtd_surface.h"
#include "rtd_lambert.h"
#if !defined(__HIPCC__)
// A host compiler sees this unit only over the stand-in runtime of tests/cpu, which RUNS the kernels of the unit it compiles, thread
// by thread on heap memory, and replaces the other units by shadow launchers.  The ocean's mode kernel joins this unit there (one
// lane per pair of cosines, no cross-lane step), so its indexing and every table it writes are bounds-checked and checked by value.
#include "rtd_surface_ocean.hip"
// likewise the corrections at the viewing angles (one thread per (column, angle) / per output, no cross-lane step)
#include "rtd_nt_view.hip"
// and the Lambertian coupling (one thread per column / per output element)
#include "rtd_lambert.hip"
#endif

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// (a failed runtime call also leaves its code in HIP's per-thread "last error": it is taken out here, or the launch check of
//  the next, unrelated, call on this thread -- hipGetLastError after its kernels -- would report it)
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      (void)hipGetLastError();                                                                 \
      return fail(RTD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));             \
    }                                                                                          \
  } while (0)

int pad_pow2(int n) {
  int p = 4;
  while (p < n) p <<= 1;
  return p;
}

// Device-buffer and stream pool (SURVEY section 8(b) "threading": the library owns only device scratch, pooled and
// guarded by a mutex).  Two reasons, two tiers:
//  * one-column pydisort() calls create and destroy a plan per call; recycling small arenas (blocks <= 64 MB, 512 MB in all, a
//    block serves requests down to a quarter of its size) and streams removes the hipMalloc / hipFree / hipStreamCreate cost
//    (milliseconds) from that path;
//  * batch calls create and destroy plans of gigabytes.  hipFree of such a block returns in ~2 ms, but the runtime reclaims the
//    memory lazily, and every so often a later hipMalloc pays for it: 0.4 ... 4.8 s, growing with the bytes freed since
//    (profiles/r05_alloc_outliers.txt: 9 of 40 creations of a 14 GB plan, the same with bare hipMalloc / hipFree).  Blocks above
//    64 MB CAN therefore be kept too, oldest out first, up to a limit PER DEVICE -- but only when the caller asks for it
//    (rtd_pool_set_limit, or RTD_POOL_BYTES in the environment): the default is 0, a library that is imported under someone
//    else's process does not sit on gigabytes of a GPU it shares with that process's allocator (round-5 verdict).  Kept blocks
//    serve requests down to 7/8 of their size -- a serving loop repeats its shapes.  rtd_pool_trim gives everything back; a
//    hipMalloc that fails trims the pool and tries again; evicted blocks are freed OUTSIDE the pool's mutex (hipFree
//    synchronises the device).
struct DevPool {
  struct Block { void* p; size_t bytes; int dev; };
  std::mutex m;
  std::vector<Block> free_blocks, big_blocks;  // (big_blocks in order of arrival)
  std::vector<std::pair<hipStream_t, int>> free_streams;
  std::vector<Block> host_blocks;  // pinned staging slabs of rtd_plan_run_fetch (hipHostMalloc + hipHostFree: ~3 ms per plan)
  size_t cached = 0, big_cached = 0, host_cached = 0;
  int64_t big_cap = -1;  // bytes PER DEVICE; -1: not read from the environment yet
  static constexpr size_t MAX_BLOCK = 64u << 20, MAX_CACHED = 512u << 20;

  int64_t limit_locked() {  // (m held)
    if (big_cap < 0) {
      const char* env = getenv("RTD_POOL_BYTES");
      big_cap = env ? std::max<long long>(0, atoll(env)) : 0;
    }
    return big_cap;
  }
  size_t big_cached_on(int dev) const {
    size_t n = 0;
    for (const Block& b : big_blocks)
      if (b.dev == dev) n += b.bytes;
    return n;
  }
  // blocks of `dev` out, oldest first, until `room` more bytes fit under the limit; the caller frees them outside the lock
  void evict_locked(int dev, int64_t room, int64_t cap, std::vector<Block>* out) {
    int64_t held = (int64_t)big_cached_on(dev);
    for (size_t i = 0; i < big_blocks.size() && held + room > cap;) {
      if (big_blocks[i].dev != dev) {
        ++i;
        continue;
      }
      held -= (int64_t)big_blocks[i].bytes;
      big_cached -= big_blocks[i].bytes;
      out->push_back(big_blocks[i]);
      big_blocks.erase(big_blocks.begin() + i);
    }
  }
  static void release(const std::vector<Block>& blocks) {
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (const Block& b : blocks) {
      if (b.dev != cur) (void)hipSetDevice(b.dev);
      (void)hipFree(b.p);
    }
    if (!blocks.empty() && cur >= 0 && blocks.back().dev != cur) (void)hipSetDevice(cur);
  }
  // bytes >= 0: the new per-device limit; < 0: an eighth of the memory of device `dev`.  Returns the previous limit.
  int64_t set_limit(int64_t bytes, int dev) {
    std::vector<Block> out;
    int64_t prev;
    {
      std::lock_guard<std::mutex> g(m);
      prev = limit_locked();
      if (bytes < 0) {
        size_t fr = 0, total = 0;
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (dev >= 0 && dev != cur) (void)hipSetDevice(dev);
        bytes = hipMemGetInfo(&fr, &total) == hipSuccess ? (int64_t)(total / 8) : 0;
        if (dev >= 0 && dev != cur && cur >= 0) (void)hipSetDevice(cur);
      }
      big_cap = bytes;
      std::vector<int> devs;
      for (const Block& b : big_blocks)
        if (std::find(devs.begin(), devs.end(), b.dev) == devs.end()) devs.push_back(b.dev);
      for (int d : devs) evict_locked(d, 0, big_cap, &out);
    }
    release(out);
    return prev;
  }

  // takes the smallest block of `list` that holds `bytes` and is no larger than `most` (on device `dev`; < 0: any) out of the list
  static void* take_best(std::vector<Block>& list, size_t bytes, size_t most, int dev, size_t* held, size_t* got) {
    int best = -1;
    for (int i = 0; i < (int)list.size(); ++i) {
      const Block& b = list[i];
      if ((dev < 0 || b.dev == dev) && b.bytes >= bytes && b.bytes <= most && (best < 0 || b.bytes < list[best].bytes)) best = i;
    }
    if (best < 0) return nullptr;
    Block b = list[best];
    list.erase(list.begin() + best);
    *held -= b.bytes;
    *got = b.bytes;
    return b.p;
  }
  void* get(size_t bytes, int dev, size_t* got) {
    std::lock_guard<std::mutex> g(m);
    if (bytes > MAX_BLOCK) return take_best(big_blocks, bytes, bytes + bytes / 7, dev, &big_cached, got);
    return take_best(free_blocks, bytes, 4 * bytes + 4096, dev, &cached, got);
  }
  bool put(void* p, size_t bytes, int dev) {
    std::vector<Block> out;
    {
      std::lock_guard<std::mutex> g(m);
      if (bytes <= MAX_BLOCK) {
        if (cached + bytes > MAX_CACHED) return false;
        free_blocks.push_back({p, bytes, dev});
        cached += bytes;
        return true;
      }
      const int64_t cap = limit_locked();
      if ((int64_t)bytes > cap) return false;
      evict_locked(dev, (int64_t)bytes, cap, &out);  // this device's oldest blocks make room; other devices keep theirs
      big_blocks.push_back({p, bytes, dev});
      big_cached += bytes;
    }
    release(out);
    return true;
  }
  void* get_host(size_t bytes, size_t* got) {
    std::lock_guard<std::mutex> g(m);
    return take_best(host_blocks, bytes, 2 * bytes + 4096, -1, &host_cached, got);
  }
  bool put_host(void* p, size_t bytes) {
    std::lock_guard<std::mutex> g(m);
    if (host_cached + bytes > (256u << 20)) return false;
    host_blocks.push_back({p, bytes, -1});
    host_cached += bytes;
    return true;
  }
  // gives the cached blocks of `dev` (-1: every device) back to the runtime; returns the device bytes released
  size_t trim(int dev) {
    std::vector<Block> out, host_out;
    size_t released = 0;
    {
      std::lock_guard<std::mutex> g(m);
      if (dev < 0) {
        host_out.swap(host_blocks);
        host_cached = 0;
      }
      for (std::vector<Block>* list : {&free_blocks, &big_blocks}) {
        std::vector<Block> keep;
        for (const Block& b : *list) {
          if (dev >= 0 && b.dev != dev) {
            keep.push_back(b);
            continue;
          }
          out.push_back(b);
          released += b.bytes;
          (list == &free_blocks ? cached : big_cached) -= b.bytes;
        }
        list->swap(keep);
      }
    }
    for (const Block& b : host_out) (void)hipHostFree(b.p);
    release(out);
    return released;
  }
  hipStream_t get_stream(int dev) {
    std::lock_guard<std::mutex> g(m);
    for (int i = 0; i < (int)free_streams.size(); ++i)
      if (free_streams[i].second == dev) {
        hipStream_t s = free_streams[i].first;
        free_streams.erase(free_streams.begin() + i);
        return s;
      }
    return nullptr;
  }
  void put_stream(hipStream_t s, int dev) {
    std::lock_guard<std::mutex> g(m);
    if (free_streams.size() < 16) free_streams.emplace_back(s, dev);
    else (void)hipStreamDestroy(s);
  }
};
DevPool& pool() {
  static DevPool* p = new DevPool();  // never destroyed: outlives the HIP runtime teardown order
  return *p;
}

// pooled device allocation: returns the block and its true size
hipError_t pooled_malloc(void** q, size_t bytes, int dev, size_t* got) {
  *q = pool().get(bytes, dev, got);
  if (*q) return hipSuccess;
  *got = bytes;
  hipError_t e = hipMalloc(q, bytes);
  if (e == hipErrorOutOfMemory && pool().trim(dev) > 0) {  // what the pool holds is this library's to give up first
    (void)hipGetLastError();
    e = hipMalloc(q, bytes);
  }
  return e;
}
void pooled_free(void* q, size_t bytes, int dev) {
  if (!pool().put(q, bytes, dev)) (void)hipFree(q);
}

// A device buffer that grows on demand (grow, below): the pointer and the doubles it was last allocated for, as one thing.
struct DevBuf {
  double* p = nullptr;
  int64_t cap = 0;
  operator double*() const { return p; }
};

}  // namespace

struct rtd_plan {
  rtd_dims dims{};
  int device = 0;
  int NP = 0;
  hipStream_t stream = nullptr;
  // d.C = all columns.  The per-column INPUT pointers of d cover them all; the intermediates of the solve (Y0, att, Ym, Am,
  // kk, Ek, Bv, dq, zneg, coef, Fws) cover one window of Cw columns: launch_windows runs window after window.
  RtdDev d{};
  int Cw = 0, nwin = 1;
  // Window pipeline (plans of more than one window): the hand-off buffers of the eigen stage exist twice, and the tables +
  // eigen kernel of window w + 1 run on eig_stream while the boundary-condition + evaluation kernels of window w run on
  // `stream`.  The eigen kernel is bound by vector-instruction issue, the boundary-condition kernel by the latency of its
  // dependent chains: wavefronts of both kinds resident on a SIMD fill each other's bubbles (profiles/archive/r03_window_pipeline.json).
  struct HandOff { double *Y0, *att, *Ym, *Am, *kk, *Bv, *dq, *zneg, *Ek, *vb; } slot1{};
  // Legendre tables at -mu0 and beam attenuations of ALL columns, kept from run to run (they depend on the inputs and the
  // mode shard only): one launch after the inputs change instead of one per window and run (19 us of 1.17 ms per 256-column
  // cfg4 window).  Plans of one window keep them in d.Y0 / d.att; larger plans in these arrays when C M P doubles fit 2 GiB.
  double *Y0_all = nullptr, *att_all = nullptr;
  bool tables_cached = false, tables_valid = false;
  bool quad_tables_valid = false;  // the column-independent table Y[m][l][i] matches the quadrature and the mode shard (a plan that is
  //                                 reused for another column of the same shape keeps it: one launch less per one-column solve)
  bool pipelined = false;
  // Retained plan (rtd_plan_create_retained): the eigen stage's hand-off arrays and the coefficients cover ALL columns instead
  // of one window (two slots), so that the evaluators can be called again after a solve without solving again -- what the
  // reference's closures do with GC_collect, K_collect, B_collect (_assemble_intensity_and_fluxes.py:170-262).  Only the
  // boundary-condition workspace Fws (5 of a cfg4 column's 8.4 MB) stays windowed.
  bool retained = false;
  // Lean retained plan (round 6): what cannot be recomputed cheaply stays for ALL columns -- the boundary-condition coefficients,
  // k, E, B and the thermal vectors (0.5 of a cfg4 column's 3.1 MB) -- while Y, A stay windowed; an evaluation re-runs the EIGEN
  // stage for the wavefront chunks its points touch (same wavefront composition as in the solve: same bits), window by window,
  // and never the boundary-condition solve.  10^5 cfg4 columns: 50 GB instead of 310 GB.
  bool lean = false;
  DevBuf sel_buf;  // chunk lists of one window [Cw][nsel] (ints), grown on demand
  bool fork_needed = true;               // inputs were (re)uploaded on `stream` since the last solve: the eigen stream must wait for them
  bool bc_recorded[2] = {false, false};  // ev_bc[slot] has been recorded by some earlier window (possibly of an earlier run)
  // Pipelined plans keep the device status words (status, col_status, sweeps) twice and alternate between them from solve to
  // solve: back-to-back runs overlap (the eigen stream starts run r + 1 while the boundary-condition and evaluation kernels of
  // run r still raise bits on the plan's stream), so run r + 1 clears and fills the other set; the set it clears was last
  // touched by run r - 1, which the eigen stream's first wait (ev_bc of run r) has behind it.
  int *status2[2] = {nullptr, nullptr}, *col_status2[2] = {nullptr, nullptr}, *sweeps2[2] = {nullptr, nullptr};
  int stat_idx = 0;
  hipStream_t eig_stream = nullptr;
  hipEvent_t ev_eig[2] = {nullptr, nullptr}, ev_bc[2] = {nullptr, nullptr}, ev_fork = nullptr;
  std::vector<void*> allocs;
  std::vector<size_t> alloc_bytes;
  int64_t bytes = 0;
  bool have_quad = false, have_cols = false, solved = false;
  int numeric_status = 0;  // RTD_ST_* bits of the last solve other than the tau range: reported until the next solve
  std::vector<double> h_tau;  // host copy of tau_arr [C][L]: recognises evaluation points that are the layer interfaces
  // Host images of the small uploads (quadrature, per-column inputs, evaluation points) live in the plan until the copy that reads
  // them is known to have completed: no hipStreamSynchronize per upload (each costs a one-column pydisort() call 10-20 us; the
  // call's only wait is now the one that brings its results back).  `*_pending`: an asynchronous copy from the image may still be
  // in flight -- the next writer of the image waits for the stream first; every call that drains the stream clears them.
  std::vector<char> quad_img, cols_img;
  std::vector<double> ev_img;
  bool quad_pending = false, cols_pending = false, ev_pending = false;
  // evaluation buffers (grown on demand)
  int eval_order = 0;  // rtd_plan_set_eval_order: -1 antiderivative, 0 value, +1 tau-derivative at the stored points
  bool ev_iface = false;  // the stored evaluation points are [0, tau_arr] of every column (fused evaluation possible)
  DevBuf um_buf;  // [Cw][M][L+1][2 NP]: Fourier modes at the interfaces, written by the boundary-condition kernel
  int ev_ntau = 0, ev_nphi = 0;
  DevBuf ev_tau, ev_phi, ev_u, ev_u0, ev_fl;
  // k-distribution bands (rtd_plan_set_columns_band, rtd_plan_set_band_weights): the columns are P profiles x band_G spectral points;
  // band_w [K][G] on the device, the reduced results [P][K][...] grown on demand like the evaluation buffers
  bool band_cols = false;
  int band_G = 0, band_K = 0;
  DevBuf band_w, rb_u, rb_u0, rb_fl;
  // actinic fluxes (rtd_plan_fetch_actinic, rtd_plan_fetch_band_actinic): res_order is the order (-1 / 0 / +1) the resident
  // results were evaluated in, RES_NONE while the buffers hold no evaluation of the stored points; ev_act [3][C][ntau] and the
  // reduced rb_act [3][P][K][ntau] are grown at the first actinic fetch, so a plan that never asks holds nothing more
  static constexpr int RES_NONE = 2;
  int res_order = RES_NONE;
  DevBuf ev_act, rb_act;
  // radiances at user polar angles (rtd_plan_set_view_mu, rtd_plan_fetch_view, rtd_plan_fetch_band_view).  The request lives on the
  // host until a fetch: view_mu_h is the caller's list [nmu] or [C][nmu], h_mu_pos the plan's positive nodes (set_quadrature), and
  // view_stale says that the device's copy of the angles, the barycentric weights view_b [N] and the basis view_l [C or 1][nmu][N]
  // with its flags view_flag (ints) do not match them.  res_has_u: the latest evaluation formed u (it had azimuths and wanted u).
  // Every buffer below is grown at the first fetch: a plan that never asks holds nothing more.
  int view_nmu = 0;
  bool view_per_column = false, view_stale = true, res_has_u = false;
  std::vector<double> view_mu_h, h_mu_pos;
  DevBuf view_mu, view_b, view_l, view_flag, ev_view_u, ev_view_u0, rb_view_u, rb_view_u0;
  // Corrections at the viewing angles themselves (rtd_plan_set_view_nt, rtd_nt_view.hip).  In mode 1 an evaluation that applies the
  // Nakajima-Tanaka corrections forms the view of u ITSELF, window by window (launch_windows): the interpolant of the uncorrected u into
  // ev_view_u, then the corrections at the angles on top; the fetches copy or reduce ev_view_u as it is.  res_nt: the latest evaluation
  // applied the corrections to u; view_u_resident: it also left the view of u in ev_view_u and neither the angles nor the mode have
  // changed since.  ntv_T [Cw][L][nmu]: the other-layer sums of one window, grown by the first such evaluation -- a plan that never asks
  // holds and launches nothing more.
  int view_nt_mode = 0;
  bool res_nt = false, view_u_resident = false;
  DevBuf ntv_T;
  // export buffers
  double* ex_buf = nullptr;
  // Nakajima-Tanaka corrections (optional)
  RtdNt nt{};
  DevBuf nt_w, nt_f, nt_ic, nt_ip, nt_R;
  bool have_nt = false, nt_tables_ready = false;
  int nt_request = 0;   // rtd_plan_request_nt: nleg_all of the device-formed inputs (0: none); sticky
  int64_t nt_rows = 0;  // rows of nt_w: C, or the P profiles of a band
  // Parametric surface (rtd_plan_request_surface): while surf_model >= 0 the raw uploads form bdrf_q / bdrf_q0 on the device from
  // surf_par [surf_rows][4] (the caller's parameters, copied) instead of taking tables; sticky.  Nothing is held on the device
  // between uploads: the scratch block of the samples and the staged parameters go back to the pool with the upload's staging block.
  int surf_model = -1, surf_nphi = 0;
  int64_t surf_rows = 0;
  std::vector<double> surf_par;
  // RCCL communicator (one rank per GPU)
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_size = 0;
  DevBuf gathered;  // fluxes only [nranks][3][C][ntau] (rtd_comm_allgather_fluxes)
  // gathered u [nranks][C][Q][ntau][nphi] and fluxes [nranks][3][C][ntau] (rtd_comm_allgather_results): the gather runs
  // on comm_stream behind ev_results, and the next run's first evaluation kernel waits for ev_gathered
  DevBuf gathered_u, gathered_fl;
  hipStream_t comm_stream = nullptr, copy_stream = nullptr;
  hipEvent_t ev_results = nullptr, ev_gathered = nullptr;
  bool gather_inflight = false;
  bool gathered_here = false;  // the last results collective left the gathered arrays of ALL ranks on this rank
  // host-to-host pipeline (rtd_plan_run_fetch): two pinned staging slabs, one per window in flight
  char* stage[2] = {nullptr, nullptr};
  size_t stage_bytes = 0, stage_cap[2] = {0, 0};  // bytes in use of each slab; true size of each (a pooled slab may be larger)
  hipEvent_t ev_win[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
  // timing
  bool timing = false;
  static constexpr int NT = 7;  // timed kernels: tables, asm, jacobi, post, iface, sweep, eval
  hipEvent_t evt[NT + 1] = {};
  double ms[NT] = {};
  int64_t nlaunch[NT] = {};
  bool pending[NT] = {};

  // What a change of the inputs undoes.  Every entry point that changes them states its transition through one member below, and
  // this table is the one place that says which flags each touches and why.  FORK: fork_needed = true, the next pipelined solve's eigen
  // stream starts behind what is queued on `stream`; TABLES / QUAD_T / NT_T: tables_valid / quad_tables_valid / nt_tables_ready = false,
  // the all-columns Y0 and att / the column-independent Y / the Nakajima-Tanaka tables are made again; SOLUTION: solved = false and
  // res_order = RES_NONE, nothing to evaluate or fetch; IFACE: ev_iface = false, the stored points are not known to be interfaces.
  //   member           entry points                                    FORK TABLES QUAD_T NT_T SOLUTION IFACE
  //   new_quadrature   rtd_plan_set_quadrature                         yes  yes    yes    yes  yes      -      and have_quad
  //   new_columns      set_columns_impl, set_columns_raw_impl          yes  yes    -      yes  yes      yes    and have_cols, band_cols
  //   (none)           rtd_plan_request_surface                        -    -      -      -    -        -      host state only
  //   solution_stale   rtd_plan_set_bdrf_samples, _solve_layers        -    -      -      -    yes      -
  //   new_mode_shard   rtd_plan_set_mode_shard                         -    yes    yes    -    yes      -
  //   fresh_tables     rtd_plan_invalidate_tables                      yes  yes    yes    -    -        -
  //   touches_handoff  _set_bdrf_samples, _solve_layers, _get_tensors  yes  -      -      -    -        -      EARLY
  // rtd_plan_request_surface changes what the NEXT raw upload does and nothing the plan holds: the tables it makes the upload form
  // are covered by that upload's new_columns, as uploaded tables are.
  // DELIBERATE: the surface samples leave the tables valid (they do not read the surface), and solve_layers has just made them; the
  // mode shard neither forks (it queues nothing on `stream`) nor touches the NT tables (they hold no mode); invalidate_tables keeps the
  // solution fetchable.  EARLY: raised before the arguments are validated, so a REFUSED call (plan not solved, nbdrf = 0, several
  // windows, column out of range) still makes the next pipelined solve fork.  Harmless (one event record and wait) and it looks
  // ACCIDENTAL: the three entry points were written alike.  Kept as it is; tests/golden/host_trace/e.txt pins it.
  enum : unsigned { FORK = 1, TABLES = 2, QUAD_TABLES = 4, NT_TABLES = 8, SOLUTION = 16, IFACE = 32 };
  void invalidate(unsigned what) {
    if (what & FORK) fork_needed = true;
    if (what & TABLES) tables_valid = false;
    if (what & QUAD_TABLES) quad_tables_valid = false;
    if (what & NT_TABLES) nt_tables_ready = false;
    if (what & SOLUTION) { solved = false; res_order = RES_NONE; }
    if (what & IFACE) ev_iface = false;
  }
  void new_quadrature() { have_quad = true; invalidate(FORK | TABLES | QUAD_TABLES | NT_TABLES | SOLUTION); }
  void new_columns(bool band) { have_cols = true; band_cols = band; invalidate(FORK | TABLES | NT_TABLES | SOLUTION | IFACE); }
  void solution_stale() { invalidate(SOLUTION); }
  void new_mode_shard() { invalidate(TABLES | QUAD_TABLES | SOLUTION); }
  void fresh_tables() { invalidate(FORK | TABLES | QUAD_TABLES); }
  void touches_handoff() { invalidate(FORK); }  // works on the hand-off buffers from the plan's own stream
  void stream_drained() { quad_pending = cols_pending = ev_pending = false; }  // no copy reads a host image any more

  template <typename T>
  int alloc(T** p, int64_t n) {
    void* q = nullptr;
    if (n <= 0) n = 1;
    size_t got = 0;
    hipError_t e = pooled_malloc(&q, (size_t)n * sizeof(T), device, &got);
    if (e != hipSuccess)
      return fail(RTD_ERR_HIP, std::string("hipMalloc of ") + std::to_string((size_t)n * sizeof(T)) + " bytes: " + hipGetErrorString(e));
    allocs.push_back(q);
    alloc_bytes.push_back(got);
    bytes += (int64_t)got;
    *p = (T*)q;
    return 0;
  }
};

// the view's basis and its apply launch (defined with the view entry points; launch_windows queues them in rtd_plan_set_view_nt's mode 1)
extern "C" {  // (the linkage of the block they are defined in)
static int view_basis_queued(rtd_plan* p);
static int view_apply_queued(rtd_plan* p, const double* X, int64_t E, int64_t c0, int64_t cnt, double* out);
}

namespace {

// Extents (in doubles) of the results at the stored points and where each lies: ev_u [C][Q][ntau][nphi]; ev_u0 holds u0 [C][Q][ntau],
// then ulast, the same again; ev_fl holds flux_up, flux_down_diffuse and flux_down_direct, [C][ntau] each.
struct ResultShape {
  int64_t C, Qr, nt, np;
  explicit ResultShape(const rtd_plan* p) : C(p->d.C), Qr(2 * p->d.N), nt(p->ev_ntau), np(p->ev_nphi) {}
  int64_t per_column_u() const { return Qr * nt * np; }
  int64_t per_column_u0() const { return Qr * nt; }
  int64_t u() const { return C * per_column_u(); }
  int64_t u0() const { return C * per_column_u0(); }
  int64_t ulast() const { return u0(); }                   // offset of ulast in ev_u0
  int64_t flux() const { return C * nt; }                  // one of the three fluxes
  int64_t flux_at(int f) const { return f * flux(); }      // offset of flux f (0 up, 1 down diffuse, 2 down direct) in ev_fl
  int64_t fl() const { return 3 * flux(); }
};

// Predicates and extents that several entry points share.
// a mode shard or a communicator: the plan holds partial sums over the Fourier modes, which bands and the Lambertian coupling refuse
bool sharded(const rtd_plan* p) { return p->comm || p->d.m0 != 0 || p->d.mstep != 1 || p->d.mtot != p->d.M; }
// the result buffers hold an evaluation of a solve at the stored points (need_order: and res_order says in which tau-order)
bool has_results(const rtd_plan* p, bool need_order) { return p->ev_ntau >= 1 && p->solved && !(need_order && p->res_order == rtd_plan::RES_NONE); }
// rows [P][K] of a reduced array: the profiles of a band x the weight sets
int64_t band_rows(const rtd_plan* p) { return (int64_t)(p->d.C / p->band_G) * p->band_K; }
// a scratch budget of the environment in doubles (env: what getenv gave for RTD_SURFACE_BYTES or RTD_LAMBERT_BYTES; default 256 MiB,
// not a tuned number), and the columns (rows, profiles) it holds at a time: as many as fit, one at least, `limit` at most
int64_t budget_doubles(const char* env) { return std::max<long long>(env ? atoll(env) : (256ll << 20), 8) / 8; }
int64_t columns_per_chunk(int64_t budget, int64_t per_column, int64_t limit) { return std::min<int64_t>(limit, std::max<int64_t>(1, budget / per_column)); }
// blocks of a one-dimensional launch over n elements
dim3 grid_1d(int64_t n, int64_t block = 256) { return dim3((unsigned)((n + block - 1) / block)); }

// A scratch block from the pool for the length of one call: it goes back when the owner leaves scope, on every path.  Nothing may
// still read it then: the call ends in a synchronising copy or wait, or in finish(), which drains the stream of a failed call.
struct Scratch {
  void* p = nullptr;
  size_t got = 0;
  int dev = 0;
  Scratch() = default;
  Scratch(Scratch&& o) : p(o.p), got(o.got), dev(o.dev) { o.p = nullptr; }  // (move-only: the copies are not declared)
  ~Scratch() {
    if (p) pooled_free(p, got, dev);
  }
  hipError_t get(int64_t doubles, int device) {
    dev = device;
    return pooled_malloc(&p, (size_t)doubles * 8, device, &got);
  }
  double* data() const { return static_cast<double*>(p); }
};
// the caller's arrays one after the other from dst on, by synchronous copies (the plan-free entry points); a null array is left out
struct HostPart { const double* src; int64_t n; };
hipError_t upload_parts(double* dst, std::initializer_list<HostPart> parts) {
  hipError_t e = hipSuccess;
  for (const HostPart& q : parts) {
    if (e == hipSuccess && q.src) e = hipMemcpy(dst, q.src, (size_t)q.n * 8, hipMemcpyHostToDevice);
    dst += q.n;
  }
  return e;
}
// the end of a call that worked in a scratch block: 0, or the message of its first failed runtime call, behind a drained stream
int finish(hipError_t e, hipStream_t s, const char* label) {
  if (e == hipSuccess) return 0;
  (void)hipStreamSynchronize(s);
  (void)hipGetLastError();
  return fail(RTD_ERR_HIP, std::string(label) + ": " + hipGetErrorString(e));
}

// a failed creation or a one-call form gives its plan back: the message of what went wrong survives rtd_plan_destroy; returns rc
int destroy_keeping_error(rtd_plan* p, int rc) {
  const std::string keep = g_err;
  rtd_plan_destroy(p);
  g_err = keep;
  return rc;
}

// The device status words of a solve, cleared on the stream whose first eigen kernel raises bits and sweep counts behind the clear.
// (plan_build's own fills stay: the first covers adjacent carves in one fill, the second takes the words in another order.)
hipError_t clear_status(const RtdDev& d, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d.sweeps, 0, sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(d.status, 0, sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(d.col_status, 0, sizeof(int) * (size_t)d.C, st);
  return e;
}

// The Legendre tables at -mu0 and the beam attenuations of ALL columns of `view` into the plan's all-columns arrays, with the column-
// independent table when that is stale too.  The callers hold the condition (tables_cached && !tables_valid; a layer shard: always).
void launch_all_tables(rtd_plan* p, RtdDev view, hipStream_t s) {
  view.Y0 = p->Y0_all;
  view.att = p->att_all;
  rtd_launch_tables(view, s, !p->quad_tables_valid);
  p->quad_tables_valid = p->tables_valid = true;
}

int acquire_stream(int device, hipStream_t* s) {  // from the pool, else a new one
  *s = pool().get_stream(device);
  if (!*s) HIP_TRY(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  return 0;
}
int ensure_event(hipEvent_t* e) {
  if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  return 0;
}
int device_memory(int device, size_t* free_b, size_t* total_b) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemGetInfo(free_b, total_b));
  return 0;
}

// (Re)allocates `b` for `need` doubles.  The old block goes back to the process-wide pool, where another plan on
// another stream may pick it up at once: this plan's streams are drained first (a plain hipFree would have
// synchronised the device).
int grow(rtd_plan* p, DevBuf& b, int64_t need) {
  if (need <= b.cap) return 0;
  if (b.p) {
    (void)hipStreamSynchronize(p->stream);
    if (p->comm_stream) (void)hipStreamSynchronize(p->comm_stream);
    for (size_t i = 0; i < p->allocs.size(); ++i)
      if (p->allocs[i] == b.p) {
        pooled_free(b.p, p->alloc_bytes[i], p->device);
        p->bytes -= (int64_t)p->alloc_bytes[i];
        p->allocs[i] = nullptr;
      }
  }
  b = DevBuf{};
  int rc = p->alloc(&b.p, need);
  if (rc) return rc;
  b.cap = need;
  return 0;
}

// collect timing of stage `k` if an event pair is pending
void harvest(rtd_plan* p) {
  for (int k = 0; k < rtd_plan::NT; ++k) {
    if (!p->pending[k]) continue;
    float t = 0.f;
    if (hipEventElapsedTime(&t, p->evt[k], p->evt[k + 1]) == hipSuccess) {
      p->ms[k] += t;
      p->nlaunch[k] += 1;
    }
    p->pending[k] = false;
  }
}

// the plan's device view restricted to the columns [c0, c0 + cnt): input pointers advanced, intermediates shared
RtdDev window_dev(const rtd_plan* p, int64_t c0, int cnt, int slot = 0) {
  RtdDev w = p->d;
  if (slot == 1) {
    const rtd_plan::HandOff& h = p->slot1;
    w.Ym = h.Ym; w.Am = h.Am;
    if (!p->lean) { w.Y0 = h.Y0; w.att = h.att; w.kk = h.kk; w.Bv = h.Bv; w.dq = h.dq; w.zneg = h.zneg; w.Ek = h.Ek; w.vb = h.vb; }
  }
  if (p->tables_cached) {  // the window's part of the all-columns tables
    w.Y0 = p->Y0_all + c0 * (int64_t)p->d.M * p->d.P;
    w.att = p->att_all + c0 * ((int64_t)p->d.L + 1);
  }
  const int64_t L = w.L, M = w.M, P = w.P, NP = w.NP, Ns = w.Ns, NB = w.NBDRF;
  if (p->retained || p->lean) {  // every column has its own place in the hand-off arrays and the coefficients
    if (p->retained) { w.Ym += c0 * M * L * NP * NP; w.Am += c0 * M * L * NP * NP; }  // (lean: Y, A stay windowed)
    w.kk += c0 * M * L * NP; w.Ek += c0 * M * L * NP;
    w.Bv += c0 * M * L * 2 * NP; w.coef += c0 * M * L * 2 * NP; w.dq += c0 * L * Ns * 2 * NP; w.zneg += c0 * L * NP;
    if (Ns > 0) w.vb += c0 * L * 4 * NP;
  }
  w.C = cnt;
  w.omega += c0 * L; w.tau += c0 * L; w.taus0 += c0 * (L + 1); w.scale += c0 * L; w.wleg += c0 * L * P;
  w.mu0 += c0; w.I0 += c0; w.phi0 += c0; w.rescale += c0;
  w.bpos += c0 * M * NP; w.bneg += c0 * M * NP; w.spoly += c0 * L * Ns;
  w.bdrfq += c0 * NB * NP * NP; w.bdrfq0 += c0 * NB * NP; w.lperm += c0 * L;
  w.col_status += c0;
  return w;
}
RtdEval window_eval(const rtd_plan* p, const RtdEval& e, int64_t c0) {
  RtdEval w = e;  // (made by make_eval at the plan's stored points: e.ntau, e.nphi are the shape's)
  const ResultShape r(p);
  w.tau += c0 * r.nt;
  if (w.u) w.u += c0 * r.per_column_u();
  if (w.u0) w.u0 += c0 * r.per_column_u0();
  if (w.ulast) w.ulast += c0 * r.per_column_u0();
  if (w.fup) w.fup += c0 * r.nt;
  if (w.fdn) w.fdn += c0 * r.nt;
  if (w.fdir) w.fdir += c0 * r.nt;
  return w;
}
RtdNt window_nt(const rtd_plan* p, int64_t c0) {
  RtdNt w = p->nt;
  const int64_t L = p->d.L;
  if (w.group > 1) w.c0 = c0;  // rows shared by a band's spectral points: the kernel forms (c0 + c) / group itself
  else w.wfull += c0 * L * w.nleg_all;
  w.f += c0 * L; w.ims_coef += c0 * w.nleg_all; w.ims_par += c0 * 2;
  w.R += c0 * 4 * p->d.NP * L;
  return w;
}
// the window's angles, its slice of the view of u (E doubles per column and angle) and the one-window table of the other-layer sums
RtdNtView window_nt_view(const rtd_plan* p, int64_t c0, int64_t E) {
  RtdNtView v{};
  v.nmu = p->view_nmu;
  v.mu_stride = p->view_per_column ? p->view_nmu : 0;
  v.mu = p->view_mu + c0 * v.mu_stride;
  v.T = p->ntv_T;
  v.out = p->ev_view_u + c0 * p->view_nmu * E;
  return v;
}

// Lean retained plans: which wavefront chunks of the eigen stage the evaluation points of a column touch.  One thread per
// column: the layer of every point exactly as the evaluation kernel finds it (rtd_eval.hip: argmax(tau <= tau_arr),
// _assemble_intensity_and_fluxes.py:185), its slot in the column's layer order lperm, slot / gpw = the chunk; the list
// sel[c][0 .. nsel) holds each touched chunk once, -1 beyond.
__global__ void rtd_chunk_select_kernel(RtdDev d, const double* tau, int ntau, int gpw, int nsel, int* sel) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d.C) return;
  int* out = sel + (long)c * nsel;
  const double* tau_arr = d.tau + (long)c * d.L;
  const int* perm = d.lperm + (long)c * d.L;
  int n = 0;
  for (int t = 0; t < ntau; ++t) {
    const double x = tau[(long)c * ntau + t];
    int l = 0;
    while (l < d.L - 1 && !(x <= tau_arr[l])) ++l;
    int slot = 0;
    while (slot < d.L - 1 && perm[slot] != l) ++slot;
    const int chunk = slot / gpw;
    bool have = false;
    for (int k = 0; k < n; ++k) have = have || out[k] == chunk;
    if (!have && n < nsel) out[n++] = chunk;
  }
  for (int k = n; k < nsel; ++k) out[k] = -1;
}

// Solve (and optionally evaluate) every window.  after_window(w, c0, cnt) is called once window w's kernels are
// queued (rtd_plan_run_fetch hangs its device-to-host copies there).
template <typename F>
int launch_windows(rtd_plan* p, bool with_solve, const RtdEval* ev, bool with_nt, F&& after_window, bool allow_fused = true) {
  (void)hipGetLastError();  // (a stale code of this thread -- another library's, an earlier failed call's -- is not this launch's)
  hipStream_t s = p->stream;
  const bool tm = p->timing;
  auto mark = [&](int k) {
    if (tm) (void)hipEventRecord(p->evt[k], s);
  };
  // two-stream window pipeline: not while the stages are being timed one by one (the HIP-event pass wants them alone)
  const bool pipe = p->pipelined && with_solve && !tm && p->nwin > 1;
  hipStream_t se = pipe ? p->eig_stream : s;
  bool nt_tables_done = false;
  // Corrections at the viewing angles (rtd_plan_set_view_nt, mode 1): this pass forms the view of u itself.  Per window, behind the
  // evaluation kernel: the interpolant of the UNCORRECTED u into the window's slice of ev_view_u; then the node corrections, as ever,
  // so that u keeps its bits; then the corrections at the angles on the slice (rtd_nt_view.hip).  A plan without corrections, an
  // evaluation that skips them or forms no u, and mode 0 queue nothing of this: the fetch interpolates the resident u, as before.
  const bool view_nt = ev && ev->u && with_nt && p->view_nt_mode == 1 && p->view_nmu > 0;
  if (ev) p->view_u_resident = false;
  if (view_nt) {
    const ResultShape r(p);
    int rc;
    if ((rc = view_basis_queued(p)) || (rc = grow(p, p->ev_view_u, r.C * p->view_nmu * r.nt * r.np)) ||
        (rc = grow(p, p->ntv_T, (int64_t)p->Cw * p->d.L * p->view_nmu)))
      return rc;
  }
  if (pipe && p->fork_needed) {  // the eigen stream starts behind the uploads queued on the plan's stream; without new inputs
    //                              it only waits, slot by slot, for the consumers of the previous run (ev_bc below), so that
    //                              back-to-back runs keep the pipeline full
    HIP_TRY(hipEventRecord(p->ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(se, p->ev_fork, 0));
    p->fork_needed = false;
  }
  // the device status words of this solve are cleared on the stream its first eigen kernel runs on.  Bits raised by an earlier
  // solve whose results were never fetched must not be reported against this one (this solve's own evaluation, queued behind the
  // clear, raises the tau bit again).
  if (with_solve) {
    if (p->status2[1]) {  // pipelined plan: the other set of status words (see rtd_plan::status2)
      p->stat_idx ^= 1;
      p->d.status = p->status2[p->stat_idx];
      p->d.col_status = p->col_status2[p->stat_idx];
      p->d.sweeps = p->sweeps2[p->stat_idx];
    }
    if (!pipe) {
      hipError_t e = clear_status(p->d, s);
      if (e != hipSuccess) return fail(RTD_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
    }  // (pipelined: inside the first eigen stage, behind its wait for the previous run)
    p->numeric_status = 0;  // a new solve starts clean
  }
  bool tables_deferred = false;
  if (with_solve && p->tables_cached && !p->tables_valid) {  // the tables of all columns, once per change of the inputs
    if (pipe) tables_deferred = true;  // launched by the first eigen stage, behind its wait: the previous run may still read them
    else launch_all_tables(p, p->d, se);
    p->tables_valid = true;
  }
  const bool per_window_tables = !p->tables_cached;
  auto eigen_stage = [&](int w) {  // tables + eigen kernel of window w into hand-off slot w & 1, on the eigen stream
    const int64_t c0 = (int64_t)w * p->Cw;
    const int cnt = (int)std::min<int64_t>(p->Cw, p->d.C - c0);
    const int slot = w & 1;
    RtdDev d = window_dev(p, c0, cnt, p->retained ? 0 : slot);
    // the slot's previous tenant has been consumed (a retained plan has a place per column, not two slots: its window w is only
    // rewritten by the NEXT run, which must not overtake this run's consumers of the same columns -- the same event says so)
    if (p->bc_recorded[slot]) (void)hipStreamWaitEvent(se, p->ev_bc[slot], 0);
    if (w == 0) (void)clear_status(p->d, se);  // (a failure here shows up as the launch error checked below)
    if (w == 0 && tables_deferred) launch_all_tables(p, p->d, se);
    if (per_window_tables) {
      rtd_launch_tables(d, se, w == 0 && !p->quad_tables_valid);
      p->quad_tables_valid = true;
    }
    rtd_launch_eig(d, se, 1);
    (void)hipEventRecord(p->ev_eig[slot], se);
  };
  if (pipe) eigen_stage(0);
  for (int w = 0; w < p->nwin; ++w) {
    const int64_t c0 = (int64_t)w * p->Cw;
    const int cnt = (int)std::min<int64_t>(p->Cw, p->d.C - c0);
    RtdDev d = window_dev(p, c0, cnt, pipe && !p->retained ? (w & 1) : 0);
    // run-path points at the layer interfaces: the boundary-condition kernel evaluates the Fourier modes there itself
    // (rtd_plan_evaluate -- the closures -- always takes the evaluation kernel, whatever the window count: a column's
    // closure values must not depend on the batch it was solved in)
    const bool fused = allow_fused && with_solve && ev && ev->antider == 0 && ev->deriv == 0 && p->ev_iface && p->um_buf && rtd_bc_fuses_eval(d);
    d.um = fused ? p->um_buf.p : nullptr;
    if (tm) {
      (void)hipStreamSynchronize(s);
      harvest(p);
    }
    if (pipe) {
      if (w + 1 < p->nwin) eigen_stage(w + 1);  // queued before this window's boundary-condition kernel: they run side by side
      (void)hipStreamWaitEvent(s, p->ev_eig[w & 1], 0);
      rtd_launch_bc(d, s, 0);
      rtd_launch_bc(d, s, 1);
    } else if (with_solve) {
      mark(0);
      if (per_window_tables) {
        rtd_launch_tables(d, s, w == 0 && !p->quad_tables_valid);
        p->quad_tables_valid = true;
      }
      for (int part = 0; part < 3; ++part) {
        mark(1 + part);
        rtd_launch_eig(d, s, part);
      }
      for (int part = 0; part < 2; ++part) {
        mark(4 + part);
        rtd_launch_bc(d, s, part);
      }
    }
    if (!with_solve && ev && p->lean && p->nwin > 1) {
      // Lean retained plan, evaluation only: Y, A of this window's columns are not resident -- the eigen stage is run again for
      // the wavefront chunks the evaluation points touch (every chunk when the points touch most of them, or for the
      // one-lane-per-problem kernel of 2 ... 8 streams, whose wavefronts span columns), into hand-off slot 0; k, E, B and the
      // thermal vectors are rewritten in their retained places with the bits they had; the coefficients are kept: no
      // boundary-condition solve.  Everything queued on the plan's stream: the solve's eigen stream is behind ev_eig already.
      if (p->tables_cached && !p->tables_valid) launch_all_tables(p, p->d, s);  // (rtd_plan_invalidate_tables since the solve)
      RtdDev dsel = d;
      const int gpw = 64 / d.NP, nchunk = (d.L + gpw - 1) / gpw;
      const int nsel = d.NP == 4 || 2 * ev->ntau >= nchunk ? 0 : ev->ntau;
      if (nsel > 0) {
        int rc = grow(p, p->sel_buf, ((int64_t)p->Cw * nsel + 1) / 2 + 1);
        if (rc) return rc;
        int* sel = reinterpret_cast<int*>(p->sel_buf.p);
        hipLaunchKernelGGL(rtd_chunk_select_kernel, grid_1d(cnt, 128), dim3(128), 0, s, d, ev->tau + c0 * ev->ntau, ev->ntau, gpw, nsel, sel);
        dsel.chunk_sel = sel;
        dsel.nsel = nsel;
      }
      rtd_launch_eig(dsel, s, 1);
    }
    mark(6);
    if (ev) {
      // (a gather of the previous run's results may still be in flight: it reads its own snapshot, not these buffers)
      RtdEval e = window_eval(p, *ev, c0);
      e.um_in = fused ? p->um_buf.p : nullptr;
      rtd_launch_eval(d, e, s);
      const int64_t Eu = (int64_t)e.ntau * e.nphi;
      if (view_nt) {
        int rc = view_apply_queued(p, e.u, Eu, c0, cnt, p->ev_view_u);
        if (rc) return rc;
      }
      if (with_nt && e.u != nullptr) {
        const RtdNt nt = window_nt(p, c0);
        if (!p->nt_tables_ready) {
          rtd_launch_nt_tables(d, nt, s);
          nt_tables_done = true;
        }
        rtd_launch_nt_apply(d, nt, e, s);
        if (view_nt) {
          const RtdNtView v = window_nt_view(p, c0, Eu);
          rtd_launch_nt_view_tables(d, v, e.antider, s);
          rtd_launch_nt_view_apply(d, nt, e, v, s);
        }
      }
      mark(7);
    }
    if (pipe) {  // slot w & 1 may be filled again
      (void)hipEventRecord(p->ev_bc[w & 1], s);
      p->bc_recorded[w & 1] = true;
    }
    if (tm) {
      for (int k = 0; k < 6; ++k) p->pending[k] = with_solve;
      p->pending[6] = ev != nullptr;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RTD_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    int rc = after_window(w, c0, cnt);
    if (rc) return rc;
  }
  if (nt_tables_done) p->nt_tables_ready = true;  // every window's tables were made in this pass
  if (ev) {
    p->res_nt = with_nt && ev->u != nullptr;
    p->view_u_resident = view_nt;
  }
  if (with_solve) p->solved = true;
  if (with_solve && !pipe) p->fork_needed = true;  // slot 0 was filled on the plan's own stream
  return 0;
}

int launch_solve(rtd_plan* p, bool with_eval, const RtdEval* ev, bool with_nt = false) {
  return launch_windows(p, true, with_eval ? ev : nullptr, with_nt, [](int, int64_t, int) { return 0; });
}

// read and clear the device status word after the stream has drained; maps it to an error code.  all_modes = false: the
// caller's outputs come from Fourier mode 0 alone (fluxes, u0): a failure confined to the modes m > 0 is not theirs -- the
// reference returns them unharmed then (and NaN for u; here u reports the failure).
int check_status(rtd_plan* p, const bool all_modes = true) {
  int st = 0;
  HIP_TRY(hipMemcpyAsync(&st, p->d.status, sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  p->stream_drained();
  if (st != 0) {
    HIP_TRY(hipMemsetAsync(p->d.status, 0, sizeof(int), p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
  }
  p->numeric_status |= st & ~RTD_ST_TAU;  // a failed solve stays failed for every later evaluation of it
  if (st & RTD_ST_TAU) return fail(RTD_ERR_TAU_RANGE, "tau input outside the tau range specified for the atmosphere");
  const int low = p->numeric_status & 0xFF, high = (p->numeric_status >> RTD_ST_HIGH_MODE_SHIFT) & 0xFF;
  st = low | (all_modes ? high : 0);
  if (st == 0) return 0;
  std::string what;
  if (st & RTD_ST_CHOL) what += " non-positive Cholesky pivot or non-finite eigenvalue (phase function not positive definite?);";
  if (st & RTD_ST_JACOBI) what += " Jacobi eigen-iteration did not converge;";
  if (st & RTD_ST_BEAM) what += " non-finite beam particular solution (1/mu0 coincides with an eigenvalue?);";
  if (st & RTD_ST_BC) what += " singular boundary-condition system (non-finite coefficients);";
  if (low == 0) what += " in Fourier modes m > 0 only: the fluxes and u0 of this solve are valid";
  {  // which columns (rtd_plan_get_column_status has the bits of every column)
    std::vector<int> cs((size_t)p->d.C);
    if (hipMemcpy(cs.data(), p->d.col_status, cs.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) {
      int64_t n = 0;
      std::string first;
      for (size_t c = 0; c < cs.size(); ++c)
        if (cs[c] & (all_modes ? 0xFFFF : 0xFF)) {
          if (n < 8) first += (n ? ", " : "") + std::to_string(c);
          ++n;
        }
      if (n > 0 && !what.empty() && what.back() == ';') what.pop_back();
      if (n > 0) what += "; " + std::to_string(n) + " of " + std::to_string(cs.size()) + " columns (" + first + (n > 8 ? ", ..." : "") + ")";
    }
  }
  return fail(RTD_ERR_NUMERIC, "numerical failure on the device:" + what);
}

}  // namespace

extern "C" {

int rtd_comm_destroy(rtd_plan* p);

int rtd_version(void) { return 219; }  // 210: rtd_plan_create_retained, rtd_plan_retained, rtd_comm_size; 211: rtd_pool_trim, rtd_pool_bytes (round 5); 212: rtd_pool_set_limit (large-block pool off by default), rtd_comm_transport (round 6); 213: rtd_band_mix, rtd_plan_set_columns_band, rtd_plan_set_band_weights, rtd_plan_fetch_band, rtd_plan_evaluate_band; 214: rtd_plan_fetch_actinic, rtd_plan_fetch_band_actinic; 215: rtd_plan_request_nt, rtd_plan_get_nt; 216: rtd_plan_set_view_mu, rtd_plan_fetch_view, rtd_plan_fetch_band_view, bit 3 of the evaluation flag word; 217: rtd_plan_request_surface, rtd_surface_samples, rtd_plan_get_bdrf; 218: rtd_plan_set_view_nt; 219: rtd_plan_couple_lambert, rtd_plan_couple_lambert_band, rtd_lambert_kappa

const char* rtd_last_error(void) { return g_err.c_str(); }

int rtd_device_count(int32_t* count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(RTD_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = n;
  return 0;
}

static int plan_build(rtd_plan* p, const rtd_dims* dims, int32_t device, int32_t work_columns, int64_t retain_bytes, int32_t form) {
  const int N = dims->nquad / 2;
  p->dims = *dims;
  p->device = device;
  p->NP = pad_pow2(N);
  int rc;
  if ((rc = acquire_stream(device, &p->stream))) return rc;
  RtdDev& d = p->d;
  const int64_t C = dims->ncols, L = dims->nlayers, M = dims->nfourier, P = dims->nleg, NP = p->NP,
                Ns = dims->nscoeffs, NB = dims->nbdrf, Q2 = 2 * NP;
  d.C = (int)C; d.L = (int)L; d.N = N; d.NP = (int)NP; d.P = (int)P; d.M = (int)M; d.Ns = (int)Ns;
  d.NBDRF = (int)NB; d.beam = dims->beam ? 1 : 0;
  // RTD_BC_FORCE_PIVOT=1: every speculative elimination of the fused kernels is redone by the LDS pivoted path (bit 0);
  // =2: every chain takes the register-resident pivoted elimination of rtd_bc_mfma_kernel throughout (bit 2)
  const char* fp = getenv("RTD_BC_FORCE_PIVOT");
  d.flags = (fp ? (atoi(fp) == 2 ? 4 : 1) : 0) | (getenv("RTD_BC_FORCE_HANDOVER") ? 2 : 0);
  d.m0 = 0; d.mstep = 1; d.mtot = (int)M;
  d.l0 = 0; d.ln = (int)L;
  // window of columns whose intermediates are resident: bytes of intermediates per column.  A plan of more than one window
  // that pipelines them holds the eigen stage's hand-off buffers twice; a one-window (or RTD_NO_PIPELINE) plan once.
  const int64_t handoff_col = 8 * (M * P + (L + 1) + 2 * M * L * NP * NP + 2 * M * L * NP + M * L * Q2 + L * Ns * Q2 + L * NP + (Ns > 0 ? 4 * L * NP : 0));
  const int64_t rest_col = 8 * (M * L * Q2 + M * (L - 1) * Q2 * Q2);
  const bool may_pipeline = !getenv("RTD_NO_PIPELINE");
  const int64_t per_col_one = handoff_col + rest_col, per_col_win = (may_pipeline ? 2 : 1) * handoff_col + rest_col;
  const char* env = getenv("RTD_WORK_BYTES");
  const double budget = env ? atof(env) : 24.0 * (double)(1ull << 30);
  auto fit_window = [&](double bytes) {  // columns per window of a multi-window plan within `bytes`
    int64_t fit = (int64_t)(bytes / (double)per_col_win);
    if (fit < 1) fit = 1;
    if (fit > 256) fit -= fit % 256;
    return fit;
  };
  int64_t Cw = C;
  if (work_columns > 0) {
    // The caller's window is honoured while it fits: RTD_WORK_BYTES when set, else 80 % of the device memory that is free
    // now (the 24 GiB default is the automatic path's choice, not a limit on an explicit request).  hipMemGetInfo is only
    // asked when the request is large: one-column plans are created per pydisort() call.
    Cw = std::min<int64_t>(C, work_columns);
    const double want = (double)Cw * (double)(Cw < C ? per_col_win : per_col_one);
    if (env ? want > budget : want > 4.0 * (double)(1ull << 30)) {
      double cap = budget;
      if (!env) {
        size_t free_b = 0, total_b = 0;
        if ((rc = device_memory(device, &free_b, &total_b))) return rc;
        cap = 0.8 * (double)free_b;
      }
      if (want > cap) Cw = std::min<int64_t>(Cw, fit_window(cap));
    }
  } else if ((double)C * (double)per_col_one > budget) {  // (a batch that fits one window pays for one hand-off slot only)
    Cw = std::min<int64_t>(C, fit_window(budget));
  }
  p->Cw = (int)Cw;
  p->nwin = (int)((C + Cw - 1) / Cw);
  p->pipelined = p->nwin > 1 && may_pipeline;
  // Retained evaluator state (rtd_plan_create_retained): everything but the boundary-condition workspace for ALL columns, when
  // that fits the caller's budget (< 0: three tenths of the device memory that is free now)
  // that fits the caller's budget; else (or when the caller asks for it: form 2) the LEAN form: the same without Y, A -- what an
  // evaluation can recompute from the inputs without solving the boundary-condition system again (see rtd_plan::lean)
  const int64_t retain_col = handoff_col + 8 * (M * L * Q2);  // + coef
  const int64_t lean_col = retain_col - 8 * (2 * M * L * NP * NP);
  if (p->nwin > 1 && retain_bytes != 0) {
    double cap = (double)retain_bytes;
    if (retain_bytes < 0) {
      size_t free_b = 0, total_b = 0;
      if ((rc = device_memory(device, &free_b, &total_b))) return rc;
      cap = 0.3 * (double)free_b;
    }
    p->retained = form != 2 && (double)C * (double)retain_col <= cap;
    // (not below 10 streams: the one-lane-per-problem eigen kernel's wavefronts span columns, and its matrices are 128 bytes)
    p->lean = !p->retained && form != 1 && NP > 4 && (double)C * (double)lean_col <= cap;
  }
  const int64_t Ch = p->retained || p->lean ? C : Cw;  // columns the coefficients, k, E, B and the thermal vectors cover
  const int64_t Cy = p->retained ? C : Cw;             // columns Y, A cover
  rtd_plan::HandOff& h1 = p->slot1;
  // one arena for every fixed-size buffer (a single hipMalloc keeps plan creation cheap for one-column calls):
  // pass 0 sizes it, pass 1 carves it
  char* arena = nullptr;
  int64_t off = 0;
  for (int pass = 0; pass < 2; ++pass) {
    off = 0;
    auto carve = [&](auto** ptr, int64_t n) {
      using E = std::remove_pointer_t<std::remove_pointer_t<decltype(ptr)>>;
      if (n <= 0) n = 1;
      const int64_t bytes = (n * (int64_t)sizeof(E) + 255) / 256 * 256;
      if (pass == 1) *ptr = reinterpret_cast<E*>(arena + off);
      off += bytes;
    };
#define A(ptr, n) carve(&ptr, (n));
    A(d.mu, NP) A(d.w, NP) A(d.invmu, NP) A(d.S, NP) A(d.T, NP)
    A(d.Y, M * P * NP)
    // inputs: all C columns
    A(d.lperm, C * L) A(d.omega, C * L) A(d.tau, C * L) A(d.taus0, C * (L + 1)) A(d.scale, C * L) A(d.wleg, C * L * P)
    A(d.mu0, C) A(d.I0, C) A(d.phi0, C) A(d.rescale, C) A(d.col_status, C)
    A(d.bpos, C * M * NP) A(d.bneg, C * M * NP) A(d.spoly, C * L * Ns) A(d.bdrfq, C * NB * NP * NP) A(d.bdrfq0, C * NB * NP)
    // intermediates: one window of Cw columns
    A(d.Y0, Ch * M * P) A(d.att, Ch * (L + 1))
    A(d.Ym, Cy * M * L * NP * NP) A(d.Am, Cy * M * L * NP * NP) A(d.kk, Ch * M * L * NP) A(d.Bv, Ch * M * L * Q2)
    A(d.dq, Ch * L * Ns * Q2) A(d.zneg, Ch * L * NP) A(d.vb, Ns > 0 ? Ch * L * 4 * NP : 1) A(d.coef, Ch * M * L * Q2)
    A(d.Fws, Cw * M * (L - 1) * Q2 * Q2) A(d.Ek, Ch * M * L * NP) A(d.need_split, Cw * M)
    A(d.sweeps, 1) A(d.status, 1) A(d.split_any, 1)
    if (p->pipelined && !p->retained) {
      A(h1.Ym, Cw * M * L * NP * NP) A(h1.Am, Cw * M * L * NP * NP)
      if (!p->lean) {  // (a lean plan keeps these per column: window_dev)
        A(h1.Y0, Cw * M * P) A(h1.att, Cw * (L + 1))
        A(h1.kk, Cw * M * L * NP) A(h1.Bv, Cw * M * L * Q2) A(h1.dq, Cw * L * Ns * Q2) A(h1.zneg, Cw * L * NP) A(h1.vb, Ns > 0 ? Cw * L * 4 * NP : 1) A(h1.Ek, Cw * M * L * NP)
      }
    }
    if (p->pipelined) {
      A(p->status2[1], 1) A(p->col_status2[1], C) A(p->sweeps2[1], 1)
    }
#undef A
    if (pass == 0 && (rc = p->alloc(&arena, off))) return rc;
  }
  if (p->nwin == 1 || p->retained || p->lean) {
    p->Y0_all = d.Y0;
    p->att_all = d.att;
    p->tables_cached = true;
  } else if ((double)C * (double)(M * P + L + 1) * 8.0 <= 2.0 * (double)(1ull << 30)) {
    if ((rc = p->alloc(&p->Y0_all, C * M * P))) return rc;
    if ((rc = p->alloc(&p->att_all, C * (L + 1)))) return rc;
    p->tables_cached = true;
  }
  // (d.sweeps, d.status, d.split_any and d.Bv, d.dq were carved next to each other: one fill each -- a fill costs ~8 us of host
  //  time, which a one-column pydisort() call notices)
  HIP_TRY(hipMemsetAsync(d.sweeps, 0, (size_t)(reinterpret_cast<char*>(d.split_any) - reinterpret_cast<char*>(d.sweeps)) + sizeof(int), p->stream));
  HIP_TRY(hipMemsetAsync(d.col_status, 0, sizeof(int) * (size_t)C, p->stream));
  if (p->pipelined) {
    p->status2[0] = d.status; p->col_status2[0] = d.col_status; p->sweeps2[0] = d.sweeps;
    HIP_TRY(hipMemsetAsync(p->status2[1], 0, sizeof(int), p->stream));
    HIP_TRY(hipMemsetAsync(p->col_status2[1], 0, sizeof(int) * (size_t)C, p->stream));
    HIP_TRY(hipMemsetAsync(p->sweeps2[1], 0, sizeof(int), p->stream));
  }
  HIP_TRY(hipMemsetAsync(d.Bv, 0, (size_t)(reinterpret_cast<char*>(d.dq) - reinterpret_cast<char*>(d.Bv)) + (Ns > 0 ? (size_t)(Ch * L * Ns * Q2) * 8 : 0), p->stream));
  if (p->pipelined) {
    if (!p->retained && !p->lean) {
      HIP_TRY(hipMemsetAsync(h1.Bv, 0, (size_t)(Cw * M * L * Q2) * 8, p->stream));
      if (Ns > 0) HIP_TRY(hipMemsetAsync(h1.dq, 0, (size_t)(Cw * L * Ns * Q2) * 8, p->stream));
    }
    // (stream priorities either way changed nothing: profiles/archive/r03_experiments.json)
    if ((rc = acquire_stream(device, &p->eig_stream))) return rc;
    for (hipEvent_t* e : {&p->ev_eig[0], &p->ev_eig[1], &p->ev_bc[0], &p->ev_bc[1], &p->ev_fork})
      if ((rc = ensure_event(e))) return rc;
  }
  // (no synchronisation here: the fills are stream-ordered before everything the plan does later, and waiting for them costs a
  //  one-column call ~15 us; a failed fill surfaces at the next synchronising call)
  return 0;
}

int rtd_plan_create_retained(const rtd_dims* dims, int32_t device, int32_t work_columns, int64_t retain_bytes, rtd_plan** out) {
  return rtd_plan_create_retained_form(dims, device, work_columns, retain_bytes, 0, out);
}

int rtd_plan_create_retained_form(const rtd_dims* dims, int32_t device, int32_t work_columns, int64_t retain_bytes, int32_t form,
                                  rtd_plan** out) {
  if (!dims || !out) return fail(RTD_ERR_ARG, "null argument");
  *out = nullptr;
  if (form < 0 || form > 2) return fail(RTD_ERR_ARG, "retained form: 0 (full, else lean), 1 (full only) or 2 (lean)");
  const int N = dims->nquad / 2;
  if (dims->ncols < 1 || dims->nlayers < 1 || dims->nquad < 2 || (dims->nquad & 1) || dims->nleg < 1 ||
      dims->nfourier < 1 || dims->nfourier > dims->nleg || dims->nscoeffs < 0 || dims->nbdrf < 0)
    return fail(RTD_ERR_ARG, "invalid dimensions");
  // include/rtd.h: nleg <= nquad (pydisort.py:232-234 of the reference).  The one-lane-per-problem eigen kernel of 2 ... 8 streams
  // reads exactly 2 NP moments per parity: more would be dropped silently.
  if (dims->nleg > dims->nquad) return fail(RTD_ERR_ARG, "invalid dimensions: nleg > nquad");
  // 2 ... 64 streams; 66 ... 128 streams: one eigenproblem per wavefront, one boundary-condition chain per workgroup (rtd_bc_wide.hip)
  if (N > 64) return fail(RTD_ERR_ARG, "NQuad > 128 is not supported by this build (N = NQuad/2 <= 64)");
  HIP_TRY(hipSetDevice(device));
  rtd_plan* p = new rtd_plan();
  const int rc = plan_build(p, dims, device, work_columns, retain_bytes, form);
  if (rc) return destroy_keeping_error(p, rc);
  *out = p;
  return 0;
}

int rtd_plan_create_windowed(const rtd_dims* dims, int32_t device, int32_t work_columns, rtd_plan** out) {
  return rtd_plan_create_retained(dims, device, work_columns, 0, out);
}

int rtd_plan_retained(rtd_plan* p, int32_t* retained) {
  if (!p || !retained) return fail(RTD_ERR_ARG, "null argument");
  *retained = p->nwin == 1 || p->retained ? 1 : p->lean ? 2 : 0;
  return 0;
}

int rtd_plan_create(const rtd_dims* dims, int32_t device, rtd_plan** out) {
  return rtd_plan_create_windowed(dims, device, 0, out);
}

int rtd_plan_windows(rtd_plan* p, int32_t* work_columns, int32_t* nwindows) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (work_columns) *work_columns = p->Cw;
  if (nwindows) *nwindows = p->nwin;
  return 0;
}

int rtd_plan_destroy(rtd_plan* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->comm_stream) (void)hipStreamSynchronize(p->comm_stream);
  if (p->copy_stream) (void)hipStreamSynchronize(p->copy_stream);
  if (p->eig_stream) (void)hipStreamSynchronize(p->eig_stream);
  rtd_comm_destroy(p);
  for (size_t i = 0; i < p->allocs.size(); ++i)
    if (p->allocs[i]) pooled_free(p->allocs[i], p->alloc_bytes[i], p->device);
  for (hipEvent_t e : p->evt)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : {p->ev_results, p->ev_gathered, p->ev_win[0], p->ev_win[1], p->ev_copied[0], p->ev_copied[1], p->ev_eig[0],
                       p->ev_eig[1], p->ev_bc[0], p->ev_bc[1], p->ev_fork})
    if (e) (void)hipEventDestroy(e);
  // (every stream was drained above: the streams and the pinned slabs can serve another plan at once)
  if (p->eig_stream) pool().put_stream(p->eig_stream, p->device);
  for (int k = 0; k < 2; ++k)
    if (p->stage[k] && !pool().put_host(p->stage[k], p->stage_cap[k])) (void)hipHostFree(p->stage[k]);
  if (p->comm_stream) (void)hipStreamDestroy(p->comm_stream);
  if (p->copy_stream) pool().put_stream(p->copy_stream, p->device);
  if (p->stream) pool().put_stream(p->stream, p->device);
  delete p;
  return 0;
}

int rtd_plan_synchronize(rtd_plan* p) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  HIP_TRY(hipStreamSynchronize(p->stream));
  p->stream_drained();
  if (p->eig_stream) HIP_TRY(hipStreamSynchronize(p->eig_stream));  // (every eigen stage is consumed on `stream`: a formality)
  if (p->comm_stream) HIP_TRY(hipStreamSynchronize(p->comm_stream));
  return 0;
}

int rtd_plan_get_column_status(rtd_plan* p, int32_t* status) {
  if (!p || !status) return fail(RTD_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (p->eig_stream) HIP_TRY(hipStreamSynchronize(p->eig_stream));
  HIP_TRY(hipMemcpy(status, p->d.col_status, sizeof(int32_t) * (size_t)p->d.C, hipMemcpyDeviceToHost));
  return 0;
}

int rtd_plan_device_bytes(rtd_plan* p, int64_t* bytes) {
  if (!p || !bytes) return fail(RTD_ERR_ARG, "null argument");
  *bytes = p->bytes;
  return 0;
}

int rtd_pool_trim(int32_t device, int64_t* released) {
  const size_t n = pool().trim(device);
  if (released) *released = (int64_t)n;
  return 0;
}

int rtd_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes) {
  size_t fr = 0, total = 0;
  if (int rc = device_memory(device, &fr, &total)) return rc;
  if (free_bytes) *free_bytes = (int64_t)fr;
  if (total_bytes) *total_bytes = (int64_t)total;
  return 0;
}

int rtd_pool_set_limit(int64_t bytes, int32_t device, int64_t* previous) {
  const int64_t prev = pool().set_limit(bytes, device);
  if (previous) *previous = prev;
  return 0;
}

int rtd_pool_bytes(int64_t* cached) {
  if (!cached) return fail(RTD_ERR_ARG, "null argument");
  DevPool& q = pool();
  std::lock_guard<std::mutex> g(q.m);
  *cached = (int64_t)(q.cached + q.big_cached);
  return 0;
}

int rtd_plan_set_quadrature(rtd_plan* p, const double* mu_pos, const double* weights) {
  if (!p || !mu_pos || !weights) return fail(RTD_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(p->device));
  const int N = p->d.N, NP = p->NP;
  std::vector<double> mu(NP), w(NP), im(NP), S(NP), T(NP);
  for (int i = 0; i < NP; ++i) {
    if (i < N) {
      if (!(mu_pos[i] > 0.0) || !(weights[i] > 0.0)) return fail(RTD_ERR_ARG, "quadrature nodes/weights must be positive");
      mu[i] = mu_pos[i]; w[i] = weights[i];
      S[i] = std::sqrt(w[i] / mu[i]); T[i] = std::sqrt(w[i] * mu[i]);
    } else {  // padding stream: decoupled, never the beam direction (1/mu = 0.5 < 1/mu0)
      mu[i] = 2.0; w[i] = 0.0; S[i] = 0.0; T[i] = 1.0;
    }
    im[i] = 1.0 / mu[i];
  }
  // mu, w, 1/mu, S, T were carved one after the other (plan_build): ONE copy of a host image of that stretch instead of five
  // (a small copy from pageable memory costs ~5 us of host time: it matters to a one-column pydisort() call)
  const size_t nb = (size_t)NP * 8;
  const char* base = reinterpret_cast<const char*>(p->d.mu);
  const size_t span = (size_t)(reinterpret_cast<const char*>(p->d.T) - base) + nb;
  if (p->quad_pending) HIP_TRY(hipStreamSynchronize(p->stream));  // (an earlier upload may still read the image)
  std::vector<char>& img = p->quad_img;
  img.assign(span, 0);
  const struct { const double* dev; const std::vector<double>* host; } rows[5] = {{p->d.mu, &mu}, {p->d.w, &w}, {p->d.invmu, &im}, {p->d.S, &S}, {p->d.T, &T}};
  for (const auto& row : rows) std::memcpy(img.data() + (reinterpret_cast<const char*>(row.dev) - base), row.host->data(), nb);
  HIP_TRY(hipMemcpyAsync((void*)p->d.mu, img.data(), span, hipMemcpyHostToDevice, p->stream));
  p->quad_pending = true;  // (no wait: the image stays with the plan)
  p->h_mu_pos.assign(mu_pos, mu_pos + N);  // (the barycentric weights of rtd_plan_fetch_view are formed from these, on the host)
  p->view_stale = true;
  p->new_quadrature();
  return 0;
}

namespace {
// Per-stream arrays from N to the NP streams of the kernels, zero beyond N (src null: all zero).  square = false: `blocks` rows
// [N] -> [NP] (b_pos, b_neg, bdrf_q0); square = true: `blocks` tables [N][N] -> [NP][NP] (bdrf_q).
extern "C++" std::vector<double> pad_streams(const double* src, int64_t blocks, bool square, int64_t N, int64_t NP) {
  const int64_t rows = square ? N : 1, rows_out = square ? NP : 1;
  std::vector<double> out((size_t)(blocks * rows_out * NP), 0.0);
  if (src)
    for (int64_t b = 0; b < blocks; ++b)
      for (int64_t i = 0; i < rows; ++i)
        for (int64_t j = 0; j < N; ++j) out[(size_t)((b * rows_out + i) * NP + j)] = src[(b * rows + i) * N + j];
  return out;
}

// The argument checks shared by the prepared and the raw uploads (two parts: each upload has checks of its own between them)
int refuse_missing_sources(const RtdDev& d, bool spoly_needed, const double* s_poly, const double* bdrf_q, const double* bdrf_q0,
                           bool surface_requested = false) {
  if (spoly_needed && !s_poly) return fail(RTD_ERR_ARG, "s_poly is required when nscoeffs > 0");
  if (surface_requested) {  // (rtd_plan_request_surface: the tables are formed on the device)
    if (bdrf_q || bdrf_q0) return fail(RTD_ERR_ARG, "rtd_plan_request_surface is set: bdrf_q and bdrf_q0 must be NULL");
    return 0;
  }
  if (d.NBDRF > 0 && (!bdrf_q || !bdrf_q0)) return fail(RTD_ERR_ARG, "BDRF tables are required when nbdrf > 0");
  return 0;
}
int refuse_beam(const RtdDev& d, const double* I0) {
  if (!d.beam)  // a plan created without a beam skips the beam terms on the device
    for (int64_t c = 0; c < d.C; ++c)
      if (I0[c] > 0.0) return fail(RTD_ERR_ARG, "the plan was created with beam = 0 but a column has I0 > 0");
  return 0;
}

// The buffers of the Nakajima-Tanaka inputs (wfull: `rows` rows -- one per column, or per profile of a band) and tables, reused or
// grown on repeated calls, and the plan's view of them once the inputs are in place.
int nt_buffers(rtd_plan* p, int64_t rows, int64_t nleg_all) {
  const int64_t C = p->d.C, L = p->d.L;
  int rc;
  if ((rc = grow(p, p->nt_w, rows * L * nleg_all)) || (rc = grow(p, p->nt_f, C * L)) || (rc = grow(p, p->nt_ic, C * nleg_all)) ||
      (rc = grow(p, p->nt_ip, C * 2)) || (rc = grow(p, p->nt_R, C * 4 * p->d.NP * L)))
    return rc;
  return 0;
}
void nt_bind(rtd_plan* p, int nleg_all, int group, int64_t rows) {
  p->nt.nleg_all = nleg_all; p->nt.group = group; p->nt.c0 = 0;
  p->nt.wfull = p->nt_w; p->nt.f = p->nt_f; p->nt.ims_coef = p->nt_ic; p->nt.ims_par = p->nt_ip; p->nt.R = p->nt_R;
  p->nt_rows = rows;
  p->have_nt = true;
}

// rtd_plan_set_columns (s_local = false: s_poly in the absolute scaled depth) and rtd_plan_set_columns_local (true: already about
// the top of each layer, as rtd_source_polynomials_local leaves them)
int set_columns_impl(rtd_plan* p, const double* scaled_omega, const double* tau, const double* taus0,
                     const double* scale_tau, const double* wleg, const double* mu0, const double* I0,
                     const double* phi0, const double* rescale, const double* b_pos, const double* b_neg,
                     const double* s_poly, const double* bdrf_q, const double* bdrf_q0, const bool s_local) {
  if (!p || !scaled_omega || !tau || !taus0 || !scale_tau || !wleg || !mu0 || !I0 || !phi0 || !rescale)
    return fail(RTD_ERR_ARG, "null argument");
  const RtdDev& d = p->d;
  if (p->surf_model >= 0)
    return fail(RTD_ERR_STATE, "rtd_plan_request_surface is set: the BDRF modes are formed by the raw uploads (set_columns_raw / _thermal / _band)");
  if (int rc = refuse_missing_sources(d, d.Ns > 0, s_poly, bdrf_q, bdrf_q0)) return rc;
  if (p->nt_request > 0)
    return fail(RTD_ERR_STATE, "rtd_plan_request_nt is set: the Nakajima-Tanaka inputs are formed from raw columns (set_columns_raw / _thermal / _band)");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t C = d.C, L = d.L, M = d.M, P = d.P, N = d.N, NP = d.NP, Ns = d.Ns, NB = d.NBDRF;
  if (int rc = refuse_beam(d, I0)) return rc;
  hipStream_t s = p->stream;
  // The per-column inputs were carved one after the other, lperm first and the BDRF tables last (plan_build).  A small plan -- a
  // one-column pydisort() call above all -- gets ONE copy of a host image of that stretch instead of fifteen small ones (~5 us of
  // host time each from pageable memory); d.col_status lies inside the stretch and is cleared by every solve anyway.
  const char* in_base = reinterpret_cast<const char*>(d.lperm);
  const size_t in_span = (size_t)(reinterpret_cast<const char*>(d.bdrfq0) - in_base) + (size_t)std::max<int64_t>(C * NB * NP, 1) * 8;
  const bool one_copy = in_span <= (size_t)(1u << 20);
  if (one_copy && p->cols_pending) HIP_TRY(hipStreamSynchronize(s));  // (an earlier upload may still read the image)
  std::vector<char>& img = p->cols_img;
  if (one_copy) img.assign(in_span, 0);
#define UP(dst, src, n)                                                                                              \
  do {                                                                                                                \
    if (one_copy) std::memcpy(img.data() + (reinterpret_cast<const char*>(dst) - in_base), (src), (size_t)(n) * 8);   \
    else HIP_TRY(hipMemcpyAsync((void*)(dst), (src), (size_t)(n) * 8, hipMemcpyHostToDevice, s));                    \
  } while (0)
  UP(d.omega, scaled_omega, C * L);
  // Layer order of the eigen stage: a wavefront iterates until the slowest of its 64/NP eigenproblems has converged,
  // and the Jacobi sweep count grows with omega* / (1 - g*) (g* = the first scaled moment).  Sorting each column's layers
  // by that key before they are dealt to wavefronts brings the mean of the per-wavefront maximum from 3.1 to 2.8
  // sweeps on the benchmark columns (2.73 is the mean per problem).  Results do not depend on the order.
  std::vector<int> perm((size_t)(C * L));
  {
    std::vector<std::pair<double, int>> key((size_t)L);
    for (int64_t c = 0; c < C; ++c) {
      for (int64_t l = 0; l < L; ++l) {
        const double g = P > 1 ? wleg[(c * L + l) * P + 1] / 3.0 : 0.0;
        key[(size_t)l] = {scaled_omega[c * L + l] / std::max(1.0 - g, 1e-6), (int)l};
      }
      std::sort(key.begin(), key.end());
      for (int64_t l = 0; l < L; ++l) perm[(size_t)(c * L + l)] = key[(size_t)l].second;
    }
  }
  if (one_copy) std::memcpy(img.data(), perm.data(), perm.size() * sizeof(int));
  else HIP_TRY(hipMemcpyAsync((void*)d.lperm, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice, s));
  UP(d.tau, tau, C * L);
  UP(d.taus0, taus0, C * (L + 1));
  UP(d.scale, scale_tau, C * L);
  UP(d.wleg, wleg, C * L * P);
  UP(d.mu0, mu0, C);
  UP(d.I0, I0, C);
  UP(d.phi0, phi0, C);
  UP(d.rescale, rescale, C);
  // The thermal source polynomials arrive as the reference's scaled_s_poly_coeffs: coefficients in the ABSOLUTE scaled optical
  // depth.  The kernels keep them about the top of their own layer (rtd_dd.h): Taylor shift by taus0[l], in double-double.
  std::vector<double> sloc;
  if (Ns > 0 && s_local) {
    UP(d.spoly, s_poly, C * L * Ns);
  } else if (Ns > 0) {
    sloc.resize((size_t)(C * L * Ns));
    for (int64_t cl = 0; cl < C * L; ++cl)
      rtd_taylor_shift_to(s_poly + cl * Ns, sloc.data() + cl * Ns, (int)Ns, taus0[cl / L * (L + 1) + cl % L]);
    UP(d.spoly, sloc.data(), C * L * Ns);
  }
  // pad the per-stream arrays from N to NP
  std::vector<double> bp, bn;
  if (N != NP) {
    b_pos = (bp = pad_streams(b_pos, C * M, false, N, NP)).data();
    b_neg = (bn = pad_streams(b_neg, C * M, false, N, NP)).data();
  }
  if (b_pos) UP(d.bpos, b_pos, C * M * NP);
  else if (!one_copy) HIP_TRY(hipMemsetAsync((void*)d.bpos, 0, (size_t)(C * M * NP) * 8, s));  // (the image is zero there)
  if (b_neg) UP(d.bneg, b_neg, C * M * NP);
  else if (!one_copy) HIP_TRY(hipMemsetAsync((void*)d.bneg, 0, (size_t)(C * M * NP) * 8, s));
  std::vector<double> q, q0;
  if (NB > 0) {
    q = pad_streams(bdrf_q, C * NB, true, N, NP);
    q0 = pad_streams(bdrf_q0, C * NB, false, N, NP);
    UP(d.bdrfq, q.data(), C * NB * NP * NP);
    UP(d.bdrfq0, q0.data(), C * NB * NP);
  }
#undef UP
  if (one_copy) {
    HIP_TRY(hipMemcpyAsync((void*)d.lperm, img.data(), in_span, hipMemcpyHostToDevice, s));
    p->cols_pending = true;  // (no wait: the image stays with the plan; the caller's arrays have been copied into it)
  } else {
    HIP_TRY(hipStreamSynchronize(s));  // the caller's arrays and the host staging vectors must outlive their copies
  }
  p->h_tau.assign(tau, tau + C * L);
  p->new_columns(false);
  return 0;
}
}  // namespace

int rtd_plan_set_columns(rtd_plan* p, const double* scaled_omega, const double* tau, const double* taus0,
                         const double* scale_tau, const double* wleg, const double* mu0, const double* I0,
                         const double* phi0, const double* rescale, const double* b_pos, const double* b_neg,
                         const double* s_poly, const double* bdrf_q, const double* bdrf_q0) {
  return set_columns_impl(p, scaled_omega, tau, taus0, scale_tau, wleg, mu0, I0, phi0, rescale, b_pos, b_neg, s_poly, bdrf_q, bdrf_q0,
                          false);
}

int rtd_plan_set_columns_local(rtd_plan* p, const double* scaled_omega, const double* tau, const double* taus0,
                               const double* scale_tau, const double* wleg, const double* mu0, const double* I0,
                               const double* phi0, const double* rescale, const double* b_pos, const double* b_neg,
                               const double* s_local, const double* bdrf_q, const double* bdrf_q0) {
  return set_columns_impl(p, scaled_omega, tau, taus0, scale_tau, wleg, mu0, I0, phi0, rescale, b_pos, b_neg, s_local, bdrf_q, bdrf_q0,
                          true);
}

int rtd_source_polynomials_local(int64_t ncolumns, int32_t nlayers, int32_t nscoeffs, const double* tau_arr, const double* omega_arr,
                                 const double* f_arr, const double* s_poly, double* s_local) {
  if (ncolumns < 0 || nlayers < 1 || nscoeffs < 1 || !tau_arr || !omega_arr || !f_arr || !s_poly || !s_local)
    return fail(RTD_ERR_ARG, "rtd_source_polynomials_local: null argument or empty dimension");
  for (int64_t c = 0; c < ncolumns; ++c) {
    double top = 0.0;
    for (int64_t l = 0; l < nlayers; ++l) {
      const int64_t cl = c * nlayers + l;
      rtd_source_local(s_poly + cl * nscoeffs, s_local + cl * nscoeffs, nscoeffs, top, 1.0 - omega_arr[cl] * f_arr[cl], omega_arr[cl]);
      top = tau_arr[cl];
    }
  }
  return 0;
}

namespace {

// Thermal sources from temperatures (include/rtd.h: rtd_thermal; the reference's host helpers generate_s_poly_coeffs,
// blackbody_contrib_to_BCs, generate_emissivity_from_BDRF: subroutines.py:413-454, :354-377, :459-486).  The math is
// csrc/rtd_planck.h; one thread per integral, no LDS, no barrier, no cross-lane operation -- the stage moves a few bytes per
// integral of ~300 exponentials and is nowhere near a limit of the device.
struct RtdThermalDev {
  const double *temper, *lo, *hi, *btemp, *ttemp, *temis, *emis;  // the caller's arrays (staged), NULL as there
  const double* tau;                                              // [C][L] unscaled lower boundaries (staged)
  double *E;                                                      // [C][L + 3]: the L + 1 levels, then bottom and top boundary
  double *spoly, *bpos, *bneg;                                    // the raw arrays the preparation kernel reads
};

__global__ void rtd_planck_band_kernel(long n, const double* T, const double* lo, const double* hi, double* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = rtd_planck_band(T[i], lo[i], hi[i]);
}

// Parametric surface models (include/rtd.h: rtd_surface; the math is csrc/rtd_surface.h).  One thread per sample rho(mu, mu',
// 2 pi p / nphi), the azimuth index p fastest; no LDS, no barrier, no cross-lane operation (the stand-in runtime of tests/cpu runs
// the kernel thread by thread).  ONE kernel for both callers, so the bits of a sample cannot differ between them:
//   N > 0   the rows of a plan's chunk of `cnt` columns from c0 on, laid out as rtd_bdrf_modes_kernel reads them: cnt N N rows
//           (c, i, j) -> rho(mu_i, mu_j), then -- mu0 not null -- cnt N rows (c, i) -> rho(mu_i, mu0[c0 + c]) with the STAGED raw mu0;
//           the parameter row of column c0 + c is (c0 + c) / group, or 0 when the surface is shared (par_rows = 1);
//   N = 0   the plan-free rows: mu[r], mup[r] and par[r][4] as given.
struct RtdSurfDev {
  int model, nphi, N, group;
  long nrows, cnt, c0, par_rows;
  const double* par;        // [par_rows][4]
  const double *mu, *mup;   // N > 0: the plan's nodes (d.mu) and the raw mu0 [C] (null: no mu0 rows); N = 0: [nrows] each
  double* out;              // [nrows][nphi]
};

__global__ void rtd_surface_samples_kernel(RtdSurfDev v) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= v.nrows * v.nphi) return;
  long r = idx / v.nphi;
  const int p = (int)(idx % v.nphi);
  double mu, mup;
  long prow;
  if (v.N > 0) {
    const long N = v.N, nqq = v.cnt * N * N;
    long c;
    if (r < nqq) {
      c = r / (N * N);
      mu = v.mu[(r / N) % N];
      mup = v.mu[r % N];
    } else {
      r -= nqq;
      c = r / N;
      mu = v.mu[r % N];
      mup = v.mup[v.c0 + c];
    }
    prow = v.par_rows == 1 ? 0 : (v.c0 + c) / v.group;
  } else {
    mu = v.mu[r];
    mup = v.mup[r];
    prow = r;
  }
  double c, s;
  rtd_surface_cs(2.0 * (double)p / (double)v.nphi, &c, &s);
  v.out[idx] = rtd_surface_rho(v.model, v.par + 4 * prow, mu, mup, c, s);
}

// A Lambertian surface needs no sampling: q^0 = albedo at the N real nodes of every column of the (zeroed) tables, q^m = 0 beyond.
// One thread per (c, i, j), j fastest; j = N stands for the mu0 column (skipped when with_q0 = 0).
__global__ void rtd_surface_lambert_kernel(RtdDev d, RtdSurfDev v, int with_q0) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long N = d.N, NP = d.NP, NB = d.NBDRF;
  if (idx >= (long)d.C * N * (N + 1)) return;
  const long c = idx / (N * (N + 1)), i = (idx / (N + 1)) % N, j = idx % (N + 1);
  const double albedo = v.par[4 * (v.par_rows == 1 ? 0 : c / v.group)];
  if (j < N) const_cast<double*>(d.bdrfq)[(c * NB * NP + i) * NP + j] = albedo;
  else if (with_q0) const_cast<double*>(d.bdrfq0)[c * NB * NP + i] = albedo;
}

__global__ void rtd_thermal_emission_kernel(RtdDev d, RtdThermalDev t) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (c, k): k <= L a level, L + 1 the bottom, L + 2 the top boundary
  const int K = d.L + 3;
  if (idx >= (long)d.C * K) return;
  const long c = idx / K;
  const int k = (int)(idx % K);
  const double T = k <= d.L ? t.temper[c * (d.L + 1) + k] : k == d.L + 1 ? (t.btemp ? t.btemp[c] : 0.0) : (t.ttemp ? t.ttemp[c] : 0.0);
  t.E[idx] = rtd_planck_band(T, t.lo[c], t.hi[c]);
}

__global__ void rtd_thermal_sources_kernel(RtdDev d, RtdThermalDev t) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d.C) return;
  const int L = d.L, M = d.M, N = d.N, NP = d.NP, NB = d.NBDRF;
  const double* E = t.E + c * (L + 3);
  // linear_spline_coefficients (subroutines.py:381-409) through (0, tau_0, ..., tau_{L-1}) x (E_0 ... E_L): (intercept, slope)
  double top = 0.0;
  for (int l = 0; l < L; ++l) {
    const double bot = t.tau[c * L + l], slope = (E[l + 1] - E[l]) / (bot - top);
    t.spoly[(c * L + l) * 2] = E[l] - slope * top;
    t.spoly[(c * L + l) * 2 + 1] = slope;
    top = bot;
  }
  if (t.btemp) {  // b_pos of mode 0 += emissivity x blackbody emission of the surface (pydisotest/9_test.py:196-197)
    const double* q = NB > 0 ? d.bdrfq + c * NB * NP * NP : nullptr;  // the zeroth mode, rows padded to NP
    for (int i = 0; i < N; ++i) {
      double em = 1.0;
      if (t.emis) {
        em = t.emis[c * N + i];
      } else if (q) {  // Kirchhoff: 1 - 2 sum_j q^0(mu_i, mu_j) mu_j w_j over the N real nodes
        double s = 0.0;
        for (int j = 0; j < N; ++j) s += q[i * NP + j] * d.mu[j] * d.w[j];
        em = 1.0 - 2.0 * s;
      }
      t.bpos[c * M * N + i] += em * E[L + 1];
    }
  }
  if (t.ttemp) {  // b_neg of mode 0 += TEMIS x blackbody emission of the top boundary (:198-199)
    const double v = (t.temis ? t.temis[c] : 1.0) * E[L + 2];
    for (int i = 0; i < N; ++i) t.bneg[c * M * N + i] += v;
  }
}

// k-distribution bands (include/rtd.h: rtd_band): the optical properties of the columns c = p G + g mixed from the band's small
// arrays, and the spectral integral of the results.  Streaming kernels, one thread per output element with the fastest thread
// index along the contiguous axis; no LDS, no barrier, no cross-lane operation (the stand-in runtime of tests/cpu runs them
// thread by thread).  Loop orders are fixed (s ascending, l ascending, g ascending): no result depends on the launch geometry.
struct RtdBandDev {
  long P;
  int G, S, L, nleg, nleg_all, delta_m;
  const double *abs, *dspec, *ospec, *lspec;  // the caller's arrays (staged): [P][G][L], [P][L][S], [P][L][S], [S][nleg_all]
  double *tau, *omega, *f, *leg;              // [C][L] x 3, [C][L][nleg]: the raw arrays the preparation kernel reads
};

// one thread per (c, l), l fastest: omega, f, and the layer's optical thickness in tau's place
__global__ void rtd_band_layers_kernel(RtdBandDev b) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= b.P * b.G * b.L) return;
  const long c = idx / b.L, p = c / b.G;
  const int l = (int)(idx % b.L), g = (int)(c % b.G);
  const double* dt = b.dspec + (p * b.L + l) * b.S;
  const double* om = b.ospec + (p * b.L + l) * b.S;
  double sca = 0.0, ext = 0.0, fs = 0.0;
  for (int s = 0; s < b.S; ++s) {
    const double t = om[s] * dt[s];
    sca += t;
    ext += dt[s];
    if (b.delta_m) fs += t * b.lspec[(long)s * b.nleg_all + b.nleg];
  }
  const double dtau = ext + b.abs[(p * b.G + g) * b.L + l];
  b.tau[idx] = dtau;
  b.omega[idx] = sca / dtau;
  b.f[idx] = (b.delta_m && sca != 0.0) ? fs / sca : 0.0;
}

// one thread per column: the running sum of the layers' thicknesses, in place (L is tens)
__global__ void rtd_band_tau_kernel(RtdBandDev b) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= b.P * b.G) return;
  double* t = b.tau + c * b.L;
  double run = 0.0;
  for (int l = 0; l < b.L; ++l) {
    run += t[l];
    t[l] = run;
  }
}

// one thread per (c, l, k), k fastest: the moments of the mixture (they do not depend on g: the absorber does not scatter)
__global__ void rtd_band_moments_kernel(RtdBandDev b) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= b.P * b.G * b.L * b.nleg) return;
  const int k = (int)(idx % b.nleg);
  const long cl = idx / b.nleg, c = cl / b.L, p = c / b.G;
  const int l = (int)(cl % b.L);
  const double* dt = b.dspec + (p * b.L + l) * b.S;
  const double* om = b.ospec + (p * b.L + l) * b.S;
  b.leg[idx] = rtd_mix_moment(dt, om, b.lspec, b.S, b.nleg_all, k);  // (rtd_nt_prep.h: shared with the band's full phase function)
}

void band_mix_launch(const RtdBandDev& b, hipStream_t s) {
  const long C = b.P * b.G, n_cl = C * b.L, n_leg = n_cl * b.nleg;
  hipLaunchKernelGGL(rtd_band_layers_kernel, grid_1d(n_cl), dim3(256), 0, s, b);
  hipLaunchKernelGGL(rtd_band_tau_kernel, grid_1d(C), dim3(256), 0, s, b);
  hipLaunchKernelGGL(rtd_band_moments_kernel, grid_1d(n_leg), dim3(256), 0, s, b);
}

// The inputs of the Nakajima-Tanaka corrections from what rtd_plan_set_columns_raw / _thermal / _band stage (rtd_plan_request_nt; the
// arithmetic is rtd_nt_prep.h), all d.C columns.  Like the band and thermal preparation these kernels live in this translation unit:
// streaming, no LDS, no barrier, no cross-lane operation, so the stand-in runtime of tests/cpu runs them thread by thread.
struct RtdNtPrep {
  int nleg_all, group;            // group: columns per row of the full moments (1: raw columns; G: a band)
  long rows;                      // d.C / group
  const double *tau, *omega, *f;  // [C][L]  the RAW tau_arr, omega_arr, f_arr (staged or mixed)
  double* leg;                    // [rows][L][nleg_all] full moments: uploaded (raw columns, only read) or mixed here (band)
  int S;                          // > 0: a band -- leg is formed from the species' arrays below
  const double *dspec, *ospec, *lspec;  // [rows][L][S], [rows][L][S], [S][nleg_all]
  double *wfull, *ims_coef, *ims_par;   // outputs: [rows][L][nleg_all], [C][nleg_all], [C][2]
};

// One thread per output element, k fastest: reads and writes are contiguous across the wavefront.
__global__ void rtd_nt_wfull_kernel(RtdNtPrep q, int L) {  // raw columns: (2k + 1) x the uploaded moment
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= q.rows * L * q.nleg_all) return;
  const int k = (int)(idx % q.nleg_all);
  q.wfull[idx] = (2.0 * k + 1.0) * q.leg[idx];
}

// a band: the mixture's moment (rtd_mix_moment, the expression of rtd_band_moments_kernel) once per PROFILE, kept unweighted for the
// IMS averages and weighted for the TMS series
__global__ void rtd_nt_wfull_band_kernel(RtdNtPrep q, int L) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= q.rows * L * q.nleg_all) return;
  const int k = (int)(idx % q.nleg_all);
  const long rl = idx / q.nleg_all;  // (row, layer)
  const double g = rtd_mix_moment(q.dspec + rl * q.S, q.ospec + rl * q.S, q.lspec, q.S, q.nleg_all, k);
  q.leg[idx] = g;
  q.wfull[idx] = (2.0 * k + 1.0) * g;
}

// One wavefront per column, lanes striding over k: at each l the wavefront reads 64 consecutive moments.  No LDS, no barrier, no
// cross-lane operation, no atomics (rtd_nt_prep.h says what each lane sums).
__global__ void rtd_nt_ims_kernel(RtdDev d, RtdNtPrep q) {
  const long c = (long)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  if (c >= d.C) return;
  const long L = d.L;
  rtd_nt_ims_lane(d.L, d.P, q.nleg_all, q.tau + c * L, q.omega + c * L, q.f + c * L, q.leg + (c / q.group) * L * q.nleg_all, d.mu0[c],
                  d.I0[c], (int)(threadIdx.x & 63), 64, q.ims_coef + c * q.nleg_all, q.ims_par + c * 2);
}

void nt_prepare_launch(const RtdDev& d, const RtdNtPrep& q, hipStream_t s) {  // behind rtd_launch_prepare: reads d.mu0, d.I0
  const long n = q.rows * d.L * q.nleg_all;
  const dim3 grid = grid_1d(n);
  if (q.S > 0) hipLaunchKernelGGL(rtd_nt_wfull_band_kernel, grid, dim3(256), 0, s, q, d.L);
  else hipLaunchKernelGGL(rtd_nt_wfull_kernel, grid, dim3(256), 0, s, q, d.L);
  hipLaunchKernelGGL(rtd_nt_ims_kernel, dim3((unsigned)(((long)d.C + 3) / 4)), dim3(256), 0, s, d, q);
}

// The device view of a band: its sizes, the four mixed arrays carved from `out` ([C][L] x 3, then [C][L][nleg]) and the caller's four
// arrays where they are staged, one after the other from `in` on (null: not staged yet).  The extents of both carves: band_extents.
struct BandExtents { int64_t n_cl, n_leg, n_abs, n_spec, n_lspec; };
BandExtents band_extents(const rtd_band* b, int64_t L, int64_t nleg) {
  const int64_t C = (int64_t)b->nprofiles * b->ngpoints;
  return {C * L, C * L * nleg, C * L, (int64_t)b->nprofiles * L * b->nspecies, (int64_t)b->nspecies * b->nleg_all};
}
RtdBandDev band_dev(const rtd_band* band, int64_t L, int64_t nleg, double* out, const double* in) {
  const BandExtents x = band_extents(band, L, nleg);
  RtdBandDev b{};
  b.P = band->nprofiles; b.G = band->ngpoints; b.S = band->nspecies; b.L = (int)L; b.nleg = (int)nleg; b.nleg_all = band->nleg_all;
  b.delta_m = band->delta_m ? 1 : 0;
  b.tau = out; b.omega = out + x.n_cl; b.f = out + 2 * x.n_cl; b.leg = out + 3 * x.n_cl;
  if (in) { b.abs = in; b.dspec = in + x.n_abs; b.ospec = in + x.n_abs + x.n_spec; b.lspec = in + x.n_abs + 2 * x.n_spec; }
  return b;
}

// argument check shared by rtd_band_mix and rtd_plan_set_columns_band; returns nullptr when the band is fine
const char* band_bad(const rtd_band* b, int64_t nleg) {
  if (!b || !b->dtau_abs || !b->dtau_spec || !b->omega_spec || !b->leg_spec) return "band: null argument";
  if (b->nprofiles < 1 || b->ngpoints < 1) return "band: need nprofiles >= 1 and ngpoints >= 1";
  if (b->nspecies < 1) return "band: need at least one scatterer species";
  if ((int64_t)b->nprofiles * b->ngpoints > INT32_MAX) return "band: nprofiles x ngpoints exceeds the column count of a plan";
  if (b->nleg_all < nleg + (b->delta_m ? 1 : 0)) return "band: nleg_all must be >= nleg (+ 1 with delta_m)";
  return nullptr;
}

// out[p][k][e] = sum_g w[k][g] X[p G + g][e]: one thread per (p, e), e fastest, so that the reads of X are contiguous across the
// wavefront; K accumulators in double-double (exact products, rtd_dd.h) held in registers in chunks of at most 4 -- X is read
// again for further chunks; the kernel is bound by that read, the arithmetic hides behind it.  mask: the bits of col_status that
// spoil this output (0xFF: mode 0 alone for u0 and the fluxes; 0xFFFF for u) -- a profile with such a column is NaN.
//
// The rounded product passes through rtd_band_opaque on its way from rtd_two_prod to rtd_dd_add.  The device compiler contracts
// floating-point expressions across inlined functions: a + fl(w v) would become fma(w, v, a), the error term of the two-sum would
// then already hold the product's rounding error, and the low half of rtd_two_prod would add it a second time -- a sum no better
// than a float64 one.  An empty asm statement that names the register keeps the multiplication and the addition apart.
__device__ __host__ inline double rtd_band_opaque(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(x));
#endif
  return x;
}

extern "C++" template <int NK>  // (this part of the file has C linkage for the entry points)
__device__ __host__ inline void rtd_band_reduce_chunk(const double* x, const double* w, int G, long E, bool bad, double* out) {
  rtd_dd acc[NK];
  for (int j = 0; j < NK; ++j) acc[j] = {0.0, 0.0};
  for (int g = 0; g < G; ++g) {
    const double v = x[(long)g * E];
    for (int j = 0; j < NK; ++j) {
      rtd_dd t = rtd_two_prod(w[(long)j * G + g], v);
      t.hi = rtd_band_opaque(t.hi);
      acc[j] = rtd_dd_add(acc[j], t);
    }
  }
  for (int j = 0; j < NK; ++j) out[(long)j * E] = bad ? __builtin_nan("") : acc[j].hi + acc[j].lo;
}

__global__ void rtd_band_reduce_kernel(const double* X, const double* w, const int* col_status, int mask, long P, int G, int K,
                                       long E, double* out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P * E) return;
  const long p = idx / E, e = idx % E;
  bool bad = false;
  for (int g = 0; g < G; ++g) bad = bad || (col_status[p * G + g] & mask) != 0;
  const double* x = X + p * G * E + e;
  for (int k0 = 0; k0 < K; k0 += 4) {
    const double* wk = w + (long)k0 * G;
    double* o = out + (p * K + k0) * E + e;
    switch (K - k0) {
      case 1: rtd_band_reduce_chunk<1>(x, wk, G, E, bad, o); break;
      case 2: rtd_band_reduce_chunk<2>(x, wk, G, E, bad, o); break;
      case 3: rtd_band_reduce_chunk<3>(x, wk, G, E, bad, o); break;
      default: rtd_band_reduce_chunk<4>(x, wk, G, E, bad, o); break;
    }
  }
}

// Actinic fluxes (4 pi x mean intensity) of the results the plan holds: the reference's generate_diff_act_flux_funcs
// (subroutines.py:258-318) for every column and point at once.  One thread per (column c, point t), lanes along t, then c: for
// each stream i a wavefront reads runs of ntau consecutive doubles of u0 [C][2N][ntau].  The sum over the streams is one chain, i
// ascending, no atomics: the bits depend on nothing but the inputs.  x = u0 carries `rescale` already; I0 here is the CALLER's
// beam, rescale * d.I0 (pydisort.py:311-326) -- the reference applies the reclassification term R with its rescaled I0 and does not
// multiply back.  order: -1 the tau-antiderivative, 0 the value, +1 the tau-derivative, the order u0 was
// evaluated in; layer lookup and one-sided conventions as rtd_eval_kernel's.
//   act [0][c][t] = 2 pi sum_i w_i x_i               (up)
//   act [1][c][t] = 2 pi sum_i w_i x_{N+i} + R       (down, diffuse; R = I0 e^(-tau* / mu0) - I0 e^(-tau / mu0))
//   act [2][c][t] = D = I0 e^(-tau / mu0)            (down, direct: flux_down_direct / mu0)
// R = D = 0 without a beam and where I0 = 0; everything is 0 on a mode shard that does not own mode 0.
__global__ void rtd_actinic_kernel(RtdDev d, const double* ev_tau, const double* u0, int ntau, int order, double* act) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x, CT = (long)d.C * ntau;
  if (idx >= CT) return;
  const long c = idx / ntau;
  const int t = (int)(idx % ntau), L = d.L, N = d.N;
  double up = 0.0, dn = 0.0, R = 0.0, D = 0.0;
  if (d.m0 == 0) {
    const double* x = u0 + c * 2 * N * ntau + t;
    for (int i = 0; i < N; ++i) {
      up += d.w[i] * x[(long)i * ntau];
      dn += d.w[i] * x[(long)(N + i) * ntau];
    }
    up *= 2.0 * M_PI;
    dn *= 2.0 * M_PI;
    const double I0 = d.beam ? d.rescale[c] * d.I0[c] : 0.0;
    if (I0 != 0.0) {
      const double tau = ev_tau[idx], mu0 = d.mu0[c];
      const double* tau_arr = d.tau + c * L;
      int l = 0;
      // argmax(tau <= tau_arr), always by search.  The fused evaluation behind rtd_plan_run takes l = t - 1 at the interfaces
      // instead (rtd_eval.hip, rtd_fourier.hip); the two agree unless a layer has zero thickness (tau_arr[l] == tau_arr[l + 1]).
      // There tau* and so the value order are the same under either rule, but sc of the derivative and antiderivative factors
      // below is the upper layer's, while the resident u0 they are added to was formed with the empty layer's.
      while (l < L - 1 && !(tau <= tau_arr[l])) ++l;
      const double sc = d.scale[c * L + l];
      const double ts = d.taus0[c * (L + 1) + l + 1] - (tau_arr[l] - tau) * sc;
      double es = I0 * exp(-ts / mu0), ed = I0 * exp(-tau / mu0);
      if (order < 0) {
        es /= (-sc / mu0);
        ed *= -mu0;
      } else if (order > 0) {
        es *= (-sc / mu0);
        ed /= -mu0;
      }
      R = es - ed;
      D = ed;
    }
  }
  act[idx] = up;
  act[CT + idx] = dn + R;
  act[2 * CT + idx] = D;
}

// Radiances at user polar angles: the reference's subroutines.interpolate (subroutines.py:614-705), barycentric polynomial
// interpolation in mu of the results the plan holds, each hemisphere on its own, for every column, angle and point at once.  The
// operator is LINEAR in the rows of u / u0 and does not touch tau or phi, so it commutes with everything the result buffers may
// hold: values, tau-antiderivatives or tau-derivatives (res_order), u with its Nakajima-Tanaka corrections, the partial sums of a
// mode shard (the shards' interpolants add up to the interpolant of the sum).  It is polynomial interpolation of the evaluated u,
// not an integration of the source function.
//
// Basis.  x_j, j < N, the positive nodes; the rows of u are [x_0 .. x_{N-1}, -x_0 .. -x_{N-1}].  mu > 0 reads the rows 0 .. N-1,
// every other mu -- +0.0 and -0.0 included, the reference's mask is `mu > 0` -- the rows N .. 2N-1.  With a = |mu| the basis is the
// same for both (the sign of the negated nodes cancels in the quotient):
//   l_j(a) = (b_j / (a - x_j)) / sum_k (b_k / (a - x_k)),   b_j = 1 / prod_{k != j} (x_j - x_k)
// b comes from the host (view_weights: long double, rounded once, scaled by the largest magnitude -- only ratios matter).  If
// a == x_j the basis is the unit vector e_j and the flag carries j: the apply kernel then COPIES row j, bit for bit, as the
// reference assigns yi[j].  One thread per (column, angle); n = C nmu, or nmu for a list shared by the columns.
//   flag = hemisphere (bit 0: 1 = the rows N .. 2N-1) | (j + 1) << 8 at a node
__global__ void rtd_view_basis_kernel(const double* mu, long n, const double* x, const double* b, int N, double* l, int* flag) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const double m = mu[idx], a = fabs(m);
  double* lj = l + idx * N;
  int hit = -1;
  for (int j = 0; j < N; ++j)
    if (a == x[j]) hit = j;
  if (hit >= 0) {
    for (int j = 0; j < N; ++j) lj[j] = j == hit ? 1.0 : 0.0;
  } else {
    double s = 0.0;
    for (int j = 0; j < N; ++j) {
      const double t = b[j] / (a - x[j]);
      lj[j] = t;
      s += t;
    }
    for (int j = 0; j < N; ++j) lj[j] /= s;
  }
  flag[idx] = (m > 0.0 ? 0 : 1) | ((hit + 1) << 8);
}

// out [C][nmu][E] = sum_j l[c][m][j] X[c][h N + j][E], X = ev_u (E = ntau nphi) or ev_u0 (E = ntau).  One thread per output
// element, e fastest across the lanes: for each j a wavefront reads runs of consecutive doubles.  The sum is one chain, j ascending,
// no atomics, no cross-lane reduction: the bits depend on the inputs alone, not on the launch geometry or the window size.
// lstride / fstride: doubles / ints from one column's basis and flags to the next, 0 for a shared list.
__global__ void rtd_view_apply_kernel(const double* l, long lstride, const int* flag, long fstride, const double* X, int N, int nmu,
                                      long E, long C, double* out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= C * nmu * E) return;
  const long e = idx % E, cm = idx / E, c = cm / nmu;
  const int m = (int)(cm % nmu), f = flag[c * fstride + m];
  const double* x = X + (c * 2 * N + ((f & 1) ? N : 0)) * E + e;
  const double* lj = l + c * lstride + (long)m * N;
  double acc;
  if (f >> 8) {
    acc = x[(long)((f >> 8) - 1) * E];
  } else {
    acc = lj[0] * x[0];
    for (int j = 1; j < N; ++j) acc += lj[j] * x[(long)j * E];
  }
  out[idx] = acc;
}

// How a plan's upload spends the scratch budget of the surface samples (RTD_SURFACE_BYTES): the staged parameters first, then the
// samples of `chunk` columns at a time.
struct SurfLayout {
  int64_t par = 0, per_col = 0, chunk = 0;
  int64_t total() const { return par + chunk * per_col; }
};
void surface_layout(const rtd_plan* p, SurfLayout* out) {
  const RtdDev& d = p->d;
  SurfLayout l;
  l.par = (int64_t)p->surf_par.size();
  if (p->surf_model != RTD_SURFACE_LAMBERT && p->surf_model != RTD_SURFACE_OCEAN) {  // (the ocean's kernel holds no samples in memory)
    l.per_col = ((int64_t)d.N * d.N + (d.beam ? d.N : 0)) * p->surf_nphi;
    l.chunk = columns_per_chunk(budget_doubles(getenv("RTD_SURFACE_BYTES")), l.per_col, d.C);
  }
  *out = l;
}

// bdrf_q / bdrf_q0 of all columns from the requested surface, queued on s behind the quadrature and the staged raw mu0 [C]: the
// tables are zeroed as rtd_plan_set_bdrf_samples zeroes them, then chunk after chunk is sampled into the scratch block and reduced
// by rtd_bdrf_modes_kernel under a descriptor shifted to the chunk's columns, as the windows shift theirs.  One wavefront reduces one
// sample vector whatever the chunk: the result does not depend on the chunk size.  group: columns per parameter row.
hipError_t surface_tables(const rtd_plan* p, const double* mu0_raw, int group, double* blk, const SurfLayout& lay, hipStream_t s) {
  const RtdDev& d = p->d;
  const int64_t C = d.C, N = d.N, NP = d.NP, NB = d.NBDRF;
  hipError_t e = hipMemcpyAsync(blk, p->surf_par.data(), (size_t)lay.par * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(const_cast<double*>(d.bdrfq), 0, (size_t)(C * NB * NP * NP) * 8, s);
  if (e == hipSuccess) e = hipMemsetAsync(const_cast<double*>(d.bdrfq0), 0, (size_t)(C * NB * NP) * 8, s);
  if (e != hipSuccess) return e;
  RtdSurfDev v{};
  v.model = p->surf_model; v.nphi = p->surf_nphi; v.N = (int)N; v.group = group; v.par_rows = p->surf_rows;
  v.par = blk; v.mu = d.mu; v.mup = d.beam ? mu0_raw : nullptr;
  if (v.model == RTD_SURFACE_LAMBERT) {
    const int64_t n = C * N * (N + 1);
    hipLaunchKernelGGL(rtd_surface_lambert_kernel, grid_1d(n), dim3(256), 0, s, d, v, d.beam ? 1 : 0);
    return hipGetLastError();
  }
  if (v.model == RTD_SURFACE_OCEAN) {  // modes on the clustered grid, one pass per pair of cosines (csrc/rtd_surface_ocean.hip)
    rtd_launch_surface_ocean(d, v.nphi, blk, p->surf_rows, group, mu0_raw, s);
    return hipGetLastError();
  }
  v.out = blk + lay.par;
  for (int64_t c0 = 0; c0 < C && e == hipSuccess; c0 += lay.chunk) {
    const int64_t cnt = std::min<int64_t>(lay.chunk, C - c0), nqq = cnt * N * N * v.nphi;
    v.c0 = c0; v.cnt = cnt; v.nrows = cnt * (N * N + (d.beam ? N : 0));
    hipLaunchKernelGGL(rtd_surface_samples_kernel, grid_1d(v.nrows * v.nphi), dim3(256), 0, s, v);
    RtdDev w = d;
    w.C = (int)cnt; w.bdrfq += c0 * NB * NP * NP; w.bdrfq0 += c0 * NB * NP;
    rtd_launch_bdrf_modes(w, v.nphi, v.out, d.beam ? v.out + nqq : nullptr, s);
    e = hipGetLastError();
  }
  return e;
}

// first row of params [rows][4] that `model` does not admit, with what is wrong in *why; -1: none
int64_t surface_bad_row(int model, int64_t rows, const double* params, const char** why) {
  for (int64_t r = 0; r < rows; ++r)
    if ((*why = rtd_surface_bad(model, params + 4 * r))) return r;
  return -1;
}

}  // namespace

int rtd_plan_request_surface(rtd_plan* p, const rtd_surface* sf) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (!sf || sf->model < 0) {  // withdrawn: the next upload takes tables again
    p->surf_model = -1;
    p->surf_par.clear();
    p->surf_rows = 0;
    return 0;
  }
  const RtdDev& d = p->d;
  if (d.NBDRF <= 0) return fail(RTD_ERR_ARG, "request_surface: the plan was created with nbdrf = 0");
  if (sf->model >= RTD_SURFACE_NMODELS || sf->rows < 1 || !sf->params) return fail(RTD_ERR_ARG, "request_surface: unknown model, rows < 1 or null params");
  if (!(2 * ((int64_t)d.NBDRF - 1) < sf->nphi && sf->nphi <= 16384)) return fail(RTD_ERR_ARG, "request_surface: need 2 (nbdrf - 1) < nphi <= 16384");
  if (sf->model == RTD_SURFACE_OCEAN && (sf->nphi % 2 != 0 || sf->nphi < 4 * (int64_t)d.NBDRF))
    return fail(RTD_ERR_ARG, "request_surface: the ocean's clustered grid needs an even nphi >= 4 nbdrf");
  const char* why = nullptr;
  const int64_t bad = surface_bad_row(sf->model, sf->rows, sf->params, &why);
  if (bad >= 0) return fail(RTD_ERR_ARG, std::string("request_surface: row ") + std::to_string(bad) + ": " + why);
  p->surf_model = sf->model;
  p->surf_nphi = sf->nphi;
  p->surf_rows = sf->rows;
  p->surf_par.assign(sf->params, sf->params + (size_t)sf->rows * 4);
  return 0;
}

int rtd_surface_samples(int32_t device, int32_t model, int64_t n, const double* params, const double* mu, const double* mup, int32_t nphi,
                        double* rho) {
  if (n < 0 || nphi < 1 || nphi > 16384 || (n > 0 && (!params || !mu || !mup || !rho)))
    return fail(RTD_ERR_ARG, "surface_samples: null argument, n < 0 or nphi outside 1 ... 16384");
  if (model < 0 || model >= RTD_SURFACE_NMODELS) return fail(RTD_ERR_ARG, "surface_samples: unknown model");
  const char* why = nullptr;
  const int64_t bad = surface_bad_row(model, n, params, &why);
  if (bad >= 0) return fail(RTD_ERR_ARG, std::string("surface_samples: row ") + std::to_string(bad) + ": " + why);
  for (int64_t r = 0; r < n; ++r)
    if (!(mu[r] > 0.0 && mu[r] <= 1.0 && mup[r] > 0.0 && mup[r] <= 1.0))
      return fail(RTD_ERR_ARG, "surface_samples: row " + std::to_string(r) + ": mu and mup must lie in (0, 1]");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(device));
  const int64_t chunk = columns_per_chunk(budget_doubles(getenv("RTD_SURFACE_BYTES")), nphi + 6, n);  // rows per pass
  Scratch blk;
  HIP_TRY(blk.get(chunk * (nphi + 6), device));
  double* buf = blk.data();
  hipError_t e = hipSuccess;
  for (int64_t r0 = 0; r0 < n && e == hipSuccess; r0 += chunk) {
    const int64_t cnt = std::min<int64_t>(chunk, n - r0);
    RtdSurfDev v{};
    v.model = model; v.nphi = nphi; v.N = 0; v.group = 1; v.nrows = cnt; v.cnt = cnt; v.par_rows = cnt;
    v.par = buf; v.mu = buf + 4 * cnt; v.mup = buf + 5 * cnt; v.out = buf + 6 * cnt;
    e = upload_parts(buf, {{params + 4 * r0, 4 * cnt}, {mu + r0, cnt}, {mup + r0, cnt}});
    if (e == hipSuccess) {
      hipLaunchKernelGGL(rtd_surface_samples_kernel, grid_1d(cnt * nphi), dim3(256), 0, (hipStream_t)0, v);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(rho + r0 * nphi, v.out, (size_t)(cnt * nphi) * 8, hipMemcpyDeviceToHost);  // (waits for the kernel)
  }
  return finish(e, (hipStream_t)0, "surface_samples");
}

int rtd_plan_get_bdrf(rtd_plan* p, double* q, double* q0) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (!p->have_cols) return fail(RTD_ERR_STATE, "get_bdrf: no columns are set");
  const RtdDev& d = p->d;
  const int64_t C = d.C, N = d.N, NP = d.NP, NB = d.NBDRF;
  if (NB <= 0 || (!q && !q0)) return 0;
  HIP_TRY(hipSetDevice(p->device));
  std::vector<double> h((size_t)(C * NB * NP * (q ? NP : 1)));
  // pad_streams undone: tables [N][N] of q, rows [N] of q0, padded from N to NP on the device
  const struct { double* host; const double* dev; int64_t rows, rows_dev; } tabs[2] = {{q, d.bdrfq, N, NP}, {q0, d.bdrfq0, 1, 1}};
  for (const auto& t : tabs) {
    if (!t.host) continue;
    HIP_TRY(hipMemcpyAsync(h.data(), t.dev, (size_t)(C * NB * t.rows_dev * NP) * 8, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    for (int64_t b = 0; b < C * NB; ++b)
      for (int64_t i = 0; i < t.rows; ++i)
        for (int64_t j = 0; j < N; ++j) t.host[(b * t.rows + i) * N + j] = h[(size_t)((b * t.rows_dev + i) * NP + j)];
  }
  p->stream_drained();
  return 0;
}

int rtd_planck_band(int32_t device, int64_t n, const double* T, const double* wvnmlo, const double* wvnmhi, double* out) {
  if (n < 0 || (n > 0 && (!T || !wvnmlo || !wvnmhi || !out))) return fail(RTD_ERR_ARG, "planck_band: null argument or n < 0");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(device));
  Scratch blk;
  HIP_TRY(blk.get(4 * n, device));
  double* buf = blk.data();
  hipError_t e = upload_parts(buf, {{T, n}, {wvnmlo, n}, {wvnmhi, n}});
  if (e == hipSuccess) {
    hipLaunchKernelGGL(rtd_planck_band_kernel, grid_1d(n), dim3(256), 0, (hipStream_t)0, (long)n, buf,
                       buf + n, buf + 2 * n, buf + 3 * n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, buf + 3 * n, (size_t)n * 8, hipMemcpyDeviceToHost);  // (waits for the kernel)
  return finish(e, (hipStream_t)0, "planck_band");
}

// rtd_plan_set_columns_raw (th == nullptr: exactly its copies and launches), rtd_plan_set_columns_thermal (s_poly == nullptr,
// the source polynomials and the boundary emissions are formed in the staging block before the preparation kernel reads it) and
// rtd_plan_set_columns_band (band != nullptr: tau_arr, omega_arr, f_arr and leg_all are not uploaded but mixed on the device into
// the same carves of the staging block, nleg moments per layer, ahead of the thermal kernels; the mixed tau comes back into h_tau)
static int set_columns_raw_impl(rtd_plan* p, const double* tau_arr, const double* omega_arr, const double* leg_all,
                                int32_t nleg_all, const double* f_arr, const double* mu0, const double* I0,
                                const double* phi0, const double* b_pos, const double* b_neg, const double* s_poly,
                                const double* bdrf_q, const double* bdrf_q0, const rtd_thermal* th, const rtd_band* band = nullptr,
                                double* tau_out = nullptr) {
  if (!p || !mu0 || !I0 || !phi0) return fail(RTD_ERR_ARG, "null argument");
  if (!band && (!tau_arr || !omega_arr || !leg_all || !f_arr)) return fail(RTD_ERR_ARG, "null argument");
  const RtdDev& d = p->d;
  if (band) {
    if (const char* bad = band_bad(band, d.P)) return fail(RTD_ERR_ARG, bad);
    if ((int64_t)band->nprofiles * band->ngpoints != d.C) return fail(RTD_ERR_ARG, "band: the plan must have ncols = nprofiles x ngpoints");
    if (sharded(p)) return fail(RTD_ERR_STATE, "band inputs are not combined with a mode shard or a communicator");
    nleg_all = d.P;  // the staging block holds the moments the solver uses
  }
  if (nleg_all < d.P) return fail(RTD_ERR_ARG, "nleg_all must be >= nleg");
  const int64_t nt_all = p->nt_request;  // > 0: the Nakajima-Tanaka inputs are formed here too (rtd_plan_request_nt)
  if (nt_all > 0) {
    if (!d.beam) return fail(RTD_ERR_ARG, "NT corrections need a beam source");
    if (band ? (nt_all != band->nleg_all || !band->delta_m) : nt_all != nleg_all)
      return fail(RTD_ERR_ARG, "request_nt: nleg_all differs from that of the columns (a band also needs delta_m)");
    if (nt_all <= d.P) return fail(RTD_ERR_ARG, "request_nt: nleg_all must be > nleg");
  }
  if (th) {
    if (d.Ns != 2) return fail(RTD_ERR_ARG, "thermal sources need a plan with nscoeffs = 2");
    if (!th->temper || !th->wvnmlo || !th->wvnmhi) return fail(RTD_ERR_ARG, "thermal: temper, wvnmlo and wvnmhi are required");
    if (th->btemp && !th->emissivity && d.NBDRF > 0 && !p->have_quad)
      return fail(RTD_ERR_STATE, "thermal: set_quadrature must precede the Kirchhoff emissivity");
  }
  const bool surf = p->surf_model >= 0;  // the BDRF tables are formed here, from the requested surface (rtd_plan_request_surface)
  if (int rc = refuse_missing_sources(d, !th && d.Ns > 0, s_poly, bdrf_q, bdrf_q0, surf)) return rc;
  if (surf) {
    if (!p->have_quad) return fail(RTD_ERR_STATE, "request_surface: set_quadrature must precede the columns");
    if (!(p->surf_rows == 1 || p->surf_rows == d.C || (band && p->surf_rows == band->nprofiles)))
      return fail(RTD_ERR_ARG, "request_surface: rows must be 1, ncols or (a band) nprofiles");
    if (d.beam)
      for (int64_t c = 0; c < d.C; ++c)
        if (!(mu0[c] > 0.0 && mu0[c] <= 1.0)) return fail(RTD_ERR_ARG, "request_surface: mu0 must lie in (0, 1] when the plan has a beam");
  }
  HIP_TRY(hipSetDevice(p->device));
  const int64_t C = d.C, L = d.L, M = d.M, N = d.N, NP = d.NP, Ns = d.Ns, NB = d.NBDRF;
  if (int rc = refuse_beam(d, I0)) return rc;
  hipStream_t s = p->stream;
  // one temporary device block for the raw arrays
  const int64_t n_cl = C * L, n_leg = C * L * nleg_all, n_b = C * M * N, n_sp = C * L * Ns;
  const bool th_bpos = th && th->btemp, th_bneg = th && th->ttemp;  // (the boundary emission is added to b_pos / b_neg, or to zero)
  const int64_t n_th = !th ? 0
                           : C * (L + 1) + 2 * C + (th->btemp ? C : 0) + (th->ttemp ? C : 0) + (th->temis ? C : 0) +
                                 (th->emissivity ? C * N : 0) + C * (L + 3) + (th_bpos && !b_pos ? n_b : 0) + (th_bneg && !b_neg ? n_b : 0);
  const int64_t bP = band ? band->nprofiles : 0, bG = band ? band->ngpoints : 0, bS = band ? band->nspecies : 0;
  const BandExtents bx = band ? band_extents(band, L, d.P) : BandExtents{};
  const int64_t n_band = bx.n_abs + 2 * bx.n_spec + bx.n_lspec;
  const int64_t nt_rows = band ? bP : C, n_mix = (nt_all > 0 && band) ? bP * L * nt_all : 0;  // a band's unweighted full moments
  const int64_t total = 3 * n_cl + n_leg + 3 * C + (b_pos ? n_b : 0) + (b_neg ? n_b : 0) + n_sp + n_th + n_band + n_mix;
  if (nt_all > 0) {  // the plan's own buffers, sized as rtd_plan_set_nt sizes them (wfull: one row per profile of a band)
    p->have_nt = false;  // (a buffer may move: on again below, once the new inputs are in place)
    if (int rc = nt_buffers(p, nt_rows, nt_all)) return rc;
  }
  // staging block from the process-wide pool (a raw hipMalloc / hipFree pair synchronises the whole device per call), and the
  // surface's scratch block (parameters, then the samples of one chunk of columns) likewise; both go back together, the staging
  // block first (owners leave in reverse order)
  Scratch surf_blk, raw_blk;
  HIP_TRY(raw_blk.get(total, p->device));
  double* raw = raw_blk.data();
  SurfLayout sl;
  if (surf) {
    surface_layout(p, &sl);
    const hipError_t es = surf_blk.get(sl.total(), p->device);
    if (es != hipSuccess) {
      (void)hipGetLastError();
      return fail(RTD_ERR_HIP, std::string("request_surface: scratch block of ") + std::to_string(sl.total() * 8) + " bytes: " + hipGetErrorString(es));
    }
  }
  RtdRaw r{};
  r.nleg_all = nleg_all;
  double* q = raw;
  hipError_t e = hipSuccess;
  auto up = [&](const double*& dst, const double* src, int64_t n) {
    dst = q;
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(q, src, (size_t)n * 8, hipMemcpyHostToDevice, s);
    q += n;
  };
  RtdBandDev bd{};
  if (band) {  // the four carves are written by the mix kernels
    bd = band_dev(band, L, d.P, q, nullptr);
    r.tau = bd.tau; r.omega = bd.omega; r.f = bd.f; r.leg = bd.leg;
    q += 3 * n_cl + n_leg;
  } else {
    up(r.tau, tau_arr, n_cl); up(r.omega, omega_arr, n_cl); up(r.f, f_arr, n_cl); up(r.leg, leg_all, n_leg);
  }
  up(r.mu0, mu0, C); up(r.I0, I0, C); up(r.phi0, phi0, C);
  if (b_pos) up(r.bpos, b_pos, n_b);
  if (b_neg) up(r.bneg, b_neg, n_b);
  RtdThermalDev t{};
  if (th) {
    auto zero = [&](const double*& dst, int64_t n) {  // an absent b_pos / b_neg that a boundary emission is added to
      dst = q;
      if (e == hipSuccess) e = hipMemsetAsync(q, 0, (size_t)n * 8, s);
      q += n;
    };
    if (th_bpos && !b_pos) zero(r.bpos, n_b);
    if (th_bneg && !b_neg) zero(r.bneg, n_b);
    r.spoly = q;
    q += n_sp;
    up(t.temper, th->temper, C * (L + 1)); up(t.lo, th->wvnmlo, C); up(t.hi, th->wvnmhi, C);
    if (th->btemp) up(t.btemp, th->btemp, C);
    if (th->ttemp) up(t.ttemp, th->ttemp, C);
    if (th->temis) up(t.temis, th->temis, C);
    if (th->emissivity) up(t.emis, th->emissivity, C * N);
    t.E = q;
    q += C * (L + 3);
    t.tau = r.tau;
    t.spoly = const_cast<double*>(r.spoly); t.bpos = const_cast<double*>(r.bpos); t.bneg = const_cast<double*>(r.bneg);
  } else if (Ns > 0) {
    up(r.spoly, s_poly, n_sp);
  }
  if (band) {
    bd = band_dev(band, L, d.P, raw, q);  // (the caller's arrays are staged here, behind the thermal carves)
    up(bd.abs, band->dtau_abs, bx.n_abs); up(bd.dspec, band->dtau_spec, bx.n_spec); up(bd.ospec, band->omega_spec, bx.n_spec);
    up(bd.lspec, band->leg_spec, bx.n_lspec);
    if (e == hipSuccess) {  // ahead of the thermal kernels, whose source slopes read the mixed tau
      band_mix_launch(bd, s);
      e = hipGetLastError();
    }
  }
  std::vector<double> qh, q0h;
  if (e == hipSuccess && surf) {  // BDRF tables from the surface model; the rows of a band's P profiles serve its G points each
    e = surface_tables(p, r.mu0, band && p->surf_rows != C ? (int)bG : 1, surf_blk.data(), sl, s);
  } else if (e == hipSuccess && NB > 0) {  // BDRF tables: padded from N to NP on the host (small)
    qh = pad_streams(bdrf_q, C * NB, true, N, NP);
    q0h = pad_streams(bdrf_q0, C * NB, false, N, NP);
    e = hipMemcpyAsync((void*)d.bdrfq, qh.data(), qh.size() * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync((void*)d.bdrfq0, q0h.data(), q0h.size() * 8, hipMemcpyHostToDevice, s);
  }
  if (e == hipSuccess && th) {  // (behind the BDRF tables and the quadrature on the plan's stream: the Kirchhoff sum reads both)
    const int64_t nE = C * (L + 3);
    hipLaunchKernelGGL(rtd_thermal_emission_kernel, grid_1d(nE), dim3(256), 0, s, d, t);
    hipLaunchKernelGGL(rtd_thermal_sources_kernel, grid_1d(C, 64), dim3(64), 0, s, d, t);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    rtd_launch_prepare(d, r, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess && nt_all > 0) {  // behind the preparation (reads the plan's mu0 and rescaled I0), before the block goes back
    RtdNtPrep np{};
    np.nleg_all = (int)nt_all; np.group = band ? (int)bG : 1; np.rows = nt_rows;
    np.tau = r.tau; np.omega = r.omega; np.f = r.f;
    np.leg = band ? q : const_cast<double*>(r.leg);
    if (band) { np.S = (int)bS; np.dspec = bd.dspec; np.ospec = bd.ospec; np.lspec = bd.lspec; }
    np.wfull = p->nt_w; np.ims_coef = p->nt_ic; np.ims_par = p->nt_ip;
    nt_prepare_launch(d, np, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(p->nt_f, r.f, (size_t)n_cl * 8, hipMemcpyDeviceToDevice, s);
  }
  if (band) {  // the host never recomputes tau: the interface detection of rtd_plan_set_eval_points compares the device's bits
    p->h_tau.resize((size_t)n_cl);
    if (e == hipSuccess) e = hipMemcpyAsync(p->h_tau.data(), r.tau, (size_t)n_cl * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && tau_out) e = hipMemcpyAsync(tau_out, r.tau, (size_t)n_cl * 8, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    if (band) p->h_tau.clear();
    return finish(e, s, "set_columns_raw");
  }
  if (!band) p->h_tau.assign(tau_arr, tau_arr + C * L);
  p->new_columns(band != nullptr);
  if (nt_all > 0) nt_bind(p, (int)nt_all, band ? (int)bG : 1, nt_rows);
  return 0;
}

int rtd_plan_set_columns_raw(rtd_plan* p, const double* tau_arr, const double* omega_arr, const double* leg_all,
                             int32_t nleg_all, const double* f_arr, const double* mu0, const double* I0,
                             const double* phi0, const double* b_pos, const double* b_neg, const double* s_poly,
                             const double* bdrf_q, const double* bdrf_q0) {
  return set_columns_raw_impl(p, tau_arr, omega_arr, leg_all, nleg_all, f_arr, mu0, I0, phi0, b_pos, b_neg, s_poly, bdrf_q, bdrf_q0,
                              nullptr);
}

int rtd_plan_set_columns_thermal(rtd_plan* p, const double* tau_arr, const double* omega_arr, const double* leg_all,
                                 int32_t nleg_all, const double* f_arr, const double* mu0, const double* I0,
                                 const double* phi0, const double* b_pos, const double* b_neg, const double* bdrf_q,
                                 const double* bdrf_q0, const rtd_thermal* th) {
  if (!th) return fail(RTD_ERR_ARG, "thermal: null description");
  return set_columns_raw_impl(p, tau_arr, omega_arr, leg_all, nleg_all, f_arr, mu0, I0, phi0, b_pos, b_neg, nullptr, bdrf_q, bdrf_q0, th);
}

int rtd_plan_set_columns_band(rtd_plan* p, const rtd_band* band, const double* mu0, const double* I0, const double* phi0,
                              const double* b_pos, const double* b_neg, const double* bdrf_q, const double* bdrf_q0,
                              const rtd_thermal* th, double* tau_out) {
  if (!p || !band) return fail(RTD_ERR_ARG, "band: null argument");
  if (!th && p->d.Ns > 0) return fail(RTD_ERR_ARG, "band: a plan with nscoeffs > 0 needs the thermal description");
  return set_columns_raw_impl(p, nullptr, nullptr, nullptr, 0, nullptr, mu0, I0, phi0, b_pos, b_neg, nullptr, bdrf_q, bdrf_q0, th, band,
                              tau_out);
}

int rtd_band_mix(int32_t device, int32_t nlayers, int32_t nleg, const rtd_band* band, double* tau_arr, double* omega_arr,
                 double* f_arr, double* leg_all) {
  if (nlayers < 1 || nleg < 1 || !tau_arr || !omega_arr || !f_arr || !leg_all) return fail(RTD_ERR_ARG, "band_mix: null argument or size < 1");
  if (const char* bad = band_bad(band, nleg)) return fail(RTD_ERR_ARG, bad);
  HIP_TRY(hipSetDevice(device));
  const BandExtents x = band_extents(band, nlayers, nleg);
  const int64_t n_cl = x.n_cl, n_leg = x.n_leg, n_abs = x.n_abs, n_spec = x.n_spec, n_lspec = x.n_lspec;
  Scratch blk;
  HIP_TRY(blk.get(3 * n_cl + n_leg + n_abs + 2 * n_spec + n_lspec, device));
  double* in = blk.data() + 3 * n_cl + n_leg;
  const RtdBandDev b = band_dev(band, nlayers, nleg, blk.data(), in);
  hipError_t e = upload_parts(in, {{band->dtau_abs, n_abs}, {band->dtau_spec, n_spec}, {band->omega_spec, n_spec}, {band->leg_spec, n_lspec}});
  if (e == hipSuccess) {
    band_mix_launch(b, (hipStream_t)0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(tau_arr, b.tau, (size_t)n_cl * 8, hipMemcpyDeviceToHost);  // (waits for the kernels)
  if (e == hipSuccess) e = hipMemcpy(omega_arr, b.omega, (size_t)n_cl * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(f_arr, b.f, (size_t)n_cl * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(leg_all, b.leg, (size_t)n_leg * 8, hipMemcpyDeviceToHost);
  return finish(e, (hipStream_t)0, "band_mix");
}

int rtd_plan_set_bdrf_samples(rtd_plan* p, int32_t nphi, const double* rho_qq, const double* rho_q0) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  p->touches_handoff();
  if (!p->have_cols) return fail(RTD_ERR_STATE, "set_columns must precede set_bdrf_samples");
  const RtdDev& d = p->d;
  if (d.NBDRF <= 0) return fail(RTD_ERR_ARG, "the plan was created with nbdrf = 0");
  if (nphi < 2 || nphi > 16384 || !rho_qq) return fail(RTD_ERR_ARG, "need 2 <= nphi <= 16384 and rho_qq");
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int64_t nqq = (int64_t)d.C * d.N * d.N * nphi, nq0 = rho_q0 ? (int64_t)d.C * d.N * nphi : 0;
  double* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, (size_t)(nqq + nq0) * sizeof(double)));
  hipError_t e = hipMemcpyAsync(tmp, rho_qq, (size_t)nqq * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess && nq0)
    e = hipMemcpyAsync(tmp + nqq, rho_q0, (size_t)nq0 * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(const_cast<double*>(d.bdrfq), 0, (size_t)d.C * d.NBDRF * d.NP * d.NP * sizeof(double), s);
  if (e == hipSuccess) e = hipMemsetAsync(const_cast<double*>(d.bdrfq0), 0, (size_t)d.C * d.NBDRF * d.NP * sizeof(double), s);
  if (e == hipSuccess) {
    rtd_launch_bdrf_modes(d, nphi, tmp, nq0 ? tmp + nqq : nullptr, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(tmp);
  if (e != hipSuccess) return fail(RTD_ERR_HIP, hipGetErrorString(e));
  p->solution_stale();
  return 0;
}

int rtd_plan_set_mode_shard(rtd_plan* p, int32_t first, int32_t stride, int32_t total) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  RtdDev& d = p->d;
  if (first < 0 || stride < 1 || total < 1 || first + (int64_t)stride * (d.M - 1) > total - 1)
    return fail(RTD_ERR_ARG, "mode shard: need 0 <= first, stride >= 1 and first + stride (nfourier - 1) <= total - 1");
  if (total > d.P) return fail(RTD_ERR_ARG, "mode shard: total number of Fourier modes exceeds nleg");
  if ((p->band_cols || p->band_G > 0) && (first != 0 || stride != 1 || total != d.M))
    return fail(RTD_ERR_STATE, "mode shard: not combined with band inputs or band weights");
  d.m0 = first;
  d.mstep = stride;
  d.mtot = total;
  p->new_mode_shard();
  return 0;
}

int rtd_plan_invalidate_tables(rtd_plan* p) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  p->fresh_tables();  // everything a fresh call would compute, the column-independent table included; as after an upload, the
  //                     next solve starts behind everything queued on the plan's stream
  return 0;
}

int rtd_plan_solve(rtd_plan* p) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (!p->have_quad || !p->have_cols) return fail(RTD_ERR_STATE, "set_quadrature and set_columns must precede solve");
  HIP_TRY(hipSetDevice(p->device));
  p->res_order = rtd_plan::RES_NONE;  // (what the result buffers hold belongs to an earlier solve)
  return launch_solve(p, false, nullptr);
}

int rtd_plan_set_eval_points(rtd_plan* p, int32_t ntau, const double* tau, int32_t nphi, const double* phi) {
  if (!p || !tau || ntau < 1 || nphi < 0 || (nphi > 0 && !phi)) return fail(RTD_ERR_ARG, "bad evaluation points");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t C = p->d.C, Qr = 2 * p->d.N;
  int rc;
  p->res_order = rtd_plan::RES_NONE;  // (the result buffers hold no evaluation at these points yet)
  if ((rc = grow(p, p->ev_tau, C * ntau))) return rc;
  if ((rc = grow(p, p->ev_phi, nphi > 0 ? nphi : 1))) return rc;
  if ((rc = grow(p, p->ev_u, C * Qr * ntau * (nphi > 0 ? nphi : 1)))) return rc;
  if ((rc = grow(p, p->ev_u0, 2 * C * Qr * ntau))) return rc;  // u0 and ulast
  if ((rc = grow(p, p->ev_fl, 3 * C * ntau))) return rc;
  if ((C * ntau + nphi) * 8 <= (int64_t)(1 << 20)) {  // small: through an image that stays with the plan, no wait
    if (p->ev_pending) HIP_TRY(hipStreamSynchronize(p->stream));
    p->ev_img.assign(tau, tau + C * ntau);
    if (nphi > 0) p->ev_img.insert(p->ev_img.end(), phi, phi + nphi);
    HIP_TRY(hipMemcpyAsync(p->ev_tau, p->ev_img.data(), (size_t)(C * ntau) * 8, hipMemcpyHostToDevice, p->stream));
    if (nphi > 0) HIP_TRY(hipMemcpyAsync(p->ev_phi, p->ev_img.data() + C * ntau, (size_t)nphi * 8, hipMemcpyHostToDevice, p->stream));
    p->ev_pending = true;
  } else {
    HIP_TRY(hipMemcpyAsync(p->ev_tau, tau, (size_t)(C * ntau) * 8, hipMemcpyHostToDevice, p->stream));
    if (nphi > 0) HIP_TRY(hipMemcpyAsync(p->ev_phi, phi, (size_t)nphi * 8, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
  }
  p->ev_ntau = ntau;
  p->ev_nphi = nphi;
  // points = the layer interfaces [0, tau_arr] of every column?  Then rtd_plan_run takes the fused evaluation.
  const int64_t L = p->d.L;
  bool iface = ntau == L + 1 && (int64_t)p->h_tau.size() == C * L;
  for (int64_t c = 0; iface && c < C; ++c) {
    const double* t = tau + c * ntau;
    iface = t[0] == 0.0 && std::memcmp(t + 1, p->h_tau.data() + c * L, (size_t)L * 8) == 0;
  }
  p->ev_iface = iface;
  if (iface && rtd_bc_fuses_eval(p->d)) {
    if ((rc = grow(p, p->um_buf, (int64_t)p->Cw * p->d.M * (L + 1) * 2 * p->d.NP))) return rc;
  }
  return 0;
}

// order: -1 the tau-antiderivative, 0 the value, +1 the tau-derivative of every output
static RtdEval make_eval(rtd_plan* p, int order, bool want_u) {
  RtdEval e{};
  const ResultShape r(p);
  e.ntau = p->ev_ntau;
  e.nphi = p->ev_nphi;
  e.antider = order < 0 ? 1 : 0;
  e.deriv = order > 0 ? 1 : 0;
  e.tau = p->ev_tau;
  e.phi = p->ev_phi;
  e.u = (want_u && p->ev_nphi > 0) ? p->ev_u.p : nullptr;
  e.u0 = p->ev_u0;
  e.ulast = p->ev_u0 + r.ulast();
  e.fup = p->ev_fl + r.flux_at(0);
  e.fdn = p->ev_fl + r.flux_at(1);
  e.fdir = p->ev_fl + r.flux_at(2);
  return e;
}

int rtd_plan_run(rtd_plan* p) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (!p->have_quad || !p->have_cols || p->ev_ntau < 1) return fail(RTD_ERR_STATE, "inputs or evaluation points missing");
  HIP_TRY(hipSetDevice(p->device));
  RtdEval e = make_eval(p, p->eval_order, true);
  int rc = launch_solve(p, true, &e, p->have_nt);
  p->res_order = rc ? rtd_plan::RES_NONE : p->eval_order;
  p->res_has_u = e.u != nullptr;
  return rc;
}

int rtd_plan_set_eval_order(rtd_plan* p, int32_t order) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (order < -1 || order > 1) return fail(RTD_ERR_ARG, "evaluation order must be -1, 0 or +1");
  p->eval_order = order;
  return 0;
}

// out[p][k][e] = sum_g w[k][g] X[p G + g][e] on the plan's stream (rtd_band_reduce_kernel), then the copy of `out` to the host
static hipError_t band_reduce(rtd_plan* p, const double* X, int mask, int64_t E, double* out, double* host) {
  const int64_t G = p->band_G, K = p->band_K, P = p->d.C / G;
  hipLaunchKernelGGL(rtd_band_reduce_kernel, grid_1d(P * E), dim3(256), 0, p->stream, X, (const double*)p->band_w,
                     (const int*)p->d.col_status, mask, (long)P, (int)G, (int)K, (long)E, out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host, out, (size_t)(P * K * E) * 8, hipMemcpyDeviceToHost, p->stream);
  return e;
}

// One output of a fetch, and the list of them that a call asks for.  Every fetch is a builder of such a list and one of two sinks:
// copy_out takes each array as it lies, reduce_out (under band weights) its sum over the spectral points [P][K][per].
//   builder            product          dev                  per          mask    reduced (slice of)
//   result_products    u                ev_u                 Q ntau nphi  0xFFFF  rb_u
//                      u0               ev_u0                Q ntau       0xFF    rb_u0
//                      flux f = 0,1,2   ev_fl + f C ntau     ntau         0xFF    rb_fl (f of 3)
//   actinic_products   f = 0, 1, 2      ev_act + f C ntau    ntau         0xFF    rb_act (f of 3)
//   view_products      u_mu             ev_view_u            nmu ntau nphi 0xFFFF rb_view_u
//                      u0_mu            ev_view_u0           nmu ntau     0xFF    rb_view_u0
// mask: the bits of col_status that spoil the output -- every Fourier mode for u, mode 0 alone for u0 and the fluxes.  The list lives
// on the caller's stack (rtd_plan_evaluate of one column comes through here: no allocation).
struct Product {
  double* host;       // the caller's array
  const double* dev;  // where it lies on the device, all columns
  int64_t per;        // doubles per column
  int mask;
  DevBuf* reduced;    // the band form's buffer, `nslices` arrays [P][K][per] of which this product is number `slice`
  int slice, nslices;
};
struct Products {
  Product v[6];
  int n = 0;
  bool all_modes = false;  // u was asked for (also where it has no extent, without azimuths): a failure in the modes m > 0 is the call's
  void add(double* host, const double* dev, int64_t per, int mask, DevBuf* reduced, int slice = 0, int nslices = 1) {
    if (host && per > 0) v[n++] = {host, dev, per, mask, reduced, slice, nslices};
  }
};
// mode0: the list of a Lambertian companion -- the same outputs, each at its counterpart of Fourier mode 0 (u0 for u)
static void result_products(rtd_plan* p, double* u, double* u0, double* flux_up, double* fdn, double* fdir, Products* xs, bool mode0 = false) {
  const ResultShape r(p);
  xs->add(u, mode0 ? p->ev_u0 : p->ev_u, mode0 ? r.per_column_u0() : r.per_column_u(), 0xFFFF, &p->rb_u);
  xs->add(u0, p->ev_u0, r.per_column_u0(), 0xFF, &p->rb_u0);
  double* fls[3] = {flux_up, fdn, fdir};
  for (int f = 0; f < 3; ++f) xs->add(fls[f], p->ev_fl + r.flux_at(f), r.nt, 0xFF, &p->rb_fl, f, 3);
  xs->all_modes = xs->all_modes || u != nullptr;
}
static void actinic_products(rtd_plan* p, double* up, double* dn, double* dir, Products* xs) {
  const ResultShape r(p);
  double* outs[3] = {up, dn, dir};
  for (int f = 0; f < 3; ++f) xs->add(outs[f], p->ev_act + r.flux_at(f), r.nt, 0xFF, &p->rb_act, f, 3);
}
static void view_products(rtd_plan* p, double* u_mu, double* u0_mu, Products* xs, bool mode0 = false) {
  const ResultShape r(p);
  const int64_t nmu = p->view_nmu;
  xs->add(u_mu, mode0 ? p->ev_view_u0 : p->ev_view_u, nmu * r.nt * (mode0 ? 1 : r.np), 0xFFFF, &p->rb_view_u);
  xs->add(u0_mu, p->ev_view_u0, nmu * r.nt, 0xFF, &p->rb_view_u0);
  xs->all_modes = xs->all_modes || u_mu != nullptr;
}
// the device-to-host copies of the list on the plan's stream, then the status check (which drains the stream)
static int copy_out(rtd_plan* p, const Products& xs) {
  for (int i = 0; i < xs.n; ++i)
    HIP_TRY(hipMemcpyAsync(xs.v[i].host, xs.v[i].dev, (size_t)(p->d.C * xs.v[i].per) * 8, hipMemcpyDeviceToHost, p->stream));
  return check_status(p, xs.all_modes);
}
// the list reduced over the spectral points: every reduced buffer is grown before the first launch; each product is reduced and
// copied out behind it (band_reduce); then the status check
static int reduce_out(rtd_plan* p, const Products& xs, const char* label) {
  const int64_t PK = band_rows(p);
  int rc;
  for (int i = 0; i < xs.n; ++i)
    if ((rc = grow(p, *xs.v[i].reduced, xs.v[i].nslices * PK * xs.v[i].per))) return rc;
  (void)hipGetLastError();
  for (int i = 0; i < xs.n; ++i) {
    const Product& x = xs.v[i];
    const hipError_t e = band_reduce(p, x.dev, x.mask, x.per, x.reduced->p + x.slice * PK * x.per, x.host);
    if (e != hipSuccess) return fail(RTD_ERR_HIP, std::string(label) + ": " + hipGetErrorString(e));
  }
  return check_status(p, xs.all_modes);
}
// band_label: the name of the band form in the message of a failed reduction; null: the plain form
static int deliver(rtd_plan* p, const Products& xs, const char* band_label) { return band_label ? reduce_out(p, xs, band_label) : copy_out(p, xs); }

// the results at the stored points, as they lie or (band_label) reduced over the spectral points
static int fetch_queued(rtd_plan* p, double* u, double* u0, double* flux_up, double* fdn, double* fdir, const char* band_label = nullptr) {
  HIP_TRY(hipSetDevice(p->device));
  Products xs;
  result_products(p, u, u0, flux_up, fdn, fdir, &xs);
  return deliver(p, xs, band_label);
}

// Whatever goes wrong, no copy into the caller's (pageable) arrays is left in flight behind the return: the caller may free or
// reuse them at once.  check_status drains the stream on its own way out; the early returns before it do not.
static int drained(rtd_plan* p, int rc) {
  if (rc != 0 && p->stream) {
    const std::string keep = g_err;
    (void)hipStreamSynchronize(p->stream);
    g_err = keep;
  }
  return rc;
}

int rtd_plan_fetch(rtd_plan* p, double* u, double* u0, double* flux_up, double* fdn, double* fdir) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (!has_results(p, false)) return fail(RTD_ERR_STATE, "nothing to fetch");
  return drained(p, fetch_queued(p, u, u0, flux_up, fdn, fdir));
}

// solve + evaluate + copy out, window by window: the device-to-host copy of window w (copy stream, pinned staging)
// and the host memcpy into the caller's arrays overlap the kernels of window w + 1
int rtd_plan_run_fetch(rtd_plan* p, double* u, double* u0, double* flux_up, double* fdn, double* fdir) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (!p->have_quad || !p->have_cols || p->ev_ntau < 1) return fail(RTD_ERR_STATE, "inputs or evaluation points missing");
  HIP_TRY(hipSetDevice(p->device));
  const ResultShape r(p);
  Products xs;  // the arrays the caller wants: where each goes, where it lies on the device, its doubles per column
  result_products(p, u, u0, flux_up, fdn, fdir, &xs);
  int64_t per_column = 0;
  for (int k = 0; k < xs.n; ++k) per_column += xs.v[k].per;
  const size_t slab = (size_t)p->Cw * (size_t)per_column * 8;
  int rc;
  if (!p->copy_stream && (rc = acquire_stream(p->device, &p->copy_stream))) return rc;
  for (int k = 0; k < 2; ++k)
    if ((rc = ensure_event(&p->ev_win[k])) || (rc = ensure_event(&p->ev_copied[k]))) return rc;
  if (slab > p->stage_bytes) {
    for (int k = 0; k < 2; ++k) {
      char*& st = p->stage[k];
      if (st && !pool().put_host(st, p->stage_cap[k])) (void)hipHostFree(st);
      st = static_cast<char*>(pool().get_host(slab, &p->stage_cap[k]));
      if (!st) HIP_TRY(hipHostMalloc((void**)&st, p->stage_cap[k] = slab, hipHostMallocDefault));
    }
    p->stage_bytes = slab;
  }
  // host side of window w: wait for its copy, scatter the staging slab into the caller's arrays
  auto drain = [&](int w) -> int {
    const int64_t c0 = (int64_t)w * p->Cw, cnt = std::min<int64_t>(p->Cw, r.C - c0);
    HIP_TRY(hipEventSynchronize(p->ev_copied[w & 1]));
    const char* src = p->stage[w & 1];
    for (int k = 0; k < xs.n; src += cnt * xs.v[k].per * 8, ++k)
      std::memcpy(xs.v[k].host + c0 * xs.v[k].per, src, (size_t)(cnt * xs.v[k].per) * 8);
    return 0;
  };
  RtdEval e = make_eval(p, p->eval_order, true);
  p->res_order = rtd_plan::RES_NONE;
  rc = launch_windows(p, true, &e, p->have_nt, [&](int w, int64_t c0, int cnt) -> int {
    const int k = w & 1;
    if (w >= 2) {  // the slab of window w - 2 must have been drained before it is overwritten
      int r = drain(w - 2);
      if (r) return r;
    }
    HIP_TRY(hipEventRecord(p->ev_win[k], p->stream));
    HIP_TRY(hipStreamWaitEvent(p->copy_stream, p->ev_win[k], 0));
    char* dst = p->stage[k];
    hipStream_t cs = p->copy_stream;
    for (int i = 0; i < xs.n; dst += cnt * xs.v[i].per * 8, ++i)
      HIP_TRY(hipMemcpyAsync(dst, xs.v[i].dev + c0 * xs.v[i].per, (size_t)(cnt * xs.v[i].per) * 8, hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipEventRecord(p->ev_copied[k], cs));
    return 0;
  });
  if (rc) return rc;
  for (int w = std::max(0, p->nwin - 2); w < p->nwin; ++w)
    if ((rc = drain(w))) return rc;
  p->res_order = p->eval_order;
  p->res_has_u = e.u != nullptr;
  return check_status(p, xs.all_modes);
}

int rtd_plan_result_dev_ptrs(rtd_plan* p, void** u_dev, int64_t* u_bytes, void** flux_dev, int64_t* flux_bytes) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  const ResultShape r(p);
  if (u_dev) *u_dev = p->ev_u;
  if (u_bytes) *u_bytes = r.u() * 8;
  if (flux_dev) *flux_dev = p->ev_fl;
  if (flux_bytes) *flux_bytes = r.fl() * 8;
  return 0;
}

// the evaluation of rtd_plan_evaluate / rtd_plan_evaluate_band into the plan's result buffers, queued on the plan's stream
static int evaluate_queued(rtd_plan* p, int32_t ntau, const double* tau, int32_t nphi, const double* phi, int32_t antiderivative,
                           bool want_u) {
  if (!p->solved) return fail(RTD_ERR_STATE, "evaluate before solve");
  if ((antiderivative & 1) && (antiderivative & 4)) return fail(RTD_ERR_ARG, "antiderivative (bit 0) and derivative (bit 2) exclude each other");
  int rc = rtd_plan_set_eval_points(p, ntau, tau, nphi, phi);
  if (rc) return rc;
  const bool skip_nt = (antiderivative & 2) != 0;
  const int order = (antiderivative & 1) ? -1 : (antiderivative & 4) ? 1 : 0;
  RtdEval e = make_eval(p, order, want_u);
  // one window, or a retained plan (rtd_plan_create_retained): what the evaluators need of the solve is resident for every
  // column, only the evaluation kernels run.  Several windows without retention: they are solved again, window by window,
  // with the evaluation behind each (the throughput form rtd_plan_run is the intended entry point for such batches).
  const bool solve_again = p->nwin > 1 && !p->retained && !p->lean;
  rc = launch_windows(p, solve_again, &e, p->have_nt && !skip_nt, [](int, int64_t, int) { return 0; }, false);
  if (rc) return rc;
  if (p->pipelined && !solve_again) p->fork_needed = true;  // the next solve's eigen stream must not overwrite what this pass still reads
  p->res_order = order;
  p->res_has_u = e.u != nullptr;
  return 0;
}

int rtd_plan_evaluate(rtd_plan* p, int32_t ntau, const double* tau, int32_t nphi, const double* phi,
                      int32_t antiderivative, double* u, double* u0, double* flux_up, double* fdn, double* fdir,
                      double* ulast) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  int rc = evaluate_queued(p, ntau, tau, nphi, phi, antiderivative, u != nullptr || (antiderivative & 8) != 0);
  if (rc) return rc;
  if (ulast) {  // queued before the fetch, whose status check drains the stream: a numerical failure of SOME columns must not
    //             leave the healthy columns' ulast unwritten (numeric_errors = "nan" keeps them)
    const ResultShape r(p);  // (at the points evaluate_queued has just stored)
    hipError_t he = hipMemcpyAsync(ulast, p->ev_u0 + r.ulast(), (size_t)r.u0() * 8, hipMemcpyDeviceToHost, p->stream);
    if (he != hipSuccess) return drained(p, fail(RTD_ERR_HIP, std::string("hipMemcpyAsync(ulast): ") + hipGetErrorString(he)));
  }
  return drained(p, rtd_plan_fetch(p, u, u0, flux_up, fdn, fdir));  // (also behind fetch's own early returns: the ulast copy is pending)
}

int rtd_plan_set_band_weights(rtd_plan* p, int32_t G, int32_t K, const double* w) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (G <= 0) {  // switch the reduction off
    p->band_G = p->band_K = 0;
    return 0;
  }
  if (K < 1 || !w || p->d.C % G != 0) return fail(RTD_ERR_ARG, "band weights: need nsets >= 1, weights and ncols % ngpoints == 0");
  if (sharded(p)) return fail(RTD_ERR_STATE, "band weights are not combined with a mode shard or a communicator");
  HIP_TRY(hipSetDevice(p->device));
  int rc = grow(p, p->band_w, (int64_t)K * G);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(p->band_w, w, (size_t)K * G * 8, hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));  // the caller's array must outlive its copy
  p->band_G = G;
  p->band_K = K;
  return 0;
}

int rtd_plan_fetch_band(rtd_plan* p, double* u, double* u0, double* flux_up, double* fdn, double* fdir) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (p->band_G <= 0) return fail(RTD_ERR_STATE, "set_band_weights must precede fetch_band");
  if (!has_results(p, false)) return fail(RTD_ERR_STATE, "nothing to fetch");
  return drained(p, fetch_queued(p, u, u0, flux_up, fdn, fdir, "fetch_band"));
}

int rtd_plan_evaluate_band(rtd_plan* p, int32_t ntau, const double* tau, int32_t nphi, const double* phi, int32_t flags, double* u,
                           double* u0, double* flux_up, double* fdn, double* fdir) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (p->band_G <= 0) return fail(RTD_ERR_STATE, "set_band_weights must precede evaluate_band");
  int rc = evaluate_queued(p, ntau, tau, nphi, phi, flags, u != nullptr || (flags & 8) != 0);
  if (rc) return rc;
  return drained(p, fetch_queued(p, u, u0, flux_up, fdn, fdir, "fetch_band"));
}

// rtd_actinic_kernel over all columns into ev_act, on the plan's stream: everything it reads is held for all columns
static int actinic_queued(rtd_plan* p) {
  HIP_TRY(hipSetDevice(p->device));
  const int64_t CT = (int64_t)p->d.C * p->ev_ntau;
  int rc = grow(p, p->ev_act, 3 * CT);
  if (rc) return rc;
  (void)hipGetLastError();
  hipLaunchKernelGGL(rtd_actinic_kernel, grid_1d(CT), dim3(256), 0, p->stream, p->d, (const double*)p->ev_tau,
                     (const double*)p->ev_u0, (int)p->ev_ntau, (int)p->res_order, p->ev_act);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RTD_ERR_HIP, std::string("rtd_actinic_kernel: ") + hipGetErrorString(e));
  return 0;
}

static int actinic_fetch_queued(rtd_plan* p, double* up, double* dn, double* dir, const char* band_label = nullptr) {
  int rc = actinic_queued(p);
  if (rc) return rc;
  if (band_label && (rc = grow(p, p->rb_act, 3 * band_rows(p) * p->ev_ntau))) return rc;  // (also when no output is asked for, as ever)
  Products xs;  // (all_modes stays false: u0 comes from Fourier mode 0 alone)
  actinic_products(p, up, dn, dir, &xs);
  return deliver(p, xs, band_label);
}

int rtd_plan_fetch_actinic(rtd_plan* p, double* act_up, double* act_down_diffuse, double* act_down_direct) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (!has_results(p, true)) return fail(RTD_ERR_STATE, "nothing to fetch");
  return drained(p, actinic_fetch_queued(p, act_up, act_down_diffuse, act_down_direct));
}

int rtd_plan_fetch_band_actinic(rtd_plan* p, double* act_up, double* act_down_diffuse, double* act_down_direct) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (p->band_G <= 0) return fail(RTD_ERR_STATE, "set_band_weights must precede fetch_band_actinic");
  if (!has_results(p, true)) return fail(RTD_ERR_STATE, "nothing to fetch");
  return drained(p, actinic_fetch_queued(p, act_up, act_down_diffuse, act_down_direct, "fetch_band_actinic"));
}

// the barycentric weights b_j = 1 / prod_{k != j} (x_j - x_k) of the plan's positive nodes: long double, k ascending, scaled by
// the largest magnitude and rounded once (64 nodes: about 38 decades between the smallest and the largest, which float64 holds)
static std::vector<double> view_weights(const std::vector<double>& x) {
  const size_t N = x.size();
  std::vector<long double> b(N);
  long double big = 0.0L;
  for (size_t j = 0; j < N; ++j) {
    long double prod = 1.0L;
    for (size_t k = 0; k < N; ++k)
      if (k != j) prod *= (long double)x[j] - (long double)x[k];
    b[j] = 1.0L / prod;
    big = std::max(big, std::fabs(b[j]));
  }
  std::vector<double> out(N);
  for (size_t j = 0; j < N; ++j) out[j] = (double)(b[j] / big);
  return out;
}

// per-column angles under band weights: the G columns of a profile must carry identical angles (their interpolants are summed)
static bool view_band_consistent(const rtd_plan* p) {
  if (!p->view_per_column || p->view_nmu <= 0 || p->band_G <= 1) return true;
  const int64_t G = p->band_G, nmu = p->view_nmu;
  for (int64_t c = 0; c < p->d.C; ++c)
    if (c % G != 0 && std::memcmp(&p->view_mu_h[c * nmu], &p->view_mu_h[(c - c % G) * nmu], (size_t)nmu * 8) != 0) return false;
  return true;
}

// mu = +-0.0 has no corrections of its own (the plane-parallel limit differs by hemisphere): refused in rtd_plan_set_view_nt's mode 1
static const char* const VIEW_NT_ZERO = "mu = 0 is not accepted with the corrections at the angles (set_view_nt): the limit differs by hemisphere";
static bool view_has_zero(const double* mu, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (mu[i] == 0.0) return true;
  return false;
}

int rtd_plan_set_view_mu(rtd_plan* p, int32_t nmu, const double* mu, int32_t per_column) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (nmu <= 0) {  // withdraw the request (the buffers, if any, stay with the plan)
    p->view_nmu = 0;
    p->view_mu_h.clear();
    p->view_stale = true;
    p->view_u_resident = false;
    return 0;
  }
  if (!mu) return fail(RTD_ERR_ARG, "set_view_mu: null angles");
  if (!p->have_quad) return fail(RTD_ERR_STATE, "set_quadrature must precede set_view_mu");
  const int64_t n = (per_column ? (int64_t)p->d.C : 1) * nmu;
  for (int64_t i = 0; i < n; ++i)
    if (!(std::fabs(mu[i]) <= 1.0)) return fail(RTD_ERR_ARG, "mu values must be between -1 and 1");
  if (p->view_nt_mode == 1 && view_has_zero(mu, n)) return fail(RTD_ERR_ARG, VIEW_NT_ZERO);
  std::vector<double> keep(mu, mu + n);
  std::swap(keep, p->view_mu_h);
  const int old_nmu = p->view_nmu;
  const bool old_pc = p->view_per_column;
  p->view_nmu = nmu;
  p->view_per_column = per_column != 0;
  if (!view_band_consistent(p)) {  // refused: the earlier request stands
    std::swap(keep, p->view_mu_h);
    p->view_nmu = old_nmu;
    p->view_per_column = old_pc;
    return fail(RTD_ERR_ARG, "set_view_mu: the columns of a band profile must carry identical angles");
  }
  p->view_stale = true;
  p->view_u_resident = false;  // (the next evaluation forms the view of u at the new angles; until then view_refused says so)
  return 0;
}

int rtd_plan_set_view_nt(rtd_plan* p, int32_t mode) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (mode != 0 && mode != 1) return fail(RTD_ERR_ARG, "set_view_nt: the mode must be 0 (interpolated) or 1 (at the angles)");
  if (mode == 1 && view_has_zero(p->view_mu_h.data(), (int64_t)p->view_mu_h.size())) return fail(RTD_ERR_ARG, VIEW_NT_ZERO);
  if (mode != p->view_nt_mode) p->view_u_resident = false;
  p->view_nt_mode = mode;
  return 0;
}

// The basis of the requested angles when the device's copy is stale, on the plan's stream.  Every fetch drains the stream before it
// returns, so no copy reads view_mu_h when set_view_mu next replaces it.
static int view_basis_queued(rtd_plan* p) {
  HIP_TRY(hipSetDevice(p->device));
  const int64_t N = p->d.N, nmu = p->view_nmu, rows = p->view_per_column ? p->d.C : 1, n = rows * nmu;
  int rc;
  (void)hipGetLastError();
  if (p->view_stale) {
    if ((rc = grow(p, p->view_mu, n)) || (rc = grow(p, p->view_b, N)) || (rc = grow(p, p->view_l, n * N)) ||
        (rc = grow(p, p->view_flag, (n + 1) / 2 + 1)))
      return rc;
    const std::vector<double> b = view_weights(p->h_mu_pos);
    HIP_TRY(hipMemcpyAsync(p->view_mu, p->view_mu_h.data(), (size_t)n * 8, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(p->view_b, b.data(), (size_t)N * 8, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));  // (b is a local; the basis is formed once per request, not per fetch)
    int* flag = reinterpret_cast<int*>(p->view_flag.p);
    hipLaunchKernelGGL(rtd_view_basis_kernel, grid_1d(n), dim3(256), 0, p->stream, (const double*)p->view_mu, (long)n,
                       (const double*)p->d.mu, (const double*)p->view_b, (int)N, p->view_l.p, flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RTD_ERR_HIP, std::string("rtd_view_basis_kernel: ") + hipGetErrorString(e));
    p->view_stale = false;
  }
  return 0;
}

// out [c0 .. c0 + cnt)[nmu][E] = the interpolant of X [cnt][2N][E], the results of those columns (X points at the first of them)
static int view_apply_queued(rtd_plan* p, const double* X, int64_t E, int64_t c0, int64_t cnt, double* out) {
  const int64_t N = p->d.N, nmu = p->view_nmu, total = cnt * nmu * E;
  const long ls = p->view_per_column ? (long)(nmu * N) : 0, fs = p->view_per_column ? (long)nmu : 0;
  const int* flag = reinterpret_cast<const int*>(p->view_flag.p);
  hipLaunchKernelGGL(rtd_view_apply_kernel, grid_1d(total), dim3(256), 0, p->stream, (const double*)p->view_l + c0 * ls, ls,
                     flag + c0 * fs, fs, X, (int)N, (int)nmu, (long)E, (long)cnt, out + c0 * nmu * E);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RTD_ERR_HIP, std::string("rtd_view_apply_kernel: ") + hipGetErrorString(e));
  return 0;
}

// the basis (when stale) and the interpolation of the resident results into ev_view_u / ev_view_u0, on the plan's stream.  The view of u
// that an evaluation formed itself (rtd_plan_set_view_nt, mode 1: view_refused has seen that it is resident) is left as it is.
static int view_queued(rtd_plan* p, bool want_u, bool want_u0) {
  int rc = view_basis_queued(p);
  if (rc) return rc;
  const ResultShape r(p);
  struct Pass { bool on; const double* X; int64_t E; DevBuf* out; } pass[2] = {{want_u && !p->view_u_resident, p->ev_u, r.nt * r.np, &p->ev_view_u},
                                                                              {want_u0, p->ev_u0, r.nt, &p->ev_view_u0}};
  for (const Pass& q : pass) {
    if (!q.on) continue;
    if ((rc = grow(p, *q.out, r.C * p->view_nmu * q.E))) return rc;
    if ((rc = view_apply_queued(p, q.X, q.E, 0, r.C, q.out->p))) return rc;
  }
  return 0;
}

// what rtd_plan_fetch_view and rtd_plan_fetch_band_view refuse alike
static int view_refused(rtd_plan* p, const double* u_mu) {
  if (p->view_nmu <= 0) return fail(RTD_ERR_STATE, "set_view_mu must precede fetch_view");
  if (!has_results(p, true)) return fail(RTD_ERR_STATE, "nothing to fetch");
  if (u_mu && !p->res_has_u) return fail(RTD_ERR_STATE, "fetch_view: the latest evaluation formed no u (no azimuths, or u was not wanted)");
  if (u_mu && p->view_nt_mode == 1 && p->res_nt && !p->view_u_resident)
    return fail(RTD_ERR_STATE, "fetch_view: with the corrections at the angles (set_view_nt) the view of u is formed by the evaluation, and the "
                               "angles or the mode were set after the latest one: evaluate again");
  return 0;
}

static int view_fetch_queued(rtd_plan* p, double* u_mu, double* u0_mu, const char* band_label = nullptr) {
  int rc = view_queued(p, u_mu != nullptr, u0_mu != nullptr);
  if (rc) return rc;
  Products xs;
  view_products(p, u_mu, u0_mu, &xs);
  return deliver(p, xs, band_label);
}

int rtd_plan_fetch_view(rtd_plan* p, double* u_mu, double* u0_mu) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  int rc = view_refused(p, u_mu);
  if (rc) return rc;
  return drained(p, view_fetch_queued(p, u_mu, u0_mu));
}

int rtd_plan_fetch_band_view(rtd_plan* p, double* u_mu, double* u0_mu) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (p->band_G <= 0) return fail(RTD_ERR_STATE, "set_band_weights must precede fetch_band_view");
  int rc = view_refused(p, u_mu);
  if (rc) return rc;
  if (!view_band_consistent(p)) return fail(RTD_ERR_ARG, "fetch_band_view: the columns of a band profile must carry identical angles");
  return drained(p, view_fetch_queued(p, u_mu, u0_mu, "fetch_band_view"));
}

// ---- Lambertian albedo sweeps (rtd_plan_couple_lambert, rtd_plan_couple_lambert_band; kernels rtd_lambert.hip) ------------------------

// what the two entry points and the plan-free rtd_lambert_kappa refuse of the caller's arrays: rows_ok lists the admissible albedo_rows
static int lambert_args_refused(int64_t C, int32_t nalb, const double* albedo, int64_t rows, const int64_t* rows_ok, int nrows_ok,
                                const double* fdown, const double* sph, const double* emission) {
  if (nalb < 1) return fail(RTD_ERR_ARG, "couple_lambert: nalb must be at least 1");
  if (!albedo || !fdown || !sph) return fail(RTD_ERR_ARG, "couple_lambert: null albedo, fdown_bottom or sph_albedo");
  bool ok = false;
  for (int i = 0; i < nrows_ok; ++i) ok = ok || (rows >= 1 && rows == rows_ok[i]);
  if (!ok) return fail(RTD_ERR_ARG, "couple_lambert: albedo_rows must be 1 or the number of columns (a band: or of profiles)");
  for (int64_t i = 0; i < rows * nalb; ++i)
    if (!(albedo[i] >= 0.0 && albedo[i] <= 1.0)) return fail(RTD_ERR_ARG, "couple_lambert: an albedo must lie in [0, 1] (row " + std::to_string(i / nalb) + ")");
  if (emission)
    for (int64_t c = 0; c < C; ++c)
      if (!(emission[c] >= 0.0 && std::isfinite(emission[c])))
        return fail(RTD_ERR_ARG, "couple_lambert: the emission must be finite and not negative (column " + std::to_string(c) + ")");
  return 0;
}

// the RTD_ERR_STATE cases of the two entry points
static int lambert_state_refused(rtd_plan* a, rtd_plan* b, bool want_u, const double* u_mu, const double* u0_mu) {
  if (a->d.C != b->d.C || a->d.L != b->d.L || a->d.N != b->d.N || a->device != b->device)
    return fail(RTD_ERR_STATE, "couple_lambert: the two plans differ in columns, layers, streams or device");
  if (b->d.M != 1 || b->d.beam || b->d.Ns != 0 || b->d.NBDRF != 0)
    return fail(RTD_ERR_STATE, "couple_lambert: the companion must have one Fourier mode, no beam, no isotropic source and no BDRF");
  if (a->d.NBDRF != 0) return fail(RTD_ERR_STATE, "couple_lambert: the primary must be solved over a black surface (nbdrf = 0)");
  if (sharded(a) || sharded(b)) return fail(RTD_ERR_STATE, "couple_lambert is not combined with a mode shard or a communicator");
  for (const rtd_plan* p : {a, b})
    if (!has_results(p, true)) return fail(RTD_ERR_STATE, "couple_lambert: nothing to couple (a plan holds no evaluated results)");
  if (a->ev_ntau != b->ev_ntau || a->res_order != b->res_order)
    return fail(RTD_ERR_STATE, "couple_lambert: the two plans were evaluated at different numbers of points or in different tau-orders");
  if (want_u && !a->res_has_u) return fail(RTD_ERR_STATE, "couple_lambert: the primary's latest evaluation formed no u (no azimuths, or u was not wanted)");
  if (u_mu || u0_mu) {
    if (a->view_nmu <= 0 || b->view_nmu <= 0) return fail(RTD_ERR_STATE, "couple_lambert: set_view_mu must precede the view outputs, on both plans");
    if (a->view_nmu != b->view_nmu) return fail(RTD_ERR_STATE, "couple_lambert: the two plans hold different numbers of viewing angles");
    int rc = view_refused(a, u_mu);
    if (rc) return rc;
  }
  return 0;
}

// Everything behind the refusals, on the primary's stream.  A block from the pool holds the caller's small arrays, kappa [C][A], the
// column flags and the coupled arrays of one chunk of columns -- for a band of whole profiles, with their reduced arrays behind them;
// output after output, chunk after chunk is coupled (reduced) there and copied out.  Nothing stays with either plan.
static int lambert_queued(rtd_plan* a, rtd_plan* b, int32_t nalb, const double* albedo, int64_t rows, const double* fdown, const double* sph,
                          const double* emission, double* u, double* u0, double* fup, double* fdn, double* u_mu, double* u0_mu, bool band) {
  HIP_TRY(hipSetDevice(a->device));
  int rc;
  if (u_mu || u0_mu) {  // the views of the resident results, each on its own plan's stream
    if ((rc = view_queued(a, u_mu != nullptr, u0_mu != nullptr)) || (rc = view_queued(b, false, true))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(b->stream));  // (the companion's evaluation and view must have landed before the primary's stream reads them)
  b->stream_drained();
  const int64_t C = a->d.C, G = band ? a->band_G : 1, K = band ? a->band_K : 0, NA = nalb;
  // the primary's outputs X and, entry for entry, the companion's mode-0 terms Y: E doubles per column of X, E / nrep of Y
  Products xs, ys;
  result_products(a, u, u0, fup, fdn, nullptr, &xs);
  result_products(b, u, u0, fup, fdn, nullptr, &ys, true);
  view_products(a, u_mu, u0_mu, &xs);
  view_products(b, u_mu, u0_mu, &ys, true);
  // columns per chunk of an output: as many as fit the budget, one column (a band: one profile) at least
  const int64_t budget = budget_doubles(getenv("RTD_LAMBERT_BYTES"));
  auto chunk_of = [&](const Product& x) { return G * columns_per_chunk(budget, (G + K) * NA * x.per, C / G); };
  int64_t work = 0;
  for (int i = 0; i < xs.n; ++i) work = std::max(work, chunk_of(xs.v[i]) / G * (G + K) * NA * xs.v[i].per);
  const int64_t n_alb = rows * NA, n_small = n_alb + 3 * C + C * NA + (C + 1) / 2 + 1;
  Scratch blk;
  HIP_TRY(blk.get(n_small + work, a->device));
  double *d_alb = blk.data(), *d_f = d_alb + n_alb, *d_s = d_f + C, *d_e = d_s + C, *d_k = d_e + C, *d_work = d_alb + n_small;
  int* d_flag = reinterpret_cast<int*>(d_k + C * NA);
  hipStream_t st = a->stream;
  (void)hipGetLastError();
  hipError_t e = hipMemcpyAsync(d_alb, albedo, (size_t)n_alb * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_f, fdown, (size_t)C * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_s, sph, (size_t)C * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && emission) e = hipMemcpyAsync(d_e, emission, (size_t)C * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    rtd_launch_lambert_kappa(d_alb, (long)(C / rows), nalb, d_f, d_s, emission ? d_e : nullptr, a->d.col_status, b->d.col_status, (long)C, d_k,
                             d_flag, st);
    e = hipGetLastError();
  }
  for (int i = 0; i < xs.n && e == hipSuccess; ++i) {
    const Product &x = xs.v[i], &y = ys.v[i];
    const bool every_mode = x.mask == 0xFFFF;  // u and its view: every azimuth of X takes the same element of Y, and Y's bits 0 ... 2 spoil
    const int64_t E = x.per, per = NA * E, chunk = chunk_of(x);
    for (int64_t c0 = 0; c0 < C && e == hipSuccess; c0 += chunk) {
      const int64_t cnt = std::min(chunk, C - c0);
      rtd_launch_lambert_couple(x.dev + c0 * E, y.dev + c0 * y.per, d_k + c0 * NA, d_flag + c0, every_mode ? 7 : 3, (long)cnt, nalb, (long)E,
                                (int)(E / y.per), d_work, st);
      e = hipGetLastError();
      if (e != hipSuccess) break;
      if (!band) {
        e = hipMemcpyAsync(x.host + c0 * per, d_work, (size_t)(cnt * per) * 8, hipMemcpyDeviceToHost, st);
      } else {  // the chunk's profiles reduced over g behind the coupled arrays, with the primary's weights
        const int64_t P = cnt / G;
        double* red = d_work + cnt * per;
        hipLaunchKernelGGL(rtd_band_reduce_kernel, grid_1d(P * per), dim3(256), 0, st, (const double*)d_work,
                           (const double*)a->band_w, (const int*)a->d.col_status + c0, x.mask, (long)P, (int)G, (int)K, (long)per, red);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(x.host + (c0 / G) * K * per, red, (size_t)(P * K * per) * 8, hipMemcpyDeviceToHost, st);
      }
    }
  }
  if (e != hipSuccess) return finish(e, st, "couple_lambert");
  rc = check_status(a, xs.all_modes);  // (drains the primary's stream: the block is free behind it)
  const std::string keep = g_err;
  const int rc_b = check_status(b, false);
  if (rc) g_err = keep;
  return rc ? rc : rc_b;
}

static int lambert_entry(rtd_plan* a, rtd_plan* b, int32_t nalb, const double* albedo, int32_t rows, const double* fdown, const double* sph,
                         const double* emission, double* u, double* u0, double* fup, double* fdn, double* u_mu, double* u0_mu, bool band) {
  if (!a || !b) return fail(RTD_ERR_ARG, "null plan");
  const int64_t C = a->d.C;
  if (band && a->band_G <= 0) return fail(RTD_ERR_STATE, "set_band_weights must precede couple_lambert_band");
  const int64_t rows_ok[3] = {1, C, band ? C / a->band_G : 1};
  int rc = lambert_args_refused(C, nalb, albedo, rows, rows_ok, 3, fdown, sph, emission);
  if (rc || (rc = lambert_state_refused(a, b, u != nullptr, u_mu, u0_mu))) return rc;
  if (band && (u_mu || u0_mu) && !view_band_consistent(a))
    return fail(RTD_ERR_ARG, "couple_lambert_band: the columns of a band profile must carry identical angles");
  return drained(a, lambert_queued(a, b, nalb, albedo, rows, fdown, sph, emission, u, u0, fup, fdn, u_mu, u0_mu, band));
}

int rtd_plan_couple_lambert(rtd_plan* primary, rtd_plan* companion, int32_t nalb, const double* albedo, int32_t albedo_rows,
                            const double* fdown_bottom, const double* sph_albedo, const double* emission, double* u, double* u0,
                            double* flux_up, double* flux_down_diffuse, double* u_mu, double* u0_mu) {
  return lambert_entry(primary, companion, nalb, albedo, albedo_rows, fdown_bottom, sph_albedo, emission, u, u0, flux_up, flux_down_diffuse,
                       u_mu, u0_mu, false);
}

int rtd_plan_couple_lambert_band(rtd_plan* primary, rtd_plan* companion, int32_t nalb, const double* albedo, int32_t albedo_rows,
                                 const double* fdown_bottom, const double* sph_albedo, const double* emission, double* u, double* u0,
                                 double* flux_up, double* flux_down_diffuse, double* u_mu, double* u0_mu) {
  return lambert_entry(primary, companion, nalb, albedo, albedo_rows, fdown_bottom, sph_albedo, emission, u, u0, flux_up, flux_down_diffuse,
                       u_mu, u0_mu, true);
}

int rtd_lambert_kappa(int32_t device, int64_t ncols, int32_t nalb, const double* albedo, int32_t albedo_rows, const double* fdown_bottom,
                      const double* sph_albedo, const double* emission, double* kappa, int32_t* flag) {
  if (ncols < 1 || !kappa) return fail(RTD_ERR_ARG, "lambert_kappa: need ncols >= 1 and an output array");
  const int64_t rows_ok[2] = {1, ncols};
  int rc = lambert_args_refused(ncols, nalb, albedo, albedo_rows, rows_ok, 2, fdown_bottom, sph_albedo, emission);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  const int64_t C = ncols, NA = nalb, n_alb = (int64_t)albedo_rows * NA, total = n_alb + 3 * C + C * NA + (C + 1) / 2 + 1;
  Scratch blk;
  HIP_TRY(blk.get(total, device));
  double *d_alb = blk.data(), *d_f = d_alb + n_alb, *d_s = d_f + C, *d_e = d_s + C, *d_k = d_e + C;
  int* d_flag = reinterpret_cast<int*>(d_k + C * NA);
  hipError_t e = upload_parts(d_alb, {{albedo, n_alb}, {fdown_bottom, C}, {sph_albedo, C}, {emission, C}});
  if (e == hipSuccess) {
    (void)hipGetLastError();
    rtd_launch_lambert_kappa(d_alb, (long)(C / albedo_rows), nalb, d_f, d_s, emission ? d_e : nullptr, nullptr, nullptr, (long)C, d_k, d_flag,
                             (hipStream_t)0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(kappa, d_k, (size_t)(C * NA) * 8, hipMemcpyDeviceToHost);  // (waits for the kernel)
  if (e == hipSuccess && flag) e = hipMemcpy(flag, d_flag, (size_t)C * 4, hipMemcpyDeviceToHost);
  return finish(e, (hipStream_t)0, "lambert_kappa");
}

int rtd_plan_set_nt(rtd_plan* p, int32_t nleg_all, const double* weighted_leg_all, const double* f_arr,
                    const double* ims_coef, const double* ims_par) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (nleg_all <= 0) {  // switch the corrections off
    p->have_nt = false;
    return 0;
  }
  if (!weighted_leg_all || !f_arr || !ims_coef || !ims_par) return fail(RTD_ERR_ARG, "null argument");
  if (!p->d.beam) return fail(RTD_ERR_ARG, "NT corrections need a beam source");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t C = p->d.C, L = p->d.L;
  if (int rc = nt_buffers(p, C, nleg_all)) return rc;
  hipStream_t s = p->stream;
  HIP_TRY(hipMemcpyAsync(p->nt_w, weighted_leg_all, (size_t)(C * L * nleg_all) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(p->nt_f, f_arr, (size_t)(C * L) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(p->nt_ic, ims_coef, (size_t)(C * nleg_all) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(p->nt_ip, ims_par, (size_t)(C * 2) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  nt_bind(p, nleg_all, 1, C);
  p->nt_tables_ready = false;
  return 0;
}

int rtd_plan_request_nt(rtd_plan* p, int32_t nleg_all) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  p->nt_request = nleg_all > 0 ? nleg_all : 0;
  return 0;
}

int rtd_plan_get_nt(rtd_plan* p, double* wfull, double* f, double* ims_coef, double* ims_par, int32_t* rows) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (!p->have_nt) return fail(RTD_ERR_STATE, "get_nt: no Nakajima-Tanaka inputs are set");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t C = p->d.C, L = p->d.L, na = p->nt.nleg_all;
  hipStream_t s = p->stream;
  if (wfull) HIP_TRY(hipMemcpyAsync(wfull, p->nt_w, (size_t)(p->nt_rows * L * na) * 8, hipMemcpyDeviceToHost, s));
  if (f) HIP_TRY(hipMemcpyAsync(f, p->nt_f, (size_t)(C * L) * 8, hipMemcpyDeviceToHost, s));
  if (ims_coef) HIP_TRY(hipMemcpyAsync(ims_coef, p->nt_ic, (size_t)(C * na) * 8, hipMemcpyDeviceToHost, s));
  if (ims_par) HIP_TRY(hipMemcpyAsync(ims_par, p->nt_ip, (size_t)(C * 2) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (rows) *rows = (int32_t)p->nt_rows;
  return 0;
}

int rtd_plan_get_tensors(rtd_plan* p, int32_t column, double* GC, double* K, double* B, double* Gim, double* G) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  p->touches_handoff();
  if (!p->solved) return fail(RTD_ERR_STATE, "get_tensors before solve");
  if (column < 0 || column >= p->d.C) return fail(RTD_ERR_ARG, "column out of range");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t M = p->d.M, L = p->d.L, Qr = 2 * p->d.N;
  const int64_t nG = M * L * Qr * Qr, nK = M * L * Qr, nZ = L * Qr;
  if (!p->ex_buf) {
    int rc = p->alloc(&p->ex_buf, 2 * nG + 2 * nK + nZ);
    if (rc) return rc;
  }
  hipStream_t s = p->stream;
  RtdDev d = p->d;
  int local = column;
  if (p->nwin > 1) {  // a view of the one column: its own place in the retained arrays, else window slot 0.  The table launches
    //                   below are not launch_all_tables: they fill the ONE column's part, and all-columns tables stay stale after them
    d = window_dev(p, column, 1);
    local = 0;
    if (p->lean) {  // lean: the column's Y, A again (a wavefront of the eigen stage never spans columns from 8 streams up; below, one
      //               column on its own is what a one-column plan computes), coefficients kept
      if (!p->tables_valid) {
        rtd_launch_tables(d, s, !p->quad_tables_valid);
        p->quad_tables_valid = true;
      }
      for (int part = 0; part < 3; ++part) rtd_launch_eig(d, s, part);
    } else if (!p->retained) {  // the column is solved again on its own (its window's intermediates may have been overwritten)
      if (!p->tables_cached || !p->tables_valid) rtd_launch_tables(d, s, false);
      for (int part = 0; part < 3; ++part) rtd_launch_eig(d, s, part);
      for (int part = 0; part < 2; ++part) rtd_launch_bc(d, s, part);
    }
  }
  double *dGC = p->ex_buf, *dG = dGC + nG, *dK = dG + nG, *dB = dK + nK, *dZ = dB + nK;
  HIP_TRY(hipMemsetAsync(dZ, 0, (size_t)nZ * 8, s));
  rtd_launch_export(d, local, dGC, dK, dB, dZ, dG, s);
  HIP_TRY(hipStreamSynchronize(s));
  const struct { double *host, *dev; int64_t n; } outs[5] = {{GC, dGC, nG}, {G, dG, nG}, {K, dK, nK}, {B, dB, nK}, {Gim, dZ, nZ}};
  for (const auto& o : outs)
    if (o.host) HIP_TRY(hipMemcpy(o.host, o.dev, (size_t)o.n * 8, hipMemcpyDeviceToHost));
  return check_status(p);
}

static int solve_once(const rtd_dims* dims, int32_t device, const rtd_inputs* in, rtd_plan** out) {
  if (!dims || !in || !out) return fail(RTD_ERR_ARG, "null argument");
  rtd_plan* p = nullptr;
  int rc = rtd_plan_create(dims, device, &p);
  if (rc) return rc;
  rc = rtd_plan_set_quadrature(p, in->mu_pos, in->weights);
  if (!rc)
    rc = rtd_plan_set_columns(p, in->scaled_omega, in->tau, in->scaled_tau_with_0, in->scale_tau, in->wleg, in->mu0,
                              in->I0, in->phi0, in->rescale, in->b_pos, in->b_neg, in->s_poly, in->bdrf_q, in->bdrf_q0);
  if (!rc) rc = rtd_plan_solve(p);
  if (rc) return destroy_keeping_error(p, rc);
  *out = p;
  return 0;
}

int rtd_solve_batch(const rtd_dims* dims, int32_t device, const rtd_inputs* in, int32_t ntau, const double* tau,
                    int32_t nphi, const double* phi, double* u, double* u0, double* flux_up, double* fdn, double* fdir) {
  rtd_plan* p = nullptr;
  int rc = solve_once(dims, device, in, &p);
  if (rc) return rc;
  rc = rtd_plan_evaluate(p, ntau, tau, nphi, phi, 0, u, u0, flux_up, fdn, fdir, nullptr);
  return destroy_keeping_error(p, rc);
}

int rtd_solve_tensors(const rtd_dims* dims, int32_t device, const rtd_inputs* in, int32_t column, double* GC, double* K,
                      double* B, double* Gim, double* G) {
  rtd_plan* p = nullptr;
  int rc = solve_once(dims, device, in, &p);
  if (rc) return rc;
  rc = rtd_plan_get_tensors(p, column, GC, K, B, Gim, G);
  return destroy_keeping_error(p, rc);
}

int rtd_plan_enable_timing(rtd_plan* p, int32_t enable) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (enable && !p->evt[0]) {
    HIP_TRY(hipSetDevice(p->device));
    for (auto& e : p->evt) HIP_TRY(hipEventCreate(&e));
  }
  if (!enable && p->timing) {
    HIP_TRY(hipStreamSynchronize(p->stream));
    harvest(p);
  }
  p->timing = enable != 0;
  return 0;
}

int rtd_plan_get_timing(rtd_plan* p, double ms[7], int64_t nlaunch[7], int32_t reset) {
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  HIP_TRY(hipStreamSynchronize(p->stream));
  harvest(p);
  for (int k = 0; k < rtd_plan::NT; ++k) {
    if (ms) ms[k] = p->ms[k];
    if (nlaunch) nlaunch[k] = p->nlaunch[k];
    if (reset) {
      p->ms[k] = 0;
      p->nlaunch[k] = 0;
    }
  }
  return 0;
}

int rtd_plan_pivoted_chains(rtd_plan* p, int32_t* chains) {
  if (!p || !chains) return fail(RTD_ERR_ARG, "null argument");
  *chains = 0;
  if (p->d.NP != 32) return 0;
  const size_t n = (size_t)p->Cw * p->d.M;
  std::vector<int> h(n);
  HIP_TRY(hipMemcpyAsync(h.data(), p->d.need_split, n * sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  int k = 0;
  for (size_t i = 0; i < n; ++i)
    if (h[i] != 0) {
      ++k;
      if (getenv("RTD_DEBUG")) fprintf(stderr, "[rtd] pivoted chain: column %zu mode %zu\n", i / p->d.M, i % p->d.M);
    }
  *chains = k;
  return 0;
}

int rtd_plan_max_sweeps(rtd_plan* p, int32_t* sweeps) {
  if (!p || !sweeps) return fail(RTD_ERR_ARG, "null argument");
  int v = 0;
  HIP_TRY(hipMemcpyAsync(&v, p->d.sweeps, sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  *sweeps = v;
  return 0;
}

/* ---- RCCL over xGMI: one communicator rank per plan/GPU ------------------ */
namespace {
struct RcclApi {
  void* h = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommCuDevice)(const ncclComm_t, int*) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  const char* (*StubTransport)(const ncclComm_t) = nullptr;  // only the tests' stand-in transport exports it
  bool stub = false;
};
RcclApi* rccl() {
  static RcclApi api;
  static std::once_flag once;  // plans may be used from different host threads (one thread per plan)
  std::call_once(once, [] {
    // The ROCm install's RCCL first, by absolute path: a process that also imports PyTorch carries a second,
    // bundled RCCL/HIP pair under the same SONAMEs, and RCCL must bind to the HIP runtime librtd itself uses.
    // RTD_RCCL_STUB (tests only; never set by the library or its Python package): the path of a stand-in for these entry
    // points, for rank processes that share ONE GPU -- RCCL refuses a second rank on a device, so this is the only way the
    // rank > 0 code of rtd_comm_* can execute on a one-GPU box (tests/stub/rccl_stub.cpp).  When it is set nothing else is
    // tried: a stub that fails to load is an error, not a silent switch to RCCL; rtd_comm_transport() reports which one runs.
    const char* stub = getenv("RTD_RCCL_STUB");
    if (stub && *stub) {
      api.h = dlopen(stub, RTLD_NOW | RTLD_LOCAL);
      api.stub = true;
      if (!api.h) fprintf(stderr, "[rtd] RTD_RCCL_STUB=%s: %s\n", stub, dlerror());
    } else {
      for (const char* name : {"/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so"}) {
        api.h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (api.h) break;
      }
    }
    if (api.h) {
      api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.h, "ncclGetUniqueId");
      api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.h, "ncclCommInitRank");
      api.AllGather = (decltype(api.AllGather))dlsym(api.h, "ncclAllGather");
      api.AllReduce = (decltype(api.AllReduce))dlsym(api.h, "ncclAllReduce");
      api.Send = (decltype(api.Send))dlsym(api.h, "ncclSend");
      api.Recv = (decltype(api.Recv))dlsym(api.h, "ncclRecv");
      api.GroupStart = (decltype(api.GroupStart))dlsym(api.h, "ncclGroupStart");
      api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.h, "ncclGroupEnd");
      api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.h, "ncclCommDestroy");
      api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.h, "ncclGetErrorString");
      api.CommCount = (decltype(api.CommCount))dlsym(api.h, "ncclCommCount");
      api.CommUserRank = (decltype(api.CommUserRank))dlsym(api.h, "ncclCommUserRank");
      api.CommCuDevice = (decltype(api.CommCuDevice))dlsym(api.h, "ncclCommCuDevice");
      if (api.stub) api.StubTransport = (decltype(api.StubTransport))dlsym(api.h, "rcclStubTransport");
      if (api.stub && !api.StubTransport) api.h = nullptr;  // RTD_RCCL_STUB must name the stub, not some other RCCL
      if (!api.GetUniqueId || !api.CommInitRank || !api.AllGather || !api.CommDestroy || !api.GetErrorString) api.h = nullptr;
    }
  });
  return api.h ? &api : nullptr;
}
}  // namespace

int rtd_comm_preload(void) {
  return rccl() ? 0 : fail(RTD_ERR_HIP, "librccl.so could not be loaded");
}

int rtd_comm_unique_id(char id[128]) {
  RcclApi* r = rccl();
  if (!r) return fail(RTD_ERR_HIP, "librccl.so could not be loaded");
  ncclUniqueId u;
  ncclResult_t rc = r->GetUniqueId(&u);
  if (rc != ncclSuccess) return fail(RTD_ERR_HIP, std::string("ncclGetUniqueId: ") + r->GetErrorString(rc));
  std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return 0;
}

int rtd_comm_init(rtd_plan* p, const char id[128], int32_t rank, int32_t nranks) {
  if (!p || !id || rank < 0 || rank >= nranks) return fail(RTD_ERR_ARG, "bad communicator arguments");
  if (p->band_cols || p->band_G > 0) return fail(RTD_ERR_STATE, "communicator: not combined with band inputs or band weights");
  RcclApi* r = rccl();
  if (!r) return fail(RTD_ERR_HIP, "librccl.so could not be loaded");
  HIP_TRY(hipSetDevice(p->device));
  ncclUniqueId u;
  std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  ncclResult_t rc = r->CommInitRank(&p->comm, nranks, u, rank);
  if (rc != ncclSuccess) {
    p->comm = nullptr;
    return fail(RTD_ERR_HIP, std::string("ncclCommInitRank: ") + r->GetErrorString(rc));
  }
  p->comm_rank = rank;
  p->comm_size = nranks;
  return 0;
}

// What RCCL itself says about the plan's communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice) -- not the
// arguments rtd_comm_init was called with.  A caller that reports "N ranks" reports this.
int rtd_comm_size(rtd_plan* p, int32_t* nranks, int32_t* rank, int32_t* device) {
  if (!p || !p->comm) return fail(RTD_ERR_STATE, "communicator not initialised");
  RcclApi* r = rccl();
  if (!r || !r->CommCount || !r->CommUserRank) return fail(RTD_ERR_HIP, "librccl.so lacks ncclCommCount / ncclCommUserRank");
  int n = -1, me = -1, dev = -1;
  ncclResult_t rc = r->CommCount(p->comm, &n);
  if (rc == ncclSuccess) rc = r->CommUserRank(p->comm, &me);
  if (rc == ncclSuccess && r->CommCuDevice) rc = r->CommCuDevice(p->comm, &dev);
  if (rc != ncclSuccess) return fail(RTD_ERR_HIP, std::string("ncclCommCount / ncclCommUserRank: ") + r->GetErrorString(rc));
  if (n != p->comm_size || me != p->comm_rank)
    return fail(RTD_ERR_STATE, "RCCL reports rank " + std::to_string(me) + " of " + std::to_string(n) + ", the plan was initialised as rank " +
                                   std::to_string(p->comm_rank) + " of " + std::to_string(p->comm_size));
  if (nranks) *nranks = n;
  if (rank) *rank = me;
  if (device) *device = dev;
  return 0;
}

// Which transport carries the collectives: "rccl" (librccl.so of the ROCm install), or "stub:ipc" / "stub:shm" when the
// environment named the tests' stand-in (RTD_RCCL_STUB).  A caller that reports a multi-rank rate must report this beside it.
int rtd_comm_transport(rtd_plan* p, char* buf, int32_t nbuf) {
  if (!buf || nbuf < 2) return fail(RTD_ERR_ARG, "transport: no buffer");
  RcclApi* r = rccl();
  if (!r) return fail(RTD_ERR_HIP, "librccl.so could not be loaded");
  const char* name = !r->stub ? "rccl" : r->StubTransport(p ? p->comm : nullptr);
  std::snprintf(buf, (size_t)nbuf, "%s", name);
  return 0;
}

int rtd_comm_allgather_fluxes(rtd_plan* p) {
  if (!p || !p->comm) return fail(RTD_ERR_STATE, "communicator not initialised");
  if (p->ev_ntau < 1) return fail(RTD_ERR_STATE, "no evaluation results to gather");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t n = ResultShape(p).fl();
  int rc = grow(p, p->gathered, n * p->comm_size);
  if (rc) return rc;
  ncclResult_t nr = rccl()->AllGather(p->ev_fl, p->gathered, (size_t)n, ncclDouble, p->comm, p->stream);
  if (nr != ncclSuccess) return fail(RTD_ERR_HIP, std::string("ncclAllGather: ") + rccl()->GetErrorString(nr));
  return 0;
}

namespace {
// The preamble of the two results collectives.  The gathered arrays are grown to `slots` shards; the rank's own results are copied
// (device to device, on the plan's stream, behind the run that produced them) into shard `my_slot`, and the collective then runs
// from there on the communication stream, behind ev_results: the result buffers are free at once, so the next run's evaluation
// kernels never wait for the collective (with windows of 256 columns only ~1 ms of the next run precedes its first evaluation
// kernel: waiting there would expose most of the gather).  The copy of the NEXT gather waits for this gather (one whole step later).
int snapshot_results(rtd_plan* p, int64_t slots, int64_t my_slot, double** my_u, double** my_fl) {
  const ResultShape r(p);
  const int64_t nu = r.u(), nfl = r.fl();
  int rc;
  if ((rc = grow(p, p->gathered_u, std::max<int64_t>(nu, 1) * slots))) return rc;
  if ((rc = grow(p, p->gathered_fl, nfl * slots))) return rc;
  if (!p->comm_stream) HIP_TRY(hipStreamCreateWithFlags(&p->comm_stream, hipStreamNonBlocking));
  if ((rc = ensure_event(&p->ev_results)) || (rc = ensure_event(&p->ev_gathered))) return rc;
  if (p->gather_inflight) HIP_TRY(hipStreamWaitEvent(p->stream, p->ev_gathered, 0));
  *my_u = p->gathered_u + my_slot * nu;
  *my_fl = p->gathered_fl + my_slot * nfl;
  if (nu > 0) HIP_TRY(hipMemcpyAsync(*my_u, p->ev_u, (size_t)nu * 8, hipMemcpyDeviceToDevice, p->stream));
  HIP_TRY(hipMemcpyAsync(*my_fl, p->ev_fl, (size_t)nfl * 8, hipMemcpyDeviceToDevice, p->stream));
  HIP_TRY(hipEventRecord(p->ev_results, p->stream));
  HIP_TRY(hipStreamWaitEvent(p->comm_stream, p->ev_results, 0));
  return 0;
}

// does this rank hold the gathered arrays of ALL ranks of the last results collective (fluxes; and u, if it is wanted)?
bool holds_gathered(const rtd_plan* p, bool want_u) {
  const ResultShape r(p);
  return p->gathered_here && p->gathered_fl.cap >= r.fl() * p->comm_size && !(want_u && r.u() > 0 && p->gathered_u.cap < r.u() * p->comm_size);
}
}  // namespace

int rtd_comm_allgather_results(rtd_plan* p) {
  if (!p || !p->comm) return fail(RTD_ERR_STATE, "communicator not initialised");
  if (p->ev_ntau < 1 || !p->solved) return fail(RTD_ERR_STATE, "no evaluation results to gather");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t nu = ResultShape(p).u(), nfl = ResultShape(p).fl();
  // every rank holds all shards, its own in the slot of its rank: the all-gather runs IN PLACE from there
  double *my_u = nullptr, *my_fl = nullptr;
  if (int rc = snapshot_results(p, p->comm_size, p->comm_rank, &my_u, &my_fl)) return rc;
  RcclApi* r = rccl();
  ncclResult_t nr = ncclSuccess;
  if (nu > 0) nr = r->AllGather(my_u, p->gathered_u, (size_t)nu, ncclDouble, p->comm, p->comm_stream);
  if (nr == ncclSuccess) nr = r->AllGather(my_fl, p->gathered_fl, (size_t)nfl, ncclDouble, p->comm, p->comm_stream);
  if (nr != ncclSuccess) return fail(RTD_ERR_HIP, std::string("ncclAllGather: ") + r->GetErrorString(nr));
  HIP_TRY(hipEventRecord(p->ev_gathered, p->comm_stream));
  p->gather_inflight = p->gathered_here = true;
  return 0;
}

int rtd_comm_gather_results(rtd_plan* p, int32_t root) {
  if (!p || !p->comm) return fail(RTD_ERR_STATE, "communicator not initialised");
  if (p->ev_ntau < 1 || !p->solved) return fail(RTD_ERR_STATE, "no evaluation results to gather");
  if (root < 0 || root >= p->comm_size) return fail(RTD_ERR_ARG, "root outside the communicator");
  RcclApi* r = rccl();
  if (!r->Send || !r->Recv || !r->GroupStart || !r->GroupEnd) return fail(RTD_ERR_HIP, "this RCCL has no ncclSend / ncclRecv");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t nu = ResultShape(p).u(), nfl = ResultShape(p).fl();
  const bool is_root = p->comm_rank == root;
  // the root holds the gathered arrays, its own results in its own slot; the other ranks one shard of each, as the send buffer
  double *my_u = nullptr, *my_fl = nullptr;
  if (int rc = snapshot_results(p, is_root ? p->comm_size : 1, is_root ? root : 0, &my_u, &my_fl)) return rc;
  hipStream_t cs = p->comm_stream;
  ncclResult_t nr = r->GroupStart();
  if (is_root) {
    for (int q = 0; q < p->comm_size && nr == ncclSuccess; ++q) {
      if (q == root) continue;
      if (nu > 0) nr = r->Recv(p->gathered_u + q * nu, (size_t)nu, ncclDouble, q, p->comm, cs);
      if (nr == ncclSuccess) nr = r->Recv(p->gathered_fl + q * nfl, (size_t)nfl, ncclDouble, q, p->comm, cs);
    }
  } else {
    if (nu > 0) nr = r->Send(my_u, (size_t)nu, ncclDouble, root, p->comm, cs);
    if (nr == ncclSuccess) nr = r->Send(my_fl, (size_t)nfl, ncclDouble, root, p->comm, cs);
  }
  ncclResult_t ne = r->GroupEnd();
  if (nr == ncclSuccess) nr = ne;
  if (nr != ncclSuccess) return fail(RTD_ERR_HIP, std::string("ncclSend / ncclRecv: ") + r->GetErrorString(nr));
  HIP_TRY(hipEventRecord(p->ev_gathered, cs));
  p->gather_inflight = true;
  p->gathered_here = is_root;  // (a non-root rank may still hold full-size buffers of an earlier all-gather: they are stale now)
  return 0;
}

int rtd_comm_fetch_gathered_results(rtd_plan* p, double* u, double* fluxes) {
  if (!p || !p->gathered_fl) return fail(RTD_ERR_STATE, "nothing gathered");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t nu = ResultShape(p).u(), nfl = ResultShape(p).fl();
  if (!holds_gathered(p, u != nullptr))
    return fail(RTD_ERR_STATE, "this rank holds no gathered arrays of the last collective (rtd_comm_gather_results: only the root does)");
  hipStream_t s = p->comm_stream;
  if (u && nu > 0) HIP_TRY(hipMemcpyAsync(u, p->gathered_u, (size_t)(nu * p->comm_size) * 8, hipMemcpyDeviceToHost, s));
  if (fluxes) HIP_TRY(hipMemcpyAsync(fluxes, p->gathered_fl, (size_t)(nfl * p->comm_size) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int rtd_comm_fetch_gathered_columns(rtd_plan* p, int32_t rank, int32_t first, int32_t count, double* u, double* fluxes) {
  if (!p || !p->gathered_fl) return fail(RTD_ERR_STATE, "nothing gathered");
  HIP_TRY(hipSetDevice(p->device));
  const ResultShape r(p);
  const int64_t C = r.C, nt = r.nt, per_u = r.per_column_u(), nu = r.u(), nfl = r.fl();
  if (rank < 0 || rank >= p->comm_size || first < 0 || count < 1 || (int64_t)first + count > C)
    return fail(RTD_ERR_ARG, "gathered columns: rank or column range outside the gathered arrays");
  if (!holds_gathered(p, u != nullptr))
    return fail(RTD_ERR_STATE, "this rank holds no gathered arrays of the last collective (rtd_comm_gather_results: only the root does)");
  hipStream_t s = p->comm_stream;  // behind the collective
  if (u && per_u > 0)
    HIP_TRY(hipMemcpyAsync(u, p->gathered_u + rank * nu + first * per_u, (size_t)(count * per_u) * 8, hipMemcpyDeviceToHost, s));
  if (fluxes)
    for (int f = 0; f < 3; ++f)
      HIP_TRY(hipMemcpyAsync(fluxes + (int64_t)f * count * nt, p->gathered_fl + rank * nfl + r.flux_at(f) + (int64_t)first * nt,
                             (size_t)(count * nt) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

namespace {
// [CM][L][E] <-> layer-major staging [L'][CM][E] for the layers [l0, l0 + ln): to_stage packs, else unpacks
__global__ void rtd_layer_stage_kernel(double* arr, double* stage, long CM, int L, int E, int l0, int ln, int to_stage) {
  const long total = (long)ln * CM * E;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int e = (int)(idx % E);
    const long cm = (idx / E) % CM;
    const int ll = (int)(idx / ((long)E * CM));
    double* a = arr + (cm * L + l0 + ll) * E + e;
    if (to_stage) stage[idx] = *a;
    else *a = stage[idx];
  }
}
struct LayerSeg { double* arr; long CM; int E; };
int layer_segments(rtd_plan* p, LayerSeg seg[8]) {
  const RtdDev& d = p->d;
  const long CM = (long)d.C * d.M;
  const int NP = d.NP, Q2 = 2 * d.NP;
  int n = 0;
  seg[n++] = {d.Ym, CM, NP * NP};
  seg[n++] = {d.Am, CM, NP * NP};
  seg[n++] = {d.kk, CM, NP};
  seg[n++] = {d.Ek, CM, NP};
  seg[n++] = {d.Bv, CM, Q2};
  if (d.Ns > 0) {
    seg[n++] = {d.dq, (long)d.C, d.Ns * Q2};
    seg[n++] = {d.zneg, (long)d.C, NP};
    seg[n++] = {d.vb, (long)d.C, 4 * NP};
  }
  return n;
}
}  // namespace

int rtd_plan_solve_layers(rtd_plan* p, int32_t first, int32_t count) {
  (void)hipGetLastError();  // (as launch_windows: a stale code of this thread is not this call's)
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  p->touches_handoff();
  if (!p->have_quad || !p->have_cols) return fail(RTD_ERR_STATE, "set_quadrature and set_columns must precede solve");
  if (p->nwin != 1) return fail(RTD_ERR_STATE, "layer shards need a plan of one window");
  if (first < 0 || count < 1 || first + count > p->d.L) return fail(RTD_ERR_ARG, "layer range outside the atmosphere");
  HIP_TRY(hipSetDevice(p->device));
  RtdDev d = p->d;
  d.l0 = first;
  d.ln = count;
  d.um = nullptr;
  HIP_TRY(clear_status(d, p->stream));  // as launch_windows: a new solve starts clean
  p->numeric_status = 0;
  launch_all_tables(p, d, p->stream);  // (one-window plan: d.Y0 / d.att are the all-columns tables; the view carries the layer shard)
  rtd_launch_eig(d, p->stream, 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RTD_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  p->solution_stale();
  return 0;
}

int rtd_comm_allgather_layers(rtd_plan* p, int32_t count) {
  if (!p || !p->comm) return fail(RTD_ERR_STATE, "communicator not initialised");
  if (p->nwin != 1) return fail(RTD_ERR_STATE, "layer shards need a plan of one window");
  if (count < 1 || (int64_t)count * p->comm_size != p->d.L)
    return fail(RTD_ERR_ARG, "layer shards: nlayers must equal count_per_rank x nranks");
  HIP_TRY(hipSetDevice(p->device));
  LayerSeg seg[8];
  const int nseg = layer_segments(p, seg);
  int64_t per_rank = 0;
  for (int k = 0; k < nseg; ++k) per_rank += (int64_t)count * seg[k].CM * seg[k].E;
  int rc;
  // staging: this rank's packed layers, then everybody's (reuses the gathered-u buffer slot of the plan)
  double* mine = nullptr;
  HIP_TRY(hipMalloc(&mine, (size_t)per_rank * 8));
  p->gathered_here = false;  // the gathered-u buffer is layer staging from here on: no results fetch may read it as gathered u
  if ((rc = grow(p, p->gathered_u, per_rank * p->comm_size))) {
    (void)hipFree(mine);
    return rc;
  }
  hipStream_t s = p->stream;
  const int L = p->d.L, l0 = p->comm_rank * count;
  int64_t off = 0;
  for (int k = 0; k < nseg; ++k) {
    hipLaunchKernelGGL(rtd_layer_stage_kernel, dim3(1024), dim3(256), 0, s, seg[k].arr, mine + off, seg[k].CM, L, seg[k].E, l0, count, 1);
    off += (int64_t)count * seg[k].CM * seg[k].E;
  }
  ncclResult_t nr = rccl()->AllGather(mine, p->gathered_u, (size_t)per_rank, ncclDouble, p->comm, s);
  if (nr == ncclSuccess) {
    for (int g = 0; g < p->comm_size; ++g) {
      if (g == p->comm_rank) continue;  // this rank's own layers are in place
      off = 0;
      for (int k = 0; k < nseg; ++k) {
        hipLaunchKernelGGL(rtd_layer_stage_kernel, dim3(1024), dim3(256), 0, s, seg[k].arr, p->gathered_u + g * per_rank + off,
                           seg[k].CM, L, seg[k].E, g * count, count, 0);
        off += (int64_t)count * seg[k].CM * seg[k].E;
      }
    }
  }
  hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(mine);
  if (nr != ncclSuccess) return fail(RTD_ERR_HIP, std::string("ncclAllGather: ") + rccl()->GetErrorString(nr));
  if (e != hipSuccess) return fail(RTD_ERR_HIP, hipGetErrorString(e));
  return 0;
}

int rtd_plan_solve_bc(rtd_plan* p) {
  (void)hipGetLastError();  // (as launch_windows: a stale code of this thread is not this call's)
  if (!p) return fail(RTD_ERR_ARG, "null plan");
  if (!p->have_quad || !p->have_cols) return fail(RTD_ERR_STATE, "inputs missing");
  if (p->nwin != 1) return fail(RTD_ERR_STATE, "layer shards need a plan of one window");
  HIP_TRY(hipSetDevice(p->device));
  RtdDev d = p->d;
  d.um = nullptr;
  rtd_launch_bc(d, p->stream, 0);
  rtd_launch_bc(d, p->stream, 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RTD_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  p->solved = true;
  return 0;
}

int rtd_comm_allreduce_results(rtd_plan* p) {
  if (!p || !p->comm) return fail(RTD_ERR_STATE, "communicator not initialised");
  if (p->ev_ntau < 1) return fail(RTD_ERR_STATE, "no evaluation results to reduce");
  RcclApi* r = rccl();
  if (!r || !r->AllReduce) return fail(RTD_ERR_HIP, "ncclAllReduce not available");
  HIP_TRY(hipSetDevice(p->device));
  const ResultShape rs(p);
  struct { double* ptr; int64_t n; } bufs[3] = {{p->ev_u, rs.u()}, {p->ev_u0, rs.u0()}, {p->ev_fl, rs.fl()}};
  for (auto& b : bufs) {
    if (!b.ptr || b.n <= 0) continue;
    ncclResult_t nr = r->AllReduce(b.ptr, b.ptr, (size_t)b.n, ncclDouble, ncclSum, p->comm, p->stream);
    if (nr != ncclSuccess) return fail(RTD_ERR_HIP, std::string("ncclAllReduce: ") + r->GetErrorString(nr));
  }
  return 0;
}

int rtd_comm_fetch_gathered(rtd_plan* p, double* out) {
  if (!p || !out || !p->gathered) return fail(RTD_ERR_STATE, "nothing gathered");
  HIP_TRY(hipSetDevice(p->device));
  const int64_t n = ResultShape(p).fl() * p->comm_size;
  HIP_TRY(hipMemcpyAsync(out, p->gathered, (size_t)n * 8, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

int rtd_comm_destroy(rtd_plan* p) {
  if (!p) return 0;
  if (p->comm && rccl()) {
    (void)hipStreamSynchronize(p->stream);
    if (p->comm_stream) (void)hipStreamSynchronize(p->comm_stream);
    rccl()->CommDestroy(p->comm);
  }
  p->comm = nullptr;
  p->gather_inflight = false;
  return 0;
}

}  // extern "C"
