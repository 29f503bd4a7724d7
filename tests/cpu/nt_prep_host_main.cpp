// TEST PROGRAM (tests/test_nt_prep_cpu.py): the routines of csrc/rtd_nt_prep.h -- what rtd_api.hip's preparation kernels of the corrections run per thread
// and per lane -- as a stand-alone host program under the address / undefined-behaviour sanitizers.  No Python is loaded under a
// sanitizer, nothing is preloaded, no runtime stands in: the header is host code as it is.
//
//   nt_prep_host_main <input> : text, hexadecimal floats throughout (no decimal conversion anywhere)
//     "ims C L nleg nleg_all"  then per column  tau[L] omega[L] f[L] leg[L][nleg_all] mu0 I0
//         -> per column one line  wfull[L][nleg_all] ims_coef[nleg_all] ims_par[2]
//            64 lanes run one after the other, as the wavefront of rtd_nt_ims_kernel runs them side by side
//     "mix R L S nleg_all"     then dspec[R][L][S] ospec[R][L][S] lspec[S][nleg_all]
//         -> per (row, layer) one line of the nleg_all mixed moments
// Every array is a heap block of exactly its documented extent: an index out of range is a sanitizer report.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pythonic-disort_amd/csrc/rtd_nt_prep.h"

typedef std::vector<double> vec;

static bool read(FILE* f, vec& v) {
  for (double& x : v)
    if (std::fscanf(f, "%la", &x) != 1) return false;
  return true;
}

static void print(const vec& v) {
  for (double x : v) std::printf("%a ", x);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = std::fopen(argv[1], "r");
  if (!in) return 2;
  char what[8];
  while (std::fscanf(in, "%7s", what) == 1) {
    if (!std::strcmp(what, "ims")) {
      int C, L, nleg, nall;
      if (std::fscanf(in, "%d %d %d %d", &C, &L, &nleg, &nall) != 4) return 3;
      for (int c = 0; c < C; ++c) {
        vec tau(L), om(L), f(L), leg((size_t)L * nall), s(2);
        if (!read(in, tau) || !read(in, om) || !read(in, f) || !read(in, leg) || !read(in, s)) return 3;
        vec wfull((size_t)L * nall), coef(nall), par(2);
        for (size_t i = 0; i < wfull.size(); ++i) wfull[i] = (2.0 * (double)(i % nall) + 1.0) * leg[i];  // rtd_nt_wfull_kernel's line
        for (int lane = 0; lane < 64; ++lane)
          rtd_nt_ims_lane(L, nleg, nall, tau.data(), om.data(), f.data(), leg.data(), s[0], s[1], lane, 64, coef.data(), par.data());
        print(wfull); print(coef); print(par);
        std::printf("\n");
      }
    } else if (!std::strcmp(what, "mix")) {
      int R, L, S, nall;
      if (std::fscanf(in, "%d %d %d %d", &R, &L, &S, &nall) != 4) return 3;
      vec ds((size_t)R * L * S), os((size_t)R * L * S), ls((size_t)S * nall);
      if (!read(in, ds) || !read(in, os) || !read(in, ls)) return 3;
      for (long rl = 0; rl < (long)R * L; ++rl) {
        vec g(nall);
        for (int k = 0; k < nall; ++k) g[k] = rtd_mix_moment(ds.data() + rl * S, os.data() + rl * S, ls.data(), S, nall, k);
        print(g);
        std::printf("\n");
      }
    } else {
      return 3;
    }
  }
  std::fclose(in);
  return 0;
}
