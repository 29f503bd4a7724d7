// TEST PROGRAM (tests/test_lambert_arith_cpu.py): the routines of csrc/rtd_lambert.h -- the very ones rtd_lambert_kappa_kernel and
// rtd_lambert_couple_kernel run -- as a stand-alone program under the address / undefined-behaviour sanitizers.  Input: a text file
// whose lines are "A F s E a b" as hexadecimal floats; output: one line "kappa bad out" per input line, kappa and out =
// rtd_lambert_couple(a, b, kappa) as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pythonic-disort_amd/csrc/rtd_lambert.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<double> rows;
  double v[6];
  while (std::fscanf(f, "%la %la %la %la %la %la", v, v + 1, v + 2, v + 3, v + 4, v + 5) == 6) rows.insert(rows.end(), v, v + 6);
  std::fclose(f);
  for (size_t i = 0; i + 5 < rows.size(); i += 6) {
    int bad = -1;
    const double kappa = rtd_lambert_kappa(rows[i], rows[i + 1], rows[i + 2], rows[i + 3], &bad);
    std::printf("%a %d %a\n", kappa, bad, rtd_lambert_couple(rows[i + 4], rows[i + 5], kappa));
  }
  return 0;
}
