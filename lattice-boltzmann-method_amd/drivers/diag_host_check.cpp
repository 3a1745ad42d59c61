// The CPU-reachable half of the diagnostics as a stand-alone program: lbm_diag_fold_host against a restatement of the
// summation order written here (64 accumulators, ascending slices, six halvings) over every row count and sub-range
// that straddles the accumulator count, and every host-side refusal of the diagnostics' entry points.  Needs no
// device.  `make san` at the root builds it against the sanitizer build of the library (ASan + UBSan) and runs it;
// the ordinary build runs it from tests/test_diag_abi.py.  Exit status 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/lbm_hip.h"

static int failures = 0;
static void expect(bool ok, const std::string& what) {
  if (!ok) {
    ++failures;
    std::printf("FAIL: %s\n", what.c_str());
  }
}

// 0 add, 1 min, 2 max
static int op_of(int q) {
  if (q == LBM_DIAG_MIN_RHO || q == LBM_DIAG_MIN_C) return 1;
  if (q == LBM_DIAG_MAX_U2 || q == LBM_DIAG_MAX_RHO || q == LBM_DIAG_MAX_C) return 2;
  return 0;
}
static double fold64(const std::vector<double>& x, int op) {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> p(64, op == 0 ? 0.0 : op == 1 ? inf : -inf);
  auto f = [op](double a, double b) { return op == 0 ? a + b : op == 1 ? std::fmin(a, b) : std::fmax(a, b); };
  for (size_t i = 0; i < x.size(); ++i) p[i % 64] = f(p[i % 64], x[i]);  // ascending i = ascending slice per accumulator
  for (int s = 32; s >= 1; s /= 2)
    for (int j = 0; j < s; ++j) p[j] = f(p[j], p[j + s]);
  return p[0];
}

// refused with LBM_ERR_INVALID and a message that names `word`
static void refused(int rc, const char* word, const char* what) {
  const std::string msg = lbm_last_error_string();
  expect(rc == LBM_ERR_INVALID && msg.find(word) != std::string::npos, std::string(what) + " -> " + std::to_string(rc) + ": " + msg);
}

int main() {
  // deterministic values of mixed sign over 12 decades (an LCG; the order of the additions visibly matters)
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto next = [&state]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) / 9007199254740992.0;  // [0, 1)
  };
  const int counts[] = {1, 2, 63, 64, 65, 128, 129, 200};
  int folds = 0;
  for (int n : counts) {
    std::vector<double> table((size_t)LBM_DIAG_NQ * n);
    for (double& v : table) v = (next() - 0.5) * std::pow(10.0, 12.0 * next() - 6.0);
    const int ranges[][2] = {{0, n}, {n > 1 ? 1 : 0, n}, {n / 3, n - n / 4}, {n > 64 ? 63 : 0, n > 64 ? n - 1 : n}};
    for (const auto& rg : ranges) {
      if (rg[0] >= rg[1]) continue;
      double out[LBM_DIAG_NQ];
      const int rc = lbm_diag_fold_host(out, table.data(), n, rg[0], rg[1]);
      expect(rc == LBM_OK, "lbm_diag_fold_host returned " + std::to_string(rc));
      for (int q = 0; q < LBM_DIAG_NQ; ++q) {
        const std::vector<double> x(table.begin() + (size_t)q * n + rg[0], table.begin() + (size_t)q * n + rg[1]);
        const double want = fold64(x, op_of(q));
        expect(std::memcmp(&want, &out[q], sizeof want) == 0,
               "fold of rows [" + std::to_string(rg[0]) + ", " + std::to_string(rg[1]) + ") of " + std::to_string(n) + ", slot " + std::to_string(q));
      }
      ++folds;
    }
  }

  // every host-side refusal; the pointers are never dereferenced
  double buf[LBM_DIAG_NQ * 4] = {0.0};
  double* p = buf;
  refused(lbm_diag_rows(nullptr, 4, 0, p, p, nullptr, nullptr, 4, 4, 0, 4, nullptr), "NULL", "diag_rows NULL table");
  refused(lbm_diag_rows(p, 4, 0, nullptr, p, nullptr, nullptr, 4, 4, 0, 4, nullptr), "NULL", "diag_rows NULL rho");
  refused(lbm_diag_rows(p, 4, 0, p, nullptr, nullptr, nullptr, 4, 4, 0, 4, nullptr), "NULL", "diag_rows NULL u");
  refused(lbm_diag_rows(p, 4, 0, p, p, nullptr, nullptr, 4, 4, 2, 2, nullptr), "row_begin", "diag_rows empty range");
  refused(lbm_diag_rows(p, 4, 0, p, p, nullptr, nullptr, 4, 4, -1, 2, nullptr), "row_begin", "diag_rows negative row_begin");
  refused(lbm_diag_rows(p, 4, 0, p, p, nullptr, nullptr, 4, 4, 0, 5, nullptr), "row_end", "diag_rows row_end > R");
  refused(lbm_diag_rows(p, 4, 1, p, p, nullptr, nullptr, 4, 4, 0, 4, nullptr), "table_row0", "diag_rows table_row0 + R > table_rows");
  refused(lbm_diag_rows(p, 4, -1, p, p, nullptr, nullptr, 4, 4, 0, 4, nullptr), "table_row0", "diag_rows negative table_row0");
  refused(lbm_diag_rows(p, 4, 0, p, p, nullptr, nullptr, 0, 4, 0, 4, nullptr), "R=", "diag_rows R = 0");
  refused(lbm_diag_fold(nullptr, p, 4, 0, 4, nullptr), "NULL", "diag_fold NULL out");
  refused(lbm_diag_fold(p, nullptr, 4, 0, 4, nullptr), "NULL", "diag_fold NULL table");
  refused(lbm_diag_fold(p, p, 4, 3, 3, nullptr), "row_begin", "diag_fold empty range");
  refused(lbm_diag_fold(p, p, 4, 0, 5, nullptr), "row_end", "diag_fold range outside the table");
  refused(lbm_diag_fold_host(nullptr, p, 4, 0, 4), "NULL", "diag_fold_host NULL out");
  refused(lbm_diag_fold_host(p, nullptr, 4, 0, 4), "NULL", "diag_fold_host NULL table");
  refused(lbm_diag_fold_host(p, p, 4, 4, 2), "row_begin", "diag_fold_host reversed range");
  refused(lbm_diag_fold_host(p, p, 4, 0, 5), "row_end", "diag_fold_host range outside the table");
  refused(lbm_diag_fold_host(p, p, 0, 0, 1), "table_rows", "diag_fold_host table_rows = 0");
  refused(lbm_solver_diag(nullptr, nullptr, 0, 4, p, nullptr), "NULL", "solver_diag NULL solver");
  refused(lbm_ade_solver_diag(nullptr, nullptr, 0, 4, p, nullptr), "NULL", "ade_solver_diag NULL solver");
  const lbm_converge good{LBM_DIAG_SUM_UR, 100, 1, 1e-12, 1.0, 0, 4};
  for (int ade = 0; ade < 2; ++ade) {
    auto run = [ade](const lbm_converge* cv, int max_steps) {
      return ade ? lbm_ade_solver_run_until(nullptr, cv, max_steps, nullptr, nullptr, nullptr)
                 : lbm_solver_run_until(nullptr, cv, max_steps, nullptr, nullptr, nullptr);
    };
    refused(run(nullptr, 10), "NULL", "run_until NULL rule");
    refused(run(&good, 10), "NULL solver", "run_until NULL solver");
    refused(run(&good, -1), "max_steps", "run_until negative max_steps");
    for (int q : {-1, LBM_DIAG_MAX_U2, LBM_DIAG_MIN_RHO, LBM_DIAG_MAX_RHO, LBM_DIAG_NONFINITE, LBM_DIAG_MIN_C, LBM_DIAG_MAX_C, LBM_DIAG_NQ}) {
      lbm_converge cv = good;
      cv.quantity = q;
      refused(run(&cv, 10), "quantity", "run_until quantity that is no sum");
    }
    lbm_converge cv = good;
    cv.interval = 0;
    refused(run(&cv, 10), "interval", "run_until interval = 0");
    cv = good;
    cv.offset = 100;
    refused(run(&cv, 10), "offset", "run_until offset = interval");
    cv = good;
    cv.tolerance = -1e-12;
    refused(run(&cv, 10), "tolerance", "run_until negative tolerance");
    cv.tolerance = std::numeric_limits<double>::quiet_NaN();
    refused(run(&cv, 10), "tolerance", "run_until NaN tolerance");
    cv = good;
    cv.row_end = 0;
    refused(run(&cv, 10), "row_begin", "run_until empty row range");
  }
  std::printf("diag_host_check: %d folds checked, %d failures\n", folds, failures);
  return failures ? 1 : 0;
}
