// The CPU-reachable half of the wall exchange as a stand-alone program: lbm_ade_wallx_fold_host against a restatement of
// the summation order written here (64 accumulators, ascending slices, six halvings) over every row count and sub-range
// that straddles the accumulator count, a table of -0.0, and every host-side refusal of the wall exchange's entry points.
// Needs no device: the tables it builds are never uploaded (an unfinalized one, and an empty one, whose finalize makes no
// device call).  `make san` at the root builds it against the sanitizer build of the library (ASan + UBSan) and runs it;
// the ordinary build runs it from tests/test_ade_wall_exchange_abi.py.  Exit status 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static double fold64(const std::vector<double>& x) {
  std::vector<double> p(64, 0.0);
  for (size_t i = 0; i < x.size(); ++i) p[i % 64] = p[i % 64] + x[i];  // ascending i = ascending slice per accumulator
  for (int s = 32; s >= 1; s /= 2)
    for (int j = 0; j < s; ++j) p[j] = p[j] + p[j + s];
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
    std::vector<double> table((size_t)LBM_WALLX_NQ * n);
    for (double& v : table) v = (next() - 0.5) * std::pow(10.0, 12.0 * next() - 6.0);
    const int ranges[][2] = {{0, n}, {n > 1 ? 1 : 0, n}, {n / 3, n - n / 4}, {n > 64 ? 63 : 0, n > 64 ? n - 1 : n}};
    for (const auto& rg : ranges) {
      if (rg[0] >= rg[1]) continue;
      double out[LBM_WALLX_NQ];
      const int rc = lbm_ade_wallx_fold_host(out, table.data(), n, rg[0], rg[1]);
      expect(rc == LBM_OK, "lbm_ade_wallx_fold_host returned " + std::to_string(rc));
      for (int q = 0; q < LBM_WALLX_NQ; ++q) {
        const std::vector<double> x(table.begin() + (size_t)q * n + rg[0], table.begin() + (size_t)q * n + rg[1]);
        const double want = fold64(x);
        expect(std::memcmp(&want, &out[q], sizeof want) == 0,
               "fold of rows [" + std::to_string(rg[0]) + ", " + std::to_string(rg[1]) + ") of " + std::to_string(n) + ", slot " + std::to_string(q));
      }
      ++folds;
    }
  }
  {  // a table of -0.0 folds to +0.0: the accumulators start at +0.0
    std::vector<double> zeros((size_t)LBM_WALLX_NQ * 70, -0.0);
    double out[LBM_WALLX_NQ];
    expect(lbm_ade_wallx_fold_host(out, zeros.data(), 70, 0, 70) == LBM_OK, "fold of -0.0");
    const double plus = 0.0;
    for (int q = 0; q < LBM_WALLX_NQ; ++q) expect(std::memcmp(&plus, &out[q], sizeof plus) == 0, "-0.0 folds to +0.0, slot " + std::to_string(q));
    ++folds;
  }

  // every host-side refusal; the pointers are never dereferenced
  double buf[LBM_WALLX_NQ * 8] = {0.0};
  double* p = buf;
  const lbm_geom g{8, 8, 0, 0, 0};
  const lbm_bc bc{0, 0, 0, 0, 0, 1.0, 1.0, 0.0, 0.0};
  const lbm_bgk_params fl{1.2, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, LBM_FORM_DEFAULT};
  const lbm_ade_params sc{1.7, 3e-3, 3e-3, LBM_FORM_DEFAULT};
  auto rows = [&](double* table, int table_rows, int table_row0, const double* fo, const double* go, const lbm_geom* lg,
                  const lbm_ade_iwalls* t, int row_begin, int row_end) {
    return lbm_ade_wallx_rows(table, table_rows, table_row0, fo, go, lg, &bc, &fl, &sc, nullptr, nullptr, t, nullptr,
                              row_begin, row_end, nullptr);
  };
  refused(rows(nullptr, 8, 0, p, p, &g, nullptr, 0, 8), "NULL", "wallx_rows NULL table");
  refused(rows(p, 8, 0, nullptr, p, &g, nullptr, 0, 8), "NULL", "wallx_rows NULL fo");
  refused(rows(p, 8, 0, p, nullptr, &g, nullptr, 0, 8), "NULL", "wallx_rows NULL go");
  refused(rows(p, 8, 0, p, p, nullptr, nullptr, 0, 8), "NULL geometry", "wallx_rows NULL geometry");
  refused(rows(p, 8, 0, p, p, &g, nullptr, 5, 2), "row_begin", "wallx_rows reversed range");
  refused(rows(p, 8, 0, p, p, &g, nullptr, 3, 3), "row_begin", "wallx_rows empty range");
  refused(rows(p, 8, 0, p, p, &g, nullptr, -1, 4), "row_begin", "wallx_rows negative row_begin");
  refused(rows(p, 8, 0, p, p, &g, nullptr, 0, 9), "row_end", "wallx_rows row_end > R");
  refused(rows(p, 8, 1, p, p, &g, nullptr, 0, 8), "table_row0", "wallx_rows rows beyond table_rows");
  refused(rows(p, 8, -1, p, p, &g, nullptr, 0, 8), "table_row0", "wallx_rows negative table_row0");
  refused(rows(p, 0, 0, p, p, &g, nullptr, 0, 8), "table_rows", "wallx_rows table_rows = 0");
  {
    lbm_bgk_params bad = fl;
    bad.omega = 2.5;
    refused(lbm_ade_wallx_rows(p, 8, 0, p, p, &g, &bc, &bad, &sc, nullptr, nullptr, nullptr, nullptr, 0, 8, nullptr), "omega",
            "wallx_rows omega outside (0, 2): the checks of the step");
    lbm_ade_scalar_bc sbc{};
    sbc.mode[0] = LBM_ADE_SCALAR_FIXED;  // FIXED on a periodic row
    refused(lbm_ade_wallx_rows(p, 8, 0, p, p, &g, &bc, &fl, &sc, &sbc, nullptr, nullptr, nullptr, 0, 8, nullptr), "FIXED",
            "wallx_rows FIXED scalar edge on a periodic row");
  }
  lbm_ade_iwalls* open_table = nullptr;  // never finalized
  expect(lbm_ade_iwalls_create(&open_table, 8, 8) == LBM_OK && lbm_ade_iwalls_add(open_table, 2, 2, 0, 1, 3, 0x64u, 0x64u, 0, 0.0) == LBM_OK,
         "building a host table");
  refused(rows(p, 8, 0, p, p, &g, open_table, 0, 8), "not finalized", "wallx_rows unfinalized table");
  lbm_ade_iwalls* other = nullptr;  // empty: finalize makes no device call
  expect(lbm_ade_iwalls_create(&other, 6, 8) == LBM_OK && lbm_ade_iwalls_finalize(other) == LBM_OK, "finalizing an empty table");
  refused(rows(p, 8, 0, p, p, &g, other, 0, 8), "6 x 8", "wallx_rows table built for another R x C");
  lbm_ade_iwalls_destroy(open_table);
  lbm_ade_iwalls_destroy(other);
  refused(lbm_ade_wallx_fold(nullptr, p, 8, 0, 8, nullptr), "NULL", "wallx_fold NULL out");
  refused(lbm_ade_wallx_fold(p, nullptr, 8, 0, 8, nullptr), "NULL", "wallx_fold NULL table");
  refused(lbm_ade_wallx_fold(p, p, 8, 3, 3, nullptr), "row_begin", "wallx_fold empty range");
  refused(lbm_ade_wallx_fold(p, p, 8, 0, 9, nullptr), "row_end", "wallx_fold range outside the table");
  refused(lbm_ade_wallx_fold_host(nullptr, p, 8, 0, 8), "NULL", "wallx_fold_host NULL out");
  refused(lbm_ade_wallx_fold_host(p, nullptr, 8, 0, 8), "NULL", "wallx_fold_host NULL table");
  refused(lbm_ade_wallx_fold_host(p, p, 8, 4, 2), "row_begin", "wallx_fold_host reversed range");
  refused(lbm_ade_wallx_fold_host(p, p, 8, 0, 9), "row_end", "wallx_fold_host range outside the table");
  refused(lbm_ade_wallx_fold_host(p, p, 0, 0, 1), "table_rows", "wallx_fold_host table_rows = 0");
  refused(lbm_ade_solver_wall_exchange(nullptr, nullptr, 0, 8, p, nullptr), "NULL", "solver_wall_exchange NULL solver");
  std::printf("wallx_host_check: %d folds checked, %d failures\n", folds, failures);
  return failures ? 1 : 0;
}
