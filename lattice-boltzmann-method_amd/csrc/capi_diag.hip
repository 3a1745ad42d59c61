// C ABI, diagnostics: reproducible sums / extrema / non-finite count over the dense macroscopic fields (kernels and the
// summation order: diag.hpp), the host fold, and what the solver contexts share for lbm_*_diag and lbm_*_run_until.
#include "diag.hpp"
#include "internal.hpp"

namespace lbm {

int diag_range_check(const char* fn, int R, int row_begin, int row_end) {
  LBM_REQUIRE(row_begin >= 0 && row_begin < row_end && row_end <= R, "%s: row range [%d, %d) is empty or outside 0..%d (row_begin, row_end)",
              fn, row_begin, row_end, R);
  return LBM_OK;
}

static bool diag_is_sum(int q) { return q >= 0 && q < LBM_DIAG_NQ && q != LBM_DIAG_NONFINITE && diag_op(q) == DIAG_ADD; }

int diag_converge_check(const char* fn, const lbm_converge* cv, int max_steps) {
  LBM_REQUIRE(cv, "%s: NULL lbm_converge", fn);
  LBM_REQUIRE(diag_is_sum(cv->quantity), "%s: quantity=%d is not a LBM_DIAG_SUM_* index", fn, cv->quantity);
  LBM_REQUIRE(cv->interval >= 1, "%s: interval=%d must be at least 1", fn, cv->interval);
  LBM_REQUIRE(cv->offset >= 0 && cv->offset < cv->interval, "%s: offset=%d outside 0..interval-1", fn, cv->offset);
  LBM_REQUIRE(cv->tolerance >= 0.0, "%s: tolerance=%g must not be negative", fn, cv->tolerance);  // (refuses NaN too)
  LBM_REQUIRE(max_steps >= 0, "%s: max_steps=%d must not be negative", fn, max_steps);
  LBM_REQUIRE(cv->row_begin >= 0 && cv->row_begin < cv->row_end, "%s: row range [%d, %d) is empty or negative (row_begin, row_end)", fn,
              cv->row_begin, cv->row_end);
  return LBM_OK;
}

static int diag_rows_check(const char* fn, const double* table, int table_rows, int table_row0, const double* rho,
                           const double* u, int R, int C, int row_begin, int row_end) {
  LBM_REQUIRE(table && rho && u, "%s: NULL argument (table, rho, u)", fn);
  LBM_REQUIRE(R > 0 && C > 0, "%s: R=%d, C=%d must be positive", fn, R, C);
  LBM_REQUIRE(table_row0 >= 0 && table_rows > 0 && (long long)table_row0 + R <= table_rows,
              "%s: table_row0=%d + R=%d rows do not fit table_rows=%d", fn, table_row0, R, table_rows);
  return diag_range_check(fn, R, row_begin, row_end);
}

static int diag_rows_launch(double* table, int table_rows, int table_row0, const double* rho, const double* u,
                            const double* conc, const double* profile, int R, int C, int row_begin, int row_end,
                            hipStream_t st) {
  const int cap = tuning("grid_cap", 0);
  const int grid = capped_grid((row_end - row_begin + 3) / 4, cap > 0 ? cap : 8192);
  with_flags([&](auto CONC, auto PROF) {
    LBM_KLAUNCH((k_diag_rows<CONC(), PROF()>), dim3(grid), dim3(256), 0, st, table, table_rows, table_row0, rho, u, conc,
                profile, R, C, row_begin, row_end);
  }, conc != nullptr, profile != nullptr);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

int diag_fold_check(const char* fn, const double* out, const double* table, int table_rows, int row_begin, int row_end) {
  LBM_REQUIRE(out && table, "%s: NULL argument (out, table)", fn);
  LBM_REQUIRE(table_rows > 0, "%s: table_rows=%d must be positive", fn, table_rows);
  return diag_range_check(fn, table_rows, row_begin, row_end);
}

void DiagBuf::release() {
  if (table) (void)hipFree(table);
  if (out_dev) (void)hipFree(out_dev);
  if (pinned) (void)hipHostFree(pinned);
  table = out_dev = pinned = nullptr;
}

int diag_reduce(const char* fn, DiagBuf& buf, const double* rho, const double* u, const double* conc, const double* profile,
                int R, int C, int row_begin, int row_end, double* out_host, double* table_host, hipStream_t st) {
  LBM_REQUIRE(out_host, "%s: NULL out_host", fn);
  int rc = diag_range_check(fn, R, row_begin, row_end);
  if (rc) return rc;
  const size_t table_bytes = (size_t)LBM_DIAG_NQ * R * sizeof(double);
  if (!buf.table) {
    LBM_CHECK_HIP(hipMalloc(&buf.table, table_bytes));
    LBM_CHECK_HIP(hipMalloc(&buf.out_dev, LBM_DIAG_NQ * sizeof(double)));
    LBM_CHECK_HIP(hipHostMalloc(&buf.pinned, LBM_DIAG_NQ * sizeof(double)));
  }
  if (table_host && (row_begin > 0 || row_end < R)) LBM_CHECK_HIP(hipMemsetAsync(buf.table, 0, table_bytes, st));
  rc = diag_rows_launch(buf.table, R, 0, rho, u, conc, profile, R, C, row_begin, row_end, st);
  if (rc) return rc;
  LBM_KLAUNCH(k_diag_fold, dim3(1), dim3(64 * DIAG_FOLD_WAVES), 0, st, buf.out_dev, buf.table, R, row_begin, row_end);
  LBM_CHECK_LAUNCH();
  LBM_CHECK_HIP(hipMemcpyAsync(buf.pinned, buf.out_dev, LBM_DIAG_NQ * sizeof(double), hipMemcpyDeviceToHost, st));
  if (table_host) LBM_CHECK_HIP(hipMemcpyAsync(table_host, buf.table, table_bytes, hipMemcpyDeviceToHost, st));
  LBM_CHECK_HIP(hipStreamSynchronize(st));
  for (int q = 0; q < LBM_DIAG_NQ; ++q) out_host[q] = buf.pinned[q];
  return LBM_OK;
}

}  // namespace lbm

using namespace lbm;

extern "C" {

int lbm_diag_rows(double* table, int table_rows, int table_row0, const double* rho, const double* u, const double* conc,
                  const double* profile, int R, int C, int row_begin, int row_end, lbm_stream_t s) {
  int rc = diag_rows_check("lbm_diag_rows", table, table_rows, table_row0, rho, u, R, C, row_begin, row_end);
  if (rc) return rc;
  return diag_rows_launch(table, table_rows, table_row0, rho, u, conc, profile, R, C, row_begin, row_end, as_stream(s));
}

int lbm_diag_fold(double* out_dev, const double* table, int table_rows, int row_begin, int row_end, lbm_stream_t s) {
  int rc = diag_fold_check("lbm_diag_fold", out_dev, table, table_rows, row_begin, row_end);
  if (rc) return rc;
  LBM_KLAUNCH(k_diag_fold, dim3(1), dim3(64 * DIAG_FOLD_WAVES), 0, as_stream(s), out_dev, table, table_rows, row_begin, row_end);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

int lbm_diag_fold_host(double* out, const double* table_host, int table_rows, int row_begin, int row_end) {
  int rc = diag_fold_check("lbm_diag_fold_host", out, table_host, table_rows, row_begin, row_end);
  if (rc) return rc;
  for (int q = 0; q < LBM_DIAG_NQ; ++q)
    out[q] = diag_fold_one(table_host + (size_t)q * table_rows + row_begin, row_end - row_begin, diag_op(q));
  return LBM_OK;
}

// the wall exchange's table (lbm_hip.h "wall exchange"): LBM_WALLX_NQ sums, the same host fold
int lbm_ade_wallx_fold_host(double* out, const double* table_host, int table_rows, int row_begin, int row_end) {
  int rc = diag_fold_check("lbm_ade_wallx_fold_host", out, table_host, table_rows, row_begin, row_end);
  if (rc) return rc;
  for (int q = 0; q < LBM_WALLX_NQ; ++q)
    out[q] = diag_fold_one(table_host + (size_t)q * table_rows + row_begin, row_end - row_begin, DIAG_ADD);
  return LBM_OK;
}

}  // extern "C"
