// Device-side diagnostics: reproducible sums, extrema and a non-finite count over the dense macroscopic fields
// rho [R][C], u [2][R][C], conc [R][C] that every model writes (DESIGN.md "Diagnostics").
//
// The value of a sum is defined by node indices alone -- never by the launch shape, the grid cap or the way rows are
// dealt to slabs:  fold64(x[0..n)) takes 64 accumulators p[j] = +0.0, adds x[j + 64 k] to p[j] for k = 0, 1, ... in
// ascending order (missing elements add nothing), then halves p[j] += p[j + s] for s = 32, 16, 8, 4, 2, 1; the value is
// p[0].  A row value is fold64 over the columns of the per-node term (k_diag_rows: one wave per row, lane j IS
// accumulator j, the halvings are wave shuffles), a range value is fold64 over the row values (k_diag_fold on the
// device, diag_fold_one on the host).  Extrema fold the same way through fmin / fmax from +inf / -inf (NaN
// operands are skipped).  Every addition is an IEEE f64 addition: the library is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "../../include/lbm_hip.h"

namespace lbm {

enum DiagOp { DIAG_ADD = 0, DIAG_MIN = 1, DIAG_MAX = 2 };
__host__ __device__ inline int diag_op(int q) {
  if (q == LBM_DIAG_MIN_RHO || q == LBM_DIAG_MIN_C) return DIAG_MIN;
  if (q == LBM_DIAG_MAX_U2 || q == LBM_DIAG_MAX_RHO || q == LBM_DIAG_MAX_C) return DIAG_MAX;
  return DIAG_ADD;
}
__host__ __device__ inline double diag_identity(int op) {
  return op == DIAG_ADD ? 0.0 : op == DIAG_MIN ? std::numeric_limits<double>::infinity() : -std::numeric_limits<double>::infinity();
}
__host__ __device__ inline double diag_combine(int op, double a, double b) {
  return op == DIAG_ADD ? a + b : op == DIAG_MIN ? fmin(a, b) : fmax(a, b);
}

// fold64 of x[0..n) on one thread (the host fold; the specification restated in the plainest form)
inline double diag_fold_one(const double* x, int n, int op) {
  double p[64];
  for (int j = 0; j < 64; ++j) p[j] = diag_identity(op);
  for (int k = 0; k < n; k += 64)
    for (int j = 0; j < 64 && k + j < n; ++j) p[j] = diag_combine(op, p[j], x[k + j]);
  for (int s = 32; s >= 1; s >>= 1)
    for (int j = 0; j < s; ++j) p[j] = diag_combine(op, p[j], p[j + s]);
  return p[0];
}

// the six halvings across a wave: lane j < s takes p[j] + p[j + s]; the other lanes hold values nobody reads
template <int OP>
__device__ inline double diag_wave_fold(double p) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double o = __shfl_down(p, s, 64);
    p = OP == DIAG_ADD ? p + o : OP == DIAG_MIN ? fmin(p, o) : fmax(p, o);
  }
  return p;
}

// per-lane accumulators of one row
template <bool CONC, bool PROF>
struct DiagAcc {
  double rho = 0.0, ur = 0.0, uc = 0.0, mr = 0.0, mc = 0.0, ke = 0.0, nonfinite = 0.0;
  double max_u2 = -std::numeric_limits<double>::infinity();
  double min_rho = std::numeric_limits<double>::infinity(), max_rho = -std::numeric_limits<double>::infinity();
  double c = 0.0, cur = 0.0, cuc = 0.0, c2 = 0.0, dev2 = 0.0;
  double min_c = std::numeric_limits<double>::infinity(), max_c = -std::numeric_limits<double>::infinity();

  // one node; the terms exactly as the quantity table writes them, left to right
  __device__ inline void add(double r, double a, double b, double cc, double prof) {
    const double u2 = a * a + b * b;
    rho = rho + r;
    ur = ur + a;
    uc = uc + b;
    mr = mr + r * a;
    mc = mc + r * b;
    ke = ke + 0.5 * (r * u2);
    max_u2 = fmax(max_u2, u2);
    min_rho = fmin(min_rho, r);
    max_rho = fmax(max_rho, r);
    bool finite = __builtin_isfinite(r) && __builtin_isfinite(a) && __builtin_isfinite(b);
    if constexpr (CONC) {
      finite = finite && __builtin_isfinite(cc);
      c = c + cc;
      cur = cur + cc * a;
      cuc = cuc + cc * b;
      min_c = fmin(min_c, cc);
      max_c = fmax(max_c, cc);
      c2 = c2 + cc * cc;
    }
    if constexpr (PROF) {
      const double d = a - prof;
      dev2 = dev2 + d * d;
    }
    nonfinite = nonfinite + (finite ? 0.0 : 1.0);
  }
};

// One wave per row, four rows per workgroup of 256 threads, grid-strided over rows [row_begin, row_end).  Lane j walks
// columns j + 64 k: each wave load is 512 contiguous bytes per field.  k is unrolled by UNROLL with the loads issued
// before the additions (several loads in flight), the additions of each accumulator staying in ascending k.  Lane 0
// writes the LBM_DIAG_NQ row values to table[q * table_rows + table_row0 + r].  No atomics, no LDS, no scratch.
template <bool CONC, bool PROF>
__global__ __launch_bounds__(256) void k_diag_rows(double* __restrict__ table, int table_rows, int table_row0,
                                                   const double* __restrict__ rho, const double* __restrict__ u,
                                                   const double* __restrict__ conc, const double* __restrict__ profile,
                                                   int R, int C, int row_begin, int row_end) {
  constexpr int UNROLL = 4;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const double* __restrict__ ur_p = u;
  const double* __restrict__ uc_p = u + (size_t)R * C;
  for (long long r = row_begin + (long long)blockIdx.x * 4 + wave; r < row_end; r += (long long)gridDim.x * 4) {
    const size_t base = (size_t)r * C;
    DiagAcc<CONC, PROF> acc;
    int c = lane;
    // full groups of UNROLL slices: every lane of the wave has all UNROLL columns (c - lane is wave-uniform)
    for (; c - lane + 64 * UNROLL <= C; c += 64 * UNROLL) {
      double vr[UNROLL], va[UNROLL], vb[UNROLL], vc[UNROLL], vp[UNROLL];
#pragma unroll
      for (int i = 0; i < UNROLL; ++i) {
        const size_t at = base + c + 64 * i;
        vr[i] = rho[at];
        va[i] = ur_p[at];
        vb[i] = uc_p[at];
        vc[i] = CONC ? conc[at] : 0.0;
        vp[i] = PROF ? profile[c + 64 * i] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < UNROLL; ++i) acc.add(vr[i], va[i], vb[i], vc[i], vp[i]);
    }
    // the remaining slices, the ragged last one included (a lane without a column adds nothing)
    for (; c < C; c += 64) {
      const size_t at = base + c;
      acc.add(rho[at], ur_p[at], uc_p[at], CONC ? conc[at] : 0.0, PROF ? profile[c] : 0.0);
    }
    double out[LBM_DIAG_NQ];
    out[LBM_DIAG_SUM_RHO] = diag_wave_fold<DIAG_ADD>(acc.rho);
    out[LBM_DIAG_SUM_UR] = diag_wave_fold<DIAG_ADD>(acc.ur);
    out[LBM_DIAG_SUM_UC] = diag_wave_fold<DIAG_ADD>(acc.uc);
    out[LBM_DIAG_SUM_MR] = diag_wave_fold<DIAG_ADD>(acc.mr);
    out[LBM_DIAG_SUM_MC] = diag_wave_fold<DIAG_ADD>(acc.mc);
    out[LBM_DIAG_SUM_KE] = diag_wave_fold<DIAG_ADD>(acc.ke);
    out[LBM_DIAG_MAX_U2] = diag_wave_fold<DIAG_MAX>(acc.max_u2);
    out[LBM_DIAG_MIN_RHO] = diag_wave_fold<DIAG_MIN>(acc.min_rho);
    out[LBM_DIAG_MAX_RHO] = diag_wave_fold<DIAG_MAX>(acc.max_rho);
    out[LBM_DIAG_NONFINITE] = diag_wave_fold<DIAG_ADD>(acc.nonfinite);
    if constexpr (CONC) {
      out[LBM_DIAG_SUM_C] = diag_wave_fold<DIAG_ADD>(acc.c);
      out[LBM_DIAG_SUM_CUR] = diag_wave_fold<DIAG_ADD>(acc.cur);
      out[LBM_DIAG_SUM_CUC] = diag_wave_fold<DIAG_ADD>(acc.cuc);
      out[LBM_DIAG_MIN_C] = diag_wave_fold<DIAG_MIN>(acc.min_c);
      out[LBM_DIAG_MAX_C] = diag_wave_fold<DIAG_MAX>(acc.max_c);
      out[LBM_DIAG_SUM_C2] = diag_wave_fold<DIAG_ADD>(acc.c2);
    } else {
#pragma unroll
      for (int q = LBM_DIAG_SUM_C; q <= LBM_DIAG_SUM_C2; ++q) out[q] = 0.0;
    }
    out[LBM_DIAG_SUM_DEV2] = PROF ? diag_wave_fold<DIAG_ADD>(acc.dev2) : 0.0;
    if (lane == 0) {
      double* __restrict__ t = table + table_row0 + r;
#pragma unroll
      for (int q = 0; q < LBM_DIAG_NQ; ++q) t[(size_t)q * table_rows] = out[q];
    }
  }
}

// Rows [row_begin, row_end) of the table to LBM_DIAG_NQ values: ONE workgroup of DIAG_FOLD_WAVES waves, wave w folds
// quantities w, w + DIAG_FOLD_WAVES, ... with lane j as accumulator j.  The slices are loaded four at a time (the loads
// in flight together) and combined in ascending order.
constexpr int DIAG_FOLD_WAVES = 16;
__global__ __launch_bounds__(64 * DIAG_FOLD_WAVES) void k_diag_fold(double* __restrict__ out, const double* __restrict__ table,
                                                                    int table_rows, int row_begin, int row_end) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  for (int q = wave; q < LBM_DIAG_NQ; q += DIAG_FOLD_WAVES) {
    const int op = diag_op(q);
    const double* __restrict__ x = table + (size_t)q * table_rows;
    double p = diag_identity(op);
    int r = row_begin + lane;
    for (; r - lane + 256 <= row_end; r += 256) {  // four full slices (r - lane is wave-uniform)
      const double a = x[r], b = x[r + 64], c = x[r + 128], d = x[r + 192];
      p = diag_combine(op, diag_combine(op, diag_combine(op, diag_combine(op, p, a), b), c), d);
    }
    for (; r < row_end; r += 64) p = diag_combine(op, p, x[r]);
    p = op == DIAG_ADD ? diag_wave_fold<DIAG_ADD>(p) : op == DIAG_MIN ? diag_wave_fold<DIAG_MIN>(p) : diag_wave_fold<DIAG_MAX>(p);
    if (lane == 0) out[q] = p;
  }
}

}  // namespace lbm
