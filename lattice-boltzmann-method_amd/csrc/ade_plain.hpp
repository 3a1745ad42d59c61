// ade.hpp's kernels that are no templates: one definition each in the library, so ONE unit includes this file
// (capi_ade.hip, which launches them); ade.hpp itself is shared with capi_ade_kbc.hip.
#pragma once
#include "ade.hpp"

namespace lbm {

// The FIXED edges of the lazily streamed scalar (lbm_ade_solver_get_state): hs = stream(post-collision g) with the
// gather modes of ade_scalar_gather_bc; u = [2][R][C] dense, the reference-order calc_u of the streamed f.  One thread per
// node of the perimeter (rows 0 and R-1, then columns 0 and C-1 without the corners), each node once.
__global__ __launch_bounds__(256) void k_ade_fixed_state(double* __restrict__ hs, Geom g, Bc bc, AdeWalls sw,
                                                         const double* __restrict__ u, double wr, double wc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, inner = g.R > 2 ? g.R - 2 : 0;
  int r, c;
  if (i < g.C) { r = 0; c = i; }
  else if (i < 2 * g.C) { r = g.R - 1; c = i - g.C; if (g.R == 1) return; }
  else if (i < 2 * g.C + inner) { r = 1 + i - 2 * g.C; c = 0; }
  else if (i < 2 * g.C + 2 * inner) { r = 1 + i - 2 * g.C - inner; c = g.C - 1; }
  else return;
  const long o = g.at(r, c), n = (long)g.R * g.C, d = (long)r * g.C + c;
  double h[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) h[q] = hs[q * g.plane + o];
  ade_fixed_walls(h, g, bc, sw, r, c, u[d], u[n + d], wr, wc);
#pragma unroll
  for (int q = 0; q < Q; ++q) hs[q * g.plane + o] = h[q];
}

// Rows [row_begin, row_end) of a wall-exchange table to LBM_WALLX_NQ values: ONE workgroup of LBM_WALLX_NQ waves, wave q
// folds quantity q with lane j as accumulator j -- k_diag_fold's fold for sums alone: the slices are loaded four at a time
// (the loads in flight together) and added in ascending order.
__global__ __launch_bounds__(64 * LBM_WALLX_NQ) void k_ade_wallx_fold(double* __restrict__ out,
                                                                     const double* __restrict__ table, int table_rows,
                                                                     int row_begin, int row_end) {
  const int lane = threadIdx.x & 63;
  const int q = threadIdx.x >> 6;
  const double* __restrict__ x = table + (size_t)q * table_rows;
  double p = 0.0;
  int r = row_begin + lane;
  for (; r - lane + 256 <= row_end; r += 256) {  // four full slices (r - lane is wave-uniform)
    const double a = x[r], b = x[r + 64], c = x[r + 128], d = x[r + 192];
    p = (((p + a) + b) + c) + d;
  }
  for (; r < row_end; r += 64) p = p + x[r];
  p = ade_wave_sum(p);
  if (lane == 0) out[q] = p;
}

// The carry of a PRE-collision state (lbm_ade_collide_o, lbm_ade_solver_set_state): u = calc_u(f, calc_rho(f)) of every
// listed node, in the reference order -- what the first streamed step reads as carry_in.
__global__ __launch_bounds__(256) void k_ade_open_prime(const double* __restrict__ f_in, Geom g,
                                                        const AdeOpenNode* __restrict__ nodes, int n_nodes,
                                                        double* __restrict__ carry_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const long o = g.at(nodes[i].r, nodes[i].c);
  double f[Q], rho, ux, uy;
#pragma unroll
  for (int q = 0; q < Q; ++q) f[q] = f_in[q * g.plane + o];
  ade_fluid_moments(f, rho, ux, uy);
  carry_out[2 * i] = ux;
  carry_out[2 * i + 1] = uy;
}

}  // namespace lbm
