// The fluid + scalar step with a KBC fluid and BUOYANCY (lbm_ade_buoyancy with beta != (0, 0)) on a single block: the
// launch sites of every kernel with the forced KBC collision -- the buoyant interior pair kernel of ade_kbc.hpp and the
// BUOYANT instantiations of ade.hpp's collide-only, edge and interior-wall kernels with KbcModel as the fluid
// (ade_forced_fluid: collide_with on the shifted u).  A translation unit of its own, so that the device code of
// capi_ade_kbc.hip and capi_ade_kbc_part.hip stays what it was.  A buoyant step runs the reference order in both halves
// whatever `form` says: KbcModel + AdeModelRef.  Called from capi_ade_kbc.hip with a call ade_kbc_resolve resolved.
#include "ade_kbc_call.hpp"

namespace lbm {

// the collide-only launch of a resolved buoyant call (the first driver iteration)
int ade_kbc_buoyant_collide_from(const AdeCall& k, double* fp, double* gp, const double* f, const double* h, double* rho,
                                 double* u, double* conc, hipStream_t st) {
  const KbcModel fm{k.kbc->s2};
  const AdeModelRef sm{k.scalar->omega_g, k.scalar->w_r, k.scalar->w_c};
  const long n = (long)k.g.R * k.g.C;
  const int grid = capped_grid((n + 255) / 256);
  with_flags([&](auto M) {
    LBM_KLAUNCH((k_ade_collide<KbcModel, AdeModelRef, M(), true>), dim3(grid), dim3(256), 0, st, fp, gp, f, h, k.g, fm, sm, rho,
                u, conc, k.by);
  }, rho != nullptr);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

// interior launch + (walls only) the edge pass + the interior-wall pass of rows [row_begin, row_end): ade_kbc_step_launch's
// sequence (capi_ade_kbc.hip) with the buoyant kernels; *launches += the kernels enqueued
int ade_kbc_buoyant_step(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, int row_begin,
                         int row_end, double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  const KbcModel fm{k.kbc->s2};
  const AdeModelRef sm{k.scalar->omega_g, k.scalar->w_r, k.scalar->w_c};
  const bool mom = rho != nullptr;
  const int nt = tuning("nt", 3);  // bit 0: non-temporal loads, bit 1: non-temporal stores
  const int cap = tuning("grid_cap", 0);
  const int tiles = (k.g.C + 511) / 512;
  const long items = (long)(row_end - row_begin) * tiles;
  const int grid = cap > 0 ? capped_grid(items, cap) : (int)(items < (1L << 30) ? items : (1L << 30));
  with_flags([&](auto NL, auto NS, auto M) {
    LBM_KLAUNCH((k_ade_kbc_stream_collide_buoyant<KbcModel, AdeModelRef, NL(), NS(), M()>), dim3(grid), dim3(256), 0, st, fn, gn,
                fo, go, k.g, fm, sm, row_begin, row_end, tiles, rho, u, conc, k.by);
  }, nt & 1, nt & 2, mom);
  LBM_CHECK_LAUNCH();
  ++*launches;
  if (bc_needs_edge_pass(k.bc)) {
    const int n_edge = 2 * k.g.C + 2 * (row_end - row_begin);
    with_flags([&](auto M, auto F) {
      LBM_KLAUNCH((k_ade_edge<KbcModel, AdeModelRef, M(), F(), true>), dim3((n_edge + 255) / 256), dim3(256), 0, st, fn, gn, fo,
                  go, k.g, k.bc, fm, sm, row_begin, row_end, rho, u, conc, k.sw, k.by);
    }, mom, k.sw.fixed);
    LBM_CHECK_LAUNCH();
    ++*launches;
  }
  if (k.n_wall_nodes == 0) return LBM_OK;
  const int nrows = row_end - row_begin;
  const AdeRanges a = ade_row_ranges(k.wall_first, row_begin, nrows, row_begin, nrows);
  if (a.w == 0) return LBM_OK;
  with_flags([&](auto M, auto F) {
    LBM_KLAUNCH((k_ade_iwalls_ranges<KbcModel, AdeModelRef, M(), F(), true>), dim3((a.w + 255) / 256), dim3(256), 0, st, fn, gn,
                fo, go, k.g, k.bc, fm, sm, rho, u, conc, k.sw, k.by, k.wall_nodes, a.first0, a.w0, a.first1, a.w);
  }, mom, k.sw.fixed);
  LBM_CHECK_LAUNCH();
  ++*launches;
  return LBM_OK;
}

}  // namespace lbm
