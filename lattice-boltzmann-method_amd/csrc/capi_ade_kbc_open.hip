// The fluid + scalar step with a KBC fluid: the open-boundary pass (lbm_ade_open: inlet, outlet, lid, zero-gradient
// copies) and the wall exchange (lbm_ade_wallx_rows_m) -- the launch sites of k_ade_kbc_open_ranges (ade_kbc.hpp) with
// KbcModel and KbcFastModel passive and KbcModel buoyant, and of ade.hpp's k_ade_wall_exchange with both KBC models.  A
// translation unit of its own, so that the device code of the other four KBC units stays what it was.  Host checks and the
// C ABI are capi_ade.hip's (ade_resolve; lbm_ade_open_collide_m, lbm_ade_open_stream_collide_m, lbm_ade_wallx_rows_m and the
// context's setters); the step units reach the open pass as the table pass they hand ade_step_sequence, before the
// interior walls.  Nothing here allocates or synchronises.
#include "ade_kbc_call.hpp"

namespace lbm {

// The open-table pass of the rows `r` (ade_row_ranges), behind the dispatch whose nodes it overwrites and on the same
// stream: one lane per listed node; rows without one enqueue nothing.  *launches += the kernels enqueued
template <bool B, class FM, class SM>
static int ade_kbc_open_launch(const AdeCall& k, const FM& fm, const SM& sm, double* fn, double* gn, const double* fo,
                               const double* go, const AdeRows& r, double* rho, double* u, double* conc, hipStream_t st,
                               long long* launches) {
  const AdeRanges a = ade_row_ranges(k.open_first, r.band0, r.n0, r.band1, r.nrows);
  if (a.w == 0) return LBM_OK;
  with_flags([&](auto M, auto F) {
    LBM_KLAUNCH((k_ade_kbc_open_ranges<FM, SM, M(), F(), B>), dim3((a.w + 255) / 256), dim3(256), 0, st, fn, gn, fo, go, k.g,
                k.bc, fm, sm, rho, u, conc, k.sw, k.by, k.open_nodes, k.open_segs, a.first0, a.w0, a.first1, a.w,
                k.carry_in, k.carry_out);
  }, rho != nullptr, k.sw.fixed);
  LBM_CHECK_LAUNCH();
  ++*launches;
  return LBM_OK;
}

// the open pass of a resolved call with a KBC fluid; call.buoyant: the forced collision, the reference order in both halves
int ade_kbc_open_pass(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, const AdeRows& rows,
                      double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  if (k.n_open_nodes == 0) return LBM_OK;
  if (k.buoyant) {
    const KbcModel fm{k.kbc->s2};
    const AdeModelRef sm{k.scalar->omega_g, k.scalar->w_r, k.scalar->w_c};
    return ade_kbc_open_launch<true>(k, fm, sm, fn, gn, fo, go, rows, rho, u, conc, st, launches);
  }
  return with_ade_kbc_models(k.kbc, k.scalar, [&](const auto& fm, const auto& sm) {
    return ade_kbc_open_launch<false>(k, fm, sm, fn, gn, fo, go, rows, rho, u, conc, st, launches);
  });
}

// The wall exchange of rows [row_begin, row_end) of a resolved call with a KBC fluid (capi_ade.hip's ade_wallx_rows has
// checked and clipped everything): one launch.  The kernel uses the collision's u alone -- in the form of the call; a
// buoyant call takes the reference-order model, whose u is the unshifted u0.
int ade_kbc_wallx_launch(const AdeCall& k, double* table, int table_rows, int table_row0, const double* fo, const double* go,
                         const int* first, const int* region4, int row_begin, int row_end, int grid, hipStream_t st) {
  auto launch = [&](const auto& fm, const auto& sm) {
    using FM = std::decay_t<decltype(fm)>;
    with_flags([&](auto F) {
      LBM_KLAUNCH((k_ade_wall_exchange<FM, F()>), dim3(grid), dim3(256), 0, st, table, table_rows, table_row0, fo, go, k.g,
                  k.bc, fm, sm.wr, sm.wc, k.sw, k.wall_nodes, first, region4[0], region4[1], region4[2], region4[3],
                  row_begin, row_end);
    }, k.sw.fixed);
    LBM_CHECK_LAUNCH();
    return (int)LBM_OK;
  };
  if (k.buoyant) return launch(KbcModel{k.kbc->s2}, AdeModelRef{k.scalar->omega_g, k.scalar->w_r, k.scalar->w_c});
  return with_ade_kbc_models(k.kbc, k.scalar, launch);
}

}  // namespace lbm
