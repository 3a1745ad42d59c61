// The launch path of the fused fluid + scalar step, once, for the translation units that launch k_ade_* kernels
// (capi_ade.hip: the BGK fluid; capi_ade_kbc.hip, capi_ade_kbc_part.hip, capi_ade_kbc_buoyant.hip,
// capi_ade_kbc_buoyant_part.hip, capi_ade_kbc_open.hip: the KBC fluid -- units of their own because the device code of each is pinned).  Everything here is a template on the models and
// BUOYANT, so a unit instantiates exactly the kernels it asks for: the sequences take the unit's interior launch and its
// table passes as callables and name no interior kernel, no open-table kernel and no model themselves.  Nothing here
// allocates or synchronises: the slab calls are captured into graphs.
#pragma once
#include "ade_call.hpp"

namespace lbm {

// The grid of an interior or part dispatch over nrows rows of C columns: 512-column tiles, every tile a block unless
// "grid_cap" caps the grid; nt: bit 0 non-temporal loads, bit 1 non-temporal stores.  The knobs are read at every launch
// (tests change them between calls).
struct AdeDispatch {
  int grid, tiles, nt;
};
inline AdeDispatch ade_dispatch(int nrows, int C) {
  const int nt = tuning("nt", 3);
  const int cap = tuning("grid_cap", 0);
  const int tiles = (C + 511) / 512;
  const long items = (long)nrows * tiles;
  return AdeDispatch{cap > 0 ? capped_grid(items, cap) : (int)(items < (1L << 30) ? items : (1L << 30)), tiles, nt};
}

// The rows of a launch: [band0, band0 + n0), then [band1, band1 + nrows - n0) where n0 < nrows
struct AdeRows {
  int band0, n0, band1, nrows;
};
// one range [row_begin, row_end)
inline AdeRows ade_rows(int row_begin, int row_end) {
  return AdeRows{row_begin, row_end - row_begin, row_begin, row_end - row_begin};
}
// a part of a slab of R rows -- FRAME: rows [0, E) then [R - E, R); INNER: rows [E, R - E)
inline AdeRows ade_part_rows(int part, int edge_rows, int R) {
  if (part == LBM_ADE_PART_FRAME) return AdeRows{0, edge_rows, R - edge_rows, 2 * edge_rows};
  return AdeRows{edge_rows, R - 2 * edge_rows, R - edge_rows, R - 2 * edge_rows};
}

// collide only, every owned node: no streaming, so no wall rule
template <bool B, class FM, class SM>
int ade_collide_launch(const AdeCall& k, const FM& fm, const SM& sm, double* fp, double* gp, const double* f, const double* h,
                       double* rho, double* u, double* conc, hipStream_t st) {
  const long n = (long)k.g.R * k.g.C;
  const int grid = capped_grid((n + 255) / 256);
  with_flags([&](auto M) { LBM_KLAUNCH((k_ade_collide<FM, SM, M(), B>), dim3(grid), dim3(256), 0, st, fp, gp, f, h, k.g, fm, sm, rho, u, conc, k.by); }, rho != nullptr);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

// The edge pass of rows [row_begin, row_end), behind the interior dispatch and on its stream: one lane per edge node; no
// launch where no edge is a wall.  *launches += the kernels enqueued
template <bool B, class FM, class SM>
int ade_edge_pass(const AdeCall& k, const FM& fm, const SM& sm, double* fn, double* gn, const double* fo, const double* go,
                  int row_begin, int row_end, double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  if (!bc_needs_edge_pass(k.bc)) return LBM_OK;
  const int n_edge = 2 * k.g.C + 2 * (row_end - row_begin);
  with_flags([&](auto M, auto F) {
    LBM_KLAUNCH((k_ade_edge<FM, SM, M(), F(), B>), dim3((n_edge + 255) / 256), dim3(256), 0, st, fn, gn, fo, go, k.g, k.bc, fm,
                sm, row_begin, row_end, rho, u, conc, k.sw, k.by);
  }, rho != nullptr, k.sw.fixed);
  LBM_CHECK_LAUNCH();
  ++*launches;
  return LBM_OK;
}

// The interior-wall pass of the rows `r` (ade_row_ranges), behind the dispatch whose nodes it overwrites and on the same
// stream: one lane per table node; rows without a node enqueue nothing.  *launches += the kernels enqueued
template <bool B, class FM, class SM>
int ade_iwalls_pass(const AdeCall& k, const FM& fm, const SM& sm, double* fn, double* gn, const double* fo, const double* go,
                    const AdeRows& r, double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  if (k.n_wall_nodes == 0) return LBM_OK;
  const AdeRanges a = ade_row_ranges(k.wall_first, r.band0, r.n0, r.band1, r.nrows);
  if (a.w == 0) return LBM_OK;
  with_flags([&](auto M, auto F) {
    LBM_KLAUNCH((k_ade_iwalls_ranges<FM, SM, M(), F(), B>), dim3((a.w + 255) / 256), dim3(256), 0, st, fn, gn, fo, go, k.g,
                k.bc, fm, sm, rho, u, conc, k.sw, k.by, k.wall_nodes, a.first0, a.w0, a.first1, a.w);
  }, rho != nullptr, k.sw.fixed);
  LBM_CHECK_LAUNCH();
  ++*launches;
  return LBM_OK;
}

// The step on rows [row_begin, row_end) of a single block: interior(dispatch) -- the unit's interior kernel with its own
// trailing arguments -- then the edge pass, then tables(rows, launches) -- the unit's table passes of those rows (the
// interior walls; the BGK unit's open table before them).  *launches += the kernels enqueued
template <bool B, class FM, class SM, class Interior, class Tables>
int ade_step_sequence(const AdeCall& k, const FM& fm, const SM& sm, double* fn, double* gn, const double* fo, const double* go,
                      int row_begin, int row_end, double* rho, double* u, double* conc, hipStream_t st, long long* launches,
                      Interior interior, Tables tables) {
  interior(ade_dispatch(row_end - row_begin, k.g.C));
  LBM_CHECK_LAUNCH();
  ++*launches;
  if (int rc = ade_edge_pass<B>(k, fm, sm, fn, gn, fo, go, row_begin, row_end, rho, u, conc, st, launches)) return rc;
  return tables(ade_rows(row_begin, row_end), launches);
}

// kernels the part launches of this process have enqueued (capi_ade.hip: what lbm_ade_part_launches reports)
void ade_part_launches_add(long long n);

// One part of a slab (after ade_part_args): interior(dispatch, rows) -- the unit's part kernel over both row bands, wall
// fix-ups inline, so no edge pass -- then tables(rows, launches) as in the step; the kernels enqueued count in
// lbm_ade_part_launches
template <class Interior, class Tables>
int ade_part_sequence(const AdeCall& k, int part, int edge_rows, Interior interior, Tables tables) {
  const AdeRows r = ade_part_rows(part, edge_rows, k.g.R);
  interior(ade_dispatch(r.nrows, k.g.C), r);
  LBM_CHECK_LAUNCH();
  long long launches = 1;
  const int rc = tables(r, &launches);
  ade_part_launches_add(launches);
  return rc;
}

// What capi_ade.hip's dispatch on the fluid of a resolved call (ade_step_from, ade_part_from, ade_collide_from) hands a KBC
// fluid to -- capi_ade_kbc.hip: the step, the collide-only pass and, for the part unit, the interior-wall pass of a part's
// rows; capi_ade_kbc_part.hip: one part; capi_ade_kbc_buoyant.hip: the step, the collide-only pass and the interior-wall pass
// of a part's rows of a call with call.buoyant (the forced collision, the reference order in both halves);
// capi_ade_kbc_buoyant_part.hip: one part of such a call
int ade_kbc_step(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old, int row_begin,
                 int row_end, double* rho, double* u, double* conc, hipStream_t st, long long* launches);
int ade_kbc_collide_from(const AdeCall& call, double* fp, double* gp, const double* f, const double* h, double* rho, double* u,
                         double* conc, hipStream_t st);
int ade_kbc_iwalls_pass(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old,
                        const AdeRows& rows, double* rho, double* u, double* conc, hipStream_t st, long long* launches);
int ade_kbc_part_from(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old, int part,
                      int edge_rows, double* rho, double* u, double* conc, hipStream_t st);
int ade_kbc_buoyant_step(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old,
                         int row_begin, int row_end, double* rho, double* u, double* conc, hipStream_t st, long long* launches);
int ade_kbc_buoyant_collide_from(const AdeCall& call, double* fp, double* gp, const double* f, const double* h, double* rho,
                                 double* u, double* conc, hipStream_t st);
int ade_kbc_buoyant_iwalls_pass(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old,
                                const AdeRows& rows, double* rho, double* u, double* conc, hipStream_t st, long long* launches);
int ade_kbc_buoyant_part_from(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old,
                              int part, int edge_rows, double* rho, double* u, double* conc, hipStream_t st);
// capi_ade_kbc_open.hip: the open-table pass of the rows of a call with either KBC collision (call.buoyant decides; no
// launch without listed nodes in those rows) -- what the two step units run before their interior-wall pass -- and the one
// launch of the wall exchange (region4: the region clipped to the lattice, first: the table's row index on the device)
int ade_kbc_open_pass(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old,
                      const AdeRows& rows, double* rho, double* u, double* conc, hipStream_t st, long long* launches);
int ade_kbc_wallx_launch(const AdeCall& call, double* table, int table_rows, int table_row0, const double* f_old,
                         const double* g_old, const int* first, const int* region4, int row_begin, int row_end, int grid,
                         hipStream_t st);

}  // namespace lbm
