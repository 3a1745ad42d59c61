// C ABI, fluid + transported scalar with the entropic KBC collision as the fluid (lbm_ade_fluid, lbm_hip.h): the `_m`
// entry points.  A BGK fluid forwards to the existing calls of capi_ade.hip; a KBC fluid is checked and launched here --
// the interior pair kernel of ade_kbc.hpp, and ade.hpp's edge, interior-wall and collide-only kernels with a KBC model
// as the fluid.  On a slab the part kernel of ade_kbc.hpp is launched from capi_ade_kbc_part.hip -- a unit of its own, so
// that the device code of this one stays what it was -- and the interior-wall pass of the part's rows from here
// (ade_kbc_iwalls_pass).  Buoyancy on a single block (the `_mb` entry points): the forced collision is launched from
// capi_ade_kbc_buoyant.hip, a unit of its own for the same reason.  No open boundaries, no wall exchange.
#include <cmath>

#include "ade_kbc_call.hpp"

namespace lbm {

// the KBC parameters as lbm_kbc_* checks them, what the step cannot do with this fluid, then every check of the step
// that does not depend on the fluid (ade_resolve with a stand-in BGK fluid that passes; slab: its flag of that name; buoy:
// the buoyancy of a single block, NULL allowed -- call->buoyant then picks the forced collision at the launch sites).  The
// resolved call keeps kbc (borrowed, like scalar): ade_part_from and ade_collide_from launch from it with this fluid.
int ade_kbc_resolve(const char* fn, const lbm_geom* g, const lbm_bc* bc, const lbm_kbc_params* kbc,
                    const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc, const lbm_ade_iwalls* iwalls, bool slab,
                    AdeCall* call, const lbm_ade_buoyancy* buoy) {
  LBM_REQUIRE(kbc, "%s: NULL fluid params", fn);
  LBM_REQUIRE(kbc->s2 > 0.0 && kbc->s2 <= 2.0, "%s: KBC fluid: s2=%g outside (0, 2]", fn, kbc->s2);
  LBM_REQUIRE(kbc->form >= LBM_FORM_DEFAULT && kbc->form <= LBM_FORM_REASSOCIATED, "%s: KBC fluid: form=%d (LBM_FORM_*)", fn,
              kbc->form);
  LBM_REQUIRE(!(bc && bc->pressure_rows), "%s: pressure rows (pressure_rows=%d) are not supported by the fluid + scalar "
              "step with a KBC fluid", fn, bc ? bc->pressure_rows : 0);
  const lbm_bgk_params stand_in{1.0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, LBM_FORM_DEFAULT};
  if (int rc = ade_resolve(fn, g, bc, &stand_in, scalar, sbc, buoy, iwalls, slab, call)) return rc;
  call->fluid = nullptr;  // (the stand-in's lifetime ends here; the KBC launches never read it)
  call->kbc = kbc;
  LBM_REQUIRE(kbc->form == LBM_FORM_DEFAULT || kbc->form == scalar->form,
              "%s: KBC fluid form=%d differs from the scalar form=%d (lbm_ade_params.form sets both halves)", fn, kbc->form,
              scalar->form);
  return LBM_OK;
}

// The interior-wall pass of rows [band0, band0 + n0) and [band1, band1 + nrows - n0) (ade_row_ranges), behind the dispatch
// whose nodes it overwrites and on the same stream: the one launch site of k_ade_iwalls_ranges with a KBC model.  Rows
// without a table node enqueue nothing.  *launches += the kernels enqueued
template <class FM, class SM>
static int ade_kbc_iwalls_launch(const AdeCall& k, const FM& fm, const SM& sm, double* fn, double* gn, const double* fo,
                                 const double* go, int band0, int n0, int band1, int nrows, double* rho, double* u,
                                 double* conc, hipStream_t st, long long* launches) {
  if (k.n_wall_nodes == 0) return LBM_OK;
  const AdeRanges a = ade_row_ranges(k.wall_first, band0, n0, band1, nrows);
  if (a.w == 0) return LBM_OK;
  with_flags([&](auto M, auto F) {
    LBM_KLAUNCH((k_ade_iwalls_ranges<FM, SM, M(), F(), false>), dim3((a.w + 255) / 256), dim3(256), 0, st, fn, gn, fo, go,
                k.g, k.bc, fm, sm, rho, u, conc, k.sw, k.by, k.wall_nodes, a.first0, a.w0, a.first1, a.w);
  }, rho != nullptr, k.sw.fixed);
  LBM_CHECK_LAUNCH();
  ++*launches;
  return LBM_OK;
}

int ade_kbc_iwalls_pass(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, int band0, int n0,
                        int band1, int nrows, double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  return with_ade_kbc_models(k.kbc, k.scalar, [&](const auto& fm, const auto& sm) {
    return ade_kbc_iwalls_launch(k, fm, sm, fn, gn, fo, go, band0, n0, band1, nrows, rho, u, conc, st, launches);
  });
}

// interior launch + (walls only) the edge pass + the interior-wall pass of rows [row_begin, row_end): ade_step_launch's
// sequence (capi_ade.hip) with the pair kernel of this fluid
template <class FM, class SM>
static int ade_kbc_step_launch(const AdeCall& k, const FM& fm, const SM& sm, double* fn, double* gn, const double* fo,
                               const double* go, int row_begin, int row_end, double* rho, double* u, double* conc,
                               hipStream_t st, long long* launches) {
  const bool mom = rho != nullptr;
  const int nt = tuning("nt", 3);  // bit 0: non-temporal loads, bit 1: non-temporal stores
  const int cap = tuning("grid_cap", 0);
  const int tiles = (k.g.C + 511) / 512;
  const long items = (long)(row_end - row_begin) * tiles;
  const int grid = cap > 0 ? capped_grid(items, cap) : (int)(items < (1L << 30) ? items : (1L << 30));
  // the g loads before the fluid's collisions for the reassociated pair (measured: 1.3 % faster at 8192^2), after the f
  // stores for the reference-order pair (ade_kbc.hpp G_EARLY; profiles/ade_kbc.txt)
  constexpr bool kEarly = std::is_same<FM, KbcFastModel>::value;
  with_flags([&](auto NL, auto NS, auto M) {
    LBM_KLAUNCH((k_ade_kbc_stream_collide<FM, SM, NL(), NS(), M(), kEarly>), dim3(grid), dim3(256), 0, st, fn, gn, fo, go, k.g,
                fm, sm, row_begin, row_end, tiles, rho, u, conc);
  }, nt & 1, nt & 2, mom);
  LBM_CHECK_LAUNCH();
  ++*launches;
  if (bc_needs_edge_pass(k.bc)) {
    const int n_edge = 2 * k.g.C + 2 * (row_end - row_begin);
    with_flags([&](auto M, auto F) {
      LBM_KLAUNCH((k_ade_edge<FM, SM, M(), F(), false>), dim3((n_edge + 255) / 256), dim3(256), 0, st, fn, gn, fo, go, k.g,
                  k.bc, fm, sm, row_begin, row_end, rho, u, conc, k.sw, k.by);
    }, mom, k.sw.fixed);
    LBM_CHECK_LAUNCH();
    ++*launches;
  }
  const int nrows = row_end - row_begin;
  return ade_kbc_iwalls_launch(k, fm, sm, fn, gn, fo, go, row_begin, nrows, row_begin, nrows, rho, u, conc, st, launches);
}

int ade_kbc_validate(const char* fn, const lbm_geom* g, const lbm_bc* bc, const lbm_kbc_params* kbc,
                     const lbm_ade_params* scalar) {
  AdeCall k;
  return ade_kbc_resolve(fn, g, bc, kbc, scalar, nullptr, nullptr, false, &k);
}

// collide only: no streaming, so no wall rule -- the scalar's walls and the interior walls are checked and nothing more
int ade_kbc_collide(const char* fn, double* fp, double* gp, const double* f, const double* h, const lbm_geom* lg,
                    const lbm_bc* bc, const lbm_kbc_params* kbc, const lbm_ade_params* scalar,
                    const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls, double* rho,
                    double* u, double* conc, hipStream_t st, long long* launches) {
  AdeCall k;
  int rc = ade_kbc_resolve(fn, lg, bc, kbc, scalar, sbc, iwalls, false, &k, buoy);
  if (!rc) rc = ade_kbc_collide_from(fn, k, fp, gp, f, h, rho, u, conc, st);
  if (!rc && launches) ++*launches;
  return rc;
}

// the collide-only launch of a resolved call (a single block or a slab: the owned rows)
int ade_kbc_collide_from(const char* fn, const AdeCall& k, double* fp, double* gp, const double* f, const double* h,
                         double* rho, double* u, double* conc, hipStream_t st) {
  if (int rc = ade_lattice_args(fn, fp, gp, f, h, rho, u, conc, false)) return rc;
  if (k.buoyant) return ade_kbc_buoyant_collide_from(k, fp, gp, f, h, rho, u, conc, st);
  const long n = (long)k.g.R * k.g.C;
  const int grid = capped_grid((n + 255) / 256);
  return with_ade_kbc_models(k.kbc, k.scalar, [&](const auto& fm, const auto& sm) {
    using FM = std::decay_t<decltype(fm)>;
    using SM = std::decay_t<decltype(sm)>;
    with_flags([&](auto M) {
      LBM_KLAUNCH((k_ade_collide<FM, SM, M(), false>), dim3(grid), dim3(256), 0, st, fp, gp, f, h, k.g, fm, sm, rho, u, conc, k.by);
    }, rho != nullptr);
    LBM_CHECK_LAUNCH();
    return (int)LBM_OK;
  });
}

int ade_kbc_stream_collide(const char* fn, double* fn_, double* gn, const double* fo, const double* go,
                           const lbm_geom* lg, const lbm_bc* bc, const lbm_kbc_params* kbc, const lbm_ade_params* scalar,
                           const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                           int row_begin, int row_end, double* rho, double* u, double* conc, hipStream_t st,
                           long long* launches) {
  AdeCall k;
  int rc = ade_kbc_resolve(fn, lg, bc, kbc, scalar, sbc, iwalls, false, &k, buoy);
  if (!rc) rc = ade_lattice_args(fn, fn_, gn, fo, go, rho, u, conc, true);
  if (rc) return rc;
  LBM_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= lg->R, "%s: row range [%d, %d) outside [0, %d)", fn,
              row_begin, row_end, lg->R);
  if (row_begin == row_end) return LBM_OK;
  long long uncounted = 0;
  if (!launches) launches = &uncounted;
  if (k.buoyant) return ade_kbc_buoyant_step(k, fn_, gn, fo, go, row_begin, row_end, rho, u, conc, st, launches);
  return with_ade_kbc_models(kbc, scalar, [&](const auto& fm, const auto& sm) {
    return ade_kbc_step_launch(k, fm, sm, fn_, gn, fo, go, row_begin, row_end, rho, u, conc, st, launches);
  });
}

int ade_fluid_model(const char* fn, const lbm_ade_fluid* fluid) {
  LBM_REQUIRE(fluid, "%s: NULL fluid (lbm_ade_fluid)", fn);
  LBM_REQUIRE(fluid->model == LBM_MODEL_BGK || fluid->model == LBM_MODEL_KBC,
              "%s: fluid model=%d (LBM_MODEL_BGK or LBM_MODEL_KBC)", fn, fluid->model);
  return LBM_OK;
}

}  // namespace lbm

using namespace lbm;

extern "C" {

int lbm_ade_collide_m(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                      const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc, double* rho,
                      double* u, double* conc, lbm_stream_t s) {
  if (int rc = ade_fluid_model("lbm_ade_collide_m", fluid)) return rc;
  if (fluid->model == LBM_MODEL_BGK)
    return lbm_ade_collide_b(fp, gp, f, g_in, g, bc, &fluid->bgk, scalar, sbc, nullptr, rho, u, conc, s);
  return ade_kbc_collide("lbm_ade_collide_m", fp, gp, f, g_in, g, bc, &fluid->kbc, scalar, sbc, nullptr, nullptr, rho, u,
                         conc, as_stream(s), nullptr);
}

int lbm_ade_collide_mb(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                       const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                       const lbm_ade_buoyancy* buoy, double* rho, double* u, double* conc, lbm_stream_t s) {
  if (int rc = ade_fluid_model("lbm_ade_collide_mb", fluid)) return rc;
  if (fluid->model == LBM_MODEL_BGK)
    return lbm_ade_collide_b(fp, gp, f, g_in, g, bc, &fluid->bgk, scalar, sbc, buoy, rho, u, conc, s);
  return ade_kbc_collide("lbm_ade_collide_mb", fp, gp, f, g_in, g, bc, &fluid->kbc, scalar, sbc, buoy, nullptr, rho, u, conc,
                         as_stream(s), nullptr);
}

int lbm_ade_stream_collide_m(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_iwalls* iwalls, int row_begin, int row_end,
                             double* rho, double* u, double* conc, lbm_stream_t s) {
  if (int rc = ade_fluid_model("lbm_ade_stream_collide_m", fluid)) return rc;
  if (fluid->model == LBM_MODEL_BGK)
    return lbm_ade_stream_collide_w(fn, gn, fo, go, g, bc, &fluid->bgk, scalar, sbc, nullptr, iwalls, row_begin, row_end,
                                    rho, u, conc, s);
  return ade_kbc_stream_collide("lbm_ade_stream_collide_m", fn, gn, fo, go, g, bc, &fluid->kbc, scalar, sbc, nullptr, iwalls,
                                row_begin, row_end, rho, u, conc, as_stream(s), nullptr);
}

int lbm_ade_stream_collide_mb(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                              const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                              const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                              int row_begin, int row_end, double* rho, double* u, double* conc, lbm_stream_t s) {
  if (int rc = ade_fluid_model("lbm_ade_stream_collide_mb", fluid)) return rc;
  if (fluid->model == LBM_MODEL_BGK)
    return lbm_ade_stream_collide_w(fn, gn, fo, go, g, bc, &fluid->bgk, scalar, sbc, buoy, iwalls, row_begin, row_end, rho, u,
                                    conc, s);
  return ade_kbc_stream_collide("lbm_ade_stream_collide_mb", fn, gn, fo, go, g, bc, &fluid->kbc, scalar, sbc, buoy, iwalls,
                                row_begin, row_end, rho, u, conc, as_stream(s), nullptr);
}

int lbm_ade_stream_collide_part_m(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                  const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_iwalls* iwalls, int part, int edge_rows,
                                  double* rho, double* u, double* conc, lbm_stream_t s) {
  const char* name = "lbm_ade_stream_collide_part_m";
  if (int rc = ade_fluid_model(name, fluid)) return rc;
  if (fluid->model == LBM_MODEL_BGK)
    return lbm_ade_stream_collide_part_w(fn, gn, fo, go, g, bc, &fluid->bgk, scalar, sbc, nullptr, iwalls, part, edge_rows,
                                         rho, u, conc, s);
  AdeCall k;
  int rc = ade_kbc_resolve(name, g, bc, &fluid->kbc, scalar, sbc, iwalls, true, &k);
  if (!rc) rc = ade_part_args(name, k, fn, gn, fo, go, part, edge_rows, rho, u, conc);
  return rc ? rc : ade_kbc_part_from(k, fn, gn, fo, go, part, edge_rows, rho, u, conc, as_stream(s));
}

}  // extern "C"
