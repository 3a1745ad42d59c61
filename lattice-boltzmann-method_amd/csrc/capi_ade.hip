// C ABI, fluid + transported scalar: the compressible BGK fluid f and the advection-diffusion scalar g of
// test/rectangle_sedimentation_test.cpp:88-247 in one fused pull step per node (ade.hpp), and the solver
// context that runs the driver loop on one block.
#include <cmath>
#include <cstdint>
#include <new>
#include <type_traits>

#include "ade.hpp"
#include "launch.hpp"

namespace lbm {

static const char* edge_name(int m) {
  switch (m) {
    case LBM_EDGE_PERIODIC: return "PERIODIC";
    case LBM_EDGE_HALO: return "HALO";
    case LBM_EDGE_BOUNCE_BACK: return "BOUNCE_BACK";
    case LBM_EDGE_SPECULAR: return "SPECULAR";
    case LBM_EDGE_ABB_VELOCITY: return "ABB_VELOCITY";
    case LBM_EDGE_WRAP_NOSHIFT: return "WRAP_NOSHIFT";
    default: return "unknown";
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Everything the fused step accepts, checked on the host before any device call.  Single block (slab = false): ghost
// 0, rows PERIODIC or BOUNCE_BACK.  Slab (the part launches and the ring): ghost 0 with PERIODIC or BOUNCE_BACK rows, or
// ghost >= 1 with HALO or BOUNCE_BACK rows -- ghost rows are read where a row edge is HALO and nothing wraps.  Columns:
// PERIODIC, BOUNCE_BACK or SPECULAR.  The scalar takes the fluid's fix-up at every wall.
static int ade_validate(const char* fn, const lbm_geom* g, const lbm_bc* bc, const lbm_bgk_params* fluid,
                        const lbm_ade_params* scalar, bool slab = false) {
  LBM_REQUIRE(g, "%s: NULL geometry", fn);
  LBM_REQUIRE(g->R >= 1 && g->C >= 1, "%s: R=%d C=%d must be positive", fn, g->R, g->C);
  if (slab) LBM_REQUIRE(g->ghost >= 0 && g->ghost <= 15, "%s: ghost=%d must be 0..15", fn, g->ghost);
  else LBM_REQUIRE(g->ghost == 0, "%s: ghost=%d: the fluid + scalar step runs on a single block (ghost = 0)", fn, g->ghost);
  LBM_REQUIRE(g->C % 2 == 0, "%s: C=%d must be even (two nodes per lane)", fn, g->C);
  LBM_REQUIRE(g->row_pitch == 0 || (g->row_pitch >= g->C && g->row_pitch % 2 == 0),
              "%s: row_pitch=%d must be even and >= C=%d (0 = dense)", fn, g->row_pitch, g->C);
  const long long pitch = g->row_pitch > 0 ? g->row_pitch : g->C;
  LBM_REQUIRE(g->plane_stride == 0 || (g->plane_stride >= (long long)(g->R + 2 * g->ghost) * pitch && g->plane_stride % 2 == 0),
              "%s: plane_stride=%lld must be even and at least a plane (0 = dense)", fn, g->plane_stride);
  if (slab && g->ghost > 0)
    LBM_REQUIRE(bc && bc->row_lo != LBM_EDGE_PERIODIC && bc->row_hi != LBM_EDGE_PERIODIC,
                "%s: ghost=%d: a slab's row edges are HALO or BOUNCE_BACK (row edge mode PERIODIC given: nothing wraps "
                "where there are ghost rows)", fn, g->ghost);
  if (bc) {
    LBM_REQUIRE(bc->pressure_rows == 0, "%s: pressure_rows=%d not supported by the fluid + scalar step", fn,
                bc->pressure_rows);
    auto row_ok = [](int m) { return m == LBM_EDGE_PERIODIC || m == LBM_EDGE_BOUNCE_BACK; };
    auto col_ok = [](int m) { return m == LBM_EDGE_PERIODIC || m == LBM_EDGE_BOUNCE_BACK || m == LBM_EDGE_SPECULAR; };
    if (slab) {
      for (int m : {bc->row_lo, bc->row_hi}) {
        LBM_REQUIRE(m != LBM_EDGE_HALO || g->ghost > 0, "%s: row edge mode HALO needs ghost rows (ghost=0)", fn);
        LBM_REQUIRE(row_ok(m) || m == LBM_EDGE_HALO,
                    "%s: row edge mode %s (%d) not supported (PERIODIC, HALO or BOUNCE_BACK)", fn, edge_name(m), m);
      }
    }
    LBM_REQUIRE(slab || row_ok(bc->row_lo), "%s: row edge mode %s (%d) not supported (PERIODIC or BOUNCE_BACK)", fn,
                edge_name(bc->row_lo), bc->row_lo);
    LBM_REQUIRE(slab || row_ok(bc->row_hi), "%s: row edge mode %s (%d) not supported (PERIODIC or BOUNCE_BACK)", fn,
                edge_name(bc->row_hi), bc->row_hi);
    LBM_REQUIRE(col_ok(bc->col_lo), "%s: column edge mode %s (%d) not supported (PERIODIC, BOUNCE_BACK or SPECULAR)",
                fn, edge_name(bc->col_lo), bc->col_lo);
    LBM_REQUIRE(col_ok(bc->col_hi), "%s: column edge mode %s (%d) not supported (PERIODIC, BOUNCE_BACK or SPECULAR)",
                fn, edge_name(bc->col_hi), bc->col_hi);
  }
  LBM_REQUIRE(fluid, "%s: NULL fluid params", fn);
  LBM_REQUIRE(fluid->omega > 0.0 && fluid->omega < 2.0, "%s: omega=%g outside (0, 2)", fn, fluid->omega);
  LBM_REQUIRE(fluid->incompressible == 0, "%s: incompressible=%d: the fluid is the compressible BGK model", fn,
              fluid->incompressible);
  LBM_REQUIRE(fluid->force_mode == 0, "%s: force_mode=%d: no body force in the fluid + scalar step", fn,
              fluid->force_mode);
  LBM_REQUIRE(fluid->delta_form == 0, "%s: delta_form=%d not supported by the fluid + scalar step", fn, fluid->delta_form);
  LBM_REQUIRE(fluid->form >= LBM_FORM_DEFAULT && fluid->form <= LBM_FORM_REASSOCIATED, "%s: fluid form=%d (LBM_FORM_*)",
              fn, fluid->form);
  LBM_REQUIRE(scalar, "%s: NULL scalar params", fn);
  LBM_REQUIRE(scalar->omega_g > 0.0 && scalar->omega_g < 2.0, "%s: omega_g=%g outside (0, 2)", fn, scalar->omega_g);
  LBM_REQUIRE(scalar->form >= LBM_FORM_DEFAULT && scalar->form <= LBM_FORM_REASSOCIATED,
              "%s: scalar form=%d (LBM_FORM_*)", fn, scalar->form);
  LBM_REQUIRE(fluid->form == LBM_FORM_DEFAULT || fluid->form == scalar->form,
              "%s: fluid form=%d differs from the scalar form=%d (lbm_ade_params.form sets both halves)", fn, fluid->form,
              scalar->form);
  return LBM_OK;
}

// one form for both halves, lbm_ade_params.form; LBM_FORM_DEFAULT resolves through "bgk_fast", as for BGK
static bool ade_fast(const lbm_ade_params* scalar) {
  return scalar->form == LBM_FORM_DEFAULT ? tuning("bgk_fast", 1) != 0 : scalar->form == LBM_FORM_REASSOCIATED;
}

// The buoyancy (lbm_ade_buoyancy, NULL allowed) on the host: every field finite.  *by receives the device copy and
// *buoyant whether the step is a buoyant one -- beta = (0, 0), like NULL, is the passive step.
static int ade_buoyancy_check(const char* fn, const lbm_ade_buoyancy* b, AdeBuoyancy* by, bool* buoyant) {
  *by = AdeBuoyancy{};
  *buoyant = false;
  if (!b) return LBM_OK;
  LBM_REQUIRE(std::isfinite(b->beta_r) && std::isfinite(b->beta_c), "%s: buoyancy beta=(%g, %g) must be finite", fn,
              b->beta_r, b->beta_c);
  LBM_REQUIRE(std::isfinite(b->c_ref), "%s: buoyancy c_ref=%g must be finite", fn, b->c_ref);
  LBM_REQUIRE(std::isfinite(b->u_shift), "%s: buoyancy u_shift=%g must be finite", fn, b->u_shift);
  LBM_REQUIRE(std::isfinite(b->guo_a) && std::isfinite(b->guo_b), "%s: buoyancy guo=(%g, %g) must be finite", fn,
              b->guo_a, b->guo_b);
  *by = AdeBuoyancy{b->beta_r, b->beta_c, b->c_ref, b->u_shift, b->guo_a, b->guo_b};
  *buoyant = b->beta_r != 0.0 || b->beta_c != 0.0;
  return LBM_OK;
}

// f(fluid model, scalar model, BUOYANT): the reassociated pair or the reference-order pair; a buoyant step is the
// reference-order pair whatever the form
template <class F>
static int with_ade_models(const lbm_bgk_params* fluid, const lbm_ade_params* scalar, bool buoyant, F f) {
  if (buoyant)
    return f(BgkModelT<0, 0>{fluid->omega}, AdeModelRef{scalar->omega_g, scalar->w_r, scalar->w_c}, std::true_type{});
  if (ade_fast(scalar))
    return f(BgkFastModel(fluid->omega), AdeFastModel(scalar->omega_g, scalar->w_r, scalar->w_c), std::false_type{});
  return f(BgkModelT<0, 0>{fluid->omega}, AdeModelRef{scalar->omega_g, scalar->w_r, scalar->w_c}, std::false_type{});
}

// The lattice and field arguments of a launch: four lattices given (distinct: also pairwise different and 16-byte
// aligned -- the collide-only launch reads and writes node by node and asks for neither); rho, u, conc all or none.
static int ade_lattice_args(const char* fn, const double* fn_, const double* gn, const double* fo, const double* go,
                            const double* rho, const double* u, const double* conc, bool distinct) {
  LBM_REQUIRE(fn_ && gn && fo && go, "%s: NULL lattice", fn);
  if (distinct) {
    LBM_REQUIRE(fn_ != fo && fn_ != go && gn != fo && gn != go && fn_ != gn && fo != go, "%s: aliased lattices", fn);
    LBM_REQUIRE(aligned16(fn_) && aligned16(gn) && aligned16(fo) && aligned16(go), "%s: lattices must be 16-byte aligned", fn);
  }
  LBM_REQUIRE((rho == nullptr) == (u == nullptr) && (rho == nullptr) == (conc == nullptr),
              "%s: rho, u and conc must all be given or all be NULL", fn);
  return LBM_OK;
}

static const char* const kEdge[4] = {"row_lo", "row_hi", "col_lo", "col_hi"};

// The scalar's walls (lbm_ade_scalar_bc) against the edges `bc` the launch runs with, on the host: a FIXED edge must be a
// wall of the fluid there -- a BOUNCE_BACK row, a BOUNCE_BACK or SPECULAR column.  *sw receives the device copy.
static int ade_scalar_bc_check(const char* fn, const lbm_ade_scalar_bc* sbc, const lbm_bc* bc, AdeWalls* sw) {
  *sw = AdeWalls{};
  if (!sbc) return LBM_OK;
  const int modes[4] = {bc ? bc->row_lo : LBM_EDGE_PERIODIC, bc ? bc->row_hi : LBM_EDGE_PERIODIC,
                        bc ? bc->col_lo : LBM_EDGE_PERIODIC, bc ? bc->col_hi : LBM_EDGE_PERIODIC};
  for (int e = 0; e < 4; ++e) {
    const int m = sbc->mode[e];
    LBM_REQUIRE(m == LBM_ADE_SCALAR_NO_FLUX || m == LBM_ADE_SCALAR_FIXED,
                "%s: scalar edge %s: mode=%d (LBM_ADE_SCALAR_NO_FLUX or LBM_ADE_SCALAR_FIXED)", fn, kEdge[e], m);
    if (m != LBM_ADE_SCALAR_FIXED) continue;
    const bool wall = modes[e] == LBM_EDGE_BOUNCE_BACK || (e >= 2 && modes[e] == LBM_EDGE_SPECULAR);
    LBM_REQUIRE(wall, "%s: scalar edge %s: FIXED on a %s (%d) edge (a BOUNCE_BACK row, a BOUNCE_BACK or SPECULAR column)",
                fn, kEdge[e], edge_name(modes[e]), modes[e]);
    LBM_REQUIRE(std::isfinite(sbc->conc[e]), "%s: scalar edge %s: conc=%g must be finite", fn, kEdge[e], sbc->conc[e]);
    LBM_REQUIRE(((uintptr_t)sbc->profile[e] & 7u) == 0, "%s: scalar edge %s: profile %p must be 8-byte aligned", fn,
                kEdge[e], (const void*)sbc->profile[e]);
    sw->fixed |= 1 << e;
    sw->conc[e] = sbc->conc[e];
    sw->profile[e] = sbc->profile[e];
  }
  return LBM_OK;
}

template <bool B, class FM, class SM>
static int ade_collide_launch(double* fp, double* gp, const double* f, const double* h, const Geom& g, const FM& fm,
                              const SM& sm, const AdeBuoyancy& by, double* rho, double* u, double* conc, hipStream_t st) {
  const long n = (long)g.R * g.C;
  const int grid = capped_grid((n + 255) / 256);
  with_flags([&](auto M) { LBM_KLAUNCH((k_ade_collide<FM, SM, M(), B>), dim3(grid), dim3(256), 0, st, fp, gp, f, h, g, fm, sm, rho, u, conc, by); }, rho != nullptr);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

// interior launch + (walls only) the edge pass; *launches += the kernels enqueued
template <bool B, class FM, class SM>
static int ade_step_launch(double* fn, double* gn, const double* fo, const double* go, const Geom& g, const Bc& bc,
                           const FM& fm, const SM& sm, const AdeWalls& sw, const AdeBuoyancy& by, int row_begin,
                           int row_end, double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  const bool mom = rho != nullptr;
  const int nt = tuning("nt", 3);  // bit 0: non-temporal loads, bit 1: non-temporal stores
  const int cap = tuning("grid_cap", 0);
  const int tiles = (g.C + 511) / 512;
  const long items = (long)(row_end - row_begin) * tiles;
  const int grid = cap > 0 ? capped_grid(items, cap) : (int)(items < (1L << 30) ? items : (1L << 30));
  with_flags([&](auto NL, auto NS, auto M) {
    LBM_KLAUNCH((k_ade_stream_collide<FM, SM, NL(), NS(), M(), B>), dim3(grid), dim3(256), 0, st, fn, gn, fo, go, g, fm,
                sm, row_begin, row_end, tiles, rho, u, conc, by);
  }, nt & 1, nt & 2, mom);
  LBM_CHECK_LAUNCH();
  ++*launches;
  if (bc_needs_edge_pass(bc)) {
    const int n_edge = 2 * g.C + 2 * (row_end - row_begin);
    const dim3 grid_e((n_edge + 255) / 256);
    with_flags([&](auto M, auto F) {
      LBM_KLAUNCH((k_ade_edge<FM, SM, M(), F(), B>), grid_e, dim3(256), 0, st, fn, gn, fo, go, g, bc, fm, sm, row_begin,
                  row_end, rho, u, conc, sw, by);
    }, mom, sw.fixed);
    LBM_CHECK_LAUNCH();
    ++*launches;
  }
  return LBM_OK;
}

// one dispatch over rows [band0, band0 + n0) and [band1, band1 + nrows - n0), wall fix-ups inline
template <bool B, class FM, class SM>
static int ade_part_launch(double* fn, double* gn, const double* fo, const double* go, const Geom& g, const Bc& bc,
                           const FM& fm, const SM& sm, const AdeWalls& sw, const AdeBuoyancy& by, int band0, int n0,
                           int band1, int nrows, double* rho, double* u, double* conc, hipStream_t st) {
  const bool mom = rho != nullptr;
  const int nt = tuning("nt", 3);  // as the single-block step
  const int cap = tuning("grid_cap", 0);
  const int tiles = (g.C + 511) / 512;
  const long items = (long)nrows * tiles;
  const int grid = cap > 0 ? capped_grid(items, cap) : (int)(items < (1L << 30) ? items : (1L << 30));
  with_flags([&](auto NL, auto NS, auto M, auto F) {
    LBM_KLAUNCH((k_ade_stream_collide_part<FM, SM, NL(), NS(), M(), F(), B>), dim3(grid), dim3(256), 0, st, fn, gn, fo, go,
                g, bc, fm, sm, band0, n0, band1, nrows, tiles, rho, u, conc, sw, by);
  }, nt & 1, nt & 2, mom, sw.fixed);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

// collide only: no streaming, so no wall rule -- the scalar's walls (sbc) are checked and nothing more
static int ade_collide(const char* fn, double* fp, double* gp, const double* f, const double* h, const lbm_geom* lg,
                       const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                       const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, double* rho, double* u, double* conc,
                       hipStream_t st, bool slab = false) {
  AdeWalls sw;
  AdeBuoyancy by;
  bool buoyant;
  int rc = ade_scalar_bc_check(fn, sbc, bc, &sw);
  if (!rc) rc = ade_validate(fn, lg, bc, fluid, scalar, slab);
  if (!rc) rc = ade_buoyancy_check(fn, buoy, &by, &buoyant);
  if (!rc) rc = ade_lattice_args(fn, fp, gp, f, h, rho, u, conc, false);
  if (rc) return rc;
  const Geom g = make_geom(*lg);
  return with_ade_models(fluid, scalar, buoyant, [&](const auto& fm, const auto& sm, auto B) {
    return ade_collide_launch<B()>(fp, gp, f, h, g, fm, sm, by, rho, u, conc, st);
  });
}

static int ade_stream_collide(const char* fn, double* fn_, double* gn, const double* fo, const double* go,
                              const lbm_geom* lg, const lbm_bc* lbc, const lbm_bgk_params* fluid,
                              const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy,
                              int row_begin, int row_end, double* rho, double* u, double* conc, hipStream_t st,
                              long long* launches) {
  AdeWalls sw;  // the scalar's walls first: a FIXED edge names the edge mode it cannot sit on
  AdeBuoyancy by;
  bool buoyant;
  int rc = ade_scalar_bc_check(fn, sbc, lbc, &sw);
  if (!rc) rc = ade_validate(fn, lg, lbc, fluid, scalar);
  if (!rc) rc = ade_buoyancy_check(fn, buoy, &by, &buoyant);
  if (!rc) rc = ade_lattice_args(fn, fn_, gn, fo, go, rho, u, conc, true);
  if (rc) return rc;
  LBM_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= lg->R, "%s: row range [%d, %d) outside [0, %d)", fn,
              row_begin, row_end, lg->R);
  if (row_begin == row_end) return LBM_OK;
  const Geom g = make_geom(*lg);
  const Bc bc = make_bc(lbc);
  return with_ade_models(fluid, scalar, buoyant, [&](const auto& fm, const auto& sm, auto B) {
    return ade_step_launch<B()>(fn_, gn, fo, go, g, bc, fm, sm, sw, by, row_begin, row_end, rho, u, conc, st, launches);
  });
}

int ade_part_check(const char* name, const double* fn, const double* gn, const double* fo, const double* go,
                   const lbm_geom* lg, const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                   int part, int edge_rows, const double* rho, const double* u, const double* conc) {
  int rc = ade_validate(name, lg, lbc, fluid, scalar, true);
  if (!rc) rc = ade_lattice_args(name, fn, gn, fo, go, rho, u, conc, true);
  if (rc) return rc;
  LBM_REQUIRE(part == LBM_ADE_PART_FRAME || part == LBM_ADE_PART_INNER,
              "%s: part=%d (LBM_ADE_PART_FRAME or LBM_ADE_PART_INNER)", name, part);
  LBM_REQUIRE(edge_rows >= 1 && 2 * edge_rows < lg->R, "%s: edge_rows=%d: need 1 <= edge_rows and 2 x edge_rows < R=%d",
              name, edge_rows, lg->R);
  return LBM_OK;
}

int ade_scalar_bc_validate(const char* fn, const lbm_ade_scalar_bc* sbc, const lbm_bc* bc) {
  AdeWalls sw;
  return ade_scalar_bc_check(fn, sbc, bc, &sw);
}

int ade_buoyancy_validate(const char* fn, const lbm_ade_buoyancy* buoy) {
  AdeBuoyancy by;
  bool buoyant;
  return ade_buoyancy_check(fn, buoy, &by, &buoyant);
}

// lbm_ade_stream_collide_part(_ex, _b) under the caller's name
static int ade_part(const char* name, double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                    const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                    const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, int part, int edge_rows, double* rho,
                    double* u, double* conc, hipStream_t st) {
  AdeWalls sw;  // the scalar's walls first, as ade_stream_collide
  AdeBuoyancy by;
  bool buoyant;
  int rc = ade_scalar_bc_check(name, sbc, lbc, &sw);
  if (!rc) rc = ade_buoyancy_check(name, buoy, &by, &buoyant);
  if (!rc) rc = ade_part_check(name, fn, gn, fo, go, lg, lbc, fluid, scalar, part, edge_rows, rho, u, conc);
  if (rc) return rc;
  const int R = lg->R;
  const Geom g = make_geom(*lg);
  const Bc bc = make_bc(lbc);
  // FRAME: rows [0, E) then [R - E, R); INNER: rows [E, R - E)
  const int band0 = part == LBM_ADE_PART_FRAME ? 0 : edge_rows;
  const int n0 = part == LBM_ADE_PART_FRAME ? edge_rows : R - 2 * edge_rows;
  const int band1 = R - edge_rows, nrows = part == LBM_ADE_PART_FRAME ? 2 * edge_rows : n0;
  return with_ade_models(fluid, scalar, buoyant, [&](const auto& fm, const auto& sm, auto B) {
    return ade_part_launch<B()>(fn, gn, fo, go, g, bc, fm, sm, sw, by, band0, n0, band1, nrows, rho, u, conc, st);
  });
}

int ade_validate_slab(const char* fn, const lbm_geom* g, const lbm_bc* bc, const lbm_bgk_params* fluid,
                      const lbm_ade_params* scalar) {
  return ade_validate(fn, g, bc, fluid, scalar, true);
}

int ade_collide_slab(const char* fn, double* fp, double* gp, const double* f, const double* h, const lbm_geom* g,
                     const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                     const lbm_ade_buoyancy* buoy, hipStream_t st) {
  return ade_collide(fn, fp, gp, f, h, g, bc, fluid, scalar, nullptr, buoy, nullptr, nullptr, nullptr, st, true);
}

}  // namespace lbm

// the driver loop on one block: two time levels, each one allocation holding the 9 planes of f followed by the
// 9 planes of g (18 padded planes in a row: the 36 concurrent streams of the step spread over the HBM channels)
struct lbm_ade_solver {
  lbm_geom g;  // padded geometry of either lattice
  lbm_bc bc;
  lbm_bgk_params fluid;
  lbm_ade_params scalar;
  lbm_ade_scalar_bc sbc;  // all NO_FLUX unless set
  bool fixed;             // some edge of sbc is FIXED
  lbm_ade_buoyancy buoy;  // lbm_ade_solver_set_buoyancy
  bool buoyant;           // buoy is set (beta = (0, 0) included: the launches decide)
  hipStream_t st;
  double* lat[2];
  double* dense;  // [9][R][C] SoA scratch of get_state
  double* stage;  // [R][C][9] AoS staging
  double *rho, *u, *conc;
  int cur;    // lat[cur] holds the state
  bool post;  // the state is post-collision (P-form); false: pre-collision f_adve, g_adve
  long long steps, launches;
  double* f(int k) const { return lat[k]; }
  double* h(int k) const { return lat[k] + 9 * g.plane_stride; }
};

using namespace lbm;

extern "C" {

int lbm_ade_collide(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                    const lbm_bgk_params* fluid, const lbm_ade_params* scalar, double* rho, double* u, double* conc,
                    lbm_stream_t s) {
  return ade_collide("lbm_ade_collide", fp, gp, f, g_in, g, bc, fluid, scalar, nullptr, nullptr, rho, u, conc,
                     as_stream(s));
}

int lbm_ade_collide_b(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                      const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                      const lbm_ade_buoyancy* buoy, double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_collide("lbm_ade_collide_b", fp, gp, f, g_in, g, bc, fluid, scalar, sbc, buoy, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                           const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar, int row_begin,
                           int row_end, double* rho, double* u, double* conc, lbm_stream_t s) {
  long long launches = 0;
  return ade_stream_collide("lbm_ade_stream_collide", fn, gn, fo, go, g, bc, fluid, scalar, nullptr, nullptr, row_begin,
                            row_end, rho, u, conc, as_stream(s), &launches);
}

int lbm_ade_stream_collide_ex(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                              const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                              const lbm_ade_scalar_bc* sbc, int row_begin, int row_end, double* rho, double* u,
                              double* conc, lbm_stream_t s) {
  long long launches = 0;
  return ade_stream_collide("lbm_ade_stream_collide_ex", fn, gn, fo, go, g, bc, fluid, scalar, sbc, nullptr, row_begin,
                            row_end, rho, u, conc, as_stream(s), &launches);
}

int lbm_ade_stream_collide_b(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, int row_begin, int row_end,
                             double* rho, double* u, double* conc, lbm_stream_t s) {
  long long launches = 0;
  return ade_stream_collide("lbm_ade_stream_collide_b", fn, gn, fo, go, g, bc, fluid, scalar, sbc, buoy, row_begin,
                            row_end, rho, u, conc, as_stream(s), &launches);
}

int lbm_ade_stream_collide_part(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                                const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar, int part,
                                int edge_rows, double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_part("lbm_ade_stream_collide_part", fn, gn, fo, go, lg, lbc, fluid, scalar, nullptr, nullptr, part,
                  edge_rows, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_part_ex(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                                   const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                   const lbm_ade_scalar_bc* sbc, int part, int edge_rows, double* rho, double* u,
                                   double* conc, lbm_stream_t s) {
  return ade_part("lbm_ade_stream_collide_part_ex", fn, gn, fo, go, lg, lbc, fluid, scalar, sbc, nullptr, part,
                  edge_rows, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_part_b(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                                  const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, int part, int edge_rows,
                                  double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_part("lbm_ade_stream_collide_part_b", fn, gn, fo, go, lg, lbc, fluid, scalar, sbc, buoy, part, edge_rows,
                  rho, u, conc, as_stream(s));
}

int lbm_ade_solver_create(lbm_ade_solver** out, const lbm_geom* g, const lbm_bc* bc, const lbm_bgk_params* fluid,
                          const lbm_ade_params* scalar, lbm_stream_t s) {
  LBM_REQUIRE(out, "lbm_ade_solver_create: NULL argument");
  int rc = ade_validate("lbm_ade_solver_create", g, bc, fluid, scalar);
  if (rc) return rc;
  LBM_REQUIRE(g->row_pitch == 0 && g->plane_stride == 0,
              "lbm_ade_solver_create: the context pads its own lattices (row_pitch and plane_stride must be 0)");
  lbm_ade_solver* sv = new (std::nothrow) lbm_ade_solver();
  LBM_REQUIRE(sv, "lbm_ade_solver_create: out of host memory");
  sv->g = *g;
  sv->bc = bc ? *bc : lbm_bc{0, 0, 0, 0, 0, 1.0, 1.0, 0.0, 0.0};
  sv->fluid = *fluid;
  sv->scalar = *scalar;
  sv->sbc = lbm_ade_scalar_bc{};
  sv->fixed = false;
  sv->buoy = lbm_ade_buoyancy{};
  sv->buoyant = false;
  sv->st = as_stream(s);
  sv->cur = 0;
  sv->post = false;
  sv->steps = sv->launches = 0;
  // padded as the solver contexts pad: rows a power of two apart off the same L2 sets / DRAM pages, planes off
  // a power-of-two stride
  const int pitch = lbm_default_row_pitch(g->C);
  sv->g.row_pitch = pitch > g->C ? pitch : 0;
  sv->g.plane_stride = (long long)g->R * pitch + lbm_default_plane_pad(g->R, pitch);
  const size_t n = (size_t)g->R * g->C;
  const size_t lat_doubles = (size_t)sv->g.plane_stride * 18;
  hipError_t e = hipMalloc(&sv->lat[0], lat_doubles * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&sv->lat[1], lat_doubles * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&sv->dense, n * 9 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&sv->stage, n * 9 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&sv->rho, n * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&sv->u, n * 2 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&sv->conc, n * sizeof(double));
  // the row / plane padding is never written by a step: zero it once so that it holds no stale bits
  if (e == hipSuccess) e = hipMemsetAsync(sv->lat[0], 0, lat_doubles * sizeof(double), sv->st);
  if (e == hipSuccess) e = hipMemsetAsync(sv->lat[1], 0, lat_doubles * sizeof(double), sv->st);
  if (e != hipSuccess) {
    set_error("lbm_ade_solver_create: %s", hipGetErrorString(e));
    lbm_ade_solver_destroy(sv);
    return LBM_ERR_HIP;
  }
  *out = sv;
  return LBM_OK;
}

int lbm_ade_solver_destroy(lbm_ade_solver* sv) {
  if (!sv) return LBM_OK;
  if (sv->lat[0] || sv->lat[1]) (void)hipStreamSynchronize(sv->st);
  for (double* p : {sv->lat[0], sv->lat[1], sv->dense, sv->stage, sv->rho, sv->u, sv->conc})
    if (p) (void)hipFree(p);
  delete sv;
  return LBM_OK;
}

int lbm_ade_solver_set_state(lbm_ade_solver* sv, const double* f_host, const double* g_host) {
  LBM_REQUIRE(sv && f_host && g_host, "lbm_ade_solver_set_state: NULL argument");
  const lbm_geom& g = sv->g;
  const size_t bytes = (size_t)g.R * g.C * 9 * sizeof(double);
  LBM_CHECK_HIP(hipMemcpyAsync(sv->stage, f_host, bytes, hipMemcpyHostToDevice, sv->st));
  int rc = lbm_aos_to_soa_pitched(sv->f(sv->cur), sv->stage, g.R, g.C, 9, g.plane_stride, g.row_pitch, sv->st);
  if (rc) return rc;
  LBM_CHECK_HIP(hipMemcpyAsync(sv->dense, g_host, bytes, hipMemcpyHostToDevice, sv->st));
  rc = lbm_aos_to_soa_pitched(sv->h(sv->cur), sv->dense, g.R, g.C, 9, g.plane_stride, g.row_pitch, sv->st);
  if (rc) return rc;
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));  // the host arrays may be reused by the caller
  sv->post = false;
  return LBM_OK;
}

// n driver iterations: the first on a pre-collision state is collide-only, every later one the fused step
// (one launch, two with wall edges).  Enqueues only: no allocation, no host synchronisation.
int lbm_ade_solver_step(lbm_ade_solver* sv, int n) {
  LBM_REQUIRE(sv && n >= 0, "lbm_ade_solver_step: bad argument (n=%d)", n);
  const lbm_ade_buoyancy* buoy = sv->buoyant ? &sv->buoy : nullptr;
  for (int i = 0; i < n; ++i) {
    const int k = sv->cur, o = k ^ 1;
    int rc;
    if (!sv->post) {
      rc = ade_collide("lbm_ade_solver_step", sv->f(o), sv->h(o), sv->f(k), sv->h(k), &sv->g, &sv->bc, &sv->fluid,
                       &sv->scalar, nullptr, buoy, nullptr, nullptr, nullptr, sv->st);
      if (!rc) ++sv->launches;
    } else {
      rc = ade_stream_collide("lbm_ade_solver_step", sv->f(o), sv->h(o), sv->f(k), sv->h(k), &sv->g, &sv->bc,
                              &sv->fluid, &sv->scalar, sv->fixed ? &sv->sbc : nullptr, buoy, 0, sv->g.R, nullptr,
                              nullptr, nullptr, sv->st, &sv->launches);
    }
    if (rc) return rc;
    sv->cur = o;
    sv->post = true;
    ++sv->steps;
  }
  return LBM_OK;
}

// What the reference loop holds after the iterations run so far: f_adve, g_adve (AoS [R][C][9]),
// rho = calc_rho(f_adve), u = calc_u(f_adve, rho) (AoS [R][C][2]), C = calc_rho(g_adve), through the parity
// operators whatever the form and with or without buoyancy (u is calc_u(f_adve, rho): the velocity that enters the
// next step's equilibria is u + u_shift beta (C - c_ref)).  The post-collision state is streamed lazily (lbm_stream: the fix-ups are the
// same for both distributions) into the dead time level.  Any output may be NULL; synchronises.
int lbm_ade_solver_get_state(lbm_ade_solver* sv, double* f, double* g_out, double* rho, double* u, double* conc) {
  LBM_REQUIRE(sv, "lbm_ade_solver_get_state: NULL solver");
  const lbm_geom& g = sv->g;
  const int R = g.R, C = g.C;
  const size_t n = (size_t)R * C;
  int k = sv->cur;
  const lbm_geom dg{R, C, 0, 0, 0};
  const bool fixed = sv->post && sv->fixed;
  if (sv->post) {
    int rc = lbm_stream(sv->f(k ^ 1), sv->f(k), &g, &sv->bc, sv->st);
    if (rc) return rc;
    AdeWalls sw;
    rc = ade_scalar_bc_check("lbm_ade_solver_get_state", fixed ? &sv->sbc : nullptr, &sv->bc, &sw);
    if (rc) return rc;
    // g gathers as BOUNCE_BACK at a FIXED column (ade_scalar_gather_bc); the FIXED edges then take their rule with
    // u = the reference-order calc_u of the streamed f
    lbm_bc gbc = sv->bc;
    if (sw.fixed & 4) gbc.col_lo = LBM_EDGE_BOUNCE_BACK;
    if (sw.fixed & 8) gbc.col_hi = LBM_EDGE_BOUNCE_BACK;
    rc = lbm_stream(sv->h(k ^ 1), sv->h(k), &g, &gbc, sv->st);
    if (rc) return rc;
    k ^= 1;
    if (fixed) {
      rc = lbm_lattice_copy_rows(sv->dense, &dg, 0, sv->f(k), &g, 0, R, sv->st);
      if (!rc) rc = lbm_calc_rho(sv->rho, sv->dense, R, C, sv->st);
      if (!rc) rc = lbm_calc_u(sv->u, sv->dense, sv->rho, R, C, sv->st);
      if (rc) return rc;
      const int n_edge = 2 * C + 2 * R;
      LBM_KLAUNCH(k_ade_fixed_state, dim3((n_edge + 255) / 256), dim3(256), 0, sv->st, sv->h(k), make_geom(g),
                  make_bc(&sv->bc), sw, sv->u, sv->scalar.w_r, sv->scalar.w_c);
      LBM_CHECK_LAUNCH();
    }
  }
  if (f || rho || u) {
    if (f) {
      int rc = lbm_soa_to_aos_pitched(sv->stage, sv->f(k), R, C, 9, g.plane_stride, g.row_pitch, sv->st);
      if (rc) return rc;
      LBM_CHECK_HIP(hipMemcpyAsync(f, sv->stage, n * 9 * sizeof(double), hipMemcpyDeviceToHost, sv->st));
    }
    if ((rho || u) && !fixed) {
      int rc = lbm_lattice_copy_rows(sv->dense, &dg, 0, sv->f(k), &g, 0, R, sv->st);
      if (!rc) rc = lbm_calc_rho(sv->rho, sv->dense, R, C, sv->st);
      if (!rc) rc = lbm_calc_u(sv->u, sv->dense, sv->rho, R, C, sv->st);
      if (rc) return rc;
    }
    if (rho || u) {
      if (rho) LBM_CHECK_HIP(hipMemcpyAsync(rho, sv->rho, n * sizeof(double), hipMemcpyDeviceToHost, sv->st));
      if (u) {
        int rc = lbm_soa_to_aos(sv->stage, sv->u, R, C, 2, sv->st);
        if (rc) return rc;
        LBM_CHECK_HIP(hipMemcpyAsync(u, sv->stage, n * 2 * sizeof(double), hipMemcpyDeviceToHost, sv->st));
      }
    }
  }
  if (g_out) {
    int rc = lbm_soa_to_aos_pitched(sv->stage, sv->h(k), R, C, 9, g.plane_stride, g.row_pitch, sv->st);
    if (rc) return rc;
    LBM_CHECK_HIP(hipMemcpyAsync(g_out, sv->stage, n * 9 * sizeof(double), hipMemcpyDeviceToHost, sv->st));
  }
  if (conc) {
    int rc = lbm_lattice_copy_rows(sv->dense, &dg, 0, sv->h(k), &g, 0, R, sv->st);
    if (!rc) rc = lbm_calc_rho(sv->conc, sv->dense, R, C, sv->st);
    if (rc) return rc;
    LBM_CHECK_HIP(hipMemcpyAsync(conc, sv->conc, n * sizeof(double), hipMemcpyDeviceToHost, sv->st));
  }
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));
  return LBM_OK;
}

int lbm_ade_solver_sync(lbm_ade_solver* sv) {
  LBM_REQUIRE(sv, "lbm_ade_solver_sync: NULL solver");
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));
  return LBM_OK;
}

int lbm_ade_solver_lattices(lbm_ade_solver* sv, double** f_cur, double** g_cur, double** f_other, double** g_other,
                            lbm_geom* geom) {
  LBM_REQUIRE(sv && f_cur && g_cur && f_other && g_other, "lbm_ade_solver_lattices: NULL argument");
  *f_cur = sv->f(sv->cur);
  *g_cur = sv->h(sv->cur);
  *f_other = sv->f(sv->cur ^ 1);
  *g_other = sv->h(sv->cur ^ 1);
  if (geom) *geom = sv->g;
  return LBM_OK;
}

long long lbm_ade_solver_launches(const lbm_ade_solver* sv) { return sv ? sv->launches : -1; }

int lbm_ade_solver_set_scalar_bc(lbm_ade_solver* sv, const lbm_ade_scalar_bc* sbc) {
  LBM_REQUIRE(sv, "lbm_ade_solver_set_scalar_bc: NULL solver");
  AdeWalls sw;
  int rc = ade_scalar_bc_check("lbm_ade_solver_set_scalar_bc", sbc, &sv->bc, &sw);
  if (rc) return rc;
  sv->sbc = sbc ? *sbc : lbm_ade_scalar_bc{};
  sv->fixed = sw.fixed != 0;
  return LBM_OK;
}

int lbm_ade_solver_set_buoyancy(lbm_ade_solver* sv, const lbm_ade_buoyancy* buoy) {
  LBM_REQUIRE(sv, "lbm_ade_solver_set_buoyancy: NULL solver");
  int rc = ade_buoyancy_validate("lbm_ade_solver_set_buoyancy", buoy);
  if (rc) return rc;
  sv->buoy = buoy ? *buoy : lbm_ade_buoyancy{};
  sv->buoyant = buoy != nullptr;
  return LBM_OK;
}

}  // extern "C"
