// The CPU-reachable half of the fluid + scalar step with a KBC fluid as a stand-alone program: every host-side check of
// lbm_ade_collide_m, lbm_ade_stream_collide_m and lbm_ade_solver_create_m, and of their buoyant forms lbm_ade_collide_mb,
// lbm_ade_stream_collide_mb and lbm_ade_solver_set_buoyancy_m, and of the buoyant slab and ring entries
// lbm_ade_slab_stream_collide_mb, lbm_ring_ade_slab_collide_mb and lbm_ring_ade_slab_step_mb, and of open boundaries and the wall
// exchange with the fluid by model, lbm_ade_open_collide_m, lbm_ade_open_stream_collide_m, lbm_ade_solver_set_open_m,
// lbm_ade_wallx_rows_m and lbm_ade_solver_wall_exchange_m -- the fluid by model, the KBC parameters, what
// the step refuses with this fluid, the checks it shares with the BGK fluid, and model = BGK answering with the message of
// the call it names -- and, for both fluids, WHICH fault a call with two faults reports (the order of the host checks is
// observable and differs per fluid; the last section).  Needs no device: every call is refused before a device call (the interior-wall table it
// builds is empty, whose finalize makes none).  `make san` at the root builds it against the sanitizer build of the
// library (ASan + UBSan) and runs it; the ordinary build runs it from tests/test_ade_kbc_abi.py.  Exit status 0 = all
// checks passed.
#include <cmath>
#include <cstdio>
#include <string>

#include "../../include/lbm_hip.h"

static int failures = 0, checks = 0;

// refused with LBM_ERR_INVALID and a message that names `word`
static void refused(int rc, const char* word, const char* what) {
  const std::string msg = lbm_last_error_string();
  ++checks;
  if (rc == LBM_ERR_INVALID && msg.find(word) != std::string::npos) return;
  ++failures;
  std::printf("FAIL: %s -> %d: %s\n", what, rc, msg.c_str());
}

int main() {
  double buf[8] = {0.0}, other[8] = {0.0};
  const lbm_geom g{8, 8, 0, 0, 0};
  const lbm_ade_params sc{1.7, 3e-3, 3e-3, LBM_FORM_DEFAULT};
  lbm_ade_fluid kbc{};
  kbc.model = LBM_MODEL_KBC;
  kbc.kbc = lbm_kbc_params{1.9, LBM_FORM_DEFAULT};
  // the three entry points on one fluid / geometry / edges / scalar: each refuses before it looks at a lattice
  auto all = [&](const lbm_ade_fluid* fl, const lbm_geom* lg, const lbm_bc* bc, const lbm_ade_params* s, const char* word,
                 const char* what) {
    refused(lbm_ade_stream_collide_m(nullptr, nullptr, nullptr, nullptr, lg, bc, fl, s, nullptr, nullptr, 0, 8, nullptr, nullptr,
                                     nullptr, nullptr), word, what);
    refused(lbm_ade_collide_m(nullptr, nullptr, nullptr, nullptr, lg, bc, fl, s, nullptr, nullptr, nullptr, nullptr, nullptr), word, what);
    lbm_ade_solver* sv = nullptr;
    refused(lbm_ade_solver_create_m(&sv, lg, bc, fl, s, nullptr), word, what);
    if (sv) {
      ++failures;
      std::printf("FAIL: %s left a context\n", what);
    }
  };
  all(nullptr, &g, nullptr, &sc, "NULL fluid", "NULL fluid");
  {
    lbm_ade_fluid f = kbc;
    f.model = 7;
    all(&f, &g, nullptr, &sc, "fluid model=7", "unknown model");
    f = kbc;
    f.kbc.s2 = 0.0;
    all(&f, &g, nullptr, &sc, "s2=0 outside (0, 2]", "s2 = 0");
    f.kbc.s2 = 2.5;
    all(&f, &g, nullptr, &sc, "s2=2.5 outside (0, 2]", "s2 = 2.5");
    f = kbc;
    f.kbc.form = 9;
    all(&f, &g, nullptr, &sc, "KBC fluid: form=9", "unknown KBC form");
    f.kbc.form = LBM_FORM_REFERENCE_ORDER;
    const lbm_ade_params fast{1.7, 0.0, 0.0, LBM_FORM_REASSOCIATED};
    all(&f, &g, nullptr, &fast, "KBC fluid form=1 differs from the scalar form=2", "forms differ");
  }
  {
    const lbm_bc pressure{0, 0, 0, 0, 1, 1.0, 1.0, 0.0, 0.0};
    all(&kbc, &g, &pressure, &sc, "pressure rows", "pressure rows with a KBC fluid");
    all(&kbc, &g, &pressure, &sc, "KBC fluid", "pressure rows name the model");
    const lbm_geom odd{8, 7, 0, 0, 0}, ghost{8, 8, 2, 0, 0};
    all(&kbc, &odd, nullptr, &sc, "C=7 must be even", "odd C");
    all(&kbc, &ghost, nullptr, &sc, "ghost=2", "ghost rows");
    all(&kbc, nullptr, nullptr, &sc, "NULL geometry", "NULL geometry");
    all(&kbc, &g, nullptr, nullptr, "NULL scalar params", "NULL scalar");
    const lbm_bc halo{LBM_EDGE_HALO, 0, 0, 0, 0, 1.0, 1.0, 0.0, 0.0};
    all(&kbc, &g, &halo, &sc, "row edge mode HALO", "HALO rows on a single block");
  }
  // past the fluid: the lattices, the moments, the range, the scalar's walls, the interior walls
  refused(lbm_ade_stream_collide_m(nullptr, nullptr, nullptr, nullptr, &g, nullptr, &kbc, &sc, nullptr, nullptr, 0, 8, nullptr, nullptr,
                                   nullptr, nullptr), "NULL lattice", "NULL lattices with a good KBC fluid");
  refused(lbm_ade_stream_collide_m(buf, buf, other, other, &g, nullptr, &kbc, &sc, nullptr, nullptr, 0, 8, nullptr, nullptr, nullptr,
                                   nullptr), "aliased lattices", "aliased lattices");
  refused(lbm_ade_collide_m(buf, buf, buf, buf, &g, nullptr, &kbc, &sc, nullptr, buf, nullptr, nullptr, nullptr), "rho, u and conc",
          "rho without u and conc");
  {
    lbm_ade_scalar_bc sbc{};
    sbc.mode[0] = LBM_ADE_SCALAR_FIXED;  // FIXED on a periodic row
    refused(lbm_ade_stream_collide_m(nullptr, nullptr, nullptr, nullptr, &g, nullptr, &kbc, &sc, &sbc, nullptr, 0, 8, nullptr, nullptr,
                                     nullptr, nullptr), "FIXED on a PERIODIC", "FIXED scalar edge on a periodic row");
    lbm_ade_iwalls* table = nullptr;  // empty: finalize makes no device call
    if (lbm_ade_iwalls_create(&table, 6, 8) != LBM_OK || lbm_ade_iwalls_finalize(table) != LBM_OK) {
      ++failures;
      std::printf("FAIL: building an empty table\n");
    }
    refused(lbm_ade_stream_collide_m(nullptr, nullptr, nullptr, nullptr, &g, nullptr, &kbc, &sc, nullptr, table, 0, 8, nullptr, nullptr,
                                     nullptr, nullptr), "6 x 8", "table built for another R x C");
    lbm_ade_iwalls_destroy(table);
  }
  {  // model = BGK: the message of the call it forwards to; the kbc member is not read
    lbm_ade_fluid bgk{};
    bgk.model = LBM_MODEL_BGK;
    bgk.bgk = lbm_bgk_params{2.0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, LBM_FORM_DEFAULT};
    bgk.kbc = lbm_kbc_params{-3.0, 9};
    refused(lbm_ade_stream_collide_m(nullptr, nullptr, nullptr, nullptr, &g, nullptr, &bgk, &sc, nullptr, nullptr, 0, 8, nullptr, nullptr,
                                     nullptr, nullptr), "lbm_ade_stream_collide_w: omega=2", "BGK through stream_collide_m");
    refused(lbm_ade_collide_m(nullptr, nullptr, nullptr, nullptr, &g, nullptr, &bgk, &sc, nullptr, nullptr, nullptr, nullptr, nullptr),
            "lbm_ade_collide_b: omega=2", "BGK through collide_m");
    lbm_ade_solver* sv = nullptr;
    refused(lbm_ade_solver_create_m(&sv, &g, nullptr, &bgk, &sc, nullptr), "lbm_ade_solver_create: omega=2", "BGK through create_m");
    bgk.bgk.omega = 1.2;
    refused(lbm_ade_stream_collide_m(nullptr, nullptr, nullptr, nullptr, &g, nullptr, &bgk, &sc, nullptr, nullptr, 0, 8, nullptr, nullptr,
                                     nullptr, nullptr), "lbm_ade_stream_collide_w: NULL lattice", "good BGK through stream_collide_m");
  }
  {  // a part of a slab, lbm_ade_stream_collide_part_m: the fluid, the geometry of a slab, the part, the table
    auto part = [&](const lbm_ade_fluid* fl, const lbm_geom* lg, const lbm_bc* bc, const lbm_ade_params* s, double* fn, double* gn,
                    double* fo, double* go, const lbm_ade_iwalls* t, int which, int edge_rows, const char* word, const char* what) {
      refused(lbm_ade_stream_collide_part_m(fn, gn, fo, go, lg, bc, fl, s, nullptr, t, which, edge_rows, nullptr, nullptr, nullptr,
                                            nullptr), word, what);
    };
    alignas(16) double l0[2], l1[2], l2[2], l3[2];  // four distinct, aligned "lattices": the part is refused before any is read
    const int F = LBM_ADE_PART_FRAME;
    part(nullptr, &g, nullptr, &sc, l0, l1, l2, l3, nullptr, F, 1, "lbm_ade_stream_collide_part_m: NULL fluid", "part: NULL fluid");
    lbm_ade_fluid f = kbc;
    f.model = 7;
    part(&f, &g, nullptr, &sc, l0, l1, l2, l3, nullptr, F, 1, "fluid model=7", "part: unknown model");
    f = kbc;
    f.kbc.s2 = 0.0;
    part(&f, &g, nullptr, &sc, l0, l1, l2, l3, nullptr, F, 1, "s2=0 outside (0, 2]", "part: s2 = 0");
    f.kbc.s2 = 2.5;
    part(&f, &g, nullptr, &sc, l0, l1, l2, l3, nullptr, F, 1, "s2=2.5 outside (0, 2]", "part: s2 = 2.5");
    f = kbc;
    f.kbc.form = LBM_FORM_REFERENCE_ORDER;
    const lbm_ade_params fast{1.7, 0.0, 0.0, LBM_FORM_REASSOCIATED};
    part(&f, &g, nullptr, &fast, l0, l1, l2, l3, nullptr, F, 1, "KBC fluid form=1 differs from the scalar form=2", "part: forms differ");
    const lbm_bc pressure{0, 0, 0, 0, 1, 1.0, 1.0, 0.0, 0.0};
    part(&kbc, &g, &pressure, &sc, l0, l1, l2, l3, nullptr, F, 1, "pressure rows", "part: pressure rows");
    part(&kbc, &g, &pressure, &sc, l0, l1, l2, l3, nullptr, F, 1, "KBC fluid", "part: pressure rows name the model");
    part(&kbc, &g, nullptr, &sc, l0, l1, l2, l3, nullptr, 5, 1, "part=5", "part: neither FRAME nor INNER");
    part(&kbc, &g, nullptr, &sc, l0, l1, l2, l3, nullptr, F, 0, "edge_rows=0", "part: edge_rows = 0");
    part(&kbc, &g, nullptr, &sc, l0, l1, l2, l3, nullptr, F, 4, "2 x edge_rows < R=8", "part: 2 x edge_rows = R");
    part(&kbc, &g, nullptr, &sc, nullptr, l1, l2, l3, nullptr, F, 1, "NULL lattice", "part: NULL lattice");
    part(&kbc, &g, nullptr, &sc, l0, l0, l2, l3, nullptr, F, 1, "aliased lattices", "part: aliased lattices");
    const lbm_bc halo{LBM_EDGE_HALO, LBM_EDGE_HALO, 0, 0, 0, 1.0, 1.0, 0.0, 0.0};
    part(&kbc, &g, &halo, &sc, l0, l1, l2, l3, nullptr, F, 1, "HALO needs ghost rows", "part: HALO rows with ghost = 0");
    const lbm_geom slab{8, 8, 1, 0, 0};
    part(&kbc, &slab, nullptr, &sc, l0, l1, l2, l3, nullptr, F, 1, "row edge mode PERIODIC given", "part: PERIODIC rows with ghost = 1 (NULL bc)");
    const lbm_bc periodic{0, 0, 0, 0, 0, 1.0, 1.0, 0.0, 0.0};
    part(&kbc, &slab, &periodic, &sc, l0, l1, l2, l3, nullptr, F, 1, "row edge mode PERIODIC given", "part: PERIODIC rows with ghost = 1");
    // a good slab geometry passes the fluid's and the geometry's checks and is stopped at the part
    part(&kbc, &slab, &halo, &sc, l0, l1, l2, l3, nullptr, 5, 1, "part=5", "part: ghost = 1 with HALO rows is a geometry of the call");
    lbm_ade_iwalls* table = nullptr;
    if (lbm_ade_iwalls_create(&table, 8, 8) != LBM_OK) {
      ++failures;
      std::printf("FAIL: creating a table\n");
    }
    part(&kbc, &slab, &halo, &sc, l0, l1, l2, l3, table, F, 1, "finalize", "part: unfinalized table");
    lbm_ade_iwalls_destroy(table);
    table = nullptr;
    if (lbm_ade_iwalls_create(&table, 6, 8) != LBM_OK || lbm_ade_iwalls_finalize(table) != LBM_OK) {
      ++failures;
      std::printf("FAIL: building an empty table\n");
    }
    part(&kbc, &slab, &halo, &sc, l0, l1, l2, l3, table, F, 1, "6 x 8", "part: table built for another R x C");
    lbm_ade_iwalls_destroy(table);
    // model = BGK: lbm_ade_stream_collide_part_w's message
    lbm_ade_fluid bgk{};
    bgk.model = LBM_MODEL_BGK;
    bgk.bgk = lbm_bgk_params{2.0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, LBM_FORM_DEFAULT};
    bgk.kbc = lbm_kbc_params{-3.0, 9};
    part(&bgk, &slab, &halo, &sc, l0, l1, l2, l3, nullptr, F, 1, "lbm_ade_stream_collide_part_w: omega=2", "BGK through part_m");
    bgk.bgk.omega = 1.2;
    part(&bgk, &slab, &halo, &sc, l0, l1, l2, l3, nullptr, F, 4, "lbm_ade_stream_collide_part_w: edge_rows=4", "good BGK through part_m");
    // the ring's entries look at the fluid before they look at the ring
    refused(lbm_ring_ade_collide_m(nullptr, l0, l1, l2, l3, nullptr, nullptr, &sc, nullptr, nullptr), "lbm_ring_ade_collide_m: NULL fluid",
            "ring collide: NULL fluid");
    f = kbc;
    f.model = 7;
    refused(lbm_ring_ade_step_m(nullptr, l0, l1, l2, l3, nullptr, &f, &sc, nullptr, nullptr, 1, nullptr), "fluid model=7",
            "ring step: unknown model");
    refused(lbm_ring_ade_step_m(nullptr, l0, l1, l2, l3, nullptr, &kbc, &sc, nullptr, nullptr, 1, nullptr), "lbm_ring_ade_step_m: NULL argument",
            "ring step: NULL ring");
    refused(lbm_ring_ade_collide_m(nullptr, l0, l1, l2, l3, nullptr, &kbc, &sc, nullptr, nullptr), "lbm_ring_ade_collide_m: NULL argument",
            "ring collide: NULL ring");
  }
  {  // buoyancy by model, lbm_ade_collide_mb / lbm_ade_stream_collide_mb / lbm_ade_solver_set_buoyancy_m: the descriptor, the fluid
    const double nan = std::nan(""), inf = HUGE_VAL;
    auto both = [&](const lbm_ade_fluid* fl, const lbm_bc* bc, const lbm_ade_params* s, const lbm_ade_buoyancy* by, const char* word,
                    const char* what) {
      refused(lbm_ade_stream_collide_mb(nullptr, nullptr, nullptr, nullptr, &g, bc, fl, s, nullptr, by, nullptr, 0, 8, nullptr, nullptr,
                                        nullptr, nullptr), word, what);
      refused(lbm_ade_collide_mb(nullptr, nullptr, nullptr, nullptr, &g, bc, fl, s, nullptr, by, nullptr, nullptr, nullptr, nullptr), word,
              what);
    };
    const lbm_ade_buoyancy good{1e-2, -5e-3, 0.4, 1.0, 1.0 / 3.0, 1.0 / 9.0};
    lbm_ade_buoyancy b = good;
    b.beta_r = nan;
    both(&kbc, nullptr, &sc, &b, "_mb: buoyancy beta=(nan, -0.005) must be finite", "mb: beta_r = NaN");
    b = good;
    b.beta_c = inf;
    both(&kbc, nullptr, &sc, &b, "_mb: buoyancy beta=(0.01, inf) must be finite", "mb: beta_c = inf");
    b = good;
    b.c_ref = nan;
    both(&kbc, nullptr, &sc, &b, "_mb: buoyancy c_ref=nan must be finite", "mb: c_ref = NaN");
    b = good;
    b.u_shift = -inf;
    both(&kbc, nullptr, &sc, &b, "_mb: buoyancy u_shift=-inf must be finite", "mb: u_shift = -inf");
    b = good;
    b.guo_b = nan;
    both(&kbc, nullptr, &sc, &b, "_mb: buoyancy guo=", "mb: guo_b = NaN (not read for this fluid, still checked)");
    both(nullptr, nullptr, &sc, &good, "_mb: NULL fluid", "mb: NULL fluid");
    const lbm_bc pressure{0, 0, 0, 0, 1, 1.0, 1.0, 0.0, 0.0};
    both(&kbc, &pressure, &sc, &good, "pressure rows", "mb: pressure rows with a KBC fluid");
    lbm_ade_fluid f = kbc;
    f.kbc.form = LBM_FORM_REFERENCE_ORDER;
    const lbm_ade_params fast{1.7, 0.0, 0.0, LBM_FORM_REASSOCIATED};
    both(&f, nullptr, &fast, &good, "KBC fluid form=1 differs from the scalar form=2", "mb: forms differ");
    both(&kbc, nullptr, &sc, &good, "_mb: NULL lattice", "mb: a good descriptor is stopped at the lattices");
    both(&kbc, nullptr, &sc, nullptr, "_mb: NULL lattice", "mb: a NULL descriptor is stopped at the lattices");
    lbm_ade_fluid bgk{};  // model = BGK: the messages of lbm_ade_stream_collide_w / lbm_ade_collide_b
    bgk.model = LBM_MODEL_BGK;
    bgk.bgk = lbm_bgk_params{1.2, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, LBM_FORM_DEFAULT};
    b = good;
    b.c_ref = inf;
    refused(lbm_ade_stream_collide_mb(nullptr, nullptr, nullptr, nullptr, &g, nullptr, &bgk, &sc, nullptr, &b, nullptr, 0, 8, nullptr,
                                      nullptr, nullptr, nullptr), "lbm_ade_stream_collide_w: buoyancy c_ref=inf", "BGK through stream_collide_mb");
    refused(lbm_ade_collide_mb(nullptr, nullptr, nullptr, nullptr, &g, nullptr, &bgk, &sc, nullptr, &b, nullptr, nullptr, nullptr, nullptr),
            "lbm_ade_collide_b: buoyancy c_ref=inf", "BGK through collide_mb");
    refused(lbm_ade_solver_set_buoyancy_m(nullptr, &good), "lbm_ade_solver_set_buoyancy_m: NULL solver", "set_buoyancy_m: NULL solver");
  }
  {  // two faults in one call: the one reported is the one the call checks FIRST -- the order per fluid, every entry kind
    // (BGK entries, the `_m` / `_mb` entries with both models, the part entries).  Each pair: the earlier fault, then the later
    struct Call {
      lbm_ade_fluid fl;
      lbm_geom g;
      const lbm_bc* bc;
      lbm_ade_params sc;
      const lbm_ade_scalar_bc* sbc;
      const lbm_ade_buoyancy* buoy;
      const lbm_ade_iwalls* walls;
      bool lattices;  // four distinct aligned lattices given (false: all NULL)
      int row_begin, row_end, part, edge_rows;
    };
    alignas(16) double l0[2], l1[2], l2[2], l3[2];
    auto lat = [&](const Call& c, double* l) { return c.lattices ? l : nullptr; };
    // the BGK entries take c.fl.bgk, the `_m` / `_mb` entries c.fl by model; an entry without a parameter drops it
    auto stream_w = [&](const Call& c) {
      return lbm_ade_stream_collide_w(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl.bgk, &c.sc, c.sbc, c.buoy,
                                      c.walls, c.row_begin, c.row_end, nullptr, nullptr, nullptr, nullptr);
    };
    auto collide_b = [&](const Call& c) {
      return lbm_ade_collide_b(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl.bgk, &c.sc, c.sbc, c.buoy, nullptr,
                               nullptr, nullptr, nullptr);
    };
    auto part_w = [&](const Call& c) {
      return lbm_ade_stream_collide_part_w(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl.bgk, &c.sc, c.sbc,
                                           c.buoy, c.walls, c.part, c.edge_rows, nullptr, nullptr, nullptr, nullptr);
    };
    auto stream_m = [&](const Call& c) {
      return lbm_ade_stream_collide_m(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl, &c.sc, c.sbc, c.walls,
                                      c.row_begin, c.row_end, nullptr, nullptr, nullptr, nullptr);
    };
    auto stream_mb = [&](const Call& c) {
      return lbm_ade_stream_collide_mb(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl, &c.sc, c.sbc, c.buoy,
                                       c.walls, c.row_begin, c.row_end, nullptr, nullptr, nullptr, nullptr);
    };
    auto collide_m = [&](const Call& c) {
      return lbm_ade_collide_m(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl, &c.sc, c.sbc, nullptr, nullptr,
                               nullptr, nullptr);
    };
    auto collide_mb = [&](const Call& c) {
      return lbm_ade_collide_mb(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl, &c.sc, c.sbc, c.buoy, nullptr,
                                nullptr, nullptr, nullptr);
    };
    auto part_m = [&](const Call& c) {
      return lbm_ade_stream_collide_part_m(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl, &c.sc, c.sbc, c.walls,
                                           c.part, c.edge_rows, nullptr, nullptr, nullptr, nullptr);
    };
    lbm_ade_scalar_bc fixed{};
    fixed.mode[0] = LBM_ADE_SCALAR_FIXED;  // on a PERIODIC row (NULL bc)
    lbm_ade_buoyancy bad_buoy{1e-2, -5e-3, HUGE_VAL, 1.0, 1.0 / 3.0, 1.0 / 9.0};  // c_ref = inf
    lbm_ade_iwalls* open_table = nullptr;  // never finalized
    if (lbm_ade_iwalls_create(&open_table, 8, 8) != LBM_OK) {
      ++failures;
      std::printf("FAIL: creating a table\n");
    }
    const lbm_bc pressure{0, 0, 0, 0, 1, 1.0, 1.0, 0.0, 0.0};
    Call good_bgk{};
    good_bgk.fl.model = LBM_MODEL_BGK;
    good_bgk.fl.bgk = lbm_bgk_params{1.2, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, LBM_FORM_DEFAULT};
    good_bgk.fl.kbc = lbm_kbc_params{-3.0, 9};  // not read with model = BGK
    good_bgk.g = g;
    good_bgk.sc = sc;
    good_bgk.lattices = true;
    good_bgk.row_begin = 0, good_bgk.row_end = 8, good_bgk.part = LBM_ADE_PART_FRAME, good_bgk.edge_rows = 1;
    Call good_kbc = good_bgk;
    good_kbc.fl = kbc;
    Call c;

    // ---- the BGK fluid: scalar walls, geometry, edges, fluid, scalar, form mismatch, buoyancy, interior walls, lattices, range
    c = good_bgk;  // FIXED on a PERIODIC edge + odd C
    c.sbc = &fixed, c.g.C = 7;
    refused(stream_w(c), "lbm_ade_stream_collide_w: scalar edge row_lo: FIXED on a PERIODIC", "2 faults: FIXED on PERIODIC + odd C, stream_w");
    refused(collide_b(c), "lbm_ade_collide_b: scalar edge row_lo: FIXED on a PERIODIC", "2 faults: FIXED on PERIODIC + odd C, collide_b");
    refused(part_w(c), "lbm_ade_stream_collide_part_w: scalar edge row_lo: FIXED on a PERIODIC", "2 faults: FIXED on PERIODIC + odd C, part_w");
    refused(stream_m(c), "lbm_ade_stream_collide_w: scalar edge row_lo: FIXED on a PERIODIC", "2 faults: FIXED on PERIODIC + odd C, stream_m (BGK)");
    refused(collide_mb(c), "lbm_ade_collide_b: scalar edge row_lo: FIXED on a PERIODIC", "2 faults: FIXED on PERIODIC + odd C, collide_mb (BGK)");
    refused(part_m(c), "lbm_ade_stream_collide_part_w: scalar edge row_lo: FIXED on a PERIODIC", "2 faults: FIXED on PERIODIC + odd C, part_m (BGK)");
    c = good_bgk;  // odd C + omega outside range
    c.g.C = 7, c.fl.bgk.omega = 2.0;
    refused(stream_w(c), "lbm_ade_stream_collide_w: C=7 must be even", "2 faults: odd C + omega, stream_w");
    refused(collide_b(c), "lbm_ade_collide_b: C=7 must be even", "2 faults: odd C + omega, collide_b");
    refused(part_w(c), "lbm_ade_stream_collide_part_w: C=7 must be even", "2 faults: odd C + omega, part_w");
    refused(stream_mb(c), "lbm_ade_stream_collide_w: C=7 must be even", "2 faults: odd C + omega, stream_mb (BGK)");
    refused(collide_m(c), "lbm_ade_collide_b: C=7 must be even", "2 faults: odd C + omega, collide_m (BGK)");
    refused(part_m(c), "lbm_ade_stream_collide_part_w: C=7 must be even", "2 faults: odd C + omega, part_m (BGK)");
    c = good_bgk;  // omega + omega_g outside range
    c.fl.bgk.omega = 2.0, c.sc.omega_g = 2.5;
    refused(stream_w(c), "lbm_ade_stream_collide_w: omega=2 outside (0, 2)", "2 faults: omega + omega_g, stream_w");
    refused(collide_b(c), "lbm_ade_collide_b: omega=2 outside (0, 2)", "2 faults: omega + omega_g, collide_b");
    refused(part_w(c), "lbm_ade_stream_collide_part_w: omega=2 outside (0, 2)", "2 faults: omega + omega_g, part_w");
    refused(stream_m(c), "lbm_ade_stream_collide_w: omega=2 outside (0, 2)", "2 faults: omega + omega_g, stream_m (BGK)");
    refused(collide_mb(c), "lbm_ade_collide_b: omega=2 outside (0, 2)", "2 faults: omega + omega_g, collide_mb (BGK)");
    refused(part_m(c), "lbm_ade_stream_collide_part_w: omega=2 outside (0, 2)", "2 faults: omega + omega_g, part_m (BGK)");
    c = good_bgk;  // omega_g outside range + non-finite buoyancy
    c.sc.omega_g = 2.5, c.buoy = &bad_buoy;
    refused(stream_w(c), "lbm_ade_stream_collide_w: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + buoyancy, stream_w");
    refused(collide_b(c), "lbm_ade_collide_b: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + buoyancy, collide_b");
    refused(part_w(c), "lbm_ade_stream_collide_part_w: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + buoyancy, part_w");
    refused(stream_mb(c), "lbm_ade_stream_collide_w: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + buoyancy, stream_mb (BGK)");
    refused(collide_mb(c), "lbm_ade_collide_b: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + buoyancy, collide_mb (BGK)");
    c = good_bgk;  // fluid / scalar form mismatch + non-finite buoyancy
    c.fl.bgk.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED, c.buoy = &bad_buoy;
    refused(stream_w(c), "lbm_ade_stream_collide_w: fluid form=1 differs from the scalar form=2", "2 faults: BGK form mismatch + buoyancy, stream_w");
    refused(collide_mb(c), "lbm_ade_collide_b: fluid form=1 differs from the scalar form=2", "2 faults: BGK form mismatch + buoyancy, collide_mb (BGK)");
    c = good_bgk;  // non-finite buoyancy + unfinalized interior-wall table
    c.buoy = &bad_buoy, c.walls = open_table;
    refused(stream_w(c), "lbm_ade_stream_collide_w: buoyancy c_ref=inf", "2 faults: buoyancy + unfinalized table, stream_w");
    refused(part_w(c), "lbm_ade_stream_collide_part_w: buoyancy c_ref=inf", "2 faults: buoyancy + unfinalized table, part_w");
    refused(stream_mb(c), "lbm_ade_stream_collide_w: buoyancy c_ref=inf", "2 faults: buoyancy + unfinalized table, stream_mb (BGK)");
    c = good_bgk;  // unfinalized table + NULL lattice
    c.walls = open_table, c.lattices = false;
    refused(stream_w(c), "lbm_ade_stream_collide_w: interior walls: the table is not finalized", "2 faults: unfinalized table + NULL lattice, stream_w");
    refused(part_w(c), "lbm_ade_stream_collide_part_w: interior walls: the table is not finalized", "2 faults: unfinalized table + NULL lattice, part_w");
    refused(stream_m(c), "lbm_ade_stream_collide_w: interior walls: the table is not finalized", "2 faults: unfinalized table + NULL lattice, stream_m (BGK)");
    refused(stream_mb(c), "lbm_ade_stream_collide_w: interior walls: the table is not finalized", "2 faults: unfinalized table + NULL lattice, stream_mb (BGK)");
    refused(part_m(c), "lbm_ade_stream_collide_part_w: interior walls: the table is not finalized", "2 faults: unfinalized table + NULL lattice, part_m (BGK)");
    c = good_bgk;  // NULL lattice + bad row range / bad part
    c.lattices = false, c.row_begin = 5, c.row_end = 3, c.part = 5;
    refused(stream_w(c), "lbm_ade_stream_collide_w: NULL lattice", "2 faults: NULL lattice + bad row range, stream_w");
    refused(stream_mb(c), "lbm_ade_stream_collide_w: NULL lattice", "2 faults: NULL lattice + bad row range, stream_mb (BGK)");
    refused(part_w(c), "lbm_ade_stream_collide_part_w: NULL lattice", "2 faults: NULL lattice + part=5, part_w");
    refused(part_m(c), "lbm_ade_stream_collide_part_w: NULL lattice", "2 faults: NULL lattice + part=5, part_m (BGK)");
    c = good_bgk;  // part=5 + bad edge_rows
    c.part = 5, c.edge_rows = 0;
    refused(part_w(c), "lbm_ade_stream_collide_part_w: part=5", "2 faults: part=5 + edge_rows=0, part_w");
    refused(part_m(c), "lbm_ade_stream_collide_part_w: part=5", "2 faults: part=5 + edge_rows=0, part_m (BGK)");

    // ---- the KBC fluid: s2, KBC form, pressure rows; scalar walls, geometry, edges, scalar, buoyancy, interior walls; the KBC
    // form mismatch; lattices, range or part
    c = good_kbc;  // s2 outside range + FIXED on a PERIODIC edge
    c.fl.kbc.s2 = 2.5, c.sbc = &fixed;
    refused(stream_m(c), "lbm_ade_stream_collide_m: KBC fluid: s2=2.5 outside (0, 2]", "2 faults: s2 + FIXED on PERIODIC, stream_m");
    refused(collide_m(c), "lbm_ade_collide_m: KBC fluid: s2=2.5 outside (0, 2]", "2 faults: s2 + FIXED on PERIODIC, collide_m");
    refused(stream_mb(c), "lbm_ade_stream_collide_mb: KBC fluid: s2=2.5 outside (0, 2]", "2 faults: s2 + FIXED on PERIODIC, stream_mb");
    refused(collide_mb(c), "lbm_ade_collide_mb: KBC fluid: s2=2.5 outside (0, 2]", "2 faults: s2 + FIXED on PERIODIC, collide_mb");
    refused(part_m(c), "lbm_ade_stream_collide_part_m: KBC fluid: s2=2.5 outside (0, 2]", "2 faults: s2 + FIXED on PERIODIC, part_m");
    c = good_kbc;  // pressure rows + odd C
    c.bc = &pressure, c.g.C = 7;
    refused(stream_m(c), "lbm_ade_stream_collide_m: pressure rows (pressure_rows=1) are not supported by the fluid + scalar step with a KBC fluid",
            "2 faults: pressure rows + odd C, stream_m");
    refused(collide_mb(c), "lbm_ade_collide_mb: pressure rows (pressure_rows=1)", "2 faults: pressure rows + odd C, collide_mb");
    refused(part_m(c), "lbm_ade_stream_collide_part_m: pressure rows (pressure_rows=1)", "2 faults: pressure rows + odd C, part_m");
    c = good_kbc;  // omega_g outside range + KBC / scalar form mismatch
    c.sc.omega_g = 2.5, c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED;
    refused(stream_m(c), "lbm_ade_stream_collide_m: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + KBC form mismatch, stream_m");
    refused(collide_m(c), "lbm_ade_collide_m: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + KBC form mismatch, collide_m");
    refused(stream_mb(c), "lbm_ade_stream_collide_mb: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + KBC form mismatch, stream_mb");
    refused(part_m(c), "lbm_ade_stream_collide_part_m: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + KBC form mismatch, part_m");
    c = good_kbc;  // non-finite buoyancy + KBC / scalar form mismatch
    c.buoy = &bad_buoy, c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED;
    refused(stream_mb(c), "lbm_ade_stream_collide_mb: buoyancy c_ref=inf", "2 faults: buoyancy + KBC form mismatch, stream_mb");
    refused(collide_mb(c), "lbm_ade_collide_mb: buoyancy c_ref=inf", "2 faults: buoyancy + KBC form mismatch, collide_mb");
    c = good_kbc;  // unfinalized table + KBC / scalar form mismatch
    c.walls = open_table, c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED;
    refused(stream_m(c), "lbm_ade_stream_collide_m: interior walls: the table is not finalized", "2 faults: unfinalized table + KBC form mismatch, stream_m");
    refused(stream_mb(c), "lbm_ade_stream_collide_mb: interior walls: the table is not finalized", "2 faults: unfinalized table + KBC form mismatch, stream_mb");
    refused(part_m(c), "lbm_ade_stream_collide_part_m: interior walls: the table is not finalized", "2 faults: unfinalized table + KBC form mismatch, part_m");
    c = good_kbc;  // KBC / scalar form mismatch + NULL lattice
    c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED, c.lattices = false;
    refused(stream_m(c), "lbm_ade_stream_collide_m: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + NULL lattice, stream_m");
    refused(collide_m(c), "lbm_ade_collide_m: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + NULL lattice, collide_m");
    refused(stream_mb(c), "lbm_ade_stream_collide_mb: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + NULL lattice, stream_mb");
    refused(collide_mb(c), "lbm_ade_collide_mb: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + NULL lattice, collide_mb");
    refused(part_m(c), "lbm_ade_stream_collide_part_m: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + NULL lattice, part_m");
    c = good_kbc;  // KBC / scalar form mismatch + part=5
    c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED, c.part = 5;
    refused(part_m(c), "lbm_ade_stream_collide_part_m: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + part=5, part_m");
    c = good_kbc;  // NULL lattice + bad row range
    c.lattices = false, c.row_begin = 5, c.row_end = 3;
    refused(stream_m(c), "lbm_ade_stream_collide_m: NULL lattice", "2 faults: NULL lattice + bad row range, stream_m");
    refused(stream_mb(c), "lbm_ade_stream_collide_mb: NULL lattice", "2 faults: NULL lattice + bad row range, stream_mb");
    c = good_kbc;  // part=5 + bad edge_rows
    c.part = 5, c.edge_rows = 0;
    refused(part_m(c), "lbm_ade_stream_collide_part_m: part=5", "2 faults: part=5 + edge_rows=0, part_m");

    // ---- buoyancy over row slabs and the ring: lbm_ade_slab_stream_collide_mb, lbm_ring_ade_slab_collide_mb,
    // lbm_ring_ade_slab_step_mb.  The ring's entries are given a NULL ring: what they refuse before they look at it
    auto slab_mb = [&](const Call& c) {
      return lbm_ade_slab_stream_collide_mb(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl, &c.sc, c.sbc, c.buoy,
                                            c.walls, c.part, c.edge_rows, nullptr, nullptr, nullptr, nullptr);
    };
    auto ring_collide_mb = [&](const Call& c, const lbm_ade_fluid* fl) {
      return lbm_ring_ade_slab_collide_mb(nullptr, lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), c.bc, fl, &c.sc, c.sbc, c.buoy, nullptr);
    };
    auto ring_step_mb = [&](const Call& c, const lbm_ade_fluid* fl) {
      return lbm_ring_ade_slab_step_mb(nullptr, lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), c.bc, fl, &c.sc, c.sbc, c.buoy, c.walls,
                                       c.edge_rows, nullptr);
    };
    lbm_ade_buoyancy good_buoy{1e-2, -5e-3, 0.4, 1.0, 1.0 / 3.0, 1.0 / 9.0};
    lbm_ade_buoyancy nan_beta = good_buoy;
    nan_beta.beta_r = std::nan("");
    const lbm_geom slab{8, 8, 1, 0, 0};
    const lbm_bc seams{LBM_EDGE_HALO, LBM_EDGE_HALO, 0, 0, 0, 1.0, 1.0, 0.0, 0.0};
    Call good_slab = good_kbc;
    good_slab.g = slab, good_slab.bc = &seams, good_slab.buoy = &good_buoy;
    refused(lbm_ade_slab_stream_collide_mb(l0, l1, l2, l3, &slab, &seams, nullptr, &sc, nullptr, &good_buoy, nullptr, LBM_ADE_PART_FRAME, 1,
                                           nullptr, nullptr, nullptr, nullptr), "lbm_ade_slab_stream_collide_mb: NULL fluid", "slab_mb: NULL fluid");
    c = good_slab;
    c.fl.model = 7;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: fluid model=7", "slab_mb: unknown model");
    for (int field = 0; field < 6; ++field) {  // every field of the descriptor, non-finite
      lbm_ade_buoyancy b = good_buoy;
      if (field == 0) b.beta_r = HUGE_VAL;
      if (field == 1) b.beta_c = std::nan("");
      if (field == 2) b.c_ref = -HUGE_VAL;
      if (field == 3) b.u_shift = std::nan("");
      if (field == 4) b.guo_a = HUGE_VAL;
      if (field == 5) b.guo_b = std::nan("");
      static const char* const kWord[6] = {"buoyancy beta=", "buoyancy beta=", "buoyancy c_ref=", "buoyancy u_shift=", "buoyancy guo=",
                                           "buoyancy guo="};
      c = good_slab;
      c.buoy = &b;
      refused(slab_mb(c), kWord[field], "slab_mb: a non-finite field of the descriptor");
      refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: buoyancy", "slab_mb: a non-finite field under the new name");
      refused(ring_collide_mb(c, &c.fl), "lbm_ring_ade_slab_collide_mb: buoyancy", "ring_collide_mb: a non-finite field");
      refused(ring_step_mb(c, &c.fl), "lbm_ring_ade_slab_step_mb: buoyancy", "ring_step_mb: a non-finite field");
    }
    c = good_slab;  // beta = (0, 0) is the passive step, but the descriptor is still checked
    lbm_ade_buoyancy zero_inf{0.0, 0.0, HUGE_VAL, 1.0, 0.0, 0.0};
    c.buoy = &zero_inf;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: buoyancy c_ref=inf", "slab_mb: zero beta, c_ref = inf");
    c = good_slab;
    c.fl.kbc.s2 = 2.5;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: KBC fluid: s2=2.5 outside (0, 2]", "slab_mb: s2 = 2.5");
    c.fl.kbc.s2 = 0.0;
    refused(slab_mb(c), "s2=0 outside (0, 2]", "slab_mb: s2 = 0");
    c = good_slab;
    c.bc = &pressure;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: pressure rows", "slab_mb: pressure rows");
    c = good_slab;
    c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: KBC fluid form=1 differs from the scalar form=2", "slab_mb: forms differ");
    c = good_slab;
    c.part = 5;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: part=5", "slab_mb: part = 5");
    c = good_slab;
    c.edge_rows = 0;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: edge_rows=0", "slab_mb: edge_rows = 0");
    c.edge_rows = 4;
    refused(slab_mb(c), "edge_rows=4: need 1 <= edge_rows and 2 x edge_rows < R=8", "slab_mb: edge_rows = R / 2");
    c = good_slab;
    c.lattices = false;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: NULL lattice", "slab_mb: NULL lattices, buoyant");
    c.buoy = nullptr;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: NULL lattice", "slab_mb: NULL lattices, NULL descriptor");
    c = good_slab;
    c.g.ghost = 0;  // HALO rows without ghost rows
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: row edge mode HALO needs ghost rows", "slab_mb: HALO without ghost rows");
    c = good_slab;
    c.walls = open_table;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: interior walls: the table is not finalized", "slab_mb: unfinalized table");
    // the ring's entries before the ring: the fluid, then the descriptor, then their arguments
    c = good_slab;
    refused(ring_collide_mb(c, nullptr), "lbm_ring_ade_slab_collide_mb: NULL fluid", "ring_collide_mb: NULL fluid");
    refused(ring_step_mb(c, nullptr), "lbm_ring_ade_slab_step_mb: NULL fluid", "ring_step_mb: NULL fluid");
    refused(ring_collide_mb(c, &c.fl), "lbm_ring_ade_slab_collide_mb: NULL argument", "ring_collide_mb: NULL ring");
    refused(ring_step_mb(c, &c.fl), "lbm_ring_ade_slab_step_mb: NULL argument", "ring_step_mb: NULL ring");
    c.fl.model = 7;
    refused(ring_collide_mb(c, &c.fl), "lbm_ring_ade_slab_collide_mb: fluid model=7", "ring_collide_mb: unknown model");
    refused(ring_step_mb(c, &c.fl), "lbm_ring_ade_slab_step_mb: fluid model=7", "ring_step_mb: unknown model");
    // model = BGK: the entries they forward to answer, with the same descriptor
    c = good_slab;
    c.fl = good_bgk.fl;
    c.part = 5;
    refused(slab_mb(c), "lbm_ade_stream_collide_part_w: part=5", "slab_mb (BGK): part = 5");
    c.buoy = &nan_beta;
    refused(slab_mb(c), "lbm_ade_stream_collide_part_w: buoyancy beta=", "slab_mb (BGK): non-finite beta");
    refused(ring_collide_mb(c, &c.fl), "lbm_ring_ade_collide_b: buoyancy beta=", "ring_collide_mb (BGK): non-finite beta");
    refused(ring_step_mb(c, &c.fl), "lbm_ring_ade_step_w: buoyancy beta=", "ring_step_mb (BGK): non-finite beta");
    c.buoy = &good_buoy;
    refused(ring_collide_mb(c, &c.fl), "lbm_ring_ade_collide_b: NULL argument", "ring_collide_mb (BGK): NULL ring");
    refused(ring_step_mb(c, &c.fl), "lbm_ring_ade_step_w: NULL argument", "ring_step_mb (BGK): NULL ring");
    c.fl.bgk.omega = 2.0;
    refused(slab_mb(c), "lbm_ade_stream_collide_part_w: omega=2 outside (0, 2)", "slab_mb (BGK): omega = 2");
    // two faults: which one is reported
    c = good_slab;  // s2 outside range + non-finite buoyancy
    c.fl.kbc.s2 = 2.5, c.buoy = &bad_buoy;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: KBC fluid: s2=2.5", "2 faults: s2 + buoyancy, slab_mb");
    c = good_slab;  // pressure rows + non-finite buoyancy
    c.bc = &pressure, c.buoy = &bad_buoy;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: pressure rows (pressure_rows=1)", "2 faults: pressure rows + buoyancy, slab_mb");
    c = good_slab;  // odd C + non-finite buoyancy
    c.g.C = 7, c.buoy = &bad_buoy;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: C=7 must be even", "2 faults: odd C + buoyancy, slab_mb");
    c = good_slab;  // omega_g outside range + non-finite buoyancy
    c.sc.omega_g = 2.5, c.buoy = &bad_buoy;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + buoyancy, slab_mb");
    c = good_slab;  // non-finite buoyancy + unfinalized table
    c.buoy = &bad_buoy, c.walls = open_table;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: buoyancy c_ref=inf", "2 faults: buoyancy + unfinalized table, slab_mb");
    c = good_slab;  // non-finite buoyancy + KBC / scalar form mismatch
    c.buoy = &bad_buoy, c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: buoyancy c_ref=inf", "2 faults: buoyancy + KBC form mismatch, slab_mb");
    c = good_slab;  // unfinalized table + KBC / scalar form mismatch
    c.walls = open_table, c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: interior walls: the table is not finalized", "2 faults: unfinalized table + KBC form mismatch, slab_mb");
    c = good_slab;  // KBC / scalar form mismatch + NULL lattice
    c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED, c.lattices = false;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + NULL lattice, slab_mb");
    c = good_slab;  // NULL lattice + part=5
    c.lattices = false, c.part = 5;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: NULL lattice", "2 faults: NULL lattice + part=5, slab_mb");
    c = good_slab;  // part=5 + bad edge_rows
    c.part = 5, c.edge_rows = 0;
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: part=5", "2 faults: part=5 + edge_rows=0, slab_mb");
    c = good_slab;  // the ring's entries: non-finite buoyancy + NULL ring
    c.buoy = &bad_buoy;
    refused(ring_collide_mb(c, &c.fl), "lbm_ring_ade_slab_collide_mb: buoyancy c_ref=inf", "2 faults: buoyancy + NULL ring, ring_collide_mb");
    refused(ring_step_mb(c, &c.fl), "lbm_ring_ade_slab_step_mb: buoyancy c_ref=inf", "2 faults: buoyancy + NULL ring, ring_step_mb");
    c.fl.model = 7;  // unknown model + non-finite buoyancy
    refused(ring_collide_mb(c, &c.fl), "lbm_ring_ade_slab_collide_mb: fluid model=7", "2 faults: model + buoyancy, ring_collide_mb");
    refused(ring_step_mb(c, &c.fl), "lbm_ring_ade_slab_step_mb: fluid model=7", "2 faults: model + buoyancy, ring_step_mb");
    refused(slab_mb(c), "lbm_ade_slab_stream_collide_mb: fluid model=7", "2 faults: model + buoyancy, slab_mb");
    lbm_ade_iwalls_destroy(open_table);
  }
  {  // open boundaries and the wall exchange with the fluid by model: lbm_ade_open_collide_m, lbm_ade_open_stream_collide_m,
    // lbm_ade_solver_set_open_m, lbm_ade_wallx_rows_m, lbm_ade_solver_wall_exchange_m.  Without a device only an EMPTY open
    // table can be finalized, so what needs listed nodes (the carry, the row range, the overlap rule) is the GPU suite's
    struct Call {
      lbm_ade_fluid fl;
      lbm_geom g;
      const lbm_bc* bc;
      lbm_ade_params sc;
      const lbm_ade_scalar_bc* sbc;
      const lbm_ade_buoyancy* buoy;
      const lbm_ade_iwalls* walls;
      const lbm_ade_open* open;
      bool lattices;  // four distinct aligned lattices / the exchange's table, fo, go given (false: all NULL)
      int row_begin, row_end;
    };
    alignas(16) double l0[2], l1[2], l2[2], l3[2];
    auto lat = [&](const Call& c, double* l) { return c.lattices ? l : nullptr; };
    auto collide_o = [&](const Call& c) {
      return lbm_ade_collide_o(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl.bgk, &c.sc, c.sbc, c.buoy, c.open, nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    auto stream_o = [&](const Call& c) {
      return lbm_ade_stream_collide_o(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl.bgk, &c.sc, c.sbc, c.buoy, c.walls, c.open, nullptr, nullptr, c.row_begin, c.row_end, nullptr, nullptr, nullptr, nullptr);
    };
    auto wallx = [&](const Call& c) {
      return lbm_ade_wallx_rows(lat(c, l0), 8, 0, lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl.bgk, &c.sc, c.sbc, c.buoy, c.walls, nullptr, c.row_begin, c.row_end, nullptr);
    };
    auto open_collide_m = [&](const Call& c) {
      return lbm_ade_open_collide_m(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl, &c.sc, c.sbc, c.buoy, c.open, nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    auto open_stream_m = [&](const Call& c) {
      return lbm_ade_open_stream_collide_m(lat(c, l0), lat(c, l1), lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl, &c.sc, c.sbc, c.buoy, c.walls, c.open, nullptr, nullptr, c.row_begin, c.row_end, nullptr, nullptr, nullptr, nullptr);
    };
    auto wallx_m = [&](const Call& c) {
      return lbm_ade_wallx_rows_m(lat(c, l0), 8, 0, lat(c, l2), lat(c, l3), &c.g, c.bc, &c.fl, &c.sc, c.sbc, c.buoy, c.walls, nullptr, c.row_begin, c.row_end, nullptr);
    };
    lbm_ade_scalar_bc fixed{};
    fixed.mode[0] = LBM_ADE_SCALAR_FIXED;  // on a PERIODIC row (NULL bc)
    lbm_ade_buoyancy bad_buoy{1e-2, -5e-3, HUGE_VAL, 1.0, 1.0 / 3.0, 1.0 / 9.0};  // c_ref = inf
    const lbm_bc pressure{0, 0, 0, 0, 1, 1.0, 1.0, 0.0, 0.0};
    lbm_ade_iwalls* raw_walls = nullptr;                                   // never finalized
    lbm_ade_open *raw_open = nullptr, *small = nullptr, *view = nullptr;  // a column of rules, never finalized; an empty 6 x 8
    bool built = lbm_ade_iwalls_create(&raw_walls, 8, 8) == LBM_OK && lbm_ade_open_create(&raw_open, 8, 8) == LBM_OK;
    built = built && lbm_ade_open_add_f(raw_open, 0, 0, 1, 0, 8, 0xFFu, LBM_ADE_OPEN_BOUNCE_BACK, 0.0, 0.0, 0, 0) == LBM_OK;
    built = built && lbm_ade_open_create(&small, 6, 8) == LBM_OK && lbm_ade_open_finalize(small) == LBM_OK;
    built = built && lbm_ade_open_slab(&view, raw_open, 0, 8) == LBM_OK;  // a slab view of all rows, never finalized
    if (!built) {
      ++failures;
      std::printf("FAIL: building the tables of the open-boundary section\n");
    }
    Call good_bgk{};
    good_bgk.fl.model = LBM_MODEL_BGK;
    good_bgk.fl.bgk = lbm_bgk_params{1.2, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, LBM_FORM_DEFAULT};
    good_bgk.fl.kbc = lbm_kbc_params{-3.0, 9};  // not read with model = BGK
    good_bgk.g = g;
    good_bgk.sc = sc;
    good_bgk.lattices = true;
    good_bgk.row_begin = 0, good_bgk.row_end = 8;
    Call good_kbc = good_bgk;
    good_kbc.fl = kbc;
    Call c;

    // ---- the fluid of the new entries, and everything the `_m` / `_mb` calls refuse, under the new names
    refused(lbm_ade_open_collide_m(l0, l1, l2, l3, &g, nullptr, nullptr, &sc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "lbm_ade_open_collide_m: NULL fluid", "open_collide_m: NULL fluid");
    refused(lbm_ade_open_stream_collide_m(l0, l1, l2, l3, &g, nullptr, nullptr, &sc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 8, nullptr, nullptr, nullptr, nullptr), "lbm_ade_open_stream_collide_m: NULL fluid", "open_stream_m: NULL fluid");
    refused(lbm_ade_wallx_rows_m(l0, 8, 0, l2, l3, &g, nullptr, nullptr, &sc, nullptr, nullptr, nullptr, nullptr, 0, 8, nullptr), "lbm_ade_wallx_rows_m: NULL fluid", "wallx_m: NULL fluid");
    c = good_kbc;
    c.fl.model = 7;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: fluid model=7", "open_collide_m: unknown model");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: fluid model=7", "open_stream_m: unknown model");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: fluid model=7", "wallx_m: unknown model");
    c = good_kbc;
    c.fl.kbc.s2 = 2.5;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: KBC fluid: s2=2.5 outside (0, 2]", "open_collide_m: s2 = 2.5");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: KBC fluid: s2=2.5 outside (0, 2]", "open_stream_m: s2 = 2.5");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: KBC fluid: s2=2.5 outside (0, 2]", "wallx_m: s2 = 2.5");
    c.fl.kbc.s2 = 0.0;
    refused(open_stream_m(c), "s2=0 outside (0, 2]", "open_stream_m: s2 = 0");
    c = good_kbc;
    c.bc = &pressure;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: pressure rows (pressure_rows=1) are not supported by the fluid + scalar step with a KBC fluid", "open_collide_m: pressure rows");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: pressure rows (pressure_rows=1)", "open_stream_m: pressure rows");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: pressure rows (pressure_rows=1)", "wallx_m: pressure rows");
    c = good_kbc;
    c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: KBC fluid form=1 differs from the scalar form=2", "open_collide_m: forms differ");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: KBC fluid form=1 differs from the scalar form=2", "open_stream_m: forms differ");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: KBC fluid form=1 differs from the scalar form=2", "wallx_m: forms differ");
    c = good_kbc;
    c.buoy = &bad_buoy;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: buoyancy c_ref=inf must be finite", "open_collide_m: non-finite buoyancy");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: buoyancy c_ref=inf must be finite", "open_stream_m: non-finite buoyancy");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: buoyancy c_ref=inf must be finite", "wallx_m: non-finite buoyancy");
    c = good_kbc;
    c.g.C = 7;
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: C=7 must be even", "open_stream_m: odd C");
    c = good_kbc;
    c.sbc = &fixed;
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: scalar edge row_lo: FIXED on a PERIODIC", "open_stream_m: FIXED on a periodic row");
    c = good_kbc;
    c.walls = raw_walls;
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: interior walls: the table is not finalized", "open_stream_m: unfinalized interior walls");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: interior walls: the table is not finalized", "wallx_m: unfinalized interior walls");

    // ---- everything the `_o` calls refuse that needs no listed node, under the new names
    c = good_kbc;
    c.open = raw_open;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: open boundaries: the table is not finalized", "open_collide_m: unfinalized table");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: open boundaries: the table is not finalized", "open_stream_m: unfinalized table");
    c.open = small;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: open boundaries: the table is for a 6 x 8 lattice, the call for 8 x 8", "open_collide_m: table of another size");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: open boundaries: the table is for a 6 x 8 lattice, the call for 8 x 8", "open_stream_m: table of another size");
    c.open = view;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: open boundaries: the table is a slab view", "open_collide_m: slab view");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: open boundaries: the table is a slab view", "open_stream_m: slab view");
    c = good_kbc;  // a NULL table is the `_mb` call, stopped at its lattices and its range under the new name
    c.lattices = false;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: NULL lattice", "open_collide_m: NULL lattices");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: NULL lattice", "open_stream_m: NULL lattices");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: NULL argument (table, fo, go)", "wallx_m: NULL table, fo, go");
    c = good_kbc;
    c.row_begin = 5, c.row_end = 3;
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: row range [5, 3) outside [0, 8)", "open_stream_m: bad row range");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: ", "wallx_m: bad row range");
    c = good_kbc;
    c.row_end = 9;
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: ", "wallx_m: rows beyond the lattice");
    refused(lbm_ade_wallx_rows_m(l0, 4, 0, l2, l3, &g, nullptr, &kbc, &sc, nullptr, nullptr, nullptr, nullptr, 0, 8, nullptr), "lbm_ade_wallx_rows_m: table_row0=0 + rows [0, 8) do not fit table_rows=4", "wallx_m: table too short");
    // the context's entries without a context
    refused(lbm_ade_solver_set_open_m(nullptr, nullptr), "NULL solver", "set_open_m: NULL solver");
    double out6[LBM_WALLX_NQ];
    refused(lbm_ade_solver_wall_exchange_m(nullptr, nullptr, 0, 8, out6, nullptr), "NULL argument (solver, out_host)", "wall_exchange_m: NULL solver");

    // ---- model = BGK: the siblings answer, under their names
    c = good_bgk;
    c.fl.bgk.omega = 2.0;
    refused(open_collide_m(c), "lbm_ade_collide_o: omega=2 outside (0, 2)", "BGK through open_collide_m");
    refused(open_stream_m(c), "lbm_ade_stream_collide_o: omega=2 outside (0, 2)", "BGK through open_stream_m");
    refused(wallx_m(c), "lbm_ade_wallx_rows: omega=2 outside (0, 2)", "BGK through wallx_m");
    c = good_bgk;
    c.open = raw_open;
    refused(open_collide_m(c), "lbm_ade_collide_o: open boundaries: the table is not finalized", "BGK through open_collide_m: unfinalized table");
    refused(open_stream_m(c), "lbm_ade_stream_collide_o: open boundaries: the table is not finalized", "BGK through open_stream_m: unfinalized table");
    c = good_bgk;
    c.lattices = false;
    refused(wallx_m(c), "lbm_ade_wallx_rows: NULL argument (table, fo, go)", "BGK through wallx_m: NULL table, fo, go");

    // ---- two faults in one call.  model = BGK: the new entry reports what its sibling reports, word for word
    c = good_bgk;  // omega_g outside range + unfinalized open table
    c.sc.omega_g = 2.5, c.open = raw_open;
    refused(collide_o(c), "lbm_ade_collide_o: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + unfinalized open table, collide_o");
    refused(stream_o(c), "lbm_ade_stream_collide_o: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + unfinalized open table, stream_o");
    refused(open_collide_m(c), "lbm_ade_collide_o: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + unfinalized open table, open_collide_m (BGK)");
    refused(open_stream_m(c), "lbm_ade_stream_collide_o: omega_g=2.5 outside (0, 2)", "2 faults: omega_g + unfinalized open table, open_stream_m (BGK)");
    c = good_bgk;  // unfinalized interior walls + unfinalized open table
    c.walls = raw_walls, c.open = raw_open;
    refused(stream_o(c), "lbm_ade_stream_collide_o: interior walls: the table is not finalized", "2 faults: unfinalized walls + unfinalized open table, stream_o");
    refused(open_stream_m(c), "lbm_ade_stream_collide_o: interior walls: the table is not finalized", "2 faults: unfinalized walls + unfinalized open table, open_stream_m (BGK)");
    c = good_bgk;  // unfinalized open table + NULL lattice
    c.open = raw_open, c.lattices = false;
    refused(collide_o(c), "lbm_ade_collide_o: open boundaries: the table is not finalized", "2 faults: unfinalized open table + NULL lattice, collide_o");
    refused(stream_o(c), "lbm_ade_stream_collide_o: open boundaries: the table is not finalized", "2 faults: unfinalized open table + NULL lattice, stream_o");
    refused(open_collide_m(c), "lbm_ade_collide_o: open boundaries: the table is not finalized", "2 faults: unfinalized open table + NULL lattice, open_collide_m (BGK)");
    refused(open_stream_m(c), "lbm_ade_stream_collide_o: open boundaries: the table is not finalized", "2 faults: unfinalized open table + NULL lattice, open_stream_m (BGK)");
    c = good_bgk;  // a slab view that is not finalized either: the kind is named first
    c.open = view;
    refused(stream_o(c), "lbm_ade_stream_collide_o: open boundaries: the table is a slab view", "2 faults: slab view + unfinalized, stream_o");
    refused(open_stream_m(c), "lbm_ade_stream_collide_o: open boundaries: the table is a slab view", "2 faults: slab view + unfinalized, open_stream_m (BGK)");
    c = good_bgk;  // table of another size + bad row range
    c.open = small, c.row_begin = 5, c.row_end = 3;
    refused(stream_o(c), "lbm_ade_stream_collide_o: open boundaries: the table is for a 6 x 8 lattice", "2 faults: table size + bad row range, stream_o");
    refused(open_stream_m(c), "lbm_ade_stream_collide_o: open boundaries: the table is for a 6 x 8 lattice", "2 faults: table size + bad row range, open_stream_m (BGK)");
    c = good_bgk;  // NULL lattice + bad row range
    c.lattices = false, c.row_begin = 5, c.row_end = 3;
    refused(stream_o(c), "lbm_ade_stream_collide_o: NULL lattice", "2 faults: NULL lattice + bad row range, stream_o");
    refused(open_stream_m(c), "lbm_ade_stream_collide_o: NULL lattice", "2 faults: NULL lattice + bad row range, open_stream_m (BGK)");
    c = good_bgk;  // the exchange: non-finite buoyancy + NULL table, fo, go
    c.buoy = &bad_buoy, c.lattices = false;
    refused(wallx(c), "lbm_ade_wallx_rows: buoyancy c_ref=inf", "2 faults: buoyancy + NULL argument, wallx_rows");
    refused(wallx_m(c), "lbm_ade_wallx_rows: buoyancy c_ref=inf", "2 faults: buoyancy + NULL argument, wallx_m (BGK)");
    c = good_bgk;  // the exchange: unfinalized interior walls + NULL table, fo, go
    c.walls = raw_walls, c.lattices = false;
    refused(wallx(c), "lbm_ade_wallx_rows: interior walls: the table is not finalized", "2 faults: unfinalized walls + NULL argument, wallx_rows");
    refused(wallx_m(c), "lbm_ade_wallx_rows: interior walls: the table is not finalized", "2 faults: unfinalized walls + NULL argument, wallx_m (BGK)");
    c = good_bgk;  // the exchange: NULL table, fo, go + bad row range
    c.lattices = false, c.row_begin = 5, c.row_end = 3;
    refused(wallx(c), "lbm_ade_wallx_rows: NULL argument (table, fo, go)", "2 faults: NULL argument + bad row range, wallx_rows");
    refused(wallx_m(c), "lbm_ade_wallx_rows: NULL argument (table, fo, go)", "2 faults: NULL argument + bad row range, wallx_m (BGK)");

    // ---- two faults, model = KBC: the fluid's own checks first, the KBC form mismatch after the interior walls, the open
    // table last of what the call resolves, the lattices and the range after
    c = good_kbc;  // s2 outside range + unfinalized open table
    c.fl.kbc.s2 = 2.5, c.open = raw_open;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: KBC fluid: s2=2.5 outside (0, 2]", "2 faults: s2 + unfinalized open table, open_collide_m");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: KBC fluid: s2=2.5 outside (0, 2]", "2 faults: s2 + unfinalized open table, open_stream_m");
    c = good_kbc;  // pressure rows + slab view
    c.bc = &pressure, c.open = view;
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: pressure rows (pressure_rows=1)", "2 faults: pressure rows + slab view, open_stream_m");
    c = good_kbc;  // non-finite buoyancy + unfinalized open table
    c.buoy = &bad_buoy, c.open = raw_open;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: buoyancy c_ref=inf", "2 faults: buoyancy + unfinalized open table, open_collide_m");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: buoyancy c_ref=inf", "2 faults: buoyancy + unfinalized open table, open_stream_m");
    c = good_kbc;  // KBC / scalar form mismatch + unfinalized open table
    c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED, c.open = raw_open;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + unfinalized open table, open_collide_m");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + unfinalized open table, open_stream_m");
    c = good_kbc;  // unfinalized interior walls + KBC / scalar form mismatch
    c.walls = raw_walls, c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED;
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: interior walls: the table is not finalized", "2 faults: unfinalized walls + KBC form mismatch, open_stream_m");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: interior walls: the table is not finalized", "2 faults: unfinalized walls + KBC form mismatch, wallx_m");
    c = good_kbc;  // unfinalized open table + NULL lattice
    c.open = raw_open, c.lattices = false;
    refused(open_collide_m(c), "lbm_ade_open_collide_m: open boundaries: the table is not finalized", "2 faults: unfinalized open table + NULL lattice, open_collide_m");
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: open boundaries: the table is not finalized", "2 faults: unfinalized open table + NULL lattice, open_stream_m");
    c = good_kbc;  // a slab view that is not finalized either
    c.open = view;
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: open boundaries: the table is a slab view", "2 faults: slab view + unfinalized, open_stream_m");
    c = good_kbc;  // NULL lattice + bad row range
    c.lattices = false, c.row_begin = 5, c.row_end = 3;
    refused(open_stream_m(c), "lbm_ade_open_stream_collide_m: NULL lattice", "2 faults: NULL lattice + bad row range, open_stream_m");
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: NULL argument (table, fo, go)", "2 faults: NULL argument + bad row range, wallx_m");
    c = good_kbc;  // the exchange: KBC / scalar form mismatch + NULL table, fo, go
    c.fl.kbc.form = LBM_FORM_REFERENCE_ORDER, c.sc.form = LBM_FORM_REASSOCIATED, c.lattices = false;
    refused(wallx_m(c), "lbm_ade_wallx_rows_m: KBC fluid form=1 differs from the scalar form=2", "2 faults: KBC form mismatch + NULL argument, wallx_m");
    lbm_ade_open_destroy(view);
    lbm_ade_open_destroy(small);
    lbm_ade_open_destroy(raw_open);
    lbm_ade_iwalls_destroy(raw_walls);
  }
  std::printf("ade_kbc_host_check: %d refusals checked, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
