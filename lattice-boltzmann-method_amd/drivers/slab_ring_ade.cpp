// Fluid + transported scalar (lbm_ade_*, the sediment loop of test/rectangle_sedimentation_test.cpp:88-247 without its
// driver-specific edges) slab-decomposed along r: one ghost row per side, ONE packed message per neighbour per step
// carrying the single-step halo of both lattices (2 x 3 rows), FRAME + pack + exchange on the ring's stream beside the
// INNER rows (lbm_ring_ade_step_w / _o / _m).  C++ host on lbm_ring_* + lbm_ade_stream_collide_part_w / _o / _m; one
// process per GPU.
//
//   slab_ring_ade --spawn N [...]          fork N ranks on this node (rank i -> GPU i; --one-gpu 1: all on GPU 0,
//                                          with --transport ipc: N real ranks sharing one device)
//   RANK=i WORLD_SIZE=N LOCAL_RANK=i slab_ring_ade --id-file /tmp/x [...]   under any launcher
//   slab_ring_ade --emulate N [...]        ONE process / one GPU playing all N slabs in turn: the same two part launches
//                                          on the same two streams, the messages by device copies, per-slab time by HIP
//                                          events, each step alternated with the step of one slab-sized single block
//
// Options: --rows R (per slab, weak scaling) --cols C --steps K --warmup W --edge-rows E --omega w --omega-g wg
//          --walls 1 (bounce-back rows on the chain ends, bounce-back column 0, specular column C-1: a chain; default a
//          closed, periodic ring)  --form ref|fast (both halves)  --check 1 (bitwise against one block: small sizes; a one
//          block that is not finite fails the check, and the line reports how many values as "one_block_nonfinite")
//          --scalar-fixed 1 (with --walls 1: fixed-concentration walls of the scalar, lbm_ade_scalar_bc -- row 0 of the
//          chain at C_w = 1e-3, column 0 at a profile, 1e-3 on the last quarter of the global rows and 0 elsewhere, read
//          from a device array of which each slab passes its slice, column C-1 absorbing, C_w = 0, beside the specular
//          fluid column; the last row stays no-flux)
//          --buoyancy beta_r,beta_c,c_ref[,u_shift,guo_a,guo_b] (the scalar pushes on the fluid, lbm_ade_buoyancy: the
//          _b entry points, reference order whatever --form; --check's one block runs the same buoyant step)
//          --rectangle 1 (with --walls 1: interior walls, lbm_ade_iwalls -- the sedimentation driver's rectangle scaled to
//          the GLOBAL box, ceiling Rg/3 above the last row, columns 2C/8 .. 5C/16, absorbing (FIXED at 0).  One global
//          table per process; each slab or rank takes its view, lbm_ade_iwalls_slab; --check's one block runs
//          lbm_ade_stream_collide_w with the global table)
//          --channel 1 (with --walls 1: open boundaries, lbm_ade_open -- the sedimentation channel of
//          lbm_ade_open_add_channel on the GLOBAL box, u_in = 0.03, C_w = 1e-3 on the last quarter of the inlet's rows; the
//          columns become PERIODIC edges that the inlet and outlet replace, the rows stay the chain's walls.  One global
//          table per process; each slab or rank takes its view, lbm_ade_open_slab, and owns its carry; the _o entry points.
//          Combines with --rectangle 1 and --buoyancy; --check's one block runs lbm_ade_collide_o / lbm_ade_stream_collide_o
//          with the global tables and compares the carry as well)
//          --exchange 1 (with --emulate and --rectangle 1: the wall exchange of the final state -- every slab fills its rows
//          of ONE global row table, lbm_ade_wallx_rows with its view; printed before the JSON line: `wallx_slabs=` the
//          fold of that table, `wallx_one_block=` the fold of the one block's, six values each in LBM_WALLX_* order)
//
//          --fluid bgk|kbc (default bgk) --s2 X (default --omega): kbc = the entropic KBC collision as the fluid
//          (lbm_ade_fluid) through the _m entry points -- lbm_ring_ade_collide_m / lbm_ring_ade_step_m,
//          lbm_ade_stream_collide_part_m; --check's one block runs lbm_ade_collide_m / lbm_ade_stream_collide_m.  KBC's
//          stabiliser is 0/0 on a lattice exactly at equilibrium, so this fluid starts as passive_scalar_box --fluid kbc
//          does: lbm_kbc_equilibrium without the u^2 terms on a shear wave that drifts along r.  Combines with --walls 1,
//          --scalar-fixed 1, --rectangle 1 and --form; --buoyancy, --channel 1 and --exchange 1 are refused with it.
//
// Printed: one JSON line; ms per step of the slowest slab, and the one-block step of a slab-sized lattice beside it.
//
// run_rank / run_emulated hold the model and its lbm_ring_* calls; options, main(), the timed run, --check's comparison
// and the emulation's links are ring_common.hpp.
#include <cmath>

#include "ring_common.hpp"

namespace {

struct Args : RingOpts {
  int walls = 0, scalar_fixed = 0, rectangle = 0, channel = 0, exchange = 0;
  double omega = 1.2, omega_g = 1.7;
  bool fast = true;
  bool kbc = false;  // --fluid kbc
  double s2 = 1.2;   // --s2
  bool buoyant = false;
  lbm_ade_buoyancy buoy{};
  const lbm_ade_buoyancy* buoyancy() const { return buoyant ? &buoy : nullptr; }
  // the JSON line's field, empty without --buoyancy
  std::string buoyancy_field() const {
    if (!buoyant) return "";
    char t[256];
    std::snprintf(t, sizeof t, ", \"buoyancy\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g]", buoy.beta_r, buoy.beta_c,
                  buoy.c_ref, buoy.u_shift, buoy.guo_a, buoy.guo_b);
    return t;
  }
};

// shear wave + Taylor-Green vortices on the GLOBAL box, scalar: a Gaussian blob; f = feq(u, rho), g = feq(u + w, C) in
// the reference's operation order (solver.cpp:51-62) -- the same bits for every decomposition
const double kW[2] = {3e-3, 3e-3};
// kbc: rho = 1 on the shear wave u = (U0 / 2, U0 sin(2 pi r / Rg)), U0 = 0.02, of passive_scalar_box --fluid kbc; f9 is then
// a placeholder (upload_rows forms f on the device, lbm_kbc_equilibrium) and (rho_u[0], rho_u[1], rho_u[2]) = (rho, u)
void init_node(double* f9, double* g9, int gr, int c, int Rg, int C, bool kbc = false, double* rho_u = nullptr) {
  const double pi = 3.14159265358979323846;
  const double x = 2 * pi * gr / Rg, y = 2 * pi * c / C;
  const double u0 = kbc ? 0.01 : 0.03 * std::sin(x) * std::cos(y);
  const double u1 = kbc ? 0.02 * std::sin(x) : 0.03 * std::sin(x) - 0.02 * std::cos(x) * std::sin(y);
  const double rho = kbc ? 1.0 : 1.0 + 0.01 * std::cos(2 * x);
  if (rho_u) rho_u[0] = rho, rho_u[1] = u0, rho_u[2] = u1;
  const double dr = gr - 0.45 * Rg, dc = c - 0.55 * C, s = 0.12 * std::min(Rg, C);
  const double conc = 1e-3 * std::exp(-(dr * dr + dc * dc) / (2 * s * s));
  d2q9_equilibrium(f9, rho, u0, u1);
  d2q9_equilibrium(g9, conc, u0 + kW[0], u1 + kW[1]);
}

// the plain compressible fluid and the scalar, both halves in the form of --form
lbm_bgk_params fluid_params(const Args& a) {
  lbm_bgk_params p{};
  p.omega = a.omega;
  p.form = a.fast ? LBM_FORM_REASSOCIATED : LBM_FORM_REFERENCE_ORDER;
  return p;
}
// the fluid by model (the _m entry points): --fluid kbc with the rate --s2, in the form of --form
lbm_ade_fluid fluid_model(const Args& a) {
  lbm_ade_fluid m{};
  m.model = a.kbc ? LBM_MODEL_KBC : LBM_MODEL_BGK;
  m.bgk = fluid_params(a);
  m.kbc = lbm_kbc_params{a.s2, a.fast ? LBM_FORM_REASSOCIATED : LBM_FORM_REFERENCE_ORDER};
  return m;
}
lbm_ade_params scalar_params(const Args& a) {
  return lbm_ade_params{a.omega_g, kW[0], kW[1], a.fast ? LBM_FORM_REASSOCIATED : LBM_FORM_REFERENCE_ORDER};
}

lbm_bc global_bc(const Args& a) {
  lbm_bc b{0, 0, 0, 0, 0, 1.0, 1.0, 0.0, 0.0};
  if (a.walls) {
    b.row_lo = b.row_hi = LBM_EDGE_BOUNCE_BACK;
    b.col_lo = a.channel ? LBM_EDGE_PERIODIC : LBM_EDGE_BOUNCE_BACK;  // --channel: the inlet and the outlet are the table's
    b.col_hi = a.channel ? LBM_EDGE_PERIODIC : LBM_EDGE_SPECULAR;
  }
  return b;
}

// --scalar-fixed: the column-0 profile of the global box on the device (Rg values), NULL without the flag
double* scalar_profile(const Args& a, int Rg) {
  if (!a.scalar_fixed) return nullptr;
  std::vector<double> p(Rg);
  for (int r = 0; r < Rg; ++r) p[r] = r >= Rg - Rg / 4 ? 1e-3 : 0.0;
  double* d = nullptr;
  check(lbm_malloc((void**)&d, (size_t)Rg * 8), "lbm_malloc");
  check(lbm_memcpy_h2d(d, p.data(), (size_t)Rg * 8, nullptr), "h2d");
  check(lbm_stream_sync(nullptr), "sync");
  return d;
}

// the scalar's walls of the rows [row0, row0 + R) of the global box: the profile's slice; a seam (HALO row edge) carries
// no FIXED row -- what lbm_ring_ade_step_ex does with the global descriptor
lbm_ade_scalar_bc scalar_bc(const double* profile, int row0, const lbm_bc& bc) {
  lbm_ade_scalar_bc s{};
  s.mode[0] = bc.row_lo == LBM_EDGE_HALO ? LBM_ADE_SCALAR_NO_FLUX : LBM_ADE_SCALAR_FIXED;
  s.conc[0] = 1e-3;
  s.mode[2] = s.mode[3] = LBM_ADE_SCALAR_FIXED;
  s.profile[2] = profile ? profile + row0 : nullptr;
  s.conc[3] = 0.0;
  return s;
}

// --rectangle: the table of the global box (test/rectangle_sedimentation_test.cpp:184-196, :220-232 scaled as
// scripts/ade_bench.py --interior-walls scales it), not finalized; NULL without the flag
lbm_ade_iwalls* rectangle_table(const Args& a, int Rg) {
  if (!a.rectangle) return nullptr;
  const int C = a.cols, r_top = Rg - Rg / 3, c1 = C * 2 / 8, c2 = C * 5 / 16, n_side = Rg / 3 - 2;  // rows r_top + 1 .. Rg - 2
  if (n_side < 1) throw std::runtime_error("--rectangle 1 needs at least 9 global rows");
  const unsigned neg = LBM_ADE_FACE_COL_NEG, pos = LBM_ADE_FACE_COL_POS, top = LBM_ADE_FACE_ROW_NEG;
  const int fx = LBM_ADE_SCALAR_FIXED;
  lbm_ade_iwalls* t = nullptr;
  check(lbm_ade_iwalls_create(&t, Rg, C), "lbm_ade_iwalls_create");
  check(lbm_ade_iwalls_add(t, r_top + 1, c1, 1, 0, n_side, neg, neg, fx, 0.0), "lbm_ade_iwalls_add");  // first wall; g runs
  check(lbm_ade_iwalls_add(t, -1, c1, 1, 0, 1, 0, neg & ~0x40u, fx, 0.0), "lbm_ade_iwalls_add");  // through the last row, slot 7 of its foot left to the bottom wall
  check(lbm_ade_iwalls_add(t, r_top, c1, 0, 1, c2 - c1 + 1, top, top, fx, 0.0), "lbm_ade_iwalls_add");  // ceiling
  check(lbm_ade_iwalls_add(t, r_top + 1, c2, 1, 0, n_side, pos, pos, fx, 0.0), "lbm_ade_iwalls_add");   // second wall
  return t;
}
// the finalized view of rows [row0, row0 + R) of the global table; NULL for NULL
lbm_ade_iwalls* slab_view(const lbm_ade_iwalls* global, int row0, int R) {
  if (!global) return nullptr;
  lbm_ade_iwalls* v = nullptr;
  check(lbm_ade_iwalls_slab(&v, global, row0, R), "lbm_ade_iwalls_slab");
  check(lbm_ade_iwalls_finalize(v), "lbm_ade_iwalls_finalize");
  return v;
}

// --channel: the open table of the global box, finalized (the one block of --check and the emulation's first iteration run
// it); NULL without the flag
lbm_ade_open* channel_table(const Args& a, int Rg) {
  if (!a.channel) return nullptr;
  lbm_ade_open* t = nullptr;
  check(lbm_ade_open_create(&t, Rg, a.cols), "lbm_ade_open_create");
  check(lbm_ade_open_add_channel(t, 0.03, 1e-3, Rg / 4), "lbm_ade_open_add_channel");
  check(lbm_ade_open_finalize(t), "lbm_ade_open_finalize");
  return t;
}
// the finalized view of rows [row0, row0 + R) of the global open table; NULL for NULL
lbm_ade_open* open_view(const lbm_ade_open* global, int row0, int R) {
  if (!global) return nullptr;
  lbm_ade_open* v = nullptr;
  check(lbm_ade_open_slab(&v, global, row0, R), "lbm_ade_open_slab");
  check(lbm_ade_open_finalize(v), "lbm_ade_open_finalize");
  return v;
}

// --check: the values of the one block's lattices that are not finite.  The comparison is on bit patterns, and equal NaNs
// are equal bits: a yardstick that is not finite is a failed check, and the JSON line says how many values ("one_block_nonfinite")
size_t count_nonfinite(const std::vector<double>& a) {
  size_t n = 0;
  for (double x : a) n += std::isfinite(x) ? 0 : 1;
  return n;
}
std::string nonfinite_field(int check, size_t n) {
  return check ? ", \"one_block_nonfinite\": " + std::to_string(n) : "";
}

// pre-collision f, g of global rows [row0, row0 + R) into lattices of geometry g (owned rows; the rest zero).  kbc: f =
// lbm_kbc_equilibrium(rho, u) without the u^2 terms, formed on the device node by node -- the same bits for every
// decomposition
void upload_rows(double* f, double* h, const lbm_geom& g, int row0, int Rg, bool kbc) {
  const int R = g.R, C = g.C;
  const lbm_geom d{R, C, 0, 0, 0};
  const size_t n = (size_t)R * C;
  std::vector<double> hf(9 * n), hg(9 * n), hm(kbc ? 3 * n : 0);  // hm: rho [R][C], then u [2][R][C]
  double f9[9], g9[9], m[3];
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < C; ++c) {
      init_node(f9, g9, row0 + r, c, Rg, C, kbc, m);
      const size_t i = (size_t)r * C + c;
      for (int q = 0; q < 9; ++q) {
        hf[(size_t)q * n + i] = f9[q];
        hg[(size_t)q * n + i] = g9[q];
      }
      if (kbc)
        for (int k = 0; k < 3; ++k) hm[k * n + i] = m[k];
    }
  double* stage = nullptr;
  check(lbm_malloc((void**)&stage, hf.size() * 8), "lbm_malloc");
  for (auto [dst, src] : {std::pair<double*, std::vector<double>*>{f, &hf}, {h, &hg}}) {
    check(lbm_memset(dst, 0, plane_doubles(g) * 9 * 8, nullptr), "memset");
    if (kbc && dst == f) {
      double* mom = alloc_doubles(3 * n);
      check(lbm_memcpy_h2d(mom, hm.data(), hm.size() * 8, nullptr), "h2d");
      check(lbm_kbc_equilibrium(stage, mom, mom + n, R, C, /*zero_u2=*/1, nullptr), "lbm_kbc_equilibrium");
      check(lbm_stream_sync(nullptr), "sync");
      lbm_free(mom);
    } else {
      check(lbm_memcpy_h2d(stage, src->data(), src->size() * 8, nullptr), "h2d");
    }
    check(lbm_lattice_copy_rows(dst, &g, 0, stage, &d, 0, R, nullptr), "lbm_lattice_copy_rows");
  }
  check(lbm_stream_sync(nullptr), "sync");
  lbm_free(stage);
}

// One block of Rg x C (ghost 0, dense), collide-only + `steps` fused steps: the yardstick of --check.  Returns f, g of
// the owned rows as dense [9][Rg][C] on the host.
// With an open table (--channel) the _o entry points run it and its carry comes back as well (the table's order).
// wallx_out (--exchange): the wall exchange of the stream from that state, lbm_ade_wallx_rows + lbm_ade_wallx_fold.
void one_block(const Args& a, int Rg, const lbm_bgk_params& fl, const lbm_ade_params& sc, lbm_ade_iwalls* walls,
               std::vector<double>& f_out, std::vector<double>& g_out, const lbm_ade_open* open = nullptr,
               std::vector<double>* carry_out = nullptr, std::vector<double>* wallx_out = nullptr) {
  if (walls) check(lbm_ade_iwalls_finalize(walls), "lbm_ade_iwalls_finalize");  // the global table: this is its one use on the device
  const lbm_geom g{Rg, a.cols, 0, 0, 0};
  const lbm_bc bc = global_bc(a);
  double *f[2] = {alloc_lattice(g), alloc_lattice(g)}, *h[2] = {alloc_lattice(g), alloc_lattice(g)};
  double* prof = scalar_profile(a, Rg);
  const lbm_ade_scalar_bc sbc = scalar_bc(prof, 0, bc);
  upload_rows(f[0], h[0], g, 0, Rg, a.kbc);
  const lbm_ade_fluid fm = fluid_model(a);
  double* carry[2] = {alloc_doubles((size_t)lbm_ade_open_carry_len(open)), alloc_doubles((size_t)lbm_ade_open_carry_len(open))};
  if (a.kbc)
    check(lbm_ade_collide_m(f[1], h[1], f[0], h[0], &g, &bc, &fm, &sc, nullptr, nullptr, nullptr, nullptr, nullptr),
          "lbm_ade_collide_m");
  else if (open)
    check(lbm_ade_collide_o(f[1], h[1], f[0], h[0], &g, &bc, &fl, &sc, nullptr, a.buoyancy(), open, carry[1], nullptr, nullptr,
                            nullptr, nullptr), "lbm_ade_collide_o");
  else
    check(lbm_ade_collide_b(f[1], h[1], f[0], h[0], &g, &bc, &fl, &sc, nullptr, a.buoyancy(), nullptr, nullptr, nullptr,
                            nullptr), "lbm_ade_collide_b");
  int cur = 1;
  for (int t = 0; t < a.warmup + a.steps; ++t, cur ^= 1)
    if (a.kbc)
      check(lbm_ade_stream_collide_m(f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &g, &bc, &fm, &sc, prof ? &sbc : nullptr, walls, 0,
                                     Rg, nullptr, nullptr, nullptr, nullptr), "lbm_ade_stream_collide_m");
    else if (open)
      check(lbm_ade_stream_collide_o(f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &g, &bc, &fl, &sc, prof ? &sbc : nullptr,
                                     a.buoyancy(), walls, open, carry[cur], carry[cur ^ 1], 0, Rg, nullptr, nullptr, nullptr,
                                     nullptr), "lbm_ade_stream_collide_o");
    else
      check(lbm_ade_stream_collide_w(f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &g, &bc, &fl, &sc, prof ? &sbc : nullptr,
                                     a.buoyancy(), walls, 0, Rg, nullptr, nullptr, nullptr, nullptr), "lbm_ade_stream_collide_w");
  if (wallx_out) {
    double* t = alloc_doubles((size_t)LBM_WALLX_NQ * (Rg + 1));  // the row table, then the folded values
    check(lbm_ade_wallx_rows(t, Rg, 0, f[cur], h[cur], &g, &bc, &fl, &sc, prof ? &sbc : nullptr, a.buoyancy(), walls, nullptr,
                             0, Rg, nullptr), "lbm_ade_wallx_rows");
    check(lbm_ade_wallx_fold(t + (size_t)LBM_WALLX_NQ * Rg, t, Rg, 0, Rg, nullptr), "lbm_ade_wallx_fold");
    *wallx_out = doubles_to_host(t + (size_t)LBM_WALLX_NQ * Rg, LBM_WALLX_NQ);
    lbm_free(t);
  }
  if (prof) lbm_free(prof);
  if (carry_out) *carry_out = doubles_to_host(carry[cur], (size_t)lbm_ade_open_carry_len(open));
  for (double* c : carry) lbm_free(c);
  f_out = owned_to_host(f[cur], g);
  g_out = owned_to_host(h[cur], g);
  for (int k = 0; k < 2; ++k) {
    lbm_free(f[k]);
    lbm_free(h[k]);
  }
}

// The one-block step of a slab-sized lattice (R x C, ghost 0, periodic, padded as the solver context pads): ms per step
struct SlabSizedBlock {
  lbm_geom g;
  double *f[2], *h[2];
  int cur = 0;
  void* ev[2];
  double ms = 0;
  SlabSizedBlock(int R, int C, bool kbc) : g(padded_geom(R, C, 0)) {
    for (int k = 0; k < 2; ++k) {
      f[k] = alloc_lattice(g);
      h[k] = alloc_lattice(g);
      check(lbm_event_create(&ev[k]), "lbm_event_create");
    }
    upload_rows(f[0], h[0], g, 0, R, kbc);
  }
  // fm: the fluid by model where it is a KBC fluid (NULL: the BGK fluid fl)
  void step(const lbm_bgk_params& fl, const lbm_ade_params& sc, const lbm_ade_buoyancy* by, bool timed,
            const lbm_ade_fluid* fm = nullptr) {
    check(lbm_event_record(ev[0], nullptr), "event");
    if (fm)
      check(lbm_ade_stream_collide_m(f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &g, nullptr, fm, &sc, nullptr, nullptr, 0, g.R,
                                     nullptr, nullptr, nullptr, nullptr), "lbm_ade_stream_collide_m");
    else
      check(lbm_ade_stream_collide_b(f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &g, nullptr, &fl, &sc, nullptr, by, 0, g.R,
                                     nullptr, nullptr, nullptr, nullptr), "lbm_ade_stream_collide_b");
    check(lbm_event_record(ev[1], nullptr), "event");
    float m = 0;
    check(lbm_event_elapsed_ms(&m, ev[0], ev[1]), "elapsed");
    if (timed) ms += m;
    cur ^= 1;
  }
  ~SlabSizedBlock() {
    for (int k = 0; k < 2; ++k) {
      lbm_free(f[k]);
      lbm_free(h[k]);
      lbm_event_destroy(ev[k]);
    }
  }
};

// --emulate N: every slab in turn on ONE GPU.  A slab's step is what lbm_ring_ade_step_w enqueues -- FRAME on the ring's
// stream, INNER on the main stream beside it (each followed by the wall pass of its rows where the slab's view of the
// table has nodes there), the pack behind FRAME -- with the messages (both lattices, 2 x 3 rows per
// side) as device copies between the steps.  Slab k's edges: the global box's, seams HALO (both row edges of a closed
// ring).  The initial state is the one block's post-collision state, scattered into the slabs with their ghost rows.
int run_emulated(const Args& a, int N) {
  check(lbm_set_device(0), "lbm_set_device");
  const int R = a.rows, C = a.cols, Rg = R * N, E = a.edge_rows;
  if (E < 1 || 2 * E >= R) throw std::runtime_error("--edge-rows must satisfy 1 <= E and 2 E < rows");
  const lbm_bgk_params fl = fluid_params(a);
  const lbm_ade_params sc = scalar_params(a);
  const lbm_ade_fluid fm = fluid_model(a);
  const lbm_bc gbc = global_bc(a);
  const bool closed = !a.walls;
  const lbm_geom g = padded_geom(R, C, 1);
  const size_t msg = (size_t)lbm_halo_rows(1) * C;  // per lattice
  double* prof = scalar_profile(a, Rg);
  lbm_ade_iwalls* table = rectangle_table(a, Rg);
  lbm_ade_open* channel = channel_table(a, Rg);
  struct Slab {
    lbm_bc bc;
    lbm_ade_scalar_bc sbc;
    lbm_ade_iwalls* walls;
    lbm_ade_open* open;  // the slab's view of the channel and its two carries (carry[k] goes with f[k], h[k])
    double* carry[2];
    double *f[2], *h[2];
  };
  std::vector<Slab> S(N);
  EmulatedLinks links(N, closed);  // a message: f then g
  {
    // the one block's post-collision state (lbm_ade_collide on the global lattice), scattered into the slabs
    const lbm_geom gg{Rg, C, 0, 0, 0};
    double *f0 = alloc_lattice(gg), *h0 = alloc_lattice(gg), *fp = alloc_lattice(gg), *hp = alloc_lattice(gg);
    upload_rows(f0, h0, gg, 0, Rg, a.kbc);
    double* carry0 = alloc_doubles((size_t)lbm_ade_open_carry_len(channel));  // of the global table: a view's is a slice of it
    if (a.kbc)
      check(lbm_ade_collide_m(fp, hp, f0, h0, &gg, &gbc, &fm, &sc, nullptr, nullptr, nullptr, nullptr, nullptr), "lbm_ade_collide_m");
    else if (channel)
      check(lbm_ade_collide_o(fp, hp, f0, h0, &gg, &gbc, &fl, &sc, nullptr, a.buoyancy(), channel, carry0, nullptr, nullptr,
                              nullptr, nullptr), "lbm_ade_collide_o");
    else
      check(lbm_ade_collide_b(fp, hp, f0, h0, &gg, &gbc, &fl, &sc, nullptr, a.buoyancy(), nullptr, nullptr, nullptr, nullptr),
            "lbm_ade_collide_b");
    size_t first = 0;  // the views partition the table in its order
    for (int k = 0; k < N; ++k) {
      Slab& s = S[k];
      s.bc = gbc;
      if (links.prev(k)) s.bc.row_lo = LBM_EDGE_HALO;
      if (links.next(k)) s.bc.row_hi = LBM_EDGE_HALO;
      s.sbc = scalar_bc(prof, k * R, s.bc);
      s.walls = slab_view(table, k * R, R);
      s.open = open_view(channel, k * R, R);
      const size_t len = (size_t)lbm_ade_open_carry_len(s.open);
      for (int b = 0; b < 2; ++b) s.carry[b] = alloc_doubles(len);
      if (len) check(lbm_memcpy_d2d(s.carry[0], carry0 + first, len * 8, nullptr), "lbm_memcpy_d2d");
      first += len;
      for (int b = 0; b < 2; ++b) {
        s.f[b] = alloc_lattice(g);
        s.h[b] = alloc_lattice(g);
        links.alloc(k, /*side=*/b, 2 * msg, 2 * msg);
      }
      // owned rows and the ghost rows beside them (wrapping on a closed ring): the exchange would bring the same bits
      for (int r = -1; r <= R; ++r) {
        const int gr = k * R + r;
        if (gr < 0 && !closed) continue;
        if (gr >= Rg && !closed) continue;
        const int src = (gr + Rg) % Rg;
        check(lbm_lattice_copy_rows(s.f[0], &g, r, fp, &gg, src, 1, nullptr), "lbm_lattice_copy_rows");
        check(lbm_lattice_copy_rows(s.h[0], &g, r, hp, &gg, src, 1, nullptr), "lbm_lattice_copy_rows");
      }
    }
    check(lbm_stream_sync(nullptr), "sync");
    for (double* p : {f0, h0, fp, hp, carry0}) lbm_free(p);
  }
  EdgeStream es;
  SlabSizedBlock block(R, C, a.kbc);
  auto part = [&](Slab& s, int cur, int which, lbm_stream_t st) {
    if (a.kbc) {
      check(lbm_ade_stream_collide_part_m(s.f[cur ^ 1], s.h[cur ^ 1], s.f[cur], s.h[cur], &g, &s.bc, &fm, &sc,
                                          prof ? &s.sbc : nullptr, s.walls, which, E, nullptr, nullptr, nullptr, st),
            "lbm_ade_stream_collide_part_m");
      return;
    }
    if (s.open) {
      check(lbm_ade_stream_collide_part_o(s.f[cur ^ 1], s.h[cur ^ 1], s.f[cur], s.h[cur], &g, &s.bc, &fl, &sc,
                                          prof ? &s.sbc : nullptr, a.buoyancy(), s.walls, s.open, s.carry[cur], s.carry[cur ^ 1],
                                          which, E, nullptr, nullptr, nullptr, st), "lbm_ade_stream_collide_part_o");
      return;
    }
    check(lbm_ade_stream_collide_part_w(s.f[cur ^ 1], s.h[cur ^ 1], s.f[cur], s.h[cur], &g, &s.bc, &fl, &sc,
                                        prof ? &s.sbc : nullptr, a.buoyancy(), s.walls, which, E, nullptr, nullptr, nullptr,
                                        st), "lbm_ade_stream_collide_part_w");
  };
  auto pack = [&](int k, double* f, double* h, lbm_stream_t st) {
    for (int side = 0; side < 2; ++side) {
      if (!links.has(k, side)) continue;
      check(lbm_halo_pack(links.send(k, side), f, &g, 1, side, st), "lbm_halo_pack");
      check(lbm_halo_pack(links.send(k, side) + msg, h, &g, 1, side, st), "lbm_halo_pack");
    }
  };
  int cur = 0;
  for (int i = 0; i < a.warmup + a.steps; ++i) {
    for (int k = 0; k < N; ++k) {
      Slab& s = S[k];
      links.begin(k);
      if (links.prev(k) || links.next(k)) {
        es.fork();
        part(s, cur, LBM_ADE_PART_FRAME, es.edge);
        part(s, cur, LBM_ADE_PART_INNER, nullptr);
        pack(k, s.f[cur ^ 1], s.h[cur ^ 1], es.edge);
        es.join();
      } else {
        part(s, cur, LBM_ADE_PART_FRAME, nullptr);
        part(s, cur, LBM_ADE_PART_INNER, nullptr);
      }
      links.end(k);
    }
    links.deliver(2 * msg);  // slab k's side-1 message is slab k+1's side-0 input and vice versa
    for (int k = 0; k < N; ++k) {
      Slab& s = S[k];
      for (int side = 0; side < 2; ++side) {
        if (!links.has(k, side)) continue;
        check(lbm_halo_unpack(s.f[cur ^ 1], links.recv(k, side), &g, 1, side, nullptr), "lbm_halo_unpack");
        check(lbm_halo_unpack(s.h[cur ^ 1], links.recv(k, side) + msg, &g, 1, side, nullptr), "lbm_halo_unpack");
      }
      links.add_elapsed(k, i >= a.warmup);
    }
    block.step(fl, sc, a.buoyancy(), i >= a.warmup, a.kbc ? &fm : nullptr);  // alternated with the chain's step
    cur ^= 1;
  }
  check(lbm_stream_sync(es.edge), "sync");
  // --exchange: every slab fills its rows of ONE global table from its own lattices (ghost rows as the last exchange left
  // them) and its view of the walls; the fold of that table against the one block's
  std::vector<double> wallx, wallx_block;
  if (a.exchange) {
    double* t = alloc_doubles((size_t)LBM_WALLX_NQ * (Rg + 1));  // the row table, then the folded values
    for (int k = 0; k < N; ++k)
      check(lbm_ade_wallx_rows(t, Rg, k * R, S[k].f[cur], S[k].h[cur], &g, &S[k].bc, &fl, &sc, prof ? &S[k].sbc : nullptr,
                               a.buoyancy(), S[k].walls, nullptr, 0, R, nullptr), "lbm_ade_wallx_rows");
    check(lbm_ade_wallx_fold(t + (size_t)LBM_WALLX_NQ * Rg, t, Rg, 0, Rg, nullptr), "lbm_ade_wallx_fold");
    wallx = doubles_to_host(t + (size_t)LBM_WALLX_NQ * Rg, LBM_WALLX_NQ);
    lbm_free(t);
  }
  if (prof) lbm_free(prof);
  int bad = 0;
  std::vector<double> want[2], want_carry;
  if (a.check || a.exchange)
    one_block(a, Rg, fl, sc, table, want[0], want[1], channel, &want_carry, a.exchange ? &wallx_block : nullptr);
  if (a.exchange) {
    for (const auto* v : {&wallx, &wallx_block}) {
      std::printf(v == &wallx ? "wallx_slabs=" : "wallx_one_block=");
      for (int q = 0; q < LBM_WALLX_NQ; ++q) std::printf("%s%.17g", q ? "," : "", (*v)[q]);
      std::printf("\n");
    }
  }
  size_t nonfinite = 0;
  if (a.check) {
    nonfinite = count_nonfinite(want[0]) + count_nonfinite(want[1]);
    bad += nonfinite ? 1 : 0;
    size_t first = 0;
    for (int k = 0; k < N; ++k) {
      for (int lat = 0; lat < 2; ++lat)
        bad += mismatching_planes(want[lat], Rg, owned_to_host(lat ? S[k].h[cur] : S[k].f[cur], g), R, k * R, C);
      const size_t len = (size_t)lbm_ade_open_carry_len(S[k].open);
      bad += mismatching_doubles(want_carry.data() + first, doubles_to_host(S[k].carry[cur], len).data(), len) ? 1 : 0;
      first += len;
    }
  }
  const double slowest = links.slowest_ms() / a.steps, blk = block.ms / a.steps;
  std::printf("{\"driver\": \"slab_ring_ade\", \"mode\": \"emulated %s on one GPU\", \"slabs\": %d, \"rows_per_slab\": %d, "
              "\"cols\": %d, \"global_rows\": %d, \"walls\": %d, \"scalar_fixed\": %d, \"form\": \"%s\", \"fluid\": \"%s\", \"s2\": %.17g, \"steps\": %d, "
              "\"edge_rows\": %d, \"message_rows_per_side\": %d, \"slowest_slab_ms_per_step\": %.4f, "
              "\"one_block_slab_sized_ms_per_step\": %.4f, \"slab_rate_over_one_block\": %.3f, \"per_slab_ms\": [",
              closed ? "closed ring" : "chain", N, R, C, Rg, a.walls, a.scalar_fixed, a.fast ? "fast" : "ref",
              a.kbc ? "kbc" : "bgk", a.s2, a.steps, E,
              2 * lbm_halo_rows(1), slowest, blk, blk / slowest);
  for (int k = 0; k < N; ++k) std::printf("%s%.4f", k ? ", " : "", links.ms(k) / a.steps);
  std::printf("]");
  if (table) {
    std::printf(", \"interior_wall_nodes\": %d, \"interior_wall_nodes_per_slab\": [", lbm_ade_iwalls_count(table));
    for (int k = 0; k < N; ++k) std::printf("%s%d", k ? ", " : "", lbm_ade_iwalls_count(S[k].walls));
    std::printf("]");
  }
  if (channel) {
    std::printf(", \"open_nodes\": %d, \"open_nodes_per_slab\": [", lbm_ade_open_count(channel));
    for (int k = 0; k < N; ++k) std::printf("%s%d", k ? ", " : "", lbm_ade_open_count(S[k].open));
    std::printf("]");
  }
  std::printf("%s%s%s}\n", a.buoyancy_field().c_str(), nonfinite_field(a.check, nonfinite).c_str(), check_field(a.check, bad));
  std::fflush(stdout);
  for (auto& s : S) {
    for (int b = 0; b < 2; ++b) {
      lbm_free(s.f[b]);
      lbm_free(s.h[b]);
      lbm_free(s.carry[b]);
    }
    lbm_ade_iwalls_destroy(s.walls);
    lbm_ade_open_destroy(s.open);
  }
  lbm_ade_iwalls_destroy(table);
  lbm_ade_open_destroy(channel);
  return bad ? 3 : 0;
}

int run_rank(const Args& a, int rank, int world, int local_rank) {
  check(lbm_set_device(ring_device(local_rank)), "lbm_set_device");
  const int R = a.rows, C = a.cols, Rg = R * world;
  const lbm_bgk_params fl = fluid_params(a);
  const lbm_ade_params sc = scalar_params(a);
  const lbm_ade_fluid fm = fluid_model(a);
  const lbm_bc gbc = global_bc(a);
  const lbm_geom g = padded_geom(R, C, 1);
  unsigned char id[128];
  share_unique_id(id, rank, world, a.id_file);
  lbm_ring* ring = nullptr;
  check(lbm_ring_create(&ring, id, rank, world, &g, /*periodic=*/a.walls ? 0 : 1), "lbm_ring_create");
  double *f[2] = {alloc_lattice(g), alloc_lattice(g)}, *h[2] = {alloc_lattice(g), alloc_lattice(g)};
  upload_rows(f[1], h[1], g, rank * R, Rg, a.kbc);  // pre-collision, then the first driver iteration: collide + one exchange
  lbm_ade_open* channel = channel_table(a, Rg);  // the global table, this slab's view and its carries
  lbm_ade_open* open = open_view(channel, rank * R, R);
  double* carry[2] = {alloc_doubles((size_t)lbm_ade_open_carry_len(open)), alloc_doubles((size_t)lbm_ade_open_carry_len(open))};
  if (a.kbc)
    check(lbm_ring_ade_collide_m(ring, f[0], h[0], f[1], h[1], &gbc, &fm, &sc, nullptr, nullptr), "lbm_ring_ade_collide_m");
  else if (open)
    check(lbm_ring_ade_collide_o(ring, f[0], h[0], f[1], h[1], &gbc, &fl, &sc, nullptr, a.buoyancy(), open, carry[0], nullptr),
          "lbm_ring_ade_collide_o");
  else
    check(lbm_ring_ade_collide_b(ring, f[0], h[0], f[1], h[1], &gbc, &fl, &sc, nullptr, a.buoyancy(), nullptr),
          "lbm_ring_ade_collide_b");
  double* prof = scalar_profile(a, Rg);
  const lbm_ade_scalar_bc sbc = scalar_bc(prof, rank * R, gbc);  // the global descriptor, this slab's profile rows
  lbm_ade_iwalls* table = rectangle_table(a, Rg);                 // the global table, this slab's view
  lbm_ade_iwalls* walls = slab_view(table, rank * R, R);
  int cur = 0;
  auto step = [&]() {
    if (a.kbc)
      check(lbm_ring_ade_step_m(ring, f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &gbc, &fm, &sc, prof ? &sbc : nullptr, walls,
                                a.edge_rows, nullptr), "lbm_ring_ade_step_m");
    else if (open)
      check(lbm_ring_ade_step_o(ring, f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &gbc, &fl, &sc, prof ? &sbc : nullptr,
                                a.buoyancy(), walls, open, carry[cur], carry[cur ^ 1], a.edge_rows, nullptr), "lbm_ring_ade_step_o");
    else
      check(lbm_ring_ade_step_w(ring, f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &gbc, &fl, &sc, prof ? &sbc : nullptr,
                                a.buoyancy(), walls, a.edge_rows, nullptr), "lbm_ring_ade_step_w");
    cur ^= 1;
  };
  double tmax = 0;
  if (const int failed = timed_ring_run(ring, "slab_ring_ade", a, rank, world, a.warmup, a.steps, step, &tmax)) return failed;

  int bad = 0;
  size_t nonfinite = 0;
  if (a.check) {
    publish_owned_rows(a, ".f", rank, f[cur], g);
    publish_owned_rows(a, ".g", rank, h[cur], g);
    if (rank == 0) {
      std::vector<double> want[2];
      one_block(a, Rg, fl, sc, table, want[0], want[1], channel);
      nonfinite = count_nonfinite(want[0]) + count_nonfinite(want[1]);
      bad += nonfinite ? 1 : 0;
      for (int r = 0; r < world; ++r)
        for (int lat = 0; lat < 2; ++lat)
          bad += mismatching_planes(want[lat], Rg, read_owned_rows(a, lat ? ".g" : ".f", r, R, C), R, r * R, C);
    }
  }
  if (rank == 0) {
    // the one-block step of a slab-sized lattice on this GPU, after the ring's run
    SlabSizedBlock block(R, C, a.kbc);
    for (int i = 0; i < a.warmup + a.steps; ++i) block.step(fl, sc, a.buoyancy(), i >= a.warmup, a.kbc ? &fm : nullptr);
    const double ms = 1e3 * tmax / a.steps, blk = block.ms / a.steps;
    std::printf("{\"driver\": \"slab_ring_ade\", \"n_gpus\": %d, \"rows_per_gpu\": %d, \"cols\": %d, \"walls\": %d, "
                "\"scalar_fixed\": %d, \"form\": \"%s\", \"fluid\": \"%s\", \"s2\": %.17g, \"steps\": %d, \"edge_rows\": %d, "
                "\"message_rows_per_side\": %d, "
                "\"slowest_slab_ms_per_step\": %.4f, \"one_block_slab_sized_ms_per_step\": %.4f, \"slab_rate_over_one_block\": %.3f, "
                "\"mlups\": %.1f%s%s%s%s%s}\n",
                world, R, C, a.walls, a.scalar_fixed, a.fast ? "fast" : "ref", a.kbc ? "kbc" : "bgk", a.s2, a.steps, a.edge_rows,
                2 * lbm_halo_rows(1), ms, blk, blk / ms,
                (double)Rg * C / (ms * 1e3),
                table ? (", \"interior_wall_nodes\": " + std::to_string(lbm_ade_iwalls_count(table))).c_str() : "",
                channel ? (", \"open_nodes\": " + std::to_string(lbm_ade_open_count(channel))).c_str() : "",
                a.buoyancy_field().c_str(), nonfinite_field(a.check, nonfinite).c_str(), check_field(a.check, bad));
    std::fflush(stdout);
  }
  lbm_ring_destroy(ring);
  lbm_ade_iwalls_destroy(walls);
  lbm_ade_iwalls_destroy(table);
  lbm_ade_open_destroy(open);
  lbm_ade_open_destroy(channel);
  if (prof) lbm_free(prof);
  for (int k = 0; k < 2; ++k) {
    lbm_free(f[k]);
    lbm_free(h[k]);
    lbm_free(carry[k]);
  }
  return bad ? 3 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  parse_ring_opts(a, argc, argv, /*rows=*/512, /*cols=*/1024, /*steps=*/50, /*warmup=*/5, /*edge_rows=*/16);
  a.steps = std::max(1, a.steps);
  a.warmup = std::max(0, a.warmup);
  // the default edge band on a slab too low for it: the widest that leaves an INNER row (an --edge-rows given is taken as it is)
  if (arg_value(argc, argv, "--edge-rows", "").empty()) a.edge_rows = std::max(1, std::min(a.edge_rows, (a.rows - 1) / 2));
  a.walls = int_arg(argc, argv, "--walls", 0);
  a.scalar_fixed = int_arg(argc, argv, "--scalar-fixed", 0);
  if (a.scalar_fixed && !a.walls) {
    std::fprintf(stderr, "--scalar-fixed 1 needs --walls 1 (fixed-concentration walls sit on walls of the fluid)\n");
    return 1;
  }
  a.rectangle = int_arg(argc, argv, "--rectangle", 0);
  a.exchange = int_arg(argc, argv, "--exchange", 0);
  if (a.exchange && (!a.rectangle || arg_value(argc, argv, "--emulate", "").empty())) {
    std::fprintf(stderr, "--exchange 1 needs --emulate N and --rectangle 1 (ranks fold their row tables over a transport of "
                         "their own: lbm_ade_wallx_fold_host)\n");
    return 1;
  }
  if (a.rectangle && !a.walls) {
    std::fprintf(stderr, "--rectangle 1 needs --walls 1 (the rectangle stands on the bounce-back last row of the chain)\n");
    return 1;
  }
  a.channel = int_arg(argc, argv, "--channel", 0);
  if (a.channel && (!a.walls || a.scalar_fixed)) {
    std::fprintf(stderr, "--channel 1 needs --walls 1 (the channel's floor is the bounce-back last row of the chain) and no "
                         "--scalar-fixed (its column walls are the channel's inlet and outlet)\n");
    return 1;
  }
  a.omega = std::atof(arg_value(argc, argv, "--omega", "1.2").c_str());
  a.omega_g = std::atof(arg_value(argc, argv, "--omega-g", "1.7").c_str());
  const std::string form = arg_value(argc, argv, "--form", "fast");
  if (form != "fast" && form != "ref") {
    std::fprintf(stderr, "slab_ring_ade: --form ref|fast\n");
    return 2;
  }
  a.fast = form == "fast";
  const std::string fluid = arg_value(argc, argv, "--fluid", "bgk");
  if (fluid != "bgk" && fluid != "kbc") {
    std::fprintf(stderr, "slab_ring_ade: --fluid bgk|kbc\n");
    return 2;
  }
  a.kbc = fluid == "kbc";
  a.s2 = std::atof(arg_value(argc, argv, "--s2", arg_value(argc, argv, "--omega", "1.2")).c_str());
  if (a.kbc) {  // what the step cannot do with this fluid: named here, never silently ignored
    const char* flag = !arg_value(argc, argv, "--buoyancy", "").empty() ? "--buoyancy" : a.channel ? "--channel 1"
                     : a.exchange ? "--exchange 1" : nullptr;
    if (flag) {
      std::fprintf(stderr, "slab_ring_ade: %s is not supported with --fluid kbc (the fluid + scalar step with a KBC fluid has no "
                           "buoyancy, no open boundaries and no wall exchange)\n", flag);
      return 1;
    }
  }
  try {
    double bv[6];
    a.buoyant = parse_buoyancy(arg_value(argc, argv, "--buoyancy", ""), bv);
    if (a.buoyant) a.buoy = lbm_ade_buoyancy{bv[0], bv[1], bv[2], bv[3], bv[4], bv[5]};
  } catch (const std::exception& e) {
    std::fprintf(stderr, "slab_ring_ade: %s\n", e.what());
    return 2;
  }
  return ring_main("slab_ring_ade", a, run_rank, run_emulated);
}
