// Rayleigh-Benard convection over row slabs: rayleigh_benard's box -- a fluid heated from below between two rigid plates,
// the temperature the transported scalar, buoyancy the coupling -- cut into a chain of slabs whose end slabs carry the
// plates, with the compressible BGK fluid (Guo's forcing) or the entropic KBC collision (the forced KBC collision) through
// the buoyant entries of the fluid by model: lbm_ring_ade_slab_collide_mb / lbm_ring_ade_slab_step_mb on the ring,
// lbm_ade_collide_mb / lbm_ade_slab_stream_collide_mb with emulated links under --emulate N.
//   usage: slab_ring_benard [--emulate N | --spawn N [--one-gpu 1] [--transport rccl|ipc]] [--fluid bgk|kbc]
//          [--omega X | --s2 X] [--omega-g X] [--ra X | --beta X] [--rows R per slab] [--cols C] [--steps N] [--warmup W]
//          [--edge-rows E] [--seed-mode A] [--check 1] [--compare 1]
// The box, the parameters and the initial state are rayleigh_benard's on (slabs x R) x C: bounce-back rows (row 0 the hot
// plate, the last row the cold one), periodic columns, the scalar FIXED at 1 and at 0 on them, c_ref = 0.5, w = 0, F = beta
// (C - 0.5) along +r with beta from --beta or from --ra (default 5000) as Ra nu kappa / Rg^3, rho = 1, u = 0, C = the
// conduction profile plus one mode of amplitude A; f and g are formed on the device by lbm_equilibrium, node by node -- the
// same bits for every decomposition.  The run is the collide-only first iteration, then W + N fused steps (the last N
// timed): 1 + W + N iterations, "iterations" of the JSON line -- rayleigh_benard --steps (1 + W + N) runs the same.
// Output: one JSON line.  nusselt, max_u and nonfinite are rayleigh_benard's, formed from the slabs: every slab runs one
// passive reference-order part step into scratch lattices for the moments of the streamed state (rho, u0 = calc_u(f, rho),
// C), lbm_diag_rows puts them into the slab's rows of a global row table, and lbm_diag_fold (--emulate) or
// lbm_diag_fold_host (ranks, their tables gathered through files) folds it: the bits of lbm_ade_solver_diag on one block.
// --check 1: the lattices against one block (lbm_ade_collide_mb / lbm_ade_stream_collide_mb), bit for bit, and the number
// of non-finite values of that block.  --compare 1 (--emulate): per timed step and slab also (b) the passive
// reference-order lbm_ade_stream_collide_part_m step of the same slab into scratch lattices and (c) the one-block buoyant
// step of a slab-sized lattice, alternated with the chain's own step (a): DESIGN.md section 11.  --compare 2 adds (a'), the
// buoyant step once more into the scratch lattices with the knob "kbc_part_g_fenced" set: the candidate order of the part
// kernel in a library built with EXPERIMENTS=1, the built kernel again (a control of "into scratch") in any other.
#include <cmath>

#include "ring_common.hpp"

namespace {

struct Args : RingOpts {
  bool kbc = false;
  int compare = 0;
  double rate = 1.4, omega_g = 1.4, beta = 0, seed = 1e-3;
};
const double kCRef = 0.5;

lbm_ade_fluid fluid_model(const Args& a, int form = LBM_FORM_DEFAULT) {
  lbm_ade_fluid m{};
  m.model = a.kbc ? LBM_MODEL_KBC : LBM_MODEL_BGK;
  m.bgk.omega = a.rate;
  m.bgk.form = form;
  m.kbc = lbm_kbc_params{a.rate, form};
  return m;
}
lbm_ade_params scalar_params(const Args& a, int form = LBM_FORM_DEFAULT) { return lbm_ade_params{a.omega_g, 0.0, 0.0, form}; }
// rayleigh_benard's: the velocity shift u_shift = 1 for the KBC fluid (guo is not read), Guo's scheme for BGK
lbm_ade_buoyancy buoyancy(const Args& a) {
  return a.kbc ? lbm_ade_buoyancy{a.beta, 0.0, kCRef, 1.0, 1.0 / 3.0, 1.0 / 9.0} : lbm_ade_buoyancy{a.beta, 0.0, kCRef, 0.5, 3.0, 9.0};
}
lbm_bc global_bc() { return lbm_bc{LBM_EDGE_BOUNCE_BACK, LBM_EDGE_BOUNCE_BACK, 0, 0, 0, 1.0, 1.0, 0.0, 0.0}; }
// the plates: the scalar FIXED at 1 on row_lo and at 0 on row_hi; a seam (HALO row edge) carries no FIXED row
lbm_ade_scalar_bc plates(const lbm_bc& bc) {
  lbm_ade_scalar_bc s{};
  s.mode[0] = bc.row_lo == LBM_EDGE_HALO ? LBM_ADE_SCALAR_NO_FLUX : LBM_ADE_SCALAR_FIXED;
  s.mode[1] = bc.row_hi == LBM_EDGE_HALO ? LBM_ADE_SCALAR_NO_FLUX : LBM_ADE_SCALAR_FIXED;
  s.conc[0] = 1.0;
  s.conc[1] = 0.0;
  return s;
}

// pre-collision f, g of global rows [row0, row0 + R) into lattices of geometry g (owned rows; the rest zero)
void upload_rows(const Args& a, double* f, double* h, const lbm_geom& g, int row0, int Rg) {
  const int R = g.R, C = g.C;
  const lbm_geom d{R, C, 0, 0, 0};
  const size_t n = (size_t)R * C;
  const double pi = std::acos(-1.0);
  std::vector<double> conc(n), rho(n, 1.0);
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < C; ++c)
      conc[(size_t)r * C + c] = 1.0 - (row0 + r + 0.5) / Rg + a.seed * std::sin(pi * (row0 + r + 0.5) / Rg) * std::cos(2.0 * pi * c / C);
  double *u = alloc_doubles(2 * n), *m = alloc_doubles(n), *stage = alloc_doubles(9 * n);
  for (auto [dst, src] : {std::pair<double*, std::vector<double>*>{f, &rho}, {h, &conc}}) {
    check(lbm_memset(dst, 0, plane_doubles(g) * 9 * 8, nullptr), "memset");
    check(lbm_memcpy_h2d(m, src->data(), n * 8, nullptr), "h2d");
    check(lbm_equilibrium(stage, u, m, R, C, nullptr), "lbm_equilibrium");
    check(lbm_lattice_copy_rows(dst, &g, 0, stage, &d, 0, R, nullptr), "lbm_lattice_copy_rows");
    check(lbm_stream_sync(nullptr), "sync");
  }
  for (double* p : {u, m, stage}) lbm_free(p);
}

// One block of Rg x C (ghost 0, dense), the collide-only iteration + `steps` fused steps: the yardstick of --check.
// Returns f, g of the owned rows as dense [9][Rg][C] on the host.
void one_block(const Args& a, int Rg, int steps, std::vector<double>& f_out, std::vector<double>& g_out) {
  const lbm_geom g{Rg, a.cols, 0, 0, 0};
  const lbm_bc bc = global_bc();
  const lbm_ade_scalar_bc sbc = plates(bc);
  const lbm_ade_fluid fm = fluid_model(a);
  const lbm_ade_params sc = scalar_params(a);
  const lbm_ade_buoyancy by = buoyancy(a);
  double *f[2] = {alloc_lattice(g), alloc_lattice(g)}, *h[2] = {alloc_lattice(g), alloc_lattice(g)};
  upload_rows(a, f[0], h[0], g, 0, Rg);
  check(lbm_ade_collide_mb(f[1], h[1], f[0], h[0], &g, &bc, &fm, &sc, &sbc, &by, nullptr, nullptr, nullptr, nullptr), "lbm_ade_collide_mb");
  int cur = 1;
  for (int t = 0; t < steps; ++t, cur ^= 1)
    check(lbm_ade_stream_collide_mb(f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &g, &bc, &fm, &sc, &sbc, &by, nullptr, 0, Rg, nullptr,
                                    nullptr, nullptr, nullptr), "lbm_ade_stream_collide_mb");
  f_out = owned_to_host(f[cur], g);
  g_out = owned_to_host(h[cur], g);
  for (int k = 0; k < 2; ++k) {
    lbm_free(f[k]);
    lbm_free(h[k]);
  }
}

size_t count_nonfinite(const std::vector<double>& a) {
  size_t n = 0;
  for (double x : a) n += std::isfinite(x) ? 0 : 1;
  return n;
}

// The moments of the streamed state a slab's post-collision lattices lead to (ghost rows as the last exchange left them):
// one PASSIVE part step in the reference order into scratch lattices -- rho, u0 = calc_u(f, rho), C, what
// lbm_ade_solver_diag forms -- and their row values into rows [table_row0, table_row0 + R) of a device row table
struct SlabMoments {
  lbm_geom g;
  double *f, *h, *rho, *u, *conc;
  explicit SlabMoments(const lbm_geom& g_) : g(g_), f(alloc_lattice(g_)), h(alloc_lattice(g_)) {
    const size_t n = (size_t)g.R * g.C;
    rho = alloc_doubles(n), u = alloc_doubles(2 * n), conc = alloc_doubles(n);
  }
  SlabMoments(const SlabMoments&) = delete;
  ~SlabMoments() {
    for (double* p : {f, h, rho, u, conc}) lbm_free(p);
  }
  void rows(const Args& a, const double* fo, const double* go, const lbm_bc& bc, int E, double* table, int table_rows, int table_row0) {
    const lbm_ade_fluid fm = fluid_model(a, LBM_FORM_REFERENCE_ORDER);
    const lbm_ade_params sc = scalar_params(a, LBM_FORM_REFERENCE_ORDER);
    const lbm_ade_scalar_bc sbc = plates(bc);
    for (int which : {LBM_ADE_PART_FRAME, LBM_ADE_PART_INNER})
      check(lbm_ade_stream_collide_part_m(f, h, fo, go, &g, &bc, &fm, &sc, &sbc, nullptr, which, E, rho, u, conc, nullptr),
            "lbm_ade_stream_collide_part_m");
    check(lbm_diag_rows(table, table_rows, table_row0, rho, u, conc, nullptr, g.R, g.C, 0, g.R, nullptr), "lbm_diag_rows");
  }
};

// rayleigh_benard's figures from the folded values: nusselt = 1 + <C u_r> Rg / kappa with the physical velocity u0 + F / 2
std::string benard_fields(const Args& a, const double* d, int Rg) {
  const double kappa = (1.0 / a.omega_g - 0.5) / 3.0;
  const double flux = d[LBM_DIAG_SUM_CUR] + 0.5 * a.beta * (d[LBM_DIAG_SUM_C2] - kCRef * d[LBM_DIAG_SUM_C]);
  const double nusselt = 1.0 + flux / ((double)Rg * a.cols) * Rg / kappa;
  char t[256];
  std::snprintf(t, sizeof t, ", \"nusselt\": %.17g, \"max_u\": %.17g, \"nonfinite\": %lld", std::isfinite(nusselt) ? nusselt : -1.0,
                std::isfinite(d[LBM_DIAG_MAX_U2]) ? std::sqrt(d[LBM_DIAG_MAX_U2]) : -1.0, (long long)d[LBM_DIAG_NONFINITE]);
  return t;
}
std::string common_fields(const Args& a, int Rg) {
  const lbm_ade_buoyancy by = buoyancy(a);
  char t[512];
  std::snprintf(t, sizeof t, "\"fluid\": \"%s\", \"global_rows\": %d, \"cols\": %d, \"steps\": %d, \"iterations\": %d, \"edge_rows\": %d, "
                "\"rate\": %.17g, \"omega_g\": %.17g, \"beta\": %.17g, \"u_shift\": %.17g, \"guo\": [%.17g, %.17g]",
                a.kbc ? "kbc" : "bgk", Rg, a.cols, a.steps, 1 + a.warmup + a.steps, a.edge_rows, a.rate, a.omega_g, a.beta, by.u_shift,
                by.guo_a, by.guo_b);
  return t;
}

// timed on the main stream between two events
struct Timed {
  void* ev[2];
  double ms = 0;
  Timed() {
    for (void*& e : ev) check(lbm_event_create(&e), "lbm_event_create");
  }
  Timed(const Timed&) = delete;
  ~Timed() {
    for (void* e : ev) lbm_event_destroy(e);
  }
  void begin() { check(lbm_event_record(ev[0], nullptr), "event"); }
  void end(bool timed) {
    check(lbm_event_record(ev[1], nullptr), "event");
    float m = 0;
    check(lbm_event_elapsed_ms(&m, ev[0], ev[1]), "elapsed");
    if (timed) ms += m;
  }
};

// --emulate N: every slab in turn on ONE GPU.  A slab's step is what lbm_ring_ade_slab_step_mb enqueues -- FRAME on the
// ring's stream, INNER on the main stream beside it, the pack behind FRAME -- with the messages (both lattices) as device
// copies between the steps.  The initial state is the one block's post-collision state, scattered into the slabs.
int run_emulated(const Args& a, int N) {
  check(lbm_set_device(0), "lbm_set_device");
  const int R = a.rows, C = a.cols, Rg = R * N, E = a.edge_rows;
  if (E < 1 || 2 * E >= R) throw std::runtime_error("--edge-rows must satisfy 1 <= E and 2 E < rows");
  const lbm_ade_fluid fm = fluid_model(a);
  const lbm_ade_params sc = scalar_params(a);
  const lbm_ade_buoyancy by = buoyancy(a);
  const lbm_bc gbc = global_bc();
  const lbm_geom g = padded_geom(R, C, 1);
  const size_t msg = (size_t)lbm_halo_rows(1) * C;  // per lattice
  struct Slab {
    lbm_bc bc;
    lbm_ade_scalar_bc sbc;
    double *f[2], *h[2];
  };
  std::vector<Slab> S(N);
  EmulatedLinks links(N, /*closed=*/false);  // a message: f then g
  {
    const lbm_geom gg{Rg, C, 0, 0, 0};
    const lbm_ade_scalar_bc gsbc = plates(gbc);
    double *f0 = alloc_lattice(gg), *h0 = alloc_lattice(gg), *fp = alloc_lattice(gg), *hp = alloc_lattice(gg);
    upload_rows(a, f0, h0, gg, 0, Rg);
    check(lbm_ade_collide_mb(fp, hp, f0, h0, &gg, &gbc, &fm, &sc, &gsbc, &by, nullptr, nullptr, nullptr, nullptr), "lbm_ade_collide_mb");
    for (int k = 0; k < N; ++k) {
      Slab& s = S[k];
      s.bc = gbc;
      if (links.prev(k)) s.bc.row_lo = LBM_EDGE_HALO;
      if (links.next(k)) s.bc.row_hi = LBM_EDGE_HALO;
      s.sbc = plates(s.bc);
      for (int b = 0; b < 2; ++b) {
        s.f[b] = alloc_lattice(g);
        s.h[b] = alloc_lattice(g);
        links.alloc(k, /*side=*/b, 2 * msg, 2 * msg);
      }
      for (int r = -1; r <= R; ++r) {  // owned rows and the ghost rows beside them: the exchange would bring the same bits
        const int gr = k * R + r;
        if (gr < 0 || gr >= Rg) continue;
        check(lbm_lattice_copy_rows(s.f[0], &g, r, fp, &gg, gr, 1, nullptr), "lbm_lattice_copy_rows");
        check(lbm_lattice_copy_rows(s.h[0], &g, r, hp, &gg, gr, 1, nullptr), "lbm_lattice_copy_rows");
      }
    }
    check(lbm_stream_sync(nullptr), "sync");
    for (double* p : {f0, h0, fp, hp}) lbm_free(p);
  }
  EdgeStream es;
  SlabMoments scratch(g);
  // --compare: (b) the passive reference-order part step of the same slab into the scratch lattices, packed into a buffer of
  // its own, and (c) the one-block buoyant step of a slab-sized lattice (R x C, ghost 0, periodic, padded as a context pads)
  const lbm_ade_fluid fm_ref = fluid_model(a, LBM_FORM_REFERENCE_ORDER);
  const lbm_ade_params sc_ref = scalar_params(a, LBM_FORM_REFERENCE_ORDER);
  double* spare = a.compare ? alloc_doubles(2 * msg) : nullptr;
  const lbm_geom bg = padded_geom(R, C, 0);
  double *bf[2] = {nullptr, nullptr}, *bh[2] = {nullptr, nullptr};
  if (a.compare) {
    for (int k = 0; k < 2; ++k) bf[k] = alloc_lattice(bg), bh[k] = alloc_lattice(bg);
    upload_rows(a, bf[0], bh[0], bg, 0, R);
  }
  std::vector<Timed> passive(N), again(N);
  Timed block;
  int bcur = 0;
  // FRAME on the edge stream with the pack behind it, INNER on the main stream beside them (a chain of one slab: both on main)
  auto slab_step = [&](int k, double* fn, double* hn, const double* fo, const double* ho, const lbm_ade_fluid& fl,
                       const lbm_ade_params& scl, const lbm_ade_buoyancy* b, double* send0, double* send1) {
    Slab& s = S[k];
    auto part = [&](int which, lbm_stream_t st) {
      check(lbm_ade_slab_stream_collide_mb(fn, hn, fo, ho, &g, &s.bc, &fl, &scl, &s.sbc, b, nullptr, which, E, nullptr, nullptr, nullptr,
                                           st), "lbm_ade_slab_stream_collide_mb");
    };
    if (!links.prev(k) && !links.next(k)) {
      part(LBM_ADE_PART_FRAME, nullptr);
      part(LBM_ADE_PART_INNER, nullptr);
      return;
    }
    es.fork();
    part(LBM_ADE_PART_FRAME, es.edge);
    part(LBM_ADE_PART_INNER, nullptr);
    for (int side = 0; side < 2; ++side) {
      if (!links.has(k, side)) continue;
      double* send = side ? send1 : send0;
      check(lbm_halo_pack(send, fn, &g, 1, side, es.edge), "lbm_halo_pack");
      check(lbm_halo_pack(send + msg, hn, &g, 1, side, es.edge), "lbm_halo_pack");
    }
    es.join();
  };
  int cur = 0;
  for (int i = 0; i < a.warmup + a.steps; ++i) {
    const bool timed = i >= a.warmup;
    for (int k = 0; k < N; ++k) {
      Slab& s = S[k];
      links.begin(k);
      slab_step(k, s.f[cur ^ 1], s.h[cur ^ 1], s.f[cur], s.h[cur], fm, sc, &by, links.send(k, 0), links.send(k, 1));
      links.end(k);
      if (a.compare) {  // (b): a NULL descriptor is the passive lbm_ade_stream_collide_part_m step, the same launches
        passive[k].begin();
        slab_step(k, scratch.f, scratch.h, s.f[cur], s.h[cur], fm_ref, sc_ref, nullptr, spare, spare);
        passive[k].end(timed);
      }
      if (a.compare > 1) {  // (a'): the buoyant step again into the scratch lattices, with the candidate order where the library has it
        check(lbm_set_tuning("kbc_part_g_fenced", 1), "lbm_set_tuning");
        again[k].begin();
        slab_step(k, scratch.f, scratch.h, s.f[cur], s.h[cur], fm, sc, &by, spare, spare);
        again[k].end(timed);
        check(lbm_set_tuning("kbc_part_g_fenced", -1), "lbm_set_tuning");
      }
    }
    links.deliver(2 * msg);
    for (int k = 0; k < N; ++k) {
      Slab& s = S[k];
      for (int side = 0; side < 2; ++side) {
        if (!links.has(k, side)) continue;
        check(lbm_halo_unpack(s.f[cur ^ 1], links.recv(k, side), &g, 1, side, nullptr), "lbm_halo_unpack");
        check(lbm_halo_unpack(s.h[cur ^ 1], links.recv(k, side) + msg, &g, 1, side, nullptr), "lbm_halo_unpack");
      }
      links.add_elapsed(k, timed);
    }
    if (a.compare) {  // (c)
      block.begin();
      check(lbm_ade_stream_collide_mb(bf[bcur ^ 1], bh[bcur ^ 1], bf[bcur], bh[bcur], &bg, nullptr, &fm, &sc, nullptr, &by, nullptr, 0, R,
                                      nullptr, nullptr, nullptr, nullptr), "lbm_ade_stream_collide_mb");
      block.end(timed);
      bcur ^= 1;
    }
    cur ^= 1;
  }
  check(lbm_stream_sync(es.edge), "sync");
  check(lbm_stream_sync(nullptr), "sync");
  // the diagnostics: every slab's rows of ONE global table, folded on the device
  double* table = alloc_doubles((size_t)LBM_DIAG_NQ * (Rg + 1));  // the row table, then the folded values
  for (int k = 0; k < N; ++k) scratch.rows(a, S[k].f[cur], S[k].h[cur], S[k].bc, E, table, Rg, k * R);
  check(lbm_diag_fold(table + (size_t)LBM_DIAG_NQ * Rg, table, Rg, 0, Rg, nullptr), "lbm_diag_fold");
  const std::vector<double> d = doubles_to_host(table + (size_t)LBM_DIAG_NQ * Rg, LBM_DIAG_NQ);
  lbm_free(table);
  int bad = 0;
  size_t nonfinite = 0;
  if (a.check) {
    std::vector<double> want[2];
    one_block(a, Rg, a.warmup + a.steps, want[0], want[1]);
    nonfinite = count_nonfinite(want[0]) + count_nonfinite(want[1]);
    bad += nonfinite ? 1 : 0;
    for (int k = 0; k < N; ++k)
      for (int lat = 0; lat < 2; ++lat)
        bad += mismatching_planes(want[lat], Rg, owned_to_host(lat ? S[k].h[cur] : S[k].f[cur], g), R, k * R, C);
  }
  std::printf("{\"driver\": \"slab_ring_benard\", \"mode\": \"emulated chain on one GPU\", \"slabs\": %d, \"rows_per_slab\": %d, %s, "
              "\"message_rows_per_side\": %d, \"slowest_slab_ms_per_step\": %.4f, \"per_slab_ms\": [",
              N, R, common_fields(a, Rg).c_str(), 2 * lbm_halo_rows(1), links.slowest_ms() / a.steps);
  for (int k = 0; k < N; ++k) std::printf("%s%.4f", k ? ", " : "", links.ms(k) / a.steps);
  std::printf("]");
  if (a.compare) {
    double slow_b = 0;
    std::printf(", \"passive_part_m_per_slab_ms\": [");
    for (int k = 0; k < N; ++k) {
      std::printf("%s%.4f", k ? ", " : "", passive[k].ms / a.steps);
      slow_b = std::max(slow_b, passive[k].ms / a.steps);
    }
    std::printf("], \"passive_part_m_slowest_slab_ms_per_step\": %.4f, \"one_block_slab_sized_ms_per_step\": %.4f", slow_b,
                block.ms / a.steps);
    if (a.compare > 1) {
      double slow = 0;
      for (int k = 0; k < N; ++k) slow = std::max(slow, again[k].ms / a.steps);
      std::printf(", \"again_into_scratch_slowest_slab_ms_per_step\": %.4f", slow);
    }
  }
  std::printf("%s%s%s}\n", benard_fields(a, d.data(), Rg).c_str(),
              a.check ? (", \"one_block_nonfinite\": " + std::to_string(nonfinite)).c_str() : "", check_field(a.check, bad));
  std::fflush(stdout);
  for (auto& s : S)
    for (int b = 0; b < 2; ++b) {
      lbm_free(s.f[b]);
      lbm_free(s.h[b]);
    }
  for (int k = 0; k < 2; ++k) {
    lbm_free(bf[k]);
    lbm_free(bh[k]);
  }
  lbm_free(spare);
  return bad ? 3 : (d[LBM_DIAG_NONFINITE] != 0.0 ? 4 : 0);
}

int run_rank(const Args& a, int rank, int world, int local_rank) {
  check(lbm_set_device(ring_device(local_rank)), "lbm_set_device");
  const int R = a.rows, C = a.cols, Rg = R * world;
  const lbm_ade_fluid fm = fluid_model(a);
  const lbm_ade_params sc = scalar_params(a);
  const lbm_ade_buoyancy by = buoyancy(a);
  const lbm_bc gbc = global_bc();
  const lbm_ade_scalar_bc gsbc = plates(gbc);  // the global descriptor: the ring drops a FIXED row at a seam
  const lbm_geom g = padded_geom(R, C, 1);
  unsigned char id[128];
  share_unique_id(id, rank, world, a.id_file);
  lbm_ring* ring = nullptr;
  check(lbm_ring_create(&ring, id, rank, world, &g, /*periodic=*/0), "lbm_ring_create");
  double *f[2] = {alloc_lattice(g), alloc_lattice(g)}, *h[2] = {alloc_lattice(g), alloc_lattice(g)};
  upload_rows(a, f[1], h[1], g, rank * R, Rg);  // pre-collision, then the first driver iteration: collide + one exchange
  check(lbm_ring_ade_slab_collide_mb(ring, f[0], h[0], f[1], h[1], &gbc, &fm, &sc, &gsbc, &by, nullptr), "lbm_ring_ade_slab_collide_mb");
  int cur = 0;
  auto step = [&]() {
    check(lbm_ring_ade_slab_step_mb(ring, f[cur ^ 1], h[cur ^ 1], f[cur], h[cur], &gbc, &fm, &sc, &gsbc, &by, nullptr, a.edge_rows,
                                    nullptr), "lbm_ring_ade_slab_step_mb");
    cur ^= 1;
  };
  double tmax = 0;
  if (const int failed = timed_ring_run(ring, "slab_ring_benard", a, rank, world, a.warmup, a.steps, step, &tmax)) return failed;
  // the diagnostics: this slab's row table, gathered on rank 0 through files and folded on the host
  {
    lbm_bc bc = gbc;
    if (rank > 0) bc.row_lo = LBM_EDGE_HALO;
    if (rank < world - 1) bc.row_hi = LBM_EDGE_HALO;
    SlabMoments scratch(g);
    double* table = alloc_doubles((size_t)LBM_DIAG_NQ * R);
    scratch.rows(a, f[cur], h[cur], bc, a.edge_rows, table, R, 0);
    const std::vector<double> rows = doubles_to_host(table, (size_t)LBM_DIAG_NQ * R);
    lbm_free(table);
    write_file_atomic(a.id_file + ".d" + std::to_string(rank), rows.data(), rows.size() * 8);
  }
  std::vector<double> d(LBM_DIAG_NQ, 0.0);
  if (rank == 0) {
    std::vector<double> global((size_t)LBM_DIAG_NQ * Rg), rows((size_t)LBM_DIAG_NQ * R);
    for (int r = 0; r < world; ++r) {
      const std::string path = a.id_file + ".d" + std::to_string(r);
      wait_file(path, rows.data(), rows.size() * 8);
      std::remove(path.c_str());
      for (int q = 0; q < LBM_DIAG_NQ; ++q)
        std::copy(rows.begin() + (size_t)q * R, rows.begin() + (size_t)(q + 1) * R, global.begin() + (size_t)q * Rg + (size_t)r * R);
    }
    check(lbm_diag_fold_host(d.data(), global.data(), Rg, 0, Rg), "lbm_diag_fold_host");
  }
  int bad = 0;
  size_t nonfinite = 0;
  if (a.check) {
    publish_owned_rows(a, ".f", rank, f[cur], g);
    publish_owned_rows(a, ".g", rank, h[cur], g);
    if (rank == 0) {
      std::vector<double> want[2];
      one_block(a, Rg, a.warmup + a.steps, want[0], want[1]);
      nonfinite = count_nonfinite(want[0]) + count_nonfinite(want[1]);
      bad += nonfinite ? 1 : 0;
      for (int r = 0; r < world; ++r)
        for (int lat = 0; lat < 2; ++lat)
          bad += mismatching_planes(want[lat], Rg, read_owned_rows(a, lat ? ".g" : ".f", r, R, C), R, r * R, C);
    }
  }
  if (rank == 0) {
    const double ms = 1e3 * tmax / a.steps;
    std::printf("{\"driver\": \"slab_ring_benard\", \"n_gpus\": %d, \"rows_per_gpu\": %d, %s, \"message_rows_per_side\": %d, "
                "\"slowest_slab_ms_per_step\": %.4f, \"mlups\": %.1f%s%s%s}\n",
                world, R, common_fields(a, Rg).c_str(), 2 * lbm_halo_rows(1), ms, (double)Rg * C / (ms * 1e3),
                benard_fields(a, d.data(), Rg).c_str(),
                a.check ? (", \"one_block_nonfinite\": " + std::to_string(nonfinite)).c_str() : "", check_field(a.check, bad));
    std::fflush(stdout);
  }
  lbm_ring_destroy(ring);
  for (int k = 0; k < 2; ++k) {
    lbm_free(f[k]);
    lbm_free(h[k]);
  }
  return bad ? 3 : (d[LBM_DIAG_NONFINITE] != 0.0 ? 4 : 0);
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  parse_ring_opts(a, argc, argv, /*rows=*/24, /*cols=*/48, /*steps=*/50, /*warmup=*/5, /*edge_rows=*/16);
  a.steps = std::max(1, a.steps);
  a.warmup = std::max(0, a.warmup);
  // the default edge band on a slab too low for it: the widest that leaves an INNER row (an --edge-rows given is taken as it is)
  if (arg_value(argc, argv, "--edge-rows", "").empty()) a.edge_rows = std::max(1, std::min(a.edge_rows, (a.rows - 1) / 2));
  const std::string fluid = arg_value(argc, argv, "--fluid", "bgk");
  if (fluid != "bgk" && fluid != "kbc") {
    std::fprintf(stderr, "slab_ring_benard: --fluid bgk|kbc\n");
    return 2;
  }
  a.kbc = fluid == "kbc";
  a.compare = int_arg(argc, argv, "--compare", 0);
  if (a.compare && a.emulate <= 0) {
    std::fprintf(stderr, "slab_ring_benard: --compare 1 needs --emulate N (the candidates alternate on one device)\n");
    return 1;
  }
  try {
    a.rate = std::stod(arg_value(argc, argv, a.kbc ? "--s2" : "--omega", "1.4"));
    a.omega_g = std::stod(arg_value(argc, argv, "--omega-g", std::to_string(a.rate)));
    a.seed = std::stod(arg_value(argc, argv, "--seed-mode", "1e-3"));
    const int slabs = a.emulate > 0 ? a.emulate : a.spawn > 0 ? a.spawn : std::max(1, std::atoi(std::getenv("WORLD_SIZE") ? std::getenv("WORLD_SIZE") : "1"));
    const double Rg = (double)a.rows * slabs;
    const double nu = (1.0 / a.rate - 0.5) / 3.0, kappa = (1.0 / a.omega_g - 0.5) / 3.0;
    const std::string beta_arg = arg_value(argc, argv, "--beta", "");
    const double Ra = std::stod(arg_value(argc, argv, "--ra", "5000"));
    a.beta = beta_arg.empty() ? Ra * nu * kappa / (Rg * Rg * Rg) : std::stod(beta_arg);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "slab_ring_benard: %s\n", e.what());
    return 2;
  }
  if (a.rows < 3 || a.cols < 2) {
    std::fprintf(stderr, "slab_ring_benard: --rows must be at least 3 and --cols at least 2\n");
    return 1;
  }
  return ring_main("slab_ring_benard", a, run_rank, run_emulated);
}
