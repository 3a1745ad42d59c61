// C ABI, fluid + transported scalar: the compressible BGK fluid f and the advection-diffusion scalar g of
// test/rectangle_sedimentation_test.cpp:88-247 in one fused pull step per node (ade.hpp), and the solver
// context that runs the driver loop on one block.  Every host check of the step is here, for either fluid (ade_resolve:
// the fluid is an AdeFluid, a BGK parameter block or a KBC one), and every entry point, the `_m` / `_mb` ones included; a
// resolved call is launched by its fluid (ade_step_from, ade_part_from, ade_collide_from) -- the BGK fluid's kernels from
// here, the KBC fluid's from the capi_ade_kbc*.hip units (its open pass and wall exchange: capi_ade_kbc_open.hip), all through
// the one launch path of ade_launch.hpp.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <iterator>
#include <map>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#include "ade_launch.hpp"
#include "ade_plain.hpp"

// Interior walls of the fused step: a host table of wall nodes, merged per node and kept sorted by (r, c) while it is
// built; lbm_ade_iwalls_finalize uploads it once (the only device call) and it is immutable from then on.  first: the
// index of the first node of each row (R + 1 entries, first[R] = n), kept on the host by finalize -- a part of a slab
// finds the node ranges of its rows there, with no allocation and no host synchronisation in the step path -- and uploaded
// beside the nodes (d_first) for the wall exchange, whose waves find their rows on the device.
struct lbm_ade_iwalls {
  struct Entry {
    unsigned f = 0, g = 0, g_fixed = 0;  // slot masks, bit s-1 = slot s; g_fixed: the g slots that are FIXED
    double conc = 0.0;                   // C_w of the FIXED slots
    bool has_conc = false;               // some FIXED segment has named the node
  };
  int R = 0, C = 0;
  std::map<std::pair<int, int>, Entry> nodes;
  bool finalized = false;
  int n = 0;                              // nodes uploaded
  lbm::AdeIwallNode* d_nodes = nullptr;   // device copy, sorted by (r, c)
  int* d_first = nullptr;                 // device copy of first
  std::vector<int> first;                 // finalized: first[r] = index of the first node of rows >= r
};

// Open boundaries of the fused step: the segments in the order added, and the table resolved from them after every add
// (resolve below) -- the listed nodes sorted by (r, c), each with the segment that won every slot, its nine g sources
// (gsrc: (row + 1) C + column, lbm::ade_open_at) and its extrapolation neighbours.  lbm_ade_open_finalize uploads nodes
// and segments once and keeps the row index first (R + 1 entries, as lbm_ade_iwalls.first); immutable from then on.
struct lbm_ade_open {
  enum Kind { F_RULE, G_RULE, G_COPY };
  struct Seg {
    Kind kind;
    int r0, c0, dr, dc, n;
    unsigned slots;
    int rule;       // F_RULE: LBM_ADE_OPEN_*; G_RULE: LBM_ADE_SCALAR_*
    double p0, p1;  // AdeOpenSeg's
    int nr, nc;     // ABB_EXTRAPOLATED: the inward neighbour; G_COPY: the source offset
  };
  int R = 0, C = 0;
  std::vector<Seg> segs;
  std::vector<lbm::AdeOpenNode> nodes;  // resolved
  bool finalized = false;
  int n = 0;  // nodes uploaded
  lbm::AdeOpenNode* d_nodes = nullptr;
  lbm::AdeOpenSeg* d_segs = nullptr;
  std::vector<int> first;
  // A slab VIEW (lbm_ade_open_slab): the parent's nodes of rows [row0, row0 + R) at r - row0 and its segments; the rows of
  // gsrc lie in [-1, R] (an ordinary table's in [0, R)), pad the mask of the g sources the slab cannot reach (bit q), xn
  // indices into the view.
  bool view = false;
  int row0 = 0, R_parent = 0;
  // the call configuration (edge modes, ghost rows, FIXED edges) the reach check has last passed with, + 1: a step loop
  // checks the view's sources once, not once per call
  mutable std::atomic<unsigned> reach_ok{0};
};

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

// The BGK fluid's own parameters: where ade_validate asks, between the edges and the scalar's parameters
static int ade_bgk_fluid_check(const char* fn, const lbm_bgk_params* fluid) {
  LBM_REQUIRE(fluid, "%s: NULL fluid params", fn);
  LBM_REQUIRE(fluid->omega > 0.0 && fluid->omega < 2.0, "%s: omega=%g outside (0, 2)", fn, fluid->omega);
  LBM_REQUIRE(fluid->incompressible == 0, "%s: incompressible=%d: the fluid is the compressible BGK model", fn,
              fluid->incompressible);
  LBM_REQUIRE(fluid->force_mode == 0, "%s: force_mode=%d: no body force in the fluid + scalar step", fn,
              fluid->force_mode);
  LBM_REQUIRE(fluid->delta_form == 0, "%s: delta_form=%d not supported by the fluid + scalar step", fn, fluid->delta_form);
  LBM_REQUIRE(fluid->form >= LBM_FORM_DEFAULT && fluid->form <= LBM_FORM_REASSOCIATED, "%s: fluid form=%d (LBM_FORM_*)",
              fn, fluid->form);
  return LBM_OK;
}

// The KBC fluid's own parameters, as lbm_kbc_* checks them, and what the step cannot do with this fluid: the first checks
// of a call with a KBC fluid, before ade_resolve looks at anything else
static int ade_kbc_fluid_check(const char* fn, const lbm_kbc_params* kbc, const lbm_bc* bc) {
  LBM_REQUIRE(kbc->s2 > 0.0 && kbc->s2 <= 2.0, "%s: KBC fluid: s2=%g outside (0, 2]", fn, kbc->s2);
  LBM_REQUIRE(kbc->form >= LBM_FORM_DEFAULT && kbc->form <= LBM_FORM_REASSOCIATED, "%s: KBC fluid: form=%d (LBM_FORM_*)", fn,
              kbc->form);
  LBM_REQUIRE(!(bc && bc->pressure_rows), "%s: pressure rows (pressure_rows=%d) are not supported by the fluid + scalar "
              "step with a KBC fluid", fn, bc ? bc->pressure_rows : 0);
  return LBM_OK;
}

// Everything the fused step accepts but the KBC fluid's own parameters (ade_kbc_fluid_check, before this), checked on the
// host before any device call.  Single block (slab = false): ghost
// 0, rows PERIODIC or BOUNCE_BACK.  Slab (the part launches and the ring): ghost 0 with PERIODIC or BOUNCE_BACK rows, or
// ghost >= 1 with HALO or BOUNCE_BACK rows -- ghost rows are read where a row edge is HALO and nothing wraps.  Columns:
// PERIODIC, BOUNCE_BACK or SPECULAR.  The scalar takes the fluid's fix-up at every wall.
static int ade_validate(const char* fn, const lbm_geom* g, const lbm_bc* bc, const AdeFluid& fluid,
                        const lbm_ade_params* scalar, bool slab) {
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
  if (!fluid.kbc)
    if (int rc = ade_bgk_fluid_check(fn, fluid.bgk)) return rc;
  LBM_REQUIRE(scalar, "%s: NULL scalar params", fn);
  LBM_REQUIRE(scalar->omega_g > 0.0 && scalar->omega_g < 2.0, "%s: omega_g=%g outside (0, 2)", fn, scalar->omega_g);
  LBM_REQUIRE(scalar->form >= LBM_FORM_DEFAULT && scalar->form <= LBM_FORM_REASSOCIATED,
              "%s: scalar form=%d (LBM_FORM_*)", fn, scalar->form);
  LBM_REQUIRE(fluid.kbc || fluid.bgk->form == LBM_FORM_DEFAULT || fluid.bgk->form == scalar->form,
              "%s: fluid form=%d differs from the scalar form=%d (lbm_ade_params.form sets both halves)", fn, fluid.bgk->form,
              scalar->form);
  return LBM_OK;
}

// one form for both halves, lbm_ade_params.form; LBM_FORM_DEFAULT resolves through "bgk_fast", as for BGK
static bool ade_fast(const lbm_ade_params* scalar) {
  return scalar->form == LBM_FORM_DEFAULT ? tuning("bgk_fast", 1) != 0 : scalar->form == LBM_FORM_REASSOCIATED;
}

// The buoyancy (lbm_ade_buoyancy, NULL allowed) on the host: every field finite.  *by receives the device copy and
// *buoyant whether the step is a buoyant one -- beta = (0, 0), like NULL, is the passive step (both or neither given).
int ade_buoyancy_check(const char* fn, const lbm_ade_buoyancy* b, AdeBuoyancy* by, bool* buoyant) {
  AdeBuoyancy unused_by;
  bool unused_flag;
  if (!by) by = &unused_by, buoyant = &unused_flag;
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
// wall of the fluid there -- a BOUNCE_BACK row, a BOUNCE_BACK or SPECULAR column.  *sw (if given) receives the device copy.
int ade_scalar_bc_check(const char* fn, const lbm_ade_scalar_bc* sbc, const lbm_bc* bc, AdeWalls* sw) {
  AdeWalls unused;
  if (!sw) sw = &unused;
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

// The interior walls (lbm_ade_iwalls, NULL allowed) against the geometry of the call, on the host: finalized, and built
// for the same R x C.  *nodes / *n receive the device table and *first (if wanted) the host's row index; an empty table
// is NULL's (nullptr, 0, nullptr).
static int ade_iwalls_check(const char* fn, const lbm_ade_iwalls* t, const lbm_geom* g, const AdeIwallNode** nodes, int* n,
                            const int** first = nullptr) {
  *nodes = nullptr;
  *n = 0;
  if (first) *first = nullptr;
  if (!t) return LBM_OK;
  LBM_REQUIRE(t->finalized, "%s: interior walls: the table is not finalized (lbm_ade_iwalls_finalize)", fn);
  LBM_REQUIRE(g && t->R == g->R && t->C == g->C, "%s: interior walls: the table is for a %d x %d lattice, the call for %d x %d",
              fn, t->R, t->C, g ? g->R : 0, g ? g->C : 0);
  *nodes = t->d_nodes;
  *n = t->n;
  if (first && t->n > 0) *first = t->first.data();
  return LBM_OK;
}

// The table resolved from the segments added so far (lbm_ade_open.nodes), on the host: the scalar's source map from the
// copy segments (each sets map[dst] = map[src] for all its nodes at once, in the order added), the segment that won every
// slot, and the listed nodes -- exactly the union of (a) the nodes with a rule, (b) the nine nodes that pull from a node
// whose map entry is not itself, under periodic wrap in both axes, (c) the inward neighbour of a node with an extrapolated
// slot -- sorted by (r, c), each with its nine g sources and the table index of its extrapolation neighbours.
static void ade_open_resolve(lbm_ade_open* t) {
  const int R = t->R, C = t->C;
  auto dense = [C](int r, int c) { return (long long)r * C + c; };
  std::map<long long, long long> map;  // entries a copy has set; every other node maps to itself
  auto look = [&map](long long n) {
    const auto it = map.find(n);
    return it == map.end() ? n : it->second;
  };
  struct Slots {
    unsigned char f[8] = {}, g[8] = {};
  };
  std::map<long long, Slots> listed;  // dense order = (r, c) order
  for (size_t j = 0; j < t->segs.size(); ++j) {
    const lbm_ade_open::Seg& s = t->segs[j];
    if (s.kind == lbm_ade_open::G_COPY) {
      std::vector<long long> src((size_t)s.n);
      for (int k = 0; k < s.n; ++k) src[k] = look(dense(s.r0 + k * s.dr + s.nr, s.c0 + k * s.dc + s.nc));
      for (int k = 0; k < s.n; ++k) map[dense(s.r0 + k * s.dr, s.c0 + k * s.dc)] = src[k];
      continue;
    }
    for (int k = 0; k < s.n; ++k) {
      Slots& e = listed[dense(s.r0 + k * s.dr, s.c0 + k * s.dc)];
      for (int q = 1; q < Q; ++q)
        if ((s.slots >> (q - 1)) & 1u) (s.kind == lbm_ade_open::F_RULE ? e.f : e.g)[q - 1] = (unsigned char)(j + 1);
    }
  }
  auto extrapolated = [t](const Slots& e, int q) {
    return e.f[q - 1] && t->segs[e.f[q - 1] - 1].rule == LBM_ADE_OPEN_ABB_EXTRAPOLATED;
  };
  std::vector<long long> more;
  for (const auto& kv : map) {
    if (kv.second == kv.first) continue;
    const int r = (int)(kv.first / C), c = (int)(kv.first % C);
    for (int q = 0; q < Q; ++q) more.push_back(dense((r + icx(q) + R) % R, (c + icy(q) + C) % C));
  }
  for (const auto& kv : listed)
    for (int q = 1; q < Q; ++q)
      if (extrapolated(kv.second, q)) {
        const lbm_ade_open::Seg& s = t->segs[kv.second.f[q - 1] - 1];
        more.push_back(kv.first + dense(s.nr, s.nc));
      }
  for (long long n : more) listed[n];
  std::map<long long, int> index;
  for (const auto& kv : listed) index.emplace_hint(index.end(), kv.first, (int)index.size());
  t->nodes.clear();
  t->nodes.reserve(listed.size());
  for (const auto& kv : listed) {
    AdeOpenNode nd{};
    nd.r = (int)(kv.first / C), nd.c = (int)(kv.first % C);
    for (int q = 1; q < Q; ++q) {
      nd.fseg[(q - 1) >> 2] |= (unsigned)kv.second.f[q - 1] << (8 * ((q - 1) & 3));
      nd.gseg[(q - 1) >> 2] |= (unsigned)kv.second.g[q - 1] << (8 * ((q - 1) & 3));
      if (extrapolated(kv.second, q)) {
        const lbm_ade_open::Seg& s = t->segs[kv.second.f[q - 1] - 1];
        nd.xn[q - 1] = index[kv.first + dense(s.nr, s.nc)];
      }
    }
    for (int q = 0; q < Q; ++q) nd.gsrc[q] = (int)(look(dense((nd.r - icx(q) + R) % R, (nd.c - icy(q) + C) % C)) + C);
    t->nodes.push_back(nd);
  }
}

// slot q of g at node (r, c) is one the domain's wall gather replaces (bc_fixups_own under the scalar's gather modes)
static bool ade_wall_replaces(const Bc& gbc, int R, int C, int r, int c, int q) {
  if (r == 0 && gbc.row_lo == LBM_EDGE_BOUNCE_BACK && icx(q) == 1) return true;
  if (r == R - 1 && gbc.row_hi == LBM_EDGE_BOUNCE_BACK && icx(q) == -1) return true;
  if (c == C - 1 && bc_is_wall(gbc.col_hi) && icy(q) == -1) return true;
  return c == 0 && bc_is_wall(gbc.col_lo) && icy(q) == 1;
}

// What a slab may reach, per call (only the call knows the slab's edges): the g source of slot q of a listed node of a
// view is USABLE if it lies in an owned row, or in the ghost row of a side whose row edge is HALO (ghost = 0: in the
// wrapped row of a PERIODIC side) -- and is not marked unreachable.  Every slot needs a usable source or must be one the
// domain's wall gather replaces at the node (gbc: the scalar's gather modes); the node's own source gsrc[0] must be usable.
static int ade_open_reach(const char* fn, const lbm_ade_open* t, const lbm_geom* g, const Bc& bc, const Bc& gbc, int fixed) {
  const unsigned key = 1u + ((unsigned)bc.row_lo | (unsigned)bc.row_hi << 3 | (unsigned)bc.col_lo << 6 | (unsigned)bc.col_hi << 9 |
                             (unsigned)(g->ghost > 0) << 12 | (unsigned)fixed << 13);
  if (t->reach_ok.load(std::memory_order_relaxed) == key) return LBM_OK;
  const int R = t->R, C = t->C;
  const bool lo_ok = g->ghost > 0 ? bc.row_lo == LBM_EDGE_HALO : bc.row_lo == LBM_EDGE_PERIODIC;
  const bool hi_ok = g->ghost > 0 ? bc.row_hi == LBM_EDGE_HALO : bc.row_hi == LBM_EDGE_PERIODIC;
  for (const AdeOpenNode& nd : t->nodes)
    for (int q = 0; q < Q; ++q) {
      const int sr = nd.gsrc[q] / C - 1, sc = nd.gsrc[q] % C;
      const bool unreachable = (nd.pad >> q) & 1;
      if (!unreachable && ((sr >= 0 && sr < R) || (sr == -1 && lo_ok) || (sr == R && hi_ok))) continue;
      if (q > 0 && ade_wall_replaces(gbc, R, C, nd.r, nd.c, q)) continue;
      LBM_REQUIRE(!unreachable, "%s: open boundaries: node (%d, %d), g slot %d: its source lies more than one row outside "
                  "the slab's rows (unreachable) and no domain wall replaces the slot there", fn, nd.r, nd.c, q);
      LBM_REQUIRE(false, "%s: open boundaries: node (%d, %d), g slot %d: its source (%d, %d) lies in the ghost row of %s, "
                  "whose edge mode is %s (%s holds the neighbour's rows) and no domain wall replaces the slot there", fn, nd.r,
                  nd.c, q, sr, sc, sr < 0 ? "row_lo" : "row_hi", edge_name(sr < 0 ? bc.row_lo : bc.row_hi),
                  g->ghost > 0 ? "only a HALO side" : "with ghost = 0 only a PERIODIC side");
    }
  t->reach_ok.store(key, std::memory_order_relaxed);
  return LBM_OK;
}

// The open table (NULL allowed) against the call, on the host: finalized, built for the same R x C, and sharing no node
// with the interior walls of the call -- but for a node the open table gives no rule and whose redirected g slots are all
// slots a domain wall replaces there (gbc: the scalar's gather modes), which the interior-wall pass recomputes to the
// same populations on its own.  An empty table is NULL's.
static int ade_open_check(const char* fn, const lbm_ade_open* t, const lbm_geom* g, const Bc& gbc,
                          const lbm_ade_iwalls* iwalls, const AdeOpenNode** nodes, const AdeOpenSeg** segs, int* n,
                          bool slab = false, const Bc* bc = nullptr, int fixed = 0) {
  // the two kinds of table do not mix (before anything else: a wrong kind is named whatever state the table is in)
  LBM_REQUIRE(slab || !t->view, "%s: open boundaries: the table is a slab view (lbm_ade_open_slab): "
              "lbm_ade_stream_collide_part_o, lbm_ring_ade_collide_o and lbm_ring_ade_step_o take it", fn);
  LBM_REQUIRE(!slab || t->view, "%s: open boundaries: the table is not a slab view: a slab takes lbm_ade_open_slab of the "
              "global table (lbm_ade_collide_o and lbm_ade_stream_collide_o take an ordinary table)", fn);
  LBM_REQUIRE(t->finalized, "%s: open boundaries: the table is not finalized (lbm_ade_open_finalize)", fn);
  LBM_REQUIRE(g && t->R == g->R && t->C == g->C, "%s: open boundaries: the table is for a %d x %d lattice, the call for %d x %d",
              fn, t->R, t->C, g ? g->R : 0, g ? g->C : 0);
  if (t->n == 0) return LBM_OK;
  if (t->view)
    if (int rc = ade_open_reach(fn, t, g, *bc, gbc, fixed)) return rc;
  if (iwalls) {
    const int R = t->R, C = t->C;
    for (const auto& kv : iwalls->nodes) {
      const int r = kv.first.first, c = kv.first.second;
      const auto it = std::lower_bound(t->nodes.begin(), t->nodes.end(), kv.first, [](const AdeOpenNode& a, const std::pair<int, int>& b) {
        return std::make_pair(a.r, a.c) < b;
      });
      if (it == t->nodes.end() || it->r != r || it->c != c) continue;
      LBM_REQUIRE(!(it->fseg[0] | it->fseg[1] | it->gseg[0] | it->gseg[1]),
                  "%s: open boundaries: node (%d, %d) carries an open-boundary rule and is in the interior-wall table as well",
                  fn, r, c);
      for (int q = 0; q < Q; ++q) {
        // the plain pull source in the table's encoding (a view holds the row unwrapped, in [-1, R])
        const int pull = t->view ? r - icx(q) : (r - icx(q) + R) % R;
        const long long plain = (long long)(pull + 1) * C + (c - icy(q) + C) % C;
        LBM_REQUIRE((it->gsrc[q] == plain && !((it->pad >> q) & 1)) || ade_wall_replaces(gbc, R, C, r, c, q),
                    "%s: open boundaries: node (%d, %d) is in the interior-wall table and its g slot %d is redirected by a "
                    "copy with no domain wall replacing it there", fn, r, c, q);
      }
    }
  }
  *nodes = t->d_nodes;
  *segs = t->d_segs;
  *n = t->n;
  return LBM_OK;
}

// the fluid of an `_m` entry: given, its model BGK or KBC; *out: the parameter block of that model
int ade_fluid_model(const char* fn, const lbm_ade_fluid* fluid, AdeFluid* out) {
  LBM_REQUIRE(fluid, "%s: NULL fluid (lbm_ade_fluid)", fn);
  LBM_REQUIRE(fluid->model == LBM_MODEL_BGK || fluid->model == LBM_MODEL_KBC,
              "%s: fluid model=%d (LBM_MODEL_BGK or LBM_MODEL_KBC)", fn, fluid->model);
  *out = fluid->model == LBM_MODEL_KBC ? AdeFluid{nullptr, &fluid->kbc} : AdeFluid{&fluid->bgk, nullptr};
  return LBM_OK;
}

// The host checks of a call with either fluid, once, under the caller's name: a KBC fluid's own parameters; the scalar's
// walls (a FIXED edge names the edge mode it cannot sit on), geometry and parameters -- a BGK fluid's among them --
// buoyancy, interior walls; a KBC fluid's form against the scalar's; the open table.  An entry checks its lattices and range
// or part after.  The order is observable (a call with two faults reports the first) and differs per fluid.
int ade_resolve(const char* fn, const lbm_geom* lg, const lbm_bc* lbc, const AdeFluid& fluid, const lbm_ade_params* scalar,
                const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls, bool slab,
                AdeCall* call, const lbm_ade_open* open) {
  const lbm_kbc_params* kbc = fluid.kbc;
  int rc = kbc ? ade_kbc_fluid_check(fn, kbc, lbc) : LBM_OK;
  if (!rc) rc = ade_scalar_bc_check(fn, sbc, lbc, &call->sw);
  if (!rc) rc = ade_validate(fn, lg, lbc, fluid, scalar, slab);
  if (!rc) rc = ade_buoyancy_check(fn, buoy, &call->by, &call->buoyant);
  if (!rc) rc = ade_iwalls_check(fn, iwalls, lg, &call->wall_nodes, &call->n_wall_nodes, &call->wall_first);
  if (rc) return rc;
  if (kbc) {
    LBM_REQUIRE(kbc->form == LBM_FORM_DEFAULT || kbc->form == scalar->form,
                "%s: KBC fluid form=%d differs from the scalar form=%d (lbm_ade_params.form sets both halves)", fn, kbc->form,
                scalar->form);
  }
  call->g = make_geom(*lg);
  call->bc = make_bc(lbc);
  call->fluid = fluid.bgk;
  call->kbc = kbc;
  call->scalar = scalar;
  call->open_nodes = nullptr;
  call->open_segs = nullptr;
  call->n_open_nodes = 0;
  call->open_first = nullptr;
  call->carry_in = nullptr;
  call->carry_out = nullptr;
  if (!open) return LBM_OK;
  rc = ade_open_check(fn, open, lg, ade_scalar_gather_bc(call->bc, call->sw.fixed), call->n_wall_nodes > 0 ? iwalls : nullptr,
                      &call->open_nodes, &call->open_segs, &call->n_open_nodes, slab, &call->bc, call->sw.fixed);
  if (rc) return rc;
  // a slab's view with a KBC fluid has no launch (the open pass of this fluid runs on one block: capi_ade_kbc_open.hip).  No
  // public call reaches this: the `_m` / `_mb` part and ring entries have no parameter for a view, and the `_o` part and
  // ring entries take BGK parameters only
  LBM_REQUIRE(!(kbc && slab && call->n_open_nodes > 0), "%s: open boundaries over row slabs (a view of %d nodes) are not "
              "supported with a KBC fluid", fn, call->n_open_nodes);
  if (call->n_open_nodes > 0) call->open_first = open->first.data();
  return LBM_OK;
}

// The open-table pass of the rows `r` (ade_row_ranges), behind the dispatch whose nodes it overwrites and on the same
// stream: one lane per listed node; rows without one enqueue nothing.  The one launch site of k_ade_open_ranges, which
// exists with the BGK fluid alone (a KBC fluid's: k_ade_kbc_open_ranges, capi_ade_kbc_open.hip).  *launches += the kernels enqueued
template <bool B, class FM, class SM>
static int ade_open_pass(const AdeCall& k, const FM& fm, const SM& sm, double* fn, double* gn, const double* fo,
                         const double* go, const AdeRows& r, double* rho, double* u, double* conc, hipStream_t st,
                         long long* launches) {
  if (k.n_open_nodes == 0) return LBM_OK;
  const AdeRanges a = ade_row_ranges(k.open_first, r.band0, r.n0, r.band1, r.nrows);
  if (a.w == 0) return LBM_OK;
  with_flags([&](auto M, auto F) {
    LBM_KLAUNCH((k_ade_open_ranges<FM, SM, M(), F(), B>), dim3((a.w + 255) / 256), dim3(256), 0, st, fn, gn, fo, go, k.g,
                k.bc, fm, sm, rho, u, conc, k.sw, k.by, k.open_nodes, k.open_segs, a.first0, a.w0, a.first1, a.w,
                k.carry_in, k.carry_out);
  }, rho != nullptr, k.sw.fixed);
  LBM_CHECK_LAUNCH();
  ++*launches;
  return LBM_OK;
}

// the two table passes of a launch with the BGK fluid: the open table's listed nodes of the rows, then the interior walls'
template <bool B, class FM, class SM>
static int ade_table_passes(const AdeCall& k, const FM& fm, const SM& sm, double* fn, double* gn, const double* fo,
                            const double* go, const AdeRows& r, double* rho, double* u, double* conc, hipStream_t st,
                            long long* launches) {
  if (int rc = ade_open_pass<B>(k, fm, sm, fn, gn, fo, go, r, rho, u, conc, st, launches)) return rc;
  return ade_iwalls_pass<B>(k, fm, sm, fn, gn, fo, go, r, rho, u, conc, st, launches);
}

// kernels the part launches of this process have enqueued (lbm_ade_part_launches): what "a NULL view adds no launch" is
// tested with, there being no solver context for slabs to count them
static std::atomic<long long> g_part_launches{0};
void ade_part_launches_add(long long n) { g_part_launches.fetch_add(n, std::memory_order_relaxed); }

// The launches of a resolved call, by its fluid: BGK here, KBC in capi_ade_kbc.hip (a part: capi_ade_kbc_part.hip), KBC with
// call.buoyant in capi_ade_kbc_buoyant.hip (a part: capi_ade_kbc_buoyant_part.hip).
// collide only: no streaming, so no wall rule -- the scalar's walls and the interior walls of the call are checked and
// nothing more
int ade_collide_from(const char* fn, const AdeCall& k, double* fp, double* gp, const double* f, const double* h,
                     double* rho, double* u, double* conc, hipStream_t st) {
  if (int rc = ade_lattice_args(fn, fp, gp, f, h, rho, u, conc, false)) return rc;
  if (k.kbc && k.buoyant) return ade_kbc_buoyant_collide_from(k, fp, gp, f, h, rho, u, conc, st);
  if (k.kbc) return ade_kbc_collide_from(k, fp, gp, f, h, rho, u, conc, st);
  return with_ade_models(k.fluid, k.scalar, k.buoyant, [&](const auto& fm, const auto& sm, auto B) {
    return ade_collide_launch<B()>(k, fm, sm, fp, gp, f, h, rho, u, conc, st);
  });
}

// the step on rows [row_begin, row_end) of a single block; *launches (if given) += the kernels enqueued
static int ade_step_from(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, int row_begin,
                         int row_end, double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  long long uncounted = 0;
  if (!launches) launches = &uncounted;
  if (k.kbc && k.buoyant) return ade_kbc_buoyant_step(k, fn, gn, fo, go, row_begin, row_end, rho, u, conc, st, launches);
  if (k.kbc) return ade_kbc_step(k, fn, gn, fo, go, row_begin, row_end, rho, u, conc, st, launches);
  return with_ade_models(k.fluid, k.scalar, k.buoyant, [&](const auto& fm, const auto& sm, auto B) {
    using FM = std::decay_t<decltype(fm)>;
    using SM = std::decay_t<decltype(sm)>;
    constexpr bool kB = decltype(B)::value;
    return ade_step_sequence<kB>(k, fm, sm, fn, gn, fo, go, row_begin, row_end, rho, u, conc, st, launches,
        [&](const AdeDispatch& d) {
          with_flags([&](auto NL, auto NS, auto M) {
            LBM_KLAUNCH((k_ade_stream_collide<FM, SM, NL(), NS(), M(), kB>), dim3(d.grid), dim3(256), 0, st, fn, gn, fo, go,
                        k.g, fm, sm, row_begin, row_end, d.tiles, rho, u, conc, k.by);
          }, d.nt & 1, d.nt & 2, rho != nullptr);
        },
        [&](const AdeRows& r, long long* n) { return ade_table_passes<kB>(k, fm, sm, fn, gn, fo, go, r, rho, u, conc, st, n); });
  });
}

// one part of a call, after ade_part_args
int ade_part_from(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, int part, int edge_rows,
                  double* rho, double* u, double* conc, hipStream_t st) {
  if (k.kbc && k.buoyant) return ade_kbc_buoyant_part_from(k, fn, gn, fo, go, part, edge_rows, rho, u, conc, st);
  if (k.kbc) return ade_kbc_part_from(k, fn, gn, fo, go, part, edge_rows, rho, u, conc, st);
  return with_ade_models(k.fluid, k.scalar, k.buoyant, [&](const auto& fm, const auto& sm, auto B) {
    using FM = std::decay_t<decltype(fm)>;
    using SM = std::decay_t<decltype(sm)>;
    constexpr bool kB = decltype(B)::value;
    return ade_part_sequence(k, part, edge_rows,
        [&](const AdeDispatch& d, const AdeRows& r) {
          with_flags([&](auto NL, auto NS, auto M, auto F) {
            LBM_KLAUNCH((k_ade_stream_collide_part<FM, SM, NL(), NS(), M(), F(), kB>), dim3(d.grid), dim3(256), 0, st, fn, gn,
                        fo, go, k.g, k.bc, fm, sm, r.band0, r.n0, r.band1, r.nrows, d.tiles, rho, u, conc, k.sw, k.by);
          }, d.nt & 1, d.nt & 2, rho != nullptr, k.sw.fixed);
        },
        [&](const AdeRows& r, long long* n) { return ade_table_passes<kB>(k, fm, sm, fn, gn, fo, go, r, rho, u, conc, st, n); });
  });
}

// the carry pointers of a call against its open table: both given (carry_in: where the call reads one) and distinct
static int ade_carry_args(const char* fn, const AdeCall& k, bool reads, const double* carry_in, const double* carry_out) {
  if (k.n_open_nodes == 0) return LBM_OK;
  LBM_REQUIRE((!reads || carry_in) && carry_out, "%s: open boundaries: NULL carry with a table of %d nodes (%d doubles each)",
              fn, k.n_open_nodes, 2 * k.n_open_nodes);
  LBM_REQUIRE(!reads || carry_in != carry_out, "%s: open boundaries: carry_in and carry_out alias", fn);
  return LBM_OK;
}

// the carry of a slab's call, checked and kept in the call for its launches
int ade_carry_set(const char* fn, AdeCall* k, bool reads, const double* carry_in, double* carry_out) {
  if (int rc = ade_carry_args(fn, *k, reads, carry_in, carry_out)) return rc;
  k->carry_in = carry_in;
  k->carry_out = carry_out;
  return LBM_OK;
}

// The carry of a pre-collision state f -- u of the n listed nodes, k_ade_open_prime (it addresses through Geom::at) -- the
// one launch site of that kernel; an empty table enqueues nothing
static int ade_open_prime(const Geom& g, const AdeOpenNode* nodes, int n, const double* f, double* carry, hipStream_t st) {
  if (n == 0) return LBM_OK;
  LBM_KLAUNCH(k_ade_open_prime, dim3((n + 255) / 256), dim3(256), 0, st, f, g, nodes, n, carry);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

// the carry of a pre-collision state on a slab, over the call's view
int ade_open_prime_from(const AdeCall& k, const double* f, hipStream_t st) {
  return ade_open_prime(k.g, k.open_nodes, k.n_open_nodes, f, k.carry_out, st);
}

// the collide-only iteration; with a non-empty open table one more small launch writes carry_out from the pre-collision f
static int ade_collide(const char* fn, double* fp, double* gp, const double* f, const double* h, const lbm_geom* lg,
                       const lbm_bc* bc, const AdeFluid& fluid, const lbm_ade_params* scalar,
                       const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                       double* rho, double* u, double* conc, hipStream_t st, const lbm_ade_open* open = nullptr,
                       double* carry_out = nullptr, long long* launches = nullptr) {
  AdeCall k;
  int rc = ade_resolve(fn, lg, bc, fluid, scalar, sbc, buoy, iwalls, false, &k, open);
  if (!rc) rc = ade_carry_args(fn, k, false, nullptr, carry_out);
  if (!rc) rc = ade_collide_from(fn, k, fp, gp, f, h, rho, u, conc, st);
  if (rc) return rc;
  if (launches) ++*launches;
  if (k.n_open_nodes == 0) return LBM_OK;
  rc = ade_open_prime(k.g, k.open_nodes, k.n_open_nodes, f, carry_out, st);
  if (!rc && launches) ++*launches;
  return rc;
}

static int ade_stream_collide(const char* fn, double* fn_, double* gn, const double* fo, const double* go,
                              const lbm_geom* lg, const lbm_bc* lbc, const AdeFluid& fluid,
                              const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy,
                              const lbm_ade_iwalls* iwalls, int row_begin, int row_end, double* rho, double* u,
                              double* conc, hipStream_t st, long long* launches = nullptr,
                              const lbm_ade_open* open = nullptr, const double* carry_in = nullptr,
                              double* carry_out = nullptr) {
  AdeCall k;
  int rc = ade_resolve(fn, lg, lbc, fluid, scalar, sbc, buoy, iwalls, false, &k, open);
  if (!rc) rc = ade_lattice_args(fn, fn_, gn, fo, go, rho, u, conc, true);
  if (!rc) rc = ade_carry_set(fn, &k, true, carry_in, carry_out);
  if (rc) return rc;
  LBM_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= lg->R, "%s: row range [%d, %d) outside [0, %d)", fn,
              row_begin, row_end, lg->R);
  LBM_REQUIRE(k.n_open_nodes == 0 || (row_begin == 0 && row_end == lg->R),
              "%s: open boundaries: row range [%d, %d): the whole block [0, %d) only", fn, row_begin, row_end, lg->R);
  if (row_begin == row_end) return LBM_OK;
  return ade_step_from(k, fn_, gn, fo, go, row_begin, row_end, rho, u, conc, st, launches);
}

// the lattices and the part of a part launch, on the host
int ade_part_args(const char* fn, const AdeCall& k, const double* fn_, const double* gn, const double* fo,
                  const double* go, int part, int edge_rows, const double* rho, const double* u, const double* conc) {
  if (int rc = ade_lattice_args(fn, fn_, gn, fo, go, rho, u, conc, true)) return rc;
  LBM_REQUIRE(part == LBM_ADE_PART_FRAME || part == LBM_ADE_PART_INNER,
              "%s: part=%d (LBM_ADE_PART_FRAME or LBM_ADE_PART_INNER)", fn, part);
  LBM_REQUIRE(edge_rows >= 1 && 2 * edge_rows < k.g.R, "%s: edge_rows=%d: need 1 <= edge_rows and 2 x edge_rows < R=%d",
              fn, edge_rows, k.g.R);
  return LBM_OK;
}

// lbm_ade_stream_collide_part(_ex, _b, _w, _o, _m) under the caller's name
static int ade_part(const char* name, double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                    const lbm_bc* lbc, const AdeFluid& fluid, const lbm_ade_params* scalar,
                    const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls, int part,
                    int edge_rows, double* rho, double* u, double* conc, hipStream_t st,
                    const lbm_ade_open* view = nullptr, const double* carry_in = nullptr, double* carry_out = nullptr) {
  AdeCall k;
  int rc = ade_resolve(name, lg, lbc, fluid, scalar, sbc, buoy, iwalls, true, &k, view);
  if (!rc) rc = ade_part_args(name, k, fn, gn, fo, go, part, edge_rows, rho, u, conc);
  if (!rc) rc = ade_carry_set(name, &k, true, carry_in, carry_out);
  return rc ? rc : ade_part_from(k, fn, gn, fo, go, part, edge_rows, rho, u, conc, st);
}

// The wall exchange of rows [row_begin, row_end) of the stream from fo, go, under the caller's name: the host checks of the
// stream itself (ade_resolve; a single block or a slab, as the geometry says), the table's rows, one launch.  The region
// is clipped to the lattice here.  A buoyant call takes the reference-order model, as its step does.  Either fluid: a KBC
// fluid's launch is capi_ade_kbc_open.hip's.
static int ade_wallx_rows(const char* fn, double* table, int table_rows, int table_row0, const double* fo, const double* go,
                          const lbm_geom* lg, const lbm_bc* lbc, const AdeFluid& fluid, const lbm_ade_params* scalar,
                          const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                          const int* region4, int row_begin, int row_end, hipStream_t st) {
  AdeCall k;
  int rc = ade_resolve(fn, lg, lbc, fluid, scalar, sbc, buoy, iwalls, true, &k);
  if (rc) return rc;
  LBM_REQUIRE(table && fo && go, "%s: NULL argument (table, fo, go)", fn);
  rc = diag_range_check(fn, lg->R, row_begin, row_end);
  if (rc) return rc;
  LBM_REQUIRE(table_row0 >= 0 && table_rows > 0 && (long long)table_row0 + row_end <= table_rows,
              "%s: table_row0=%d + rows [%d, %d) do not fit table_rows=%d", fn, table_row0, row_begin, row_end, table_rows);
  auto clip = [](int v, int n) { return v < 0 ? 0 : v > n ? n : v; };
  const int r0 = region4 ? clip(region4[0], lg->R) : 0, r1 = region4 ? clip(region4[1], lg->R) : lg->R;
  const int c0 = region4 ? clip(region4[2], lg->C) : 0, c1 = region4 ? clip(region4[3], lg->C) : lg->C;
  const int* first = k.n_wall_nodes > 0 ? iwalls->d_first : nullptr;
  const int cap = tuning("grid_cap", 0);
  const int grid = capped_grid((row_end - row_begin + 3) / 4, cap > 0 ? cap : 8192);
  if (k.kbc) {  // capi_ade_kbc_open.hip
    const int region[4] = {r0, r1, c0, c1};
    return ade_kbc_wallx_launch(k, table, table_rows, table_row0, fo, go, first, region, row_begin, row_end, grid, st);
  }
  return with_ade_models(k.fluid, k.scalar, k.buoyant, [&](const auto& fm, const auto& sm, auto) {
    using FM = std::decay_t<decltype(fm)>;
    with_flags([&](auto F) {
      LBM_KLAUNCH((k_ade_wall_exchange<FM, F()>), dim3(grid), dim3(256), 0, st, table, table_rows, table_row0, fo, go, k.g,
                  k.bc, fm, sm.wr, sm.wc, k.sw, k.wall_nodes, first, r0, r1, c0, c1, row_begin, row_end);
    }, k.sw.fixed);
    LBM_CHECK_LAUNCH();
    return (int)LBM_OK;
  });
}

static int ade_wallx_fold_launch(double* out_dev, const double* table, int table_rows, int row_begin, int row_end,
                                 hipStream_t st) {
  LBM_KLAUNCH(k_ade_wallx_fold, dim3(1), dim3(64 * LBM_WALLX_NQ), 0, st, out_dev, table, table_rows, row_begin, row_end);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

}  // namespace lbm

// the driver loop on one block: two time levels, each one allocation holding the 9 planes of f followed by the
// 9 planes of g (18 padded planes in a row: the 36 concurrent streams of the step spread over the HBM channels)
struct lbm_ade_solver {
  lbm_geom g;  // padded geometry of either lattice
  lbm_bc bc;
  int model;             // LBM_MODEL_BGK: fluid; LBM_MODEL_KBC: kbc (lbm_ade_solver_create_m)
  lbm_bgk_params fluid;
  lbm_kbc_params kbc;
  lbm_ade_params scalar;
  lbm_ade_scalar_bc sbc;  // all NO_FLUX unless set
  bool fixed;             // some edge of sbc is FIXED
  lbm_ade_buoyancy buoy;  // lbm_ade_solver_set_buoyancy
  bool buoyant;           // buoy is set (beta = (0, 0) included: the launches decide)
  const lbm_ade_iwalls* walls;  // lbm_ade_solver_set_walls: borrowed, never copied
  const lbm_ade_open* open;     // lbm_ade_solver_set_open: borrowed, never copied
  double* carry[2];             // the open table's carried u, one per time level (carry[k] goes with lat[k]); NULL without
  hipStream_t st;
  double* lat[2];
  double* dense;  // [9][R][C] SoA scratch of get_state
  double* stage;  // [R][C][9] AoS staging
  double *rho, *u, *conc;
  int cur;    // lat[cur] holds the state
  bool post;  // the state is post-collision (P-form); false: pre-collision f_adve, g_adve
  long long steps, launches;
  lbm::DiagBuf diag;  // row table and result buffers of lbm_ade_solver_diag (allocated by its first call)
  lbm::DiagBuf wallx;  // the same of lbm_ade_solver_wall_exchange: [LBM_WALLX_NQ][R], LBM_WALLX_NQ values
  double* f(int k) const { return lat[k]; }
  double* h(int k) const { return lat[k] + 9 * g.plane_stride; }
};

using namespace lbm;

extern "C" {

int lbm_ade_collide(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                    const lbm_bgk_params* fluid, const lbm_ade_params* scalar, double* rho, double* u, double* conc,
                    lbm_stream_t s) {
  return ade_collide("lbm_ade_collide", fp, gp, f, g_in, g, bc, {fluid, nullptr}, scalar, nullptr, nullptr, nullptr, rho, u, conc,
                     as_stream(s));
}

int lbm_ade_collide_b(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                      const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                      const lbm_ade_buoyancy* buoy, double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_collide("lbm_ade_collide_b", fp, gp, f, g_in, g, bc, {fluid, nullptr}, scalar, sbc, buoy, nullptr, rho, u, conc,
                     as_stream(s));
}

int lbm_ade_stream_collide(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                           const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar, int row_begin,
                           int row_end, double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_stream_collide("lbm_ade_stream_collide", fn, gn, fo, go, g, bc, {fluid, nullptr}, scalar, nullptr, nullptr, nullptr,
                            row_begin, row_end, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_ex(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                              const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                              const lbm_ade_scalar_bc* sbc, int row_begin, int row_end, double* rho, double* u,
                              double* conc, lbm_stream_t s) {
  return ade_stream_collide("lbm_ade_stream_collide_ex", fn, gn, fo, go, g, bc, {fluid, nullptr}, scalar, sbc, nullptr, nullptr,
                            row_begin, row_end, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_b(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, int row_begin, int row_end,
                             double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_stream_collide("lbm_ade_stream_collide_b", fn, gn, fo, go, g, bc, {fluid, nullptr}, scalar, sbc, buoy, nullptr,
                            row_begin, row_end, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_w(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                             int row_begin, int row_end, double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_stream_collide("lbm_ade_stream_collide_w", fn, gn, fo, go, g, bc, {fluid, nullptr}, scalar, sbc, buoy, iwalls,
                            row_begin, row_end, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_part(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                                const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar, int part,
                                int edge_rows, double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_part("lbm_ade_stream_collide_part", fn, gn, fo, go, lg, lbc, {fluid, nullptr}, scalar, nullptr, nullptr, nullptr,
                  part, edge_rows, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_part_ex(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                                   const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                   const lbm_ade_scalar_bc* sbc, int part, int edge_rows, double* rho, double* u,
                                   double* conc, lbm_stream_t s) {
  return ade_part("lbm_ade_stream_collide_part_ex", fn, gn, fo, go, lg, lbc, {fluid, nullptr}, scalar, sbc, nullptr, nullptr, part,
                  edge_rows, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_part_b(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                                  const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, int part, int edge_rows,
                                  double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_part("lbm_ade_stream_collide_part_b", fn, gn, fo, go, lg, lbc, {fluid, nullptr}, scalar, sbc, buoy, nullptr, part,
                  edge_rows, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_part_w(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                                  const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                                  int part, int edge_rows, double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_part("lbm_ade_stream_collide_part_w", fn, gn, fo, go, lg, lbc, {fluid, nullptr}, scalar, sbc, buoy, iwalls, part,
                  edge_rows, rho, u, conc, as_stream(s));
}

// the context of either fluid, under the caller's name
static int ade_solver_create(const char* fn, lbm_ade_solver** out, const lbm_geom* g, const lbm_bc* bc, const AdeFluid& fluid,
                             const lbm_ade_params* scalar, lbm_stream_t s) {
  LBM_REQUIRE(out, "%s: NULL argument", fn);
  AdeCall unused;
  if (int rc = ade_resolve(fn, g, bc, fluid, scalar, nullptr, nullptr, nullptr, false, &unused)) return rc;
  LBM_REQUIRE(g->row_pitch == 0 && g->plane_stride == 0,
              "%s: the context pads its own lattices (row_pitch and plane_stride must be 0)", fn);
  lbm_ade_solver* sv = new (std::nothrow) lbm_ade_solver();
  LBM_REQUIRE(sv, "%s: out of host memory", fn);
  sv->g = *g;
  sv->bc = bc ? *bc : lbm_bc{0, 0, 0, 0, 0, 1.0, 1.0, 0.0, 0.0};
  sv->model = fluid.kbc ? LBM_MODEL_KBC : LBM_MODEL_BGK;
  sv->fluid = fluid.bgk ? *fluid.bgk : lbm_bgk_params{};
  sv->kbc = fluid.kbc ? *fluid.kbc : lbm_kbc_params{};
  sv->scalar = *scalar;
  sv->sbc = lbm_ade_scalar_bc{};
  sv->fixed = false;
  sv->buoy = lbm_ade_buoyancy{};
  sv->buoyant = false;
  sv->walls = nullptr;
  sv->open = nullptr;
  sv->carry[0] = sv->carry[1] = nullptr;
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
    set_error("%s: %s", fn, hipGetErrorString(e));
    lbm_ade_solver_destroy(sv);
    return LBM_ERR_HIP;
  }
  *out = sv;
  return LBM_OK;
}

int lbm_ade_solver_create(lbm_ade_solver** out, const lbm_geom* g, const lbm_bc* bc, const lbm_bgk_params* fluid,
                          const lbm_ade_params* scalar, lbm_stream_t s) {
  return ade_solver_create("lbm_ade_solver_create", out, g, bc, {fluid, nullptr}, scalar, s);
}

int lbm_ade_solver_create_m(lbm_ade_solver** out, const lbm_geom* g, const lbm_bc* bc, const lbm_ade_fluid* fluid,
                            const lbm_ade_params* scalar, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_solver_create_m", fluid, &fl)) return rc;
  return ade_solver_create(fl.kbc ? "lbm_ade_solver_create_m" : "lbm_ade_solver_create", out, g, bc, fl, scalar, s);
}

int lbm_ade_solver_destroy(lbm_ade_solver* sv) {
  if (!sv) return LBM_OK;
  if (sv->lat[0] || sv->lat[1]) (void)hipStreamSynchronize(sv->st);
  for (double* p : {sv->lat[0], sv->lat[1], sv->dense, sv->stage, sv->rho, sv->u, sv->conc, sv->carry[0], sv->carry[1]})
    if (p) (void)hipFree(p);
  sv->diag.release();
  sv->wallx.release();
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
  if (sv->open) {  // the carry of the state given
    rc = ade_open_prime(make_geom(g), sv->open->d_nodes, sv->open->n, sv->f(sv->cur), sv->carry[sv->cur], sv->st);
    if (rc) return rc;
  }
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));  // the host arrays may be reused by the caller
  sv->post = false;
  return LBM_OK;
}

// n driver iterations: the first on a pre-collision state is collide-only, every later one the fused step
// (one launch, two with wall edges).  Enqueues only: no allocation, no host synchronisation.
int lbm_ade_solver_step(lbm_ade_solver* sv, int n) {
  LBM_REQUIRE(sv && n >= 0, "lbm_ade_solver_step: bad argument (n=%d)", n);
  const lbm_ade_buoyancy* buoy = sv->buoyant ? &sv->buoy : nullptr;
  const AdeFluid fluid = sv->model == LBM_MODEL_KBC ? AdeFluid{nullptr, &sv->kbc} : AdeFluid{&sv->fluid, nullptr};
  for (int i = 0; i < n; ++i) {
    const int k = sv->cur, o = k ^ 1;
    int rc;
    if (!sv->post) {
      rc = ade_collide("lbm_ade_solver_step", sv->f(o), sv->h(o), sv->f(k), sv->h(k), &sv->g, &sv->bc, fluid, &sv->scalar,
                       nullptr, buoy, sv->walls, nullptr, nullptr, nullptr, sv->st, sv->open, sv->carry[o], &sv->launches);
    } else {
      rc = ade_stream_collide("lbm_ade_solver_step", sv->f(o), sv->h(o), sv->f(k), sv->h(k), &sv->g, &sv->bc, fluid,
                              &sv->scalar, sv->fixed ? &sv->sbc : nullptr, buoy, sv->walls, 0, sv->g.R, nullptr, nullptr,
                              nullptr, sv->st, &sv->launches, sv->open, sv->carry[k], sv->carry[o]);
    }
    if (rc) return rc;
    sv->cur = o;
    sv->post = true;
    ++sv->steps;
  }
  return LBM_OK;
}

// The device half of lbm_ade_solver_get_state, shared with lbm_ade_solver_diag: enqueues what leaves f_adve, g_adve in
// time level *k_out (the state itself, or its streamed image with every table's and edge's rule applied, in the dead
// level) and, if wanted, sv->rho / sv->u = the parity-operator moments of that f and sv->conc = calc_rho of that g.
static int ade_solver_form_state(lbm_ade_solver* sv, const char* fn, bool want_moments, bool want_conc, int* k_out) {
  const lbm_geom& g = sv->g;
  const int R = g.R, C = g.C;
  int k = sv->cur;
  const lbm_geom dg{R, C, 0, 0, 0};
  const bool fixed = sv->post && sv->fixed;
  bool have_u = false;  // sv->rho, sv->u hold the moments of the streamed f
  auto moments_of_f = [&]() {  // sv->rho = calc_rho, sv->u = calc_u of sv->f(k), through the parity operators
    int rc = lbm_lattice_copy_rows(sv->dense, &dg, 0, sv->f(k), &g, 0, R, sv->st);
    if (!rc) rc = lbm_calc_rho(sv->rho, sv->dense, R, C, sv->st);
    if (!rc) rc = lbm_calc_u(sv->u, sv->dense, sv->rho, R, C, sv->st);
    have_u = true;
    return rc;
  };
  if (sv->post) {
    const AdeIwallNode* wall_nodes;
    int n_wall_nodes;
    int rc = ade_iwalls_check(fn, sv->walls, &g, &wall_nodes, &n_wall_nodes);
    if (rc) return rc;
    const dim3 grid_w((n_wall_nodes + 255) / 256);
    // the open table, in the reference's order and without touching the carry: its f slots with the carry the next step
    // would read, moments, the domain's FIXED edges, its g slots through the map
    const int n_open = sv->open ? sv->open->n : 0;
    const dim3 grid_o((n_open + 255) / 256);
    const AdeOpenNode* open_nodes = n_open ? sv->open->d_nodes : nullptr;
    const AdeOpenSeg* open_segs = n_open ? sv->open->d_segs : nullptr;
    rc = lbm_stream(sv->f(k ^ 1), sv->f(k), &g, &sv->bc, sv->st);
    if (rc) return rc;
    if (n_open > 0) {
      LBM_KLAUNCH(k_ade_open_state<0>, grid_o, dim3(256), 0, sv->st, sv->f(k ^ 1), sv->f(k), make_geom(g), make_bc(&sv->bc),
                  open_nodes, open_segs, n_open, sv->carry[k], nullptr, 0.0, 0.0);
      LBM_CHECK_LAUNCH();
    }
    if (n_wall_nodes > 0) {  // the f slots, before the moments that the scalar's rules read
      LBM_KLAUNCH(k_ade_iwalls_state<false>, grid_w, dim3(256), 0, sv->st, sv->f(k ^ 1), sv->f(k), make_geom(g), wall_nodes,
                  n_wall_nodes, nullptr, 0.0, 0.0);
      LBM_CHECK_LAUNCH();
    }
    AdeWalls sw;
    rc = ade_scalar_bc_check(fn, fixed ? &sv->sbc : nullptr, &sv->bc, &sw);
    if (rc) return rc;
    // g gathers as BOUNCE_BACK at a FIXED column; the FIXED edges then take their rule with u = the reference-order
    // calc_u of the streamed f
    const Bc gather = ade_scalar_gather_bc(make_bc(&sv->bc), sw.fixed);
    lbm_bc gbc = sv->bc;
    gbc.col_lo = gather.col_lo, gbc.col_hi = gather.col_hi;
    rc = lbm_stream(sv->h(k ^ 1), sv->h(k), &g, &gbc, sv->st);
    if (rc) return rc;
    if (n_open > 0) {  // g of the listed nodes pulled again, through the map
      LBM_KLAUNCH(k_ade_open_state<1>, grid_o, dim3(256), 0, sv->st, sv->h(k ^ 1), sv->h(k), make_geom(g), gather, open_nodes,
                  open_segs, n_open, nullptr, nullptr, 0.0, 0.0);
      LBM_CHECK_LAUNCH();
    }
    k ^= 1;
    if (fixed || n_wall_nodes > 0 || n_open > 0)
      if ((rc = moments_of_f())) return rc;
    if (fixed) {
      const int n_edge = 2 * C + 2 * R;
      LBM_KLAUNCH(k_ade_fixed_state, dim3((n_edge + 255) / 256), dim3(256), 0, sv->st, sv->h(k), make_geom(g),
                  make_bc(&sv->bc), sw, sv->u, sv->scalar.w_r, sv->scalar.w_c);
      LBM_CHECK_LAUNCH();
    }
    if (n_wall_nodes > 0) {  // the g slots last: the table wins every slot it names (post-collision level: k ^ 1)
      LBM_KLAUNCH(k_ade_iwalls_state<true>, grid_w, dim3(256), 0, sv->st, sv->h(k), sv->h(k ^ 1), make_geom(g), wall_nodes,
                  n_wall_nodes, sv->u, sv->scalar.w_r, sv->scalar.w_c);
      LBM_CHECK_LAUNCH();
    }
    if (n_open > 0) {  // (no node carries a g slot of both tables: the step's host check)
      LBM_KLAUNCH(k_ade_open_state<2>, grid_o, dim3(256), 0, sv->st, sv->h(k), sv->h(k ^ 1), make_geom(g), gather, open_nodes,
                  open_segs, n_open, nullptr, sv->u, sv->scalar.w_r, sv->scalar.w_c);
      LBM_CHECK_LAUNCH();
    }
  }
  if (want_moments && !have_u)
    if (int rc = moments_of_f()) return rc;
  if (want_conc) {
    int rc = lbm_lattice_copy_rows(sv->dense, &dg, 0, sv->h(k), &g, 0, R, sv->st);
    if (!rc) rc = lbm_calc_rho(sv->conc, sv->dense, R, C, sv->st);
    if (rc) return rc;
  }
  *k_out = k;
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
  int k;
  int rc = ade_solver_form_state(sv, "lbm_ade_solver_get_state", rho || u, conc != nullptr, &k);
  if (rc) return rc;
  if (f) {
    rc = lbm_soa_to_aos_pitched(sv->stage, sv->f(k), R, C, 9, g.plane_stride, g.row_pitch, sv->st);
    if (rc) return rc;
    LBM_CHECK_HIP(hipMemcpyAsync(f, sv->stage, n * 9 * sizeof(double), hipMemcpyDeviceToHost, sv->st));
  }
  if (rho || u) {
    if (rho) LBM_CHECK_HIP(hipMemcpyAsync(rho, sv->rho, n * sizeof(double), hipMemcpyDeviceToHost, sv->st));
    if (u) {
      rc = lbm_soa_to_aos(sv->stage, sv->u, R, C, 2, sv->st);
      if (rc) return rc;
      LBM_CHECK_HIP(hipMemcpyAsync(u, sv->stage, n * 2 * sizeof(double), hipMemcpyDeviceToHost, sv->st));
    }
  }
  if (g_out) {
    rc = lbm_soa_to_aos_pitched(sv->stage, sv->h(k), R, C, 9, g.plane_stride, g.row_pitch, sv->st);
    if (rc) return rc;
    LBM_CHECK_HIP(hipMemcpyAsync(g_out, sv->stage, n * 9 * sizeof(double), hipMemcpyDeviceToHost, sv->st));
  }
  if (conc) LBM_CHECK_HIP(hipMemcpyAsync(conc, sv->conc, n * sizeof(double), hipMemcpyDeviceToHost, sv->st));
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));
  return LBM_OK;
}

int lbm_ade_solver_diag(lbm_ade_solver* sv, const double* profile_dev, int row_begin, int row_end, double* out_host,
                        double* table_host) {
  LBM_REQUIRE(sv && out_host, "lbm_ade_solver_diag: NULL argument (solver, out_host)");
  int rc = diag_range_check("lbm_ade_solver_diag", sv->g.R, row_begin, row_end);
  if (rc) return rc;
  int k;
  rc = ade_solver_form_state(sv, "lbm_ade_solver_diag", true, true, &k);
  if (rc) return rc;
  return diag_reduce("lbm_ade_solver_diag", sv->diag, sv->rho, sv->u, sv->conc, profile_dev, sv->g.R, sv->g.C, row_begin,
                     row_end, out_host, table_host, sv->st);
}

int lbm_ade_wallx_rows(double* table, int table_rows, int table_row0, const double* fo, const double* go, const lbm_geom* g,
                       const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                       const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                       const int* region4, int row_begin, int row_end, lbm_stream_t s) {
  return ade_wallx_rows("lbm_ade_wallx_rows", table, table_rows, table_row0, fo, go, g, bc, {fluid, nullptr}, scalar, sbc, buoy,
                        iwalls, region4, row_begin, row_end, as_stream(s));
}

int lbm_ade_wallx_rows_m(double* table, int table_rows, int table_row0, const double* fo, const double* go, const lbm_geom* g,
                         const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                         const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                         const int* region4, int row_begin, int row_end, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_wallx_rows_m", fluid, &fl)) return rc;
  return ade_wallx_rows(fl.kbc ? "lbm_ade_wallx_rows_m" : "lbm_ade_wallx_rows", table, table_rows, table_row0, fo, go, g, bc, fl,
                        scalar, sbc, buoy, iwalls, region4, row_begin, row_end, as_stream(s));
}

int lbm_ade_wallx_fold(double* out_dev, const double* table, int table_rows, int row_begin, int row_end, lbm_stream_t s) {
  int rc = diag_fold_check("lbm_ade_wallx_fold", out_dev, table, table_rows, row_begin, row_end);
  if (rc) return rc;
  return ade_wallx_fold_launch(out_dev, table, table_rows, row_begin, row_end, as_stream(s));
}

// the wall exchange of a context under the caller's name; kbc_ok: the entry serves a KBC context (the `_m` one)
static int ade_solver_wall_exchange(const char* fn, bool kbc_ok, lbm_ade_solver* sv, const int* region4, int row_begin,
                                    int row_end, double* out_host, double* table_host) {
  LBM_REQUIRE(sv && out_host, "%s: NULL argument (solver, out_host)", fn);
  LBM_REQUIRE(kbc_ok || sv->model != LBM_MODEL_KBC, "%s: the wall exchange is not supported with a KBC fluid", fn);
  const int R = sv->g.R;
  int rc = diag_range_check(fn, R, row_begin, row_end);
  if (rc) return rc;
  if (!sv->post) {
    set_error("%s: the state is pre-collision (no step yet): nothing has streamed", fn);
    return LBM_ERR_STATE;
  }
  DiagBuf& buf = sv->wallx;
  const size_t table_bytes = (size_t)LBM_WALLX_NQ * R * sizeof(double);
  if (!buf.table) {
    LBM_CHECK_HIP(hipMalloc(&buf.table, table_bytes));
    LBM_CHECK_HIP(hipMalloc(&buf.out_dev, LBM_WALLX_NQ * sizeof(double)));
    LBM_CHECK_HIP(hipHostMalloc(&buf.pinned, LBM_WALLX_NQ * sizeof(double)));
  }
  if (table_host && (row_begin > 0 || row_end < R)) LBM_CHECK_HIP(hipMemsetAsync(buf.table, 0, table_bytes, sv->st));
  const int k = sv->cur;
  const AdeFluid fluid = sv->model == LBM_MODEL_KBC ? AdeFluid{nullptr, &sv->kbc} : AdeFluid{&sv->fluid, nullptr};
  rc = ade_wallx_rows(fn, buf.table, R, 0, sv->f(k), sv->h(k), &sv->g, &sv->bc, fluid, &sv->scalar,
                      sv->fixed ? &sv->sbc : nullptr, sv->buoyant ? &sv->buoy : nullptr, sv->walls, region4, row_begin,
                      row_end, sv->st);
  if (!rc) rc = ade_wallx_fold_launch(buf.out_dev, buf.table, R, row_begin, row_end, sv->st);
  if (rc) return rc;
  LBM_CHECK_HIP(hipMemcpyAsync(buf.pinned, buf.out_dev, LBM_WALLX_NQ * sizeof(double), hipMemcpyDeviceToHost, sv->st));
  if (table_host) LBM_CHECK_HIP(hipMemcpyAsync(table_host, buf.table, table_bytes, hipMemcpyDeviceToHost, sv->st));
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));
  for (int q = 0; q < LBM_WALLX_NQ; ++q) out_host[q] = buf.pinned[q];
  return LBM_OK;
}

int lbm_ade_solver_wall_exchange(lbm_ade_solver* sv, const int* region4, int row_begin, int row_end, double* out_host,
                                 double* table_host) {
  return ade_solver_wall_exchange("lbm_ade_solver_wall_exchange", false, sv, region4, row_begin, row_end, out_host, table_host);
}

// a BGK context: the call above, under its name
int lbm_ade_solver_wall_exchange_m(lbm_ade_solver* sv, const int* region4, int row_begin, int row_end, double* out_host,
                                   double* table_host) {
  const bool kbc = sv && sv->model == LBM_MODEL_KBC;
  return ade_solver_wall_exchange(kbc ? "lbm_ade_solver_wall_exchange_m" : "lbm_ade_solver_wall_exchange", true, sv, region4,
                                  row_begin, row_end, out_host, table_host);
}

int lbm_ade_solver_run_until(lbm_ade_solver* sv, const lbm_converge* cv, int max_steps, int* steps_done, int* converged,
                             double* last_value) {
  int rc = diag_converge_check("lbm_ade_solver_run_until", cv, max_steps);
  if (rc) return rc;
  LBM_REQUIRE(sv, "lbm_ade_solver_run_until: NULL solver");
  rc = diag_range_check("lbm_ade_solver_run_until", sv->g.R, cv->row_begin, cv->row_end);
  if (rc) return rc;
  const double nodes = (double)(cv->row_end - cv->row_begin) * sv->g.C;
  return diag_run_until(
      cv, max_steps, steps_done, converged, last_value, [&](int n) { return lbm_ade_solver_step(sv, n); },
      [&](double* v) {
        double out[LBM_DIAG_NQ] = {0.0};
        const int rc2 = lbm_ade_solver_diag(sv, nullptr, cv->row_begin, cv->row_end, out, nullptr);
        *v = out[cv->quantity] / nodes;
        return rc2;
      });
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
  int rc = ade_buoyancy_check("lbm_ade_solver_set_buoyancy", buoy);
  if (rc) return rc;
  LBM_REQUIRE(sv->model != LBM_MODEL_KBC || !buoy || (buoy->beta_r == 0.0 && buoy->beta_c == 0.0),
              "lbm_ade_solver_set_buoyancy: buoyancy with beta=(%g, %g) is not supported with a KBC fluid (the forced "
              "collision is the BGK fluid's)", buoy->beta_r, buoy->beta_c);
  sv->buoy = buoy ? *buoy : lbm_ade_buoyancy{};
  sv->buoyant = buoy != nullptr;
  return LBM_OK;
}

int lbm_ade_solver_set_buoyancy_m(lbm_ade_solver* sv, const lbm_ade_buoyancy* buoy) {
  LBM_REQUIRE(sv, "lbm_ade_solver_set_buoyancy_m: NULL solver");
  if (sv->model == LBM_MODEL_BGK) return lbm_ade_solver_set_buoyancy(sv, buoy);
  int rc = ade_buoyancy_check("lbm_ade_solver_set_buoyancy_m", buoy);
  if (rc) return rc;
  sv->buoy = buoy ? *buoy : lbm_ade_buoyancy{};
  sv->buoyant = buoy != nullptr;
  return LBM_OK;
}

int lbm_ade_solver_set_walls(lbm_ade_solver* sv, const lbm_ade_iwalls* iwalls) {
  LBM_REQUIRE(sv, "lbm_ade_solver_set_walls: NULL solver");
  const AdeIwallNode* nodes;
  int n;
  int rc = ade_iwalls_check("lbm_ade_solver_set_walls", iwalls, &sv->g, &nodes, &n);
  if (rc) return rc;
  sv->walls = iwalls;
  return LBM_OK;
}

int lbm_ade_iwalls_create(lbm_ade_iwalls** out, int R, int C) {
  LBM_REQUIRE(out, "lbm_ade_iwalls_create: NULL argument");
  LBM_REQUIRE(R >= 1 && C >= 1, "lbm_ade_iwalls_create: R=%d C=%d must be positive", R, C);
  lbm_ade_iwalls* t = new (std::nothrow) lbm_ade_iwalls();
  LBM_REQUIRE(t, "lbm_ade_iwalls_create: out of host memory");
  t->R = R;
  t->C = C;
  *out = t;
  return LBM_OK;
}

int lbm_ade_iwalls_add(lbm_ade_iwalls* t, int r0, int c0, int dr, int dc, int n, unsigned f_slots, unsigned g_slots,
                       int g_mode, double conc) {
  const char* fn = "lbm_ade_iwalls_add";
  LBM_REQUIRE(t, "%s: NULL table", fn);
  LBM_REQUIRE(!t->finalized, "%s: the table is finalized (immutable after lbm_ade_iwalls_finalize)", fn);
  LBM_REQUIRE(n >= 1, "%s: n=%d must be at least 1", fn, n);
  LBM_REQUIRE(dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1 && (dr != 0 || dc != 0),
              "%s: step (dr, dc)=(%d, %d): each of -1, 0, 1 and not both 0", fn, dr, dc);
  LBM_REQUIRE(f_slots <= 0xFFu && g_slots <= 0xFFu, "%s: slot mask f_slots=0x%x g_slots=0x%x above 0xFF (bit s-1 = slot s, s in 1..8)",
              fn, f_slots, g_slots);
  LBM_REQUIRE(f_slots != 0 || g_slots != 0, "%s: f_slots and g_slots are both 0: the segment names no slot", fn);
  LBM_REQUIRE(g_mode == LBM_ADE_SCALAR_NO_FLUX || g_mode == LBM_ADE_SCALAR_FIXED,
              "%s: g_mode=%d (LBM_ADE_SCALAR_NO_FLUX or LBM_ADE_SCALAR_FIXED)", fn, g_mode);
  LBM_REQUIRE(std::isfinite(conc), "%s: conc=%g must be finite", fn, conc);
  if (r0 < 0) r0 += t->R;  // from the end, as the reference's slices count
  if (c0 < 0) c0 += t->C;
  for (long long k : {0LL, (long long)n - 1}) {  // the segment is linear: its two ends decide
    const long long r = r0 + k * dr, c = c0 + k * dc;
    LBM_REQUIRE(r >= 0 && r < t->R && c >= 0 && c < t->C, "%s: node (%lld, %lld) outside the %d x %d lattice", fn, r, c,
                t->R, t->C);
  }
  const bool fixed = g_mode == LBM_ADE_SCALAR_FIXED && g_slots != 0;
  // conflicts first: nothing is added on a refusal
  for (int k = 0; k < n; ++k) {
    const int r = r0 + k * dr, c = c0 + k * dc;
    const auto it = t->nodes.find({r, c});
    if (it == t->nodes.end()) continue;
    const lbm_ade_iwalls::Entry& e = it->second;
    const unsigned clash = g_slots & (fixed ? e.g & ~e.g_fixed : e.g_fixed);
    if (clash) {
      int s = 1;
      while (!((clash >> (s - 1)) & 1u)) ++s;
      LBM_REQUIRE(false, "%s: node (%d, %d): g slot %d named with two modes (NO_FLUX and FIXED)", fn, r, c, s);
    }
    LBM_REQUIRE(!fixed || !e.has_conc || e.conc == conc, "%s: node (%d, %d): FIXED conc=%g differs from the conc=%g the node has",
                fn, r, c, conc, e.conc);
  }
  for (int k = 0; k < n; ++k) {
    lbm_ade_iwalls::Entry& e = t->nodes[{r0 + k * dr, c0 + k * dc}];
    e.f |= f_slots;
    e.g |= g_slots;
    if (fixed) {
      e.g_fixed |= g_slots;
      e.conc = conc;
      e.has_conc = true;
    }
  }
  return LBM_OK;
}

int lbm_ade_iwalls_slab(lbm_ade_iwalls** out, const lbm_ade_iwalls* table, int row0, int R) {
  const char* fn = "lbm_ade_iwalls_slab";
  LBM_REQUIRE(out && table, "%s: NULL argument", fn);
  LBM_REQUIRE(row0 >= 0, "%s: row0=%d must not be negative", fn, row0);
  LBM_REQUIRE(R >= 1, "%s: R=%d must be at least 1", fn, R);
  LBM_REQUIRE((long long)row0 + R <= table->R, "%s: rows [%d, %lld) beyond the %d rows of the table", fn, row0,
              (long long)row0 + R, table->R);
  lbm_ade_iwalls* t = new (std::nothrow) lbm_ade_iwalls();
  LBM_REQUIRE(t, "%s: out of host memory", fn);
  t->R = R;
  t->C = table->C;
  // the map is sorted by (r, c): the rows of the view are one range of it, and stay in order with r - row0
  for (auto it = table->nodes.lower_bound({row0, 0}); it != table->nodes.end() && it->first.first < row0 + R; ++it)
    t->nodes.emplace_hint(t->nodes.end(), std::make_pair(it->first.first - row0, it->first.second), it->second);
  *out = t;
  return LBM_OK;
}

int lbm_ade_iwalls_count(const lbm_ade_iwalls* t) { return t ? (int)t->nodes.size() : 0; }

int lbm_ade_iwalls_node(const lbm_ade_iwalls* t, int i, int* r, int* c, unsigned* f_slots, unsigned* g_slots,
                        unsigned* g_fixed_slots, double* conc) {
  LBM_REQUIRE(t, "lbm_ade_iwalls_node: NULL table");
  LBM_REQUIRE(i >= 0 && i < (int)t->nodes.size(), "lbm_ade_iwalls_node: node %d outside [0, %d)", i, (int)t->nodes.size());
  auto it = t->nodes.begin();
  std::advance(it, i);
  if (r) *r = it->first.first;
  if (c) *c = it->first.second;
  if (f_slots) *f_slots = it->second.f;
  if (g_slots) *g_slots = it->second.g;
  if (g_fixed_slots) *g_fixed_slots = it->second.g_fixed;
  if (conc) *conc = it->second.conc;
  return LBM_OK;
}

int lbm_ade_iwalls_finalize(lbm_ade_iwalls* t) {
  LBM_REQUIRE(t, "lbm_ade_iwalls_finalize: NULL table");
  LBM_REQUIRE(!t->finalized, "lbm_ade_iwalls_finalize: the table is finalized already");
  if (!t->nodes.empty()) {  // an empty table makes no device call: it is NULL's
    std::vector<AdeIwallNode> host;
    std::vector<int> first((size_t)t->R + 1, 0);  // node counts per row, then their running sum
    host.reserve(t->nodes.size());
    for (const auto& kv : t->nodes) ++first[(size_t)kv.first.first + 1];
    for (int r = 0; r < t->R; ++r) first[(size_t)r + 1] += first[r];
    for (const auto& kv : t->nodes)
      host.push_back(AdeIwallNode{kv.first.first, kv.first.second, kv.second.f | (kv.second.g << 8) | (kv.second.g_fixed << 16),
                                  0, kv.second.conc});
    LBM_CHECK_HIP(hipMalloc(&t->d_nodes, host.size() * sizeof(AdeIwallNode)));
    hipError_t e = hipMalloc(&t->d_first, first.size() * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(t->d_nodes, host.data(), host.size() * sizeof(AdeIwallNode), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_first, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(t->d_nodes);
      if (t->d_first) (void)hipFree(t->d_first);
      t->d_nodes = nullptr;
      t->d_first = nullptr;
      set_error("lbm_ade_iwalls_finalize: %s", hipGetErrorString(e));
      return LBM_ERR_HIP;
    }
    t->n = (int)host.size();
    t->first = std::move(first);
  }
  t->finalized = true;
  return LBM_OK;
}

int lbm_ade_iwalls_destroy(lbm_ade_iwalls* t) {
  if (!t) return LBM_OK;
  if (t->d_nodes) (void)hipFree(t->d_nodes);
  if (t->d_first) (void)hipFree(t->d_first);
  delete t;
  return LBM_OK;
}

// ---- open boundaries (lbm_ade_open) -------------------------------------------------------------------------------------
int lbm_ade_open_create(lbm_ade_open** out, int R, int C) {
  LBM_REQUIRE(out, "lbm_ade_open_create: NULL argument");
  LBM_REQUIRE(R >= 1 && C >= 1, "lbm_ade_open_create: R=%d C=%d must be positive", R, C);
  LBM_REQUIRE(((long long)R + 2) * C < (1LL << 31), "lbm_ade_open_create: R=%d C=%d: (R + 2) x C is more than 2^31 - 1 nodes "
              "(the table's source encoding)", R, C);
  lbm_ade_open* t = new (std::nothrow) lbm_ade_open();
  LBM_REQUIRE(t, "lbm_ade_open_create: out of host memory");
  t->R = R;
  t->C = C;
  *out = t;
  return LBM_OK;
}

// the checks every kind of segment shares; r0 / c0 come back counted from the start
static int ade_open_segment(const char* fn, lbm_ade_open* t, int* r0, int* c0, int dr, int dc, int n) {
  LBM_REQUIRE(t, "%s: NULL table", fn);
  LBM_REQUIRE(!t->view, "%s: the table is a slab view (lbm_ade_open_slab): it takes no segments -- add them to the global "
              "table and take the view after", fn);
  LBM_REQUIRE(!t->finalized, "%s: the table is finalized (immutable after lbm_ade_open_finalize)", fn);
  LBM_REQUIRE(t->segs.size() < 255, "%s: the table holds 255 segments already", fn);
  LBM_REQUIRE(n >= 1, "%s: n=%d must be at least 1", fn, n);
  LBM_REQUIRE(dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1 && (dr != 0 || dc != 0),
              "%s: step (dr, dc)=(%d, %d): each of -1, 0, 1 and not both 0", fn, dr, dc);
  if (*r0 < 0) *r0 += t->R;  // from the end, as the reference's slices count
  if (*c0 < 0) *c0 += t->C;
  for (long long k : {0LL, (long long)n - 1}) {  // the segment is linear: its two ends decide
    const long long r = *r0 + k * dr, c = *c0 + k * dc;
    LBM_REQUIRE(r >= 0 && r < t->R && c >= 0 && c < t->C, "%s: node (%lld, %lld) outside the %d x %d lattice", fn, r, c,
                t->R, t->C);
  }
  return LBM_OK;
}

// node + (or, oc) inside the lattice for both ends of the segment (no wrap)
static int ade_open_offset(const char* fn, const lbm_ade_open* t, int r0, int c0, int dr, int dc, int n, int or_, int oc,
                           const char* what) {
  LBM_REQUIRE(or_ != 0 || oc != 0, "%s: %s offset (0, 0): the node itself", fn, what);
  for (long long k : {0LL, (long long)n - 1}) {
    const long long r = r0 + k * dr, c = c0 + k * dc;
    LBM_REQUIRE(r + or_ >= 0 && r + or_ < t->R && c + oc >= 0 && c + oc < t->C,
                "%s: node (%lld, %lld): %s (%lld, %lld) outside the %d x %d lattice", fn, r, c, what, r + or_, c + oc, t->R,
                t->C);
  }
  return LBM_OK;
}

int lbm_ade_open_add_f(lbm_ade_open* t, int r0, int c0, int dr, int dc, int n, unsigned slots, int rule, double p0,
                       double p1, int nr, int nc) {
  const char* fn = "lbm_ade_open_add_f";
  if (int rc = ade_open_segment(fn, t, &r0, &c0, dr, dc, n)) return rc;
  LBM_REQUIRE(slots >= 1 && slots <= 0xFFu, "%s: slot mask slots=0x%x (bit s-1 = slot s, s in 1..8; at least one)", fn, slots);
  LBM_REQUIRE(rule >= LBM_ADE_OPEN_BOUNCE_BACK && rule <= LBM_ADE_OPEN_ABB_EXTRAPOLATED, "%s: rule=%d (LBM_ADE_OPEN_*)", fn, rule);
  const bool abb = rule == LBM_ADE_OPEN_ABB || rule == LBM_ADE_OPEN_ABB_EXTRAPOLATED;
  LBM_REQUIRE(!abb || (std::isfinite(p0) && std::isfinite(p1)), "%s: (p0, p1)=(%g, %g) must be finite", fn, p0, p1);
  if (rule == LBM_ADE_OPEN_ABB_EXTRAPOLATED) {
    if (int rc = ade_open_offset(fn, t, r0, c0, dr, dc, n, nr, nc, "neighbour")) return rc;
  } else {
    nr = nc = 0;
  }
  t->segs.push_back(lbm_ade_open::Seg{lbm_ade_open::F_RULE, r0, c0, dr, dc, n, slots, rule, abb ? p0 : 0.0, abb ? p1 : 0.0, nr, nc});
  ade_open_resolve(t);
  return LBM_OK;
}

int lbm_ade_open_add_g(lbm_ade_open* t, int r0, int c0, int dr, int dc, int n, unsigned slots, int g_mode, double conc) {
  const char* fn = "lbm_ade_open_add_g";
  if (int rc = ade_open_segment(fn, t, &r0, &c0, dr, dc, n)) return rc;
  LBM_REQUIRE(slots >= 1 && slots <= 0xFFu, "%s: slot mask slots=0x%x (bit s-1 = slot s, s in 1..8; at least one)", fn, slots);
  LBM_REQUIRE(g_mode == LBM_ADE_SCALAR_NO_FLUX || g_mode == LBM_ADE_SCALAR_FIXED,
              "%s: g_mode=%d (LBM_ADE_SCALAR_NO_FLUX or LBM_ADE_SCALAR_FIXED)", fn, g_mode);
  LBM_REQUIRE(std::isfinite(conc), "%s: conc=%g must be finite", fn, conc);
  t->segs.push_back(lbm_ade_open::Seg{lbm_ade_open::G_RULE, r0, c0, dr, dc, n, slots, g_mode, conc, 0.0, 0, 0});
  ade_open_resolve(t);
  return LBM_OK;
}

int lbm_ade_open_add_g_copy(lbm_ade_open* t, int r0, int c0, int dr, int dc, int n, int from_dr, int from_dc) {
  const char* fn = "lbm_ade_open_add_g_copy";
  if (int rc = ade_open_segment(fn, t, &r0, &c0, dr, dc, n)) return rc;
  if (int rc = ade_open_offset(fn, t, r0, c0, dr, dc, n, from_dr, from_dc, "copy source")) return rc;
  t->segs.push_back(lbm_ade_open::Seg{lbm_ade_open::G_COPY, r0, c0, dr, dc, n, 0u, 0, 0.0, 0.0, from_dr, from_dc});
  ade_open_resolve(t);
  return LBM_OK;
}

int lbm_ade_open_add_channel(lbm_ade_open* t, double u_in, double conc_w, int conc_rows) {
  const char* fn = "lbm_ade_open_add_channel";
  LBM_REQUIRE(t, "%s: NULL table", fn);
  LBM_REQUIRE(!t->view, "%s: the table is a slab view (lbm_ade_open_slab): it takes no segments -- add them to the global "
              "table and take the view after", fn);
  LBM_REQUIRE(!t->finalized, "%s: the table is finalized (immutable after lbm_ade_open_finalize)", fn);
  const int R = t->R, C = t->C;
  LBM_REQUIRE(R >= 3 && C >= 2, "%s: R=%d C=%d: the channel needs R >= 3 and C >= 2", fn, R, C);
  LBM_REQUIRE(std::isfinite(u_in) && std::isfinite(conc_w), "%s: u_in=%g conc_w=%g must be finite", fn, u_in, conc_w);
  LBM_REQUIRE(conc_rows >= 0, "%s: conc_rows=%d must not be negative", fn, conc_rows);
  LBM_REQUIRE(t->segs.size() + 9 <= 255, "%s: the table holds too many segments already", fn);
  const int first = R - conc_rows > 1 ? R - conc_rows : 1;  // the inlet's rows of the last conc_rows rows: first .. R-2
  // f: inlet (:150-161), outlet over all rows (:163-172), the specular top (:175-177), and the bottom corner of the outlet
  // column back to the no-slip row (:180-182; the row itself is the domain's)
  int rc = lbm_ade_open_add_f(t, 1, 0, 1, 0, R - 2, 0xFFu, LBM_ADE_OPEN_ABB, 0.0, u_in, 0, 0);
  if (!rc) rc = lbm_ade_open_add_f(t, 0, C - 1, 1, 0, R, 0xFFu, LBM_ADE_OPEN_ABB_EXTRAPOLATED, 1.5, -0.5, 0, -1);
  if (!rc) rc = lbm_ade_open_add_f(t, 0, 0, 0, 1, C, 0x91u, LBM_ADE_OPEN_SPECULAR_ROW, 0.0, 0.0, 0, 0);
  if (!rc) rc = lbm_ade_open_add_f(t, R - 1, C - 1, 0, 1, 1, 0x64u, LBM_ADE_OPEN_BOUNCE_BACK, 0.0, 0.0, 0, 0);
  // g: the zero-gradient copies, top then outlet (:138-141); the concentration inlet (:203-218)
  if (!rc) rc = lbm_ade_open_add_g_copy(t, 0, 0, 0, 1, C, 1, 0);
  if (!rc && R > 2) rc = lbm_ade_open_add_g_copy(t, 1, C - 1, 1, 0, R - 2, 0, -1);
  if (!rc) rc = lbm_ade_open_add_g(t, 1, 0, 1, 0, R - 2, 0xFFu, LBM_ADE_SCALAR_FIXED, 0.0);
  if (!rc && first <= R - 2) rc = lbm_ade_open_add_g(t, first, 0, 1, 0, R - 1 - first, 0xFFu, LBM_ADE_SCALAR_FIXED, conc_w);
  return rc;
}

int lbm_ade_open_count(const lbm_ade_open* t) { return t ? (int)t->nodes.size() : 0; }

long long lbm_ade_open_carry_len(const lbm_ade_open* t) { return t ? 2LL * (long long)t->nodes.size() : 0; }

int lbm_ade_open_node(const lbm_ade_open* t, int i, int* r, int* c, int* f_rule, int* g_rule, int* g_src_r, int* g_src_c) {
  LBM_REQUIRE(t, "lbm_ade_open_node: NULL table");
  LBM_REQUIRE(i >= 0 && i < (int)t->nodes.size(), "lbm_ade_open_node: node %d outside [0, %d)", i, (int)t->nodes.size());
  const AdeOpenNode& nd = t->nodes[(size_t)i];
  if (r) *r = nd.r;
  if (c) *c = nd.c;
  for (int s = 1; s < Q; ++s) {
    const int jf = (int)((nd.fseg[(s - 1) >> 2] >> (8 * ((s - 1) & 3))) & 0xFFu);
    const int jg = (int)((nd.gseg[(s - 1) >> 2] >> (8 * ((s - 1) & 3))) & 0xFFu);
    if (f_rule) f_rule[s - 1] = jf ? t->segs[(size_t)jf - 1].rule : 0;
    if (g_rule) g_rule[s - 1] = jg ? 1 + t->segs[(size_t)jg - 1].rule : 0;
  }
  for (int q = 0; q < Q; ++q) {
    if (g_src_r) g_src_r[q] = nd.gsrc[q] / t->C - 1;  // an ordinary table: in [0, R); a view: in [-1, R]
    if (g_src_c) g_src_c[q] = nd.gsrc[q] % t->C;
  }
  return LBM_OK;
}

int lbm_ade_open_unreachable(const lbm_ade_open* t, int i) {
  if (!t || i < 0 || i >= (int)t->nodes.size()) return 0;
  return t->nodes[(size_t)i].pad;  // 0 but in a view
}

int lbm_ade_open_finalize(lbm_ade_open* t) {
  LBM_REQUIRE(t, "lbm_ade_open_finalize: NULL table");
  LBM_REQUIRE(!t->finalized, "lbm_ade_open_finalize: the table is finalized already");
  if (!t->nodes.empty()) {  // an empty table makes no device call: it is NULL's
    std::vector<AdeOpenSeg> segs;
    segs.reserve(t->segs.size());
    for (const lbm_ade_open::Seg& s : t->segs) segs.push_back(AdeOpenSeg{s.rule, 0, s.p0, s.p1});
    LBM_CHECK_HIP(hipMalloc(&t->d_nodes, t->nodes.size() * sizeof(AdeOpenNode)));
    hipError_t e = hipMalloc(&t->d_segs, segs.size() * sizeof(AdeOpenSeg));
    if (e == hipSuccess) e = hipMemcpy(t->d_nodes, t->nodes.data(), t->nodes.size() * sizeof(AdeOpenNode), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_segs, segs.data(), segs.size() * sizeof(AdeOpenSeg), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(t->d_nodes);
      if (t->d_segs) (void)hipFree(t->d_segs);
      t->d_nodes = nullptr;
      t->d_segs = nullptr;
      set_error("lbm_ade_open_finalize: %s", hipGetErrorString(e));
      return LBM_ERR_HIP;
    }
    t->n = (int)t->nodes.size();
    t->first.assign((size_t)t->R + 1, 0);  // the row index: node counts per row, then their running sum
    for (const AdeOpenNode& nd : t->nodes) ++t->first[(size_t)nd.r + 1];
    for (int r = 0; r < t->R; ++r) t->first[(size_t)r + 1] += t->first[r];
  }
  t->finalized = true;
  return LBM_OK;
}

int lbm_ade_open_slab(lbm_ade_open** out, const lbm_ade_open* table, int row0, int R) {
  const char* fn = "lbm_ade_open_slab";
  LBM_REQUIRE(out && table, "%s: NULL argument", fn);
  LBM_REQUIRE(!table->view, "%s: the table is itself a slab view: views are taken of the global table", fn);
  LBM_REQUIRE(row0 >= 0, "%s: row0=%d must not be negative", fn, row0);
  LBM_REQUIRE(R >= 1, "%s: R=%d must be at least 1", fn, R);
  LBM_REQUIRE((long long)row0 + R <= table->R, "%s: rows [%d, %lld) beyond the %d rows of the table", fn, row0,
              (long long)row0 + R, table->R);
  const int C = table->C, Rg = table->R;  // (R + 2) C <= (Rg + 2) C < 2^31: the source encoding holds (lbm_ade_open_create)
  // the parent's nodes are sorted by (r, c): the rows of the view are one range [i0, i1) of them
  auto row_begin = [table](int r) {
    return (int)(std::lower_bound(table->nodes.begin(), table->nodes.end(), r,
                                  [](const AdeOpenNode& a, int b) { return a.r < b; }) - table->nodes.begin());
  };
  const int i0 = row_begin(row0), i1 = row_begin(row0 + R);
  std::vector<AdeOpenNode> nodes(table->nodes.begin() + i0, table->nodes.begin() + i1);
  for (AdeOpenNode& nd : nodes) {
    const int rg = nd.r;
    nd.r -= row0;
    nd.pad = 0;
    for (int q = 0; q < Q; ++q) {
      // the source's global row modulo the parent's rows, as the slab-local row in [-1, R] nearest to the plain pull
      const int sr = nd.gsrc[q] / C - 1, pull = nd.r - icx(q);
      int sc = nd.gsrc[q] % C, best = 0;
      bool found = false;
      for (int cand : {sr - row0 - Rg, sr - row0, sr - row0 + Rg})
        if (cand >= -1 && cand <= R && (!found || std::abs(cand - pull) < std::abs(best - pull))) best = cand, found = true;
      if (!found) {  // more than one row outside the slab: the plain pull source, marked unreachable
        nd.pad |= 1 << q;
        best = pull;
        sc = (nd.c - icy(q) + C) % C;
      }
      nd.gsrc[q] = (best + 1) * C + sc;
    }
    for (int s = 1; s < Q; ++s) {
      const int j = (int)((nd.fseg[(s - 1) >> 2] >> (8 * ((s - 1) & 3))) & 0xFFu);
      if (!j || table->segs[(size_t)j - 1].rule != LBM_ADE_OPEN_ABB_EXTRAPOLATED) continue;
      const int m = nd.xn[s - 1];
      LBM_REQUIRE(m >= i0 && m < i1, "%s: node (%d, %d), f slot %d: its extrapolation neighbour (%d, %d) lies outside rows "
                  "[%d, %d) of the view (the carry is slab-local: no carry exchange between slabs)", fn, rg, nd.c, s,
                  table->nodes[(size_t)m].r, table->nodes[(size_t)m].c, row0, row0 + R);
      nd.xn[s - 1] = m - i0;
    }
  }
  lbm_ade_open* t = new (std::nothrow) lbm_ade_open();
  LBM_REQUIRE(t, "%s: out of host memory", fn);
  t->R = R;
  t->C = C;
  t->segs = table->segs;
  t->nodes = std::move(nodes);
  t->view = true;
  t->row0 = row0;
  t->R_parent = Rg;
  *out = t;
  return LBM_OK;
}

int lbm_ade_open_destroy(lbm_ade_open* t) {
  if (!t) return LBM_OK;
  if (t->d_nodes) (void)hipFree(t->d_nodes);
  if (t->d_segs) (void)hipFree(t->d_segs);
  delete t;
  return LBM_OK;
}

int lbm_ade_collide_o(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                      const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                      const lbm_ade_buoyancy* buoy, const lbm_ade_open* open, double* carry_out, double* rho, double* u,
                      double* conc, lbm_stream_t s) {
  return ade_collide("lbm_ade_collide_o", fp, gp, f, g_in, g, bc, {fluid, nullptr}, scalar, sbc, buoy, nullptr, rho, u, conc,
                     as_stream(s), open, carry_out);
}

int lbm_ade_stream_collide_o(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                             const lbm_ade_open* open, const double* carry_in, double* carry_out, int row_begin,
                             int row_end, double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_stream_collide("lbm_ade_stream_collide_o", fn, gn, fo, go, g, bc, {fluid, nullptr}, scalar, sbc, buoy, iwalls, row_begin,
                            row_end, rho, u, conc, as_stream(s), nullptr, open, carry_in, carry_out);
}

int lbm_ade_stream_collide_part_o(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* lg,
                                  const lbm_bc* lbc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                                  const lbm_ade_open* view, const double* carry_in, double* carry_out, int part,
                                  int edge_rows, double* rho, double* u, double* conc, lbm_stream_t s) {
  return ade_part("lbm_ade_stream_collide_part_o", fn, gn, fo, go, lg, lbc, {fluid, nullptr}, scalar, sbc, buoy, iwalls, part,
                  edge_rows, rho, u, conc, as_stream(s), view, carry_in, carry_out);
}

// The fluid by model (lbm_ade_fluid): the `_m` entries and their buoyant forms `_mb`.  model = BGK: the checks and launches
// of the call they name in lbm_hip.h -- lbm_ade_collide_b, lbm_ade_stream_collide_w, lbm_ade_stream_collide_part_w --
// under that call's name; model = KBC: the same entry with the KBC fluid, under their own.
int lbm_ade_collide_m(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                      const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc, double* rho,
                      double* u, double* conc, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_collide_m", fluid, &fl)) return rc;
  return ade_collide(fl.kbc ? "lbm_ade_collide_m" : "lbm_ade_collide_b", fp, gp, f, g_in, g, bc, fl, scalar, sbc, nullptr,
                     nullptr, rho, u, conc, as_stream(s));
}

int lbm_ade_collide_mb(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                       const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                       const lbm_ade_buoyancy* buoy, double* rho, double* u, double* conc, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_collide_mb", fluid, &fl)) return rc;
  return ade_collide(fl.kbc ? "lbm_ade_collide_mb" : "lbm_ade_collide_b", fp, gp, f, g_in, g, bc, fl, scalar, sbc, buoy,
                     nullptr, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_m(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_iwalls* iwalls, int row_begin, int row_end,
                             double* rho, double* u, double* conc, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_stream_collide_m", fluid, &fl)) return rc;
  return ade_stream_collide(fl.kbc ? "lbm_ade_stream_collide_m" : "lbm_ade_stream_collide_w", fn, gn, fo, go, g, bc, fl, scalar,
                            sbc, nullptr, iwalls, row_begin, row_end, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_mb(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                              const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                              const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                              int row_begin, int row_end, double* rho, double* u, double* conc, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_stream_collide_mb", fluid, &fl)) return rc;
  return ade_stream_collide(fl.kbc ? "lbm_ade_stream_collide_mb" : "lbm_ade_stream_collide_w", fn, gn, fo, go, g, bc, fl, scalar,
                            sbc, buoy, iwalls, row_begin, row_end, rho, u, conc, as_stream(s));
}

int lbm_ade_stream_collide_part_m(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                  const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_iwalls* iwalls, int part, int edge_rows,
                                  double* rho, double* u, double* conc, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_stream_collide_part_m", fluid, &fl)) return rc;
  return ade_part(fl.kbc ? "lbm_ade_stream_collide_part_m" : "lbm_ade_stream_collide_part_w", fn, gn, fo, go, g, bc, fl, scalar,
                  sbc, nullptr, iwalls, part, edge_rows, rho, u, conc, as_stream(s));
}

// lbm_ade_stream_collide_part_m with the descriptor of lbm_ade_buoyancy after sbc (the name: lbm_hip.h)
int lbm_ade_slab_stream_collide_mb(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                   const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                                   const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                                   int part, int edge_rows, double* rho, double* u, double* conc, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_slab_stream_collide_mb", fluid, &fl)) return rc;
  return ade_part(fl.kbc ? "lbm_ade_slab_stream_collide_mb" : "lbm_ade_stream_collide_part_w", fn, gn, fo, go, g, bc, fl, scalar,
                  sbc, buoy, iwalls, part, edge_rows, rho, u, conc, as_stream(s));
}

long long lbm_ade_part_launches(void) { return g_part_launches.load(std::memory_order_relaxed); }

// the open table of a context under the caller's name; kbc_ok: the entry serves a KBC context (the `_m` one).  The refusal
// of a KBC context comes before everything else, the table the context already holds included
static int ade_solver_set_open(const char* fn, bool kbc_ok, lbm_ade_solver* sv, const lbm_ade_open* open) {
  LBM_REQUIRE(sv, "%s: NULL solver", fn);
  LBM_REQUIRE(kbc_ok || sv->model != LBM_MODEL_KBC || !open || open->nodes.empty(),
              "%s: open boundaries (a table of %d nodes) are not supported with a KBC fluid", fn,
              open ? (int)open->nodes.size() : 0);
  if (open == sv->open) return LBM_OK;
  if (open) {
    LBM_REQUIRE(!open->view, "%s: open boundaries: the table is a slab view (lbm_ade_open_slab): the context runs a single "
                "block and takes the global table", fn);
    LBM_REQUIRE(open->finalized, "%s: open boundaries: the table is not finalized (lbm_ade_open_finalize)", fn);
    LBM_REQUIRE(open->R == sv->g.R && open->C == sv->g.C, "%s: open boundaries: the table is for a %d x %d lattice, the call for %d x %d",
                fn, open->R, open->C, sv->g.R, sv->g.C);
    LBM_REQUIRE(open->n == 0 || !sv->post, "%s: the state is post-collision: the carried velocity of a new table cannot be formed "
                "(set it before the first step or before lbm_ade_solver_set_state)", fn);
  }
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));  // nothing in flight reads the old carries
  for (double*& p : sv->carry) {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  sv->open = nullptr;
  if (open && open->n > 0) {
    const size_t bytes = 2 * (size_t)open->n * sizeof(double);
    hipError_t e = hipMalloc(&sv->carry[0], bytes);
    if (e == hipSuccess) e = hipMalloc(&sv->carry[1], bytes);
    if (e == hipSuccess) e = hipMemsetAsync(sv->carry[0], 0, bytes, sv->st);
    if (e == hipSuccess) e = hipMemsetAsync(sv->carry[1], 0, bytes, sv->st);
    if (e != hipSuccess) {
      set_error("%s: %s", fn, hipGetErrorString(e));
      return LBM_ERR_HIP;
    }
    if (!sv->post)  // a state set before the table: its carry
      if (int rc = ade_open_prime(make_geom(sv->g), open->d_nodes, open->n, sv->f(sv->cur), sv->carry[sv->cur], sv->st)) return rc;
  }
  sv->open = open;
  return LBM_OK;
}

int lbm_ade_solver_set_open(lbm_ade_solver* sv, const lbm_ade_open* open) {
  return ade_solver_set_open("lbm_ade_solver_set_open", false, sv, open);
}

// a BGK context: the call above, under its name
int lbm_ade_solver_set_open_m(lbm_ade_solver* sv, const lbm_ade_open* open) {
  const bool kbc = sv && sv->model == LBM_MODEL_KBC;
  return ade_solver_set_open(kbc ? "lbm_ade_solver_set_open_m" : "lbm_ade_solver_set_open", true, sv, open);
}

// lbm_ade_collide_o / lbm_ade_stream_collide_o with the fluid by model; model = BGK: those calls under their names
int lbm_ade_open_collide_m(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                           const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                           const lbm_ade_buoyancy* buoy, const lbm_ade_open* open, double* carry_out, double* rho, double* u,
                           double* conc, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_open_collide_m", fluid, &fl)) return rc;
  return ade_collide(fl.kbc ? "lbm_ade_open_collide_m" : "lbm_ade_collide_o", fp, gp, f, g_in, g, bc, fl, scalar, sbc, buoy,
                     nullptr, rho, u, conc, as_stream(s), open, carry_out);
}

int lbm_ade_open_stream_collide_m(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                  const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                                  const lbm_ade_open* open, const double* carry_in, double* carry_out, int row_begin,
                                  int row_end, double* rho, double* u, double* conc, lbm_stream_t s) {
  AdeFluid fl;
  if (int rc = ade_fluid_model("lbm_ade_open_stream_collide_m", fluid, &fl)) return rc;
  return ade_stream_collide(fl.kbc ? "lbm_ade_open_stream_collide_m" : "lbm_ade_stream_collide_o", fn, gn, fo, go, g, bc, fl,
                            scalar, sbc, buoy, iwalls, row_begin, row_end, rho, u, conc, as_stream(s), nullptr, open, carry_in,
                            carry_out);
}

}  // extern "C"
