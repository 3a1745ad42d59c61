// C ABI, part 5: colour-gradient two-phase MRT step (test/mrtcg_rayleigh_taylor.cpp).
#include <new>

#include "cg.hpp"
#include "cg_fused.hpp"
#include "launch.hpp"

// ---- solver context for the two-phase driver loop (its functions: below) ------------------------------------------
// two steps per pass (experiments build, cg_solver_step2): the frame of the lattice advances two single steps on two small
// lattices -- row band: rows [0, HB) and [R - HB, R) x all columns; column band: all rows x columns [0, WB) and [C - WB, C)
// -- on a helper stream.  Made on first use; empty in the default build.
struct CgTwoStepBands {
  double* rband[2][2] = {};  // [buffer][colour]
  double* cband[2][2] = {};
  lbm_geom rbg{}, cbg{};
  lbm::SideStream side;
  void release() {
    side.destroy();
    for (int b = 0; b < 2; ++b)
      for (int k = 0; k < 2; ++k) {
        if (rband[b][k]) (void)hipFree(rband[b][k]);
        if (cband[b][k]) (void)hipFree(cband[b][k]);
      }
  }
};
struct lbm_cg_solver {
  lbm_geom g;
  lbm_bc bc;
  lbm_cg_params prm;
  hipStream_t st;
  double* lat[2][2];  // [buffer][colour]
  double *rho_r, *rho_b, *u, *psi, *snu, *stage;
  int cur;
  bool post;
  long steps;
  CgTwoStepBands x2;
  long pair_launches;  // passes that took two steps
};

namespace lbm {

__global__ __launch_bounds__(256) void k_cg_equilibrium(double* __restrict__ f,
                                                        const double* __restrict__ rho_k,
                                                        const double* __restrict__ u, long n,
                                                        long plane, CgColour k) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    double e[Q];
    cg_feq(e, rho_k[i], k, u[i], u[n + i]);
#pragma unroll
    for (int q = 0; q < Q; ++q) f[q * plane + i] = e[q];
  }
}

// stand-alone differential::x / ::y (src/differential.cpp:23-33): 5x5 cross-correlation with
// replicate padding; dir 0 = d/d(row) ("x"), 1 = d/d(col) ("y").  Same tap order as the fused
// collide kernel.  Not on the hot path (the fused step reads its stencils from LDS).
__global__ __launch_bounds__(256) void k_diff5(double* __restrict__ out,
                                               const double* __restrict__ psi, int R, int C, int dir) {
  const long n = (long)R * C;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int r = (int)(idx / C), c = (int)(idx % C);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const double w = ((1.0 / 5040.0) * cg_xi(i, j)) * (double)(dir == 0 ? i - 2 : j - 2);
        int rr = r + i - 2, cc = c + j - 2;
        rr = rr < 0 ? 0 : (rr > R - 1 ? R - 1 : rr);
        cc = cc < 0 ? 0 : (cc > C - 1 ? C - 1 : cc);
        s += w * psi[(long)rr * C + cc];
      }
    out[idx] = s;
  }
}

static int check_cg(const char* fn, const lbm_geom* g, const lbm_bc* bc, const lbm_cg_params* p) {
  int rc = validate_geom_bc(fn, g, bc);
  if (rc) return rc;
  LBM_REQUIRE(p, "%s: NULL params", fn);
  LBM_REQUIRE(g->ghost == 0 || g->ghost == 3, "%s: ghost=%d (the two-phase step needs 0 or 3 ghost rows)", fn, g->ghost);
  LBM_REQUIRE(p->red.rho_0 > 0 && p->blue.rho_0 > 0 && p->delta > 0, "%s: bad colour parameters", fn);
  LBM_REQUIRE(p->red.alpha < 1.0 && p->blue.alpha < 1.0, "%s: alpha must be < 1", fn);
  LBM_REQUIRE(p->form >= LBM_FORM_DEFAULT && p->form <= LBM_FORM_REASSOCIATED, "%s: form=%d (LBM_FORM_*)", fn, p->form);
  return LBM_OK;
}

static int launch_cg_collide(bool from_post, double* pn_r, double* pn_b, const double* in_r,
                             const double* in_b, const double* rho_r, const double* rho_b,
                             const double* u, const lbm_geom* lg, const lbm_bc* lbc,
                             const lbm_cg_params* prm, double* psi, double* snu, int row_begin,
                             int row_end, hipStream_t st) {
  const Geom g = make_geom(*lg);
  const Bc bc = make_bc(lbc);
  const CgConsts cc = make_cg_consts(*prm);
  const MacroIdx mi = make_macro_idx(g);
  LBM_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= g.R, "lbm_cg: row range [%d, %d) outside [0, %d)", row_begin, row_end, g.R);
  if (row_begin == row_end) return LBM_OK;
  const int tiles = ((row_end - row_begin + CG_TR - 1) / CG_TR) * ((g.C + CG_TC - 1) / CG_TC);
  with_flags([&](auto POST, auto FIELDS) {
    LBM_KLAUNCH((k_cg_collide<POST(), FIELDS()>), dim3(tiles), dim3(256), 0, st, pn_r, pn_b, in_r, in_b, rho_r, rho_b, u, g, bc, cc, psi, snu, mi, row_begin, row_end);
  }, from_post, psi != nullptr);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

static thread_local int g_last_inner_form = -1;  // lbm_cg_last_inner_form

// what every launch of one fused two-phase step takes: the lattices, the geometry and constants, the five field outputs
// (all or none: the launches write psi, s_nu and the moments) and the row range
struct CgStepArgs {
  double *pn_r, *pn_b;
  const double *in_r, *in_b;
  const Geom& g;
  const Bc& bc;
  const CgFast& cf;
  double *rho_r, *rho_b, *u, *psi, *snu;
  const MacroIdx& mi;
  int row_begin, row_end;
};

#ifdef LBM_EXPERIMENTS  // every launch form that was measured and not kept, behind three hooks: csrc/experiments/cg_launch.hpp
#include "experiments/cg_launch.hpp"
#else
constexpr bool kCgExperiments = false;
#endif

// the inner rectangle of a split launch (cg_plan.hpp), on `st`; the caller reads the launch's status
template <int TR, int TC, int WAVES>
static void launch_cg_inner(const CgStepArgs& a, const CgPlan& p, int xs, hipStream_t st) {
  const Geom& g = a.g;
  const bool fields = a.psi != nullptr;
  const int ra = a.row_begin + p.rc.ir0 * TR, rb = a.row_begin + p.rc.ir1 * TR, ca = p.rc.ic0 * TC, cb = p.rc.ic1 * TC;
  if (p.n_btr && p.shape == 2) {  // k_cg_tile_mn: 16 x 64 big tiles, 2 nodes per thread, the second parked in LDS
    // patches of 4 x 2 tiles per XCD (100 PR + PC): ring rows and ring columns inside a patch are hits of one L2.  Larger
    // patches read less and less (4.09 GB per step with pairs of column neighbours, 3.99 with 4 x 2, 3.90 with 8 x 2, 3.73 with
    // 8 x 4) but the rate the memory system delivers falls with them on some boxes: 4 x 2 is the order that is never slower
    // than the pairs (+3.6 %, +0.4 %, +0.2 % on three boxes; 8 x 2: +4.7 %, -0.3 %, -2.9 %), profiles/r04_cg_order_pmc.txt
    g_last_inner_form = 102;
    with_flags([&](auto PSI) { LBM_KLAUNCH((k_cg_tile_mn<16, 64, 512, 4, true, PSI()>), dim3(p.n_btr * p.n_btc), dim3(512), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, g, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, ra, ca, p.n_btc, p.big_xcd); }, fields);
    return;
  }
  // "cg_strip2" = 41 .. 47: k_cg_walk -- a workgroup of TR x WC waves walking down a strip of 64 WC - 4 columns, TR rows a step
  const int sw4 = p.n_btr ? 0 : tuning("cg_strip2", 0);
  if (sw4 >= 41 && sw4 <= 47 && ca >= 4 && 9.0 * (double)g.plane * 8.0 < 4.0e9) {  // 32-bit plane offsets
    static const int shapes[7][2] = {{4, 1}, {6, 1}, {2, 2}, {3, 2}, {2, 3}, {2, 1}, {3, 1}};
    const int wtr = shapes[sw4 - 41][0], wc = shapes[sw4 - 41][1], outc = 64 * wc - 4;
    const int strips = (cb - ca + outc - 1) / outc;
    int rpc = tuning("cg_rows2", 0);
    // chunks of 128 rows: several rounds of workgroups, dispatched as slots free up.  One round of long chunks (every
    // workgroup resident at once) is 6-8 % slower on six boxes of nine: a static partition ends with its slowest workgroup
    if (rpc <= 0) rpc = 128;
    rpc = (rpc + wtr - 1) / wtr * wtr;
    if (rpc > rb - ra) rpc = rb - ra;
    const int chunks = (rb - ra + rpc - 1) / rpc, nb = strips * chunks, grid = (nb + 7) / 8 * 8;
    const int xo = tuning("cg_walk_xcd", 1);
    g_last_inner_form = sw4;
#define LBM_CG_WALK(WTR, WWC, PF)                                                                                      \
    with_flags([&](auto PSI) { LBM_KLAUNCH((k_cg_walk<WTR, WWC, PSI(), PF>), dim3(grid), dim3(WTR * WWC * 64), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, g, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, ra, rb, ca, cb, rpc, strips, nb, xo); }, fields);
    switch (sw4) {
      case 41:
        if (tuning("cg_walk_pf", 1) == 0) { LBM_CG_WALK(4, 1, false) }  // the 4 x 1 block without prefetch, 4 waves per SIMD
        else { LBM_CG_WALK(4, 1, true) }
        break;
      case 42: LBM_CG_WALK(6, 1, true) break;
      case 43: LBM_CG_WALK(2, 2, true) break;
      case 44: LBM_CG_WALK(3, 2, true) break;
      case 45: LBM_CG_WALK(2, 3, true) break;
      case 46: LBM_CG_WALK(2, 1, true) break;
      default: LBM_CG_WALK(3, 1, true) break;
    }
#undef LBM_CG_WALK
    return;
  }
#ifdef LBM_EXPERIMENTS
  if (cg_exp_inner(a, p, ra, rb, ca, cb, st)) return;
#endif
  with_flags([&](auto PSI) { LBM_KLAUNCH((k_cg_fused<TR, TC, WAVES, PSI(), 1>), dim3(p.inner), dim3(TR * TC), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, g, a.bc, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, a.row_begin, a.row_end, xs, p.rc); }, fields);
}

// part 0: the whole row range (frame beside the inner launch on a helper stream); FRAME / INNER: ONLY the frame -- widened to
// every node of the first and last `edge_rows` rows of the range -- / ONLY the inner rectangle, on `st`: a slab runs the
// two on two streams and sends its edge rows while the inner launch is still busy (lbm_cg_step_fused_part)
template <int TR, int TC, int WAVES>
static int launch_cg_fused_t(const CgStepArgs& a, hipStream_t st, int part = 0, int edge_rows = 0) {
  const Geom& g = a.g;
  const bool fields = a.psi != nullptr;
  const int xs = tuning("cg_xcd", 2);  // pairs of column-neighbour tiles per XCD: +5 % at 4 waves per SIMD
  const CgPlanKnobs knobs{tuning("cg_split", 1), tuning("cg_big", 2), tuning("cg_big_xcd", 402), kCgExperiments};
  const CgPlan p = cg_plan({TR, TC, g.R, g.C, g.ghost, a.bc.row_lo == LBM_EDGE_HALO, a.bc.row_hi == LBM_EDGE_HALO, a.row_begin, a.row_end, part, edge_rows}, knobs);
#ifdef LBM_EXPERIMENTS
  if (const int e = cg_exp_one_launch<TR, TC, WAVES>(a, p, part, xs, st); e != kCgNotMine) return e;
#endif
  g_last_inner_form = 0;
  if (!p.split) {
    if (part == LBM_CG_PART_INNER) return LBM_OK;  // no inner rectangle: the frame part runs every tile
    with_flags([&](auto PSI) { LBM_KLAUNCH((k_cg_fused<TR, TC, WAVES, PSI()>), dim3(p.tiles_r * p.tiles_c), dim3(TR * TC), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, g, a.bc, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, a.row_begin, a.row_end, xs); }, fields);
    LBM_CHECK_LAUNCH();
    return LBM_OK;
  }
  // the frame (3-4 % of the tiles, latency-bound: 63 us on its own) goes FIRST and on the helper stream, so
  // that it runs beside the inner launch instead of behind it (fork / join through two events, launch.hpp)
  SideStream* sd = !part && p.frame > 0 && tuning("cg_frame_beside", 1) ? sw_side_stream() : nullptr;
  if (sd && !sd->try_fork(st)) sd = nullptr;
  hipStream_t fs = sd ? sd->st : st;
  auto launched = [&]() -> int {  // the last launch's status; main waits for the helper stream whatever it is
    LBM_CHECK_LAUNCH();
    return LBM_OK;
  };
  if (p.frame > 0 && part != LBM_CG_PART_INNER) {
    with_flags([&](auto PSI) { LBM_KLAUNCH((k_cg_fused<TR, TC, WAVES, PSI(), 2>), dim3(p.frame), dim3(TR * TC), 0, fs, a.pn_r, a.pn_b, a.in_r, a.in_b, g, a.bc, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, a.row_begin, a.row_end, 0, p.rc); }, fields);
    if (const int e = launched()) return sd ? sd->join(st, e) : e;
  }
  if (part == LBM_CG_PART_FRAME) return LBM_OK;
  launch_cg_inner<TR, TC, WAVES>(a, p, xs, st);
  const int e = launched();
  return sd ? sd->join(st, e) : e;
}

}  // namespace lbm

using namespace lbm;

extern "C" {

int lbm_diff5(double* out, const double* psi, int R, int C, int dir, lbm_stream_t s) {
  LBM_REQUIRE(out && psi && out != psi && R > 0 && C > 0 && (dir == 0 || dir == 1), "lbm_diff5: bad argument");
  const long n = (long)R * C;
  LBM_KLAUNCH(k_diff5, dim3(capped_grid((n + 255) / 256)), dim3(256), 0, as_stream(s), out, psi, R, C, dir);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

void lbm_cg_default_bc(lbm_bc* bc) {
  // apply_boundary_conditions, mrtcg_rayleigh_taylor.cpp:495-533
  if (!bc) return;
  *bc = lbm_bc{LBM_EDGE_BOUNCE_BACK, LBM_EDGE_BOUNCE_BACK, LBM_EDGE_WRAP_NOSHIFT,
               LBM_EDGE_WRAP_NOSHIFT, 0, 1.0, 1.0, 0.0, 0.0};
}

int lbm_cg_equilibrium(double* f, const double* rho_k, const double* u, const lbm_cg_colour* k,
                       int R, int C, long long plane_stride, lbm_stream_t s) {
  LBM_REQUIRE(f && rho_k && u && k && R > 0 && C > 0, "lbm_cg_equilibrium: bad argument");
  lbm_cg_params p{*k, *k, 0.0, 0.0, 0.0, 0, 0.1};
  const CgConsts cc = make_cg_consts(p);
  const long n = (long)R * C;
  LBM_REQUIRE(plane_stride == 0 || plane_stride >= n, "lbm_cg_equilibrium: plane_stride too small");
  LBM_KLAUNCH(k_cg_equilibrium, dim3(capped_grid((n + 255) / 256)), dim3(256), 0, as_stream(s), f,
              rho_k, u, n, plane_stride ? (long)plane_stride : n, cc.k[0]);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

int lbm_cg_collide(double* p_r, double* p_b, const double* f_r, const double* f_b,
                   const double* rho_r, const double* rho_b, const double* u, const lbm_geom* g,
                   const lbm_bc* bc, const lbm_cg_params* prm, double* psi, double* snu,
                   lbm_stream_t s) {
  int rc = check_cg("lbm_cg_collide", g, bc, prm);
  if (rc) return rc;
  LBM_REQUIRE(p_r && p_b && f_r && f_b && rho_r && rho_b && u, "lbm_cg_collide: NULL pointer");
  LBM_REQUIRE((psi == nullptr) == (snu == nullptr), "lbm_cg_collide: psi and s_nu go together");
  return launch_cg_collide(false, p_r, p_b, f_r, f_b, rho_r, rho_b, u, g, bc, prm, psi, snu, 0, g->R, as_stream(s));
}

int lbm_cg_stream_moments(double* rho_r, double* rho_b, double* u, const double* p_r,
                          const double* p_b, const lbm_geom* g, const lbm_bc* bc,
                          const lbm_cg_params* prm, lbm_stream_t s) {
  int rc = check_cg("lbm_cg_stream_moments", g, bc, prm);
  if (rc) return rc;
  LBM_REQUIRE(rho_r && rho_b && u && p_r && p_b, "lbm_cg_stream_moments: NULL pointer");
  const Geom gg = make_geom(*g);
  const Bc bb = make_bc(bc);
  const int lo = cg_row_lo(gg, bb), hi = cg_row_hi(gg, bb) + 1;  // incl. the macro ghost rows of a slab
  const long n = (long)(hi - lo) * gg.C;
  LBM_KLAUNCH(k_cg_stream_moments, dim3(capped_grid((n + 255) / 256, 8192)), dim3(256), 0, as_stream(s),
              rho_r, rho_b, u, p_r, p_b, gg, bb, prm->gravity_r, prm->gravity_c, make_macro_idx(gg), lo, hi);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

int lbm_cg_stream_collide(double* pn_r, double* pn_b, const double* p_r, const double* p_b,
                          const double* rho_r, const double* rho_b, const double* u,
                          const lbm_geom* g, const lbm_bc* bc, const lbm_cg_params* prm,
                          int row_begin, int row_end, double* psi, double* snu, lbm_stream_t s) {
  int rc = check_cg("lbm_cg_stream_collide", g, bc, prm);
  if (rc) return rc;
  LBM_REQUIRE(pn_r && pn_b && p_r && p_b && rho_r && rho_b && u, "lbm_cg_stream_collide: NULL pointer");
  LBM_REQUIRE(pn_r != p_r && pn_b != p_b, "lbm_cg_stream_collide: aliased lattices");
  LBM_REQUIRE((psi == nullptr) == (snu == nullptr), "lbm_cg_stream_collide: psi and s_nu go together");
  return launch_cg_collide(true, pn_r, pn_b, p_r, p_b, rho_r, rho_b, u, g, bc, prm, psi, snu, row_begin, row_end, as_stream(s));
}

static int cg_step_fused(double* pn_r, double* pn_b, const double* p_r, const double* p_b,
                         const lbm_geom* g, const lbm_bc* bc, const lbm_cg_params* prm, int row_begin,
                         int row_end, double* rho_r, double* rho_b, double* u, double* psi, double* snu,
                         lbm_stream_t s, int part, int edge_rows) {
  int rc = check_cg("lbm_cg_step_fused", g, bc, prm);
  if (rc) return rc;
  LBM_REQUIRE(pn_r && pn_b && p_r && p_b, "lbm_cg_step_fused: NULL lattice");
  LBM_REQUIRE(pn_r != p_r && pn_b != p_b, "lbm_cg_step_fused: aliased lattices");
  const bool any = rho_r || rho_b || u || psi || snu, all = rho_r && rho_b && u && psi && snu;
  LBM_REQUIRE(any == all, "lbm_cg_step_fused: the five field outputs go together (all or none)");
  const Geom gg = make_geom(*g);
  const Bc bb = make_bc(bc);
  LBM_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= gg.R, "lbm_cg_step_fused: row range [%d, %d) outside [0, %d)", row_begin, row_end, gg.R);
  if (row_begin == row_end) return LBM_OK;
  const CgFast cf = make_cg_fast(make_cg_consts(*prm));
  const MacroIdx mi = make_macro_idx(gg);
  const CgStepArgs a{pn_r, pn_b, p_r, p_b, gg, bb, cf, rho_r, rho_b, u, psi, snu, mi, row_begin, row_end};
  hipStream_t st = as_stream(s);
  switch (tuning("cg_tile", 4)) {  // default: 16x32 tiles budgeted for 4 waves per SIMD (128 VGPRs)
    case 0: return launch_cg_fused_t<8, 32, 1>(a, st);
    case 2: return launch_cg_fused_t<8, 64, 1>(a, st);
    case 3: return launch_cg_fused_t<16, 32, 3>(a, st);
    case 1: return launch_cg_fused_t<16, 32, 1>(a, st);
    case 5: return launch_cg_fused_t<32, 32, 4>(a, st);
    case 6: return launch_cg_fused_t<16, 64, 4>(a, st);
    default: return launch_cg_fused_t<16, 32, 4>(a, st, part, edge_rows);
  }
}

int lbm_cg_step_fused(double* pn_r, double* pn_b, const double* p_r, const double* p_b,
                      const lbm_geom* g, const lbm_bc* bc, const lbm_cg_params* prm, int row_begin,
                      int row_end, double* rho_r, double* rho_b, double* u, double* psi, double* snu,
                      lbm_stream_t s) {
  return cg_step_fused(pn_r, pn_b, p_r, p_b, g, bc, prm, row_begin, row_end, rho_r, rho_b, u, psi, snu, s, 0, 0);
}

int lbm_cg_step_fused_part(double* pn_r, double* pn_b, const double* p_r, const double* p_b,
                           const lbm_geom* g, const lbm_bc* bc, const lbm_cg_params* prm, int part,
                           int edge_rows, double* rho_r, double* rho_b, double* u, double* psi, double* snu,
                           lbm_stream_t s) {
  LBM_REQUIRE(part == LBM_CG_PART_FRAME || part == LBM_CG_PART_INNER, "lbm_cg_step_fused_part: part=%d (LBM_CG_PART_FRAME / _INNER)", part);
  LBM_REQUIRE(g && edge_rows >= 0 && 2 * edge_rows <= g->R, "lbm_cg_step_fused_part: edge_rows=%d", edge_rows);
  LBM_REQUIRE(tuning("cg_tile", 4) == 4, "lbm_cg_step_fused_part: needs the default tile kernel (\"cg_tile\" = 4)");
  return cg_step_fused(pn_r, pn_b, p_r, p_b, g, bc, prm, 0, g->R, rho_r, rho_b, u, psi, snu, s, part, edge_rows);
}

}  // extern "C"

// ---- solver context for the two-phase driver loop (lbm_cg_solver: at the top of the file) ------------------------
extern "C" {

int lbm_cg_solver_create(lbm_cg_solver** out, const lbm_geom* g, const lbm_bc* bc,
                         const lbm_cg_params* prm, lbm_stream_t s) {
  LBM_REQUIRE(out, "lbm_cg_solver_create: NULL out pointer");
  lbm_bc dflt;
  lbm_cg_default_bc(&dflt);
  int rc = check_cg("lbm_cg_solver_create", g, bc ? bc : &dflt, prm);
  if (rc) return rc;
  lbm_cg_solver* sv = new (std::nothrow) lbm_cg_solver();
  LBM_REQUIRE(sv, "lbm_cg_solver_create: out of host memory");
  sv->g = *g;
  sv->bc = bc ? *bc : dflt;
  sv->prm = *prm;
  sv->st = as_stream(s);
  sv->cur = 0;
  sv->post = false;
  sv->steps = 0;
  sv->pair_launches = 0;
  const size_t n = (size_t)g->R * g->C;
  // the solver's own lattices: rows padded off a power-of-two stride (lbm_default_row_pitch), planes likewise.  Everything
  // that reads or writes them takes &sv->g; the macroscopic fields and the host-side AoS arrays stay dense.
  const int pitch = lbm_default_row_pitch(g->C);
  sv->g.row_pitch = pitch > g->C ? pitch : 0;
  sv->g.plane_stride = (long long)g->R * pitch + lbm_default_plane_pad(g->R, pitch);
  const size_t lat_bytes = (size_t)sv->g.plane_stride * 9 * sizeof(double);
  double** all[] = {&sv->lat[0][0], &sv->lat[0][1], &sv->lat[1][0], &sv->lat[1][1], &sv->rho_r,
                    &sv->rho_b, &sv->u, &sv->psi, &sv->snu, &sv->stage};
  const size_t bytes[] = {lat_bytes, lat_bytes, lat_bytes, lat_bytes, n * 8, n * 8, n * 16, n * 8, n * 8, n * 72};
  for (auto p : all) *p = nullptr;
  for (int i = 0; i < 10; ++i) {
    hipError_t e = hipMalloc(all[i], bytes[i]);
    if (e != hipSuccess) {
      set_error("lbm_cg_solver_create: hipMalloc failed: %s", hipGetErrorString(e));
      lbm_cg_solver_destroy(sv);
      return LBM_ERR_HIP;
    }
  }
  LBM_CHECK_HIP(hipMemsetAsync(sv->psi, 0, n * 8, sv->st));  // phase_field / s_nu start as zeros (:380,:382)
  LBM_CHECK_HIP(hipMemsetAsync(sv->snu, 0, n * 8, sv->st));
  *out = sv;
  return LBM_OK;
}

int lbm_cg_solver_destroy(lbm_cg_solver* sv) {
  if (!sv) return LBM_OK;
  sv->x2.release();
  for (double* p : {sv->lat[0][0], sv->lat[0][1], sv->lat[1][0], sv->lat[1][1], sv->rho_r, sv->rho_b,
                    sv->u, sv->psi, sv->snu, sv->stage})
    if (p) (void)hipFree(p);
  delete sv;
  return LBM_OK;
}

// host AoS state in the reference's shapes: f_r, f_b [R][C][9] (adv_f), rho_r, rho_b [R][C], u [R][C][2]
int lbm_cg_solver_set_state(lbm_cg_solver* sv, const double* f_r, const double* f_b,
                            const double* rho_r, const double* rho_b, const double* u) {
  LBM_REQUIRE(sv && f_r && f_b && rho_r && rho_b && u, "lbm_cg_solver_set_state: NULL argument");
  const int R = sv->g.R, C = sv->g.C;
  const size_t n = (size_t)R * C;
  const double* fs[2] = {f_r, f_b};
  for (int k = 0; k < 2; ++k) {
    LBM_CHECK_HIP(hipMemcpyAsync(sv->stage, fs[k], n * 72, hipMemcpyHostToDevice, sv->st));
    int rc = lbm_aos_to_soa_pitched(sv->lat[sv->cur][k], sv->stage, R, C, 9, sv->g.plane_stride, sv->g.row_pitch, sv->st);
    if (rc) return rc;
  }
  LBM_CHECK_HIP(hipMemcpyAsync(sv->rho_r, rho_r, n * 8, hipMemcpyHostToDevice, sv->st));
  LBM_CHECK_HIP(hipMemcpyAsync(sv->rho_b, rho_b, n * 8, hipMemcpyHostToDevice, sv->st));
  LBM_CHECK_HIP(hipMemcpyAsync(sv->stage, u, n * 16, hipMemcpyHostToDevice, sv->st));
  int rc = lbm_aos_to_soa(sv->u, sv->stage, R, C, 2, sv->st);
  if (rc) return rc;
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));
  sv->post = false;
  return LBM_OK;
}

long long lbm_cg_solver_pair_launches(const lbm_cg_solver* sv) { return sv ? sv->pair_launches : -1; }
int lbm_cg_last_inner_form(void) { return lbm::g_last_inner_form; }

int lbm_cg_solver_step(lbm_cg_solver* sv, int n_steps) {
  LBM_REQUIRE(sv && n_steps >= 0, "lbm_cg_solver_step: bad argument");
  const bool fused = sv->prm.form == LBM_FORM_DEFAULT ? tuning("cg_fused", 1) != 0 : sv->prm.form == LBM_FORM_REASSOCIATED;
  for (int i = 0; i < n_steps; ++i) {
#ifdef LBM_EXPERIMENTS
    if (const int e = cg_exp_two_steps(sv, fused, n_steps - i); e != kCgNotMine) {  // one pass took two steps
      if (e) return e;
      ++i;
      continue;
    }
#endif
    double** src = sv->lat[sv->cur];
    double** dst = sv->lat[sv->cur ^ 1];
    int rc;
    if (!sv->post) {  // iteration on the given (rho, u): the driver's first pass through :431-464
      rc = lbm_cg_collide(dst[0], dst[1], src[0], src[1], sv->rho_r, sv->rho_b, sv->u, &sv->g,
                          &sv->bc, &sv->prm, sv->psi, sv->snu, sv->st);
    } else if (fused) {
      // one launch per step; the observable fields are written by the last step of the call
      const bool last = (i == n_steps - 1);
      rc = lbm_cg_step_fused(dst[0], dst[1], src[0], src[1], &sv->g, &sv->bc, &sv->prm, 0, sv->g.R,
                             last ? sv->rho_r : nullptr, last ? sv->rho_b : nullptr,
                             last ? sv->u : nullptr, last ? sv->psi : nullptr,
                             last ? sv->snu : nullptr, sv->st);
    } else {
      rc = lbm_cg_stream_moments(sv->rho_r, sv->rho_b, sv->u, src[0], src[1], &sv->g, &sv->bc,
                                 &sv->prm, sv->st);
      if (rc) return rc;
      rc = lbm_cg_stream_collide(dst[0], dst[1], src[0], src[1], sv->rho_r, sv->rho_b, sv->u,
                                 &sv->g, &sv->bc, &sv->prm, 0, sv->g.R, sv->psi, sv->snu, sv->st);
    }
    if (rc) return rc;
    sv->cur ^= 1;
    sv->post = true;
    ++sv->steps;
  }
  return LBM_OK;
}

// State as the reference holds it after its loop ran: adv_f of both colours, rho_r, rho_b, u
// (all refreshed from the streamed populations, :466-477) and the last psi / s_nu.
// Any output pointer may be NULL.
int lbm_cg_solver_get_state(lbm_cg_solver* sv, double* f_r, double* f_b, double* rho_r,
                            double* rho_b, double* u, double* psi, double* snu) {
  LBM_REQUIRE(sv, "lbm_cg_solver_get_state: NULL solver");
  const int R = sv->g.R, C = sv->g.C;
  const size_t n = (size_t)R * C;
  double* fo[2] = {f_r, f_b};
  double* scratch = sv->lat[sv->cur ^ 1][0];
  for (int k = 0; k < 2; ++k) {
    if (!fo[k]) continue;
    const double* src = sv->lat[sv->cur][k];
    if (sv->post) {
      int rc = lbm_stream(scratch, src, &sv->g, &sv->bc, sv->st);
      if (rc) return rc;
      src = scratch;
    }
    int rc = lbm_soa_to_aos_pitched(sv->stage, src, R, C, 9, sv->g.plane_stride, sv->g.row_pitch, sv->st);
    if (rc) return rc;
    LBM_CHECK_HIP(hipMemcpyAsync(fo[k], sv->stage, n * 72, hipMemcpyDeviceToHost, sv->st));
    LBM_CHECK_HIP(hipStreamSynchronize(sv->st));
  }
  if (rho_r || rho_b || u) {
    if (sv->post) {
      int rc = lbm_cg_stream_moments(sv->rho_r, sv->rho_b, sv->u, sv->lat[sv->cur][0],
                                     sv->lat[sv->cur][1], &sv->g, &sv->bc, &sv->prm, sv->st);
      if (rc) return rc;
    }
    if (rho_r) LBM_CHECK_HIP(hipMemcpyAsync(rho_r, sv->rho_r, n * 8, hipMemcpyDeviceToHost, sv->st));
    if (rho_b) LBM_CHECK_HIP(hipMemcpyAsync(rho_b, sv->rho_b, n * 8, hipMemcpyDeviceToHost, sv->st));
    if (u) {
      int rc = lbm_soa_to_aos(sv->stage, sv->u, R, C, 2, sv->st);
      if (rc) return rc;
      LBM_CHECK_HIP(hipMemcpyAsync(u, sv->stage, n * 16, hipMemcpyDeviceToHost, sv->st));
    }
  }
  if (psi) LBM_CHECK_HIP(hipMemcpyAsync(psi, sv->psi, n * 8, hipMemcpyDeviceToHost, sv->st));
  if (snu) LBM_CHECK_HIP(hipMemcpyAsync(snu, sv->snu, n * 8, hipMemcpyDeviceToHost, sv->st));
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));
  return LBM_OK;
}

int lbm_cg_solver_sync(lbm_cg_solver* sv) {
  LBM_REQUIRE(sv, "lbm_cg_solver_sync: NULL solver");
  LBM_CHECK_HIP(hipStreamSynchronize(sv->st));
  return LBM_OK;
}

}  // extern "C"

// ---- asynchronous snapshots of the two-phase solver (reference: the [R,C,n_snap] stacks written by
// torch::save at the end of a run, mrtcg_rayleigh_taylor.cpp:481-485) ---------------------------------
// record(): rho_r, rho_b, u of the CURRENT state (pass A on the resident post-collision lattices =
// what the driver holds after the iterations run so far) -> device staging on the solver's stream
// -> pinned host on a private stream; returns at once, the solver may keep stepping.
struct lbm_cg_snapshot {
  lbm_cg_solver* sv;
  hipStream_t copy;
  hipEvent_t ready, done;
  double* d_stage;  // [rho_r | rho_b | u (AoS)] = 4 n doubles
  double* h_stage;  // pinned host, same layout
  long step;
};

extern "C" {

int lbm_cg_snapshot_destroy(lbm_cg_snapshot* sn) {
  if (!sn) return LBM_OK;
  if (sn->copy) (void)hipStreamSynchronize(sn->copy);
  if (sn->d_stage) (void)hipFree(sn->d_stage);
  if (sn->h_stage) (void)hipHostFree(sn->h_stage);
  if (sn->ready) (void)hipEventDestroy(sn->ready);
  if (sn->done) (void)hipEventDestroy(sn->done);
  if (sn->copy) (void)hipStreamDestroy(sn->copy);
  delete sn;
  return LBM_OK;
}

int lbm_cg_snapshot_create(lbm_cg_snapshot** out, lbm_cg_solver* sv) {
  LBM_REQUIRE(out && sv, "lbm_cg_snapshot_create: NULL argument");
  lbm_cg_snapshot* sn = new (std::nothrow) lbm_cg_snapshot();
  LBM_REQUIRE(sn, "lbm_cg_snapshot_create: out of host memory");
  *sn = lbm_cg_snapshot{sv, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  const size_t n = (size_t)sv->g.R * sv->g.C;
  hipError_t e = hipStreamCreateWithFlags(&sn->copy, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&sn->ready, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&sn->done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc(&sn->d_stage, n * 32);
  if (e == hipSuccess) e = hipHostMalloc(&sn->h_stage, n * 32);
  if (e != hipSuccess) {
    set_error("lbm_cg_snapshot_create: %s", hipGetErrorString(e));
    lbm_cg_snapshot_destroy(sn);
    return LBM_ERR_HIP;
  }
  *out = sn;
  return LBM_OK;
}

int lbm_cg_snapshot_record(lbm_cg_snapshot* sn) {
  LBM_REQUIRE(sn, "lbm_cg_snapshot_record: NULL snapshot");
  lbm_cg_solver* sv = sn->sv;
  const int R = sv->g.R, C = sv->g.C;
  const size_t n = (size_t)R * C;
  if (sv->post) {  // moments of the streamed state, :466-477
    int rc = lbm_cg_stream_moments(sv->rho_r, sv->rho_b, sv->u, sv->lat[sv->cur][0], sv->lat[sv->cur][1],
                                   &sv->g, &sv->bc, &sv->prm, sv->st);
    if (rc) return rc;
  }
  LBM_CHECK_HIP(hipStreamWaitEvent(sv->st, sn->done, 0));  // previous D2H of this snapshot finished
  LBM_CHECK_HIP(hipMemcpyAsync(sn->d_stage, sv->rho_r, n * 8, hipMemcpyDeviceToDevice, sv->st));
  LBM_CHECK_HIP(hipMemcpyAsync(sn->d_stage + n, sv->rho_b, n * 8, hipMemcpyDeviceToDevice, sv->st));
  int rc = lbm_soa_to_aos(sn->d_stage + 2 * n, sv->u, R, C, 2, sv->st);
  if (rc) return rc;
  LBM_CHECK_HIP(hipEventRecord(sn->ready, sv->st));
  LBM_CHECK_HIP(hipStreamWaitEvent(sn->copy, sn->ready, 0));
  LBM_CHECK_HIP(hipMemcpyAsync(sn->h_stage, sn->d_stage, n * 32, hipMemcpyDeviceToHost, sn->copy));
  LBM_CHECK_HIP(hipEventRecord(sn->done, sn->copy));
  sn->step = sv->steps;
  return LBM_OK;
}

int lbm_cg_snapshot_host(lbm_cg_snapshot* sn, const double** rho_r, const double** rho_b,
                         const double** u, long long* step) {
  LBM_REQUIRE(sn, "lbm_cg_snapshot_host: NULL snapshot");
  LBM_CHECK_HIP(hipStreamSynchronize(sn->copy));
  const size_t n = (size_t)sn->sv->g.R * sn->sv->g.C;
  if (rho_r) *rho_r = sn->h_stage;
  if (rho_b) *rho_b = sn->h_stage + n;
  if (u) *u = sn->h_stage + 2 * n;
  if (step) *step = sn->step;
  return LBM_OK;
}

int lbm_cg_snapshot_write_npy(lbm_cg_snapshot* sn, const char* rho_r_path, const char* rho_b_path,
                              const char* u_path) {
  LBM_REQUIRE(sn, "lbm_cg_snapshot_write_npy: NULL snapshot");
  LBM_CHECK_HIP(hipStreamSynchronize(sn->copy));
  const long R = sn->sv->g.R, C = sn->sv->g.C;
  const size_t n = (size_t)R * C;
  int rc = LBM_OK;
  if (rho_r_path) rc = write_npy(rho_r_path, sn->h_stage, {R, C});
  if (!rc && rho_b_path) rc = write_npy(rho_b_path, sn->h_stage + n, {R, C});
  if (!rc && u_path) rc = write_npy(u_path, sn->h_stage + 2 * n, {R, C, 2});
  return rc;
}

}  // extern "C"
