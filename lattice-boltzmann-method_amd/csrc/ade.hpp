// Fluid + transported scalar (advection-diffusion) on one block: the sediment concentration g of
// test/rectangle_sedimentation_test.cpp:88-247 carried with a compressible BGK fluid.  g is a second D2Q9
// distribution with the equilibrium solver::equilibrium(g_equi, u + w_s, C), C = calc_rho(g), u the fluid's
// velocity (:125), relaxed with its own BGK rate (:132) and streamed like f (:145).
//
// One fused pull step per node: stream both post-collision lattices (edge fix-ups included), form rho and u
// from f and C from g, collide both, write both -- 18 loads and 18 stores of 8 bytes, 288 B per node update.
#pragma once
#include "d2q9.hpp"

namespace lbm {

// The scalar half in the REFERENCE order: solver::equilibrium (solver.cpp:51-62) and solver::collision
// (:65-74) expression by expression with rho -> C and u -> (u_r + w_r, u_c + w_c); the sum u + w is formed
// first, as the driver's torch expression `u + w_s` does.  Bitwise equal to the oracle's primitives.
struct AdeModelRef {
  double omega, wr, wc;
  __device__ __forceinline__ void collide(double (&g)[Q], double ux, double uy, double& conc) const {
    double jx, jy, e[Q];
    BgkModel::moments(g, conc, jx, jy);  // calc_rho(g); the first moments are dead code
    (void)jx;
    (void)jy;
    BgkModel::feq_comp(e, conc, ux + wr, uy + wc);
#pragma unroll
    for (int q = 0; q < Q; ++q) g[q] = (1.0 - omega) * g[q] + omega * e[q];
  }
};

// The scalar half REASSOCIATED, in the style of BgkFastModel: pairwise zeroth moment, equilibrium split into
// its parts even / odd under c -> -c with omega folded into the weights, FMA contraction per expression.  No
// reciprocal: the scalar equilibrium is linear in C.  Agreement with AdeModelRef to rounding.
struct AdeFastModel {
  double keep, ow0, ow1, ow5, wr, wc;
  __host__ __device__ AdeFastModel(double om, double w_r, double w_c)
      : keep(1.0 - om), ow0(om * (4.0 / 9.0)), ow1(om * (1.0 / 9.0)), ow5(om * (1.0 / 36.0)), wr(w_r), wc(w_c) {}
  __device__ __forceinline__ void collide(double (&g)[Q], double ux, double uy, double& conc) const {
#pragma clang fp contract(on)
    conc = (g[0] + (g[1] + g[3])) + ((g[2] + g[4]) + ((g[5] + g[7]) + (g[6] + g[8])));
    const double vx = ux + wr, vy = uy + wc;
    const double us = vx + vy, ud = vx - vy;
    const double base = 1.0 - 1.5 * (vx * vx + vy * vy);
    const double r1 = ow1 * conc, r5 = ow5 * conc;
    // even part shared by a pair, the odd part joined before the scaling: BgkFastModel's order (d2q9.hpp) and its reason
    const double S1 = base + 4.5 * vx * vx, S2 = base + 4.5 * vy * vy;
    const double S5 = base + 4.5 * us * us, S6 = base + 4.5 * ud * ud;
    const double A1 = S1 + 3.0 * vx, A3 = S1 - 3.0 * vx, A2 = S2 + 3.0 * vy, A4 = S2 - 3.0 * vy;
    const double A5 = S5 + 3.0 * us, A7 = S5 - 3.0 * us, A8 = S6 + 3.0 * ud, A6 = S6 - 3.0 * ud;
    g[0] = keep * g[0] + (ow0 * conc) * base;
    g[1] = keep * g[1] + r1 * A1;
    g[3] = keep * g[3] + r1 * A3;
    g[2] = keep * g[2] + r1 * A2;
    g[4] = keep * g[4] + r1 * A4;
    g[5] = keep * g[5] + r5 * A5;
    g[7] = keep * g[7] + r5 * A7;
    g[8] = keep * g[8] + r5 * A8;
    g[6] = keep * g[6] + r5 * A6;
  }
};

// the two collisions of one node: fluid first (its u feeds the scalar's equilibrium)
template <class FM, class SM>
__device__ __forceinline__ void ade_collide_node(double (&f)[Q], double (&h)[Q], const FM& fm, const SM& sm, double& rho,
                                                 double& ux, double& uy, double& conc) {
  fm.collide(f, rho, ux, uy);
  sm.collide(h, ux, uy, conc);
}

// Buoyancy (lbm_ade_buoyancy, device copy): the scalar pushes on the fluid, per node F = (C - c_ref) (beta_r, beta_c)
// with the node's own C -- Boussinesq coupling, local, no halo and no launch of its own.  The fluid half becomes the
// body-force collision of test/gravity_test.cpp:141-160 (BgkModel's force_mode branch, expression for expression) with
// that per-node F:
//   rho = calc_rho(f), u0 = calc_u(f, rho);  the scalar's wall rule (ade_fixed_walls) with u0;  C = calc_rho(g);
//   F = ((C - c_ref) beta_r, (C - c_ref) beta_c);  u = u0 + u_shift F;  feq = equilibrium(u, rho);
//   S_q = ((1 - 0.5 omega) ((guo_a + guo_b (c_q.u)) (c_q.F) - guo_a (u.F)) w_q);  f* = f + (-omega (f - feq)) + S_q;
//   g* = AdeModelRef::collide(g, u) -- the same shifted u, w added inside.
// Per collision the force changes the momentum by (omega rho u_shift + (1 - omega / 2) guo_a / 3) F: with (u_shift,
// guo_a, guo_b) = (0.5, 3, 9) Guo's scheme up to rho ~ 1, with (1, 1/3, 1/9) the reference's.  The forced relaxation is a
// delta form, f + (-omega (f - feq)): it rounds differently from the passive (1 - omega) f + omega feq even as beta -> 0,
// which is why beta = (0, 0) takes the passive kernels instead.  Reference order only, in both halves.
struct AdeBuoyancy {
  double beta_r, beta_c, c_ref, u_shift, ga, gb;
};

// The two-node kernels hold 36 populations per lane and their passive instantiations come out at 114-128 VGPRs by
// themselves.  The buoyant ones collide and store the scalar FIRST (it needs the shifted u, not the fluid's collision),
// so that the forced collision -- more independent chains than the plain one -- runs with f alone in registers; they
// also tell the compiler the occupancy to keep: four waves per SIMD at 256 threads = 128 VGPRs.
#define LBM_ADE_WAVES(BUOYANT) __attribute__((amdgpu_waves_per_eu((BUOYANT) ? 4 : 1)))

// rho = calc_rho(f), u0 = calc_u(f, rho): BgkModel::moments and the two divisions
__device__ __forceinline__ void ade_fluid_moments(const double (&f)[Q], double& rho, double& ux, double& uy) {
  double jx, jy;
  BgkModel::moments(f, rho, jx, jy);
  ux = jx / rho;
  uy = jy / rho;
}

// F of a node from its C
__device__ __forceinline__ void ade_buoyant_force(double conc, const AdeBuoyancy& by, double& Fr, double& Fc) {
  const double dc = conc - by.c_ref;
  Fr = dc * by.beta_r;
  Fc = dc * by.beta_c;
}

// C and the shifted velocity of a buoyant node.  In: (ux, uy) = u0, h after the scalar's wall rule; out: conc =
// calc_rho(h), (ux, uy) = u0 + u_shift F -- the velocity of BOTH collisions.
__device__ __forceinline__ void ade_buoyant_shift(const double (&h)[Q], const AdeBuoyancy& by, double& ux, double& uy,
                                                  double& conc) {
  double Fr, Fc;
  conc = ((((((((h[0] + h[1]) + h[2]) + h[3]) + h[4]) + h[5]) + h[6]) + h[7]) + h[8]);  // calc_rho(g)
  ade_buoyant_force(conc, by, Fr, Fc);
  ux = ux + by.u_shift * Fr;
  uy = uy + by.u_shift * Fc;
}

// the same value, but one the compiler cannot trace back: what is formed from it is formed again, not kept in registers
__device__ __forceinline__ double ade_again(double x) {
  asm volatile("" : "+v"(x));
  return x;
}

// The fluid's collision of a buoyant node: BgkModel::collide's force_mode branch with the node's F; (ux, uy) shifted,
// conc = calc_rho(h).  rho and F are formed a second time here, from the f still in registers and from conc -- the same
// operations on the same values, so the same bits -- instead of being held across the scalar's collision: ten
// additions and four multiplications for five doubles of register file per node.
__device__ __forceinline__ void ade_buoyant_fluid(double (&f)[Q], double omega, const AdeBuoyancy& by, double& rho,
                                                  double ux, double uy, double conc) {
  double jx, jy, Fr, Fc, e[Q];
  f[0] = ade_again(f[0]);
  BgkModel::moments(f, rho, jx, jy);  // calc_rho(f); the first moments are dead code
  (void)jx;
  (void)jy;
  ade_buoyant_force(ade_again(conc), by, Fr, Fc);
  BgkModel::feq_comp(e, rho, ux, uy);
  const double uF = ux * Fr + uy * Fc;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const double cu = ux * (double)icx(q) + uy * (double)icy(q);
    const double cF = Fr * (double)icx(q) + Fc * (double)icy(q);
    const double S = ((1 - 0.5 * omega) * ((by.ga + by.gb * cu) * cF - by.ga * uF) * wq(q));
    f[q] = f[q] + (-omega * (f[q] - e[q])) + S;
  }
}

// The forced collision of a buoyant node by fluid model -- the hook of the one-node kernels below.  In: rho =
// calc_rho(f), (ux, uy) the shifted u, conc = calc_rho(h).  Any model with an `omega` (the BGK models) takes the force
// branch above; another fluid overloads this on its model type (KbcModel: ade_kbc.hpp), found by argument-dependent lookup
// where a kernel is instantiated with it.
template <class FM>
__device__ __forceinline__ void ade_forced_fluid(double (&f)[Q], const FM& fm, const AdeBuoyancy& by, double& rho,
                                                 double ux, double uy, double conc) {
  ade_buoyant_fluid(f, fm.omega, by, rho, ux, uy, conc);
}

// both collisions of one buoyant node; in: (rho, ux, uy) = ade_fluid_moments(f), h after the scalar's wall rule
// (sm.collide forms the same C again from the same h)
template <class FM, class SM>
__device__ __forceinline__ void ade_buoyant_collide(double (&f)[Q], double (&h)[Q], const FM& fm, const SM& sm,
                                                    const AdeBuoyancy& by, double& rho, double& ux, double& uy,
                                                    double& conc) {
  ade_buoyant_shift(h, by, ux, uy, conc);
  sm.collide(h, ux, uy, conc);
  ade_forced_fluid(f, fm, by, rho, ux, uy, conc);
}

// The scalar's fixed-concentration walls (lbm_ade_scalar_bc, device copy).  Edge e: 0 row_lo, 1 row_hi, 2 col_lo,
// 3 col_hi.  C_w of a node: profile[e][c] on a row edge, profile[e][r] on a column edge (rows of the lattice the launch
// sees), conc[e] where the edge has no profile.  The host checks that every FIXED edge is a wall of the fluid.
struct AdeWalls {
  int fixed;  // bit e: edge e is FIXED
  double conc[4];
  const double* profile[4];
};

// The populations of g that bounce back at a FIXED edge anti-bounce back instead (test/rectangle_sedimentation_test.cpp
// :203-232): h[qbar] = -h*[q] + 2 G_q(v, C_w), G_q = (1 + 3 c_q.v + 4.5 (c_q.v)^2 - 1.5 v.v) E_q C_w, v = u + w, in the
// driver's expression order.  On entry the slots a wall replaces hold the bounce-back gather (h[qbar] = h*[q]: a FIXED
// column gathers as BOUNCE_BACK, also beside a specular fluid column); u is the fluid velocity of the streamed f.  Slot
// ownership is bc_fixups_own's: rows first, a wall column wins at the corners, and each slot takes the rule and C_w of
// the edge that wins it (a NO_FLUX column keeps its corner slots bounce-back).
// One anti-bounce-back population: in hb the bounce-back value h*[q] of slot opp(q), out the FIXED value of that slot;
// (vr, vc) = u + w, vv = v.v, cw = C_w.  The one expression of the domain's FIXED edges (ade_fixed_walls) and of the
// interior walls (ade_iwalls_scalar).
__device__ __forceinline__ double ade_fixed_slot(double hb, int q, double vr, double vc, double vv, double cw) {
  // c_q.v as matmul(v, c) forms it (products with 0, +-1 are exact)
  const double cv = q == 1 ? vr : q == 2 ? vc : q == 3 ? -vr : q == 4 ? -vc : q == 5 ? vr + vc : q == 6 ? -vr + vc
                  : q == 7 ? -vr - vc : vr - vc;
  return -hb + 2.0 * (((((1.0 + 3.0 * cv) + 4.5 * (cv * cv)) - 1.5 * vv) * wq(q)) * cw);
}

__device__ __forceinline__ void ade_fixed_walls(double (&h)[Q], const Geom& g, const Bc& bc, const AdeWalls& sw, int r,
                                                int c, double ux, double uy, double wr, double wc) {
  const bool rl = r == 0 && bc.row_lo == LBM_EDGE_BOUNCE_BACK, rh = r == g.R - 1 && bc.row_hi == LBM_EDGE_BOUNCE_BACK;
  const bool cl = c == 0 && bc_is_wall(bc.col_lo), ch = c == g.C - 1 && bc_is_wall(bc.col_hi);
  // C_w of the node's edges, loaded up front (independent loads; no dynamic indexing into sw)
  const double w_rl = rl && (sw.fixed & 1) ? (sw.profile[0] ? sw.profile[0][c] : sw.conc[0]) : 0.0;
  const double w_rh = rh && (sw.fixed & 2) ? (sw.profile[1] ? sw.profile[1][c] : sw.conc[1]) : 0.0;
  const double w_cl = cl && (sw.fixed & 4) ? (sw.profile[2] ? sw.profile[2][r] : sw.conc[2]) : 0.0;
  const double w_ch = ch && (sw.fixed & 8) ? (sw.profile[3] ? sw.profile[3][r] : sw.conc[3]) : 0.0;
  const double vr = ux + wr, vc = uy + wc;
  const double vv = vr * vr + vc * vc;
#pragma unroll
  for (int s = 1; s < Q; ++s) {
    const int e = (cl && icy(s) == 1) ? 2 : (ch && icy(s) == -1) ? 3 : (rl && icx(s) == 1) ? 0 : (rh && icx(s) == -1) ? 1 : -1;
    if (e < 0 || !((sw.fixed >> e) & 1)) continue;
    const double cw = e == 0 ? w_rl : e == 1 ? w_rh : e == 2 ? w_cl : w_ch;
    h[s] = ade_fixed_slot(h[s], opp(s), vr, vc, vv, cw);  // opp(s): the outgoing direction
  }
}

// g's gather modes at the walls: a FIXED column bounces back (its anti-bounce-back pairs q with its opposite, also where
// the fluid column is specular)
__host__ __device__ inline Bc ade_scalar_gather_bc(Bc b, int fixed) {
  if (fixed & 4) b.col_lo = LBM_EDGE_BOUNCE_BACK;
  if (fixed & 8) b.col_hi = LBM_EDGE_BOUNCE_BACK;
  return b;
}

// The 9 pulled populations of node pair (r, c), (r, c + 1) of one lattice, 16-byte accesses where the pair's
// sources are column-aligned (q = 0, 1, 3) or lie inside the row (the +-1-column shifted reads, 8-byte aligned
// 16-byte loads); the first and last pair of a row wrap per node.  k_stream_collide_v2's gather, for any lattice.
template <bool NT>
__device__ __forceinline__ void pull_pair(double (&a)[Q], double (&b)[Q], const double* __restrict__ po, const Geom& g,
                                          long rm, long r0, long rp, int c) {
  dbl2 v;
  v = load2a<NT>(po + 0 * g.plane + r0 + c); a[0] = v.x; b[0] = v.y;
  v = load2a<NT>(po + 1 * g.plane + rm + c); a[1] = v.x; b[1] = v.y;
  v = load2a<NT>(po + 3 * g.plane + rp + c); a[3] = v.x; b[3] = v.y;
  if (c > 0 && c + 2 < g.C) {
    v = load2u<NT>(po + 2 * g.plane + r0 + c - 1); a[2] = v.x; b[2] = v.y;
    v = load2u<NT>(po + 5 * g.plane + rm + c - 1); a[5] = v.x; b[5] = v.y;
    v = load2u<NT>(po + 6 * g.plane + rp + c - 1); a[6] = v.x; b[6] = v.y;
    v = load2u<NT>(po + 4 * g.plane + r0 + c + 1); a[4] = v.x; b[4] = v.y;
    v = load2u<NT>(po + 7 * g.plane + rp + c + 1); a[7] = v.x; b[7] = v.y;
    v = load2u<NT>(po + 8 * g.plane + rm + c + 1); a[8] = v.x; b[8] = v.y;
  } else {
    const int cm = wrap_col(g, c - 1), cp = wrap_col(g, c + 2);
    a[2] = po[2 * g.plane + r0 + cm]; b[2] = po[2 * g.plane + r0 + c];
    a[5] = po[5 * g.plane + rm + cm]; b[5] = po[5 * g.plane + rm + c];
    a[6] = po[6 * g.plane + rp + cm]; b[6] = po[6 * g.plane + rp + c];
    a[4] = po[4 * g.plane + r0 + c + 1]; b[4] = po[4 * g.plane + r0 + cp];
    a[7] = po[7 * g.plane + rp + c + 1]; b[7] = po[7 * g.plane + rp + cp];
    a[8] = po[8 * g.plane + rm + c + 1]; b[8] = po[8 * g.plane + rm + cp];
  }
}

// Fused pull step of the pair, interior path: one thread updates two column-adjacent nodes of BOTH lattices
// (36 loads of 8 bytes as 18 16-byte accesses, the same stores); rows wrap (single block).  Boundary fix-ups are
// NOT applied here: k_ade_edge recomputes the wall nodes afterwards.  Requires C % 2 == 0, even row pitch and
// plane stride, 16-byte aligned lattices.  Moments (optional, dense [R][C] / [2][R][C]) of the streamed state.
// BUOYANT: the collisions are the buoyant ones (by; the u written is the shifted one); without it by is not read.
template <class FM, class SM, bool NT_LOAD, bool NT_STORE, bool WITH_MOMENTS, bool BUOYANT = false>
__global__ __launch_bounds__(256) LBM_ADE_WAVES(BUOYANT) void k_ade_stream_collide(
    double* __restrict__ fn, double* __restrict__ gn, const double* __restrict__ fo, const double* __restrict__ go,
    Geom g, FM fm, SM sm, int row_begin, int row_end, int tiles_per_row, double* __restrict__ rho_out,
    double* __restrict__ u_out, double* __restrict__ c_out, AdeBuoyancy by) {
  const long items = (long)(row_end - row_begin) * tiles_per_row;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const int r = row_begin + (int)(it / tiles_per_row);
    const int c = ((int)(it % tiles_per_row) * 256 + threadIdx.x) * 2;
    if (c >= g.C) continue;
    const long rm = g.at(wrap_row(g, r - 1), 0);  // source row of cx = +1 populations
    const long r0 = g.at(r, 0);
    const long rp = g.at(wrap_row(g, r + 1), 0);  // source row of cx = -1 populations
    double fa[Q], fb[Q], ha[Q], hb[Q];            // f and g of node (r, c) and node (r, c + 1)
    pull_pair<NT_LOAD>(fa, fb, fo, g, rm, r0, rp, c);
    pull_pair<NT_LOAD>(ha, hb, go, g, rm, r0, rp, c);
    double rho_a, ux_a, uy_a, c_a, rho_b, ux_b, uy_b, c_b;
    if (BUOYANT) {  // g is collided and stored first: the forced collision then has the registers to itself
      ade_fluid_moments(fa, rho_a, ux_a, uy_a);
      ade_fluid_moments(fb, rho_b, ux_b, uy_b);
      ade_buoyant_shift(ha, by, ux_a, uy_a, c_a);
      ade_buoyant_shift(hb, by, ux_b, uy_b, c_b);
      sm.collide(ha, ux_a, uy_a, c_a);
      sm.collide(hb, ux_b, uy_b, c_b);
#pragma unroll
      for (int q = 0; q < Q; ++q) store2<NT_STORE>(gn + q * g.plane + r0 + c, ha[q], hb[q]);
      ade_buoyant_fluid(fa, fm.omega, by, rho_a, ux_a, uy_a, c_a);
      ade_buoyant_fluid(fb, fm.omega, by, rho_b, ux_b, uy_b, c_b);
#pragma unroll
      for (int q = 0; q < Q; ++q) store2<NT_STORE>(fn + q * g.plane + r0 + c, fa[q], fb[q]);
    } else {
      ade_collide_node(fa, ha, fm, sm, rho_a, ux_a, uy_a, c_a);
      ade_collide_node(fb, hb, fm, sm, rho_b, ux_b, uy_b, c_b);
#pragma unroll
      for (int q = 0; q < Q; ++q) store2<NT_STORE>(fn + q * g.plane + r0 + c, fa[q], fb[q]);
    }
    if (!BUOYANT) {  // (stored above otherwise)
#pragma unroll
      for (int q = 0; q < Q; ++q) store2<NT_STORE>(gn + q * g.plane + r0 + c, ha[q], hb[q]);
    }
    if (WITH_MOMENTS) {
      const long o = (long)r * g.C + c;  // moment fields are dense
      const long n = (long)g.R * g.C;
      store2<false>(rho_out + o, rho_a, rho_b);
      store2<false>(u_out + o, ux_a, ux_b);
      store2<false>(u_out + n + o, uy_a, uy_b);
      store2<false>(c_out + o, c_a, c_b);
    }
  }
}

// Edge pass: the wall nodes of rows [row_begin, row_end) recomputed with the wall gather on both lattices,
// overwriting what the interior launch stored for them.  g takes exactly the fix-up f takes at that edge,
// applied to its own post-collision populations (the driver's no-flux bottom wall, :234-236 = :180-182).
// Edge list: [0, C) row 0 | [C, 2C) row R-1 | [2C, 2C+n) column 0 | [2C+n, 2C+2n) column C-1; an edge is
// listed only if its mode is a wall (the host passes which).
// FIXED: the scalar's FIXED edges (sw) anti-bounce back between the two collisions (ade_fixed_walls); without it the
// kernel is the no-flux pass and sw is not read.
// BUOYANT: the fluid's moments first, the FIXED edges with that unshifted u0, then ade_buoyant_collide.
template <class FM, class SM, bool WITH_MOMENTS, bool FIXED = false, bool BUOYANT = false>
__global__ __launch_bounds__(256) void k_ade_edge(double* __restrict__ fn, double* __restrict__ gn,
                                                  const double* __restrict__ fo, const double* __restrict__ go, Geom g,
                                                  Bc bc, FM fm, SM sm, int row_begin, int row_end,
                                                  double* __restrict__ rho_out, double* __restrict__ u_out,
                                                  double* __restrict__ c_out, AdeWalls sw, AdeBuoyancy by) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, n = row_end - row_begin;
  int r, c;
  if (i < g.C) { r = 0; c = i; if (!bc_is_wall(bc.row_lo)) return; }
  else if (i < 2 * g.C) { r = g.R - 1; c = i - g.C; if (!bc_is_wall(bc.row_hi)) return; }
  else if (i < 2 * g.C + n) { r = row_begin + i - 2 * g.C; c = 0; if (!bc_is_wall(bc.col_lo)) return; }
  else if (i < 2 * g.C + 2 * n) { r = row_begin + i - 2 * g.C - n; c = g.C - 1; if (!bc_is_wall(bc.col_hi)) return; }
  else return;
  if (r < row_begin || r >= row_end) return;
  // a corner with a wall row belongs to the row lists
  if (i >= 2 * g.C && ((r == 0 && bc_is_wall(bc.row_lo)) || (r == g.R - 1 && bc_is_wall(bc.row_hi)))) return;
  // the same node on both column lists (C == 1) is listed once -- unreachable from the C ABI, which refuses an odd C
  if (i >= 2 * g.C + n && g.C == 1 && bc_is_wall(bc.col_lo)) return;
  double f[Q], h[Q], rho, ux, uy, conc;
  gather_walls(f, fo, g, bc, r, c);
  if constexpr (BUOYANT) {  // (constexpr: the forced collision exists for the fluids with an ade_forced_fluid alone)
    gather_walls(h, go, g, FIXED ? ade_scalar_gather_bc(bc, sw.fixed) : bc, r, c);
    ade_fluid_moments(f, rho, ux, uy);
    if (FIXED) ade_fixed_walls(h, g, bc, sw, r, c, ux, uy, sm.wr, sm.wc);
    ade_buoyant_collide(f, h, fm, sm, by, rho, ux, uy, conc);
  } else if (FIXED) {
    gather_walls(h, go, g, ade_scalar_gather_bc(bc, sw.fixed), r, c);
    fm.collide(f, rho, ux, uy);
    ade_fixed_walls(h, g, bc, sw, r, c, ux, uy, sm.wr, sm.wc);
    sm.collide(h, ux, uy, conc);
  } else {
    gather_walls(h, go, g, bc, r, c);
    ade_collide_node(f, h, fm, sm, rho, ux, uy, conc);
  }
  const long o = g.at(r, c);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    fn[q * g.plane + o] = f[q];
    gn[q * g.plane + o] = h[q];
  }
  if (WITH_MOMENTS) {
    const long nn = (long)g.R * g.C, oo = (long)r * g.C + c;
    rho_out[oo] = rho;
    u_out[oo] = ux;
    u_out[nn + oo] = uy;
    c_out[oo] = conc;
  }
}

// The wall fix-ups of gather_walls (bc_fixups_own: rows first, columns win at the corners) for the pair (r, c), (r, c + 1)
// of one lattice after pull_pair: each replaced population is loaded from the node's own post-collision populations, as
// gather_walls loads it -- the same value, so the same bits.  Only the replaced populations are loaded (the own pair of
// a wall row as 16-byte accesses), which keeps the step's register count at the pull's.  Rows: bounce-back; columns:
// bounce-back or specular (what the fused step accepts).
template <bool NT>
__device__ __forceinline__ void wall_fixups_pair(double (&a)[Q], double (&b)[Q], const double* __restrict__ po,
                                                 const Geom& g, const Bc& bc, bool row_lo, bool row_hi, long r0, int c) {
  dbl2 v;
  if (row_lo) {  // bc_fixups_own: f[1] = own[3]; f[5] = own[7]; f[8] = own[6]
    v = load2a<NT>(po + 3 * g.plane + r0 + c); a[1] = v.x; b[1] = v.y;
    v = load2a<NT>(po + 7 * g.plane + r0 + c); a[5] = v.x; b[5] = v.y;
    v = load2a<NT>(po + 6 * g.plane + r0 + c); a[8] = v.x; b[8] = v.y;
  }
  if (row_hi) {  // f[3] = own[1]; f[7] = own[5]; f[6] = own[8]
    v = load2a<NT>(po + 1 * g.plane + r0 + c); a[3] = v.x; b[3] = v.y;
    v = load2a<NT>(po + 5 * g.plane + r0 + c); a[7] = v.x; b[7] = v.y;
    v = load2a<NT>(po + 8 * g.plane + r0 + c); a[6] = v.x; b[6] = v.y;
  }
  if (c + 2 == g.C && bc_is_wall(bc.col_hi)) {  // node b; bounce-back: f[4] = own[2], f[7] = own[5], f[8] = own[6]
    const double* o = po + r0 + c + 1;
    const bool sp = bc.col_hi == LBM_EDGE_SPECULAR;  // specular: f[7] = own[6], f[8] = own[5]
    b[4] = o[2 * g.plane];
    b[7] = o[(sp ? 6 : 5) * g.plane];
    b[8] = o[(sp ? 5 : 6) * g.plane];
  }
  if (c == 0 && bc_is_wall(bc.col_lo)) {  // node a; bounce-back: f[2] = own[4], f[5] = own[7], f[6] = own[8]
    const double* o = po + r0;
    const bool sp = bc.col_lo == LBM_EDGE_SPECULAR;  // specular: f[5] = own[8], f[6] = own[7]
    a[2] = o[4 * g.plane];
    a[5] = o[(sp ? 8 : 7) * g.plane];
    a[6] = o[(sp ? 7 : 8) * g.plane];
  }
}

// The fused step on a PART of a slab, in ONE dispatch with the wall fix-ups inline: rows [band0, band0 + n0) followed by
// rows [band1, band1 + nrows - n0) (FRAME: both edge bands; INNER: one band, n0 = nrows).  Every lane takes pull_pair;
// a lane whose pair holds a wall node -- every node of a wall row, column 0 / C-1 at a wall column -- then replaces the
// populations the wall gather replaces (wall_fixups_pair), on both lattices.  Each population is the value of the one
// load gather_walls / pull_pair take for it and the arithmetic is ade_collide_node's, so the results are those of
// k_ade_stream_collide + k_ade_edge bit for bit.  Rows come from wrap_row: ghost rows once g.ghost > 0 (HALO edges),
// wrapped on a single block (a wall row's pulled row is replaced).  Writes owned nodes only.
// FIXED: as k_ade_edge -- g gathers with ade_scalar_gather_bc and the wall lanes anti-bounce back at the FIXED edges
// between the two collisions of each node.
// BUOYANT: as k_ade_edge -- moments of f, the FIXED edges with u0, then g collided and stored before f.  f cannot be
// stored before the scalar's wall rule here (its collision needs the C that rule leaves): it stays live across the rule
// on the wall lanes.
template <class FM, class SM, bool NT_LOAD, bool NT_STORE, bool WITH_MOMENTS, bool FIXED = false, bool BUOYANT = false>
__global__ __launch_bounds__(256) LBM_ADE_WAVES(BUOYANT) void k_ade_stream_collide_part(
    double* __restrict__ fn, double* __restrict__ gn, const double* __restrict__ fo, const double* __restrict__ go,
    Geom g, Bc bc, FM fm, SM sm, int band0, int n0, int band1, int nrows, int tiles_per_row,
    double* __restrict__ rho_out, double* __restrict__ u_out, double* __restrict__ c_out, AdeWalls sw, AdeBuoyancy by) {
  const long items = (long)nrows * tiles_per_row;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const int v = (int)(it / tiles_per_row);
    const int r = v < n0 ? band0 + v : band1 + (v - n0);
    const int c = ((int)(it % tiles_per_row) * 256 + threadIdx.x) * 2;
    if (c >= g.C) continue;
    const long rm = g.at(wrap_row(g, r - 1), 0);  // source row of cx = +1 populations
    const long r0 = g.at(r, 0);
    const long rp = g.at(wrap_row(g, r + 1), 0);  // source row of cx = -1 populations
    const bool row_lo = r == 0 && bc.row_lo == LBM_EDGE_BOUNCE_BACK, row_hi = r == g.R - 1 && bc.row_hi == LBM_EDGE_BOUNCE_BACK;
    const bool wall = row_lo || row_hi || (c == 0 && bc_is_wall(bc.col_lo)) || (c + 2 == g.C && bc_is_wall(bc.col_hi));
    double fa[Q], fb[Q], ha[Q], hb[Q];            // f and g of node (r, c) and node (r, c + 1)
    pull_pair<NT_LOAD>(fa, fb, fo, g, rm, r0, rp, c);
    if (wall) wall_fixups_pair<NT_LOAD>(fa, fb, fo, g, bc, row_lo, row_hi, r0, c);
    pull_pair<NT_LOAD>(ha, hb, go, g, rm, r0, rp, c);
    double rho_a, ux_a, uy_a, c_a, rho_b, ux_b, uy_b, c_b;
    if (BUOYANT) {
      if (wall) wall_fixups_pair<NT_LOAD>(ha, hb, go, g, FIXED ? ade_scalar_gather_bc(bc, sw.fixed) : bc, row_lo, row_hi, r0, c);
      ade_fluid_moments(fa, rho_a, ux_a, uy_a);
      ade_fluid_moments(fb, rho_b, ux_b, uy_b);
      if (FIXED && wall) {
        ade_fixed_walls(ha, g, bc, sw, r, c, ux_a, uy_a, sm.wr, sm.wc);
        ade_fixed_walls(hb, g, bc, sw, r, c + 1, ux_b, uy_b, sm.wr, sm.wc);
      }
      ade_buoyant_shift(ha, by, ux_a, uy_a, c_a);
      ade_buoyant_shift(hb, by, ux_b, uy_b, c_b);
      sm.collide(ha, ux_a, uy_a, c_a);
      sm.collide(hb, ux_b, uy_b, c_b);
#pragma unroll
      for (int q = 0; q < Q; ++q) store2<NT_STORE>(gn + q * g.plane + r0 + c, ha[q], hb[q]);
      ade_buoyant_fluid(fa, fm.omega, by, rho_a, ux_a, uy_a, c_a);
      ade_buoyant_fluid(fb, fm.omega, by, rho_b, ux_b, uy_b, c_b);
#pragma unroll
      for (int q = 0; q < Q; ++q) store2<NT_STORE>(fn + q * g.plane + r0 + c, fa[q], fb[q]);
    } else if (FIXED) {  // f is stored before the scalar's walls and collisions: its registers are free for them
      if (wall) wall_fixups_pair<NT_LOAD>(ha, hb, go, g, ade_scalar_gather_bc(bc, sw.fixed), row_lo, row_hi, r0, c);
      fm.collide(fa, rho_a, ux_a, uy_a);
      fm.collide(fb, rho_b, ux_b, uy_b);
#pragma unroll
      for (int q = 0; q < Q; ++q) store2<NT_STORE>(fn + q * g.plane + r0 + c, fa[q], fb[q]);
      if (wall) {
        ade_fixed_walls(ha, g, bc, sw, r, c, ux_a, uy_a, sm.wr, sm.wc);
        ade_fixed_walls(hb, g, bc, sw, r, c + 1, ux_b, uy_b, sm.wr, sm.wc);
      }
      sm.collide(ha, ux_a, uy_a, c_a);
      sm.collide(hb, ux_b, uy_b, c_b);
    } else {
      if (wall) wall_fixups_pair<NT_LOAD>(ha, hb, go, g, bc, row_lo, row_hi, r0, c);
      ade_collide_node(fa, ha, fm, sm, rho_a, ux_a, uy_a, c_a);
      ade_collide_node(fb, hb, fm, sm, rho_b, ux_b, uy_b, c_b);
#pragma unroll
      for (int q = 0; q < Q; ++q) store2<NT_STORE>(fn + q * g.plane + r0 + c, fa[q], fb[q]);
    }
    if (!BUOYANT) {  // (stored above otherwise)
#pragma unroll
      for (int q = 0; q < Q; ++q) store2<NT_STORE>(gn + q * g.plane + r0 + c, ha[q], hb[q]);
    }
    if (WITH_MOMENTS) {
      const long o = (long)r * g.C + c;  // moment fields are dense
      const long n = (long)g.R * g.C;
      store2<false>(rho_out + o, rho_a, rho_b);
      store2<false>(u_out + o, ux_a, ux_b);
      store2<false>(u_out + n + o, uy_a, uy_b);
      store2<false>(c_out + o, c_a, c_b);
    }
  }
}

// Interior walls (lbm_ade_iwalls, device copy): one entry per wall node, sorted by (r, c).  A wall node stays a fluid
// node (test/rectangle_sedimentation_test.cpp:184-196, :220-232): the streamed population s of a named slot is replaced
// from the node's own post-collision populations.  slots: bits 0-7 the f slots, 8-15 the g slots, 16-23 the g slots that
// are FIXED (a subset of the g slots); bit s-1 of each byte is slot s.  conc: C_w of the node's FIXED slots.
struct AdeIwallNode {
  int r, c;
  unsigned slots;
  int pad;
  double conc;
};

// the f slots of an interior wall node: f[s] = f*[opp s] of the node itself (on-site bounce-back)
__device__ __forceinline__ void ade_iwalls_fluid(double (&f)[Q], const double* __restrict__ fo, const Geom& g, long o,
                                                 unsigned slots) {
#pragma unroll
  for (int s = 1; s < Q; ++s)
    if ((slots >> (s - 1)) & 1u) f[s] = fo[opp(s) * g.plane + o];
}

// the g slots: NO_FLUX h[s] = h*[opp s], FIXED the anti-bounce-back of ade_fixed_slot with the node's conc; (ux, uy) the
// velocity of the fully fixed-up f.  The table wins every slot it names, whatever the domain's rule left there.
__device__ __forceinline__ void ade_iwalls_scalar(double (&h)[Q], const double* __restrict__ go, const Geom& g, long o,
                                                  unsigned slots, double cw, double ux, double uy, double wr, double wc) {
  const double vr = ux + wr, vc = uy + wc;
  const double vv = vr * vr + vc * vc;
#pragma unroll
  for (int s = 1; s < Q; ++s) {
    if (!((slots >> (7 + s)) & 1u)) continue;
    const double hb = go[opp(s) * g.plane + o];
    h[s] = ((slots >> (15 + s)) & 1u) ? ade_fixed_slot(hb, opp(s), vr, vc, vv, cw) : hb;
  }
}

// Interior-wall pass: the table's nodes of a set of rows recomputed, one lane per node, overwriting what the interior
// launch (and the edge pass, where the node sits on a domain wall) stored for them.  Per node: the domain's gather
// (gather_walls: a node may stand on a domain wall, as the rectangle's feet do; on a slab it reads the ghost rows), the
// f slots, the same for g (FIXED: the domain's FIXED edges as in k_ade_edge), the g slots, both collisions -- in
// k_ade_edge's order, the scalar's rules between the fluid's moments and the scalar's collision.  FIXED: the DOMAIN has
// FIXED edges (sw); the table's own FIXED slots are per node and need no instantiation.
// The rows are two index ranges of the table in ONE dispatch: lane i < n0 takes node first0 + i, the other lanes node
// first1 + (i - n0), n lanes in all.  The table is sorted by (r, c), so the nodes of a band of rows are one range (the
// host's row index, lbm_ade_iwalls_finalize): rows [row_begin, row_end) of a single block = one range with n0 = n (the
// whole block: all nodes); of a slab, FRAME = the prefix [0, first[E]) and the suffix [first[R - E], n_nodes), INNER =
// the range between them with n0 = n.  No lane is filtered by its row.  Reads the old lattices only and writes wall
// nodes of those rows only.
template <class FM, class SM, bool WITH_MOMENTS, bool FIXED = false, bool BUOYANT = false>
__global__ __launch_bounds__(256) void k_ade_iwalls_ranges(double* __restrict__ fn, double* __restrict__ gn,
                                                           const double* __restrict__ fo, const double* __restrict__ go,
                                                           Geom g, Bc bc, FM fm, SM sm, double* __restrict__ rho_out,
                                                           double* __restrict__ u_out, double* __restrict__ c_out,
                                                           AdeWalls sw, AdeBuoyancy by,
                                                           const AdeIwallNode* __restrict__ nodes, int first0, int n0,
                                                           int first1, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const AdeIwallNode nd = nodes[i < n0 ? first0 + i : first1 + (i - n0)];
  const int r = nd.r, c = nd.c;
  const long o = g.at(r, c);
  double f[Q], h[Q], rho, ux, uy, conc;
  gather_walls(f, fo, g, bc, r, c);
  ade_iwalls_fluid(f, fo, g, o, nd.slots);
  gather_walls(h, go, g, FIXED ? ade_scalar_gather_bc(bc, sw.fixed) : bc, r, c);
  if constexpr (BUOYANT) {
    ade_fluid_moments(f, rho, ux, uy);
    if (FIXED) ade_fixed_walls(h, g, bc, sw, r, c, ux, uy, sm.wr, sm.wc);
    ade_iwalls_scalar(h, go, g, o, nd.slots, nd.conc, ux, uy, sm.wr, sm.wc);
    ade_buoyant_collide(f, h, fm, sm, by, rho, ux, uy, conc);
  } else {
    fm.collide(f, rho, ux, uy);
    if (FIXED) ade_fixed_walls(h, g, bc, sw, r, c, ux, uy, sm.wr, sm.wc);
    ade_iwalls_scalar(h, go, g, o, nd.slots, nd.conc, ux, uy, sm.wr, sm.wc);
    sm.collide(h, ux, uy, conc);
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    fn[q * g.plane + o] = f[q];
    gn[q * g.plane + o] = h[q];
  }
  if (WITH_MOMENTS) {
    const long nn = (long)g.R * g.C, oo = (long)r * g.C + c;
    rho_out[oo] = rho;
    u_out[oo] = ux;
    u_out[nn + oo] = uy;
    c_out[oo] = conc;
  }
}

// The interior walls of the lazily streamed state (lbm_ade_solver_get_state), one lane per table node.  SCALAR = false:
// xs = the streamed f, post = the post-collision f: the f slots.  SCALAR = true: xs = the streamed g after
// k_ade_fixed_state, post = the post-collision g, u = [2][R][C] dense, the reference-order calc_u of the fixed-up f: the
// g slots.
template <bool SCALAR>
__global__ __launch_bounds__(256) void k_ade_iwalls_state(double* __restrict__ xs, const double* __restrict__ post,
                                                          Geom g, const AdeIwallNode* __restrict__ nodes, int n_nodes,
                                                          const double* __restrict__ u, double wr, double wc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const AdeIwallNode nd = nodes[i];
  if (!((nd.slots >> (SCALAR ? 8 : 0)) & 0xFFu)) return;
  const long o = g.at(nd.r, nd.c);
  double x[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) x[q] = xs[q * g.plane + o];
  if (SCALAR) {
    const long n = (long)g.R * g.C, d = (long)nd.r * g.C + nd.c;
    ade_iwalls_scalar(x, post, g, o, nd.slots, nd.conc, u[d], u[n + d], wr, wc);
  } else {
    ade_iwalls_fluid(x, post, g, o, nd.slots);
  }
#pragma unroll
  for (int q = 1; q < Q; ++q) xs[q * g.plane + o] = x[q];
}

// the six halvings of fold64 across a wave (diag.hpp: diag_wave_fold<DIAG_ADD>, the same additions): lane j < s takes
// p[j] + p[j + s]; the other lanes hold values nobody reads
__device__ __forceinline__ double ade_wave_sum(double p) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_down(p, s, 64);
  return p;
}

// Wall exchange (lbm_hip.h "wall exchange"): what the table's rules take from the lattices in the stream FROM fo, go, as
// LBM_WALLX_NQ row values per lattice row.  One wave per row, four rows per workgroup, grid-strided over rows [row_begin,
// row_end); lane j takes the row's nodes first[r] + j + 64 k, k ascending, and IS accumulator j of fold64 -- the halvings
// are wave shuffles, as in k_diag_rows.  Per node the lane runs k_ade_iwalls_ranges' body up to the collisions -- the
// domain's gather of f, the f slots, the moments, the domain's gather and FIXED edges of g, the g slots -- noting each
// named slot before and after the table's rule; the only part of fm.collide that is used is its u (what the wall pass
// feeds the FIXED slots; a buoyant call passes the reference-order model, whose u is ade_fluid_moments' u0), so the
// relaxation is dead code.  A node outside rows [reg_r0, reg_r1) or columns [reg_c0, reg_c1) adds nothing.  first =
// NULL: no table, every row value +0.0.  Lane 0 writes table[q * table_rows + table_row0 + r]; nothing else is written.
// No atomics, no LDS, no scratch.  211 VGPRs (228 with FIXED) where the wall pass has 70-93: with no collision and no store
// between them the compiler issues the 72 loads of a node (two gathers, each with the node's own populations) together.
// That is what a launch of a few thousand nodes wants -- its time is load latency, not occupancy
// (profiles/ade_wall_exchange.txt).
template <class FM, bool FIXED>
__global__ __launch_bounds__(256) void k_ade_wall_exchange(double* __restrict__ table, int table_rows, int table_row0,
                                                           const double* __restrict__ fo, const double* __restrict__ go,
                                                           Geom g, Bc bc, FM fm, double wr, double wc, AdeWalls sw,
                                                           const AdeIwallNode* __restrict__ nodes,
                                                           const int* __restrict__ first, int reg_r0, int reg_r1,
                                                           int reg_c0, int reg_c1, int row_begin, int row_end) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  for (long long rr = row_begin + (long long)blockIdx.x * 4 + wave; rr < row_end; rr += (long long)gridDim.x * 4) {
    const int r = (int)rr;
    double acc[LBM_WALLX_NQ];
#pragma unroll
    for (int q = 0; q < LBM_WALLX_NQ; ++q) acc[q] = 0.0;
    const bool counted = first != nullptr && r >= reg_r0 && r < reg_r1;  // wave-uniform
    const int i1 = counted ? first[r + 1] : 0;
    for (int i = (counted ? first[r] : 0) + lane; i < i1; i += 64) {
      const AdeIwallNode nd = nodes[i];
      const int c = nd.c;
      if (c < reg_c0 || c >= reg_c1) continue;
      const long o = g.at(r, c);
      double f[Q], h[Q], x[Q], rho, ux, uy;
      gather_walls(f, fo, g, bc, r, c);
#pragma unroll
      for (int q = 0; q < Q; ++q) x[q] = f[q];
      ade_iwalls_fluid(f, fo, g, o, nd.slots);
      double t_r = 0.0, t_c = 0.0, t_m = 0.0, t_s = 0.0, t_f = 0.0;
#pragma unroll
      for (int s = 1; s < Q; ++s) {
        if (!((nd.slots >> (s - 1)) & 1u)) continue;
        const double d = x[s] - f[s];
        if (icx(s) == 1) t_r = t_r + d;
        if (icx(s) == -1) t_r = t_r - d;
        if (icy(s) == 1) t_c = t_c + d;
        if (icy(s) == -1) t_c = t_c - d;
        t_m = t_m + d;
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) x[q] = f[q];
      fm.collide(x, rho, ux, uy);
      gather_walls(h, go, g, FIXED ? ade_scalar_gather_bc(bc, sw.fixed) : bc, r, c);
      if (FIXED) ade_fixed_walls(h, g, bc, sw, r, c, ux, uy, wr, wc);
#pragma unroll
      for (int q = 0; q < Q; ++q) x[q] = h[q];
      ade_iwalls_scalar(h, go, g, o, nd.slots, nd.conc, ux, uy, wr, wc);
#pragma unroll
      for (int s = 1; s < Q; ++s) {
        if (!((nd.slots >> (7 + s)) & 1u)) continue;
        const double d = x[s] - h[s];
        t_s = t_s + d;
        if ((nd.slots >> (15 + s)) & 1u) t_f = t_f + d;
      }
      acc[LBM_WALLX_FORCE_R] = acc[LBM_WALLX_FORCE_R] + t_r;
      acc[LBM_WALLX_FORCE_C] = acc[LBM_WALLX_FORCE_C] + t_c;
      acc[LBM_WALLX_MASS] = acc[LBM_WALLX_MASS] + t_m;
      acc[LBM_WALLX_SCALAR] = acc[LBM_WALLX_SCALAR] + t_s;
      acc[LBM_WALLX_SCALAR_FIXED] = acc[LBM_WALLX_SCALAR_FIXED] + t_f;
      acc[LBM_WALLX_NODES] = acc[LBM_WALLX_NODES] + 1.0;
    }
#pragma unroll
    for (int q = 0; q < LBM_WALLX_NQ; ++q) acc[q] = ade_wave_sum(acc[q]);
    if (lane == 0) {
      double* __restrict__ t = table + table_row0 + r;
#pragma unroll
      for (int q = 0; q < LBM_WALLX_NQ; ++q) t[(size_t)q * table_rows] = acc[q];
    }
  }
}

// Collide only, no streaming: the driver's first iteration on the pre-collision state (one node per thread).
template <class FM, class SM, bool WITH_MOMENTS, bool BUOYANT = false>
__global__ __launch_bounds__(256) void k_ade_collide(double* __restrict__ fp, double* __restrict__ gp,
                                                     const double* __restrict__ f_in, const double* __restrict__ g_in,
                                                     Geom g, FM fm, SM sm, double* __restrict__ rho_out,
                                                     double* __restrict__ u_out, double* __restrict__ c_out,
                                                     AdeBuoyancy by) {
  const long n_nodes = (long)g.R * g.C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / g.C), c = (int)(i % g.C);
    const long o = g.at(r, c);
    double f[Q], h[Q], rho, ux, uy, conc;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      f[q] = f_in[q * g.plane + o];
      h[q] = g_in[q * g.plane + o];
    }
    if constexpr (BUOYANT) {
      ade_fluid_moments(f, rho, ux, uy);
      ade_buoyant_collide(f, h, fm, sm, by, rho, ux, uy, conc);
    } else {
      ade_collide_node(f, h, fm, sm, rho, ux, uy, conc);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      fp[q * g.plane + o] = f[q];
      gp[q * g.plane + o] = h[q];
    }
    if (WITH_MOMENTS) {
      rho_out[i] = rho;
      u_out[i] = ux;
      u_out[n_nodes + i] = uy;
      c_out[i] = conc;
    }
  }
}

// Open boundaries (lbm_ade_open, device copy): one entry per listed node, sorted by (r, c), and the table's segments.
// The host resolves everything (lbm_ade_open_finalize): per slot s the segment that won it (fseg / gseg: byte s-1 of the
// two words = segment index + 1, 0 = the domain's own gather stays), the nine nodes the node's g is pulled from through
// the scalar's source map (gsrc[q], (r + 1) C + c: ade_open_at; gsrc[0] = the node its OWN post-collision g is read
// from), and per extrapolating slot the index in this table of the inward neighbour (xn).  The kernels look nothing up.
struct AdeOpenSeg {
  int kind, pad;  // LBM_ADE_OPEN_* of an f segment; of a g segment LBM_ADE_SCALAR_*
  double p0, p1;  // ABB: u_w = (p0, p1); ABB_EXTRAPOLATED: u_w = p0 u_prev(node) + p1 u_prev(neighbour); g FIXED: C_w = p0
};
struct AdeOpenNode {
  int r, c;
  unsigned fseg[2], gseg[2];
  int gsrc[Q];
  int xn[Q - 1];
  int pad;
};

__device__ __forceinline__ int ade_open_seg_of(const unsigned (&w)[2], int s) {
  return (int)((w[(s - 1) >> 2] >> (8 * ((s - 1) & 3))) & 0xFFu);
}
// slot s with c_x (the row component) / c_y negated
__host__ __device__ __forceinline__ constexpr int ade_flip_row(int s) {
  return s == 1 ? 3 : s == 3 ? 1 : s == 5 ? 6 : s == 6 ? 5 : s == 7 ? 8 : s == 8 ? 7 : s;
}
__host__ __device__ __forceinline__ constexpr int ade_flip_col(int s) {
  return s == 2 ? 4 : s == 4 ? 2 : s == 5 ? 8 : s == 8 ? 5 : s == 6 ? 7 : s == 7 ? 6 : s;
}

// the f slots of a listed node from its own post-collision populations; the anti-bounce-back is the driver's :150, :164
// expression, f[s] = -f*[q] + ((2 + 9 (u_w.c_q)^2) - 3 u_w.u_w) E_q with q = opp(s); carry = the u of every listed node
// before the iteration (two doubles per node, this table's order), i = this node's index
__device__ __forceinline__ void ade_open_fluid(double (&f)[Q], const double (&own)[Q], const AdeOpenNode& nd,
                                               const AdeOpenSeg* __restrict__ segs, const double* __restrict__ carry,
                                               int i) {
#pragma unroll
  for (int s = 1; s < Q; ++s) {
    const int j = ade_open_seg_of(nd.fseg, s);
    if (!j) continue;
    const AdeOpenSeg sg = segs[j - 1];
    const int q = opp(s);
    if (sg.kind == LBM_ADE_OPEN_BOUNCE_BACK) f[s] = own[q];
    else if (sg.kind == LBM_ADE_OPEN_SPECULAR_ROW) f[s] = own[ade_flip_row(s)];
    else if (sg.kind == LBM_ADE_OPEN_SPECULAR_COL) f[s] = own[ade_flip_col(s)];
    else {
      double wr = sg.p0, wc = sg.p1;
      if (sg.kind == LBM_ADE_OPEN_ABB_EXTRAPOLATED) {
        const int m = nd.xn[s - 1];
        wr = sg.p0 * carry[2 * i] + sg.p1 * carry[2 * m];
        wc = sg.p0 * carry[2 * i + 1] + sg.p1 * carry[2 * m + 1];
      }
      const double uu = wr * wr + wc * wc;
      const double uc = wr * (double)icx(q) + wc * (double)icy(q);
      f[s] = -own[q] + ((2.0 + 9.0 * (uc * uc)) - 3.0 * uu) * wq(q);
    }
  }
}

// the g slots: NO_FLUX h[s] = h*[opp s], FIXED ade_fixed_slot with the segment's C_w; own = the post-collision g of the
// node the map names for this one; (ux, uy) the velocity of the fully fixed-up f
__device__ __forceinline__ void ade_open_scalar(double (&h)[Q], const double (&own)[Q], const AdeOpenNode& nd,
                                                const AdeOpenSeg* __restrict__ segs, double ux, double uy, double wr,
                                                double wc) {
  const double vr = ux + wr, vc = uy + wc;
  const double vv = vr * vr + vc * vc;
#pragma unroll
  for (int s = 1; s < Q; ++s) {
    const int j = ade_open_seg_of(nd.gseg, s);
    if (!j) continue;
    const AdeOpenSeg sg = segs[j - 1];
    const double hb = own[opp(s)];
    h[s] = sg.kind == LBM_ADE_SCALAR_FIXED ? ade_fixed_slot(hb, opp(s), vr, vc, vv, sg.p0) : hb;
  }
}

// A g source of a table: (row + 1) C + column with the row in [-1, R].  An ordinary table's rows lie in [0, R); -1 and R
// are the ghost rows of a slab (a VIEW of the table, lbm_ade_open_slab), and wrap on a ghost = 0 geometry (wrap_row)
__device__ __forceinline__ long ade_open_at(const Geom& g, int biased) {
  return g.at(wrap_row(g, biased / g.C - 1), biased % g.C);
}

// g of a listed node pulled through the map, with the domain's wall gather (bc: the scalar's gather modes) taken from the
// mapped own node; own is left holding those own populations
__device__ __forceinline__ void ade_open_gather_scalar(double (&h)[Q], double (&own)[Q], const double* __restrict__ go,
                                                       const Geom& g, const Bc& bc, const AdeOpenNode& nd) {
  const long om = ade_open_at(g, nd.gsrc[0]);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    h[q] = go[q * g.plane + ade_open_at(g, nd.gsrc[q])];
    own[q] = go[q * g.plane + om];
  }
  bc_fixups_own(h, own, g, bc, nd.r, nd.c);
}

// Open-boundary pass: the table's nodes of a set of rows recomputed, one lane per node, after the interior launch and the
// edge pass and BEFORE the interior-wall pass (a node of both tables carries no rule here: the host checks).  Per node:
// the domain's gather of f (on a slab it reads the ghost rows) and the table's f slots; the moments; g pulled from the
// nine resolved sources with the domain's gather, the domain's FIXED edges, the table's g slots; both collisions in
// k_ade_edge's order.  The rows are two index ranges of the sorted table in ONE dispatch, the launch shape of
// k_ade_iwalls_ranges: lane i < n0 takes node first0 + i, the other lanes node first1 + (i - n0), n lanes in all; the
// whole block is first0 = 0, n0 = n = n_nodes.  No lane is filtered by its row.  carry_out[2 m], [2 m + 1] = the u of the
// fixed-up f (the unshifted u0 of a buoyant step) of node m of the table: the next step's carry_in.  Reads the old
// lattices and carry_in only and writes, of its own nodes only, fn, gn, the moments and carry_out.
template <class FM, class SM, bool WITH_MOMENTS, bool FIXED = false, bool BUOYANT = false>
__global__ __launch_bounds__(256) void k_ade_open_ranges(double* __restrict__ fn, double* __restrict__ gn,
                                                         const double* __restrict__ fo, const double* __restrict__ go,
                                                         Geom g, Bc bc, FM fm, SM sm, double* __restrict__ rho_out,
                                                         double* __restrict__ u_out, double* __restrict__ c_out,
                                                         AdeWalls sw, AdeBuoyancy by,
                                                         const AdeOpenNode* __restrict__ nodes,
                                                         const AdeOpenSeg* __restrict__ segs, int first0, int n0,
                                                         int first1, int n, const double* __restrict__ carry_in,
                                                         double* __restrict__ carry_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int m = i < n0 ? first0 + i : first1 + (i - n0);
  const AdeOpenNode nd = nodes[m];
  const int r = nd.r, c = nd.c;
  const long o = g.at(r, c);
  double f[Q], h[Q], own[Q], rho, ux, uy, conc, u0r, u0c;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    f[q] = fo[q * g.plane + g.at(wrap_row(g, r - icx(q)), wrap_col(g, c - icy(q)))];
    own[q] = fo[q * g.plane + o];
  }
  bc_fixups_own(f, own, g, bc, r, c);
  ade_open_fluid(f, own, nd, segs, carry_in, m);
  ade_open_gather_scalar(h, own, go, g, FIXED ? ade_scalar_gather_bc(bc, sw.fixed) : bc, nd);
  if (BUOYANT) {
    ade_fluid_moments(f, rho, ux, uy);
    u0r = ux, u0c = uy;
    if (FIXED) ade_fixed_walls(h, g, bc, sw, r, c, ux, uy, sm.wr, sm.wc);
    ade_open_scalar(h, own, nd, segs, ux, uy, sm.wr, sm.wc);
    ade_buoyant_collide(f, h, fm, sm, by, rho, ux, uy, conc);
  } else {
    fm.collide(f, rho, ux, uy);
    u0r = ux, u0c = uy;
    if (FIXED) ade_fixed_walls(h, g, bc, sw, r, c, ux, uy, sm.wr, sm.wc);
    ade_open_scalar(h, own, nd, segs, ux, uy, sm.wr, sm.wc);
    sm.collide(h, ux, uy, conc);
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    fn[q * g.plane + o] = f[q];
    gn[q * g.plane + o] = h[q];
  }
  carry_out[2 * m] = u0r;
  carry_out[2 * m + 1] = u0c;
  if (WITH_MOMENTS) {
    const long nn = (long)g.R * g.C, oo = (long)r * g.C + c;
    rho_out[oo] = rho;
    u_out[oo] = ux;
    u_out[nn + oo] = uy;
    c_out[oo] = conc;
  }
}

// The open boundaries of the lazily streamed state (lbm_ade_solver_get_state), one lane per listed node; xs = the
// streamed level, post = the post-collision one.  MODE 0: the f slots (carry: the one the next step would read).  MODE 1:
// g gathered again through the map, with the domain's wall gather (bc: the scalar's gather modes) -- before
// k_ade_fixed_state.  MODE 2: the g slots, u = [2][R][C] dense, the reference-order calc_u of the fixed-up f.
template <int MODE>
__global__ __launch_bounds__(256) void k_ade_open_state(double* __restrict__ xs, const double* __restrict__ post, Geom g,
                                                        Bc bc, const AdeOpenNode* __restrict__ nodes,
                                                        const AdeOpenSeg* __restrict__ segs, int n_nodes,
                                                        const double* __restrict__ carry, const double* __restrict__ u,
                                                        double wr, double wc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const AdeOpenNode nd = nodes[i];
  if (MODE == 0 && !(nd.fseg[0] | nd.fseg[1])) return;
  if (MODE == 2 && !(nd.gseg[0] | nd.gseg[1])) return;
  const long o = g.at(nd.r, nd.c);
  double x[Q], own[Q];
  if (MODE == 1) {
    ade_open_gather_scalar(x, own, post, g, bc, nd);
  } else {
    const long om = MODE == 2 ? ade_open_at(g, nd.gsrc[0]) : o;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      x[q] = xs[q * g.plane + o];
      own[q] = post[q * g.plane + om];
    }
    if (MODE == 0) {
      ade_open_fluid(x, own, nd, segs, carry, i);
    } else {
      const long n = (long)g.R * g.C, d = (long)nd.r * g.C + nd.c;
      ade_open_scalar(x, own, nd, segs, u[d], u[n + d], wr, wc);
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) xs[q * g.plane + o] = x[q];
}

}  // namespace lbm
