// Fluid + transported scalar with the entropic KBC collision as the fluid: the interior pair kernel of that step and its
// part form for row slabs.  The edge pass, the interior-wall pass and the collide-only launch are ade.hpp's kernels with a
// KBC model as FM (one node per lane, latency-bound); only the kernels that hold two nodes of both lattices per lane are
// written for this fluid.
#pragma once
#include "ade.hpp"
#include "kbc.hpp"

namespace lbm {

// nothing moves across this point in the instruction schedule: the phases of k_ade_kbc_stream_collide stay phases
__device__ __forceinline__ void ade_kbc_phase() { __builtin_amdgcn_sched_barrier(0); }

// k_ade_stream_collide for a KBC fluid: the same pair of column-adjacent nodes per lane, the same 16-byte gather
// (pull_pair), stores, grid stride and optional moments -- in another ORDER.  The KBC collision keeps ~100 doubles of
// its own live (nine central moments, two 9-vectors and the equilibrium of each node), so with all 36 populations of
// the pair in registers beside it the kernel comes out at 222-252 VGPRs: two waves per SIMD.  Here the lane holds one
// lattice at a time:
//   f pair in -> collide node a, node b -> f pair out; (rho, ux, uy) of both nodes stay (6 doubles)
//   g pair in -> the scalar's collision of both nodes with those u -> g pair out -> moments out
// G_EARLY: the 18 loads of g are issued BEFORE the fluid's collisions (their latency hides behind ~400 f64 operations,
// at 36 more registers during the collisions, which then run one after the other behind a fence: 186 VGPRs, interleaved
// 222); without it after the f stores (152 VGPRs reassociated, 172 reference order).  The phases are fenced
// (ade_kbc_phase): the scheduler would otherwise hoist the g loads -- independent, __restrict__ -- to the top of the
// iteration, which is the naive kernel again.  Measured at 8192^2 (profiles/ade_kbc.txt): reassociated early 3.46 ms, late
// 3.51 ms per step in every repeat -- two waves per SIMD with the loads in flight beat three that wait for them -- so the
// reassociated pair runs early; the reference-order pair (234 VGPRs early) runs late.  128 VGPRs were not to be had
// without scratch: amdgpu_waves_per_eu(4) spills 124-260 B, (3) on the reference order 20 B.  The attribute asks for two
// waves: with it the reference-order pair comes out at 172 VGPRs, without it at 218.
// The arithmetic is fm.collide's and sm.collide's, expression for expression: only the order of independent loads and
// stores differs from k_ade_stream_collide<FM, SM>, so the populations stored are the same bits.
// Requirements as k_ade_stream_collide: C % 2 == 0, even pitch and plane stride, 16-byte aligned lattices; no wall
// fix-ups (k_ade_edge recomputes the wall nodes afterwards).
template <class FM, class SM, bool NT_LOAD, bool NT_STORE, bool WITH_MOMENTS, bool G_EARLY>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_ade_kbc_stream_collide(
    double* __restrict__ fn, double* __restrict__ gn, const double* __restrict__ fo, const double* __restrict__ go,
    Geom g, FM fm, SM sm, int row_begin, int row_end, int tiles_per_row, double* __restrict__ rho_out,
    double* __restrict__ u_out, double* __restrict__ c_out) {
  const long items = (long)(row_end - row_begin) * tiles_per_row;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const int r = row_begin + (int)(it / tiles_per_row);
    const int c = ((int)(it % tiles_per_row) * 256 + threadIdx.x) * 2;
    if (c >= g.C) continue;
    const long rm = g.at(wrap_row(g, r - 1), 0);  // source row of cx = +1 populations
    const long r0 = g.at(r, 0);
    const long rp = g.at(wrap_row(g, r + 1), 0);  // source row of cx = -1 populations
    double xa[Q], xb[Q], ha[Q], hb[Q];            // the lattice in flight of node (r, c) and node (r, c + 1)
    double rho_a, ux_a, uy_a, c_a, rho_b, ux_b, uy_b, c_b;
    pull_pair<NT_LOAD>(xa, xb, fo, g, rm, r0, rp, c);
    if (G_EARLY) pull_pair<NT_LOAD>(ha, hb, go, g, rm, r0, rp, c);
    ade_kbc_phase();
    fm.collide(xa, rho_a, ux_a, uy_a);
    if (G_EARLY) ade_kbc_phase();  // with g in registers too: one collision at a time (interleaved: 222 VGPRs, fenced: 186)
    fm.collide(xb, rho_b, ux_b, uy_b);
    ade_kbc_phase();
#pragma unroll
    for (int q = 0; q < Q; ++q) store2<NT_STORE>(fn + q * g.plane + r0 + c, xa[q], xb[q]);
    if (!G_EARLY) {
      ade_kbc_phase();
      pull_pair<NT_LOAD>(ha, hb, go, g, rm, r0, rp, c);
    }
    sm.collide(ha, ux_a, uy_a, c_a);
    sm.collide(hb, ux_b, uy_b, c_b);
#pragma unroll
    for (int q = 0; q < Q; ++q) store2<NT_STORE>(gn + q * g.plane + r0 + c, ha[q], hb[q]);
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

// The forced collision of a KBC fluid (ade.hpp ade_forced_fluid, the hook of the one-node kernels): kbc::collide() on the
// moments the driver HOLDS (src/ulbm.cpp:91-126) -- m0 = rho = calc_rho(f) and m1 = the shifted u = u0 + u_shift F.  The
// conserved central moments relax with rate 1 (S = {1, 1, 1, s2, ...}, ulbm.cpp:46-49), so the post-collision momentum is
// rho (u0 + u_shift F): a velocity-shift forcing with a momentum input of exactly rho u_shift F per collision and no
// source term -- by.ga, by.gb and conc are not read.  KbcFastModel drops the conserved central moments and has no such
// collision: a buoyant step runs the reference order.
__device__ __forceinline__ void ade_forced_fluid(double (&f)[Q], const KbcModel& fm, const AdeBuoyancy&, double& rho,
                                                 double ux, double uy, double) {
  fm.collide_with(f, rho, ux, uy);
}

// k_ade_kbc_stream_collide, BUOYANT: the scalar pushes on the fluid (AdeBuoyancy; lbm_hip.h "buoyancy with a KBC fluid").
// The fluid's collision needs C now, so the passive order (f in, collide, f out, then g) cannot stay; the order is the one
// that made the BGK buoyant kernels fit -- the scalar is collided and STORED before the fluid's collisions, which then run
// with f alone in registers:
//   f pair in -> rho, u0 of both nodes (ade_fluid_moments, as KbcModel::collide forms them)
//   g pair in -> C, the shifted u (ade_buoyant_shift) -> the scalar's collisions with that u -> g pair out
//   collide_with node a | collide_with node b, fenced one after the other -> f pair out -> moments out (the shifted u)
// There is no fence between the fluid's moments and the g pull: the scheduler issues the 18 loads of g with those of f
// (36 populations in registers while nothing else is live).  A candidate with that fence -- the g loads wait for the
// moments -- has the same registers and measured 0.2 - 0.3 % slower at 8192^2 in every repeat (profiles/
// ade_kbc_buoyancy.txt); it is not built.  172 VGPRs (178 with the moments), no scratch: the passive reference-order pair's.
// The arithmetic is ade_fluid_moments', ade_buoyant_shift's, sm.collide's and fm.collide_with's, expression for
// expression: the stored bits are those of k_ade_collide<KbcModel, SM, ., true> on the streamed populations.
// Requirements as k_ade_kbc_stream_collide; no wall fix-ups (k_ade_edge recomputes the wall nodes afterwards).
template <class FM, class SM, bool NT_LOAD, bool NT_STORE, bool WITH_MOMENTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_ade_kbc_stream_collide_buoyant(
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
    double xa[Q], xb[Q], ha[Q], hb[Q];            // f and g of node (r, c) and node (r, c + 1)
    double rho_a, ux_a, uy_a, c_a, rho_b, ux_b, uy_b, c_b;
    pull_pair<NT_LOAD>(xa, xb, fo, g, rm, r0, rp, c);
    ade_fluid_moments(xa, rho_a, ux_a, uy_a);
    ade_fluid_moments(xb, rho_b, ux_b, uy_b);
    pull_pair<NT_LOAD>(ha, hb, go, g, rm, r0, rp, c);
    ade_buoyant_shift(ha, by, ux_a, uy_a, c_a);
    ade_buoyant_shift(hb, by, ux_b, uy_b, c_b);
    sm.collide(ha, ux_a, uy_a, c_a);
    sm.collide(hb, ux_b, uy_b, c_b);
#pragma unroll
    for (int q = 0; q < Q; ++q) store2<NT_STORE>(gn + q * g.plane + r0 + c, ha[q], hb[q]);
    ade_kbc_phase();
    fm.collide_with(xa, rho_a, ux_a, uy_a);
    ade_kbc_phase();  // one collision at a time
    fm.collide_with(xb, rho_b, ux_b, uy_b);
    ade_kbc_phase();
#pragma unroll
    for (int q = 0; q < Q; ++q) store2<NT_STORE>(fn + q * g.plane + r0 + c, xa[q], xb[q]);
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

// k_ade_stream_collide_part for a KBC fluid: the fused step on a PART of a slab in ONE dispatch with the wall fix-ups
// inline -- rows [band0, band0 + n0) followed by rows [band1, band1 + nrows - n0), rows through wrap_row (ghost rows once
// g.ghost > 0), owned nodes written only -- in the ORDER of k_ade_kbc_stream_collide, one lattice per lane at a time:
//   f pair in, its wall fix-ups -> collide node a, node b -> f pair out; (rho, ux, uy) of both nodes stay
//   g pair in, its wall fix-ups (FIXED: gathered with ade_scalar_gather_bc) -> FIXED: the wall lanes anti-bounce back at
//   the FIXED edges with the kept u -> the scalar's collisions -> g pair out -> moments out
// G_EARLY: the g pull and its fix-ups in front of the fluid's collisions, as in the interior kernel.  Measured on 4 slabs
// of 2048 x 8192 (profiles/ade_kbc_slabs.txt), the answer is NOT the interior kernel's: the reference-order pair runs early
// (206-210 VGPRs; faster than late, 174-177, in every repeat, with and without walls), the reassociated pair late (154-156
// VGPRs, three waves; early, 186-189, wins on the walled chain and loses on the ring).  No instantiation has scratch.
// Instantiating k_ade_stream_collide_part with a KBC model instead holds all 36 populations beside the collision: the
// naive kernel.  Launched from a translation unit of its own (capi_ade_kbc_part.hip).
// Each population is the value of the one load gather_walls / pull_pair take for it, and the arithmetic is fm.collide's,
// ade_fixed_walls' and sm.collide's in k_ade_edge's FIXED order, expression for expression: the stored bits are those of
// k_ade_kbc_stream_collide + k_ade_edge<KbcModel ...> on one block.  The BUOYANT form is a kernel of its own,
// k_ade_kbc_stream_collide_part_buoyant below.  Requirements as k_ade_stream_collide_part.
template <class FM, class SM, bool NT_LOAD, bool NT_STORE, bool WITH_MOMENTS, bool FIXED, bool G_EARLY>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_ade_kbc_stream_collide_part(
    double* __restrict__ fn, double* __restrict__ gn, const double* __restrict__ fo, const double* __restrict__ go,
    Geom g, Bc bc, FM fm, SM sm, int band0, int n0, int band1, int nrows, int tiles_per_row,
    double* __restrict__ rho_out, double* __restrict__ u_out, double* __restrict__ c_out, AdeWalls sw) {
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
    double xa[Q], xb[Q], ha[Q], hb[Q];            // the lattice in flight of node (r, c) and node (r, c + 1)
    double rho_a, ux_a, uy_a, c_a, rho_b, ux_b, uy_b, c_b;
    pull_pair<NT_LOAD>(xa, xb, fo, g, rm, r0, rp, c);
    if (wall) wall_fixups_pair<NT_LOAD>(xa, xb, fo, g, bc, row_lo, row_hi, r0, c);
    if (G_EARLY) {
      pull_pair<NT_LOAD>(ha, hb, go, g, rm, r0, rp, c);
      if (wall) wall_fixups_pair<NT_LOAD>(ha, hb, go, g, FIXED ? ade_scalar_gather_bc(bc, sw.fixed) : bc, row_lo, row_hi, r0, c);
    }
    ade_kbc_phase();
    fm.collide(xa, rho_a, ux_a, uy_a);
    if (G_EARLY) ade_kbc_phase();  // with g in registers too: one collision at a time
    fm.collide(xb, rho_b, ux_b, uy_b);
    ade_kbc_phase();
#pragma unroll
    for (int q = 0; q < Q; ++q) store2<NT_STORE>(fn + q * g.plane + r0 + c, xa[q], xb[q]);
    if (!G_EARLY) {
      ade_kbc_phase();
      pull_pair<NT_LOAD>(ha, hb, go, g, rm, r0, rp, c);
      if (wall) wall_fixups_pair<NT_LOAD>(ha, hb, go, g, FIXED ? ade_scalar_gather_bc(bc, sw.fixed) : bc, row_lo, row_hi, r0, c);
    }
    if (FIXED && wall) {
      ade_fixed_walls(ha, g, bc, sw, r, c, ux_a, uy_a, sm.wr, sm.wc);
      ade_fixed_walls(hb, g, bc, sw, r, c + 1, ux_b, uy_b, sm.wr, sm.wc);
    }
    sm.collide(ha, ux_a, uy_a, c_a);
    sm.collide(hb, ux_b, uy_b, c_b);
#pragma unroll
    for (int q = 0; q < Q; ++q) store2<NT_STORE>(gn + q * g.plane + r0 + c, ha[q], hb[q]);
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

// k_ade_kbc_stream_collide_part, BUOYANT: the forced KBC collision on a PART of a slab.  The launch shape is the part
// kernel's -- both row bands in one dispatch, a column pair per lane, rows through wrap_row, owned nodes written only, wall
// fix-ups inline -- and the order is k_ade_kbc_stream_collide_buoyant's, the scalar collided and STORED before the fluid:
//   f pair in, its wall fix-ups -> rho, u0 of both nodes (ade_fluid_moments)
//   g pair in, its wall fix-ups (FIXED: gathered with ade_scalar_gather_bc) -> FIXED: the wall lanes anti-bounce back at
//   the FIXED edges with the UNSHIFTED u0 (k_ade_edge's BUOYANT order) -> C, the shifted u (ade_buoyant_shift) -> the
//   scalar's collisions with that u -> g pair out
//   collide_with node a | collide_with node b, fenced one after the other with f alone in registers -> f pair out ->
//   moments out (the shifted u)
// f cannot be stored before the scalar's wall rule (its collision needs the C that rule leaves): on the wall lanes it stays
// live across the rule, as in k_ade_stream_collide_part<..., BUOYANT>.
// G_FENCED: a fence between the fluid's moments and the g pull -- the g loads wait for the moments instead of being issued
// with those of f.  The candidate of the order; built with LBM_EXPERIMENTS alone.
// Each population is the value of the one load gather_walls / pull_pair take for it, and the arithmetic is
// ade_fluid_moments', ade_fixed_walls', ade_buoyant_shift's, sm.collide's and fm.collide_with's, expression for expression:
// FRAME + INNER store the bits of k_ade_kbc_stream_collide_buoyant + k_ade_edge<KbcModel, ., ., ., BUOYANT> on one block.
// Launched from a translation unit of its own (capi_ade_kbc_buoyant_part.hip).  Requirements as k_ade_stream_collide_part.
template <class FM, class SM, bool NT_LOAD, bool NT_STORE, bool WITH_MOMENTS, bool FIXED, bool G_FENCED = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_ade_kbc_stream_collide_part_buoyant(
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
    double xa[Q], xb[Q], ha[Q], hb[Q];            // f and g of node (r, c) and node (r, c + 1)
    double rho_a, ux_a, uy_a, c_a, rho_b, ux_b, uy_b, c_b;
    pull_pair<NT_LOAD>(xa, xb, fo, g, rm, r0, rp, c);
    if (wall) wall_fixups_pair<NT_LOAD>(xa, xb, fo, g, bc, row_lo, row_hi, r0, c);
    ade_fluid_moments(xa, rho_a, ux_a, uy_a);
    ade_fluid_moments(xb, rho_b, ux_b, uy_b);
    if (G_FENCED) ade_kbc_phase();
    pull_pair<NT_LOAD>(ha, hb, go, g, rm, r0, rp, c);
    if (wall) wall_fixups_pair<NT_LOAD>(ha, hb, go, g, FIXED ? ade_scalar_gather_bc(bc, sw.fixed) : bc, row_lo, row_hi, r0, c);
    if (FIXED && wall) {  // with the unshifted u0
      ade_fixed_walls(ha, g, bc, sw, r, c, ux_a, uy_a, sm.wr, sm.wc);
      ade_fixed_walls(hb, g, bc, sw, r, c + 1, ux_b, uy_b, sm.wr, sm.wc);
    }
    ade_buoyant_shift(ha, by, ux_a, uy_a, c_a);
    ade_buoyant_shift(hb, by, ux_b, uy_b, c_b);
    sm.collide(ha, ux_a, uy_a, c_a);
    sm.collide(hb, ux_b, uy_b, c_b);
#pragma unroll
    for (int q = 0; q < Q; ++q) store2<NT_STORE>(gn + q * g.plane + r0 + c, ha[q], hb[q]);
    ade_kbc_phase();
    fm.collide_with(xa, rho_a, ux_a, uy_a);
    ade_kbc_phase();  // one collision at a time
    fm.collide_with(xb, rho_b, ux_b, uy_b);
    ade_kbc_phase();
#pragma unroll
    for (int q = 0; q < Q; ++q) store2<NT_STORE>(fn + q * g.plane + r0 + c, xa[q], xb[q]);
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

// k_ade_open_ranges for a KBC fluid: the open-boundary pass of a set of rows, one lane per listed node -- the same launch
// shape (two index ranges of the sorted table in one dispatch), the same loads, rules, stores and carry, expression for
// expression, so what it stores are the bits of k_ade_open_ranges<FM, SM, ...> were that instantiated.  A kernel of its
// own for one reason: the shared template chooses its BUOYANT branch with a plain `if`, so it also compiles the forced
// collision for the passive models, and KbcFastModel has none (it drops the conserved central moments: ade_forced_fluid
// above).  Here the branch is `if constexpr`.  BUOYANT: the forced collision (collide_with on u0 + u_shift F) through
// ade_buoyant_collide; the domain's FIXED edges, the table's g slots and carry_out see the UNSHIFTED u0, the moments
// written hold the shifted u.  One node per lane: f, h, own and the collision are what is live.
template <class FM, class SM, bool WITH_MOMENTS, bool FIXED, bool BUOYANT>
__global__ __launch_bounds__(256) void k_ade_kbc_open_ranges(double* __restrict__ fn, double* __restrict__ gn,
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
  if constexpr (BUOYANT) {
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

}  // namespace lbm
