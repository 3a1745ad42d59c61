// Internal: what the slab objects of the multi-step blocks share (capi_slab_ibm.hip, capi_slab_pressure.hip; the RCCL
// transport on top of them lives in capi_ring.hip) -- the per-side messages of a block, and the per-rank state of a BGK row
// slab that may (co-)own the band of rows around an immersed boundary.
#pragma once
#include <hip/hip_runtime.h>

#include "internal.hpp"

namespace lbm {

inline long long plane_of(const lbm_geom& g) { return g.plane_stride > 0 ? g.plane_stride : (long long)(g.R + 2 * g.ghost) * g.C; }
// a message buffer of n rows viewed as a dense lattice [9][n][C]
inline lbm_geom msg_geom(int n, int C) { return lbm_geom{n, C, 0, (long long)n * C}; }

// One side's message of a D-step block (side 0 = previous slab, 1 = next; 9 D rows of C doubles either way).  Across an
// ordinary seam it is the complete D-row halo.  Across a SHARED seam -- the neighbour runs the same replicated small lattice
// (a straddled forced band, the pressure seam) -- it is the D rows from slab row `shared_row` that the neighbour's copy of
// that lattice needs at its outer end; they arrive in the stash the next block loads them from.
inline int slab_pack_side(double* send, const double* lat, const lbm_geom& g, int D, int side, bool shared, int shared_row,
                          lbm_stream_t s) {
  if (!shared) return lbm_halo_pack(send, lat, &g, LBM_HALO_FULL(D), side, s);
  const lbm_geom mg = msg_geom(D, g.C);
  return lbm_rows_copy(send, &mg, 0, lat, &g, shared_row, D, s);
}
inline int slab_finish_side(double* lat, double* stash, const double* recv, const lbm_geom& g, int D, int side, bool shared,
                            lbm_stream_t s) {
  if (!shared) return lbm_halo_unpack(lat, recv, &g, LBM_HALO_FULL(D), side, s);
  LBM_CHECK_HIP(hipMemcpyAsync(stash, recv, (size_t)9 * D * g.C * sizeof(double), hipMemcpyDeviceToDevice, as_stream(s)));
  return LBM_OK;
}

}  // namespace lbm

struct lbm_slab_ibm {
  lbm_geom g;            // slab geometry, ghost >= depth
  int row0, rows_global; // global row of slab row 0; rows of the whole domain
  lbm_bc bc_global, bc;  // the domain's edges; this slab's (seams = HALO)
  lbm_bgk_params prm;
  int D;                 // steps per block
  bool has_prev, has_next;
  // the band: global rows [b0, b1) = ROI +- 2 D; rows [b0 + D, b1 - D) are valid after a block
  bool owner;            // the valid band rows intersect this slab's owned rows
  bool straddle_prev, straddle_next;  // ... and reach into the previous / next slab (co-owner there)
  int b0, b1;
  lbm_geom bg;           // band lattice: b1 - b0 rows, periodic (the wrap only ever reaches rows that are dropped)
  lbm_bc bbc;
  double* blat[2];
  int bcur;
  double *brho, *bu;
  lbm_ibm* ib;           // created in band-local rows
  double ga, gb;
  double* stash;         // [9][D][C]: the outer band rows the co-owner computed (state after its last block)
  lbm::SideStream aux;   // full-width band chain, beside the far rows on the caller's stream
  // the forced BOX inside the band: rows of the band x columns ROI +- 2 D (widened to multiples of 8), a small
  // periodic lattice pair for the D forced single steps; everything else in the band takes the D-step window
  bool boxed;
  int bc0, bc1;          // box columns [bc0, bc1) of the lattice
  lbm_geom xg;           // box lattice: band rows x (bc1 - bc0) columns
  double* box[2];
  double *xrho, *xu;
  lbm::SideStream bg_side;  // the window launches (band + far rows) beside the box chain
  bool blat_stale;       // a sole owner's boxed blocks work on the slab lattice directly: the band lattice is behind
};
