// Internal: the schedules of the multi-step BLOCKS that the single-block solver (capi_solver.hip) and the slab objects
// (capi_slab_ibm.hip, capi_slab_pressure.hip) share -- the forced box and the full-width forced band around an immersed
// boundary, and the chain of single steps on the small lattice across pressure-periodic rows.
#pragma once
#include "internal.hpp"

namespace lbm {

// The forced BOX of a D-step block with an immersed boundary.  The forcing reaches a node only through the ROI, so the D
// forced single steps are cut to rows and columns ROI +- 2 D: `box` (bg.R x bg.C nodes, with rho, u of its own) is read out
// of `in` at (row, col), advances D forced single steps as a small periodic lattice pair (what its wrap spoils is the frame
// that is dropped anyway), and its inner part -- ROI +- D -- goes into `out` at (row + D, col + D); in and out share the
// geometry g.  The boundary's tables live in a lattice whose node (ib_row, ib_col) is the box's first node.
// `windows(stream)` enqueues the D-step window launch(es) that run BESIDE this chain of small launches: on the stream
// `beside`, forked at the point BEFORE the box is copied in (the windows read the time-t lattice only and do not wait for
// the copy) and joined before the box is copied out, which overwrites their unforced result.  beside = NULL: everything on st, the
// windows behind the chain.  Every exit after the fork joins.
template <class Windows>
int ibm_forced_box_block(const double* in, double* out, const lbm_geom& g, int row, int col, double* const box[2],
                         const lbm_geom& bg, double* box_rho, double* box_u, lbm_ibm* ib, int ib_row, int ib_col,
                         const lbm_bgk_params& prm, double guo_a, double guo_b, int D, SideStream* beside, Windows&& windows,
                         hipStream_t st) {
  const int Rb = bg.R, Cb = bg.C;
  const lbm_bc pb{LBM_EDGE_PERIODIC, LBM_EDGE_PERIODIC, LBM_EDGE_PERIODIC, LBM_EDGE_PERIODIC, 0, 1.0, 1.0, 0.0, 0.0};
  if (beside)
    if (int rc = beside->mark(st)) return rc;
  int cur = 0;
  auto chain = [&]() -> int {
    int rc = box_copy(box[0], bg, 0, 0, in, g, row, col, Rb, Cb, st);
    if (rc) return rc;
    // "ibm_chain_kernel" = 1 (opt-in): the chain as ONE launch of a few workgroups on compute units of their own, the
    // window launch held back until they are resident.  Bit-identical; measured level with the 3 D small launches
    // (73 / 87 / 118 k against 77 / 98 / 121 k MLUPS at 2048 / 4096 / 16384 rows): what it gains in isolation it loses to
    // coherent (L2-bypassing) accesses and 3 D grid barriers -- DESIGN 5.3
    rc = tuning("ibm_chain_kernel", 0)
             ? ibm_box_chain(ib, ib_row, ib_col, box, &cur, &bg, &prm, bgk_uses_fast_model(&prm, &pb), D, box_rho, box_u, guo_a, guo_b, st)
             : 1;
    if (rc < 0) return rc;
    const bool one_launch = rc == 0;
    if (beside) {
      rc = beside->start();  // (only now: the chain's first launches above are what the block waits for)
      if (!rc && one_launch) rc = ibm_gate(ib, beside->st);
      // (round 4, measured and not kept: the window as PERSISTENT waves that leave 32 .. 256 wave slots of the card free for
      // the chain from its first cycle to its last -- 143 - 150 k MLUPS against 148.5 / 149.3 k with every slot taken, and
      // 115 - 118 k against 124 - 128 k in the reference order: the chain is not waiting for slots.  profiles/r04_ibm_reserve.txt)
      if (!rc) rc = windows(beside->st);
      if (rc) return rc;
    }
    for (int k = 1; k <= D && !one_launch; ++k, cur ^= 1) {  // cylinder_test.cpp:103-127 on the shrinking trapezoid
      rc = lbm_bgk_stream_collide(box[cur ^ 1], box[cur], &bg, &pb, &prm, k, Rb - k, box_rho, box_u, st);
      if (!rc) rc = ibm_step_window(ib, ib_row, ib_col, box[cur ^ 1], &bg, box_u, box_rho, prm.omega, guo_a, guo_b, st);
      if (rc) return rc;
    }
    return beside ? LBM_OK : windows(st);
  };
  int rc = chain();
  if (beside) rc = beside->join(st, rc);
  if (rc) return rc;
  return box_copy(out, g, row + D, col + D, box[cur], bg, D, D, Rb - 2 * D, Cb - 2 * D, st);
}

// The full-width forced BAND: D forced single steps on a trapezoid that loses one row per side and step -- step k computes
// rows [row_lo + k, row_hi - k) from step k - 1, the first from `in`.  The steps alternate between two lattices and END in
// `last` (step k writes `last` when D - k is even, `other` when odd; `in` may be the one the first step does not write).
// The whole band in ONE launch per step (rho, u are written for its rows outside the ROI too: harmless, and four launches
// fewer per step), then the forcing on the same stream: beside its one workgroup there is nothing left to run, and a
// cross-stream dependency costs more than it could hide.
inline int ibm_forced_band_chain(lbm_ibm* ib, const double* in, double* last, double* other, const lbm_geom& g, const lbm_bc& bc,
                                 const lbm_bgk_params& prm, int row_lo, int row_hi, double* rho, double* u, double guo_a,
                                 double guo_b, int D, hipStream_t st) {
  for (int k = 1; k <= D; ++k) {
    double* o = (D - k) % 2 == 0 ? last : other;
    int rc = lbm_bgk_stream_collide(o, in, &g, &bc, &prm, row_lo + k, row_hi - k, rho, u, st);
    if (!rc) rc = lbm_ibm_step(ib, o, &g, u, rho, prm.omega, guo_a, guo_b, st);
    if (rc) return rc;
    in = o;
  }
  return LBM_OK;
}

// The chain across PRESSURE-PERIODIC rows: D ordinary single steps of the small lattice pair `lat` (all g.R rows, the
// pressure rows of bc included), by the model's own single-step launch; *cur flips with every step.
inline int seam_chain(double* const lat[2], int* cur, const lbm_geom& g, const lbm_bc& bc, int model, const lbm_bgk_params& bgk,
                      const lbm_kbc_params& kbc, int D, hipStream_t st) {
  for (int k = 0; k < D; ++k, *cur ^= 1) {
    const int rc = model == LBM_MODEL_BGK ? lbm_bgk_stream_collide(lat[*cur ^ 1], lat[*cur], &g, &bc, &bgk, 0, g.R, nullptr, nullptr, st)
                                          : lbm_kbc_stream_collide(lat[*cur ^ 1], lat[*cur], &g, &bc, &kbc, 0, g.R, nullptr, nullptr, st);
    if (rc) return rc;
  }
  return LBM_OK;
}

}  // namespace lbm
