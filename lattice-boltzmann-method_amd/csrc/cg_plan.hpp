// The tile plan of one launch of the fused two-phase step (launch_cg_fused_t, capi_cg.hip): which tiles form the plain
// INNER rectangle, which the FRAME around it, and how the rectangle is cut into big tiles.  Host arithmetic on plain
// integers only -- no HIP, no tuning table -- so that drivers/cg_plan_dump.cpp and tests/test_cg_plan.py reach it
// without a GPU.
#pragma once
#include "../../include/lbm_hip.h"

namespace lbm {

// The tiles of a launch split into an INNER rectangle [ir0, ir1) x [ic0, ic1) (tile coordinates) --
// every node of the tile, of its +-2 ring and of their +-1 gathers lies inside the block or its
// ghost rows and carries no boundary fix-up: plain offsets, no clamps, no wraps -- and the FRAME
// around it, which keeps the general boundary gather.
struct CgTileRect {
  int ir0, ir1, ic0, ic1;
};

// one launch: TR x TC tiles over rows [row_begin, row_end) of an R x C block; lo_halo / hi_halo: that row edge is
// LBM_EDGE_HALO (with ghost rows, the rows across the seam count as plain nodes)
struct CgPlanCase {
  int TR, TC, R, C, ghost;
  bool lo_halo, hi_halo;
  int row_begin, row_end, part, edge_rows;
};

// the tuning values the plan depends on ("cg_split", "cg_big", "cg_big_xcd"), read by the caller
struct CgPlanKnobs {
  int cg_split = 1, cg_big = 2, cg_big_xcd = 402;
  bool experiments = false;  // the build has the losing big-tile shapes and the walking tile
};

// several nodes per thread (k_cg_tile_mn): {rows, columns, threads, waves per SIMD the registers are budgeted for}
// default (round 4): shape 2, 16 x 64 tiles, two nodes per thread, the waiting one parked in LDS -- +4 .. +7 % over the 16 x 32
// tile kernel on every box measured (profiles/r04_cg_big_sweep.txt); "cg_big" = 0 restores k_cg_fused<16,32,4> on the inner rectangle
constexpr int kCgBigShapes[][4] = {{32, 32, 512, 4}, {16, 64, 512, 4}, {16, 128, 1024, 4}, {32, 64, 1024, 4}, {32, 64, 512, 2},
                                   {8, 64, 512, 4},  {16, 64, 1024, 4}, {16, 128, 512, 2},  {16, 32, 512, 4}};
constexpr int kCgWalkTile = 10;  // "cg_big" = 10: the WALKING tile (k_cg_walk_tile) on the big tiles of shape 2

struct CgPlan {
  int tiles_r, tiles_c;
  CgTileRect rc;
  bool split;        // false: every tile through the general path, one launch (frame = all tiles, inner = 0)
  int frame, inner;  // tiles of each launch; frame + inner = tiles_r * tiles_c
  // big tiles: the rectangle is cut into n_btr x n_btc tiles of shape `shape` (1 .. 9: kCgBigShapes[shape - 1], kCgWalkTile:
  // shape 2) from its top-left corner and SHRUNK to them, what does not fill a big tile joins the frame; 0 x 0: none
  int n_btr, n_btc, shape;
  int big_xcd;  // the patch order k_cg_tile_mn gets
};

inline CgPlan cg_plan(const CgPlanCase& a, const CgPlanKnobs& k) {
  const int TR = a.TR, TC = a.TC;
  CgPlan p{};
  // part 0: the whole row range; FRAME / INNER: ONLY the frame -- widened to every node of the first and last `edge_rows`
  // rows of the range -- / ONLY the inner rectangle (lbm_cg_step_fused_part)
  p.tiles_r = (a.row_end - a.row_begin + TR - 1) / TR;
  p.tiles_c = (a.C + TC - 1) / TC;
  // inner rectangle of tiles: the tile's ring rows r_base-2 .. r_base+TR+1 are plain nodes (not the
  // wall rows of the global domain; across a seam the ghost rows count as plain), its ring columns
  // c_base-2 .. c_base+TC+1 lie in [1, C-2] (their gathers do not wrap), and the tile is complete
  const int lo_row = (a.ghost && a.lo_halo) ? -2 : 1;
  const int hi_row = (a.ghost && a.hi_halo) ? a.R + 1 : a.R - 2;
  CgTileRect rc{p.tiles_r, 0, 1, 0};
  for (int i = 0; i < p.tiles_r; ++i) {
    const int rb = a.row_begin + i * TR;
    if (rb - 2 >= lo_row && rb + TR + 1 <= hi_row && rb + TR <= a.row_end) {
      rc.ir0 = rc.ir0 < i ? rc.ir0 : i;
      rc.ir1 = i + 1;
    }
  }
  rc.ic1 = (a.C - 3) / TC;  // last tile column with c_base + TC + 1 <= C - 2
  if (rc.ic1 > p.tiles_c) rc.ic1 = p.tiles_c;
  if (a.part && a.edge_rows > 0) {
    // clamp by rows counted from row_begin, not by tiles counted back from the last one: that tile may be partial, and
    // tiles_r - ceil(edge_rows / TR) would leave up to TR - 1 of the last edge_rows rows inside the inner rectangle
    // (R = 130, edge_rows = 3: row 127).  Where TR divides the height the two bounds agree.
    const int first = (a.edge_rows + TR - 1) / TR, last = (a.row_end - a.row_begin - a.edge_rows) / TR;
    rc.ir0 = rc.ir0 > first ? rc.ir0 : first;
    rc.ir1 = rc.ir1 < last ? rc.ir1 : last;
  }
  p.split = (a.part || k.cg_split != 0) && rc.ir1 - rc.ir0 >= 1 && rc.ic1 - rc.ic0 >= 1;
  // the default build ships shape 2 only (any non-zero "cg_big" selects it)
  const int big = TR == 16 && TC == 32 ? k.cg_big : 0;
  const int n_shapes = (int)(sizeof kCgBigShapes / sizeof kCgBigShapes[0]);
  if (!k.experiments) p.shape = big > 0 ? 2 : 0;
  else p.shape = big == kCgWalkTile || (big >= 1 && big <= n_shapes) ? big : 0;
  if (p.split && p.shape) {
    const int* s = kCgBigShapes[(p.shape == kCgWalkTile ? 2 : p.shape) - 1];
    const int rows16 = ((rc.ir1 - rc.ir0) * 16 / s[0]) * s[0] / 16 * 16;  // rows the big tiles cover: whole big tiles AND whole 16-row units
    p.n_btr = rows16 / s[0];
    p.n_btc = (rc.ic1 - rc.ic0) * 32 / s[1];
    if (p.n_btr >= 1 && p.n_btc >= 1 && p.n_btr * s[0] == rows16 && (p.n_btc * s[1]) % 32 == 0) {
      rc.ir1 = rc.ir0 + rows16 / 16;
      rc.ic1 = rc.ic0 + p.n_btc * s[1] / 32;
    } else p.n_btr = p.n_btc = 0;
  }
  p.rc = rc;
  p.inner = p.split ? (rc.ir1 - rc.ir0) * (rc.ic1 - rc.ic0) : 0;
  p.frame = p.tiles_r * p.tiles_c - p.inner;
  // patches of PR x PC tiles per XCD (100 PR + PC): k_cg_tile_mn divides by both sides, so a code with a zero side
  // (100, 200, 400, ...) is the default order, 4 x 2
  const bool patches = k.cg_big_xcd >= 100;
  p.big_xcd = patches && (k.cg_big_xcd / 100 == 0 || k.cg_big_xcd % 100 == 0) ? 402 : k.cg_big_xcd;
  return p;
}

}  // namespace lbm
