// Host-only helper for the test-suite: the tile plan of the fused two-phase step (csrc/cg_plan.hpp) for the default
// 16 x 32 tile, one JSON line per case.  No GPU, no liblbm_hip.  Cases on stdin, one per line:
//   R C ghost lo_halo hi_halo row_begin row_end part edge_rows cg_split cg_big cg_big_xcd
// A 13th field, if given, is 1 for the plan of the experiments build.
#include <cstdio>

#include "../csrc/cg_plan.hpp"

int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    int R, C, ghost, lo, hi, rb, re, part, edge, split, big, xcd, exper = 0;
    const int n = std::sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d %d", &R, &C, &ghost, &lo, &hi, &rb, &re, &part, &edge,
                              &split, &big, &xcd, &exper);
    if (n <= 0) continue;  // blank line
    if (n < 12 || R < 1 || C < 1 || rb < 0 || rb > re || re > R) {
      std::printf("{\"error\": \"bad case\"}\n");
      return 2;
    }
    const lbm::CgPlan p = lbm::cg_plan({16, 32, R, C, ghost, lo != 0, hi != 0, rb, re, part, edge}, {split, big, xcd, exper != 0});
    std::printf("{\"tiles_r\": %d, \"tiles_c\": %d, \"ir0\": %d, \"ir1\": %d, \"ic0\": %d, \"ic1\": %d, \"split\": %d, \"frame\": %d, "
                "\"inner\": %d, \"n_btr\": %d, \"n_btc\": %d, \"shape\": %d, \"big_xcd\": %d}\n",
                p.tiles_r, p.tiles_c, p.rc.ir0, p.rc.ir1, p.rc.ic0, p.rc.ic1, (int)p.split, p.frame, p.inner, p.n_btr, p.n_btc,
                p.shape, p.big_xcd);
  }
  return 0;
}
