// The fluid + scalar step with a KBC fluid on a PART of a slab: the launch site of k_ade_kbc_stream_collide_part
// (ade_kbc.hpp).  A translation unit of its own: with the part kernel's 32 instantiations in capi_ade_kbc.hip the compiler
// lays out the interior kernel k_ade_kbc_stream_collide of that unit differently (profiles/ade_kbc_slabs.txt), and every
// existing kernel is to stay instruction for instruction what it is.  Host checks and C ABI: capi_ade_kbc.hip.
#include "ade_kbc_call.hpp"

namespace lbm {

// G_EARLY of the part kernel per form (ade_kbc.hpp), each measured on 4 slabs of 2048 x 8192, plain and with walls
// (profiles/ade_kbc_slabs.txt), and not the interior kernel's answer: the reference-order pair runs with the g loads early
// (faster in every repeat), the reassociated pair late (no winner in every repeat, so the variant with fewer registers)
template <class FM>
constexpr bool kAdeKbcPartEarly = !std::is_same<FM, KbcFastModel>::value;

// one dispatch over rows [band0, band0 + n0) and [band1, band1 + nrows - n0), wall fix-ups inline, + the interior-wall
// pass of those rows (capi_ade_kbc.hip): ade_part_launch (capi_ade.hip) with the part kernel of this fluid; no edge pass, no
// open table
template <class FM, class SM>
static int ade_kbc_part_launch(const AdeCall& k, const FM& fm, const SM& sm, double* fn, double* gn, const double* fo,
                               const double* go, int band0, int n0, int band1, int nrows, double* rho, double* u,
                               double* conc, hipStream_t st) {
  const bool mom = rho != nullptr;
  const int nt = tuning("nt", 3);  // as the single-block step
  const int cap = tuning("grid_cap", 0);
  const int tiles = (k.g.C + 511) / 512;
  const long items = (long)nrows * tiles;
  const int grid = cap > 0 ? capped_grid(items, cap) : (int)(items < (1L << 30) ? items : (1L << 30));
  with_flags([&](auto NL, auto NS, auto M, auto F) {
    LBM_KLAUNCH((k_ade_kbc_stream_collide_part<FM, SM, NL(), NS(), M(), F(), kAdeKbcPartEarly<FM>>), dim3(grid), dim3(256), 0, st, fn, gn,
                fo, go, k.g, k.bc, fm, sm, band0, n0, band1, nrows, tiles, rho, u, conc, k.sw);
  }, nt & 1, nt & 2, mom, k.sw.fixed);
  LBM_CHECK_LAUNCH();
  long long launches = 1;
  const int rc = ade_kbc_iwalls_pass(k, fn, gn, fo, go, band0, n0, band1, nrows, rho, u, conc, st, &launches);
  ade_part_launches_add(launches);
  return rc;
}

// one part of a resolved call, after ade_part_args: ade_part_from's rows (capi_ade.hip)
int ade_kbc_part_from(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, int part,
                      int edge_rows, double* rho, double* u, double* conc, hipStream_t st) {
  const int R = k.g.R;
  // FRAME: rows [0, E) then [R - E, R); INNER: rows [E, R - E)
  const int band0 = part == LBM_ADE_PART_FRAME ? 0 : edge_rows;
  const int n0 = part == LBM_ADE_PART_FRAME ? edge_rows : R - 2 * edge_rows;
  const int band1 = R - edge_rows, nrows = part == LBM_ADE_PART_FRAME ? 2 * edge_rows : n0;
  return with_ade_kbc_models(k.kbc, k.scalar, [&](const auto& fm, const auto& sm) {
    return ade_kbc_part_launch(k, fm, sm, fn, gn, fo, go, band0, n0, band1, nrows, rho, u, conc, st);
  });
}

}  // namespace lbm
