// The resolved call of the fused fluid + scalar step: for the translation units that launch ade.hpp's kernels
// (capi_ade.hip: the BGK fluid and every host check; capi_ade_kbc.hip, capi_ade_kbc_part.hip, capi_ade_kbc_buoyant.hip,
// capi_ade_kbc_buoyant_part.hip, capi_ade_kbc_open.hip: the KBC fluid), which share their launch path in ade_launch.hpp.  Every other unit keeps a call in an AdeCallBuf
// (internal.hpp) and never sees its members.
#pragma once
#include <type_traits>

#include "ade.hpp"
#include "launch.hpp"

namespace lbm {

// One call of the fused step after its host checks (ade_resolve): the device copies that every launch of the call takes.
// The fluid -- exactly one of fluid, kbc -- and scalar are borrowed for the call (with_ade_models / with_ade_kbc_models
// pick the models per launch).
struct AdeCall {
  Geom g;
  Bc bc;
  AdeWalls sw;
  AdeBuoyancy by;
  bool buoyant;
  const AdeIwallNode* wall_nodes;
  int n_wall_nodes;
  const int* wall_first;  // host: the table's row index (R + 1 entries), NULL without nodes
  const lbm_bgk_params* fluid;  // a BGK fluid: the launches are capi_ade.hip's; NULL for a KBC fluid
  const lbm_kbc_params* kbc;    // a KBC fluid: the launches are capi_ade_kbc(_part, _buoyant, _open).hip's; NULL for a BGK fluid
  const lbm_ade_params* scalar;
  const AdeOpenNode* open_nodes;  // the open-boundary table (lbm_ade_open), NULL without nodes
  const AdeOpenSeg* open_segs;
  int n_open_nodes;
  const int* open_first;   // host: the table's row index (R + 1 entries), NULL without nodes
  const double* carry_in;  // the carry of the call (ade_carry_set)
  double* carry_out;
};
static_assert(sizeof(AdeCall) <= sizeof(AdeCallBuf) && alignof(AdeCall) <= alignof(AdeCallBuf) &&
              std::is_trivially_copyable<AdeCall>::value, "AdeCallBuf (internal.hpp) holds an AdeCall");

// The rows of a launch -- [band0, band0 + n0), then [band1, band1 + nrows - n0) where n0 < nrows -- as two index ranges of
// a table sorted by (r, c), from its row index first[]: nodes [first0, first0 + w0), then from first1 on, w in all
struct AdeRanges {
  int first0, w0, first1, w;
};
inline AdeRanges ade_row_ranges(const int* first, int band0, int n0, int band1, int nrows) {
  const int first0 = first[band0], w0 = first[band0 + n0] - first0, first1 = first[band1];
  return AdeRanges{first0, w0, first1, w0 + (n0 < nrows ? first[band1 + nrows - n0] - first1 : 0)};
}

}  // namespace lbm
