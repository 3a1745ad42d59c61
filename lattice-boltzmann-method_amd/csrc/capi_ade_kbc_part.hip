// The fluid + scalar step with a KBC fluid on a PART of a slab: the launch site of k_ade_kbc_stream_collide_part
// (ade_kbc.hpp).  A translation unit of its own: with the part kernel's 32 instantiations in capi_ade_kbc.hip the compiler
// lays out the interior kernel k_ade_kbc_stream_collide of that unit differently (profiles/ade_kbc_slabs.txt), and every
// existing kernel is to stay instruction for instruction what it is.  Host checks, C ABI and the dispatch on the fluid:
// capi_ade.hip (ade_part_from); the sequence: ade_launch.hpp.
#include "ade_kbc_call.hpp"

namespace lbm {

// G_EARLY of the part kernel per form (ade_kbc.hpp), each measured on 4 slabs of 2048 x 8192, plain and with walls
// (profiles/ade_kbc_slabs.txt), and not the interior kernel's answer: the reference-order pair runs with the g loads early
// (faster in every repeat), the reassociated pair late (no winner in every repeat, so the variant with fewer registers)
template <class FM>
constexpr bool kAdeKbcPartEarly = !std::is_same<FM, KbcFastModel>::value;

// one part of a resolved call, after ade_part_args: the part kernel of this fluid, then the interior-wall pass of the part's
// rows, which capi_ade_kbc.hip launches (this unit holds the part kernel alone); no open table
int ade_kbc_part_from(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, int part,
                      int edge_rows, double* rho, double* u, double* conc, hipStream_t st) {
  return with_ade_kbc_models(k.kbc, k.scalar, [&](const auto& fm, const auto& sm) {
    using FM = std::decay_t<decltype(fm)>;
    using SM = std::decay_t<decltype(sm)>;
    return ade_part_sequence(k, part, edge_rows,
        [&](const AdeDispatch& d, const AdeRows& r) {
          with_flags([&](auto NL, auto NS, auto M, auto F) {
            LBM_KLAUNCH((k_ade_kbc_stream_collide_part<FM, SM, NL(), NS(), M(), F(), kAdeKbcPartEarly<FM>>), dim3(d.grid), dim3(256),
                        0, st, fn, gn, fo, go, k.g, k.bc, fm, sm, r.band0, r.n0, r.band1, r.nrows, d.tiles, rho, u, conc, k.sw);
          }, d.nt & 1, d.nt & 2, rho != nullptr, k.sw.fixed);
        },
        [&](const AdeRows& r, long long* n) { return ade_kbc_iwalls_pass(k, fn, gn, fo, go, r, rho, u, conc, st, n); });
  });
}

}  // namespace lbm
