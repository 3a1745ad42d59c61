// The fluid + transported scalar step with the entropic KBC collision as the fluid (lbm_ade_fluid, model =
// LBM_MODEL_KBC), without buoyancy: the launch sites of the interior pair kernel of ade_kbc.hpp and of ade.hpp's edge,
// interior-wall and collide-only kernels with a KBC model as the fluid.  Host checks, C ABI and the dispatch on the fluid
// of a resolved call are capi_ade.hip's (ade_resolve, ade_step_from, ade_collide_from); the sequences are ade_launch.hpp's.
// On a slab the part kernel is launched from capi_ade_kbc_part.hip and the forced collision from
// capi_ade_kbc_buoyant.hip -- units of their own, so that the device code of this one stays what it was; the
// interior-wall pass of a part's rows is launched from here (ade_kbc_iwalls_pass).  The open-boundary pass and the wall
// exchange are capi_ade_kbc_open.hip's; the step runs the open pass before the interior walls (ade_kbc_open_pass).
#include "ade_kbc_call.hpp"

namespace lbm {

// the interior-wall pass of a part's rows: the part unit must not instantiate k_ade_iwalls_ranges
int ade_kbc_iwalls_pass(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, const AdeRows& rows,
                        double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  return with_ade_kbc_models(k.kbc, k.scalar, [&](const auto& fm, const auto& sm) {
    return ade_iwalls_pass<false>(k, fm, sm, fn, gn, fo, go, rows, rho, u, conc, st, launches);
  });
}

// the step on rows [row_begin, row_end) of a single block, with the pair kernel of this fluid
int ade_kbc_step(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, int row_begin, int row_end,
                 double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  return with_ade_kbc_models(k.kbc, k.scalar, [&](const auto& fm, const auto& sm) {
    using FM = std::decay_t<decltype(fm)>;
    using SM = std::decay_t<decltype(sm)>;
    // the g loads before the fluid's collisions for the reassociated pair (measured: 1.3 % faster at 8192^2), after the f
    // stores for the reference-order pair (ade_kbc.hpp G_EARLY; profiles/ade_kbc.txt)
    constexpr bool kEarly = std::is_same<FM, KbcFastModel>::value;
    return ade_step_sequence<false>(k, fm, sm, fn, gn, fo, go, row_begin, row_end, rho, u, conc, st, launches,
        [&](const AdeDispatch& d) {
          with_flags([&](auto NL, auto NS, auto M) {
            LBM_KLAUNCH((k_ade_kbc_stream_collide<FM, SM, NL(), NS(), M(), kEarly>), dim3(d.grid), dim3(256), 0, st, fn, gn, fo,
                        go, k.g, fm, sm, row_begin, row_end, d.tiles, rho, u, conc);
          }, d.nt & 1, d.nt & 2, rho != nullptr);
        },
        [&](const AdeRows& r, long long* n) {  // the open table's listed nodes (capi_ade_kbc_open.hip), then the interior walls'
          if (int rc = ade_kbc_open_pass(k, fn, gn, fo, go, r, rho, u, conc, st, n)) return rc;
          return ade_iwalls_pass<false>(k, fm, sm, fn, gn, fo, go, r, rho, u, conc, st, n);
        });
  });
}

// the collide-only launch (a single block or a slab: the owned rows)
int ade_kbc_collide_from(const AdeCall& k, double* fp, double* gp, const double* f, const double* h, double* rho, double* u,
                         double* conc, hipStream_t st) {
  return with_ade_kbc_models(k.kbc, k.scalar, [&](const auto& fm, const auto& sm) {
    return ade_collide_launch<false>(k, fm, sm, fp, gp, f, h, rho, u, conc, st);
  });
}

}  // namespace lbm
