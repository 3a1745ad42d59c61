// The fluid + scalar step with a KBC fluid and BUOYANCY (lbm_ade_buoyancy with beta != (0, 0)): the launch sites of every
// kernel with the forced KBC collision but the part kernel of a slab (capi_ade_kbc_buoyant_part.hip) -- the buoyant interior
// pair kernel of ade_kbc.hpp and the BUOYANT instantiations of ade.hpp's collide-only, edge and interior-wall kernels with
// KbcModel as the fluid (ade_forced_fluid: collide_with on the shifted u); the interior-wall pass serves a single block's
// rows and a part's (ade_kbc_buoyant_iwalls_pass).  A translation unit of its own, so that the device code of
// capi_ade_kbc.hip and capi_ade_kbc_part.hip stays what it was.  A buoyant step runs the reference order in both halves
// whatever `form` says: KbcModel + AdeModelRef.  Called from capi_ade.hip (ade_step_from, ade_collide_from) with a call
// ade_resolve resolved; the sequences are ade_launch.hpp's.
#include "ade_kbc_call.hpp"

namespace lbm {

// the interior-wall pass of a part's rows: the buoyant part unit must not instantiate k_ade_iwalls_ranges
int ade_kbc_buoyant_iwalls_pass(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go,
                                const AdeRows& rows, double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  const KbcModel fm{k.kbc->s2};
  const AdeModelRef sm{k.scalar->omega_g, k.scalar->w_r, k.scalar->w_c};
  return ade_iwalls_pass<true>(k, fm, sm, fn, gn, fo, go, rows, rho, u, conc, st, launches);
}

// the collide-only launch (the first driver iteration; a single block or a slab: the owned rows)
int ade_kbc_buoyant_collide_from(const AdeCall& k, double* fp, double* gp, const double* f, const double* h, double* rho,
                                 double* u, double* conc, hipStream_t st) {
  const KbcModel fm{k.kbc->s2};
  const AdeModelRef sm{k.scalar->omega_g, k.scalar->w_r, k.scalar->w_c};
  return ade_collide_launch<true>(k, fm, sm, fp, gp, f, h, rho, u, conc, st);
}

// the step on rows [row_begin, row_end), with the buoyant kernels
int ade_kbc_buoyant_step(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, int row_begin,
                         int row_end, double* rho, double* u, double* conc, hipStream_t st, long long* launches) {
  const KbcModel fm{k.kbc->s2};
  const AdeModelRef sm{k.scalar->omega_g, k.scalar->w_r, k.scalar->w_c};
  return ade_step_sequence<true>(k, fm, sm, fn, gn, fo, go, row_begin, row_end, rho, u, conc, st, launches,
      [&](const AdeDispatch& d) {
        with_flags([&](auto NL, auto NS, auto M) {
          LBM_KLAUNCH((k_ade_kbc_stream_collide_buoyant<KbcModel, AdeModelRef, NL(), NS(), M()>), dim3(d.grid), dim3(256), 0, st,
                      fn, gn, fo, go, k.g, fm, sm, row_begin, row_end, d.tiles, rho, u, conc, k.by);
        }, d.nt & 1, d.nt & 2, rho != nullptr);
      },
      [&](const AdeRows& r, long long* n) {  // the open table's listed nodes (capi_ade_kbc_open.hip), then the interior walls'
        if (int rc = ade_kbc_open_pass(k, fn, gn, fo, go, r, rho, u, conc, st, n)) return rc;
        return ade_iwalls_pass<true>(k, fm, sm, fn, gn, fo, go, r, rho, u, conc, st, n);
      });
}

}  // namespace lbm
