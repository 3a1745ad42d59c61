// The fluid + scalar step with a KBC fluid and BUOYANCY on a PART of a slab: the launch site of
// k_ade_kbc_stream_collide_part_buoyant (ade_kbc.hpp).  A translation unit of its own, so that the device code of
// capi_ade_kbc.hip, capi_ade_kbc_part.hip and capi_ade_kbc_buoyant.hip stays what it was; this unit holds the buoyant part
// kernel alone -- the interior-wall pass of a part's rows is launched from capi_ade_kbc_buoyant.hip, where the BUOYANT
// k_ade_iwalls_ranges with KbcModel is instantiated already (ade_kbc_buoyant_iwalls_pass).  A buoyant step runs the
// reference order in both halves whatever `form` says: KbcModel + AdeModelRef.  Host checks, C ABI and the dispatch on the
// fluid: capi_ade.hip (ade_part_from); the sequence: ade_launch.hpp.
#include "ade_kbc_call.hpp"

namespace lbm {

// one part of a resolved call with call.buoyant, after ade_part_args; no open table.  With LBM_EXPERIMENTS the knob
// "kbc_part_g_fenced" picks the candidate order (the g loads behind a fence after the fluid's moments)
int ade_kbc_buoyant_part_from(const AdeCall& k, double* fn, double* gn, const double* fo, const double* go, int part,
                              int edge_rows, double* rho, double* u, double* conc, hipStream_t st) {
  const KbcModel fm{k.kbc->s2};
  const AdeModelRef sm{k.scalar->omega_g, k.scalar->w_r, k.scalar->w_c};
  return ade_part_sequence(k, part, edge_rows,
      [&](const AdeDispatch& d, const AdeRows& r) {
#ifdef LBM_EXPERIMENTS
        if (tuning("kbc_part_g_fenced", 0)) {
          with_flags([&](auto NL, auto NS, auto M, auto F) {
            LBM_KLAUNCH((k_ade_kbc_stream_collide_part_buoyant<KbcModel, AdeModelRef, NL(), NS(), M(), F(), true>), dim3(d.grid),
                        dim3(256), 0, st, fn, gn, fo, go, k.g, k.bc, fm, sm, r.band0, r.n0, r.band1, r.nrows, d.tiles, rho, u, conc,
                        k.sw, k.by);
          }, d.nt & 1, d.nt & 2, rho != nullptr, k.sw.fixed);
          return;
        }
#endif
        with_flags([&](auto NL, auto NS, auto M, auto F) {
          LBM_KLAUNCH((k_ade_kbc_stream_collide_part_buoyant<KbcModel, AdeModelRef, NL(), NS(), M(), F()>), dim3(d.grid), dim3(256),
                      0, st, fn, gn, fo, go, k.g, k.bc, fm, sm, r.band0, r.n0, r.band1, r.nrows, d.tiles, rho, u, conc, k.sw, k.by);
        }, d.nt & 1, d.nt & 2, rho != nullptr, k.sw.fixed);
      },
      [&](const AdeRows& r, long long* n) { return ade_kbc_buoyant_iwalls_pass(k, fn, gn, fo, go, r, rho, u, conc, st, n); });
}

}  // namespace lbm
