// What the two translation units of the fluid + scalar step with a KBC fluid share on the host (capi_ade_kbc.hip: checks,
// C ABI and every launch but one; capi_ade_kbc_part.hip: the part kernel of a slab).
#pragma once
#include "ade_call.hpp"
#include "ade_kbc.hpp"

namespace lbm {

// f(fluid model, scalar model): one form for both halves, lbm_ade_params.form; LBM_FORM_DEFAULT resolves through
// "kbc_fast", as for lbm_kbc_*
template <class F>
static int with_ade_kbc_models(const lbm_kbc_params* kbc, const lbm_ade_params* scalar, F f) {
  const bool fast = scalar->form == LBM_FORM_DEFAULT ? tuning("kbc_fast", 1) != 0 : scalar->form == LBM_FORM_REASSOCIATED;
  if (fast) return f(KbcFastModel(kbc->s2), AdeFastModel(scalar->omega_g, scalar->w_r, scalar->w_c));
  return f(KbcModel{kbc->s2}, AdeModelRef{scalar->omega_g, scalar->w_r, scalar->w_c});
}

// capi_ade_kbc.hip: the interior-wall pass of a resolved call over the rows of ade_row_ranges, on `st`; *launches += the
// kernels enqueued (none where those rows hold no table node)
int ade_kbc_iwalls_pass(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old,
                        int band0, int n0, int band1, int nrows, double* rho, double* u, double* conc, hipStream_t st,
                        long long* launches);

// capi_ade_kbc_buoyant.hip: the launches of a resolved call with call.buoyant on a single block -- the collide-only
// iteration, and the step on rows [row_begin, row_end) (interior pair kernel, edge pass with wall edges, interior-wall pass
// with table nodes in those rows; *launches += the kernels enqueued).  The reference order in both halves.
int ade_kbc_buoyant_collide_from(const AdeCall& call, double* fp, double* gp, const double* f, const double* h, double* rho,
                                 double* u, double* conc, hipStream_t st);
int ade_kbc_buoyant_step(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old,
                         int row_begin, int row_end, double* rho, double* u, double* conc, hipStream_t st,
                         long long* launches);

}  // namespace lbm
