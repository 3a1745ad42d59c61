// What the four translation units of the fluid + scalar step with a KBC fluid share on the host (capi_ade_kbc.hip: every
// launch without buoyancy but one; capi_ade_kbc_part.hip: the part kernel of a slab; capi_ade_kbc_buoyant.hip: the forced
// collision; capi_ade_kbc_buoyant_part.hip: its part kernel): the kernels of ade_kbc.hpp, the launch path and the choice of
// the model pair.
#pragma once
#include "ade_kbc.hpp"
#include "ade_launch.hpp"

namespace lbm {

// f(fluid model, scalar model): one form for both halves, lbm_ade_params.form; LBM_FORM_DEFAULT resolves through
// "kbc_fast", as for lbm_kbc_*
template <class F>
static int with_ade_kbc_models(const lbm_kbc_params* kbc, const lbm_ade_params* scalar, F f) {
  const bool fast = scalar->form == LBM_FORM_DEFAULT ? tuning("kbc_fast", 1) != 0 : scalar->form == LBM_FORM_REASSOCIATED;
  if (fast) return f(KbcFastModel(kbc->s2), AdeFastModel(scalar->omega_g, scalar->w_r, scalar->w_c));
  return f(KbcModel{kbc->s2}, AdeModelRef{scalar->omega_g, scalar->w_r, scalar->w_c});
}

}  // namespace lbm
