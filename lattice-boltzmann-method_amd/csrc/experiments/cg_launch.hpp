// EXPERIMENTS: every launch path of the two-phase step that was measured and not kept (DESIGN.md "experiments").  Included
// once by capi_cg.hip, inside namespace lbm, in the LBM_EXPERIMENTS build only; capi_cg.hip reaches it through three hooks,
// each of which answers with a status (it launched, or failed) or with "not mine":
//   cg_exp_one_launch   before the frame / inner split: the column-strip window ("cg_strip") and the merged dispatch ("cg_merge")
//   cg_exp_inner        in the choice of the inner form: big-tile shapes 1 and 3 .. 9, the walking tile ("cg_big" = 10), the
//                       strip kernels of generations 2 to 5 ("cg_strip2" = 1 / 2 / 4, 11 / 12, 21 / 22, 31 / 32)
//   cg_exp_two_steps    in lbm_cg_solver_step: two steps per pass ("cg_depth" = 2)
constexpr bool kCgExperiments = true;
constexpr int kCgNotMine = 1;  // (statuses are <= 0)

// "cg_rows2" = rows per chunk of every strip launch below, else fitted to the resident wave slots of the instance (sw_plan)
template <class Kernel>
static SwPlan cg_exp_chunks(Kernel* kernel, int block_threads, int nrows, int strips, int depth = 3, int rows_unfitted = 64) {
  return sw_plan(kernel, block_threads, nrows, strips, depth, 0, "cg_rows2", rows_unfitted);
}

// ---- before the frame / inner split ---------------------------------------------------------------------------------------
// column-strip sliding window (opt-in: slower as written, cg_fused.hpp), WAVES waves per workgroup
template <int WAVES>
static int launch_cg_strip_t(const CgStepArgs& a, hipStream_t st) {
  int rpc = tuning("cg_rows", 16);
  const int nrows = a.row_end - a.row_begin;
  if (rpc > nrows) rpc = nrows;
  const int strips = (a.g.C + CG_SW - 1) / CG_SW, chunks = (nrows + rpc - 1) / rpc;
  const int n_waves = strips * chunks;
  const dim3 grid((n_waves + WAVES - 1) / WAVES);
  with_flags([&](auto PSI) { LBM_KLAUNCH((k_cg_strip<WAVES, PSI()>), grid, dim3(64 * WAVES), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, a.g, a.bc, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, a.row_begin, a.row_end, rpc, strips, n_waves); }, a.psi != nullptr);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

template <int TR, int TC, int WAVES>
static int cg_exp_one_launch(const CgStepArgs& a, const CgPlan& p, int part, int xs, hipStream_t st) {
  switch (a.g.P != a.g.C ? 0 : tuning("cg_strip", 0)) {  // (dense rows only; whatever the tile, the part and the plan)
    case 0: break;
    case 2: return launch_cg_strip_t<2>(a, st);
    case 4: return launch_cg_strip_t<4>(a, st);
    default: return launch_cg_strip_t<1>(a, st);
  }
  // frame + inner tiles in one dispatch (opt-in: measured level with the two-launch form, 15.24 k either way)
  if (!p.split || part || p.frame <= 0 || tuning("cg_strip2", 0) || !tuning("cg_merge", 0)) return kCgNotMine;
  g_last_inner_form = 0;
  with_flags([&](auto PSI) { LBM_KLAUNCH((k_cg_fused_merged<TR, TC, WAVES, PSI()>), dim3(p.frame + p.inner), dim3(TR * TC), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, a.g, a.bc, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, a.row_begin, a.row_end, xs, p.rc, p.frame); }, a.psi != nullptr);
  LBM_CHECK_LAUNCH();
  return LBM_OK;
}

// ---- the inner rectangle: rows [ra, rb) x columns [ca, cb) ------------------------------------------------------------------
template <int BR, int BC, int BT, int BM, bool BP>
static void cg_exp_big(const CgStepArgs& a, const CgPlan& p, int ra, int ca, hipStream_t st) {
  with_flags([&](auto PSI) { LBM_KLAUNCH((k_cg_tile_mn<BR, BC, BT, BM, BP, PSI()>), dim3(p.n_btr * p.n_btc), dim3(BT), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, a.g, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, ra, ca, p.n_btc, p.big_xcd); }, a.psi != nullptr);
}

// the WALKING tile (k_cg_walk_tile): the 16 x 64 tile advancing through chunks of "cg_walk_rows" rows
static void cg_exp_walk_tile(const CgStepArgs& a, const CgPlan& p, int ra, int ca, hipStream_t st) {
  int rpc = tuning("cg_walk_rows", 128) / 16 * 16;
  if (rpc < 16) rpc = 16;
  const int rows_total = p.n_btr * 16, chunks = (rows_total + rpc - 1) / rpc;
  const int wx = tuning("cg_walk_tile_xcd", 2);
  with_flags([&](auto PSI) { LBM_KLAUNCH((k_cg_walk_tile<PSI()>), dim3(chunks * p.n_btc), dim3(512), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, a.g, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, ra, ca, p.n_btc, rows_total, rpc, wx); }, a.psi != nullptr);
}

// k_cg_strip2 (one wave per SIMD), WV waves per workgroup
// rows per wave: at 16.8 M nodes the launch is only 1-3 rounds of resident waves deep -- a chunk height
// that leaves the last round nearly empty costs up to a whole round; fit it to the resident wave slots
template <int WV>
static void cg_exp_strip2(const CgStepArgs& a, int ra, int rb, int ca, int cb, hipStream_t st) {
  const int strips = (cb - ca + CG_SW2 - 1) / CG_SW2;
  with_flags([&](auto PSI) {
    const SwPlan c = cg_exp_chunks(k_cg_strip2<WV, PSI()>, 64 * WV, rb - ra, strips);
    LBM_KLAUNCH((k_cg_strip2<WV, PSI()>), dim3((c.n_waves + WV - 1) / WV), dim3(64 * WV), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, a.g, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, ra, rb, ca, cb, c.rpc, strips, c.n_waves);
  }, a.psi != nullptr);
}

// k_cg_strip3 (colour sums of the ring rows in LDS, two waves per SIMD), WV waves per workgroup
template <int WV>
static void cg_exp_strip3(const CgStepArgs& a, int ra, int rb, int ca, int cb, hipStream_t st) {
  const int strips = (cb - ca + CG_SW2 - 1) / CG_SW2;
  const int xo = tuning("cg_strip_xcd", 0);  // XCD k takes the k-th contiguous eighth of the strip sequence (measured: no effect)
  with_flags([&](auto PSI) {
    const SwPlan c = cg_exp_chunks(k_cg_strip3<WV, PSI()>, 64 * WV, rb - ra, strips);
    const int nblk = (c.n_waves + WV - 1) / WV, grid = xo ? ((nblk + 7) / 8) * 8 : nblk;
    LBM_KLAUNCH((k_cg_strip3<WV, PSI()>), dim3(grid), dim3(64 * WV), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, a.g, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, ra, rb, ca, cb, c.rpc, strips, c.n_waves, xo);
  }, a.psi != nullptr);
}

// the lockstep block kernel (k_cg_strip4), WV waves per block
template <int WV>
static void cg_exp_strip4(const CgStepArgs& a, int ra, int rb, int ca, int cb, hipStream_t st) {
  constexpr int S = 64 * WV - 2 * CG_S4_EDGE;
  const int win0 = (ca - CG_S4_EDGE) / 16 * 16;  // line-aligned window start; lane CG_S4_EDGE = first possible output
  const int bstrips = (cb - (win0 + CG_S4_EDGE) + S - 1) / S;
  with_flags([&](auto PSI) {
    const int rpc = cg_exp_chunks(k_cg_strip4<WV, PSI()>, 64 * WV, rb - ra, bstrips * WV).rpc;
    const int chunks = (rb - ra + rpc - 1) / rpc;
    LBM_KLAUNCH((k_cg_strip4<WV, PSI()>), dim3(bstrips * chunks), dim3(64 * WV), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, a.g, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, ra, rb, ca, cb, rpc, bstrips, win0);
  }, a.psi != nullptr);
}

// k_cg_strip5 -- private windows, WV adjacent strips per workgroup, a barrier every "cg_sync" rows (0: none)
template <int WV>
static void cg_exp_strip5(const CgStepArgs& a, int ra, int rb, int ca, int cb, hipStream_t st) {
  const int strips = (cb - ca + CG_SW2 - 1) / CG_SW2, groups = (strips + WV - 1) / WV;
  const int sync = tuning("cg_sync", 8);
  with_flags([&](auto PSI) {
    const int rpc = cg_exp_chunks(k_cg_strip5<WV, PSI()>, 64 * WV, rb - ra, groups * WV).rpc;
    const int chunks = (rb - ra + rpc - 1) / rpc;
    LBM_KLAUNCH((k_cg_strip5<WV, PSI()>), dim3(groups * chunks), dim3(64 * WV), 0, st, a.pn_r, a.pn_b, a.in_r, a.in_b, a.g, a.cf, a.rho_r, a.rho_b, a.u, a.psi, a.snu, a.mi, ra, rb, ca, cb, rpc, groups, sync);
  }, a.psi != nullptr);
}

// true: launched on `st` (the caller reads the status).  The big tiles of shape 2 and the walking block ("cg_strip2" =
// 41 .. 47) are the shipped forms: launch_cg_inner has taken them before it asks here.
static bool cg_exp_inner(const CgStepArgs& a, const CgPlan& p, int ra, int rb, int ca, int cb, hipStream_t st) {
  if (p.n_btr) {
    switch (p.shape) {  // the shapes of the round-4 sweep that lost to 16 x 64 (profiles/r04_cg_big_sweep.txt)
      case 1: cg_exp_big<32, 32, 512, 4, true>(a, p, ra, ca, st); break;    // 2 nodes per thread, the second parked in LDS: 2 workgroups per CU
      case 3: cg_exp_big<16, 128, 1024, 4, true>(a, p, ra, ca, st); break;  // 1024 threads: one workgroup per CU
      case 4: cg_exp_big<32, 64, 1024, 4, true>(a, p, ra, ca, st); break;
      case 5: cg_exp_big<32, 64, 512, 2, false>(a, p, ra, ca, st); break;   // 4 nodes per thread, 2 waves per SIMD: one workgroup per CU
      case 6: cg_exp_big<8, 64, 512, 4, false>(a, p, ra, ca, st); break;    // one node per thread in the wide shape (what the width alone is worth)
      case 7: cg_exp_big<16, 64, 1024, 4, false>(a, p, ra, ca, st); break;
      case 8: cg_exp_big<16, 128, 512, 2, false>(a, p, ra, ca, st); break;
      case 9: cg_exp_big<16, 32, 512, 4, false>(a, p, ra, ca, st); break;   // the default tile's shape, one node per thread: what the patch orders alone are worth
      case kCgWalkTile: cg_exp_walk_tile(a, p, ra, ca, st); break;
      default: return false;
    }
    g_last_inner_form = 100 + p.shape;
    return true;
  }
  const int s2 = tuning("cg_strip2", 0);
  const int sw4 = a.g.P != a.g.C || s2 >= 41 ? 0 : s2;  // the strip forms know dense rows only
  if ((sw4 == 31 || sw4 == 32) && ca >= 8) {
    if (sw4 == 31) cg_exp_strip5<2>(a, ra, rb, ca, cb, st);
    else cg_exp_strip5<4>(a, ra, rb, ca, cb, st);
  } else if ((sw4 == 21 || sw4 == 22) && a.g.C % 16 == 0 && a.g.plane % 16 == 0 && ca >= 2 * CG_S4_EDGE) {  // needs line-aligned rows and planes
    if (sw4 == 21) cg_exp_strip4<4>(a, ra, rb, ca, cb, st);
    else cg_exp_strip4<8>(a, ra, rb, ca, cb, st);
  } else if (sw4 && sw4 < 21) {  // the inner rectangle through a register-ring strip kernel: 1, 2, 4: k_cg_strip2; 11, 12: k_cg_strip3
    if (sw4 == 2) cg_exp_strip2<2>(a, ra, rb, ca, cb, st);
    else if (sw4 == 1) cg_exp_strip2<1>(a, ra, rb, ca, cb, st);
    else if (sw4 == 11) cg_exp_strip3<1>(a, ra, rb, ca, cb, st);
    else if (sw4 == 12) cg_exp_strip3<2>(a, ra, rb, ca, cb, st);
    else cg_exp_strip2<4>(a, ra, rb, ca, cb, st);
  } else return false;
  g_last_inner_form = sw4;
  return true;
}

// ---- two steps per pass ---------------------------------------------------------------------------------------------------
// k_cg_two_step (cg_fused.hpp) on the nodes whose two-step dependency cone holds plain nodes only -- rows [16, R - 16) x
// columns [32, C - 32) --, and the frame around them through TWO single steps of the ordinary one-launch kernel on two small
// lattices (CgTwoStepBands): a row band (rows [0, 32) then [R - 32, R): its first / last rows ARE the walls, the artificial
// seam in its middle spoils 3 rows per side and step, rows [0, 16) and [48, 64) are copied back) and a column band (columns
// [0, 48) then [C - 48, C): its first / last columns are the pair the driver's same-row column copy couples, :517-523).  The
// band chain runs on a helper stream beside the big launch.  Same kernels per node as two single steps: same bits.
static constexpr int kCgX2RowBand = 16, kCgX2ColBand = 32;  // the frame the two-step kernel leaves out (tile-aligned)
static constexpr int kCgX2HB = 32, kCgX2WB = 48;            // rows / columns per side the band lattices hold (valid after 2 steps: HB - 6, WB - 6)

static bool cg_two_step_applies(const lbm_cg_solver* sv) {
  lbm_bc d;
  lbm_cg_default_bc(&d);
  const lbm_bc& b = sv->bc;
  const bool walls = b.row_lo == d.row_lo && b.row_hi == d.row_hi && b.col_lo == d.col_lo && b.col_hi == d.col_hi && !b.pressure_rows;
  const long long plane = sv->g.plane_stride;
  return walls && sv->g.row_pitch == 0 && sv->g.ghost == 0 && sv->g.C % 16 == 0 && plane % 16 == 0 && sv->g.R >= 2 * kCgX2HB + 64 && sv->g.C >= 2 * kCgX2WB + 256;
}

static int cg_two_step_prepare(lbm_cg_solver* sv) {
  CgTwoStepBands& x = sv->x2;
  if (x.side) return LBM_OK;
  const int R = sv->g.R, C = sv->g.C;
  x.rbg = lbm_geom{2 * kCgX2HB, C, 0, (long long)2 * kCgX2HB * C + 1088};
  x.cbg = lbm_geom{R, 2 * kCgX2WB, 0, (long long)R * 2 * kCgX2WB + 1088};
  for (int b = 0; b < 2; ++b)
    for (int k = 0; k < 2; ++k) {
      LBM_CHECK_HIP(hipMalloc(&x.rband[b][k], (size_t)x.rbg.plane_stride * 9 * sizeof(double)));
      LBM_CHECK_HIP(hipMalloc(&x.cband[b][k], (size_t)x.cbg.plane_stride * 9 * sizeof(double)));
    }
  return x.side.create();
}

// the inner rectangle: two steps in one pass, M = "cg_x2_unroll"
template <int M>
static void cg_two_step_inner(double* const* dst, double* const* src, const Geom& g, const CgFast& cf, hipStream_t st) {
  constexpr int Wv = 4, S = 64 * Wv - 2 * CG_X2_EDGE;
  const int ra = kCgX2RowBand, rb = g.R - kCgX2RowBand, ca = kCgX2ColBand, cb = g.C - kCgX2ColBand;
  const int win0 = (ca - CG_X2_EDGE) / 16 * 16;
  const int bstrips = (cb - (win0 + CG_X2_EDGE) + S - 1) / S;
  const int rpc = cg_exp_chunks(k_cg_two_step<Wv, M>, 64 * Wv, rb - ra, bstrips * Wv, 8, 256).rpc;  // 14 warm-up rows ~ a depth-8 window's
  const int chunks = (rb - ra + rpc - 1) / rpc;
  LBM_KLAUNCH((k_cg_two_step<Wv, M>), dim3(bstrips * chunks), dim3(64 * Wv), 0, st, dst[0], dst[1], src[0], src[1], g, cf, ra, rb, ca, cb, rpc, bstrips, win0);
}

static int cg_solver_step2(lbm_cg_solver* sv) {
  int rc = cg_two_step_prepare(sv);
  if (rc) return rc;
  CgTwoStepBands& x = sv->x2;
  const int R = sv->g.R, C = sv->g.C, HB = kCgX2HB, WB = kCgX2WB;
  double** src = sv->lat[sv->cur];
  double** dst = sv->lat[sv->cur ^ 1];
  hipStream_t st = sv->st, bs = x.side.st;
  rc = x.side.fork(st);
  if (rc) return rc;
  // ---- the frame: copy in, two single steps, on the helper stream ----
  for (int k = 0; k < 2 && !rc; ++k) {
    rc = box_copy(x.rband[0][k], x.rbg, 0, 0, src[k], sv->g, 0, 0, HB, C, bs);
    if (!rc) rc = box_copy(x.rband[0][k], x.rbg, HB, 0, src[k], sv->g, R - HB, 0, HB, C, bs);
    if (!rc) rc = box_copy(x.cband[0][k], x.cbg, 0, 0, src[k], sv->g, 0, 0, R, WB, bs);
    if (!rc) rc = box_copy(x.cband[0][k], x.cbg, 0, WB, src[k], sv->g, 0, C - WB, R, WB, bs);
  }
  for (int t = 0; t < 2 && !rc; ++t) {
    rc = lbm_cg_step_fused(x.rband[t ^ 1][0], x.rband[t ^ 1][1], x.rband[t][0], x.rband[t][1], &x.rbg, &sv->bc, &sv->prm, 0,
                           2 * HB, nullptr, nullptr, nullptr, nullptr, nullptr, bs);
    if (!rc) rc = lbm_cg_step_fused(x.cband[t ^ 1][0], x.cband[t ^ 1][1], x.cband[t][0], x.cband[t][1], &x.cbg, &sv->bc, &sv->prm,
                                    0, R, nullptr, nullptr, nullptr, nullptr, nullptr, bs);
  }
  if (rc) return x.side.join(st, rc);
  // ---- the inner rectangle: two steps in one pass, on the caller's stream ----
  {
    const Geom g = make_geom(sv->g);
    const CgFast cf = make_cg_fast(make_cg_consts(sv->prm));
    switch (tuning("cg_x2_unroll", 0) & 3) {
      case 0: cg_two_step_inner<0>(dst, src, g, cf, st); break;
      case 1: cg_two_step_inner<1>(dst, src, g, cf, st); break;
      case 2: cg_two_step_inner<2>(dst, src, g, cf, st); break;
      default: cg_two_step_inner<3>(dst, src, g, cf, st); break;
    }
    rc = [&]() -> int {
      LBM_CHECK_LAUNCH();
      return LBM_OK;
    }();
  }
  // ---- the frame's valid part into the new lattice (behind the big launch: the regions are disjoint, but one stream writes) ----
  rc = x.side.join(st, rc);
  if (rc) return rc;
  for (int k = 0; k < 2 && !rc; ++k) {
    rc = box_copy(dst[k], sv->g, 0, 0, x.rband[0][k], x.rbg, 0, 0, kCgX2RowBand, C, st);
    if (!rc) rc = box_copy(dst[k], sv->g, R - kCgX2RowBand, 0, x.rband[0][k], x.rbg, 2 * HB - kCgX2RowBand, 0, kCgX2RowBand, C, st);
    if (!rc) rc = box_copy(dst[k], sv->g, 0, 0, x.cband[0][k], x.cbg, 0, 0, R, kCgX2ColBand, st);
    if (!rc) rc = box_copy(dst[k], sv->g, 0, C - kCgX2ColBand, x.cband[0][k], x.cbg, 0, 2 * WB - kCgX2ColBand, R, kCgX2ColBand, st);
  }
  if (rc) return rc;
  sv->cur ^= 1;
  sv->steps += 2;
  ++sv->pair_launches;
  return LBM_OK;
}

// "cg_depth" = 2 (opt-in): two steps per pass while at least three remain (the LAST step of a call writes the observable
// fields: a single step).  Bit-identical and slower: 13.6 k against 15.7-16.1 k MLUPS at 8192 x 2048.
static int cg_exp_two_steps(lbm_cg_solver* sv, bool fused, int steps_left) {
  if (!(fused && tuning("cg_depth", 1) >= 2 && cg_two_step_applies(sv) && sv->post && steps_left >= 3)) return kCgNotMine;
  return cg_solver_step2(sv);
}
