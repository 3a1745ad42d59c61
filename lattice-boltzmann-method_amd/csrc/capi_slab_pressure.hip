// C ABI, part 9: pressure-periodic rows (test/horizontal_poiseuille_test.cpp:25-45; the two-block form of
// test/decompose_domain.cpp:50-73) over row slabs, in blocks of D steps.
//
// The virtual rows 0 / Rg-1 of the GLOBAL domain are rewritten every step from the collision of rows Rg-2 / 1
// -- rows that live on the OTHER end slab of the (periodic) ring.  As inside one block (capi_solver.hip
// solver_pressure_block) the 2 D rows on either side of that seam advance D ordinary single steps on a small
// periodic lattice of 4 D rows whose own wrap is the seam, and every row at least D away from the virtual rows
// takes the D-step window.  Over slabs the small lattice is REPLICATED on the two end slabs: both run the whole
// chain (same kernels, same inputs: same bits), each keeps its D rows next to the seam, and per block they swap
// the D rows at distance [D, 2D) from the seam -- far rows of their owner -- in place of that seam's halo (same
// size: 9 D rows of C doubles).  Middle slabs see an ordinary slab with wall columns.  Transport-free like
// capi_slab_ibm.hip: *_compute fills two send buffers, *_finish consumes two receive buffers.
#include <cstring>
#include <new>

#include "blocks.hpp"
#include "d2q9.hpp"
#include "slab.hpp"

using namespace lbm;

// An END slab's place at the pressure seam, in rows (first slab: owns the virtual row 0 / last slab: row Rg - 1).  The small
// lattice holds rows [0, 2D) of the domain, then rows [Rg - 2D, Rg): its own wrap is the seam.
struct SeamEnd {
  int side;             // the message side that crosses the pressure seam: 0 (previous) / 1 (next); -1: a middle slab
  int own, own_s;       // my 2 D rows next to the seam: slab row 0 / R - 2D, small-lattice row 0 / 2D
  int partner_s;        // the partner's 2 D rows in the small lattice: row 2D / 0
  int near, near_s;     // my D rows next to the seam (valid after a block): slab row 0 / R - D, small-lattice row 0 / 3D
  int far, far_s;       // my rows at distance [D, 2D) from the seam: slab row D / R - 2D, small-lattice row D / 2D
  int partner_far_s;    // the partner's rows at that distance (they travel, and wait in the stash): small-lattice row 2D / D
};
static SeamEnd seam_end(bool first, bool last, int R, int D) {
  if (first) return SeamEnd{0, 0, 0, 2 * D, 0, 0, D, D, 2 * D};
  if (last) return SeamEnd{1, R - 2 * D, 2 * D, 0, R - D, 3 * D, R - 2 * D, 2 * D, D};
  return SeamEnd{-1, 0, 0, 0, 0, 0, 0, 0, 0};
}

struct lbm_slab_pressure {
  int model;               // LBM_MODEL_BGK / LBM_MODEL_KBC
  lbm_kbc_params kprm;     // KBC: blocks of 2 steps, far rows through the reference-order 2-step window
  double *sm0, *sm1;       // KBC: the held moments of the small lattice's rows for the driver's first iteration
  lbm_geom g;
  int row0, rows_global, D;
  lbm_bc bc_seam, bc_far;  // the small lattice's edges (= the domain's, pressure rows on); this slab's far rows (HALO rows, no pressure rows)
  lbm_bgk_params prm;
  bool first, last;        // owns the virtual row 0 / Rg - 1
  SeamEnd se;
  lbm_geom sg;             // small lattice: rows [0, 2D) of the domain, then rows [Rg - 2D, Rg)
  double* slat[2];
  int scur;
  double* stash;           // [9][D][C]: the partner's rows at distance [D, 2D) from the seam
  SideStream aux;          // the small lattice's chain, beside the far rows on the caller's stream
};

extern "C" {

int lbm_slab_pressure_info(const lbm_slab_pressure* sl, int* R, int* C, int* ghost, int* depth) {
  LBM_REQUIRE(sl, "lbm_slab_pressure_info: NULL slab");
  if (R) *R = sl->g.R;
  if (C) *C = sl->g.C;
  if (ghost) *ghost = sl->g.ghost;
  if (depth) *depth = sl->D;
  return LBM_OK;
}

int lbm_slab_pressure_destroy(lbm_slab_pressure* sl) {
  if (!sl) return LBM_OK;
  sl->aux.destroy();
  for (double* p : {sl->slat[0], sl->slat[1], sl->stash, sl->sm0, sl->sm1})
    if (p) (void)hipFree(p);
  delete sl;
  return LBM_OK;
}

static int slab_pressure_create(lbm_slab_pressure** out, const lbm_geom* slab, int slab_row0, int rows_global,
                                const lbm_bc* bc_global, const lbm_bgk_params* prm, const lbm_kbc_params* kprm, int depth);

int lbm_slab_pressure_create(lbm_slab_pressure** out, const lbm_geom* slab, int slab_row0, int rows_global,
                             const lbm_bc* bc_global, const lbm_bgk_params* prm, int depth) {
  LBM_REQUIRE(prm, "lbm_slab_pressure_create: NULL argument");
  return slab_pressure_create(out, slab, slab_row0, rows_global, bc_global, prm, nullptr, depth);
}

// KBC + pressure-periodic rows (test/ulbm_poiseuille.cpp:36-58, :85-139) over slabs: blocks of 2 steps (the depth of the
// reference-order KBC window, as on one block); the driver's first iteration collides on HELD moments (:85-86), which the
// start-up calls below take per slab
int lbm_slab_pressure_create_kbc(lbm_slab_pressure** out, const lbm_geom* slab, int slab_row0, int rows_global,
                                 const lbm_bc* bc_global, const lbm_kbc_params* prm) {
  LBM_REQUIRE(prm && prm->s2 > 0.0 && prm->s2 <= 2.0, "lbm_slab_pressure_create_kbc: bad parameters");
  return slab_pressure_create(out, slab, slab_row0, rows_global, bc_global, nullptr, prm, 2);
}

static int slab_pressure_create(lbm_slab_pressure** out, const lbm_geom* slab, int slab_row0, int rows_global,
                                const lbm_bc* bc_global, const lbm_bgk_params* prm, const lbm_kbc_params* kprm, int depth) {
  LBM_REQUIRE(out && slab && bc_global, "lbm_slab_pressure_create: NULL argument");
  LBM_REQUIRE(slab->row_pitch == 0 || slab->row_pitch == slab->C, "lbm_slab_pressure_create: dense rows only (row_pitch = %d)", slab->row_pitch);
  const int R = slab->R, C = slab->C, D = depth;
  LBM_REQUIRE(D >= 2 && D <= 5, "lbm_slab_pressure_create: depth=%d (supported: 2..5)", D);
  LBM_REQUIRE(slab->ghost >= D && R >= 6 * D + 8 && C >= 64, "lbm_slab_pressure_create: slab %dx%d with %d ghost rows too small for %d-step blocks", R, C, slab->ghost, D);
  LBM_REQUIRE(slab_row0 >= 0 && slab_row0 + R <= rows_global && R < rows_global,
              "lbm_slab_pressure_create: rows [%d,%d) of %d (a single block runs lbm_solver_step)", slab_row0, slab_row0 + R, rows_global);
  auto col_ok = [](int m) { return m == LBM_EDGE_PERIODIC || bc_is_wall(m); };
  LBM_REQUIRE(bc_global->pressure_rows == 1 && bc_global->row_lo == LBM_EDGE_PERIODIC && bc_global->row_hi == LBM_EDGE_PERIODIC &&
                  col_ok(bc_global->col_lo) && col_ok(bc_global->col_hi) && !bc_mixed_axis(make_bc(bc_global)),
              "lbm_slab_pressure_create: needs pressure rows on periodic row edges and periodic / wall columns");
  lbm_slab_pressure* sl = new (std::nothrow) lbm_slab_pressure();
  LBM_REQUIRE(sl, "lbm_slab_pressure_create: out of host memory");
  sl->g = *slab;
  sl->row0 = slab_row0;
  sl->rows_global = rows_global;
  sl->D = D;
  sl->model = kprm ? LBM_MODEL_KBC : LBM_MODEL_BGK;
  if (prm) sl->prm = *prm;
  if (kprm) {
    sl->kprm = *kprm;
    sl->kprm.form = LBM_FORM_REFERENCE_ORDER;  // lattices with pressure rows keep the reference order on every path
  }
  sl->bc_seam = *bc_global;
  sl->bc_far = *bc_global;
  sl->bc_far.pressure_rows = 0;
  sl->bc_far.row_lo = sl->bc_far.row_hi = LBM_EDGE_HALO;  // every seam of the ring, the periodic one included
  sl->first = slab_row0 == 0;
  sl->last = slab_row0 + R == rows_global;
  sl->se = seam_end(sl->first, sl->last, R, D);
  if (!sl->first && !sl->last) {
    *out = sl;
    return LBM_OK;
  }
  sl->sg = lbm_geom{4 * D, C, 0, (long long)4 * D * C + 1088};
  const size_t lat_bytes = (size_t)sl->sg.plane_stride * 9 * sizeof(double), stash_bytes = (size_t)9 * D * C * sizeof(double);
  hipError_t e = hipSuccess;
  for (double** p : {&sl->slat[0], &sl->slat[1]}) {
    if (e == hipSuccess) e = hipMalloc(p, lat_bytes);
    if (e == hipSuccess) e = hipMemset(*p, 0, lat_bytes);
  }
  if (e == hipSuccess) e = hipMalloc(&sl->stash, stash_bytes);
  if (e == hipSuccess) e = hipMemset(sl->stash, 0, stash_bytes);
  if (kprm) {
    if (e == hipSuccess) e = hipMalloc(&sl->sm0, (size_t)4 * D * C * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&sl->sm1, (size_t)8 * D * C * sizeof(double));
  }
  const int rc = e == hipSuccess ? sl->aux.create() : LBM_OK;
  if (e != hipSuccess) set_error("lbm_slab_pressure_create: %s", hipGetErrorString(e));
  if (e != hipSuccess || rc) {
    lbm_slab_pressure_destroy(sl);
    return LBM_ERR_HIP;
  }
  *out = sl;
  return LBM_OK;
}

// doubles of the message towards `side` (0 = previous slab, 1 = next; the ring is periodic): per block every
// message is 9 D rows; the start-up message across the pressure seam carries the 2 D rows next to it
long long lbm_slab_pressure_msg_doubles(const lbm_slab_pressure* sl, int side, int start) {
  if (!sl) return -1;
  const bool seam = (side == 0 && sl->first) || (side == 1 && sl->last);
  // (KBC start-up across the pressure seam: the 2 D rows AND their held moments m0, m1: 9 + 3 planes)
  const int planes = (start && seam && sl->model == LBM_MODEL_KBC) ? 12 : 9;
  return (long long)planes * (start && seam ? 2 * sl->D : sl->D) * sl->g.C;
}

// the start-up message of one side from the PRE-collision state: the complete D-row halo across an ordinary seam, my 2 D rows
// next to it across the pressure seam
static int start_pack_side(lbm_slab_pressure* sl, const double* pre, double* send, int side, lbm_stream_t s) {
  if (side != sl->se.side) return lbm_halo_pack(send, pre, &sl->g, LBM_HALO_FULL(sl->D), side, s);
  const lbm_geom mg = msg_geom(2 * sl->D, sl->g.C);
  return lbm_rows_copy(send, &mg, 0, pre, &sl->g, sl->se.own, 2 * sl->D, s);
}
// the small lattice at start-up, pre-collision: my 2 D rows from the slab, the partner's from its message
static int start_fill_small(lbm_slab_pressure* sl, const double* pre, const double* recv, lbm_stream_t s) {
  const int D = sl->D;
  const lbm_geom mg = msg_geom(2 * D, sl->g.C);
  double* sp = sl->slat[sl->scur];
  const int rc = lbm_rows_copy(sp, &sl->sg, sl->se.own_s, pre, &sl->g, sl->se.own, 2 * D, s);
  return rc ? rc : lbm_rows_copy(sp, &sl->sg, sl->se.partner_s, recv, &mg, 0, 2 * D, s);
}
// ... and once it is collided: my 2 D rows into `post`, the partner's rows at distance [D, 2D) from the seam into the stash
static int start_take_small(lbm_slab_pressure* sl, double* post, lbm_stream_t s) {
  const int D = sl->D;
  const double* so = sl->slat[sl->scur];
  const lbm_geom dg = msg_geom(D, sl->g.C);
  const int rc = lbm_rows_copy(post, &sl->g, sl->se.own, so, &sl->sg, sl->se.own_s, 2 * D, s);
  return rc ? rc : lbm_rows_copy(sl->stash, &dg, 0, so, &sl->sg, sl->se.partner_far_s, D, s);
}

// start-up, on the driver's PRE-collision state: complete D-row halos across ordinary seams, the 2 D rows next to
// the pressure seam across that one
int lbm_slab_pressure_start_pack(lbm_slab_pressure* sl, const double* pre, double* send_prev, double* send_next, lbm_stream_t s) {
  LBM_REQUIRE(sl && pre && send_prev && send_next, "lbm_slab_pressure_start_pack: NULL argument");
  LBM_REQUIRE(sl->model == LBM_MODEL_BGK, "lbm_slab_pressure_start_pack: a KBC slab starts with lbm_slab_pressure_start_pack_kbc (held moments)");
  const int rc = start_pack_side(sl, pre, send_prev, 0, s);
  return rc ? rc : start_pack_side(sl, pre, send_next, 1, s);
}

// ... then the driver's first iteration (collision of every row; the virtual rows and their neighbours from the
// small lattice, horizontal_poiseuille_test.cpp:130-140 on the initial state): `post` = post-collision state with
// current ghost rows on the ordinary seams, small lattice primed
int lbm_slab_pressure_start_finish(lbm_slab_pressure* sl, double* post, double* pre, const double* recv_prev,
                                   const double* recv_next, lbm_stream_t s) {
  LBM_REQUIRE(sl && post && pre && post != pre && recv_prev && recv_next, "lbm_slab_pressure_start_finish: bad argument");
  LBM_REQUIRE(sl->model == LBM_MODEL_BGK, "lbm_slab_pressure_start_finish: a KBC slab starts with lbm_slab_pressure_start_finish_kbc");
  const int R = sl->g.R, C = sl->g.C, G = sl->g.ghost, full = LBM_HALO_FULL(sl->D);
  int rc = LBM_OK;
  if (!sl->first) rc = lbm_halo_unpack(pre, recv_prev, &sl->g, full, 0, s);
  if (!rc && !sl->last) rc = lbm_halo_unpack(pre, recv_next, &sl->g, full, 1, s);
  if (rc) return rc;
  const lbm_geom tall{R + 2 * G, C, 0, plane_of(sl->g)};  // all rows, ghost rows included: collision is node-local
  rc = bgk_collide_ref(post, pre, &tall, &sl->prm, as_stream(s));
  if (rc || sl->se.side < 0) return rc;
  rc = start_fill_small(sl, pre, sl->se.side ? recv_next : recv_prev, s);
  if (!rc) rc = lbm_bgk_collide(sl->slat[sl->scur ^ 1], sl->slat[sl->scur], &sl->sg, &sl->bc_seam, &sl->prm, nullptr, nullptr, s);  // incl. the pressure rows
  if (rc) return rc;
  sl->scur ^= 1;
  return start_take_small(sl, post, s);
}

// ---- KBC start-up (ulbm_poiseuille.cpp:85-139 on the initial state: adve_f as given, HELD moments m0 [R][C], m1 [2][R][C]
// of the slab's owned rows).  Across the pressure seam travel the 2 D rows next to it and their moments (12 planes);
// across ordinary seams nothing is needed (the message is the pre-collision halo, unused).  The collision with held
// moments is not node-local in what it needs (the moments of ghost rows live on the neighbour), so ghost rows of `post`
// are NOT current afterwards: exchange complete halos of `post` (LBM_HALO_FULL(2)) over the ordinary seams before the
// first block -- lbm_ring_pressure_start_kbc does.
static int rows_copy_plane(double* dst, const double* src, int n_rows, int C, hipStream_t st) {
  LBM_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)n_rows * C * sizeof(double), hipMemcpyDeviceToDevice, st));
  return LBM_OK;
}

int lbm_slab_pressure_start_pack_kbc(lbm_slab_pressure* sl, const double* pre, const double* m0, const double* m1,
                                     double* send_prev, double* send_next, lbm_stream_t s) {
  LBM_REQUIRE(sl && pre && m0 && m1 && send_prev && send_next, "lbm_slab_pressure_start_pack_kbc: NULL argument");
  LBM_REQUIRE(sl->model == LBM_MODEL_KBC, "lbm_slab_pressure_start_pack_kbc: not a KBC slab");
  const int R = sl->g.R, C = sl->g.C, D = sl->D;
  const size_t n = (size_t)R * C, rows = (size_t)2 * D * C, o = (size_t)sl->se.own * C;
  double* const send[2] = {send_prev, send_next};
  const double* const mom[3] = {m0, m1, m1 + n};  // m0, then the two planes of m1: message planes 9, 10, 11
  for (int side = 0; side < 2; ++side) {
    int rc = start_pack_side(sl, pre, send[side], side, s);
    for (int k = 0; k < 3 && !rc && side == sl->se.side; ++k)
      rc = rows_copy_plane(send[side] + (9 + k) * rows, mom[k] + o, 2 * D, C, as_stream(s));
    if (rc) return rc;
  }
  return LBM_OK;
}

int lbm_slab_pressure_start_finish_kbc(lbm_slab_pressure* sl, double* post, double* pre, const double* m0, const double* m1,
                                       const double* recv_prev, const double* recv_next, lbm_stream_t s) {
  LBM_REQUIRE(sl && post && pre && post != pre && m0 && m1 && recv_prev && recv_next, "lbm_slab_pressure_start_finish_kbc: bad argument");
  LBM_REQUIRE(sl->model == LBM_MODEL_KBC, "lbm_slab_pressure_start_finish_kbc: not a KBC slab");
  const int R = sl->g.R, C = sl->g.C, D = sl->D, G = sl->g.ghost;
  const SeamEnd& se = sl->se;
  // the owned rows on their held moments (kbc::collide with the driver's m0, m1, ulbm.cpp:91-126)
  const lbm_geom own{R, C, 0, plane_of(sl->g)};
  int rc = lbm_kbc_collide_first(post + (size_t)G * C, pre + (size_t)G * C, m0, m1, &own, nullptr, &sl->kprm, s);
  if (rc || se.side < 0) return rc;
  // small lattice, pre-collision, and its held moments likewise: mine from the slab, the partner's from its message
  const double* recv = se.side ? recv_next : recv_prev;
  const size_t n = (size_t)R * C, rows = (size_t)2 * D * C, sn = (size_t)4 * D * C;
  rc = start_fill_small(sl, pre, recv, s);
  double* const small[3] = {sl->sm0, sl->sm1, sl->sm1 + sn};
  const double* const mom[3] = {m0, m1, m1 + n};
  for (int k = 0; k < 3 && !rc; ++k) rc = rows_copy_plane(small[k] + (size_t)se.own_s * C, mom[k] + (size_t)se.own * C, 2 * D, C, as_stream(s));
  for (int k = 0; k < 3 && !rc; ++k) rc = rows_copy_plane(small[k] + (size_t)se.partner_s * C, recv + (9 + k) * rows, 2 * D, C, as_stream(s));
  if (!rc) rc = lbm_kbc_collide_first(sl->slat[sl->scur ^ 1], sl->slat[sl->scur], sl->sm0, sl->sm1, &sl->sg, &sl->bc_seam, &sl->kprm, s);  // incl. the pressure rows (:36-58)
  if (rc) return rc;
  sl->scur ^= 1;
  return start_take_small(sl, post, s);
}

// one block of D steps, phase A: dst from src on the owned rows, both outgoing messages packed
int lbm_slab_pressure_block_compute(lbm_slab_pressure* sl, double* dst, const double* src, double* send_prev,
                                    double* send_next, lbm_stream_t s) {
  LBM_REQUIRE(sl && dst && src && dst != src && send_prev && send_next, "lbm_slab_pressure_block_compute: bad argument");
  const int R = sl->g.R, C = sl->g.C, D = sl->D;
  const SeamEnd& se = sl->se;
  hipStream_t st = as_stream(s), aux = sl->aux.st;
  const bool end = se.side >= 0;
  int rc = end ? sl->aux.fork(st) : LBM_OK;
  if (rc) return rc;
  if (end) {
    double* sp = sl->slat[sl->scur];
    const lbm_geom dg = msg_geom(D, C);
    // the rows at distance [D, 2D) from the seam at time t: mine from the slab, the partner's from the stash
    rc = lbm_rows_copy(sp, &sl->sg, se.far_s, src, &sl->g, se.far, D, aux);
    if (!rc) rc = lbm_rows_copy(sp, &sl->sg, se.partner_far_s, sl->stash, &dg, 0, D, aux);
    if (!rc) rc = seam_chain(sl->slat, &sl->scur, sl->sg, sl->bc_seam, sl->model, sl->prm, sl->kprm, D, aux);
    // my D rows next to the seam (rows [0, D) and [3D, 4D) of the small lattice are valid)
    if (!rc) rc = lbm_rows_copy(dst, &sl->g, se.near, sl->slat[sl->scur], &sl->sg, se.near_s, D, aux);
  }
  // far rows: the D-step window in the reference operation order (lattices with pressure rows keep it on every path)
  const int r0 = sl->first ? D : 0, r1 = sl->last ? R - D : R;
  if (!rc)
    rc = sl->model == LBM_MODEL_KBC ? kbc_stream_collide_x2_ref(dst, src, &sl->g, &sl->bc_far, &sl->kprm, r0, r1, st)
                                    : bgk_stream_collide_xn_ref(dst, src, &sl->g, &sl->bc_far, &sl->prm, D, r0, r1, st);
  if (end) rc = sl->aux.join(st, rc);
  if (!rc) rc = slab_pack_side(send_prev, dst, sl->g, D, 0, se.side == 0, se.far, s);
  if (!rc) rc = slab_pack_side(send_next, dst, sl->g, D, 1, se.side == 1, se.far, s);
  return rc;
}

// phase B: ordinary halos into the ghost rows of dst, the partner's rows into the stash
int lbm_slab_pressure_block_finish(lbm_slab_pressure* sl, double* dst, const double* recv_prev, const double* recv_next, lbm_stream_t s) {
  LBM_REQUIRE(sl && dst && recv_prev && recv_next, "lbm_slab_pressure_block_finish: NULL argument");
  const int rc = slab_finish_side(dst, sl->stash, recv_prev, sl->g, sl->D, 0, sl->se.side == 0, s);
  return rc ? rc : slab_finish_side(dst, sl->stash, recv_next, sl->g, sl->D, 1, sl->se.side == 1, s);
}

}  // extern "C"
