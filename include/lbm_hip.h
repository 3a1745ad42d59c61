/* lbm_hip.h -- C ABI of the MI355X-native D2Q9 lattice-Boltzmann engine (liblbm_hip.so).
 *
 * Drop-in boundary for ONE hot path of cristian-jfv/lattice-boltzmann-method: the
 * collide-then-stream time step of src/solver.cpp and the variants built on it.
 * The reference has no FFI of its own (its "API" is the C++ headers in src/ consumed by
 * the drivers in test/); every entry point below cites the reference interface it
 * replaces.  Plain pointers and sizes only -- no torch / HIP types in the signatures
 * (lbm_stream_t is a hipStream_t passed as void*; NULL = the default stream).
 *
 * DATA LAYOUT.  The reference holds f as contiguous row-major [R][C][Q] f64 ("AoS", q
 * innermost; src/domain.cpp:7-11).  The engine works on Structure-of-Arrays planes
 *     f[q][r][c]   (q slowest, c fastest, f64)
 * so that a wavefront reads 64 consecutive doubles of one population.  lbm_aos_to_soa /
 * lbm_soa_to_aos convert bit-exactly: AoS element ((r*C)+c)*Q+q  <->  SoA q*R*C + r*C + c.
 * Scalar fields: rho[R][C]; vector fields u[2][R][C] (component slowest).
 * A lattice with g ghost rows per side (multi-GPU slabs; g = the steps per launch D, or m x D with one
 * exchange per m launches, 3 for the two-phase step, 1 for the fluid + scalar pair) stores planes of (R+2g) rows: row index r in
 * [-g, R+g) lives at plane offset (r+g)*C; see lbm_geom.
 *
 * All functions return 0 (LBM_OK) or a negative status and never throw; the message of
 * the last failure on the calling thread is lbm_last_error_string().  Calls enqueue work
 * on the given stream and return; nothing allocates inside a step call (graph-capturable).
 */
#ifndef LBM_HIP_H
#define LBM_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LBM_OK 0
#define LBM_ERR_INVALID (-1) /* bad argument (shape, NULL pointer, unknown mode) */
#define LBM_ERR_HIP (-2)     /* a HIP runtime call or kernel launch failed */
#define LBM_ERR_STATE (-3)   /* call not valid in the solver's current state */

typedef void* lbm_stream_t;

const char* lbm_last_error_string(void);
int lbm_abi_version(void);
/* number of visible HIP devices (0 when none); never fails */
int lbm_device_count(void);
int lbm_set_device(int dev);

/* ---- device memory / streams / events (so a C or C++ host needs no HIP headers) ---- */
int lbm_malloc(void** dptr, size_t bytes);
int lbm_free(void* dptr);
int lbm_memset(void* dptr, int value, size_t bytes, lbm_stream_t s);
int lbm_memcpy_h2d(void* dst, const void* src, size_t bytes, lbm_stream_t s);
int lbm_memcpy_d2h(void* dst, const void* src, size_t bytes, lbm_stream_t s);
int lbm_memcpy_d2d(void* dst, const void* src, size_t bytes, lbm_stream_t s);
int lbm_stream_create(lbm_stream_t* s);
int lbm_stream_destroy(lbm_stream_t s);
int lbm_stream_sync(lbm_stream_t s);
int lbm_event_create(void** ev);
int lbm_event_destroy(void* ev);
int lbm_event_record(void* ev, lbm_stream_t s);
int lbm_stream_wait_event(lbm_stream_t s, void* ev); /* work enqueued on s afterwards waits for ev (hipStreamWaitEvent) */
int lbm_event_elapsed_ms(float* ms, void* start, void* stop); /* synchronises on stop */

/* ---- HIP graphs: capture a launch sequence of this library once, replay it per step -----------------
 * Step calls only enqueue kernels, so a launch-bound loop (many small launches per step: small
 * lattices, multi-block topologies) can be captured from a created (non-default) stream and
 * replayed with one submission per step.  Pointers and parameters are frozen at capture time. */
typedef struct lbm_graph lbm_graph;
int lbm_graph_begin_capture(lbm_stream_t s);
int lbm_graph_end_capture(lbm_stream_t s, lbm_graph** out);
int lbm_graph_launch(lbm_graph* g, int times, lbm_stream_t s);
int lbm_graph_destroy(lbm_graph* g);

/* ---- layout converters (device buffers).  Q = 9 (f), 1 (rho), 2 (u) ---------------- */
int lbm_aos_to_soa(double* soa, const double* aos, int R, int C, int Q, lbm_stream_t s);
int lbm_soa_to_aos(double* aos, const double* soa, int R, int C, int Q, lbm_stream_t s);
/* same with an explicit SoA plane stride in doubles (0 = dense R*C), see lbm_geom */
int lbm_aos_to_soa_ex(double* soa, const double* aos, int R, int C, int Q, long long plane_stride,
                      lbm_stream_t s);
int lbm_soa_to_aos_ex(double* aos, const double* soa, int R, int C, int Q, long long plane_stride,
                      lbm_stream_t s);
/* the same with a row pitch on the SoA side (lbm_geom.row_pitch; 0 = dense): node (r, c) of plane q at
 * q * plane_stride + r * row_pitch + c */
int lbm_aos_to_soa_pitched(double* soa, const double* aos, int R, int C, int Q,
                           long long plane_stride, int row_pitch, lbm_stream_t s);
int lbm_soa_to_aos_pitched(double* aos, const double* soa, int R, int C, int Q,
                           long long plane_stride, int row_pitch, lbm_stream_t s);
/* padding (doubles) the engine recommends between population planes of an R x C lattice */
long long lbm_default_plane_pad(int R, int C);

/* ---- unfused parity operators: one per solver:: function (src/solver.hpp:11-36) -----
 * SoA planes without ghost rows.  Unlike the reference outputs are written in
 * place, never re-bound. */
int lbm_calc_rho(double* rho, const double* f, int R, int C, lbm_stream_t s);                 /* solver.cpp:23-26 */
int lbm_calc_u(double* u, const double* f, const double* rho, int R, int C, lbm_stream_t s);  /* solver.cpp:34-37 */
int lbm_calc_incomp_u(double* u, const double* f, int R, int C, lbm_stream_t s);              /* solver.cpp:28-31 */
int lbm_equilibrium(double* feq, const double* u, const double* rho, int R, int C, lbm_stream_t s);        /* :51-62 */
int lbm_incomp_equilibrium(double* feq, const double* u, const double* rho, int R, int C, lbm_stream_t s); /* :39-49 */
int lbm_collision(double* f_coll, const double* f_curr, const double* f_equi, double omega,
                  int R, int C, lbm_stream_t s);                                              /* solver.cpp:65-74 */
int lbm_advect(double* g, const double* f, int R, int C, lbm_stream_t s);                     /* solver.cpp:76-131 */

/* ---- geometry and boundary descriptors ------------------------------------------------ */
typedef struct lbm_geom {
  int R;     /* rows owned by this block / slab (reference dim 0, pairs with c_x) */
  int C;     /* columns (reference dim 1, pairs with c_y) */
  int ghost; /* 0: planes are [R][C] and streaming wraps rows periodically inside the block
                g >= 1: planes are [R+2g][C]; rows -g..-1 and R..R+g-1 are ghost rows owned by the
                neighbouring slabs (1: one step per launch; n: n-step launches; 3: the
                colour-gradient step) */
  long long plane_stride; /* doubles between consecutive population planes; 0 = dense
                             ((R + 2*ghost) * row pitch).  Padding it off a power of two spreads the 18
                             concurrent streams of the fused step over the HBM channels. */
  int row_pitch;          /* doubles between consecutive rows of a plane; 0 = dense (C).  Node (r, c) of plane q
                             lives at q * plane_stride + (r + ghost) * row_pitch + c ("row padding, hidden behind the
                             ABI"): with C a power of two, rows a power of two apart land on the same
                             L2 sets and DRAM pages -- the solver contexts pad their own lattices (lbm_default_row_pitch).
                             Must be even and >= C.  Entry points that take a lattice honour it; buffers of
                             macroscopic fields (rho, u, psi ...) and AoS arrays are always dense. */
} lbm_geom;
/* rows [src_row, src_row + n_rows) of all 9 planes of `src` (geometry sg) into rows [dst_row, ...) of `dst` (geometry dg):
 * a node-addressed copy (row indices in owned-row numbering, ghost rows allowed), so that padded rows / planes and ghost
 * rows on either side do not matter; sg->C == dg->C.  For hosts that hold lattices of their own in a padded layout. */
int lbm_lattice_copy_rows(double* dst, const lbm_geom* dg, int dst_row, const double* src, const lbm_geom* sg,
                          int src_row, int n_rows, lbm_stream_t s);
/* the row pitch the solver contexts use for a lattice of C columns: C + 64 doubles where C * 8 bytes is a multiple
 * of 4 KiB and C >= 1024 (tuning "row_pad": that many doubles instead of 64, 0 = never), else C */
int lbm_default_row_pitch(int C);

/* What the reference drivers do to the populations a node cannot receive from inside the
 * domain.  Every mode restates one driver fix-up (all applied post-streaming, reading the
 * post-collision populations of the SAME node). */
enum lbm_edge_mode {
  LBM_EDGE_PERIODIC = 0,     /* nothing: solver::advect's own wrap (solver.cpp:84-128) */
  LBM_EDGE_HALO = 1,         /* rows only: ghost row is filled by the neighbouring slab */
  LBM_EDGE_BOUNCE_BACK = 2,  /* halfway bounce-back: horizontal_poiseuille_test.cpp:146-152 (columns),
                                mrtcg_rayleigh_taylor.cpp:525-531 (rows) */
  LBM_EDGE_SPECULAR = 3,     /* columns: cylinder_test.cpp:157-163 */
  LBM_EDGE_ABB_VELOCITY = 4, /* rows: anti-bounce-back with wall velocity, cylinder_test.cpp:135-154 */
  LBM_EDGE_WRAP_NOSHIFT = 5  /* columns, rows 1..R-2 only: the colour-gradient driver's same-row column
                                copy, mrtcg_rayleigh_taylor.cpp:517-523 */
};

typedef struct lbm_bc {
  int row_lo, row_hi; /* mode at global row 0 / row R-1 (enum lbm_edge_mode) */
  int col_lo, col_hi; /* mode at column 0 / column C-1 */
  /* pressure-periodic virtual rows, horizontal_poiseuille_test.cpp:25-45 (applied to the
     post-collision rows 0 and R-1 before streaming): 0 = off, 1 = on, using the model's own
     equilibrium (incompressible in that driver, compressible in decompose_domain.cpp:25-48) */
  int pressure_rows;
  double rho_inlet, rho_outlet;
  double uw_r, uw_c; /* wall velocity of LBM_EDGE_ABB_VELOCITY rows (u_w, cylinder_test.cpp:73) */
} lbm_bc;

/* ---- slab halo (multi-GPU): pack the rows a neighbour needs into ONE contiguous message -------
 * depth = ghost rows in use (1: one step per launch, n: n-step launches), or LBM_HALO_TWO_PHASE for
 * the colour-gradient step (3 ghost rows; the second row travels complete because of the driver's
 * same-row column copy, mrtcg_rayleigh_taylor.cpp:517-523).
 * Message = lbm_halo_rows(depth) rows of C doubles: 3 for depth 1, else 9 (depth - 1); 21 two-phase
 * (the block binding of test/decompose_domain.cpp:181-187 generalised).
 * pack  side 1: my last `depth` rows  -> message for the NEXT slab;  side 0: my first rows -> PREVIOUS.
 * unpack side 0: message from the PREVIOUS slab -> ghost rows above row 0;  side 1: from NEXT -> below. */
#define LBM_HALO_TWO_PHASE (-3)
/* all 9 populations of every one of d ghost rows (9 d rows): multi-step launches on slabs whose
 * columns are walls -- the fix-ups of a ghost-row wall node read that node's own populations */
#define LBM_HALO_FULL(d) (100 + (d))
int lbm_halo_rows(int depth);
int lbm_halo_pack(double* buf, const double* lattice, const lbm_geom* g, int depth, int side,
                  lbm_stream_t s);
int lbm_halo_unpack(double* lattice, const double* buf, const lbm_geom* g, int depth, int side,
                    lbm_stream_t s);

/* ---- which implementation of a collision runs (field `form` of the parameter structs below) ----------
 * Every model exists twice: in the reference's OPERATION ORDER (-ffp-contract=off, same expression order:
 * bitwise equal to the CPU oracle) and REASSOCIATED (same mathematics, fewer operations, reciprocals, FMA
 * decided per source expression: agreement to rounding, tolerances in tests/).  The choice is part of the
 * parameters of a solver / a call, so two solvers in one process may differ; LBM_FORM_DEFAULT (0, what a
 * zero-initialised struct holds) = the process-wide default of lbm_set_tuning ("bgk_fast", "kbc_fast",
 * "cg_fused": reassociated unless set to 0).  Lattices with pressure rows, a body force or the
 * incompressible equilibrium always run the reference order. */
#define LBM_FORM_DEFAULT 0
#define LBM_FORM_REFERENCE_ORDER 1
#define LBM_FORM_REASSOCIATED 2

/* ---- BGK (solver.cpp:23-74 fused with :76-131) ---------------------------------------- */
typedef struct lbm_bgk_params {
  double omega;
  int incompressible; /* 0: calc_u + equilibrium; 1: calc_incomp_u + incomp_equilibrium */
  int delta_form;     /* how the driver writes the relaxation (different rounding, same maths):
                         0: f* = (1-omega) f + omega feq        solver::collision, solver.cpp:73
                         1: f* = f + (-omega (f - feq))          cylinder_test.cpp:108,123-125 */
  /* constant body force as test/gravity_test.cpp applies it: force_mode = 1:
     u += (force_r, force_c) before the equilibrium (:146), and the source
     S_q = (1 - omega/2) w_q [(guo_a + guo_b c_q.u)(c_q.F) - guo_a u.F] (:154, (1/3, 1/9) there) is
     added to the post-collision populations: f* = f + (-omega (f - feq)) + S (:158-160);
     implies delta_form.  force_mode = 0: off. */
  int force_mode;
  double force_r, force_c, guo_a, guo_b;
  int form; /* LBM_FORM_*: REASSOCIATED on a delta_form lattice = the reassociated model standing in for the delta
               form (<= 1e-10 relative, not bitwise; the process-wide default needs "bgk_fast_delta" = 1 for that) */
} lbm_bgk_params;

/* P = collide(f): moments, equilibrium, collision of every node in place of one driver
 * iteration's calc_rho..collision calls; local, no streaming.  rho/u may be NULL. */
int lbm_bgk_collide(double* p, const double* f, const lbm_geom* g, const lbm_bc* bc,
                    const lbm_bgk_params* prm, double* rho, double* u, lbm_stream_t s);
/* The hot loop: p_new = collide(stream(p_old)) for rows [row_begin, row_end), boundary
 * fix-ups included.  p_old holds POST-collision populations (f_coll of the reference);
 * streaming happens at read time (pull).  rho/u (may be NULL) receive the moments of the
 * streamed state, i.e. what calc_rho/calc_u return at the top of the next driver iteration. */
int lbm_bgk_stream_collide(double* p_new, const double* p_old, const lbm_geom* g,
                           const lbm_bc* bc, const lbm_bgk_params* prm, int row_begin,
                           int row_end, double* rho, double* u, lbm_stream_t s);
/* Temporal blocking: p_new = TWO applications of the step above in one launch (an LDS tile keeps
 * the intermediate lattice on chip: 72 instead of 144 HBM bytes per lattice update; every node
 * undergoes the same arithmetic, results are bit-identical to two single steps).  Periodic or
 * ghost-row edges only (ghost = 0 or 2; with 2 the caller keeps TWO ghost rows per side current),
 * C % 64 == 0. */
int lbm_bgk_stream_collide_x2(double* p_new, const double* p_old, const lbm_geom* g,
                              const lbm_bc* bc, const lbm_bgk_params* prm, int row_begin,
                              int row_end, lbm_stream_t s);
/* Deeper temporal blocking: p_new = n_steps (2..6) applications of the step in one launch with
 * the register sliding-window kernel (a wavefront walks down a 64-column strip keeping the last
 * three rows of every intermediate step in registers; no LDS).  One lattice read + one write per
 * n_steps updates; results identical to n_steps single-step launches.  Edges: periodic or ghost rows
 * (ghost = 0 or >= n_steps); also bounce-back / specular columns and bounce-back / anti-bounce-back-
 * velocity rows (n_steps <= 5), applied inside the window at every level -- over slabs the ghost
 * rows must then be complete: exchange with LBM_HALO_FULL(n_steps). */
int lbm_bgk_stream_collide_xn(double* p_new, const double* p_old, const lbm_geom* g,
                              const lbm_bc* bc, const lbm_bgk_params* prm, int n_steps,
                              int row_begin, int row_end, lbm_stream_t s);
/* the same on TWO row ranges of equal height in one launch: [row_begin, row_end) and [row_begin2,
 * row_begin2 + (row_end - row_begin)), row_begin2 >= row_end -- the edge rows at both ends of a slab
 * ahead of the halo exchange (block binding, test/decompose_domain.cpp:181-187) */
int lbm_bgk_stream_collide_xn2(double* p_new, const double* p_old, const lbm_geom* g,
                               const lbm_bc* bc, const lbm_bgk_params* prm, int n_steps,
                               int row_begin, int row_end, int row_begin2, lbm_stream_t s);
/* f = stream(p) incl. boundary fix-ups == solver::advect + the driver's post-advect BCs. */
int lbm_stream(double* f, const double* p, const lbm_geom* g, const lbm_bc* bc, lbm_stream_t s);

/* ---- KBC entropic central-moment collision (src/ulbm.cpp; BASELINE config 3) -------------- */
typedef struct lbm_kbc_params {
  double s2; /* ulbm::d2q9::kbc ctor argument (src/ulbm.hpp:23) */
  int form;  /* LBM_FORM_*; multi-step launches exist for the reassociated collision only */
} lbm_kbc_params;
/* kbc::eval_equilibrium (ulbm.cpp:248-263) on SoA m0[R][C], m1[2][R][C].  zero_u2 != 0 is the
 * state in which the driver calls it (ux2 = uy2 = 0 from the ctor, ulbm_double_shear_flow.cpp:96) */
int lbm_kbc_equilibrium(double* feq, const double* m0, const double* m1, int R, int C,
                        int zero_u2, lbm_stream_t s);
/* kbc::collide (ulbm.cpp:91-126) with the moments the caller holds (unit parity) */
int lbm_kbc_collide_given_moments(double* coll, const double* f, const double* m0,
                                  const double* m1, const lbm_kbc_params* prm, int R, int C,
                                  lbm_stream_t s);
/* as the BGK pair above: moments recomputed from the populations
 * (ulbm_double_shear_flow.cpp:141-142), collide, (pull-)stream */
int lbm_kbc_collide(double* p, const double* f, const lbm_geom* g, const lbm_bc* bc,
                    const lbm_kbc_params* prm, double* rho, double* u, lbm_stream_t s);
int lbm_kbc_stream_collide(double* p_new, const double* p_old, const lbm_geom* g,
                           const lbm_bc* bc, const lbm_kbc_params* prm, int row_begin,
                           int row_end, double* rho, double* u, lbm_stream_t s);
/* n_steps = 2..4 time steps per launch (register sliding window, as lbm_bgk_stream_collide_xn) with the
 * reassociated KBC collision; periodic / halo edges, and on a single block bounce-back / specular /
 * velocity walls with n_steps <= 3 */
int lbm_kbc_stream_collide_xn(double* p_new, const double* p_old, const lbm_geom* g,
                              const lbm_bc* bc, const lbm_kbc_params* prm, int n_steps,
                              int row_begin, int row_end, lbm_stream_t s);
/* First iteration of a driver that HOLDS its moments (test/ulbm_poiseuille.cpp:85-86 starts from
 * adve_f = 0 with m0 = 1, m1 = 0): kbc::collide() on the given (m0 [R][C], m1 [2][R][C]) instead of
 * the populations' own moments, single block.  With bc->pressure_rows the KBC flavour of the
 * pressure-periodic rows is applied (ulbm_poiseuille.cpp:36-58: solver::incomp_equilibrium for the
 * imposed density, kbc.iequi_f.pow(-1) as f_equi); lbm_kbc_stream_collide applies it on the later
 * iterations. */
int lbm_kbc_collide_first(double* p, const double* f, const double* m0, const double* m1,
                          const lbm_geom* g, const lbm_bc* bc, const lbm_kbc_params* prm,
                          lbm_stream_t s);

/* ---- colour-gradient two-phase MRT (test/mrtcg_rayleigh_taylor.cpp; BASELINE config 4) ----
 * Two passes per step over post-collision populations of both colours:
 * lbm_cg_stream_moments (stream -> rho_r, rho_b, u) then lbm_cg_stream_collide (5x5 stencils
 * from an LDS tile, MRT + perturbation + recolouring + gravity source).  496 B/LUP + halo. */
typedef struct lbm_cg_colour {
  double rho_0; /* [red]/[blue] initial_density            (src/colour.cpp:12) */
  double alpha; /* alpha                                    (:13) */
  double nu;    /* kinematic_viscosity                      (:15) */
  double beta;  /* interface_thickness_control              (:17) */
} lbm_cg_colour;
typedef struct lbm_cg_params {
  lbm_cg_colour red, blue;
  double sigma;     /* [general] sigma              (mrtcg_rayleigh_taylor.cpp:360) */
  double gravity_r; /* Fg = (gravity_r, gravity_c): Rayleigh-Taylor driver ([general] gravity_magnitude, 0)
                       (:361,:403); static-droplet driver (0, -6.25e-6) (mrtcg_static_droplet.cpp:452) */
  double gravity_c;
  int add_source;   /* 1: the source term built from Fg is added to both colours (:460-464);
                       0: Fg only shifts the velocity, u += Fg/(2 rho) -- the static-droplet driver
                       comments the source out (mrtcg_static_droplet.cpp:513-514) */
  double delta;     /* interface half-width of the s_nu blend; the drivers hard-code 0.1 (:375) */
  int form;         /* LBM_FORM_* for lbm_cg_solver_step: REFERENCE_ORDER = the two-pass kernels (lbm_cg_stream_moments +
                       lbm_cg_stream_collide), REASSOCIATED = the one-launch step (lbm_cg_step_fused) */
} lbm_cg_params;
/* differential::x (dir 0, d/d row) and ::y (dir 1, d/d column): isotropic 5x5 finite
 * differences with replicate padding (src/differential.hpp:9-40, src/differential.cpp:3-33);
 * psi, out: [R][C].  Stand-alone parity operator; the fused step has its own LDS stencil. */
int lbm_diff5(double* out, const double* psi, int R, int C, int dir, lbm_stream_t s);
/* the driver's boundary set (:495-533): bounce-back rows, same-row column copy */
void lbm_cg_default_bc(lbm_bc* bc);
/* eval_equilibrium (:233-247): f[9][R][C] (plane stride as given) from rho_k[R][C], u[2][R][C] */
int lbm_cg_equilibrium(double* f, const double* rho_k, const double* u, const lbm_cg_colour* k,
                       int R, int C, long long plane_stride, lbm_stream_t s);
/* one loop body :431-464 on the GIVEN macroscopic fields and un-streamed populations (the
 * driver's first iteration: u = 0, rho_k = init); writes post-collision col_f of both colours */
int lbm_cg_collide(double* p_r, double* p_b, const double* f_r, const double* f_b,
                   const double* rho_r, const double* rho_b, const double* u, const lbm_geom* g,
                   const lbm_bc* bc, const lbm_cg_params* prm, double* psi /* may be NULL */,
                   double* s_nu /* may be NULL */, lbm_stream_t s);
/* Slabs: populations with lbm_geom.ghost = 3; the macroscopic fields then carry 2 ghost rows per
 * side (rho[(R+4)][C], u[2][(R+4)][C], row r at (r+2)*C): pass A recomputes them on rows -2..R+1
 * from the populations' ghost rows, so ONE population exchange per step (3 rows, both colours)
 * feeds both the streaming and the 5x5 stencils; the stencils clamp at GLOBAL edges only
 * (row_lo/row_hi != LBM_EDGE_HALO).  Single block: ghost = 0, fields [R][C]. */
/* pass A: :466-477 fused -- advect + BCs of both colours, rho_k, u incl. the Fg/(2 rho) shift */
int lbm_cg_stream_moments(double* rho_r, double* rho_b, double* u, const double* p_r,
                          const double* p_b, const lbm_geom* g, const lbm_bc* bc,
                          const lbm_cg_params* prm, lbm_stream_t s);
/* pass B: :431-464 on the streamed populations */
int lbm_cg_stream_collide(double* pn_r, double* pn_b, const double* p_r, const double* p_b,
                          const double* rho_r, const double* rho_b, const double* u,
                          const lbm_geom* g, const lbm_bc* bc, const lbm_cg_params* prm,
                          int row_begin, int row_end, double* psi, double* s_nu, lbm_stream_t s);
/* The whole step :431-477 in ONE launch (what lbm_cg_solver_step runs; tuning "cg_fused" = 0 selects
 * the two passes above).  Same mathematics, reassociated: the MRT operator is applied once to the
 * colour-summed non-equilibrium part (only the sum enters recolouring, :455), divisions by rho and
 * |grad psi| become reciprocals, rho_k / u / psi are rebuilt inside the tile from the streamed
 * populations (no macroscopic arrays are read; 288 B per node update instead of 496).  Results agree
 * with the two-pass form to rounding (see tests/test_gpu_cg.py for the stated tolerance), not bit for
 * bit.  Slabs: populations with 3 ghost rows, exactly as for the two passes.  The five field outputs
 * (rho_r, rho_b, u with the macro layout above; psi, s_nu dense [R][C]) are optional: all or none. */
int lbm_cg_step_fused(double* pn_r, double* pn_b, const double* p_r, const double* p_b,
                      const lbm_geom* g, const lbm_bc* bc, const lbm_cg_params* prm, int row_begin,
                      int row_end, double* rho_r, double* rho_b, double* u, double* psi, double* s_nu,
                      lbm_stream_t s);
/* the same step as TWO launches for a slab whose neighbours wait for its edge rows.  The nodes each part writes (both
 * colours, all 9 planes; the field outputs at the same nodes):
 *   LBM_CG_PART_INNER: one rectangle of whole 16 x 32 tiles through the plain-offset inner kernel, inside rows
 *     [edge_rows, R - edge_rows) and away from the wall rows and the wall / copy columns -- possibly empty;
 *   LBM_CG_PART_FRAME: every other node of [0, R) x [0, C) through the boundary-gather instantiation, so ALWAYS every node
 *     of rows [0, edge_rows) and [R - edge_rows, R) and of columns 0 and C - 1, whatever R % 16 is.
 * Neither writes a ghost row, the row-pitch padding or the plane padding.  The parts are disjoint and may run on two
 * streams at once (lbm_ring_cg_step: frame, pack and exchange on the ring's stream beside the inner launch); together
 * they are lbm_cg_step_fused on [0, R), bit for bit (test/mrtcg_rayleigh_taylor.cpp:431-477 per node).
 * tests/test_gpu_write_sets.py pins both sets. */
#define LBM_CG_PART_FRAME 1
#define LBM_CG_PART_INNER 2
int lbm_cg_step_fused_part(double* pn_r, double* pn_b, const double* p_r, const double* p_b,
                           const lbm_geom* g, const lbm_bc* bc, const lbm_cg_params* prm, int part,
                           int edge_rows, double* rho_r, double* rho_b, double* u, double* psi, double* s_nu,
                           lbm_stream_t s);
/* which kernel the calling thread's last lbm_cg_step_fused launched for the INNER rectangle of the lattice: 102 the
 * 16 x 64 tile kernel with two nodes per thread (the default since round 4; 101, 103..109: other shapes of an EXPERIMENTS
 * build, tuning "cg_big"), 0 the 16 x 32 tile kernel with one node per thread (tuning "cg_big" = 0, and every lattice too
 * small for an inner rectangle), 41..47 the walking block ("cg_big" = 0 and "cg_strip2"), other values the
 * strip kernels of an EXPERIMENTS build; -1 before the first call.  An opt-in form the geometry does not admit falls back to the tile kernel --
 * this says so (tests/test_gpu_cg.py asserts on it). */
int lbm_cg_last_inner_form(void);
/* driver loop context (single block); host arrays in the reference's shapes */
typedef struct lbm_cg_solver lbm_cg_solver;
int lbm_cg_solver_create(lbm_cg_solver** out, const lbm_geom* g, const lbm_bc* bc /* NULL = default */,
                         const lbm_cg_params* prm, lbm_stream_t s);
int lbm_cg_solver_destroy(lbm_cg_solver* sv);
int lbm_cg_solver_set_state(lbm_cg_solver* sv, const double* f_r, const double* f_b,
                            const double* rho_r, const double* rho_b, const double* u);
int lbm_cg_solver_step(lbm_cg_solver* sv, int n_steps);
/* how many two-step passes lbm_cg_solver_step has run so far.  EXPERIMENTS build only (0 otherwise): with tuning "cg_depth" = 2
 * single blocks with the driver's walls (rows >= 128, columns >= 352, multiple of 16) advance TWO steps per pass -- every
 * lattice row read once and written once per two steps (k_cg_two_step), the frame of the lattice through two single steps on
 * two small band lattices; same bits as single steps, measured SLOWER than them, hence not in the default build */
long long lbm_cg_solver_pair_launches(const lbm_cg_solver* sv);
int lbm_cg_solver_get_state(lbm_cg_solver* sv, double* f_r, double* f_b, double* rho_r,
                            double* rho_b, double* u, double* psi, double* s_nu);
int lbm_cg_solver_sync(lbm_cg_solver* sv);

/* ---- immersed boundary, multi-direct forcing (src/ibm.cpp; BASELINE config 5) ---------------
 * The reference loops over the markers on the HOST (~10 ATen launches per marker per forcing
 * iteration, ibm.cpp:166-187).  Here: markers, their 4x4 Peskin weight boxes and a per-node
 * CSR list of (marker, tap) pairs live on the device; one forcing iteration is two kernels
 * (interpolate + force per marker; gather-spread + velocity update per ROI node).  Spreading is
 * a GATHER in marker order, so the sums are bit-reproducible and equal the reference's
 * sequential accumulation -- no atomics.  The boundary is stationary (f_j = -2 rho_j u_j,
 * SURVEY Q10) and the weights keep the reference's transposed kernel (Q9). */
typedef struct lbm_ibm lbm_ibm;
/* x[i], y[i]: marker row / column coordinates (TOML arrays "x", "y", ibm.cpp:78-102);
 * m_max: ibm.hpp:25 default 5 (m_max - 1 forcing iterations); X, Y: lattice size */
int lbm_ibm_create(lbm_ibm** out, const double* x, const double* y, int n_markers, int m_max,
                   int X, int Y);
/* the same for a row slab that owns the whole ROI: X = rows of the slab, which start at global
 * row `row_offset`; x stays in GLOBAL coordinates (weights identical to the single-block ones),
 * lbm_ibm_roi and the u/rho/lattice arguments of the calls below are slab-local */
int lbm_ibm_create_slab(lbm_ibm** out, const double* x, const double* y, int n_markers, int m_max,
                        int X, int Y, int row_offset);
int lbm_ibm_destroy(lbm_ibm* ib);
/* EXTENSION without a reference counterpart (the reference's boundary is stationary, f_j = -2 rho_j u_j,
 * SURVEY Q10): a uniform marker velocity U_b = (Ur, Uc) -- the boundary drags the fluid along,
 * f_j = 2 rho_j (U_b - u_j), marker positions unchanged (a wall sliding in itself / a cylinder seen
 * from a moving frame).  (0, 0) restores the reference behaviour bit for bit. */
int lbm_ibm_set_velocity(lbm_ibm* ib, double Ur, double Uc);
/* region of interest rows [r0, r1), columns [c0, c1)  (ibm.cpp:104-156) */
int lbm_ibm_roi(const lbm_ibm* ib, int* r0, int* r1, int* c0, int* c1);
/* eulerian_force_density (ibm.cpp:158-190): u[2][X][Y], rho[X][Y] device SoA ->
 * F kept inside the context; F_out (may be NULL) receives it as [2][ROI_r][ROI_c] */
int lbm_ibm_force(lbm_ibm* ib, const double* u, const double* rho, double* F_out, lbm_stream_t s);
/* Guo source of the driver on the ROI (cylinder_test.cpp:116-127):
 * p[q][roi] += (1 - omega/2) w_q [ (a + b c_q.u)(c_q.F) - a u.F ]  with the UNcorrected u */
int lbm_ibm_add_source(lbm_ibm* ib, double* p, const lbm_geom* g, const double* u, double omega,
                       double a, double b, lbm_stream_t s);
/* lbm_ibm_force + lbm_ibm_add_source of one time step as TWO launches -- all forcing iterations in one
 * workgroup with its working set in LDS, then the source term on the touched nodes -- instead of
 * 2 (m_max-1) + 2 small dependent ones; bit-identical results.  What the solver context and the slab
 * engines call.  Tuning: "ibm_step_opt" 0 = the round-1 table layout, "ibm_step_split" 0 = source term
 * inside the workgroup, "ibm_step_chain" 1 = the launch chain. */
int lbm_ibm_step(lbm_ibm* ib, double* p, const lbm_geom* g, const double* u, const double* rho,
                 double omega, double a, double b, lbm_stream_t s);
/* F_s = sum over the ROI of F (drag, lift), cylinder_test.cpp:112; host out[2], synchronises */
int lbm_ibm_surface_force(lbm_ibm* ib, double* out2, lbm_stream_t s);

/* ---- solver context: one block, two lattices, the driver loop ----------------------------
 * Replaces the hand-written time loops of the reference drivers (e.g.
 * horizontal_poiseuille_test.cpp:100-153).  The context keeps POST-collision populations
 * resident and streams at read time, so n driver iterations cost one collide-only launch
 * plus n-1 fused launches; get_f streams lazily and returns the reference's f_adve. */
typedef struct lbm_solver lbm_solver;
enum lbm_model { LBM_MODEL_BGK = 0, LBM_MODEL_KBC = 1 };

int lbm_solver_create(lbm_solver** out, int model, const lbm_geom* g, const lbm_bc* bc,
                      const void* params /* lbm_bgk_params* or lbm_kbc_params* */, lbm_stream_t s);
int lbm_solver_destroy(lbm_solver* sv);
/* f_adve of the reference, host AoS [R][C][9] */
int lbm_solver_set_f_aos(lbm_solver* sv, const double* f_host);
int lbm_solver_get_f_aos(lbm_solver* sv, double* f_host);
/* same, device SoA [9][R][C] (no ghost rows) */
int lbm_solver_set_f_soa_dev(lbm_solver* sv, const double* f_dev);
/* KBC only, after set_f: the first iteration collides on these moments (host AoS rho [R][C],
 * u [R][C][2]) instead of the populations' own -- drivers that hold m0 / m1 (ulbm_poiseuille.cpp) */
int lbm_solver_set_moments_aos(lbm_solver* sv, const double* rho_host, const double* u_host);
int lbm_solver_get_f_soa_dev(lbm_solver* sv, double* f_dev);
/* n driver iterations; record_moments != 0: the last one also stores rho/u exactly as the
 * reference's rho/u tensors hold them when its loop has run n iterations */
int lbm_solver_step(lbm_solver* sv, int n, int record_moments);
/* host AoS rho[R][C], u[R][C][2] recorded by the last step(.., 1) */
int lbm_solver_get_moments_aos(lbm_solver* sv, double* rho_host, double* u_host);
int lbm_solver_sync(lbm_solver* sv);
/* how many multi-step blocks lbm_solver_step has launched so far (periodic / wall-bounded windows,
 * immersed-boundary blocks, pressure-row blocks): lets a caller or a test see that steps were fused
 * rather than silently run one per launch; -1 for NULL */
long long lbm_solver_block_launches(const lbm_solver* sv);
/* attach an immersed boundary to a BGK solver: every step then runs lbm_ibm_force on the
 * step's moments and adds the Guo source (a, b) on the ROI, as cylinder_test.cpp:110-127.
 * The solver does not take ownership. */
int lbm_solver_attach_ibm(lbm_solver* sv, lbm_ibm* ib, double guo_a, double guo_b);
/* device pointers of the resident lattices (current post-collision, scratch) for callers
 * that drive lbm_*_stream_collide themselves (benchmarks, multi-GPU slabs) */
int lbm_solver_lattices(lbm_solver* sv, double** cur, double** other, lbm_geom* geom /* may be NULL */);

/* ---- fluid + transported scalar (advection-diffusion; test/rectangle_sedimentation_test.cpp:88-247) -------
 * A second D2Q9 distribution g carried with a compressible BGK fluid f: the scalar's equilibrium is
 * solver::equilibrium(g_equi, u + w, C) with C = calc_rho(g) and u the fluid's velocity (:125), it relaxes with its
 * own BGK rate (:132) and streams like f (:145-146).  Dye, temperature, sediment: passive, or pushing on the fluid through
 * lbm_ade_buoyancy below.
 * One fused pull step per node streams both post-collision lattices, forms rho, u from f and C from g, collides both
 * and writes both (288 B per node update).  Single block (ghost = 0; row slabs: lbm_ade_stream_collide_part and
 * lbm_ring_ade_* below), C even.  Edges: PERIODIC or BOUNCE_BACK rows,
 * PERIODIC, BOUNCE_BACK or SPECULAR columns; g takes exactly the fix-up f takes at a wall, on its own post-collision
 * populations -- a no-flux wall (the driver's bottom wall, :234-236 = :180-182) -- unless lbm_ade_scalar_bc below makes
 * the edge a fixed-concentration wall.  Everything else (HALO, ABB_VELOCITY,
 * WRAP_NOSHIFT, pressure rows, ghost rows) is refused on the host.  The fluid parameters must be the plain
 * compressible model: incompressible = delta_form = force_mode = 0 (a force that follows the scalar: lbm_ade_buoyancy).
 * Both halves run in the form of `scalar->form`
 * (LBM_FORM_DEFAULT resolves through "bgk_fast" as for BGK): REFERENCE_ORDER = solver.cpp's operation order, the fluid
 * half bitwise equal to lbm_bgk_stream_collide; REASSOCIATED = BgkFastModel for f and its counterpart for g. */
typedef struct lbm_ade_params {
  double omega_g;  /* scalar relaxation rate; the driver uses lp.omega / Sc with Sc = 1 (:132) */
  double w_r, w_c; /* velocity added to u in the scalar's equilibrium; the driver adds w_s to BOTH components (:125) */
  int form;        /* LBM_FORM_*, both halves */
} lbm_ade_params;
/* collide only (the first iteration, like lbm_bgk_collide): post-collision fp, gp from pre-collision f, g_in; in
 * place allowed.  rho [R][C], u [2][R][C], conc [R][C] (dense; all or none may be NULL) receive the moments. */
int lbm_ade_collide(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                    const lbm_bgk_params* fluid, const lbm_ade_params* scalar, double* rho, double* u, double* conc,
                    lbm_stream_t s);
/* the fused step on rows [row_begin, row_end): (fn, gn) = collide(stream(fo, go)), wall fix-ups included; one launch,
 * two with wall edges (interior + edge pass).  Lattices distinct and 16-byte aligned, row pitch and plane stride even.
 * rho, u, conc (all or none may be NULL): the moments of the streamed state. */
int lbm_ade_stream_collide(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                           const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar, int row_begin,
                           int row_end, double* rho, double* u, double* conc, lbm_stream_t s);
/* The same step on a PART of a slab, for a slab whose neighbours wait for its edge rows (lbm_ring_ade_step).  One
 * dispatch per part, the wall fix-ups inline: lanes of wall nodes (every node of a wall row; column 0 / C-1 at a wall
 * column) gather with the fix-ups on both lattices, all others take the plain pull -- bit for bit the loads and the
 * arithmetic of lbm_ade_stream_collide.  The nodes each part writes (f and g, all 9 planes; the moments at the same nodes):
 *   LBM_ADE_PART_FRAME: every node of rows [0, edge_rows) and [R - edge_rows, R), both bands in one dispatch;
 *   LBM_ADE_PART_INNER: every node of rows [edge_rows, R - edge_rows).
 * 1 <= edge_rows, 2 x edge_rows < R.  Neither writes a ghost row, the row-pitch padding or the plane padding; the parts are
 * disjoint and may run on two streams at once; together they are lbm_ade_stream_collide on [0, R), bit for bit, in both
 * forms.  Geometries: ghost = 0 with PERIODIC (wrapping) or BOUNCE_BACK rows, as lbm_ade_stream_collide; or ghost >= 1
 * with HALO or BOUNCE_BACK rows (a slab of a chain or ring: a HALO edge reads the ghost row beside it, which the caller
 * keeps current -- lbm_halo_pack / _unpack at depth 1 on both lattices).  Everything else lbm_ade_stream_collide refuses
 * is refused here too, and so are HALO without ghost rows and PERIODIC rows with them. */
#define LBM_ADE_PART_FRAME 1
#define LBM_ADE_PART_INNER 2
int lbm_ade_stream_collide_part(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar, int part,
                                int edge_rows, double* rho, double* u, double* conc, lbm_stream_t s);
/* driver loop context (single block; g->row_pitch and g->plane_stride 0: the context pads its own lattices).
 * set_state takes f_adve, g_adve (host AoS [R][C][9]); step(n) runs n driver iterations, enqueueing only (no
 * allocation, no host synchronisation: a created stream can capture it, lbm_graph_*); get_state returns what the
 * reference loop holds after them: f_adve, g_adve, rho = calc_rho(f_adve), u = calc_u(f_adve, rho) (AoS [R][C][2]),
 * C = calc_rho(g_adve) -- any output may be NULL; synchronises. */
typedef struct lbm_ade_solver lbm_ade_solver;
int lbm_ade_solver_create(lbm_ade_solver** out, const lbm_geom* g, const lbm_bc* bc /* NULL = periodic */,
                          const lbm_bgk_params* fluid, const lbm_ade_params* scalar, lbm_stream_t s);
int lbm_ade_solver_destroy(lbm_ade_solver* sv);
int lbm_ade_solver_set_state(lbm_ade_solver* sv, const double* f_host, const double* g_host);
int lbm_ade_solver_step(lbm_ade_solver* sv, int n_steps);
int lbm_ade_solver_get_state(lbm_ade_solver* sv, double* f_host, double* g_host, double* rho_host, double* u_host,
                             double* conc_host);
int lbm_ade_solver_sync(lbm_ade_solver* sv);
/* device pointers of the resident lattices (current post-collision state, scratch) and their padded geometry */
int lbm_ade_solver_lattices(lbm_ade_solver* sv, double** f_cur, double** g_cur, double** f_other, double** g_other,
                            lbm_geom* geom /* may be NULL */);
/* kernel launches lbm_ade_solver_step has enqueued so far; -1 for NULL */
long long lbm_ade_solver_launches(const lbm_ade_solver* sv);

/* The scalar's walls, per edge in the order row_lo, row_hi, col_lo, col_hi (additive to all of the above; NULL, or every
 * mode NO_FLUX, is the no-flux wall: the same bits and the same launches).
 *   LBM_ADE_SCALAR_NO_FLUX  g takes the fix-up f takes (bounce-back or specular on its own populations);
 *   LBM_ADE_SCALAR_FIXED    a fixed concentration C_w: every population the no-flux wall replaces is replaced by
 *     anti-bounce-back, g[qbar] = -g*[q] + 2 ((1 + 3 c_q.v + 4.5 (c_q.v)^2 - 1.5 v.v) E_q C_w), v = u + w, u the node's
 *     fluid velocity after streaming, g* its own post-collision populations -- the inlet of
 *     test/rectangle_sedimentation_test.cpp:203-218 restricted to the incoming populations; C_w = 0 is its absorbing
 *     obstacle (:221-232).  On a SPECULAR fluid column g pairs q with its opposite all the same.  Corners: rows first,
 *     columns win; each population takes the rule and C_w of the edge that wins it.
 * FIXED needs a wall of the fluid there: a BOUNCE_BACK row, a BOUNCE_BACK or SPECULAR column (never PERIODIC, HALO,
 * ABB_VELOCITY, WRAP_NOSHIFT).  C_w: conc[e], or, where profile[e] is not NULL, a device array (8-byte aligned) of C
 * values on a row edge / R values on a column edge, in the rows of the lattice the call sees (a slab passes its own
 * slice).  The array is read by every step, never copied: rewriting it between graph replays changes the boundary;
 * the descriptor itself is taken by value at each call (a captured graph keeps the one of its capture). */
#define LBM_ADE_SCALAR_NO_FLUX 0
#define LBM_ADE_SCALAR_FIXED 1
typedef struct lbm_ade_scalar_bc {
  int mode[4];              /* LBM_ADE_SCALAR_* */
  double conc[4];           /* C_w of a FIXED edge without a profile; finite */
  const double* profile[4]; /* NULL or device C_w per node along the edge */
} lbm_ade_scalar_bc;
/* lbm_ade_stream_collide / _part with the scalar's walls (sbc may be NULL) */
int lbm_ade_stream_collide_ex(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                              const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                              const lbm_ade_scalar_bc* sbc, int row_begin, int row_end, double* rho, double* u,
                              double* conc, lbm_stream_t s);
int lbm_ade_stream_collide_part_ex(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                   const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                   const lbm_ade_scalar_bc* sbc, int part, int edge_rows, double* rho, double* u,
                                   double* conc, lbm_stream_t s);
/* the context's scalar walls from the next stream on (the lazy one of get_state included); NULL = all NO_FLUX.  Checked
 * against the context's edges; the descriptor is copied, a profile array is not. */
int lbm_ade_solver_set_scalar_bc(lbm_ade_solver* sv, const lbm_ade_scalar_bc* sbc);

/* Buoyancy: the transported scalar drives the fluid (Boussinesq coupling; additive to all of the above).  Per node the
 * force is F = (C - c_ref) (beta_r, beta_c) with the node's own C = calc_rho(g), and the fluid half becomes the body-force
 * collision of test/gravity_test.cpp:141-160 (lbm_bgk_params.force_mode) with that F.  After streaming and the fluid's
 * wall fix-ups, in this order:
 *   1. rho = calc_rho(f), u0 = calc_u(f, rho);
 *   2. the scalar's wall rule (lbm_ade_scalar_bc) with v = u0 + w -- it never sees the shifted velocity;
 *   3. C = calc_rho(g);   4. F = ((C - c_ref) beta_r, (C - c_ref) beta_c);   5. u = u0 + u_shift F;
 *   6. feq = equilibrium(u, rho), S_q = ((1 - 0.5 omega) ((guo_a + guo_b (c_q.u)) (c_q.F) - guo_a (u.F)) w_q),
 *      f* = f + (-omega (f - feq)) + S_q;
 *   7. g* = collision(g, equilibrium(u + w, C)) with the same shifted u.
 * Per collision the force changes the momentum by (omega rho u_shift + (1 - omega / 2) guo_a / 3) F: (u_shift, guo_a,
 * guo_b) = (0.5, 3, 9) is Guo's scheme up to rho ~ 1, (1, 1/3, 1/9) the reference's (gravity_test.cpp:81-82,146,154).
 * A NULL descriptor, or beta_r == 0 && beta_c == 0, is the passive step: the same bits and the same launches.  The forced
 * relaxation is written as a delta form, so it rounds differently from the passive (1 - omega) f + omega feq even as
 * beta -> 0.  A buoyant step always runs the REFERENCE order in both halves, whatever `form` says (the rule for BGK
 * lattices with a body force), costs no launch and no halo traffic of its own, and keeps 288 B per node update.  Every
 * field must be finite; the fluid parameters stay the plain compressible model; everything the passive calls refuse is
 * refused, on the host, before any device call.  The moment outputs of the raw entry points are the values above: u is
 * the shifted u of item 5 (what gravity_test's u holds after :146).  lbm_ade_solver_get_state is unchanged: it returns
 * u = calc_u(f, rho); the velocity that enters the equilibria of the next step is u + u_shift beta (C - c_ref). */
typedef struct lbm_ade_buoyancy {
  double beta_r, beta_c; /* force per unit of (C - c_ref), row / column component */
  double c_ref;
  double u_shift;        /* multiple of F added to u before both equilibria: 1.0 = gravity_test.cpp:146 */
  double guo_a, guo_b;   /* as lbm_bgk_params: (1/3, 1/9) = gravity_test.cpp:81-82,154 */
} lbm_ade_buoyancy;
/* lbm_ade_collide / lbm_ade_stream_collide_ex / _part_ex with the buoyancy; sbc and buoy may each be NULL (the
 * collide-only call checks sbc and applies no wall rule: its input is a pre-collision state) */
int lbm_ade_collide_b(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                      const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                      const lbm_ade_buoyancy* buoy, double* rho, double* u, double* conc, lbm_stream_t s);
int lbm_ade_stream_collide_b(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, int row_begin, int row_end,
                             double* rho, double* u, double* conc, lbm_stream_t s);
int lbm_ade_stream_collide_part_b(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                  const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, int part, int edge_rows,
                                  double* rho, double* u, double* conc, lbm_stream_t s);
/* the context's buoyancy from the next step on; NULL = the passive scalar.  The descriptor is copied; a captured graph
 * keeps the descriptor of its capture. */
int lbm_ade_solver_set_buoyancy(lbm_ade_solver* sv, const lbm_ade_buoyancy* buoy);

/* Interior walls: wall nodes anywhere inside the block (additive to all of the above) -- the obstacle of
 * test/rectangle_sedimentation_test.cpp:184-196 (f) and :220-232 (g), a step, a baffle, a heated plate.  A wall node
 * stays a fluid node, as in the reference: for each named slot s in 1..8 the streamed population s is replaced from the
 * node's OWN post-collision populations, x[s] = x*[opp(s)] -- what a BOUNCE_BACK domain edge does to its three slots.  A
 * slot mask has bit s-1 for slot s; the four axis-aligned facings (c_s of d2q9: rows first) are
 *   LBM_ADE_FACE_ROW_POS  slots 1, 5, 8: fluid on the +row side      LBM_ADE_FACE_ROW_NEG  slots 3, 6, 7
 *   LBM_ADE_FACE_COL_POS  slots 2, 5, 6: fluid on the +column side   LBM_ADE_FACE_COL_NEG  slots 4, 7, 8
 * (the driver's first wall is COL_NEG, its ceiling ROW_NEG, its second wall COL_POS).  f and g take separate masks -- the
 * reference's g first wall runs through the bottom row, its f first wall stops one row short -- and g_mode is the rule
 * of the segment's g slots: LBM_ADE_SCALAR_NO_FLUX the replacement above, LBM_ADE_SCALAR_FIXED the anti-bounce-back of
 * lbm_ade_scalar_bc with C_w = conc, g[s] = -g*[q] + 2 ((((1 + 3 c_q.v) + 4.5 (c_q.v)^2) - 1.5 v.v) E_q) conc, q = opp(s),
 * v = u + w, u the velocity of the node's fully fixed-up f (the unshifted u0 of a buoyant step); conc = 0 is the driver's
 * absorbing rectangle.
 * lbm_ade_iwalls_add names the n >= 1 nodes (r0 + i dr, c0 + i dc), dr, dc in {-1, 0, 1} and not both 0; a negative r0 /
 * c0 counts from the end (-1 = the last row / column).  Either mask may be 0, not both.  Segments may overlap: per node
 * the masks are OR-ed, each g slot keeps one mode and the node one conc -- naming a g slot of a node with two modes, or a
 * node with two FIXED conc values, is refused at add (nothing of the segment is added).  A node may stand on a domain
 * wall: the domain's rule is applied first, the table wins every slot it names and the domain keeps the rest.
 * Everything is checked on the host.  lbm_ade_iwalls_finalize uploads the merged table, sorted by (r, c) -- the one
 * device call; an empty finalized table makes none and behaves like NULL (the same bits, the same launches).  The table
 * is immutable after finalize; steps BORROW it, it is never copied (the rule of lbm_ade_scalar_bc.profile): it must
 * outlive every solver and every captured graph that uses it.
 * The step with a non-empty table costs one more launch: one lane per table node, after the interior launch and the
 * edge pass, overwriting its nodes (rows of [row_begin, row_end) only).  The collide-only first iteration applies no
 * wall rule.  Row slabs take a slab-local table (lbm_ade_iwalls_slab, lbm_ade_stream_collide_part_w, lbm_ring_ade_step_w
 * below). */
#define LBM_ADE_FACE_ROW_POS 0x91u
#define LBM_ADE_FACE_ROW_NEG 0x64u
#define LBM_ADE_FACE_COL_POS 0x32u
#define LBM_ADE_FACE_COL_NEG 0xC8u
typedef struct lbm_ade_iwalls lbm_ade_iwalls;
int lbm_ade_iwalls_create(lbm_ade_iwalls** out, int R, int C);
int lbm_ade_iwalls_add(lbm_ade_iwalls* t, int r0, int c0, int dr, int dc, int n, unsigned f_slots, unsigned g_slots,
                       int g_mode /* LBM_ADE_SCALAR_* */, double conc);
int lbm_ade_iwalls_count(const lbm_ade_iwalls* t); /* distinct nodes so far; host only; 0 for NULL */
/* node i of the merged table, sorted by (r, c); any output may be NULL; host only */
int lbm_ade_iwalls_node(const lbm_ade_iwalls* t, int i, int* r, int* c, unsigned* f_slots, unsigned* g_slots,
                        unsigned* g_fixed_slots, double* conc);
int lbm_ade_iwalls_finalize(lbm_ade_iwalls* t);
int lbm_ade_iwalls_destroy(lbm_ade_iwalls* t);
/* The slab view of a table: a new, ordinary, unfinalized table for an R x C lattice (C the parent's) holding the parent's
 * merged nodes of rows [row0, row0 + R) with r - row0 -- order, slot masks, FIXED slots and conc unchanged.  The parent
 * may be finalized or not and is not modified; the view owns its nodes, takes further lbm_ade_iwalls_add calls (the
 * clash rules hold against the inherited nodes) and is finalized and destroyed like any table.  Host only, no device
 * call.  The wall rule is on-site and its gather reads the slab's ghost rows, so a body that crosses a seam needs no halo
 * data of its own: each slab fixes up the wall nodes it owns. */
int lbm_ade_iwalls_slab(lbm_ade_iwalls** out, const lbm_ade_iwalls* table, int row0, int R);
/* lbm_ade_stream_collide_b with the table (NULL or empty: lbm_ade_stream_collide_b itself); the table must be finalized
 * and built for the R x C of g */
int lbm_ade_stream_collide_w(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                             int row_begin, int row_end, double* rho, double* u, double* conc, lbm_stream_t s);
/* lbm_ade_stream_collide_part_b with a slab-local table: built, or viewed with lbm_ade_iwalls_slab, for the R x C of g,
 * and finalized (NULL or empty: lbm_ade_stream_collide_part_b itself, the same bits and the same launches).  Behind the
 * part's dispatch, on the same stream, one more dispatch recomputes the table's nodes of the part's rows -- one lane per
 * node, found through the row index lbm_ade_iwalls_finalize keeps on the host: no allocation, no host synchronisation,
 * capturable in a graph; a part without a table node enqueues nothing.  FRAME writes the wall nodes of FRAME rows only,
 * INNER those of INNER rows; both read the old lattices only.  The moment outputs of wall nodes are overwritten as well. */
int lbm_ade_stream_collide_part_w(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                  const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                                  int part, int edge_rows, double* rho, double* u, double* conc, lbm_stream_t s);
/* the context's interior walls from the next stream on (the lazy one of get_state included); NULL clears them.  The
 * table is borrowed, not copied. */
int lbm_ade_solver_set_walls(lbm_ade_solver* sv, const lbm_ade_iwalls* iwalls);

/* The fluid of the step by model: the compressible BGK fluid of everything above, or the entropic KBC collision
 * (lbm_kbc_params; src/ulbm.cpp kbc::collide on the populations' own moments, as lbm_kbc_stream_collide runs it) for the
 * regimes BGK does not survive -- a scalar in an under-resolved shear layer, a viscosity with omega next to 2.  The
 * scalar half is unchanged: its equilibrium takes the u the fluid's collision forms.
 * model = LBM_MODEL_BGK: the `_m` calls ARE lbm_ade_collide_b / lbm_ade_stream_collide_w / lbm_ade_solver_create with
 * `bgk` (buoyancy NULL) -- the same checks under those names, the same launches, the same bits.
 * model = LBM_MODEL_KBC: kbc.s2 in (0, 2]; kbc.form LBM_FORM_DEFAULT or equal to scalar->form, which sets both halves
 * (LBM_FORM_DEFAULT resolves through "kbc_fast"): REFERENCE_ORDER = KbcModel with the reference-order scalar, the fluid
 * half bitwise equal to lbm_kbc_stream_collide in that form; REASSOCIATED = KbcFastModel with the reassociated scalar.
 * Supported, single block, ghost = 0, C even: the edge modes of lbm_ade_stream_collide, lbm_ade_scalar_bc (NO_FLUX and
 * FIXED, constant or profile), the interior-wall table, the optional moments, the collide-only first iteration, row
 * ranges, graph capture of the context's step.  Launches as for BGK: one per step on a periodic box (the interior pair
 * kernel written for this fluid, ade_kbc.hpp), one more with wall edges, one more per non-empty table.
 * Refused on the host (LBM_ERR_INVALID, the message names the feature and the model): bc->pressure_rows; on a context
 * lbm_ade_solver_set_buoyancy with beta != (0, 0) (the forced collision is the BGK driver's: the reference has no forced
 * KBC; the forced KBC collision is lbm_ade_solver_set_buoyancy_m's, below), lbm_ade_solver_set_open with a non-empty
 * table, lbm_ade_solver_wall_exchange -- those two keep refusing a KBC context; open boundaries and the wall exchange with
 * this fluid are lbm_ade_open_collide_m / lbm_ade_open_stream_collide_m / lbm_ade_solver_set_open_m and
 * lbm_ade_wallx_rows_m / lbm_ade_solver_wall_exchange_m, below.  Row slabs and the ring: lbm_ade_stream_collide_part_m below, lbm_ring_ade_collide_m / lbm_ring_ade_step_m with the ring. */
typedef struct lbm_ade_fluid {
  int model;          /* LBM_MODEL_BGK or LBM_MODEL_KBC */
  lbm_bgk_params bgk; /* read when model == LBM_MODEL_BGK */
  lbm_kbc_params kbc; /* read when model == LBM_MODEL_KBC */
} lbm_ade_fluid;
int lbm_ade_collide_m(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                      const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc, double* rho,
                      double* u, double* conc, lbm_stream_t s);
int lbm_ade_stream_collide_m(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_iwalls* iwalls, int row_begin, int row_end,
                             double* rho, double* u, double* conc, lbm_stream_t s);
/* One part of a slab's step with either fluid: lbm_ade_stream_collide_part_w's arguments with the fluid by model.
 * model = LBM_MODEL_BGK: IS lbm_ade_stream_collide_part_w with `bgk` and a NULL buoyancy -- the same checks under that
 * name, the same launches, the same bits.
 * model = LBM_MODEL_KBC: the geometries and edges of lbm_ade_stream_collide_part (ghost = 0 with PERIODIC or BOUNCE_BACK
 * rows; ghost >= 1 with HALO or BOUNCE_BACK rows), lbm_ade_scalar_bc, a slab-local interior-wall table
 * (lbm_ade_iwalls_slab) and the optional moments.  ONE dispatch per part -- the part kernel written for this fluid
 * (ade_kbc.hpp: both row bands, wall fix-ups inline, one lattice in registers at a time; there is no edge pass) -- and one
 * more, the interior-wall pass, where the part's rows hold table nodes; both count in lbm_ade_part_launches.  The stored
 * bits are those of lbm_ade_stream_collide_m on one block.  The call only enqueues: no allocation, no host
 * synchronisation, capturable in a graph.  Refused on the host before any device call, the message naming the feature
 * and the model: bc->pressure_rows; a kbc.form that differs from scalar->form.  There is no parameter for buoyancy or
 * for an open view; the wall exchange of a slab's rows with this fluid is lbm_ade_wallx_rows_m. */
int lbm_ade_stream_collide_part_m(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                  const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_iwalls* iwalls, int part, int edge_rows,
                                  double* rho, double* u, double* conc, lbm_stream_t s);
/* the context with either fluid; with a KBC fluid it supports set_state, step, get_state, sync, lattices, launches,
 * set_scalar_bc, set_walls, lbm_ade_solver_diag and lbm_ade_solver_run_until */
int lbm_ade_solver_create_m(lbm_ade_solver** out, const lbm_geom* g, const lbm_bc* bc /* NULL = periodic */,
                            const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, lbm_stream_t s);

/* Buoyancy with the fluid by model: lbm_ade_collide_m / lbm_ade_stream_collide_m with the descriptor of
 * lbm_ade_buoyancy after sbc, and the context's setter for either fluid.
 * model = LBM_MODEL_BGK: the calls ARE lbm_ade_collide_b / lbm_ade_stream_collide_w / lbm_ade_solver_set_buoyancy with
 * `bgk` -- the same checks under those names, the same launches, the same bits.
 * model = LBM_MODEL_KBC: the forced KBC collision.  The reference has no forced KBC and needs none: kbc::collide()
 * collides on the moments the driver HOLDS (src/ulbm.cpp:91-126), and the conserved central moments relax with rate 1
 * (ulbm.cpp:46-49), so colliding on m1 = u0 + u_shift F instead of the populations' own u0 leaves the post-collision
 * momentum at rho (u0 + u_shift F) -- a velocity-shift forcing.  Per node, after streaming and the fluid's wall fix-ups,
 * the list of lbm_ade_buoyancy with item 6 replaced:
 *   1. rho = calc_rho(f), u0 = calc_u(f, rho);
 *   2. the scalar's wall rule (lbm_ade_scalar_bc, the FIXED slots of an interior-wall table) with v = u0 + w;
 *   3. C = calc_rho(g);   4. F = ((C - c_ref) beta_r, (C - c_ref) beta_c);   5. u = u0 + u_shift F;
 *   6. f* = kbc::collide() on the held moments m0 = rho, m1 = u;
 *   7. g* = collision(g, equilibrium(u + w, C)) with the same shifted u.
 * Per collision the momentum changes by exactly rho u_shift F and the mass not at all; the physical velocity is
 * u0 + u_shift F / 2, and u_shift = 1 gives F per step at rho ~ 1.  guo_a and guo_b are NOT read for this fluid (there is
 * no source term); they must still be finite, like every field.  A NULL descriptor or beta = (0, 0) is the passive step of
 * the `_m` calls in either form: the same bits and the same launches.  A buoyant step runs the REFERENCE order in both
 * halves whatever `form` says (KbcModel and the reference-order scalar).  The moment outputs of the raw calls hold the
 * shifted u of item 5; lbm_ade_solver_get_state keeps returning u = calc_u(f, rho).  288 B per node update, no launch of
 * its own (one per step on a periodic box, one more with wall edges, one more per non-empty table), no halo traffic.
 * Refused on the host before any device call, under the `_mb` name: a non-finite field of the descriptor and everything the
 * `_m` calls refuse.  The calls only enqueue; a captured graph keeps the descriptor of its capture.
 * Row slabs and the ring: lbm_ade_slab_stream_collide_mb below, lbm_ring_ade_slab_collide_mb / lbm_ring_ade_slab_step_mb
 * with the ring.  Open boundaries on one block and the wall exchange with a KBC fluid, buoyant or not, are
 * lbm_ade_open_stream_collide_m and lbm_ade_wallx_rows_m below; open boundaries over slabs and the ring stay refused with
 * this fluid, there is no solver context for slabs, and lbm_ade_solver_set_buoyancy itself still refuses beta != (0, 0) on
 * a KBC context. */
int lbm_ade_collide_mb(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                       const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                       const lbm_ade_buoyancy* buoy, double* rho, double* u, double* conc, lbm_stream_t s);
int lbm_ade_stream_collide_mb(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                              const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                              const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                              int row_begin, int row_end, double* rho, double* u, double* conc, lbm_stream_t s);
/* the context's buoyancy for either fluid, from the next step on; NULL = the passive scalar.  The descriptor is copied */
int lbm_ade_solver_set_buoyancy_m(lbm_ade_solver* sv, const lbm_ade_buoyancy* buoy);
/* One part of a slab's step with the fluid by model AND buoyancy: lbm_ade_stream_collide_part_m's arguments with the
 * descriptor of lbm_ade_buoyancy after sbc.  (Its name, like those of the two ring entries lbm_ring_ade_slab_collide_mb /
 * lbm_ring_ade_slab_step_mb, does not continue the lbm_ade_stream_collide_part* family: the set of those names is closed.)
 * model = LBM_MODEL_KBC, beta != (0, 0): the forced collision of the seven-step list above on the part's rows -- the
 * geometries, edges, lbm_ade_scalar_bc, slab-local interior-wall table and optional moments (the shifted u) of
 * lbm_ade_stream_collide_part_m.  ONE dispatch per part, the buoyant part kernel (ade_kbc.hpp: both row bands, wall fix-ups
 * inline, the scalar collided and stored before the fluid's two collisions; there is no edge pass), and one more, the
 * interior-wall pass, where the part's rows hold table nodes; both count in lbm_ade_part_launches.  The reference order in
 * both halves whatever `form` says.  FRAME + INNER store the bits of lbm_ade_stream_collide_mb on one block.  The call only
 * enqueues: no allocation, no host synchronisation, capturable in a graph, which keeps the descriptor of its capture.
 * model = LBM_MODEL_KBC, NULL descriptor or beta = (0, 0): the passive lbm_ade_stream_collide_part_m step of either form --
 * the same bits, the same launches.
 * model = LBM_MODEL_BGK: IS lbm_ade_stream_collide_part_w with `bgk` and the same `buoy` -- the same checks under that
 * name, the same launches, the same bits.
 * Refused on the host before any device call, under this name: NULL arguments, a non-finite field of the descriptor and
 * everything lbm_ade_stream_collide_part_m refuses (pressure rows, a kbc.form that differs from scalar->form, s2 outside
 * (0, 2], a bad part or edge_rows).  There is no parameter for an open view; the wall exchange of a slab's rows with this
 * fluid is lbm_ade_wallx_rows_m. */
int lbm_ade_slab_stream_collide_mb(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                   const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                                   const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                                   int part, int edge_rows, double* rho, double* u, double* conc, lbm_stream_t s);

/* Open boundaries of the fused step on a single block: the inlet, the outlet, the specular lid and the zero-gradient
 * copies of test/rectangle_sedimentation_test.cpp (:134-177, :203-218), as a host table built like lbm_ade_iwalls --
 * create / add / finalize / destroy, segments (r0 + i dr, c0 + i dc), i < n, negative r0 / c0 counting from the end.
 * Three kinds of segment, applied to the listed nodes AFTER the domain's own gather (bc, lbm_ade_scalar_bc), in the
 * order added; per node and slot the segment added last wins, for f and g separately, and a slot no segment names keeps
 * what the domain's gather gives it:
 *   lbm_ade_open_add_f      an f rule on the slots of the mask (bit s-1 = slot s), q = opp(s), f* the node's own
 *                           post-collision populations:
 *     LBM_ADE_OPEN_BOUNCE_BACK        f[s] = f*[q]
 *     LBM_ADE_OPEN_SPECULAR_ROW       f[s] = f*[s with c_x, the row component, negated]  (the driver's top: 8<-7, 1<-3, 5<-6)
 *     LBM_ADE_OPEN_SPECULAR_COL       f[s] = f*[s with c_y negated]
 *     LBM_ADE_OPEN_ABB                f[s] = -f*[q] + ((2 + 9 (u_w.c_q)^2) - 3 u_w.u_w) E_q, u_w = (p0, p1)
 *     LBM_ADE_OPEN_ABB_EXTRAPOLATED   the same with u_w = p0 u_prev(node) + p1 u_prev(node + (nr, nc)) per component
 *                                     (the driver's outlet: 1.5, -0.5, (0, -1)); u_prev = calc_u of the streamed state
 *                                     BEFORE this iteration, which the step carries (below); (nr, nc) is not (0, 0) and
 *                                     the neighbour lies inside the lattice (no wrap).  p0, p1, nr, nc unused otherwise.
 *   lbm_ade_open_add_g      a g rule on the slots of the mask: LBM_ADE_SCALAR_NO_FLUX g[s] = g*[q], LBM_ADE_SCALAR_FIXED
 *                           the anti-bounce-back of lbm_ade_iwalls with C_w = conc; v = u + w with the u of the node's
 *                           fully fixed-up f (the unshifted u0 of a buoyant step).
 *   lbm_ade_open_add_g_copy the zero-gradient copy g*[node] = g*[node + (from_dr, from_dc)] before streaming, the source
 *                           inside the lattice.  g* is formed again every step, so a copy is a redirection: every read of
 *                           the post-collision g of a node -- the nine pulls that target it, the own-population reads of
 *                           every wall rule at it -- reads the node its map entry names.  The map starts as the identity
 *                           and every copy segment sets map[dst] = map[src] for all its nodes at once, in the order added
 *                           (a second copy sees the first).  f has no copy.
 * lbm_ade_open_add_channel adds the sedimentation channel of the driver for the table's R x C (R >= 4, C >= 4): f inlet
 * ABB (0, u_in) on all eight slots of column 0, rows 1 .. R-2; f outlet ABB_EXTRAPOLATED (1.5, -0.5, (0, -1)) on column
 * C-1, all rows; SPECULAR_ROW on slots 8, 1, 5 of row 0; BOUNCE_BACK on slots 7, 3, 6 of node (R-1, C-1) -- the bottom
 * wall itself is the domain's (bc.row_hi = BOUNCE_BACK), this segment takes the corner back from the outlet; the copies
 * row 0 <- row 1 and column C-1 <- column C-2 (rows 1 .. R-2); g FIXED on all eight slots of column 0, rows 1 .. R-2, at
 * conc 0, then at conc_w on the rows of the last conc_rows rows that the inlet has (R - conc_rows .. R-2).
 * The resolved table (lbm_ade_open_count / _node, host only, valid after every add) lists, sorted by (r, c), exactly:
 * every node with a rule; for every node whose map entry is not itself the nine nodes that pull from it under periodic
 * wrap in both axes, itself included; the inward neighbour of every node with an extrapolated slot.  Per node it holds
 * the rule of each slot (f_rule[s-1]: LBM_ADE_OPEN_*, 0 = none; g_rule[s-1]: 0 = none, 1 + LBM_ADE_SCALAR_*) and the nine
 * nodes its g is pulled from (g_src_r / g_src_c[q]: the map entry of the periodic pull source of q; q = 0: of the node).
 * Everything is checked on the host; lbm_ade_open_finalize uploads the table (the one device call; an empty table makes
 * none and behaves like NULL: the same bits, the same launches).  Immutable after finalize and BORROWED by steps, solvers
 * and captured graphs.
 * The carry: lbm_ade_open_carry_len(table) doubles, two per listed node (u_r, u_c in the table's order).  A streamed step
 * reads carry_in -- the u of the listed nodes before the iteration -- and writes carry_out, the u of their fixed-up f;
 * the two must not alias and may be NULL only with a NULL or empty table.  lbm_ade_collide_o (the first iteration: no
 * rule is applied) writes carry_out from the pre-collision f.  The context owns two carries and swaps them with its
 * lattices.
 * The step with a non-empty table costs one more launch, one lane per listed node, after the interior launch and the edge
 * pass and before the interior-wall pass (collide-only: one more small launch that writes the carry).  A node may not be
 * in the call's interior-wall table as well, unless the open table gives it no rule and every g slot whose resolved
 * source differs from the plain pull is one a domain wall replaces at that node (the rectangle's foot on the bottom row).
 * lbm_ade_collide_o / lbm_ade_stream_collide_o run the whole block: a row range other than [0, R) is refused, and so is a
 * slab view.  Row slabs and the ring take a VIEW of the table (lbm_ade_open_slab, lbm_ade_stream_collide_part_o,
 * lbm_ring_ade_collide_o, lbm_ring_ade_step_o below) and refuse an ordinary table; each refusal names the function to
 * use. */
#define LBM_ADE_OPEN_BOUNCE_BACK 1
#define LBM_ADE_OPEN_SPECULAR_ROW 2
#define LBM_ADE_OPEN_SPECULAR_COL 3
#define LBM_ADE_OPEN_ABB 4
#define LBM_ADE_OPEN_ABB_EXTRAPOLATED 5
typedef struct lbm_ade_open lbm_ade_open;
int lbm_ade_open_create(lbm_ade_open** out, int R, int C);
int lbm_ade_open_add_f(lbm_ade_open* t, int r0, int c0, int dr, int dc, int n, unsigned slots, int rule /* LBM_ADE_OPEN_* */,
                       double p0, double p1, int nr, int nc);
int lbm_ade_open_add_g(lbm_ade_open* t, int r0, int c0, int dr, int dc, int n, unsigned slots,
                       int g_mode /* LBM_ADE_SCALAR_* */, double conc);
int lbm_ade_open_add_g_copy(lbm_ade_open* t, int r0, int c0, int dr, int dc, int n, int from_dr, int from_dc);
int lbm_ade_open_add_channel(lbm_ade_open* t, double u_in, double conc_w, int conc_rows);
int lbm_ade_open_count(const lbm_ade_open* t); /* listed nodes so far; host only; 0 for NULL */
/* node i of the resolved table; f_rule, g_rule: 8 ints, g_src_r, g_src_c: 9 ints; any output may be NULL; host only */
int lbm_ade_open_node(const lbm_ade_open* t, int i, int* r, int* c, int* f_rule, int* g_rule, int* g_src_r, int* g_src_c);
long long lbm_ade_open_carry_len(const lbm_ade_open* t); /* 2 x count; 0 for NULL */
int lbm_ade_open_finalize(lbm_ade_open* t);
int lbm_ade_open_destroy(lbm_ade_open* t);
/* lbm_ade_collide_b / lbm_ade_stream_collide_w with the open table (NULL or empty: those calls themselves) */
int lbm_ade_collide_o(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                      const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                      const lbm_ade_buoyancy* buoy, const lbm_ade_open* open, double* carry_out, double* rho, double* u,
                      double* conc, lbm_stream_t s);
int lbm_ade_stream_collide_o(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                             const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                             const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                             const lbm_ade_open* open, const double* carry_in, double* carry_out, int row_begin,
                             int row_end, double* rho, double* u, double* conc, lbm_stream_t s);
/* The slab view of an open table: a new, unfinalized table for an R x C lattice (C the parent's) that lists exactly the
 * parent's resolved nodes of rows [row0, row0 + R), 0 <= row0, row0 + R <= the parent's rows, at r - row0 and in the
 * parent's order, each with its winning segment per f and g slot and the segments' parameters.  The parent may be finalized
 * or not and is not modified.  Host only; lbm_ade_open_finalize uploads the view and keeps a host index of the first node
 * of each row.  A view takes no lbm_ade_open_add_* call.  Re-resolved per view:
 *   the nine g sources  slab-local, the row in [-1, R]: -1 and R are the slab's ghost rows (lbm_ade_open_node reports
 *                       them so).  The source's global row counts modulo the parent's rows: a view that ends at the
 *                       parent's last row sees global row 0 in its row R.  A source more than one row outside the slab
 *                       cannot be addressed: it is marked unreachable and points at the slot's plain pull source.
 *   the neighbours      of extrapolating slots must lie in the view's rows, or lbm_ade_open_slab fails and names the node:
 *                       the carry is slab-local and no carry travels between slabs (the channel's neighbour is in the
 *                       same row).
 *   the carry           lbm_ade_open_carry_len(view) doubles, two per node of the view in the view's order.
 * What a slab may reach is decided per call, on the host, from the slab's bc: a g source is usable in an owned row, or in
 * the ghost row of a side whose row edge is HALO (ghost = 0: the wrapped row of a PERIODIC side).  Every slot of a listed
 * node needs a usable source or must be one the domain's wall gather replaces at that node; the node's own source must be
 * usable; an unreachable source never is.  Anything else is refused, naming node and slot.  The overlap rule with an
 * interior-wall table holds between the two slab-local tables. */
int lbm_ade_open_slab(lbm_ade_open** out, const lbm_ade_open* table, int row0, int R);
/* the unreachable mark of node i of a view: bit q = the source of g slot q (q = 0: the node's own) lies more than one row
 * outside the slab; 0 for an ordinary table, NULL or a node outside the table; host only */
int lbm_ade_open_unreachable(const lbm_ade_open* t, int i);
/* lbm_ade_stream_collide_part_w with this slab's view and its carry (NULL or empty view: lbm_ade_stream_collide_part_w
 * itself, the same bits and the same launches; the carry follows the rules above).  Behind the part's dispatch, on the same
 * stream and before the interior-wall pass, one more dispatch recomputes the view's nodes of the part's rows -- one lane
 * per node, found through the view's row index: no allocation, no host synchronisation, capturable; a part without a
 * listed node enqueues nothing.  Each part writes the lattices, moments and carry_out entries of its own rows' nodes only
 * and reads the old lattices and carry_in only. */
int lbm_ade_stream_collide_part_o(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                  const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                                  const lbm_ade_open* view, const double* carry_in, double* carry_out, int part,
                                  int edge_rows, double* rho, double* u, double* conc, lbm_stream_t s);
/* kernels enqueued so far by the part launches of this process (lbm_ade_stream_collide_part*, lbm_ring_ade_step*): a part's
 * dispatch, its open pass and its interior-wall pass count one each.  There is no solver context for slabs; this is what
 * "one more launch per part with a listed node, none without" is tested with. */
long long lbm_ade_part_launches(void);
/* the context's open table from the next step on (the lazy stream of get_state included, which applies it without
 * touching the carry); NULL clears it.  Borrowed, not copied.  A non-empty table is taken on a pre-collision state only
 * (before the first step, or after lbm_ade_solver_set_state, which primes the carry): the u before the iteration of a
 * post-collision state cannot be formed for nodes that were not carried. */
int lbm_ade_solver_set_open(lbm_ade_solver* sv, const lbm_ade_open* open);
/* Open boundaries with the fluid by model, on a single block: lbm_ade_collide_o / lbm_ade_stream_collide_o /
 * lbm_ade_solver_set_open with a lbm_ade_fluid where those take lbm_bgk_params (the context's setter: for either fluid).
 * model = LBM_MODEL_BGK: the calls ARE lbm_ade_collide_o / lbm_ade_stream_collide_o with `bgk` -- the same checks under
 * those names, the same launches, the same bits; on a BGK context lbm_ade_solver_set_open_m IS lbm_ade_solver_set_open.
 * model = LBM_MODEL_KBC, NULL or empty table: the calls ARE lbm_ade_collide_mb / lbm_ade_stream_collide_mb -- the same
 * bits, the same launches, no carry needed.
 * model = LBM_MODEL_KBC, a table with nodes: the step of lbm_ade_stream_collide_o with the fluid's collision replaced.
 * One more launch follows the interior launch and the edge pass, before the interior-wall pass, one lane per listed node.
 * Per node: the domain's gather of f, then the table's f slots (bounce-back, specular row / column, ABB and
 * ABB_EXTRAPOLATED with the carried u: expressions on populations, independent of the collision); g pulled through the
 * source map with the domain's gather, the domain's FIXED edges, the table's g slots with v = u + w, u the velocity of the
 * fully fixed-up f; both collisions in the edge pass's order.  carry_out holds the unshifted u0 of the fixed-up f.  Passive,
 * the fluid's collision is kbc::collide in the form of the call; with beta != (0, 0) it is the forced KBC collision of
 * lbm_ade_collide_mb (collide_with on u0 + u_shift F), the table's g slots and the FIXED edges see the UNSHIFTED u0, the
 * moment outputs hold the shifted u, and the step runs the reference order in both halves whatever `form` says.  The
 * collide-only call writes carry_out from the pre-collision f in one more launch.  The calls only enqueue: no atomics, no
 * allocation, no host synchronisation; a captured graph keeps the table and the descriptor of its capture.
 * lbm_ade_solver_set_open_m on a KBC context follows the rule of lbm_ade_solver_set_open: a non-empty table is taken on a
 * pre-collision state only, the table is borrowed, NULL clears it; lbm_ade_solver_step then carries the table and the two
 * carries through, lbm_ade_solver_set_state primes the carry, and get_state, diag and run_until apply the table to the lazy
 * stream.  lbm_ade_solver_set_open itself keeps refusing a non-empty table on that context.
 * Refused on the host before any device call, under the new entry's name, the message naming feature and model -- the
 * fluid's own checks first: pressure rows, s2 outside (0, 2], a kbc.form that differs from scalar->form, a non-finite
 * field of the buoyancy descriptor (everything the `_m` / `_mb` calls refuse); an unfinalized table, a table for another
 * lattice, a slab view, a NULL or aliasing carry, a row range other than the whole block, the overlap rule with the
 * interior walls (everything the `_o` calls refuse).  Open boundaries over row slabs and the ring stay refused with this
 * fluid: no entry takes a view with a lbm_ade_fluid. */
int lbm_ade_open_collide_m(double* fp, double* gp, const double* f, const double* g_in, const lbm_geom* g, const lbm_bc* bc,
                           const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                           const lbm_ade_buoyancy* buoy, const lbm_ade_open* open, double* carry_out, double* rho, double* u,
                           double* conc, lbm_stream_t s);
int lbm_ade_open_stream_collide_m(double* fn, double* gn, const double* fo, const double* go, const lbm_geom* g,
                                  const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                                  const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                                  const lbm_ade_open* open, const double* carry_in, double* carry_out, int row_begin,
                                  int row_end, double* rho, double* u, double* conc, lbm_stream_t s);
int lbm_ade_solver_set_open_m(lbm_ade_solver* sv, const lbm_ade_open* open);

/* ---- slab ring in C++: one process per GPU, packed halo messages between row slabs ------------------
 * Native counterpart of pylbm/slab.py (same kernels, same halo sets): edge rows + pack + ONE message
 * to and from each neighbour + unpack on the ring's own high-priority stream, interior rows on the
 * caller's stream (the block binding of test/decompose_domain.cpp:181-187, generalised to D ghost rows).
 * Two transports carry the messages:
 *   LBM_RING_RCCL  ncclSend / ncclRecv in one group (RCCL is dlopen()ed on first use): the default;
 *   LBM_RING_IPC   peer-mapped direct stores: every rank owns a receive window in device memory that its
 *                  neighbours map through hipIpcMemHandle_t; a message is stored straight into the
 *                  neighbour's window and announced by a sequence word (bounded device-side waits,
 *                  lbm_ring_status).  One node; also between processes that share ONE GPU, where RCCL
 *                  refuses to run.  Same bits either way.
 *   LBM_RING_DEFAULT = environment LBM_RING_TRANSPORT ("rccl" | "ipc"), else RCCL.
 * Rank 0 calls lbm_ring_unique_id(_ex) and distributes the 128 bytes by any means (file, MPI,
 * torch.distributed); every rank then calls lbm_ring_create(_ex) with its slab geometry (ghost = halo
 * depth; same columns and ghost rows on every rank). */
#define LBM_RING_DEFAULT (-1)
#define LBM_RING_RCCL 0
#define LBM_RING_IPC 1
typedef struct lbm_ring lbm_ring;
int lbm_ring_unique_id(unsigned char* id128);
int lbm_ring_unique_id_ex(unsigned char* id128, int transport);
int lbm_ring_create(lbm_ring** out, const unsigned char* id128, int rank, int nranks,
                    const lbm_geom* slab, int periodic);
int lbm_ring_create_ex(lbm_ring** out, const unsigned char* id128, int rank, int nranks,
                       const lbm_geom* slab, int periodic, int transport);
int lbm_ring_destroy(lbm_ring* rg);
int lbm_ring_transport(const lbm_ring* rg); /* LBM_RING_RCCL or LBM_RING_IPC */
/* LBM_OK, or LBM_ERR_STATE once a bounded wait of the peer-mapped transport has given up on a neighbour
 * (tuning "ring_ipc_timeout_ms", default 20000; the failure is sticky: every later wait of the queue returns at
 * once, copies are skipped, nothing more is announced) or once RCCL has reported an asynchronous error
 * (ncclCommGetAsyncError; such a communicator is aborted at lbm_ring_destroy): everything computed since is
 * void.  Host-side read, no sync; meant for once per batch of launches. */
int lbm_ring_status(const lbm_ring* rg);
/* 1 if the peer-mapped transport's receive window lives in ordinary cached device memory: the runtime refused the
 * uncached allocation and the caller had accepted that beforehand (lbm_set_tuning("ring_ipc_cached_ok", 1));
 * without that tuning lbm_ring_create_ex fails instead.  0 otherwise (and for RCCL). */
int lbm_ring_window_cached(const lbm_ring* rg);
/* refresh the ghost rows of `lattice` (ordered after the work enqueued on `after`); asynchronous */
int lbm_ring_exchange(lbm_ring* rg, double* lattice, lbm_stream_t after);
/* same with complete ghost rows (LBM_HALO_FULL): the initial fill before multi-step launches on a
 * slab with walls (lbm_ring_bgk_step then keeps exchanging complete rows by itself) */
int lbm_ring_exchange_full(lbm_ring* rg, double* lattice, lbm_stream_t after);
/* same for two lattices in one message per neighbour (both colours of the two-phase model) */
int lbm_ring_exchange2(lbm_ring* rg, double* lattice_a, double* lattice_b, lbm_stream_t after);
/* make `main` wait for the ring's stream */
int lbm_ring_join(lbm_ring* rg, lbm_stream_t main);
/* one overlapped launch-step of a BGK slab: n_steps = 1 (single-step kernel) or 2..ghost (sliding
 * window); bc: the physical edges of the GLOBAL domain (NULL = periodic), seams become HALO.
 * On a closed (periodic) ring whose slabs carry ghost = m x n_steps rows (m = 2, 3; ghost <= 15) only
 * every m-th call exchanges -- all m x n_steps ghost rows in one message; the calls in between are one
 * plain launch over the owned rows plus the ghost rows the later calls of the period still read.  The
 * owned rows are current after EVERY call; any lbm_ring_exchange* starts a new period.  lbm_ring_kbc_step
 * follows the same rule (ghost = m x n_steps, n_steps <= 4). */
int lbm_ring_bgk_step(lbm_ring* rg, double* dst, const double* src, const lbm_bc* bc,
                      const lbm_bgk_params* prm, int n_steps, int edge_rows, lbm_stream_t main);
/* the same for KBC (n_steps 1, or 2..4 with the reassociated collision) */
int lbm_ring_kbc_step(lbm_ring* rg, double* dst, const double* src, const lbm_bc* bc,
                      const lbm_kbc_params* prm, int n_steps, int edge_rows, lbm_stream_t main);

/* The fluid + scalar step over row slabs (lbm_ade_stream_collide_part).  The ring's slab geometry must carry ghost = 1;
 * bc: the physical edges of the GLOBAL domain (NULL = periodic), seams become HALO, and so do both row edges of a closed
 * ring.  Every message carries the single-step halo of BOTH lattices: 2 x lbm_halo_rows(1) = 6 rows of C doubles per
 * side.  On return `main` waits for everything.  All arguments are checked on the host before any device call.
 * lbm_ring_ade_collide: the first driver iteration on a slab -- collide-only on the owned rows of (f, g_in) into
 * (fp, gp), then one exchange of both. */
int lbm_ring_ade_collide(lbm_ring* rg, double* fp, double* gp, const double* f, const double* g_in,
                         const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar, lbm_stream_t main);
/* one overlapped step: FRAME + pack + ONE message per neighbour on the ring's stream, INNER on `main` beside them */
int lbm_ring_ade_step(lbm_ring* rg, double* fn, double* gn, const double* fo, const double* go, const lbm_bc* bc,
                      const lbm_bgk_params* fluid, const lbm_ade_params* scalar, int edge_rows, lbm_stream_t main);
/* the same with the scalar's walls of the GLOBAL domain (lbm_ade_scalar_bc, checked against bc; NULL = all NO_FLUX): a
 * FIXED row edge acts at the chain end that carries it and is dropped at the seams, as bc's row walls are; a profile of a
 * column edge holds this slab's R rows */
int lbm_ring_ade_step_ex(lbm_ring* rg, double* fn, double* gn, const double* fo, const double* go, const lbm_bc* bc,
                         const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                         int edge_rows, lbm_stream_t main);
/* lbm_ring_ade_collide / lbm_ring_ade_step_ex with the buoyancy (lbm_ade_buoyancy; sbc and buoy may each be NULL): the
 * force is local to a node, so the messages and the schedule are those of the passive step */
int lbm_ring_ade_collide_b(lbm_ring* rg, double* fp, double* gp, const double* f, const double* g_in, const lbm_bc* bc,
                           const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                           const lbm_ade_buoyancy* buoy, lbm_stream_t main);
int lbm_ring_ade_step_b(lbm_ring* rg, double* fn, double* gn, const double* fo, const double* go, const lbm_bc* bc,
                        const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                        const lbm_ade_buoyancy* buoy, int edge_rows, lbm_stream_t main);
/* lbm_ring_ade_step_b with this slab's interior walls (a finalized slab-local table -- lbm_ade_iwalls_slab of the global
 * one; NULL or empty: lbm_ring_ade_step_b itself).  The wall pass of the FRAME rows runs on the ring's stream behind the
 * FRAME dispatch and BEFORE the pack -- a neighbour's ghost rows are this slab's post-collision rows, wall nodes fixed up
 * -- and the pass of the INNER rows on `main` behind INNER; a chain of one slab runs both on `main`.  There is no
 * lbm_ring_ade_collide_w: collide-only applies no wall rule, lbm_ring_ade_collide_b serves. */
int lbm_ring_ade_step_w(lbm_ring* rg, double* fn, double* gn, const double* fo, const double* go, const lbm_bc* bc,
                        const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                        const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls, int edge_rows, lbm_stream_t main);
/* lbm_ring_ade_collide_b / lbm_ring_ade_step_w with this slab's view of the open table (lbm_ade_open_slab of the global
 * one, finalized; NULL or empty: those calls themselves) and its carry.  Collide-only: one more small launch writes
 * carry_out from the pre-collision f.  A step: the open pass of the FRAME rows runs on the ring's stream behind the FRAME
 * dispatch and BEFORE the pack -- a neighbour never receives an un-fixed open node -- and the pass of the INNER rows on
 * `main`; a chain of one slab runs both on `main`.  The carry needs no synchronisation beyond the lattices'. */
int lbm_ring_ade_collide_o(lbm_ring* rg, double* fp, double* gp, const double* f, const double* g_in, const lbm_bc* bc,
                           const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                           const lbm_ade_buoyancy* buoy, const lbm_ade_open* view, double* carry_out, lbm_stream_t main);
int lbm_ring_ade_step_o(lbm_ring* rg, double* fn, double* gn, const double* fo, const double* go, const lbm_bc* bc,
                        const lbm_bgk_params* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                        const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls, const lbm_ade_open* view,
                        const double* carry_in, double* carry_out, int edge_rows, lbm_stream_t main);
/* The ring's collide-only iteration and overlapped step with the fluid by model (lbm_ade_fluid).
 * model = LBM_MODEL_BGK: ARE lbm_ring_ade_collide_b / lbm_ring_ade_step_w with `bgk` and a NULL buoyancy -- the same
 * checks under those names, the same launches, the same bits.
 * model = LBM_MODEL_KBC: the same schedule with lbm_ade_stream_collide_part_m's launches -- ghost = 1; bc and sbc of the
 * GLOBAL domain, seams HALO, a FIXED row dropped at a seam; FRAME and its wall pass on the ring's stream before the pack,
 * INNER and its wall pass on `main`; a chain of one slab runs both parts on `main`; one message per neighbour carrying
 * both lattices.  No synchronisation beyond lbm_ring_ade_step_w's.  Refusals as lbm_ade_stream_collide_part_m. */
int lbm_ring_ade_collide_m(lbm_ring* rg, double* fp, double* gp, const double* f, const double* g_in, const lbm_bc* bc,
                           const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                           lbm_stream_t main);
int lbm_ring_ade_step_m(lbm_ring* rg, double* fn, double* gn, const double* fo, const double* go, const lbm_bc* bc,
                        const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                        const lbm_ade_iwalls* iwalls, int edge_rows, lbm_stream_t main);
/* The two `_m` ring entries with the descriptor of lbm_ade_buoyancy after sbc (lbm_ade_slab_stream_collide_mb's fluids and
 * refusals, under these names).  model = LBM_MODEL_KBC with beta != (0, 0): the collide-only iteration and the step run the
 * forced KBC collision on lbm_ring_ade_step_m's schedule, unchanged -- ghost = 1, seams HALO, a FIXED row dropped at a seam,
 * FRAME and its wall pass on the ring's stream before the pack, INNER on `main`, one message per neighbour with both
 * lattices.  The force is local to a node: no synchronisation is added.  NULL or beta = (0, 0): lbm_ring_ade_collide_m /
 * lbm_ring_ade_step_m.  model = LBM_MODEL_BGK: ARE lbm_ring_ade_collide_b / lbm_ring_ade_step_w with `bgk` and the same
 * `buoy`.  Bitwise equal to lbm_ade_collide_mb / lbm_ade_stream_collide_mb on one block. */
int lbm_ring_ade_slab_collide_mb(lbm_ring* rg, double* fp, double* gp, const double* f, const double* g_in, const lbm_bc* bc,
                                 const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                                 const lbm_ade_buoyancy* buoy, lbm_stream_t main);
int lbm_ring_ade_slab_step_mb(lbm_ring* rg, double* fn, double* gn, const double* fo, const double* go, const lbm_bc* bc,
                              const lbm_ade_fluid* fluid, const lbm_ade_params* scalar, const lbm_ade_scalar_bc* sbc,
                              const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls, int edge_rows, lbm_stream_t main);
/* refresh the single-step ghost rows of two lattices in one message per neighbour (e.g. after restoring a state);
 * asynchronous, ordered after the work enqueued on `after` (lbm_ring_join makes a stream wait for it) */
int lbm_ring_exchange_pair(lbm_ring* rg, double* lattice_a, double* lattice_b, lbm_stream_t after);

/* phase timing for diagnosing a scaling run: on = 1 records timed events around the edge rows, the
 * exchange (pack + send/recv + unpack) and the interior rows of every overlapped bgk / kbc / cg / ade
 * launch-step;
 * lbm_ring_last_timing waits for the last one: out4 = {edge_rows_ms, exchange_ms, interior_ms, span_ms} */
int lbm_ring_profile(lbm_ring* rg, int on);
int lbm_ring_last_timing(lbm_ring* rg, double* out4);

/* one overlapped step of a two-phase (colour-gradient) slab: lbm_cg_step_fused on edge and interior
 * rows + ONE exchange of the 3 ghost rows of both colours (slab ghost must be 3; bc NULL = the
 * driver's walls, seams become HALO) */
int lbm_ring_cg_step(lbm_ring* rg, double* dst_r, double* dst_b, const double* src_r,
                     const double* src_b, const lbm_bc* bc, const lbm_cg_params* prm, int edge_rows,
                     lbm_stream_t main);

/* one overlapped single-step launch of a BGK slab that may own an immersed boundary (config 5 over
 * slabs): as lbm_ring_bgk_step with n_steps = 1, plus -- on the rank whose slab contains the ROI
 * (ib from lbm_ibm_create_slab; NULL elsewhere) -- rho / u written for the ROI rows only,
 * lbm_ibm_force and the Guo source on dst.  rho [R][C], u [2][R][C] slab-local. */
int lbm_ring_bgk_step_ibm(lbm_ring* rg, double* dst, const double* src, const lbm_bc* bc,
                          const lbm_bgk_params* prm, int edge_rows, lbm_ibm* ib, double guo_a,
                          double guo_b, double* rho, double* u, lbm_stream_t main);

/* ---- config 5 over slabs at multi-step speed: BGK slab with an immersed boundary anywhere, also across
 * a seam (cylinder_test.cpp:88-164 / ibm.cpp:158-190 over the block binding of decompose_domain.cpp:181-187).
 * Per block of D steps: a band of global rows [q0 - 2D, q1 + 2D) around the ROI advances D forced single
 * steps in a compact lattice of its own, replicated on every slab that owns valid band rows [q0 - D,
 * q1 + D); all other rows take the D-step window.  Across a seam inside the band the two co-owners swap
 * the band's D outermost rows instead of the ordinary halo (same size: 9 D rows of C doubles).  The
 * transport belongs to the caller (lbm_ring_bgk_block_ibm below uses RCCL): *_compute fills the two send
 * buffers, *_finish consumes the two receive buffers.  x, y: GLOBAL marker coordinates; slab: geometry with
 * ghost >= depth; the slab's rows start at global row slab_row0 of a domain of rows_global rows whose
 * physical edges are bc_global (seams become HALO).  Results equal the single-block solver bit for bit. */
typedef struct lbm_slab_ibm lbm_slab_ibm;
int lbm_slab_ibm_create(lbm_slab_ibm** out, const lbm_geom* slab, int slab_row0, int rows_global,
                        const lbm_bc* bc_global, const lbm_bgk_params* prm, int depth, const double* x,
                        const double* y, int n_markers, int m_max, double guo_a, double guo_b);
int lbm_slab_ibm_destroy(lbm_slab_ibm* sl);
/* slab heights for a chain of n_slabs slabs over rows_global rows such that all slabs finish a block together: the slab
 * that holds the forced band pays its chain of `depth` forced single steps on top of its rows, so it gets the band and few
 * other rows, and the band stays inside ONE slab (host arithmetic only; usable without a GPU).  Per-block cost model:
 * slabs without band rows far_us_per_row x rows, the owner owner_us + owner_us_per_row x rows; costs = {far_us_per_row,
 * owner_us, owner_us_per_row} or NULL = the table measured on MI355X (scaled with cols and depth).  x: GLOBAL marker rows.
 * rows_out[n_slabs] sums to rows_global; *predicted_us (may be NULL) = the slowest slab's block time under the model.
 * Every rank of a chain calls it with the same arguments and takes rows_out[rank]. */
int lbm_slab_ibm_plan_rows(int* rows_out, int n_slabs, int rows_global, int cols, int depth, const double* x,
                           int n_markers, const double* costs, double* predicted_us);
/* owner: this slab runs the band chain; straddle_*: the band's valid rows reach into that neighbour
 * (a co-owner); [b0, b1): global band rows.  Any output may be NULL. */
int lbm_slab_ibm_info(const lbm_slab_ibm* sl, int* owner, int* straddle_prev, int* straddle_next, int* b0, int* b1);
long long lbm_slab_ibm_msg_doubles(const lbm_slab_ibm* sl); /* per side per block */
/* once, on the initial post-collision state: ordinary seams exchange the complete D-row halo, co-owners
 * all their owned band rows (side 0 = previous slab, 1 = next; counts in doubles) */
int lbm_slab_ibm_prime_counts(const lbm_slab_ibm* sl, int side, long long* send, long long* recv);
int lbm_slab_ibm_prime_pack(lbm_slab_ibm* sl, const double* lattice, double* send_prev, double* send_next, lbm_stream_t s);
int lbm_slab_ibm_prime_finish(lbm_slab_ibm* sl, double* lattice, const double* recv_prev, const double* recv_next, lbm_stream_t s);
/* the driver's FIRST iteration (cylinder_test.cpp:103-127 on the initial state) instead of prime_finish:
 * prime_pack is then called on the PRE-collision lattice `pre`, whose ghost rows are filled here; `post`
 * = collision of every row + forcing and source on the band rows, ghost rows current, band primed */
int lbm_slab_ibm_start_finish(lbm_slab_ibm* sl, double* post, double* pre, const double* recv_prev,
                              const double* recv_next, lbm_stream_t s);
/* one block of `depth` steps: dst from src (ghost rows of src complete and current), messages packed */
int lbm_slab_ibm_block_compute(lbm_slab_ibm* sl, double* dst, const double* src, double* send_prev,
                               double* send_next, lbm_stream_t s);
int lbm_slab_ibm_block_finish(lbm_slab_ibm* sl, double* dst, const double* recv_prev, const double* recv_next, lbm_stream_t s);
int lbm_slab_ibm_surface_force(lbm_slab_ibm* sl, double* out2, lbm_stream_t s); /* owners: F_s of the last step */
/* n_rows complete rows (all 9 populations) between two lattices of equal column count; rows in owned-row
 * indices, ghost rows allowed where the geometry has them */
int lbm_rows_copy(double* dst, const lbm_geom* dg, int dst_row, const double* src, const lbm_geom* sg,
                  int src_row, int n_rows, lbm_stream_t s);
/* the same over the slab ring: priming exchange, then one block per call (non-owners: the overlapped
 * lbm_ring_bgk_step schedule; owners: band chain beside the far rows, exchange behind both) */
int lbm_ring_ibm_prime(lbm_ring* rg, lbm_slab_ibm* sl, double* lattice, lbm_stream_t main);
int lbm_ring_ibm_start(lbm_ring* rg, lbm_slab_ibm* sl, double* post, double* pre, lbm_stream_t main);
int lbm_ring_bgk_block_ibm(lbm_ring* rg, lbm_slab_ibm* sl, double* dst, const double* src, int edge_rows,
                           lbm_stream_t main);

/* ---- pressure-periodic rows over slabs (horizontal_poiseuille_test.cpp:25-45 over the block binding of
 * decompose_domain.cpp:50-73,181-187), blocks of `depth` steps.  The ring is PERIODIC: the virtual rows 0 / Rg-1 sit on
 * its two end slabs, which replicate the small seam lattice of lbm_solver_step's pressure blocks and swap, per block, the
 * D rows at distance [D, 2D) from the seam in place of that seam's halo (same size).  Transport-free: *_pack / *_compute
 * fill two send buffers, *_finish consume two receive buffers (side 0 = previous slab, 1 = next).  BGK; bc_global: the
 * domain's edges with pressure_rows = 1, periodic rows, periodic / wall columns.  Bitwise equal to the single block. */
typedef struct lbm_slab_pressure lbm_slab_pressure;
int lbm_slab_pressure_create(lbm_slab_pressure** out, const lbm_geom* slab, int slab_row0, int rows_global,
                             const lbm_bc* bc_global, const lbm_bgk_params* prm, int depth);
/* the same for KBC (test/ulbm_poiseuille.cpp:36-58, :85-139: KBC + pressure rows + wall columns): blocks of 2 steps (the
 * depth of the reference-order KBC window, as on one block); block_compute / block_finish / msg_doubles are shared.  The
 * driver's first iteration collides on HELD moments (kbc.m0, kbc.m1, :85-86): the start-up calls take them for the slab's
 * owned rows (m0 [R][C], m1 [2][R][C]); across the pressure seam the message carries the 2 D rows and their moments (12
 * planes).  After start_finish_kbc the ghost rows of `post` are not current: exchange complete halos (LBM_HALO_FULL(2)) over
 * the ordinary seams before the first block (lbm_ring_pressure_start_kbc does). */
int lbm_slab_pressure_create_kbc(lbm_slab_pressure** out, const lbm_geom* slab, int slab_row0, int rows_global,
                                 const lbm_bc* bc_global, const lbm_kbc_params* prm);
int lbm_slab_pressure_start_pack_kbc(lbm_slab_pressure* sl, const double* pre, const double* m0, const double* m1,
                                     double* send_prev, double* send_next, lbm_stream_t s);
int lbm_slab_pressure_start_finish_kbc(lbm_slab_pressure* sl, double* post, double* pre, const double* m0, const double* m1,
                                       const double* recv_prev, const double* recv_next, lbm_stream_t s);
int lbm_slab_pressure_destroy(lbm_slab_pressure* sl);
int lbm_slab_pressure_info(const lbm_slab_pressure* sl, int* R, int* C, int* ghost, int* depth); /* any output may be NULL */
long long lbm_slab_pressure_msg_doubles(const lbm_slab_pressure* sl, int side, int start /* 1: the start-up exchange */);
/* start-up from the driver's pre-collision state: exchange, then first iteration into `post` */
int lbm_slab_pressure_start_pack(lbm_slab_pressure* sl, const double* pre, double* send_prev, double* send_next, lbm_stream_t s);
int lbm_slab_pressure_start_finish(lbm_slab_pressure* sl, double* post, double* pre, const double* recv_prev,
                                   const double* recv_next, lbm_stream_t s);
int lbm_slab_pressure_block_compute(lbm_slab_pressure* sl, double* dst, const double* src, double* send_prev,
                                    double* send_next, lbm_stream_t s);
int lbm_slab_pressure_block_finish(lbm_slab_pressure* sl, double* dst, const double* recv_prev, const double* recv_next, lbm_stream_t s);
/* the same over the slab ring (created periodic): start-up, then one block per call (exchange behind the compute) */
int lbm_ring_pressure_start(lbm_ring* rg, lbm_slab_pressure* sl, double* post, double* pre, lbm_stream_t main);
int lbm_ring_bgk_block_pressure(lbm_ring* rg, lbm_slab_pressure* sl, double* dst, const double* src, lbm_stream_t main); /* BGK and KBC slabs alike */
/* KBC start-up over the ring: held moments of the owned rows; ends with the complete-halo exchange of `post` */
int lbm_ring_pressure_start_kbc(lbm_ring* rg, lbm_slab_pressure* sl, double* post, double* pre, const double* m0,
                                const double* m1, lbm_stream_t main);

/* ---- population links between lattices on one GPU (multi-block topologies) -----------------------
 * The reference glues blocks by slice assignments after advect (test/decompose_domain.cpp:181-187;
 * test/decompose_domain_loop.cpp:235-261, plus its slice-assignment walls :173-231): here a table of
 * element links built once, applied in ONE gather launch per step,
 *     dst[dst_lattice][q_dst][r0 + k dr][c0 + k dc] = src[src_lattice][q_src][sr0 + k sdr][sc0 + k sdc],
 * k = 0 .. count-1.  Slices are added in the order the driver executes them; where two write the
 * same destination element the later one wins (resolved on the host, the device pass is race-free).
 * dst / src of lbm_links_apply: one pointer per lattice (typically f_adve and f_coll of each block).
 * In place (dst[i] == src[j]) every link reads the value from before the call, which holds only while no
 * link reads from lattice j an element that a link of the same table writes in lattice i.  A call with such
 * a pair is refused before anything is enqueued: split the table in two and apply one after the other. */
typedef struct lbm_links lbm_links;
int lbm_links_create(lbm_links** out, int n_lattices /* <= 8 */, const lbm_geom* geoms);
int lbm_links_add(lbm_links* t, int dst_lat, int q_dst, int r0, int c0, int dr, int dc, int src_lat,
                  int q_src, int sr0, int sc0, int sdr, int sdc, int count);
/* affine links: dst = scale * src (+ addends[add0 + k add_stride]; add0 < 0: no addend).  scale = -1
 * with an addend is the anti-bounce-back "-f_coll + term" of rectangle_sedimentation_test.cpp:152-170;
 * the addend array is handed to lbm_links_apply_affine (it changes every step there).  With add0 >= 0
 * every index add0 + k add_stride must be >= 0 (both ends are checked; nothing is added otherwise). */
int lbm_links_add_affine(lbm_links* t, int dst_lat, int q_dst, int r0, int c0, int dr, int dc,
                         int src_lat, int q_src, int sr0, int sc0, int sdr, int sdc, int count,
                         double scale, long long add0, long long add_stride);
int lbm_links_apply_affine(lbm_links* t, double* const* dst, const double* const* src,
                           const double* addends, lbm_stream_t s);
int lbm_links_finalize(lbm_links* t);
int lbm_links_count(const lbm_links* t); /* distinct destination elements */
int lbm_links_apply(lbm_links* t, double* const* dst, const double* const* src, lbm_stream_t s);
int lbm_links_destroy(lbm_links* t);
/* per-row wall terms of rectangle_sedimentation_test.cpp, out[r][9], from the wall velocity
 * uw = wa u[:, r, col_a] + wb u[:, r, col_b] + shift of the moment field u [2][X][Y]:
 * mode 0: factor ((2 + 9 (uw.c_q)^2) - 3 uw.uw) w_q                       (anti-bounce-back, :135,:149)
 * mode 1: factor ((((1 + 3 uw.c_q) + 4.5 (uw.c_q)^2) - 1.5 uw.uw) w_q) field[r]   (concentration inlet, :202) */
int lbm_wall_terms(double* out, const double* u, int X, int Y, int col_a, double wa, int col_b, double wb,
                   double shift, int mode, const double* field, double factor, lbm_stream_t s);
/* one pressure-periodic virtual row at the operator level, possibly between two blocks
 * (test/decompose_domain.cpp:50-73; same lattice for dst and src: horizontal_poiseuille_test.cpp:25-45):
 * coll_dst[dst_row] = (feq(rho_bc, u_src[src_row]) + coll_src[src_row]) - equi_src[src_row];
 * u_src is the moment field [2][R][C] of the source block */
int lbm_pressure_row(double* coll_dst, const lbm_geom* g_dst, int dst_row, const double* coll_src,
                     const double* equi_src, const double* u_src, const lbm_geom* g_src, int src_row,
                     double rho_bc, int incompressible, lbm_stream_t s);
/* out = a * in + b, elementwise (the driver's "u + w_s", :124) */
int lbm_axpb(double* out, const double* in, double a, double b, long long n, lbm_stream_t s);
/* uniform momentum source on rows [row_begin, row_end) of a post-collision lattice
 * (decompose_domain_loop.cpp:152-160): p_q += ((1 - omega/2)((a + b u.c_q)(F.c_q) - a u.F)) w_q with the
 * step's u [2][R][C]; (a, b) = (3, 9) in that driver */
int lbm_bgk_add_force_rows(double* p, const lbm_geom* g, const double* u, double omega, double Fr,
                           double Fc, double a, double b, int row_begin, int row_end, lbm_stream_t s);

/* ---- snapshots and checkpoints (the reference only torch::save()s snapshot
 * stacks at the end of a run, e.g. horizontal_poiseuille_test.cpp:157-160) ------------------------ */
typedef struct lbm_snapshot lbm_snapshot;
int lbm_snapshot_create(lbm_snapshot** out, lbm_solver* sv);
int lbm_snapshot_destroy(lbm_snapshot* sn);
/* capture the moments of the last lbm_solver_step(.., record_moments = 1): device staging on the
 * solver's stream, device->pinned-host copy on a private stream; returns at once, the solver may
 * keep stepping */
int lbm_snapshot_record(lbm_snapshot* sn);
/* wait for that copy; write rho [R,C] / u [R,C,2] as NumPy .npy (either path may be NULL) */
int lbm_snapshot_write_npy(lbm_snapshot* sn, const char* rho_path, const char* u_path);
/* wait for that copy; host pointers (valid until the next record) and the step they belong to */
int lbm_snapshot_host(lbm_snapshot* sn, const double** rho, const double** u, long long* step);
/* the same for the two-phase solver: rho_r, rho_b [R,C] and u [R,C,2] of the CURRENT state (what the
 * driver holds after the iterations run so far); record() returns at once */
typedef struct lbm_cg_snapshot lbm_cg_snapshot;
int lbm_cg_snapshot_create(lbm_cg_snapshot** out, lbm_cg_solver* sv);
int lbm_cg_snapshot_destroy(lbm_cg_snapshot* sn);
int lbm_cg_snapshot_record(lbm_cg_snapshot* sn);
int lbm_cg_snapshot_host(lbm_cg_snapshot* sn, const double** rho_r, const double** rho_b,
                         const double** u, long long* step);
int lbm_cg_snapshot_write_npy(lbm_cg_snapshot* sn, const char* rho_r_path, const char* rho_b_path,
                              const char* u_path);
/* raw checkpoint of the resident lattice + state form + step counter + parameters; restart is
 * bitwise.  load needs a solver of the same model and size. */
int lbm_solver_checkpoint_save(lbm_solver* sv, const char* path);
int lbm_solver_checkpoint_load(lbm_solver* sv, const char* path);

/* ---- device-side diagnostics: reproducible field sums and run-to-convergence (DESIGN.md "Diagnostics") --------
 * Sums, extrema and a non-finite count over the dense macroscopic fields rho [R][C], u [2][R][C] (ur = u[0],
 * uc = u[1]) and, optionally, conc [R][C], without a field ever leaving the device.  The value of a sum is defined by
 * node indices alone:  fold64(x[0..n)) takes 64 accumulators p[j] = +0.0, adds x[j + 64 k] to p[j] for k = 0, 1, ...
 * in ascending order (missing elements add nothing), then p[j] += p[j + s] (j < s) for s = 32, 16, 8, 4, 2, 1, and is
 * p[0]; all additions are IEEE f64, not contracted.  The value of row r is fold64 over its columns of the per-node
 * term, the value of a row range is fold64 over its row values; minima / maxima fold the same way with fmin / fmax
 * (NaN operands skipped) from +inf / -inf.  So a table filled slab by slab, under any launch shape, folds to the
 * bits of one block.  Where a field holds a non-finite value, only NONFINITE is specified for the rows holding it. */
#define LBM_DIAG_NQ 17
#define LBM_DIAG_SUM_RHO 0    /* rho */
#define LBM_DIAG_SUM_UR 1     /* ur */
#define LBM_DIAG_SUM_UC 2     /* uc */
#define LBM_DIAG_SUM_MR 3     /* rho*ur */
#define LBM_DIAG_SUM_MC 4     /* rho*uc */
#define LBM_DIAG_SUM_KE 5     /* 0.5 * (rho * (ur*ur + uc*uc)) */
#define LBM_DIAG_MAX_U2 6     /* max of ur*ur + uc*uc */
#define LBM_DIAG_MIN_RHO 7
#define LBM_DIAG_MAX_RHO 8
#define LBM_DIAG_NONFINITE 9  /* nodes where rho, ur, uc (or conc, if given) is NaN or +-inf; exact, as a double */
#define LBM_DIAG_SUM_C 10     /* conc; slots 10-15 are 0.0 without conc */
#define LBM_DIAG_SUM_CUR 11   /* conc*ur */
#define LBM_DIAG_SUM_CUC 12   /* conc*uc */
#define LBM_DIAG_MIN_C 13
#define LBM_DIAG_MAX_C 14
#define LBM_DIAG_SUM_C2 15    /* conc*conc */
#define LBM_DIAG_SUM_DEV2 16  /* (ur - profile[c]) * (ur - profile[c]); 0.0 without profile */
/* row values of rows [row_begin, row_end) of the fields into table [LBM_DIAG_NQ][table_rows] (device): row r lands
 * at table[q * table_rows + table_row0 + r], nothing else is written -- a slab fills its rows of a global table.
 * conc, profile (device, [C]) may be NULL.  Enqueues one launch; capturable. */
int lbm_diag_rows(double* table, int table_rows, int table_row0, const double* rho, const double* u,
                  const double* conc, const double* profile, int R, int C, int row_begin, int row_end,
                  lbm_stream_t s);
/* rows [row_begin, row_end) of a table to out_dev [LBM_DIAG_NQ] (device).  Enqueues one launch; capturable. */
int lbm_diag_fold(double* out_dev, const double* table, int table_rows, int row_begin, int row_end, lbm_stream_t s);
/* the same fold of a table in host memory, in plain C++ without any device call: for ranks that gather their row
 * tables over a transport of their own */
int lbm_diag_fold_host(double* out, const double* table_host, int table_rows, int row_begin, int row_end);
/* the moments recorded by the last lbm_solver_step(.., 1), reduced over rows [row_begin, row_end): out_host
 * [LBM_DIAG_NQ], and the row table [LBM_DIAG_NQ][R] if table_host is given.  profile_dev may be NULL.  The context
 * owns the device table and a pinned buffer (allocated on first use); copies LBM_DIAG_NQ doubles (or the table)
 * and synchronises. */
int lbm_solver_diag(lbm_solver* sv, const double* profile_dev, int row_begin, int row_end, double* out_host,
                    double* table_host);
/* the same over rho, u, C of the streamed state, formed on the device as lbm_ade_solver_get_state forms them:
 * equal to the fold of what get_state returns */
int lbm_ade_solver_diag(lbm_ade_solver* sv, const double* profile_dev, int row_begin, int row_end, double* out_host,
                        double* table_host);
/* The stopping rule of the reference drivers (horizontal_poiseuille_test.cpp:113-126) on the device.  t counts the
 * iterations of the call from 0.  At every t > 0 with t % interval == offset the watched value -- the sum `quantity`
 * over rows [row_begin, row_end) of the moments of iteration t - 1, divided by the node count of that range -- is
 * formed; the run stops (converged = 1) when |value / old - 1| < tolerance, otherwise old = value.  It also ends
 * at max_steps (converged = 0; no check at t == max_steps).  Between checks the steps go through lbm_solver_step /
 * lbm_ade_solver_step (multi-step blocks fuse as ever); one host synchronisation of LBM_DIAG_NQ doubles per check.
 * steps_done, converged, last_value (the last value formed; old_value if none was) may be NULL. */
typedef struct lbm_converge {
  int quantity;         /* a LBM_DIAG_SUM_* index */
  int interval, offset; /* reference: 100, 1 */
  double tolerance;     /* reference: 1e-12 */
  double old_value;     /* the first "old" value; reference: 1.0 */
  int row_begin, row_end;
} lbm_converge;
int lbm_solver_run_until(lbm_solver* sv, const lbm_converge* cv, int max_steps, int* steps_done, int* converged,
                         double* last_value);
int lbm_ade_solver_run_until(lbm_ade_solver* sv, const lbm_converge* cv, int max_steps, int* steps_done,
                             int* converged, double* last_value);

/* ---- wall exchange: what the interior walls (lbm_ade_iwalls) take from the lattices in one stream ----------------
 * A table node of the wall pass first gets the domain's own rules (the wall gather of f and of g, and the anti-bounce-
 * back of the domain's FIXED edges), then the table's.  For every slot s the table names at the node, x_in[s] is the
 * streamed population immediately before the table's rule for that distribution, x_out[s] the one after it, and
 * d[s] = x_in[s] - x_out[s] is what the wall removes from the lattice at that slot in this stream.  Per node, each term
 * is accumulated from +0.0 over s = 1..8 ascending, named slots only, in IEEE f64 without contraction:
 *   FORCE_R       f slots: + d[s] where c_s has row component +1, - d[s] where -1 -- the momentum given to the walls, i.e.
 *                 the force on them, row component
 *   FORCE_C       the same with the column component
 *   MASS          f slots: d[s], the fluid mass taken
 *   SCALAR        all named g slots: d[s], the scalar taken (deposition)
 *   SCALAR_FIXED  the FIXED g slots only
 *   NODES         1.0 per counted node; exact
 * This is the conservation form, the model's own: a wall node stays a fluid node whose outgoing populations stream on to
 * the node behind it, so the sums are exactly what leaves the lattices (Ladd's link form would count momentum the
 * lattice never loses).  The velocity the FIXED g slots see is the pass's own: the collision's u in the form of the
 * call, the unshifted u0 in a buoyant step -- in the reference order x_out is, bit for bit, the population the pass
 * holds before it collides.  An open-boundary table plays no part (the wall pass ignores the source map as well: the
 * host refuses the overlaps where that would matter).
 * region4 = {r0, r1, c0, c1} selects the nodes of [r0, r1) x [c0, c1) in the row and column indices of the lattice of
 * the call (clipped to it; NULL: every node); a node outside contributes nothing.  Summation is the diagnostics' (fold64
 * above): the value of lattice row r is fold64 over the row's table nodes in column order (the k-th node of the row is
 * element k; a node outside the region adds nothing), the value of a row range fold64 over the row values; a row without
 * a counted node has the value +0.0.  So a table filled slab by slab, under any launch shape, folds to the bits of one
 * block. */
#define LBM_WALLX_NQ 6
#define LBM_WALLX_FORCE_R 0
#define LBM_WALLX_FORCE_C 1
#define LBM_WALLX_MASS 2
#define LBM_WALLX_SCALAR 3
#define LBM_WALLX_SCALAR_FIXED 4
#define LBM_WALLX_NODES 5
/* row values of rows [row_begin, row_end) of the stream FROM the post-collision lattices fo, go into table
 * [LBM_WALLX_NQ][table_rows] (device): row r lands at table[q * table_rows + table_row0 + r], nothing else is written
 * and the lattices are only read.  The arguments are those of lbm_ade_stream_collide_w for the same stream; on a slab g
 * carries the ghost rows (row edges HALO or BOUNCE_BACK) and iwalls is the slab's view (lbm_ade_iwalls_slab).  A NULL or
 * empty table writes +0.0 row values.  Enqueues one launch: no atomics, no allocation, no host synchronisation;
 * capturable. */
int lbm_ade_wallx_rows(double* table, int table_rows, int table_row0, const double* fo, const double* go,
                       const lbm_geom* g, const lbm_bc* bc, const lbm_bgk_params* fluid, const lbm_ade_params* scalar,
                       const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                       const int* region4, int row_begin, int row_end, lbm_stream_t s);
/* rows [row_begin, row_end) of a table to out_dev [LBM_WALLX_NQ] (device).  Enqueues one launch; capturable. */
int lbm_ade_wallx_fold(double* out_dev, const double* table, int table_rows, int row_begin, int row_end, lbm_stream_t s);
/* the same fold of a table in host memory, in plain C++ without any device call */
int lbm_ade_wallx_fold_host(double* out, const double* table_host, int table_rows, int row_begin, int row_end);
/* The exchange of the stream lbm_ade_solver_get_state shows -- from the post-collision level the context holds, with its
 * own edges, parameters, scalar walls, buoyancy and table (after the collide-only first step too, whose stream takes the
 * same rules) -- over rows [row_begin, row_end): out_host [LBM_WALLX_NQ], and the row table [LBM_WALLX_NQ][R] if
 * table_host is given (rows outside the range: 0.0).  The context owns the device table and a pinned buffer (allocated
 * on first use); copies LBM_WALLX_NQ doubles (or the table) and synchronises once.  LBM_ERR_STATE while the state is
 * pre-collision (before the first step): nothing has streamed. */
int lbm_ade_solver_wall_exchange(lbm_ade_solver* sv, const int* region4, int row_begin, int row_end, double* out_host,
                                 double* table_host);
/* The wall exchange with the fluid by model, defined exactly as above: lbm_ade_wallx_rows with a lbm_ade_fluid, and the
 * context's call for either fluid.  model = LBM_MODEL_BGK (a BGK context): the calls ARE lbm_ade_wallx_rows /
 * lbm_ade_solver_wall_exchange -- the same checks under those names, the same launch, the same bits.  model =
 * LBM_MODEL_KBC: the velocity the FIXED g slots see is the KBC collision's u in the form of the call; in a buoyant call the
 * unshifted u0 with the reference-order model.  The raw call serves a single block or a slab as the geometry says (on a
 * slab iwalls is the slab's lbm_ade_iwalls_slab view); lbm_ade_wallx_fold and lbm_ade_wallx_fold_host fold its table.  An
 * open table set on the context plays no part.  Refused on the host before any device call, under these names: what
 * lbm_ade_stream_collide_mb refuses and what lbm_ade_wallx_rows refuses; lbm_ade_solver_wall_exchange itself keeps
 * refusing a KBC context. */
int lbm_ade_wallx_rows_m(double* table, int table_rows, int table_row0, const double* fo, const double* go,
                         const lbm_geom* g, const lbm_bc* bc, const lbm_ade_fluid* fluid, const lbm_ade_params* scalar,
                         const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls,
                         const int* region4, int row_begin, int row_end, lbm_stream_t s);
int lbm_ade_solver_wall_exchange_m(lbm_ade_solver* sv, const int* region4, int row_begin, int row_end, double* out_host,
                                   double* table_host);

/* Tuning table.  Launch-shape keys (every setting produces identical results) and the three
 * implementation switches, which select between a model's two collision implementations:
 *   "bgk_fast", "kbc_fast", "cg_fused" (default 1): the reassociated collision / the one-launch
 *   two-phase step; 0 = the reference's operation order, bit-identical to the CPU oracle.
 * Further keys: "kbc_depth" (steps lbm_solver_step fuses per launch for KBC, default 4; 3 with walls), "cg_tile"
 * (0: 8x32, 1: 16x32, 2: 8x64, 3 / 4 [default]: 16x32 budgeted for 3 / 4 waves per SIMD, 5: 32x32, 6: 16x64), "cg_xcd" (0: hardware order; 1: XCD-contiguous eighths; 2 [default] / 4 / 8: groups of that many
 * column-neighbour tiles per XCD), "cg_strip" (0 [default]: LDS tile kernel; 1/2/4:
 * column-strip sliding-window kernel with that many waves per workgroup, "cg_rows" rows per chunk),
 * "cg_split" (1 [default]: inner tiles through the boundary-free instantiation + a frame launch;
 * 0: one launch, every tile through the general boundary gather; same bits).
 * The environment variable LBM_TUNE="key=value,key=value" pre-loads the table (compiled drivers).
 * Launch-shape keys: "variant" (0 generic, 1 one node/thread grid-stride,
 * 2 two nodes/thread 16-B accesses, 3 [default] 2-D grid one node/thread), "nt" (bit 0
 * non-temporal loads, bit 1 non-temporal stores; default 3), "block" (128..1024, default 256),
 * "rows" (rows per thread 1/2/4, default 1), "grid_cap" (variants 1-2); two-step LDS kernel:
 * "tb_rows" (tile height, default 8), "tb_block" (default 512), "tb_order"; sliding-window kernel:
 * "sw_rows" (rows per wavefront chunk; default: fitted per launch to the resident wave slots, 64 when the launch is many rounds deep), "sw_waves" (waves per workgroup, default 4; 2 for
 * the reassociated BGK model), "sw_xcd" (G > 0: G consecutive strip groups per XCD; measured no effect);
 * "solver_depth" (steps lbm_solver_step fuses per launch on periodic BGK blocks, default 5, 1 =
 * off), "solver_depth_walls" (the same on wall-bounded blocks, default 5), "bgk_fast_delta" (0 [default]: delta-form BGK parameters always run the reference operation order;
 * 1: they may use the reassociated model too, 1e-10 instead of bitwise on the cylinder preset), "ibm_depth" (steps lbm_solver_step advances per block on a BGK lattice with an immersed boundary: forced
 * band around the ROI in single steps, rows at least that far away through the multi-step window; default 5,
 * 1 = one step per launch everywhere; same bits), "pressure_depth" (steps per block on lattices with pressure-periodic rows: the 2 D rows on either side of the virtual rows in single steps on a small periodic
 * lattice beside the D-step window on all other rows; default 5 for BGK, 2 for KBC, 1 = one step per launch; same bits), "halo_grid" (workgroup cap of the halo pack / unpack copies, default 256), "ibm_box" (0: the forced single steps of an immersed-boundary block run over full-width band rows instead of a box of ROI +- 2 D rows and columns), "ibm_box_overlap" (0: box chain and window launch one after the other on the caller's stream), "ibm_box_sole" (0: a slab that owns the whole forced band alone still goes through the band lattice), "ibm_chain_kernel" (1: the forced-box chain of a block as ONE launch of "ibm_chain_wgs" [16] workgroups with grid barriers instead of 3 D launches; same bits, level), "bg_priority" (1: the background stream of those window launches gets the lowest priority; default 0: such a queue starves while any other queue of the process has work), "ring_period" (1: lbm_ring_bgk_step exchanges on every launch even when the slabs carry m x n_steps ghost rows; default 0 = one exchange per m launches), "ibm_gate" (1 [default]: lbm_solver_step holds its lattice launches behind a one-wave gate until the
 * forcing workgroup is resident; 0: off), "sw_split" (1 [default]: wall-bounded
 * multi-step launches run their wall-free interior through the plain instantiation and only the frame of
 * outermost strips / rows next to a wall row through the wall-carrying one, on a helper stream; 0: one
 * wall-carrying launch; same bits).  value < 0 restores the default.  Measurements: DESIGN.md "BGK kernel variants". */
int lbm_set_tuning(const char* key, int value);
/* 1 when the library was built with EXPERIMENTS=1: the launch forms that were measured and not kept (tuning keys "sw_pair",
 * "sw_pf2", "ibm_chain_kernel", "cg_strip", "cg_strip2" = 1 / 2 / 4, "cg_merge") exist; 0: those keys are
 * ignored */
int lbm_build_has_experiments(void);
/* an empty one-thread kernel ("k_lbm_marker") to cut a profiler trace at: measurement harnesses bracket the launches
 * whose counters they sum with two of these */
int lbm_marker(int tag, lbm_stream_t s);
int lbm_get_tuning(const char* key);

#ifdef __cplusplus
}
#endif
#endif /* LBM_HIP_H */
