// Host-side plumbing shared by the C-ABI translation units: per-thread error record,
// HIP status checks, launch-geometry helpers and the tuning table.
#pragma once
#include <vector>
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <type_traits>

#include "../../include/lbm_hip.h"

namespace lbm {

void set_error(const char* fmt, ...);
int tuning(const char* key, int dflt);
// capi_ibm.hip: one-wave kernel on `st` that ends once the last lbm_ibm_step's workgroup is resident
int ibm_gate(lbm_ibm* ib, hipStream_t st);
// capi_kbc.hip: 2 time steps per launch through the sliding window with the REFERENCE-ORDER KBC model
// (lattices with pressure rows keep that order: solver_pressure_block); rows [row_begin, row_end)
int kbc_stream_collide_x2_ref(double* p_new, const double* p_old, const lbm_geom* g, const lbm_bc* bc,
                              const lbm_kbc_params* prm, int row_begin, int row_end, hipStream_t st);
// capi_bgk.hip: lbm_bgk_stream_collide_xn pinned to the reference operation order
int bgk_stream_collide_xn_ref(double* p_new, const double* p_old, const lbm_geom* g, const lbm_bc* bc,
                              const lbm_bgk_params* prm, int n_steps, int row_begin, int row_end, hipStream_t st);
int bgk_collide_ref(double* p, const double* f, const lbm_geom* g, const lbm_bgk_params* prm, hipStream_t st);
// capi_ibm.hip: lbm_ibm_step on a WINDOW of the lattice the boundary was created for -- rows [row_off, row_off + g->R),
// columns [col_off, col_off + g->C) of it, held as a lattice of its own (p, u [2][R][C], rho [R][C] are the window's).
// Same tables, same arithmetic; only the origin the kernels add to ROI indices moves.
int ibm_step_window(lbm_ibm* ib, int row_off, int col_off, double* p, const lbm_geom* g, const double* u,
                    const double* rho, double omega, double a, double b, hipStream_t st);
// capi_ibm.hip: the D forced single steps of a box lattice pair (box step + forcing + source term, D times) as ONE
// launch of a few workgroups on compute units of their own; *cur flips when D is odd.  1 = not applicable.
int ibm_box_chain(lbm_ibm* ib, int row_off, int col_off, double* const box[2], int* cur, const lbm_geom* g,
                  const lbm_bgk_params* prm, bool fast_model, int D, double* xrho, double* xu, double a, double b,
                  hipStream_t st);
// capi_kbc.hip: the same question for KBC
bool kbc_uses_fast_model(const lbm_kbc_params* prm);
// capi_bgk.hip: the model lbm_bgk_stream_collide picks for these parameters (reassociated or reference order)
bool bgk_uses_fast_model(const lbm_bgk_params* prm, const lbm_bc* bc);
// capi_core.hip: a box of n_rows x n_cols nodes, all 9 populations, between two lattices (rows in owned-row
// indices, ghost rows allowed)
int box_copy(double* dst, const lbm_geom& dg, int dst_row, int dst_col, const double* src, const lbm_geom& sg,
             int src_row, int src_col, int n_rows, int n_cols, hipStream_t st);
// capi_core.hip: a non-blocking stream for a grid-filling launch that runs beside a chain of small dependent kernels
// on the caller's stream ("bg_priority" = 1: of the lowest priority, so that the dispatcher hands freed wave slots to
// the chain first -- off by default: such a queue starves whenever another queue of the process has work).
// (A stream that spares one compute unit for the chain -- hipExtStreamCreateWithCUMask -- was tried and is far slower:
// profiles/r02_ibm_box_bench.log.)
int make_background_stream(hipStream_t* out);
// capi_ade.hip: one call of the fused fluid + scalar step after its host checks -- the device copies of geometry, edges,
// scalar walls, buoyancy and the tables that every launch of the call takes.  Its members are ade.hpp's, and ade.hpp
// defines kernels, so AdeCall is complete (ade_call.hpp) in the units that launch them alone -- capi_ade.hip and the three
// capi_ade_kbc*.hip: another unit keeps one in an AdeCallBuf.
struct AdeCall;
struct AdeWalls;
struct AdeBuoyancy;
struct AdeCallBuf {
  alignas(8) unsigned char bytes[320];
  AdeCall* get() { return reinterpret_cast<AdeCall*>(bytes); }
};
// the fluid of a call: a BGK parameter block or a KBC one, exactly one of them given (both NULL: a BGK call without its
// fluid, refused where the BGK fluid is checked).  ade_fluid_model: the fluid of an `_m` entry -- given, model BGK or KBC
struct AdeFluid {
  const lbm_bgk_params* bgk;
  const lbm_kbc_params* kbc;
};
int ade_fluid_model(const char* fn, const lbm_ade_fluid* fluid, AdeFluid* out);
// the host checks, once, under the caller's name fn (slab: ghost rows and HALO row edges allowed; sbc, buoy, iwalls may be
// NULL; open: on a slab a view of the global table, lbm_ade_open_slab, on a single block an ordinary table; a KBC fluid
// takes no table with nodes and, on a slab, no buoyancy), and the two of them that need no geometry on their own (sw, by:
// the device copy, if wanted)
int ade_resolve(const char* fn, const lbm_geom* g, const lbm_bc* bc, const AdeFluid& fluid, const lbm_ade_params* scalar,
                const lbm_ade_scalar_bc* sbc, const lbm_ade_buoyancy* buoy, const lbm_ade_iwalls* iwalls, bool slab,
                AdeCall* call, const lbm_ade_open* open = nullptr);
int ade_scalar_bc_check(const char* fn, const lbm_ade_scalar_bc* sbc, const lbm_bc* bc, AdeWalls* sw = nullptr);
int ade_buoyancy_check(const char* fn, const lbm_ade_buoyancy* buoy, AdeBuoyancy* by = nullptr, bool* buoyant = nullptr);
// launches from a resolved call, whatever its fluid: one part (LBM_ADE_PART_*; its lattices and part pass ade_part_args
// first; the table passes of the part's rows follow its dispatch on the same stream) and the collide-only pass on the owned
// rows (the first driver iteration)
int ade_part_args(const char* fn, const AdeCall& call, const double* f_new, const double* g_new, const double* f_old,
                  const double* g_old, int part, int edge_rows, const double* rho, const double* u, const double* conc);
int ade_part_from(const AdeCall& call, double* f_new, double* g_new, const double* f_old, const double* g_old, int part,
                  int edge_rows, double* rho, double* u, double* conc, hipStream_t st);
int ade_collide_from(const char* fn, const AdeCall& call, double* fp, double* gp, const double* f, const double* h,
                     double* rho, double* u, double* conc, hipStream_t st);
// a slab's open table (ade_resolve's `open`: a view, lbm_ade_open_slab): the carry of the call, checked (both given with a
// non-empty view -- carry_in where the call reads one -- and distinct) and kept in the call for ade_part_from, which
// enqueues the open pass of the part's rows behind its dispatch and before the interior-wall pass; and the carry of a
// pre-collision state f, written to the call's carry_out (one small launch; none without a listed node)
int ade_carry_set(const char* fn, AdeCall* call, bool reads, const double* carry_in, double* carry_out);
int ade_open_prime_from(const AdeCall& call, const double* f, hipStream_t st);
// capi_diag.hip: what a solver context keeps for its diagnostics -- the row table [LBM_DIAG_NQ][R], the folded values on the
// device and a pinned host buffer for them, all allocated by the first diag_reduce and kept.
struct DiagBuf {
  double* table = nullptr;
  double* out_dev = nullptr;
  double* pinned = nullptr;
  void release();
};
// rows [row_begin, row_end) of the dense fields (conc, profile may be NULL) reduced on `st`: out_host [LBM_DIAG_NQ], and
// the row table [LBM_DIAG_NQ][R] if table_host is given (rows outside the range: 0.0).  Arguments are checked under the
// caller's name fn before any device call; synchronises st.
int diag_reduce(const char* fn, DiagBuf& buf, const double* rho, const double* u, const double* conc, const double* profile,
                int R, int C, int row_begin, int row_end, double* out_host, double* table_host, hipStream_t st);
int diag_range_check(const char* fn, int R, int row_begin, int row_end);
// the arguments of a fold of a row table (out, table given; table_rows positive; the range inside it), shared with the wall
// exchange's folds (capi_ade.hip)
int diag_fold_check(const char* fn, const double* out, const double* table, int table_rows, int row_begin, int row_end);
// the rule's own fields, checked before the context is looked at (its rows: diag_range_check, once the context is known)
int diag_converge_check(const char* fn, const lbm_converge* cv, int max_steps);
// the loop of lbm_solver_run_until / lbm_ade_solver_run_until (lbm_hip.h) over a context's own step(n) -- n iterations, the
// last one leaving moments to reduce -- and value(&v): the watched value of the iteration run last
template <class Step, class Value>
int diag_run_until(const lbm_converge* cv, int max_steps, int* steps_done, int* converged, double* last_value, Step step,
                   Value value) {
  int t = 0, done = 0;
  double old = cv->old_value, last = cv->old_value;
  while (t < max_steps) {
    if (t > 0 && t % cv->interval == cv->offset) {
      if (int rc = value(&last)) return rc;
      const double rel = last / old - 1.0;
      if ((rel < 0 ? -rel : rel) < cv->tolerance) {
        done = 1;
        break;
      }
      old = last;
    }
    long long next = (long long)t - t % cv->interval + cv->offset;  // the next check point after t
    if (next <= t) next += cv->interval;
    const int n = (int)(next < max_steps ? next : max_steps) - t;
    if (int rc = step(n)) return rc;
    t += n;
  }
  if (steps_done) *steps_done = t;
  if (converged) *converged = done;
  if (last_value) *last_value = last;
  return LBM_OK;
}
// NumPy .npy (v1.0, little-endian f64, C order) writer shared by the snapshot objects
int write_npy(const char* path, const double* data, const std::vector<long>& shape);

#define LBM_CHECK_HIP(expr)                                                              \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      ::lbm::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,  \
                       __LINE__);                                                        \
      return LBM_ERR_HIP;                                                                \
    }                                                                                    \
  } while (0)

#define LBM_REQUIRE(cond, ...)        \
  do {                                \
    if (!(cond)) {                    \
      ::lbm::set_error(__VA_ARGS__);  \
      return LBM_ERR_INVALID;         \
    }                                 \
  } while (0)

#define LBM_CHECK_LAUNCH() LBM_CHECK_HIP(hipGetLastError())

// Launch with the thread's sticky error cleared first: the host process (e.g. PyTorch) may
// have left an unrelated, already-handled error behind that hipGetLastError would report.
#define LBM_KLAUNCH(...)               \
  do {                                 \
    (void)hipGetLastError();           \
    hipLaunchKernelGGL(__VA_ARGS__);   \
  } while (0)

// Run-time flags as template arguments: with_flags(f, a, b, ...) calls f(A, B, ...) with std::true_type / std::false_type
// objects, so that a launch site names its kernel ONCE -- K<..., A(), B()> inside a generic lambda -- and all 2^N
// instantiations exist.  A combination that must not be compiled is pruned with `if constexpr` inside the lambda.
template <class F>
auto with_flags(F&& f) {
  return f();
}
template <class F, class... Rest>
auto with_flags(F&& f, bool flag, Rest... rest) {
  if (flag) return with_flags([&](auto... t) { return f(std::true_type{}, t...); }, rest...);
  return with_flags([&](auto... t) { return f(std::false_type{}, t...); }, rest...);
}

inline hipStream_t as_stream(lbm_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// A helper stream that runs work BESIDE a main stream, and the two events that order it: fork(main) -- the helper starts
// after everything enqueued on main so far; join(main) -- main waits for everything enqueued on the helper so far.
struct SideStream {
  hipStream_t st = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;

  explicit operator bool() const { return st != nullptr; }
  // the two events (for an owner that has made `st` itself, e.g. with a priority)
  int create_events() {
    LBM_CHECK_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    LBM_CHECK_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    return LBM_OK;
  }
  // a non-blocking stream (background: make_background_stream) and the events; all of them or, after a failure, none
  int create(bool background = false) {
    int rc = LBM_OK;
    if (background) rc = make_background_stream(&st);
    else if (hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) {
      set_error("hipStreamCreateWithFlags failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
      rc = LBM_ERR_HIP;
    }
    if (!rc) rc = create_events();
    if (rc) destroy();
    return rc;
  }
  // waits for the helper's work, then releases everything; safe on a partly created or never created one
  void destroy() {
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    st = nullptr;
    ev_fork = ev_join = nullptr;
  }
  int fork(hipStream_t main) {
    const int rc = mark(main);
    return rc ? rc : start();
  }
  // fork without an error record, for a caller that falls back to its own stream when the helper cannot be used
  bool try_fork(hipStream_t main) {
    return hipEventRecord(ev_fork, main) == hipSuccess && hipStreamWaitEvent(st, ev_fork, 0) == hipSuccess;
  }
  // fork in two halves, for a caller whose next launches on main are latency-critical: mark(main) fixes the point the helper
  // will start after, start() -- once those launches are enqueued -- makes the helper wait for it (not for them)
  int mark(hipStream_t main) {
    LBM_CHECK_HIP(hipEventRecord(ev_fork, main));
    return LBM_OK;
  }
  int start() {
    LBM_CHECK_HIP(hipStreamWaitEvent(st, ev_fork, 0));
    return LBM_OK;
  }
  // rc != 0: the caller failed after its fork; the join is enqueued all the same, best-effort (nothing left on the helper
  // runs unordered against main's next use of the buffers), and rc is what returns
  int join(hipStream_t main, int rc = LBM_OK) {
    if (rc) {
      if (hipEventRecord(ev_join, st) == hipSuccess) (void)hipStreamWaitEvent(main, ev_join, 0);
      return rc;
    }
    LBM_CHECK_HIP(hipEventRecord(ev_join, st));
    LBM_CHECK_HIP(hipStreamWaitEvent(main, ev_join, 0));
    return LBM_OK;
  }
};

// Grid for a memory-bound grid-stride kernel: enough blocks to fill 256 CUs x 8, no more
// (cdna_hip_programming.md Guideline 11).
inline int capped_grid(long work_items, int cap = 2048) {
  if (work_items < 1) work_items = 1;
  return (int)(work_items < cap ? work_items : cap);
}

}  // namespace lbm
