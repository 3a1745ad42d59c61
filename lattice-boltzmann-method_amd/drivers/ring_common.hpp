// The host of a slab ring, shared by the slab_ring_* drivers: what surrounds a driver's calls into lbm_ring_*.
//   processes   status check, the file rendezvous that distributes the RCCL unique id (no MPI in this image), the
//               fork-one-rank-per-GPU launcher, the common options and main() (ring_main)
//   a rank      its timed launches (timed_ring_run), --check: publishing owned rows and comparing them with one block
//   lattices    geometry, allocation, owned rows as dense planes on the host, the D2Q9 equilibrium of the initial states
//   --emulate   the links between N slabs played on one device (EmulatedLinks) and the ring's second stream (EdgeStream)
#pragma once
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/lbm_hip.h"
#include "common.hpp"

inline void check(int rc, const char* what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + ": " + lbm_last_error_string());
}

inline bool read_file(const std::string& path, void* buf, size_t n) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  size_t got = std::fread(buf, 1, n, f);
  std::fclose(f);
  return got == n;
}
inline void write_file_atomic(const std::string& path, const void* buf, size_t n) {
  std::string tmp = path + ".tmp";
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + tmp);
  std::fwrite(buf, 1, n, f);
  std::fclose(f);
  std::rename(tmp.c_str(), path.c_str());
}
inline void wait_file(const std::string& path, void* buf, size_t n, double timeout_s = 120) {
  auto t0 = std::chrono::steady_clock::now();
  while (!read_file(path, buf, n)) {
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
      throw std::runtime_error("timed out waiting for " + path);
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
  }
}


// fork BEFORE anything touches the GPU; every child is an ordinary one-GPU process.  Children are
// reaped in exit order: the first one that fails takes its peers with it (SIGTERM, then SIGKILL
// after a grace period) -- a rank blocked in ncclCommInitRank / send / recv on a dead peer would
// otherwise hold its GPU until an outer timeout.
template <class F>
int spawn_ranks(int n, F&& run) {
  std::vector<pid_t> kids;
  for (int r = 0; r < n; ++r) {
    pid_t pid = fork();
    if (pid == 0) {
      int rc = 1;
      try {
        rc = run(r);
      } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %d: %s\n", r, e.what());
      }
      std::fflush(nullptr);
      _exit(rc);
    }
    if (pid < 0) {
      std::perror("fork");
      for (pid_t k : kids) kill(k, SIGKILL);  // (all still our un-reaped children here)
      for (pid_t k : kids) waitpid(k, nullptr, 0);
      return 1;
    }
    kids.push_back(pid);
  }
  int worst = 0;
  size_t left = kids.size();
  bool killing = false, killed_hard = false;
  auto t_kill = std::chrono::steady_clock::now();
  while (left > 0) {
    int st = 0;
    pid_t k = waitpid(-1, &st, killing ? WNOHANG : 0);
    if (k > 0) {
      --left;
      for (pid_t& o : kids)
        if (o == k) o = -1;  // reaped: its pid may be handed to an unrelated process from now on -- never signal it again
      const int rc = WIFEXITED(st) ? WEXITSTATUS(st) : 1;
      if (rc != 0 && worst == 0) worst = rc;
      if (rc != 0 && !killing) {  // first failure: stop the survivors
        killing = true;
        t_kill = std::chrono::steady_clock::now();
        for (pid_t o : kids)
          if (o > 0) kill(o, SIGTERM);
      }
    } else if (k == 0) {  // survivors still running after SIGTERM
      if (!killed_hard && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_kill).count() > 5.0) {
        killed_hard = true;  // once
        for (pid_t o : kids)
          if (o > 0) kill(o, SIGKILL);
      }
      std::this_thread::sleep_for(std::chrono::milliseconds(20));
    } else {
      break;  // ECHILD: nothing left to wait for
    }
  }
  return worst;
}
inline void cleanup_ring_files(const std::string& id_file, int n) {
  for (const char* suf : {"", ".tmp"}) std::remove((id_file + suf).c_str());
  for (int r = 0; r < n; ++r)
    for (const char* suf : {".t", ".f", ".g"}) std::remove((id_file + suf + std::to_string(r)).c_str());
}
// rank 0 creates the id and publishes it; the others wait for the file
inline void share_unique_id(unsigned char (&id)[128], int rank, int world, const std::string& id_file) {
  if (rank == 0) {
    check(lbm_ring_unique_id(id), "lbm_ring_unique_id");
    if (world > 1) write_file_atomic(id_file, id, sizeof id);
  } else {
    wait_file(id_file, id, sizeof id);
  }
}
// after the timed launches (and their sync): a rank whose ring has given up on a neighbour -- a bounded wait of the
// peer-mapped transport, an asynchronous RCCL error -- has void lattices and void timings: it says so as JSON and the
// driver returns 4 instead of printing a rate (its peers are ended by the launcher)
inline int ring_failed(lbm_ring* ring, const char* driver, int rank) {
  if (lbm_ring_status(ring) == 0) return 0;
  std::string msg = lbm_last_error_string();
  for (char& ch : msg)
    if (ch == '"' || ch == '\\') ch = '\'';  // (the message goes into a JSON string)
  std::printf("{\"driver\": \"%s\", \"rank\": %d, \"error\": \"%s\"}\n", driver, rank, msg.c_str());
  std::fflush(stdout);
  return 4;
}
// slowest rank's time, gathered on rank 0 through files
inline double max_time_over_ranks(double sec, int rank, int world, const std::string& id_file) {
  double tmax = sec;
  if (world > 1) {
    write_file_atomic(id_file + ".t" + std::to_string(rank), &sec, sizeof sec);
    if (rank == 0)
      for (int r = 1; r < world; ++r) {
        double t;
        wait_file(id_file + ".t" + std::to_string(r), &t, sizeof t);
        tmax = t > tmax ? t : tmax;
      }
  }
  return tmax;
}

// ---- options and main() ------------------------------------------------------------------------------------------------
// what every slab-ring driver takes; a driver's Args derives from it and adds its own flags
struct RingOpts {
  int rows = 0, cols = 0, steps = 0, warmup = 0, edge_rows = 0, check = 0, emulate = 0, spawn = 0, one_gpu = 0;
  std::string id_file, transport;
};
inline int int_arg(int argc, char** argv, const char* key, int dflt) {
  return std::atoi(arg_value(argc, argv, key, std::to_string(dflt)).c_str());
}
// the defaults are the driver's (sizes, steps and edge rows differ between the four)
inline void parse_ring_opts(RingOpts& o, int argc, char** argv, int rows, int cols, int steps, int warmup, int edge_rows) {
  o.rows = int_arg(argc, argv, "--rows", rows);
  o.cols = int_arg(argc, argv, "--cols", cols);
  o.steps = int_arg(argc, argv, "--steps", steps);
  o.warmup = int_arg(argc, argv, "--warmup", warmup);
  o.edge_rows = int_arg(argc, argv, "--edge-rows", edge_rows);
  o.check = int_arg(argc, argv, "--check", 0);
  o.emulate = int_arg(argc, argv, "--emulate", 0);
  o.spawn = int_arg(argc, argv, "--spawn", 0);
  o.one_gpu = int_arg(argc, argv, "--one-gpu", 0);
  o.transport = arg_value(argc, argv, "--transport", "");
  o.id_file = arg_value(argc, argv, "--id-file", "/tmp/lbm_ring_id." + std::to_string((long)getpid()));
}
// the device of a rank: its local rank, or GPU 0 for every rank under --one-gpu 1 / LBM_ONE_GPU (an outside launcher sets
// the variable; with the peer-mapped transport that is N real ranks on one device, which RCCL refuses)
inline int ring_device(int local_rank) { return std::getenv("LBM_ONE_GPU") ? 0 : local_rank; }
// --emulate N (where the driver has an emulation), --spawn N, or one rank of RANK / WORLD_SIZE / LOCAL_RANK under any launcher
template <class A>
int ring_main(const char* name, const A& a, int (*run_rank)(const A&, int rank, int world, int local_rank),
              int (*run_emulated)(const A&, int slabs) = nullptr) {
  // --transport rccl|ipc: what carries the ring's messages (lbm_ring_unique_id / lbm_ring_create follow the environment)
  if (!a.transport.empty()) setenv("LBM_RING_TRANSPORT", a.transport.c_str(), 1);
  if (a.one_gpu) setenv("LBM_ONE_GPU", "1", 1);
  try {
    if (run_emulated && a.emulate > 0) return run_emulated(a, a.emulate);
    if (a.spawn > 0) {
      cleanup_ring_files(a.id_file, a.spawn);  // a stale id file of a killed run must not be picked up
      const int rc = spawn_ranks(a.spawn, [&](int r) { return run_rank(a, r, a.spawn, r); });
      cleanup_ring_files(a.id_file, a.spawn);
      return rc;
    }
    const char* er = std::getenv("RANK");
    const char* ew = std::getenv("WORLD_SIZE");
    const char* el = std::getenv("LOCAL_RANK");
    const int rank = er ? std::atoi(er) : 0, world = ew ? std::atoi(ew) : 1;
    return run_rank(a, rank, world, el ? std::atoi(el) : rank);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s: %s\n", name, e.what());
    return 1;
  }
}

// ---- a rank's timed run ------------------------------------------------------------------------------------------------
// `warmup` launches, then `launches` timed ones; *slowest = the slowest rank's seconds (valid on rank 0).  Returns 0, or
// ring_failed's code when the ring gave up on a neighbour.
template <class F>
int timed_ring_run(lbm_ring* ring, const char* driver, const RingOpts& o, int rank, int world, int warmup, int launches,
                   F&& launch, double* slowest) {
  for (int i = 0; i < warmup; ++i) launch();
  check(lbm_stream_sync(nullptr), "sync");
  // (each rank starts its clock after its own warm-up; the neighbour exchanges keep ranks in step)
  auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < launches; ++i) launch();
  check(lbm_stream_sync(nullptr), "sync");
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (const int failed = ring_failed(ring, driver, rank)) return failed;
  *slowest = max_time_over_ranks(sec, rank, world, o.id_file);
  return 0;
}

// ---- lattices ----------------------------------------------------------------------------------------------------------
// doubles per plane of a lattice (plane_stride 0 = dense: (R + 2 ghost) rows of the row pitch)
inline size_t plane_doubles(const lbm_geom& g) {
  if (g.plane_stride > 0) return (size_t)g.plane_stride;
  return (size_t)(g.R + 2 * g.ghost) * (size_t)(g.row_pitch > 0 ? g.row_pitch : g.C);
}
inline double* alloc_lattice(const lbm_geom& g) {
  const size_t bytes = plane_doubles(g) * 9 * 8;
  if (bytes == 0) throw std::runtime_error("empty lattice");
  double* p = nullptr;
  check(lbm_malloc((void**)&p, bytes), "lbm_malloc");
  check(lbm_memset(p, 0, bytes, nullptr), "memset");
  return p;
}
// rows padded off a power-of-two stride like the solver contexts' (lbm_default_row_pitch: +3 % for the two-phase kernel
// at 2048 columns); the planes stay (R + 2G) rows of that pitch
inline lbm_geom row_padded_geom(int R, int C, int G) {
  const int pitch = lbm_default_row_pitch(C);
  return lbm_geom{R, C, G, (long long)(R + 2 * G) * pitch, pitch > C ? pitch : 0};
}
// padded like the solver contexts' lattices (rows off a power-of-two stride, planes off a power-of-two size)
inline lbm_geom padded_geom(int R, int C, int G) {
  const int pitch = lbm_default_row_pitch(C);
  long long plane = (long long)(R + 2 * G) * pitch + lbm_default_plane_pad(R + 2 * G, pitch);
  plane += plane & 1;  // even: 16-byte accesses
  return lbm_geom{R, C, G, plane, pitch > C ? pitch : 0};
}
// owned rows of a lattice of any geometry as dense [9][R][C] on the host
inline std::vector<double> owned_to_host(const double* lat, const lbm_geom& g) {
  const lbm_geom d{g.R, g.C, 0, 0, 0};
  std::vector<double> out((size_t)9 * g.R * g.C);
  double* dense = nullptr;
  check(lbm_malloc((void**)&dense, out.size() * 8), "lbm_malloc");
  check(lbm_lattice_copy_rows(dense, &d, 0, lat, &g, 0, g.R, nullptr), "lbm_lattice_copy_rows");
  check(lbm_memcpy_d2h(out.data(), dense, out.size() * 8, nullptr), "d2h");
  check(lbm_stream_sync(nullptr), "sync");
  lbm_free(dense);
  return out;
}
// compressible D2Q9 equilibrium of (rho, u) in the reference's operation order (solver.cpp:51-62): the initial states are
// the same bits for every decomposition
inline void d2q9_equilibrium(double* e, double rho, double u0, double u1) {
  static const double w[9] = {4. / 9, 1. / 9, 1. / 9, 1. / 9, 1. / 9, 1. / 36, 1. / 36, 1. / 36, 1. / 36};
  static const int cx[9] = {0, 1, 0, -1, 0, 1, -1, -1, 1}, cy[9] = {0, 0, 1, 0, -1, 1, 1, -1, -1};
  const double uu = u0 * u0 + u1 * u1;
  for (int q = 0; q < 9; ++q) {
    const double cu = cx[q] * u0 + cy[q] * u1;
    e[q] = w[q] * rho * (1.0 + 3.0 * cu + 4.5 * cu * cu - 1.5 * uu);
  }
}

// ---- --check -----------------------------------------------------------------------------------------------------------
// every rank publishes the owned rows of a lattice as dense [9][R][C]; rank 0 reads rank r's (R = that rank's height)
inline void publish_owned_rows(const RingOpts& o, const char* suffix, int rank, const double* lat, const lbm_geom& g) {
  const std::vector<double> own = owned_to_host(lat, g);
  write_file_atomic(o.id_file + suffix + std::to_string(rank), own.data(), own.size() * 8);
}
inline std::vector<double> read_owned_rows(const RingOpts& o, const char* suffix, int rank, int R, int C) {
  std::vector<double> own((size_t)9 * R * C);
  wait_file(o.id_file + suffix + std::to_string(rank), own.data(), own.size() * 8);
  return own;
}
// planes of a slab (dense [9][R][C], first global row row0) that differ from the one block's (dense [9][Rg][C]) in any bit
inline int mismatching_planes(const std::vector<double>& one_block, int Rg, const std::vector<double>& slab, int R, int row0, int C) {
  int bad = 0;
  for (int q = 0; q < 9; ++q)
    if (std::memcmp(&slab[(size_t)q * R * C], &one_block[(size_t)q * Rg * C + (size_t)row0 * C], (size_t)R * C * 8) != 0) ++bad;
  return bad;
}
// a device array of n doubles, zeroed (NULL for n = 0), and its copy on the host: the carry of an open table, which --check
// compares beside the lattices
inline double* alloc_doubles(size_t n) {
  if (n == 0) return nullptr;
  double* d = nullptr;
  check(lbm_malloc((void**)&d, n * 8), "lbm_malloc");
  check(lbm_memset(d, 0, n * 8, nullptr), "lbm_memset");
  return d;
}
inline std::vector<double> doubles_to_host(const double* d, size_t n) {
  std::vector<double> h(n);
  if (n) check(lbm_memcpy_d2h(h.data(), d, n * 8, nullptr), "lbm_memcpy_d2h");
  check(lbm_stream_sync(nullptr), "sync");
  return h;
}
// true if the two arrays differ in any bit
inline bool mismatching_doubles(const double* a, const double* b, size_t n) { return n && std::memcmp(a, b, n * 8) != 0; }
// the tail of a driver's JSON line
inline const char* check_field(int check, int bad) {
  return !check ? "" : (bad ? ", \"check\": \"MISMATCH\"" : ", \"check\": \"bitwise equal to one block\"");
}

// ---- --emulate N: the slabs of a ring in turn on one device ----------------------------------------------------------------
// The links between the slabs: per slab and side a send and a receive buffer, the messages delivered by device copies on
// the main stream; and per slab `intervals` event pairs on the main stream, whose times add up over the timed steps.
class EmulatedLinks {
 public:
  // closed: slab N-1's next is slab 0 (a periodic ring); otherwise a chain whose end slabs lack a neighbour
  EmulatedLinks(int slabs, bool closed, int intervals = 1) : closed_(closed), iv_(intervals), s_(slabs) {
    for (Slab& s : s_) {
      s.ev.resize(2 * intervals, nullptr);
      for (void*& e : s.ev) check(lbm_event_create(&e), "lbm_event_create");
    }
  }
  EmulatedLinks(const EmulatedLinks&) = delete;
  ~EmulatedLinks() {
    for (Slab& s : s_) {
      for (double* p : {s.buf[0][0], s.buf[0][1], s.buf[1][0], s.buf[1][1]}) lbm_free(p);
      for (void* e : s.ev) lbm_event_destroy(e);
    }
  }
  int slabs() const { return (int)s_.size(); }
  bool prev(int k) const { return closed_ || k > 0; }
  bool next(int k) const { return closed_ || k < slabs() - 1; }
  bool has(int k, int side) const { return side ? next(k) : prev(k); }
  // side 0: towards slab k-1, side 1: towards slab k+1
  void alloc(int k, int side, size_t send_doubles, size_t recv_doubles) {
    check(lbm_malloc((void**)&s_[k].buf[side][0], send_doubles * 8), "lbm_malloc");
    check(lbm_malloc((void**)&s_[k].buf[side][1], recv_doubles * 8), "lbm_malloc");
  }
  double* send(int k, int side) const { return s_[k].buf[side][0]; }
  double* recv(int k, int side) const { return s_[k].buf[side][1]; }
  // the seam behind slab k: its message for the next slab (`down` doubles) and the next slab's for it (`up`)
  void deliver_seam(int k, size_t down, size_t up) {
    const int n = (k + 1) % slabs();
    check(lbm_memcpy_d2d(recv(n, 0), send(k, 1), down * 8, nullptr), "d2d");
    check(lbm_memcpy_d2d(recv(k, 1), send(n, 0), up * 8, nullptr), "d2d");
  }
  void deliver(size_t doubles) {
    for (int k = 0; k < slabs(); ++k)
      if (next(k)) deliver_seam(k, doubles, doubles);
  }
  void begin(int k, int interval = 0) { check(lbm_event_record(s_[k].ev[2 * interval], nullptr), "event"); }
  void end(int k, int interval = 0) { check(lbm_event_record(s_[k].ev[2 * interval + 1], nullptr), "event"); }
  // after a step's begin / end pairs of slab k: their times, counted when the step is a timed one
  void add_elapsed(int k, bool timed) {
    for (int i = 0; i < iv_; ++i) {
      float m = 0;
      check(lbm_event_elapsed_ms(&m, s_[k].ev[2 * i], s_[k].ev[2 * i + 1]), "elapsed");
      if (timed) s_[k].ms += m;
    }
  }
  double ms(int k) const { return s_[k].ms; }
  double slowest_ms() const {
    double m = 0;
    for (const Slab& s : s_) m = std::max(m, s.ms);
    return m;
  }

 private:
  struct Slab {
    double* buf[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [side][send / recv]
    std::vector<void*> ev;
    double ms = 0;
  };
  bool closed_;
  int iv_;
  std::vector<Slab> s_;
};

// the ring's two streams: edge (frame of the slab, pack, exchange) beside main (the inner rectangle).  fork(): what is
// enqueued on `edge` from now on waits for main's work so far; join(): main waits for edge's.
struct EdgeStream {
  lbm_stream_t edge = nullptr;
  void *ev_fork = nullptr, *ev_join = nullptr;
  EdgeStream() {
    check(lbm_stream_create(&edge), "lbm_stream_create");
    check(lbm_event_create(&ev_fork), "lbm_event_create");
    check(lbm_event_create(&ev_join), "lbm_event_create");
  }
  EdgeStream(const EdgeStream&) = delete;
  ~EdgeStream() {
    lbm_event_destroy(ev_fork);
    lbm_event_destroy(ev_join);
    lbm_stream_destroy(edge);
  }
  void fork() {
    check(lbm_event_record(ev_fork, nullptr), "event");
    check(lbm_stream_wait_event(edge, ev_fork), "wait");
  }
  void join() {
    check(lbm_event_record(ev_join, edge), "event");
    check(lbm_stream_wait_event(nullptr, ev_join), "wait");
  }
};
