// Rayleigh-Taylor two-phase run (BASELINE config 4) slab-decomposed along r over the GPUs of one
// node: a CHAIN of slabs (rows 0 and R-1 of the global domain are the driver's bounce-back walls,
// test/mrtcg_rayleigh_taylor.cpp:525-531), 3 ghost rows per colour, ONE packed message per
// neighbour per step (both colours), exchange overlapped with the interior rows.  C++ host on
// lbm_ring_* + lbm_cg_step_fused; one process per GPU.
//
//   slab_ring_rt --spawn N [--rows R_per_gpu] [--cols C] [--steps K] [--warmup W] [--edge-rows E]
//                [--check 1]   (rank 0 recomputes the whole domain as one block: small sizes only)
//                [--transport rccl|ipc] [--one-gpu 1]  (ipc + one-gpu: N real ranks sharing GPU 0 through the
//                peer-mapped transport -- RCCL refuses two ranks on one device)
//   slab_ring_rt --emulate N ...   ONE process / one GPU playing all N slabs of the chain in turn (edge rows, interior
//                rows, pack -> device copy -> unpack of the 3 ghost rows of both colours, per-slab time by HIP events;
//                --check 1: bitwise against the single block) -- BASELINE config 4 = --emulate 4 --rows 2048 --cols 2048
//   RANK=i WORLD_SIZE=N LOCAL_RANK=i slab_ring_rt --id-file /tmp/x ...     under any launcher
//
// Parameters: [red]/[blue] of mrtcg-rayleigh-taylor-gamma3.toml, sigma = 0.1, g = 6.25e-6
// (SURVEY 8d, C4); initial state = init_rho_cosine (:182-210), u = 0, f = feq.
//
// run_rank / run_emulated hold the model and its lbm_ring_* calls; options, main(), the timed run, --check's comparison
// and the emulation's links are ring_common.hpp.
#include <cmath>

#include "ring_common.hpp"

namespace {

struct Args : RingOpts {
  int parts = 1;  // 0: the emulated chain with round 3's three row ranges per step
};

lbm_cg_params rt_params() {
  lbm_cg_params p{};
  p.red = lbm_cg_colour{3.0, 0.7, 0.04, 0.7};
  p.blue = lbm_cg_colour{1.0, 0.1, 0.04, -0.7};
  p.sigma = 0.1;
  p.gravity_r = 6.25e-6;
  p.gravity_c = 0.0;
  p.add_source = 1;
  p.delta = 0.1;
  return p;
}

// the one block of --check: Rg x C without ghost rows, dense as the reference holds its tensors (the plane stride spelt out)
lbm_geom one_block_geom(int Rg, int C) { return lbm_geom{Rg, C, 0, (long long)Rg * C, 0}; }

// Post-collision lattices of rows [row0, row0 + R) of an Rg x C domain, ghost rows G (0 or 3):
// densities by init_rho_cosine, f = feq(rho_k, u = 0), then the driver's first collision
// (lbm_cg_collide on the given rho, u).  The macroscopic arrays of a slab carry 2 ghost rows.
void make_slab(int R, int C, int row0, int Rg, const lbm_geom& g, const lbm_bc& bc,
               const lbm_cg_params& prm, double** post_r, double** post_b) {
  const int G = g.ghost, mg = G ? 2 : 0;
  const size_t mplane = (size_t)(R + 2 * mg) * C;
  std::vector<double> hr(mplane), hb(mplane);
  for (int r = -mg; r < R + mg; ++r) {
    int gr = row0 + r;
    gr = gr < 0 ? 0 : (gr > Rg - 1 ? Rg - 1 : gr);
    for (int c = 0; c < C; ++c) {
      const double s = Rg / 2.0 - 0.1 * C * std::cos(2.0 * 3.141592 * c / C);  // :196-199
      const bool red = gr < s;
      hr[(size_t)(r + mg) * C + c] = red ? prm.red.rho_0 : 0.0;
      hb[(size_t)(r + mg) * C + c] = red ? 0.0 : prm.blue.rho_0;
    }
  }
  double *d_rr, *d_rb, *d_u;
  check(lbm_malloc((void**)&d_rr, mplane * 8), "lbm_malloc");
  check(lbm_malloc((void**)&d_rb, mplane * 8), "lbm_malloc");
  check(lbm_malloc((void**)&d_u, 2 * mplane * 8), "lbm_malloc");
  double *pre_r = alloc_lattice(g), *pre_b = alloc_lattice(g);
  *post_r = alloc_lattice(g);
  *post_b = alloc_lattice(g);
  check(lbm_memcpy_h2d(d_rr, hr.data(), mplane * 8, nullptr), "h2d");
  check(lbm_memcpy_h2d(d_rb, hb.data(), mplane * 8, nullptr), "h2d");
  check(lbm_memset(d_u, 0, 2 * mplane * 8, nullptr), "memset");
  // feq on the owned rows (u = 0: dense zeros) as dense planes, then into the ghosted, row-padded lattices
  {
    double* eq = nullptr;
    check(lbm_malloc((void**)&eq, (size_t)9 * R * C * 8), "lbm_malloc");
    const lbm_geom dense{R, C, 0, 0, 0};
    check(lbm_cg_equilibrium(eq, d_rr + (size_t)mg * C, d_u, &prm.red, R, C, 0, nullptr), "lbm_cg_equilibrium");
    check(lbm_lattice_copy_rows(pre_r, &g, 0, eq, &dense, 0, R, nullptr), "lbm_lattice_copy_rows");
    check(lbm_cg_equilibrium(eq, d_rb + (size_t)mg * C, d_u, &prm.blue, R, C, 0, nullptr), "lbm_cg_equilibrium");
    check(lbm_lattice_copy_rows(pre_b, &g, 0, eq, &dense, 0, R, nullptr), "lbm_lattice_copy_rows");
    check(lbm_stream_sync(nullptr), "sync");
    lbm_free(eq);
  }
  check(lbm_cg_collide(*post_r, *post_b, pre_r, pre_b, d_rr, d_rb, d_u, &g, &bc, &prm, nullptr, nullptr, nullptr), "lbm_cg_collide");
  check(lbm_stream_sync(nullptr), "sync");
  for (double* p : {d_rr, d_rb, d_u, pre_r, pre_b}) lbm_free(p);
}

// The yardstick of --check: the whole Rg x C domain as one block, warmup + steps fused steps; both colours' populations
// as dense [9][Rg][C] on the host
void one_block(const Args& a, int Rg, const lbm_cg_params& prm, std::vector<double> (&want)[2]) {
  const lbm_geom gw = one_block_geom(Rg, a.cols);
  lbm_bc bw;
  lbm_cg_default_bc(&bw);
  double *p[2], *q2[2];
  make_slab(Rg, a.cols, 0, Rg, gw, bw, prm, &p[0], &p[1]);
  for (int k = 0; k < 2; ++k) check(lbm_malloc((void**)&q2[k], plane_doubles(gw) * 9 * 8), "lbm_malloc");
  for (int t = 0; t < a.warmup + a.steps; ++t) {
    check(lbm_cg_step_fused(q2[0], q2[1], p[0], p[1], &gw, &bw, &prm, 0, Rg, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr), "lbm_cg_step_fused");
    std::swap(p[0], q2[0]);
    std::swap(p[1], q2[1]);
  }
  for (int k = 0; k < 2; ++k) {
    want[k] = owned_to_host(p[k], gw);
    lbm_free(p[k]);
    lbm_free(q2[k]);
  }
}

int run_rank(const Args& a, int rank, int world, int local_rank) {
  check(lbm_set_device(ring_device(local_rank)), "lbm_set_device");
  const int R = a.rows, C = a.cols, Rg = R * world, G = 3;
  const lbm_cg_params prm = rt_params();
  const lbm_geom g = row_padded_geom(R, C, G);
  lbm_bc bc;
  lbm_cg_default_bc(&bc);
  if (rank > 0) bc.row_lo = LBM_EDGE_HALO;
  if (rank < world - 1) bc.row_hi = LBM_EDGE_HALO;

  unsigned char id[128];
  share_unique_id(id, rank, world, a.id_file);
  lbm_ring* ring = nullptr;
  check(lbm_ring_create(&ring, id, rank, world, &g, /*periodic=*/0), "lbm_ring_create");

  double* lat[2][2];
  make_slab(R, C, rank * R, Rg, g, bc, prm, &lat[0][0], &lat[0][1]);
  for (int k = 0; k < 2; ++k) lat[1][k] = alloc_lattice(g);
  check(lbm_ring_exchange2(ring, lat[0][0], lat[0][1], nullptr), "lbm_ring_exchange2");
  check(lbm_ring_join(ring, nullptr), "lbm_ring_join");

  int cur = 0;
  auto step = [&]() {
    check(lbm_ring_cg_step(ring, lat[cur ^ 1][0], lat[cur ^ 1][1], lat[cur][0], lat[cur][1], nullptr, &prm,
                           a.edge_rows, nullptr), "lbm_ring_cg_step");
    cur ^= 1;
  };
  double tmax = 0;
  if (const int failed = timed_ring_run(ring, "slab_ring_rt", a, rank, world, a.warmup, a.steps, step, &tmax)) return failed;

  int bad = 0;
  if (a.check) {
    for (int k = 0; k < 2; ++k) publish_owned_rows(a, k ? ".g" : ".f", rank, lat[cur][k], g);
    if (rank == 0) {
      std::vector<double> want[2];
      one_block(a, Rg, prm, want);
      for (int k = 0; k < 2; ++k)
        for (int r = 0; r < world; ++r) bad += mismatching_planes(want[k], Rg, read_owned_rows(a, k ? ".g" : ".f", r, R, C), R, r * R, C);
    }
  }
  if (rank == 0) {
    std::printf("{\"driver\": \"slab_ring_rt\", \"n_gpus\": %d, \"rows_per_gpu\": %d, \"cols\": %d, \"steps\": %d, "
                "\"ms_per_step\": %.4f, \"mlups\": %.1f, \"transport\": \"%s (C++ ring)\"%s}\n",
                world, R, C, a.steps, 1e3 * tmax / a.steps, (double)Rg * C * a.steps / tmax / 1e6,
                lbm_ring_transport(ring) == LBM_RING_IPC ? "peer-mapped windows" : "rccl send/recv",
                check_field(a.check, bad));
    std::fflush(stdout);
  }
  lbm_ring_destroy(ring);
  for (int b = 0; b < 2; ++b)
    for (int k = 0; k < 2; ++k) lbm_free(lat[b][k]);
  return bad ? 3 : 0;
}

// --emulate N: every slab of the chain in turn on ONE GPU; the messages of lbm_ring_cg_step (LBM_HALO_TWO_PHASE: 21 rows per
// colour and side) travel by device copies.  Same kernels on the same row ranges as a rank of the ring runs.
int run_emulated(const Args& a, int N) {
  check(lbm_set_device(0), "lbm_set_device");
  const int R = a.rows, C = a.cols, Rg = R * N, G = 3, E = a.edge_rows < G ? G : a.edge_rows;
  if (2 * E >= R) throw std::runtime_error("--edge-rows too large for these slabs");
  const lbm_cg_params prm = rt_params();
  const lbm_geom g = row_padded_geom(R, C, G);
  const size_t msg = (size_t)lbm_halo_rows(LBM_HALO_TWO_PHASE) * C;
  struct Slab {
    lbm_bc bc;
    double* lat[2][2];   // [buffer][colour]
  };
  std::vector<Slab> S(N);
  EmulatedLinks links(N, /*closed=*/false);  // a message: both colours back to back
  for (int r = 0; r < N; ++r) {
    lbm_cg_default_bc(&S[r].bc);
    if (links.prev(r)) S[r].bc.row_lo = LBM_EDGE_HALO;
    if (links.next(r)) S[r].bc.row_hi = LBM_EDGE_HALO;
    make_slab(R, C, r * R, Rg, g, S[r].bc, prm, &S[r].lat[0][0], &S[r].lat[0][1]);
    for (int k = 0; k < 2; ++k) S[r].lat[1][k] = alloc_lattice(g);
    for (int side = 0; side < 2; ++side) links.alloc(r, side, 2 * msg, 2 * msg);
  }
  EdgeStream es;
  auto pack = [&](int r, int cur, lbm_stream_t st) {
    for (int k = 0; k < 2; ++k)
      for (int side = 0; side < 2; ++side)
        if (links.has(r, side))
          check(lbm_halo_pack(links.send(r, side) + k * msg, S[r].lat[cur][k], &g, LBM_HALO_TWO_PHASE, side, st), "lbm_halo_pack");
  };
  auto unpack = [&](int r, int cur) {
    for (int k = 0; k < 2; ++k)
      for (int side = 0; side < 2; ++side)
        if (links.has(r, side))
          check(lbm_halo_unpack(S[r].lat[cur][k], links.recv(r, side) + k * msg, &g, LBM_HALO_TWO_PHASE, side, nullptr), "lbm_halo_unpack");
  };
  int cur = 0;
  for (int r = 0; r < N; ++r) pack(r, cur, nullptr);
  links.deliver(2 * msg);
  for (int r = 0; r < N; ++r) unpack(r, cur);
  for (int i = 0; i < a.warmup + a.steps; ++i) {
    for (int r = 0; r < N; ++r) {  // a slab's step as lbm_ring_cg_step enqueues it
      links.begin(r);
      auto rows = [&](int r0, int r1) {
        check(lbm_cg_step_fused(S[r].lat[cur ^ 1][0], S[r].lat[cur ^ 1][1], S[r].lat[cur][0], S[r].lat[cur][1], &g, &S[r].bc, &prm, r0, r1,
                                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "lbm_cg_step_fused");
      };
      auto part = [&](int which, lbm_stream_t st) {
        check(lbm_cg_step_fused_part(S[r].lat[cur ^ 1][0], S[r].lat[cur ^ 1][1], S[r].lat[cur][0], S[r].lat[cur][1], &g, &S[r].bc, &prm, which, E,
                                     nullptr, nullptr, nullptr, nullptr, nullptr, st), "lbm_cg_step_fused_part");
      };
      if (N > 1 && a.parts) {
        // frame (wall / copy columns + the first and last edge rows) and the messages on the edge stream, the inner
        // rectangle on the main stream beside them; the step ends when both have
        es.fork();
        part(LBM_CG_PART_FRAME, es.edge);
        part(LBM_CG_PART_INNER, nullptr);
        pack(r, cur ^ 1, es.edge);
        es.join();
      } else if (N > 1) {  // round 3: three row ranges, each a frame + inner pair
        rows(0, E);
        rows(R - E, R);
        rows(E, R - E);
        pack(r, cur ^ 1, nullptr);
      } else {
        rows(0, R);
        pack(r, cur ^ 1, nullptr);
      }
      links.end(r);
    }
    links.deliver(2 * msg);
    for (int r = 0; r < N; ++r) unpack(r, cur ^ 1);
    for (int r = 0; r < N; ++r) links.add_elapsed(r, i >= a.warmup);
    cur ^= 1;
  }
  check(lbm_stream_sync(es.edge), "sync");
  int bad = 0;
  if (a.check) {
    std::vector<double> want[2];
    one_block(a, Rg, prm, want);
    for (int k = 0; k < 2; ++k)
      for (int r = 0; r < N; ++r) bad += mismatching_planes(want[k], Rg, owned_to_host(S[r].lat[cur][k], g), R, r * R, C);
  }
  const double slowest = links.slowest_ms() / a.steps;
  std::printf("{\"driver\": \"slab_ring_rt\", \"mode\": \"emulated chain on one GPU\", \"slabs\": %d, \"rows_per_slab\": %d, \"cols\": %d, "
              "\"global_rows\": %d, \"steps\": %d, \"edge_rows\": %d, \"message_rows_per_colour_and_side\": %d, \"slowest_slab_ms_per_step\": %.4f, "
              "\"chain_mlups_at_the_slowest_slabs_pace\": %.1f, \"per_slab\": [",
              N, R, C, Rg, a.steps, E, lbm_halo_rows(LBM_HALO_TWO_PHASE), slowest, (double)Rg * C / slowest / 1e3);
  for (int r = 0; r < N; ++r)
    std::printf("%s{\"slab\": %d, \"ms_per_step\": %.4f, \"mlups\": %.1f}", r ? ", " : "", r, links.ms(r) / a.steps, (double)R * C / (links.ms(r) / a.steps) / 1e3);
  std::printf("]%s}\n", check_field(a.check, bad));
  std::fflush(stdout);
  for (auto& sb : S)
    for (int x = 0; x < 2; ++x)
      for (int k = 0; k < 2; ++k) lbm_free(sb.lat[x][k]);
  return bad ? 3 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  parse_ring_opts(a, argc, argv, /*rows=*/2048, /*cols=*/2048, /*steps=*/50, /*warmup=*/5, /*edge_rows=*/16);
  a.parts = int_arg(argc, argv, "--parts", 1);
  return ring_main("slab_ring_rt", a, run_rank, run_emulated);
}
