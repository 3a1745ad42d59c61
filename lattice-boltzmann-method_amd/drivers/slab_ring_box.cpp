// Periodic BGK box, slab-decomposed along r over the GPUs of one node: the C++ host of the
// multi-GPU path (north star: "halo exchange via RCCL send/recv over xGMI overlapped with interior
// collision on a second HIP stream").  One process per GPU.
//
//   slab_ring_box --spawn N [...]          fork N ranks on this node (rank i -> GPU i)
//   RANK=i WORLD_SIZE=N LOCAL_RANK=i slab_ring_box --id-file /tmp/x [...]   under any launcher
//
// Options: --rows R (per GPU, weak scaling) --cols C --steps K (launch-steps timed) --warmup W
//          --depth D (time steps per launch, 1..6; KBC: 1..4) --period P (launches per halo exchange,
//          ghost rows = P x D; default 2) --edge-rows E --omega w
//          --model bgk|kbc (kbc: the entropic KBC collision with s2 = omega, config 3 over slabs)
//          --check 1 (N ranks vs rank 0 recomputing the whole box: small sizes only)
//          --desert R (fault injection: rank R joins the ring and leaves; the others must report it and return 4)
//
// The block binding this generalises: test/decompose_domain.cpp:181-187 (3 populations per
// interface row, one row per step); here 9(D-1) rows per side per D-step launch (3 for D = 1).
//
// The calls that make a host are all in run_rank, in order; what surrounds them (options, main(), the timed run,
// --check's files and comparison) is ring_common.hpp.
#include <cmath>

#include "ring_common.hpp"

namespace {

// Taylor-Green-like smooth field on the GLOBAL box -> compressible equilibrium (solver.cpp:51-62)
// for global row gr, column c; written in the reference's operation order so that the N-rank and
// the 1-rank initial states are the same bits.
void init_node(double* f9, int gr, int c, int Rg, int C) {
  const double pi = 3.14159265358979323846;
  const double x = 2 * pi * gr / Rg, y = 2 * pi * c / C;
  const double u0 = 0.04 * std::sin(x) * std::cos(y), u1 = -0.04 * std::cos(x) * std::sin(y);
  const double rho = 1.0 + 0.01 * std::cos(2 * x);
  d2q9_equilibrium(f9, rho, u0, u1);
}

struct Args : RingOpts {
  int depth = 5, period = 2, desert = -1;
  double omega = 1.2;
  bool kbc = false;
};

// post-collision slab lattice [9][R+2D][C] of rows [row0, row0+R) of an Rg x C box
double* make_slab(const Args& a, int R, int row0, int Rg, const lbm_geom& g, const lbm_bgk_params& prm) {
  const int C = a.cols, D = g.ghost;
  const size_t plane = plane_doubles(g);
  std::vector<double> h(9 * plane, 0.0);
  double f9[9];
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < C; ++c) {
      init_node(f9, row0 + r, c, Rg, C);
      for (int q = 0; q < 9; ++q) h[q * plane + (size_t)(r + D) * C + c] = f9[q];
    }
  double* pre = nullptr;
  check(lbm_malloc((void**)&pre, 9 * plane * sizeof(double)), "lbm_malloc");
  double* post = alloc_lattice(g);
  check(lbm_memcpy_h2d(pre, h.data(), 9 * plane * sizeof(double), nullptr), "h2d");
  // the collide-only launch that opens the post-collision-resident loop (ghost rows: collide of
  // zeros stays in the ghost rows and is overwritten by the first exchange)
  if (a.kbc) {
    lbm_kbc_params kp{prm.omega, LBM_FORM_DEFAULT};
    check(lbm_kbc_collide(post, pre, &g, nullptr, &kp, nullptr, nullptr, nullptr), "lbm_kbc_collide");
  } else {
    check(lbm_bgk_collide(post, pre, &g, nullptr, &prm, nullptr, nullptr, nullptr), "lbm_bgk_collide");
  }
  check(lbm_stream_sync(nullptr), "sync");
  lbm_free(pre);
  return post;
}

int run_rank(const Args& a, int rank, int world, int local_rank) {
  check(lbm_set_device(ring_device(local_rank)), "lbm_set_device");
  const int R = a.rows, C = a.cols, D = a.depth, Rg = R * world;
  // ghost = period x D rows: lbm_ring_bgk_step / _kbc_step exchange once per `period` launches
  const int G = D * (D < 2 ? 1 : a.period);
  lbm_geom g{R, C, G, 0, 0};
  lbm_bgk_params prm{};
  prm.omega = a.omega;
  lbm_kbc_params kprm{a.omega, LBM_FORM_DEFAULT};

  unsigned char id[128];
  share_unique_id(id, rank, world, a.id_file);
  lbm_ring* ring = nullptr;
  check(lbm_ring_create(&ring, id, rank, world, &g, /*periodic=*/1), "lbm_ring_create");
  if (rank == a.desert) {  // joined, mapped, gone
    std::fflush(nullptr);
    _exit(0);
  }

  double* lat[2];
  lat[0] = make_slab(a, R, rank * R, Rg, g, prm);
  lat[1] = alloc_lattice(g);
  check(lbm_ring_exchange(ring, lat[0], nullptr), "lbm_ring_exchange");
  check(lbm_ring_join(ring, nullptr), "lbm_ring_join");

  int cur = 0;
  auto launch = [&]() {
    if (a.kbc) check(lbm_ring_kbc_step(ring, lat[cur ^ 1], lat[cur], nullptr, &kprm, D, a.edge_rows, nullptr), "lbm_ring_kbc_step");
    else check(lbm_ring_bgk_step(ring, lat[cur ^ 1], lat[cur], nullptr, &prm, D, a.edge_rows, nullptr), "lbm_ring_bgk_step");
    cur ^= 1;
  };
  // the rate: all nodes / the slowest rank's time (gathered through files: no MPI here)
  double tmax = 0;
  if (const int failed = timed_ring_run(ring, "slab_ring_box", a, rank, world, a.warmup, a.steps, launch, &tmax)) return failed;

  int bad = 0;
  if (a.check) {
    // every rank dumps its owned rows; rank 0 recomputes the whole box on its own GPU (ghost 0,
    // periodic wrap inside the block) and compares bit for bit
    publish_owned_rows(a, ".f", rank, lat[cur], g);
    if (rank == 0) {
      lbm_geom gw{Rg, C, 0, 0, 0};
      double* p = make_slab(a, Rg, 0, Rg, gw, prm);
      double* q2 = nullptr;
      check(lbm_malloc((void**)&q2, plane_doubles(gw) * 9 * sizeof(double)), "lbm_malloc");
      const int total = (a.warmup + a.steps) * D;
      for (int t = 0; t < total; ++t) {
        if (a.kbc) check(lbm_kbc_stream_collide(q2, p, &gw, nullptr, &kprm, 0, Rg, nullptr, nullptr, nullptr), "ref step");
        else check(lbm_bgk_stream_collide(q2, p, &gw, nullptr, &prm, 0, Rg, nullptr, nullptr, nullptr), "ref step");
        std::swap(p, q2);
      }
      const std::vector<double> want = owned_to_host(p, gw);
      for (int r = 0; r < world; ++r) bad += mismatching_planes(want, Rg, read_owned_rows(a, ".f", r, R, C), R, r * R, C);
      lbm_free(p);
      lbm_free(q2);
    }
  }

  if (rank == 0) {
    const double lups = (double)Rg * C * D * a.steps / tmax;
    std::printf("{\"driver\": \"slab_ring_box\", \"model\": \"%s\", \"n_gpus\": %d, \"rows_per_gpu\": %d, \"cols\": %d, "
                "\"depth\": %d, \"ghost_rows\": %d, \"launches\": %d, \"ms_per_launch\": %.4f, \"mlups\": %.1f, "
                "\"transport\": \"rccl send/recv (C++ ring)\"%s}\n",
                a.kbc ? "kbc" : "bgk", world, R, C, D, G, a.steps, 1e3 * tmax / a.steps, lups / 1e6,
                check_field(a.check, bad));
    std::fflush(stdout);
  }
  lbm_ring_destroy(ring);
  lbm_free(lat[0]);
  lbm_free(lat[1]);
  return bad ? 3 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  parse_ring_opts(a, argc, argv, /*rows=*/8192, /*cols=*/8192, /*steps=*/20, /*warmup=*/5, /*edge_rows=*/32);
  a.depth = int_arg(argc, argv, "--depth", 5);
  a.period = std::max(1, std::min(3, int_arg(argc, argv, "--period", 2)));
  a.desert = int_arg(argc, argv, "--desert", -1);
  a.omega = std::atof(arg_value(argc, argv, "--omega", "1.2").c_str());
  a.kbc = arg_value(argc, argv, "--model", "bgk") == "kbc";
  if (a.kbc && a.depth > 4) a.depth = 3;
  return ring_main("slab_ring_box", a, run_rank);  // (no emulation: --emulate is not a flag of this driver)
}
