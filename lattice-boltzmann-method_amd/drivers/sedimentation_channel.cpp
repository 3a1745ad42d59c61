// A body in a channel with an inlet and an outlet, a sediment settling on it: the fluid + transported-scalar loop on
// lbm::AdeSolver with either fluid, the open-boundary table of the sedimentation channel (lbm::AdeOpenBoundary::
// channel: velocity inlet, zero-gradient outlet, specular lid, the scalar held at conc_w over the top conc_rows of the
// inlet), a bounce-back floor and, optionally, the rectangle standing on it as interior walls.  This project's own driver,
// not a restatement of a reference main.
//   usage: sedimentation_channel R C steps omega omega_g w_r w_c [--fluid bgk|kbc] [--s2 X] [--form 0|1|2]
//          [--u-in X] [--conc-w X] [--conc-rows N] [--rectangle r_top,c_first,c_second[,conc]]
//          [--buoyancy beta_r,beta_c,c_ref[,u_shift,guo_a,guo_b]] [--exchange 0|1] [--dump prefix] [--time 0|1]
// --fluid kbc: the entropic KBC collision with the rate --s2 (default: omega), through lbm::AdeSolver::kbc, set_open_m,
// set_buoyancy_m and wall_exchange_m -- which on a BGK context are set_open, set_buoyancy and wall_exchange themselves.
// Initial state, for either fluid: rho = 1, u = (U0 sin(2 pi c / C), u_in) -- a shear wave drifting towards the outlet --
// f as the reference's KBC driver starts (lbm_kbc_equilibrium, the u^2 terms left out), which leaves no node at
// equilibrium (KBC's stabiliser is 0/0 there); C = 0 but for a Gaussian blob upstream of the body, g = equilibrium(u, C).
// The run: the collide-only first iteration directly, then the fused steps captured ONCE in a graph on a created stream,
// in blocks of an even number of steps (the time levels and the carries end where they began), replayed; a remainder runs
// directly.  --rectangle as passive_scalar_box: ceiling row r_top (negative: from the end) over columns c_first..c_second
// and the two side walls down to the last row; the scalar is absorbed (FIXED, C_w = 0) unless conc is given.
// --exchange 1: what the body takes in the stream of the final state (force_r, force_c, mass, uptake, uptake_fixed,
// wall_nodes).  --dump writes prefix-{f0,g0,f,g,rho,u,C}.f64 (raw f64, [R][C][Q]).  --time 1: ms_per_step of the replays.
// Output: one line of key=value pairs (steps, launches, nonfinite, ...), then the exchange values one per line.
// Exit status 4 if the final state holds a non-finite value, 3 with the library's message on a refusal.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../include/lbm/lbm.hpp"
#include "common.hpp"

int main(int argc, char** argv) {
  if (argc < 8) {
    std::cerr << "usage: " << argv[0] << " R C steps omega omega_g w_r w_c [--fluid bgk|kbc] [--s2 X] [--form 0|1|2] [--u-in X]"
                 " [--conc-w X] [--conc-rows N] [--rectangle r_top,c_first,c_second[,conc]]"
                 " [--buoyancy beta_r,beta_c,c_ref[,u_shift,guo_a,guo_b]] [--exchange 0|1] [--dump prefix] [--time 0|1]\n";
    return 1;
  }
  lbm_stream_t st = nullptr;
  lbm_graph* graph = nullptr;
  int status = 0;
  try {
    const int R = std::stoi(argv[1]), C = std::stoi(argv[2]), steps = std::stoi(argv[3]);
    const double omega = std::stod(argv[4]), omega_g = std::stod(argv[5]);
    const double w_r = std::stod(argv[6]), w_c = std::stod(argv[7]);
    const std::string fluid = arg_value(argc, argv, "--fluid", "bgk");
    if (fluid != "bgk" && fluid != "kbc") throw std::runtime_error("--fluid: '" + fluid + "' is not bgk or kbc");
    const bool kbc = fluid == "kbc";
    const double s2 = std::stod(arg_value(argc, argv, "--s2", argv[4]));
    const int form = std::stoi(arg_value(argc, argv, "--form", "0"));
    const double u_in = std::stod(arg_value(argc, argv, "--u-in", "0.03"));
    const double conc_w = std::stod(arg_value(argc, argv, "--conc-w", "1e-3"));
    const int conc_rows = std::stoi(arg_value(argc, argv, "--conc-rows", std::to_string(R / 2)));
    const bool exchange = std::stoi(arg_value(argc, argv, "--exchange", "0")) != 0;
    const bool timed = std::stoi(arg_value(argc, argv, "--time", "0")) != 0;
    const std::string dump = arg_value(argc, argv, "--dump", "");
    if (R < 1 || C < 1 || steps < 0) throw std::runtime_error("R, C must be positive and steps not negative");
    double bv[6];
    const bool buoyant = parse_buoyancy(arg_value(argc, argv, "--buoyancy", ""), bv);
    double rect[4] = {0.0, 0.0, 0.0, 0.0};
    int n_rect = 0;
    std::stringstream rectangle(arg_value(argc, argv, "--rectangle", ""));
    for (std::string item; std::getline(rectangle, item, ',');) {
      if (n_rect == 4) throw std::runtime_error("--rectangle: r_top,c_first,c_second[,conc]");
      rect[n_rect++] = std::stod(item);
    }
    if (n_rect != 0 && n_rect < 3) throw std::runtime_error("--rectangle: r_top,c_first,c_second[,conc]");
    if (lbm_device_count() < 1) {
      std::cerr << "no HIP device available\n";
      return 2;
    }
    const double U0 = 0.02, C0 = 1e-3, sigma = 0.1 * (R < C ? R : C), pi = std::acos(-1.0);
    std::vector<double> uh((size_t)R * C * 2), ch((size_t)R * C);
    for (int r = 0; r < R; ++r)
      for (int c = 0; c < C; ++c) {
        const size_t i = (size_t)r * C + c;
        uh[2 * i] = U0 * std::sin(2.0 * pi * c / C);
        uh[2 * i + 1] = u_in;
        const double dr = r - 0.5 * R, dc = c - 0.25 * C;
        ch[i] = C0 * std::exp(-(dr * dr + dc * dc) / (2.0 * sigma * sigma));
      }
    lbm::Field u(R, C, 2), rho(R, C, 1), conc(R, C, 1), f_adve(R, C, 9), g_adve(R, C, 9);
    u.from_host(uh);
    rho.fill(1.0);
    conc.from_host(ch);
    lbm::check(lbm_kbc_equilibrium(f_adve.data(), rho.data(), u.data(), R, C, 1, nullptr));
    solver::equilibrium(g_adve, u, conc);
    const std::vector<double> f0 = f_adve.to_host(), g0 = g_adve.to_host();

    lbm::check(lbm_stream_create(&st));
    lbm::BoundarySet bc;
    bc.row_hi = LBM_EDGE_BOUNCE_BACK;
    lbm::AdeOpenBoundary channel(R, C);
    channel.channel(u_in, conc_w, conc_rows);
    channel.finalize();
    lbm::AdeInteriorWalls body(R, C);
    lbm::AdeSolver sv = kbc ? lbm::AdeSolver::kbc(R, C, s2, omega_g, w_r, w_c, bc, form, st)
                            : lbm::AdeSolver(R, C, omega, omega_g, w_r, w_c, bc, form, st);
    if (buoyant) sv.set_buoyancy_m(lbm_ade_buoyancy{bv[0], bv[1], bv[2], bv[3], bv[4], bv[5]});
    if (n_rect) {  // as passive_scalar_box adds it: first wall, its foot's g slots, ceiling, second wall
      const int r_top = (int)rect[0] < 0 ? (int)rect[0] + R : (int)rect[0], c1 = (int)rect[1], c2 = (int)rect[2];
      const int n_side = R - 2 - r_top;  // rows r_top + 1 .. R - 2
      if (r_top < 0 || n_side < 1 || c2 <= c1) throw std::runtime_error("--rectangle: need 0 <= r_top < R - 2 and c_first < c_second");
      const int fx = LBM_ADE_SCALAR_FIXED;
      body.add(r_top + 1, c1, 1, 0, n_side, LBM_ADE_FACE_COL_NEG, LBM_ADE_FACE_COL_NEG, fx, rect[3]);
      body.add(-1, c1, 1, 0, 1, 0, LBM_ADE_FACE_COL_NEG & ~0x40u, fx, rect[3]);
      body.add(r_top, c1, 0, 1, c2 - c1 + 1, LBM_ADE_FACE_ROW_NEG, LBM_ADE_FACE_ROW_NEG, fx, rect[3]);
      body.add(r_top + 1, c2, 1, 0, n_side, LBM_ADE_FACE_COL_POS, LBM_ADE_FACE_COL_POS, fx, rect[3]);
      body.finalize();
      sv.set_walls(body);
    }
    sv.set_open_m(channel);
    sv.set_state(f0, g0);
    long long launches = 0;
    double ms_per_step = -1.0;
    int left = steps;
    if (left > 0) {  // the collide-only first iteration
      sv.step(1);
      --left;
    }
    const int block = left >= 2 ? (left < 200 ? left - left % 2 : 200) : 0;  // even: time levels and carries end where they began
    if (block > 0) {
      sv.sync();
      const long long before = sv.launches();
      lbm::check(lbm_graph_begin_capture(st));
      sv.step(block);
      lbm::check(lbm_graph_end_capture(st, &graph));
      const auto t0 = std::chrono::steady_clock::now();
      lbm::check(lbm_graph_launch(graph, left / block, st));
      sv.sync();
      const std::chrono::duration<double, std::milli> dt = std::chrono::steady_clock::now() - t0;
      ms_per_step = dt.count() / ((double)(left / block) * block);
      launches += (sv.launches() - before) * (left / block - 1);  // the replays after the captured one
      left %= block;
    }
    sv.step(left);
    sv.sync();
    launches += sv.launches();
    const lbm::AdeSolver::State s = sv.state();
    long long nonfinite = 0;
    for (const std::vector<double>* a : {&s.f, &s.g, &s.rho, &s.u, &s.C})
      for (double v : *a) nonfinite += !std::isfinite(v);
    double mass = 0.0;
    for (double v : s.C) mass += v;
    std::printf("steps=%d launches=%lld nonfinite=%lld fluid=%s open_nodes=%d wall_nodes=%d mass_C=%.17g", steps, launches,
                nonfinite, fluid.c_str(), channel.count(), body.count(), std::isfinite(mass) ? mass : -1.0);
    if (timed) std::printf(" ms_per_step=%.6g", ms_per_step);
    std::printf("\n");
    if (exchange) print_wall_exchange(sv.wall_exchange_m());
    std::fflush(stdout);
    if (!dump.empty()) {
      dump_f64(dump + "-f0.f64", f0);
      dump_f64(dump + "-g0.f64", g0);
      dump_f64(dump + "-f.f64", s.f);
      dump_f64(dump + "-g.f64", s.g);
      dump_f64(dump + "-rho.f64", s.rho);
      dump_f64(dump + "-u.f64", s.u);
      dump_f64(dump + "-C.f64", s.C);
    }
    if (nonfinite != 0) status = 4;
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << std::endl;
    status = 3;
  }
  if (graph) lbm_graph_destroy(graph);
  if (st) lbm_stream_destroy(st);
  return status;
}
