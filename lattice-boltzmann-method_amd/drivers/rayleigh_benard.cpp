// Rayleigh-Benard convection on lbm::AdeSolver: a fluid heated from below between two rigid plates, the temperature the
// transported scalar, buoyancy the coupling (lbm_ade_buoyancy) -- with the compressible BGK fluid or the entropic KBC
// collision (the forced KBC collision, lbm_ade_solver_set_buoyancy_m).
//   usage: rayleigh_benard [--fluid bgk|kbc] [--omega X | --s2 X] [--omega-g X] [--ra X | --beta X] [--rows R] [--cols C]
//          [--steps N] [--seed-mode A] [--dump prefix]
// Rows are the vertical: bounce-back rows (row 0 the hot plate, row R - 1 the cold one), periodic columns; the scalar is
// FIXED at 1 on row_lo and at 0 on row_hi; c_ref = 0.5; w = 0.  The force on a node is F = beta (C - 0.5) along +r, from
// --beta, or from --ra (default 5000) as beta = Ra nu kappa / R^3 with nu = (1 / rate - 1/2) / 3 of the fluid's rate
// (--omega for bgk, --s2 for kbc, default 1.4) and kappa = (1 / omega_g - 1/2) / 3 (--omega-g, default: the fluid's rate).
// --fluid bgk runs Guo's forcing, (u_shift, guo_a, guo_b) = (0.5, 3, 9); --fluid kbc the velocity shift u_shift = 1 (guo is
// not read).  With either the physical velocity is u0 + F / 2, u0 = calc_u(f, rho).
// Initial state (--dump writes it as prefix-f0.f64, prefix-g0.f64): rho = 1, u = 0, f = equilibrium(u, rho); the conduction
// profile plus one mode of amplitude A (--seed-mode, default 1e-3), C = 1 - (r + 1/2) / R + A sin(pi (r + 1/2) / R)
// cos(2 pi c / C), g = equilibrium(u, C).  Defaults: 24 x 48, 1000 steps.
// The run: the collide-only first iteration directly, then the fused steps captured ONCE in a graph on a created stream --
// blocks of an even number of steps (both time levels end where they began), replayed; what does not fill a block runs
// directly.  Output: one JSON line -- steps, launches (kernels enqueued, replays included), beta, nusselt = 1 + <C u_r> R /
// kappa from the scalar-flux sum of lbm_ade_solver_diag with the physical velocity (SUM_CUR + beta / 2 (SUM_C2 - c_ref
// SUM_C)), max_u (of u0), nonfinite.  --dump also writes prefix-{f,g,rho,u,C}.f64 (raw f64, reference layout).
// Exit status: 0; 1 usage; 2 no device; 3 an error of the library (its message on stderr); 4 a non-zero non-finite count.
#include <cmath>
#include <iostream>
#include <string>

#include "../include/lbm/lbm.hpp"
#include "common.hpp"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--help" || std::string(argv[i]) == "-h") {
      std::cerr << "usage: " << argv[0] << " [--fluid bgk|kbc] [--omega X | --s2 X] [--omega-g X] [--ra X | --beta X] [--rows R]"
                   " [--cols C] [--steps N] [--seed-mode A] [--dump prefix]\n";
      return 1;
    }
  lbm_stream_t st = nullptr;
  lbm_graph* graph = nullptr;
  int status = 0;
  try {
    const std::string fluid = arg_value(argc, argv, "--fluid", "bgk");
    if (fluid != "bgk" && fluid != "kbc") throw std::runtime_error("--fluid: '" + fluid + "' is not bgk or kbc");
    const bool kbc = fluid == "kbc";
    const double rate = std::stod(arg_value(argc, argv, kbc ? "--s2" : "--omega", "1.4"));
    const double omega_g = std::stod(arg_value(argc, argv, "--omega-g", std::to_string(rate)));
    const int R = std::stoi(arg_value(argc, argv, "--rows", "24")), C = std::stoi(arg_value(argc, argv, "--cols", "48"));
    const int steps = std::stoi(arg_value(argc, argv, "--steps", "1000"));
    const double seed = std::stod(arg_value(argc, argv, "--seed-mode", "1e-3"));
    const std::string dump = arg_value(argc, argv, "--dump", "");
    if (R < 1 || C < 1 || steps < 0) throw std::runtime_error("--rows, --cols must be positive and --steps not negative");
    const double nu = (1.0 / rate - 0.5) / 3.0, kappa = (1.0 / omega_g - 0.5) / 3.0;
    const std::string beta_arg = arg_value(argc, argv, "--beta", "");
    const double Ra = std::stod(arg_value(argc, argv, "--ra", "5000"));
    const double beta = beta_arg.empty() ? Ra * nu * kappa / ((double)R * R * R) : std::stod(beta_arg);
    const double c_ref = 0.5;
    if (lbm_device_count() < 1) {
      std::cerr << "no HIP device available\n";
      return 2;
    }
    const double pi = std::acos(-1.0);
    std::vector<double> ch((size_t)R * C);
    for (int r = 0; r < R; ++r)
      for (int c = 0; c < C; ++c)
        ch[(size_t)r * C + c] = 1.0 - (r + 0.5) / R + seed * std::sin(pi * (r + 0.5) / R) * std::cos(2.0 * pi * c / C);
    lbm::Field u(R, C, 2), rho(R, C, 1), conc(R, C, 1), f_adve(R, C, 9), g_adve(R, C, 9);
    u.fill(0.0);
    rho.fill(1.0);
    conc.from_host(ch);
    solver::equilibrium(f_adve, u, rho);
    solver::equilibrium(g_adve, u, conc);
    const std::vector<double> f0 = f_adve.to_host(), g0 = g_adve.to_host();

    lbm::check(lbm_stream_create(&st));
    lbm::BoundarySet bc;
    bc.row_lo = bc.row_hi = LBM_EDGE_BOUNCE_BACK;
    lbm::AdeSolver sv = kbc ? lbm::AdeSolver::kbc(R, C, rate, omega_g, 0.0, 0.0, bc, LBM_FORM_DEFAULT, st)
                            : lbm::AdeSolver(R, C, rate, omega_g, 0.0, 0.0, bc, LBM_FORM_DEFAULT, st);
    lbm_ade_scalar_bc sbc{};
    sbc.mode[0] = sbc.mode[1] = LBM_ADE_SCALAR_FIXED;
    sbc.conc[0] = 1.0;
    sbc.conc[1] = 0.0;
    sv.set_scalar_bc(sbc);
    const lbm_ade_buoyancy by = kbc ? lbm_ade_buoyancy{beta, 0.0, c_ref, 1.0, 1.0 / 3.0, 1.0 / 9.0}
                                    : lbm_ade_buoyancy{beta, 0.0, c_ref, 0.5, 3.0, 9.0};
    if (kbc) sv.set_buoyancy_m(by);
    else sv.set_buoyancy(by);
    sv.set_state(f0, g0);
    long long launches = 0;
    int left = steps;
    if (left > 0) {  // the collide-only first iteration
      sv.step(1);
      --left;
    }
    const int block = left >= 2 ? (left < 200 ? left - left % 2 : 200) : 0;  // even: the time levels end where they began
    if (block > 0) {
      sv.sync();
      const long long before = sv.launches();
      lbm::check(lbm_graph_begin_capture(st));
      sv.step(block);
      lbm::check(lbm_graph_end_capture(st, &graph));
      lbm::check(lbm_graph_launch(graph, left / block, st));
      launches += (sv.launches() - before) * (left / block - 1);  // the replays after the captured one
      left %= block;
    }
    sv.step(left);
    sv.sync();
    launches += sv.launches();
    const std::vector<double> d = sv.diag();
    const double flux = d[LBM_DIAG_SUM_CUR] + 0.5 * beta * (d[LBM_DIAG_SUM_C2] - c_ref * d[LBM_DIAG_SUM_C]);
    const double nusselt = 1.0 + flux / ((double)R * C) * R / kappa;
    const long long nonfinite = (long long)d[LBM_DIAG_NONFINITE];
    std::printf("{\"driver\": \"rayleigh_benard\", \"fluid\": \"%s\", \"rows\": %d, \"cols\": %d, \"steps\": %d, \"launches\": %lld, "
                "\"rate\": %.17g, \"omega_g\": %.17g, \"beta\": %.17g, \"u_shift\": %.17g, \"guo\": [%.17g, %.17g], "
                "\"nusselt\": %.17g, \"max_u\": %.17g, \"nonfinite\": %lld}\n",
                fluid.c_str(), R, C, steps, launches, rate, omega_g, beta, by.u_shift, by.guo_a, by.guo_b,
                std::isfinite(nusselt) ? nusselt : -1.0, std::isfinite(d[LBM_DIAG_MAX_U2]) ? std::sqrt(d[LBM_DIAG_MAX_U2]) : -1.0,
                nonfinite);
    std::fflush(stdout);
    if (!dump.empty()) {
      const lbm::AdeSolver::State s = sv.state();
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
