// A passive scalar carried by a shear wave on a periodic box: the fluid + transported-scalar loop of
// test/rectangle_sedimentation_test.cpp:88-247 (its interior: equilibrium(g_equi, u + w, C), own BGK rate,
// streamed like f) on lbm::AdeSolver.  Initial state: rho = 1, u = (0, U0 sin(2 pi r / R)) -- a shear wave --
// f = equilibrium(u, rho); a Gaussian blob C = C0 exp(-|x - x_c|^2 / (2 sigma^2)) at the centre, g = equilibrium(u, C)
// (as the driver initialises g_adve, :95).
//   usage: passive_scalar_box R C steps omega omega_g w_r w_c [--dump prefix] [--form 0|1|2] [--walls 0|1|2]
//          [--fixed edge=C_w[,edge=C_w...]] [--buoyancy beta_r,beta_c,c_ref[,u_shift,guo_a,guo_b]]
//          [--rectangle r_top,c_first,c_second[,conc]] [--exchange 0|1] [--fluid bgk|kbc] [--s2 X]
// --dump writes prefix-{f0,g0,f,g,rho,u,C}.f64 (raw f64, reference layout [R][C][Q]); --walls 1: bounce-back columns,
// 2: bounce-back rows and columns.  --fixed: the named edges (row_lo, row_hi, col_lo, col_hi; walls of the fluid) hold
// the scalar at the constant C_w (lbm_ade_scalar_bc FIXED), the others stay no-flux.  --buoyancy: the scalar pushes on the
// fluid with F = beta (C - c_ref) per node (lbm_ade_buoyancy; u_shift, guo_a, guo_b default to 1, 1/3, 1/9); without it
// the scalar is passive.  --rectangle: the sedimentation driver's rectangle (rectangle_sedimentation_test.cpp:184-196,
// :220-232) standing on the last row as interior walls (lbm::AdeInteriorWalls): ceiling row r_top (negative: from the
// end) over columns c_first..c_second, the two side walls below it down to the last row; the scalar is absorbed
// (FIXED, C_w = 0) unless conc gives the C_w the body holds.  --exchange 1: what the body takes from the lattices in the
// stream of the final state (lbm::AdeSolver::wall_exchange) as force_r, force_c, mass, uptake, uptake_fixed, wall_nodes.
// --fluid kbc: the entropic KBC collision as the fluid (lbm::AdeSolver::kbc) with the rate --s2 (default: omega); omega is
// then not used.  KBC's stabiliser is 0/0 on a lattice exactly at equilibrium, in the reference too, so this fluid starts
// as the reference's KBC driver starts (ulbm_double_shear_flow.cpp:96, eval_equilibrium with the u^2 terms left out) and
// drifts with u_r = U0 / 2, which leaves no node at rest.  --buoyancy and --exchange fail with the library's message.
#include <cmath>
#include <iostream>
#include <sstream>
#include <string>

#include "../include/lbm/lbm.hpp"
#include "common.hpp"

int main(int argc, char** argv) {
  if (argc < 8) {
    std::cerr << "usage: " << argv[0] << " R C steps omega omega_g w_r w_c [--dump prefix] [--form 0|1|2] [--walls 0|1|2]"
                 " [--fixed edge=C_w[,edge=C_w...]] [--buoyancy beta_r,beta_c,c_ref[,u_shift,guo_a,guo_b]]"
                 " [--rectangle r_top,c_first,c_second[,conc]] [--exchange 0|1] [--fluid bgk|kbc] [--s2 X]\n";
    return 1;
  }
  try {
    const int R = std::stoi(argv[1]), C = std::stoi(argv[2]), steps = std::stoi(argv[3]);
    const double omega = std::stod(argv[4]), omega_g = std::stod(argv[5]);
    const double w_r = std::stod(argv[6]), w_c = std::stod(argv[7]);
    const std::string dump = arg_value(argc, argv, "--dump", "");
    const int form = std::stoi(arg_value(argc, argv, "--form", "0"));
    const int walls = std::stoi(arg_value(argc, argv, "--walls", "0"));
    const bool exchange = std::stoi(arg_value(argc, argv, "--exchange", "0")) != 0;
    const std::string fluid = arg_value(argc, argv, "--fluid", "bgk");
    if (fluid != "bgk" && fluid != "kbc") throw std::runtime_error("--fluid: '" + fluid + "' is not bgk or kbc");
    const bool kbc = fluid == "kbc";
    const double s2 = std::stod(arg_value(argc, argv, "--s2", argv[4]));
    lbm_ade_scalar_bc sbc{};
    std::stringstream fixed(arg_value(argc, argv, "--fixed", ""));
    for (std::string item; std::getline(fixed, item, ',');) {
      static const char* const names[4] = {"row_lo", "row_hi", "col_lo", "col_hi"};
      const size_t eq = item.find('=');
      int e = 0;
      while (e < 4 && item.substr(0, eq) != names[e]) ++e;
      if (eq == std::string::npos || e == 4) throw std::runtime_error("--fixed: '" + item + "' is not edge=C_w");
      sbc.mode[e] = LBM_ADE_SCALAR_FIXED;
      sbc.conc[e] = std::stod(item.substr(eq + 1));
    }
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
        uh[2 * i] = kbc ? 0.5 * U0 : 0.0;
        uh[2 * i + 1] = U0 * std::sin(2.0 * pi * r / R);
        const double dr = r - 0.5 * R, dc = c - 0.5 * C;
        ch[i] = C0 * std::exp(-(dr * dr + dc * dc) / (2.0 * sigma * sigma));
      }
    lbm::Field u(R, C, 2), rho(R, C, 1), conc(R, C, 1), f_adve(R, C, 9), g_adve(R, C, 9);
    u.from_host(uh);
    rho.fill(1.0);
    conc.from_host(ch);
    if (kbc) lbm::check(lbm_kbc_equilibrium(f_adve.data(), rho.data(), u.data(), R, C, 1, nullptr));
    else solver::equilibrium(f_adve, u, rho);
    solver::equilibrium(g_adve, u, conc);
    const std::vector<double> f0 = f_adve.to_host(), g0 = g_adve.to_host();

    lbm::BoundarySet bc;
    if (walls) bc.col_lo = bc.col_hi = LBM_EDGE_BOUNCE_BACK;
    if (walls == 2) bc.row_lo = bc.row_hi = LBM_EDGE_BOUNCE_BACK;
    lbm::AdeSolver sv = kbc ? lbm::AdeSolver::kbc(R, C, s2, omega_g, w_r, w_c, bc, form)
                            : lbm::AdeSolver(R, C, omega, omega_g, w_r, w_c, bc, form);
    sv.set_scalar_bc(sbc);
    if (buoyant) sv.set_buoyancy(lbm_ade_buoyancy{bv[0], bv[1], bv[2], bv[3], bv[4], bv[5]});
    // the rectangle as the driver adds it: first wall (f stops one row short of the last row, g runs through it with
    // slot 7 of the foot left to the domain's wall), ceiling, second wall
    lbm::AdeInteriorWalls body(R, C);
    if (n_rect) {
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
    sv.set_state(f0, g0);
    sv.step(steps);
    const lbm::AdeSolver::State s = sv.state();
    double mass0 = 0.0, mass = 0.0;
    for (size_t i = 0; i < ch.size(); ++i) {
      double m0 = 0.0;
      for (int q = 0; q < 9; ++q) m0 += g0[9 * i + q];
      mass0 += m0;
      mass += s.C[i];
    }
    std::cout.precision(17);
    std::cout << "steps=" << steps << "\nlaunches=" << sv.launches() << "\nmass_C0=" << mass0 << "\nmass_C=" << mass
              << std::endl;
    if (exchange) print_wall_exchange(sv.wall_exchange());
    if (!dump.empty()) {
      dump_f64(dump + "-f0.f64", f0);
      dump_f64(dump + "-g0.f64", g0);
      dump_f64(dump + "-f.f64", s.f);
      dump_f64(dump + "-g.f64", s.g);
      dump_f64(dump + "-rho.f64", s.rho);
      dump_f64(dump + "-u.f64", s.u);
      dump_f64(dump + "-C.f64", s.C);
    }
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << std::endl;
    return 3;
  }
  return 0;
}
