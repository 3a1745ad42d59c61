// shared by the drivers: raw snapshot writer (the reference uses torch::save, utils.cpp:21-29)
#pragma once
#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

inline void dump_f64(const std::string& path, const std::vector<double>& a) {
  if (path.empty()) return;
  if (FILE* f = std::fopen(path.c_str(), "wb")) {
    std::fwrite(a.data(), sizeof(double), a.size(), f);
    std::fclose(f);
  }
}
// --buoyancy beta_r,beta_c,c_ref[,u_shift,guo_a,guo_b]: the six fields of lbm_ade_buoyancy in order, the last three
// defaulting to the reference's (1, 1/3, 1/9).  False for an empty string (no buoyancy); throws on anything else malformed.
inline bool parse_buoyancy(const std::string& s, double (&v)[6]) {
  if (s.empty()) return false;
  v[3] = 1.0, v[4] = 1.0 / 3.0, v[5] = 1.0 / 9.0;
  size_t pos = 0;
  int n = 0;
  while (pos <= s.size()) {
    const size_t end = std::min(s.find(',', pos), s.size());
    if (n == 6) throw std::runtime_error("--buoyancy: more than six values in '" + s + "'");
    const std::string item = s.substr(pos, end - pos);
    size_t used = 0;
    try {
      v[n++] = std::stod(item, &used);
    } catch (const std::exception&) {
      used = std::string::npos;
    }
    if (used != item.size()) throw std::runtime_error("--buoyancy: '" + item + "' is not a number (in '" + s + "')");
    pos = end + 1;
  }
  if (n != 3 && n != 6) throw std::runtime_error("--buoyancy: beta_r,beta_c,c_ref[,u_shift,guo_a,guo_b] ('" + s + "')");
  return true;
}
// the six values of a wall exchange (LBM_WALLX_* order) as key=value lines, 17 significant digits
inline void print_wall_exchange(const std::vector<double>& x) {
  static const char* const keys[6] = {"force_r", "force_c", "mass", "uptake", "uptake_fixed", "wall_nodes"};
  for (size_t q = 0; q < 6 && q < x.size(); ++q) std::printf("%s=%.17g\n", keys[q], x[q]);
  std::fflush(stdout);
}
inline std::string arg_value(int argc, char** argv, const std::string& key, const std::string& dflt) {
  for (int i = 1; i + 1 < argc; ++i)
    if (key == argv[i]) return argv[i + 1];
  return dflt;
}
