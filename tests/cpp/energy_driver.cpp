// TEST DRIVER — energies of psi_t, both ways on the same device trajectory:
//   device: OptimalControl::getPsitEnergies(control)  (ocg_observe_moments: seven
//           numbers per state leave the GPU)
//   host:   <K> = sum_i 2 Re correlationFunction("Adag", i, "A", i + 1) and
//           <D> = sum_i expectationValues("N(N-1)") / 2 over getPsit()
// and InitializeState's energy / variance out-parameters against its moments.
// Built by tests/test_energy_facade_gpu.py with g++ against
// liboptimalcontrolmps_amd.so.  Usage: energy_driver <state-dir>; prints one
// JSON object.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/GpuTDMRG.hpp"
#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/InitializeState.hpp"
#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/OptimalControl.hpp"
#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/correlations.hpp"

using namespace ocmps;

static MPS load_state(const std::string& dir, const std::string& key) {
  std::ifstream f(dir + "/" + key + ".bin", std::ios::binary);
  if (!f) throw std::runtime_error("missing state " + key);
  int h[5];
  f.read(reinterpret_cast<char*>(h), sizeof h);
  std::vector<int> dims(h[3]);
  f.read(reinterpret_cast<char*>(dims.data()), sizeof(int) * h[3]);
  std::vector<Cplx> data(h[4]);
  f.read(reinterpret_cast<char*>(data.data()), sizeof(double) * 2 * h[4]);
  return MPS(h[0], h[1], h[2], dims, data);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <state-dir>\n", argv[0]);
    return 2;
  }
  try {
    const int L = 5, d = 4, Nt = 21;
    const double J = 1.0;
    BoseHubbard sites(L, d);
    MPS psi_i = load_state(argv[1], "L5_p5_N5_J1_U2.5"), psi_f = load_state(argv[1], "L5_p5_N5_J1_U50");
    GpuTDMRG stepper(sites, J, 0.01, Args(1e-8, 80));
    OptimalControl<GpuTDMRG> OC(psi_f, psi_i, stepper, Nt, 0);
    stdvec control(Nt);
    for (int i = 0; i < Nt; ++i) control[i] = 2.5 + (50.0 - 2.5) * i / (Nt - 1);
    OC.getFidelityForAllT(control);

    const TrajectoryEnergies en = OC.getPsitEnergies(control);
    const std::vector<MPS> psi_t = OC.getPsit();
    if (en.moments.size() != psi_t.size() || en.energy.size() != psi_t.size() || en.variance.size() != psi_t.size())
      throw std::runtime_error("entry count");
    double dev_k1 = 0, dev_d1 = 0, dev_e = 0, dev_helper = 0, min_var = 1e300;
    for (size_t t = 0; t < psi_t.size(); ++t) {
      double k1 = 0, d1 = 0;
      for (int i = 1; i < L; ++i) k1 += 2.0 * correlationFunction(sites, psi_t[t], "Adag", i, "A", i + 1).real();
      for (const Cplx& v : expectationValues(sites, psi_t[t], "N(N-1)")) d1 += 0.5 * v.real();
      dev_k1 = std::max(dev_k1, std::fabs(en.moments.k1(t) - k1));
      dev_d1 = std::max(dev_d1, std::fabs(en.moments.d1(t) - d1));
      dev_e = std::max(dev_e, std::fabs(en.energy[t] - (-J * k1 + control[t] * d1) / en.moments.norm2(t)));
      dev_helper = std::max(dev_helper, std::fabs(energy(en.moments, t, J, control[t]) - en.energy[t]) +
                                            std::fabs(energyVariance(en.moments, t, J, control[t]) - en.variance[t]));
      min_var = std::min(min_var, en.variance[t]);
    }
    // a subset through the engine, repeated: the same bits
    const TrajectoryMoments sub = OC.getEngine().observeMoments(0, {20, 3, 3});
    bool subset_equal = sub.size() == 3;
    for (int e = 0; e < 3 && subset_equal; ++e)
      for (int j = 0; j < 7; ++j)
        if (sub.at(e)[j] != en.moments.at(e == 0 ? 20 : 3)[j]) subset_equal = false;

    // InitializeState with its certificate
    const double U = 2.5;
    double gs_e = 0, gs_var = 0, m[7];
    const MPS gs = InitializeState(sites, 5, J, U, 80, 1e-9, true, 0, &gs_e, &gs_var, m);
    const double e_m = (-J * m[1] + U * m[2]) / m[0];
    const double var_m = (J * J * m[3] - 2 * J * U * m[5] + U * U * m[4]) / m[0] - e_m * e_m;
    const MPS plain = InitializeState(sites, 5, J, U, 80, 1e-9);
    const bool same_state = plain.dims == gs.dims && plain.data == gs.data;

    std::ostringstream o;
    o.precision(17);
    o << "{\"entries\": " << psi_t.size() << ", \"dev_k1\": " << dev_k1 << ", \"dev_d1\": " << dev_d1
      << ", \"dev_e\": " << dev_e << ", \"dev_helper\": " << dev_helper << ", \"min_var\": " << min_var
      << ", \"e_first\": " << en.energy.front() << ", \"var_first\": " << en.variance.front()
      << ", \"e_last\": " << en.energy.back() << ", \"var_last\": " << en.variance.back()
      << ", \"subset_equal\": " << (subset_equal ? "true" : "false") << ", \"gs_e\": " << gs_e
      << ", \"gs_var\": " << gs_var << ", \"gs_e_from_moments\": " << e_m << ", \"gs_var_from_moments\": " << var_m
      << ", \"gs_norm2\": " << m[0] << ", \"gs_same_state\": " << (same_state ? "true" : "false") << "}";
    std::printf("%s\n", o.str().c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
