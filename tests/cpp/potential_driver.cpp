// TEST DRIVER — the static site potential through the C++ facade (L = p = Q = 5, N_t = 9,
// gamma = 0): GpuTDMRG::setPotential + OptimalControl::getHessian on two shards, getPsitEnergies
// refusing a trapped chain and working again without the potential, one trapped single step, and
// the InitializeState overload that takes site energies.
// Built by tests/test_potential_facade_gpu.py with g++ against liboptimalcontrolmps_amd.so.
// Usage: potential_driver <state-dir> <U> <eps_1> ... <eps_L> (init.bin, target.bin, controls.txt);
// prints one JSON object.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/GpuTDMRG.hpp"
#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/InitializeState.hpp"
#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/OptimalControl.hpp"

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

template <class T>
static std::string list(const std::vector<T>& v) {
  std::ostringstream o;
  o.precision(17);
  o << "[";
  for (size_t i = 0; i < v.size(); ++i) o << (i ? ", " : "") << v[i];
  o << "]";
  return o.str();
}

static std::string state_json(const MPS& m) {
  stdvec raw(m.raw(), m.raw() + 2 * m.data.size());
  return "{\"dims\": " + list(m.dims) + ", \"data\": " + list(raw) + "}";
}

int main(int argc, char** argv) {
  const int L = 5, d = 4, Q = 5;
  if (argc != 3 + L) {
    std::fprintf(stderr, "usage: %s <state-dir> <U> <eps_1> ... <eps_%d>\n", argv[0], L);
    return 2;
  }
  try {
    const double J = 1.0, dt = 0.01, U = std::atof(argv[2]);
    std::vector<double> eps;
    for (int k = 0; k < L; ++k) eps.push_back(std::strtod(argv[3 + k], nullptr));
    stdvec u;
    {
      std::ifstream f(std::string(argv[1]) + "/controls.txt");
      double x;
      while (f >> x) u.push_back(x);
    }
    const size_t Nt = u.size();
    BoseHubbard sites(L, d);
    MPS psi_i = load_state(argv[1], "init"), psi_f = load_state(argv[1], "target");
    GpuTDMRG stepper(sites, J, dt, Args(1e-14, 512));
    const bool zero_before = stepper.getPotential() == std::vector<double>(L, 0.0) && !stepper.hasPotential();
    stepper.setPotential(eps);
    const bool roundtrip = stepper.getPotential() == eps && stepper.hasPotential();

    // getHessian on two shards: every context makeEngine creates carries the potential
    OptimalControl<GpuTDMRG> OC(psi_f, psi_i, stepper, Nt, 0);
    OC.setThreadCount(2);
    const rowmat H = OC.getHessian(u);
    std::string threw;
    try {
      OC.getPsitEnergies(u);
    } catch (const std::invalid_argument& e) {
      threw = e.what();
    }
    MPS one = psi_i;
    stepper.step(one, 3.0, 7.0, true);

    // without the potential the energies are back
    stepper.setPotential({});
    OptimalControl<GpuTDMRG> OC0(psi_f, psi_i, stepper, Nt, 0);
    OC0.getCost(u);
    const TrajectoryEnergies en = OC0.getPsitEnergies(u);
    MPS one0 = psi_i;
    stepper.step(one0, 3.0, 7.0, true);

    // InitializeState in the trap; its energy out-parameter refuses
    const MPS gs = InitializeState(sites, Q, J, U, eps);
    std::string gs_threw;
    try {
      double e = 0;
      InitializeState(sites, Q, J, U, eps, 200, 1e-9, true, 0, &e);
    } catch (const std::invalid_argument& e) {
      gs_threw = e.what();
    }

    std::ostringstream o;
    o.precision(17);
    o << "{\"zero_before\": " << (zero_before ? "true" : "false") << ", \"roundtrip\": " << (roundtrip ? "true" : "false")
      << ", \"threw\": \"" << threw << "\", \"gs_threw\": \"" << gs_threw << "\", \"n_energy\": " << en.energy.size()
      << ", \"energy0\": " << en.energy[0] << ", \"H\": [";
    for (size_t i = 0; i < H.size(); ++i) o << (i ? ", " : "") << list(H[i]);
    o << "], \"step\": " << state_json(one) << ", \"step0\": " << state_json(one0) << ", \"gs\": " << state_json(gs)
      << "}";
    std::printf("%s\n", o.str().c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
