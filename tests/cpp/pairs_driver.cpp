// TEST DRIVER — OptimalControl::getControlSensitivities on a short ramp (L = p = Q = 5,
// N_t = 21, gamma = 0): dU against getAnalyticGradient, the particle-number sum rule of
// dEps, the reuse of the trajectories with new_control = false, and a GROUP instance.
// Built by tests/test_pair_facade_gpu.py with g++ against liboptimalcontrolmps_amd.so.
// Usage: pairs_driver <state-dir> (init.bin, target.bin); prints one JSON object.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/ControlBasisFactory.hpp"
#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/GpuTDMRG.hpp"
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

static std::string list(const stdvec& v) {
  std::ostringstream o;
  o.precision(17);
  o << "[";
  for (size_t i = 0; i < v.size(); ++i) o << (i ? ", " : "") << v[i];
  o << "]";
  return o.str();
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <state-dir>\n", argv[0]);
    return 2;
  }
  try {
    const int L = 5, d = 4, Nt = 21, Q = 5;
    const double J = 1.0, dt = 0.01;
    BoseHubbard sites(L, d);
    MPS psi_i = load_state(argv[1], "init"), psi_f = load_state(argv[1], "target");
    GpuTDMRG stepper(sites, J, dt, Args(1e-8, 80));
    OptimalControl<GpuTDMRG> OC(psi_f, psi_i, stepper, Nt, 0);
    stdvec u(Nt);
    for (int i = 0; i < Nt; ++i) u[i] = 2.5 + 3.5 * i / (Nt - 1) + 0.7 * std::sin(5.0 * i / (Nt - 1));

    const ControlSensitivities s = OC.getControlSensitivities(u);
    const stdvec g = OC.getAnalyticGradient(u, false);
    const long prop0 = OC.getEngine().kernelLaunches(0);
    const ControlSensitivities again = OC.getControlSensitivities(u, false);
    const long prop1 = OC.getEngine().kernelLaunches(0);
    const bool reused_equal = again.dU == s.dU && again.dJ == s.dJ && again.dEps == s.dEps && again.overlap == s.overlap;
    // a fresh instance: gradient first, then the sensitivities of the stored trajectories
    OptimalControl<GpuTDMRG> OC2(psi_f, psi_i, stepper, Nt, 0);
    const stdvec g2 = OC2.getAnalyticGradient(u);
    const long prop2 = OC2.getEngine().kernelLaunches(0);
    const ControlSensitivities s2 = OC2.getControlSensitivities(u, false);
    const long prop3 = OC2.getEngine().kernelLaunches(0);

    const Cplx F = OC.getEngine().overlapFactor();
    double dev_grad = 0, dev_grad2 = 0, dev_sum = 0;
    for (int t = 0; t < Nt; ++t) {
      dev_grad = std::max(dev_grad, std::fabs(s.dU[t] - g[t]));
      dev_grad2 = std::max(dev_grad2, std::fabs(s2.dU[t] - g2[t]));
      double sum = 0;
      for (double e : s.dEps[t]) sum += e;
      dev_sum = std::max(dev_sum, std::fabs(sum - Q * dt * (Cplx(0, 1) * s.overlap[t] * F).real()));
    }
    double divmax = 0;
    for (int t = 0; t < Nt; ++t) divmax = std::max(divmax, std::fabs(g[t]) / dt);  // >= |Re(i divT F)|

    // GROUP: coefficients in, vectors on the time grid out
    const int M = 5;
    ControlBasis basis = ControlBasisFactory::buildChoppedSineBasis(u, dt, dt * (Nt - 1), M);
    OptimalControl<GpuTDMRG> G(psi_f, psi_i, stepper, basis, 0);
    stdvec c(M, 0.0);
    c[1] = 0.3;
    const ControlSensitivities sg = G.getControlSensitivities(c);
    const stdvec gg = G.getAnalyticGradient(c, false);

    std::ostringstream o;
    o.precision(17);
    o << "{\"n\": " << s.dU.size() << ", \"n_eps\": " << s.dEps.size() << ", \"sites\": " << s.dEps[0].size()
      << ", \"dev_grad\": " << dev_grad << ", \"dev_grad2\": " << dev_grad2 << ", \"dev_sum\": " << dev_sum
      << ", \"absF\": " << std::abs(F) << ", \"grad_max_over_dt\": " << divmax
      << ", \"reused_equal\": " << (reused_equal ? "true" : "false") << ", \"prop\": [" << prop0 << ", " << prop1 << ", "
      << prop2 << ", " << prop3 << "], \"group_n\": " << sg.dU.size() << ", \"group_n_J\": " << sg.dJ.size()
      << ", \"group_n_eps\": " << sg.dEps.size() << ", \"group_n_ovl\": " << sg.overlap.size()
      << ", \"group_grad_n\": " << gg.size() << ", \"dU\": " << list(s.dU) << ", \"dJ\": " << list(s.dJ) << "}";
    std::printf("%s\n", o.str().c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
