// TEST DRIVER — the CalculateDefects / AnalyzeQuench observable loops of the
// reference's drivers, run both ways on the same device trajectory:
//   device: OptimalControl::getPsitObservables + the TrajectoryObservables
//           overloads of correlations.hpp (nothing but the results leaves the GPU)
//   host:   expectationValues / correlationMatrix / correlationTerm over getPsit()
// Built by tests/test_observe_facade_gpu.py with g++ against
// liboptimalcontrolmps_amd.so.  Usage: observe_driver <state-dir>; prints one
// JSON object with the largest deviation per quantity and the defect measures.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../optimalcontrolmps_amd/include/optimalcontrolmps/GpuTDMRG.hpp"
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
    BoseHubbard sites(L, d);
    MPS psi_i = load_state(argv[1], "L5_p5_N5_J1_U2.5"), psi_f = load_state(argv[1], "L5_p5_N5_J1_U50");
    GpuTDMRG stepper(sites, 1.0, 0.01, Args(1e-8, 80));
    OptimalControl<GpuTDMRG> OC(psi_f, psi_i, stepper, Nt, 0);
    stdvec control(Nt);
    for (int i = 0; i < Nt; ++i) control[i] = 2.5 + (50.0 - 2.5) * i / (Nt - 1);
    const stdvec fids = OC.getFidelityForAllT(control);

    std::vector<int> rows;
    for (int i = 1; i <= L; ++i) rows.push_back(i);
    const TrajectoryObservables obs = OC.getPsitObservables({}, rows);
    const std::vector<MPS> psi_t = OC.getPsit();
    if (obs.size() != psi_t.size()) throw std::runtime_error("entry count");

    const char* ops[] = {"N", "NN", "N(N-1)", "Id", "A", "Adag"};
    double dev_exp[6] = {0, 0, 0, 0, 0, 0}, dev_ada = 0, dev_nn = 0, dev_term = 0, dev_rho = 0, dev_F2 = 0;
    bool bonds_equal = true, mirrored = true;
    // CalculateDefects: rho(t) = mean |<N_i> - 1|, F2(t) = mean var(N_i)(t) / var(N_i)(0)
    std::vector<double> F2_i_dev, F2_i_host;
    {
      const auto n = expectationValues(obs, 0, "N"), nn = expectationValues(obs, 0, "NN");
      const auto hn = expectationValues(sites, psi_i, "N"), hnn = expectationValues(sites, psi_i, "NN");
      for (int i = 0; i < L; ++i) {
        F2_i_dev.push_back(nn[i].real() - n[i].real() * n[i].real());
        F2_i_host.push_back(hnn[i].real() - hn[i].real() * hn[i].real());
      }
    }
    std::vector<double> rho_t, F2_t;
    for (size_t t = 0; t < psi_t.size(); ++t) {
      for (int o = 0; o < 6; ++o) {
        const auto a = expectationValues(obs, t, ops[o]);
        const auto b = expectationValues(sites, psi_t[t], ops[o]);
        for (int i = 0; i < L; ++i) dev_exp[o] = std::max(dev_exp[o], std::abs(a[i] - b[i]));
      }
      const auto n = expectationValues(obs, t, "N"), nn = expectationValues(obs, t, "NN");
      const auto hn = expectationValues(sites, psi_t[t], "N"), hnn = expectationValues(sites, psi_t[t], "NN");
      double rv = 0, fv = 0, hrv = 0, hfv = 0;
      for (int i = 0; i < L; ++i) {
        rv += std::fabs(n[i].real() - 1.0);
        fv += (nn[i].real() - n[i].real() * n[i].real()) / F2_i_dev[i];
        hrv += std::fabs(hn[i].real() - 1.0);
        hfv += (hnn[i].real() - hn[i].real() * hn[i].real()) / F2_i_host[i];
      }
      rho_t.push_back(rv / L);
      F2_t.push_back(fv / L);
      dev_rho = std::max(dev_rho, std::fabs(rv - hrv) / L);
      dev_F2 = std::max(dev_F2, std::fabs(fv - hfv) / L);
      const auto ra = correlationMatrix(obs, t, "Adag", "A"), rn = correlationMatrix(obs, t, "N", "N");
      const auto ha = correlationMatrix(sites, psi_t[t], "Adag", "A"), hnm = correlationMatrix(sites, psi_t[t], "N", "N");
      for (int i = 0; i < L; ++i)
        for (int j = 0; j < L; ++j) {
          dev_ada = std::max(dev_ada, std::abs(ra[i][j] - ha[i][j]));
          dev_nn = std::max(dev_nn, std::abs(rn[i][j] - hnm[i][j]));
          if (ra[i][j] != std::conj(ra[j][i]) || (i == j && ra[i][j].imag() != 0.0)) mirrored = false;
        }
      dev_term = std::max(dev_term, std::fabs(correlationTerm(obs, t) - correlationTerm(sites, psi_t[t], "Adag", "A")));
      for (int b = 0; b <= L; ++b)
        if (obs.bondDim(t, b) != psi_t[t].bondDim(b)) bonds_equal = false;
    }
    // a subset of times and rows gives the same numbers
    const TrajectoryObservables sub = OC.getPsitObservables({20, 3}, {2});
    bool subset_equal = sub.size() == 2 && sub.norm2[0] == obs.norm2[20] && sub.norm2[1] == obs.norm2[3];
    for (int j = 0; j < L; ++j)
      if (sub.ada[size_t(1) * L + j] != obs.ada[(size_t(3) * L + 1) * L + j]) subset_equal = false;

    std::ostringstream o;
    o.precision(17);
    o << "{";
    for (int k = 0; k < 6; ++k) o << "\"dev_exp_" << ops[k] << "\": " << dev_exp[k] << ", ";
    o << "\"dev_ada\": " << dev_ada << ", \"dev_nn\": " << dev_nn << ", \"dev_term\": " << dev_term
      << ", \"dev_rho\": " << dev_rho << ", \"dev_F2\": " << dev_F2 << ", \"bonds_equal\": " << (bonds_equal ? "true" : "false")
      << ", \"mirrored\": " << (mirrored ? "true" : "false") << ", \"subset_equal\": " << (subset_equal ? "true" : "false")
      << ", \"fid_last\": " << fids.back() << ", \"term_last\": " << correlationTerm(obs, psi_t.size() - 1) << ", \"rho\": [";
    for (size_t t = 0; t < rho_t.size(); ++t) o << (t ? ", " : "") << rho_t[t];
    o << "], \"F2\": [";
    for (size_t t = 0; t < F2_t.size(); ++t) o << (t ? ", " : "") << F2_t[t];
    o << "]}";
    std::printf("%s\n", o.str().c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
