// TEST DRIVER — AnalyzeQuench's entanglement-entropy loop, run both ways on
// the same device trajectory:
//   device: entanglementEntropy(OptimalControl::getPsitObservables(ts, rows, true), e)
//           (ocg_observe_spectrum: nothing but the entropies leaves the GPU)
//   host:   entanglementEntropy(sites, psi_t[e]) over getPsit()
// Built by tests/test_spectrum_facade_gpu.py with g++ against
// liboptimalcontrolmps_amd.so.  Usage: spectrum_driver <state-dir>; prints one
// JSON object.
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

    const TrajectoryObservables obs = OC.getPsitObservables({}, {1}, true);
    const std::vector<MPS> psi_t = OC.getPsit();
    if (obs.size() != psi_t.size()) throw std::runtime_error("entry count");
    double dev = 0, smax = 0;
    std::vector<double> mid;
    for (size_t t = 0; t < psi_t.size(); ++t) {
      const std::vector<double> a = entanglementEntropy(obs, t), b = entanglementEntropy(sites, psi_t[t]);
      if (a.size() != size_t(L - 1) || b.size() != a.size()) throw std::runtime_error("bond count");
      for (int k = 0; k < L - 1; ++k) {
        dev = std::max(dev, std::fabs(a[k] - b[k]));
        smax = std::max(smax, a[k]);
      }
      mid.push_back(a[L / 2 - 1]);
    }
    // without the third argument nothing changes and the entropies are absent
    const TrajectoryObservables plain = OC.getPsitObservables({}, {1});
    bool threw = false, same = plain.norm2 == obs.norm2 && plain.occ == obs.occ && plain.ada == obs.ada &&
                               plain.nn == obs.nn && plain.bond == obs.bond && plain.entropy.empty();
    try {
      (void)entanglementEntropy(plain, 0);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    // a subset of times with the weights: the same entropies, weights that sum to the norm
    const TrajectoryObservables sub = OC.getEngine().observeSpectrum(0, {20, 3}, true);
    bool subset_equal = sub.size() == 2 && sub.hasEntropy() && sub.wcap > 0;
    double dev_sum = 0;
    for (int e = 0; e < 2 && subset_equal; ++e)
      for (int b = 1; b < L; ++b) {
        if (sub.entropyAt(e, b) != obs.entropyAt(e == 0 ? 20 : 3, b)) subset_equal = false;
        double s = 0;
        int cnt = 0;
        for (int j = 0; j < sub.wcap; ++j) {
          s += sub.schmidtAt(e, b, j);
          cnt += sub.sectorAt(e, b, j) >= 0;
        }
        if (cnt != sub.bondDim(e, b)) subset_equal = false;
        dev_sum = std::max(dev_sum, std::fabs(s - obs.norm2[e == 0 ? 20 : 3]));
      }

    std::ostringstream o;
    o.precision(17);
    o << "{\"dev_entropy\": " << dev << ", \"dev_sum\": " << dev_sum << ", \"entropy_max\": " << smax
      << ", \"threw\": " << (threw ? "true" : "false") << ", \"plain_same\": " << (same ? "true" : "false")
      << ", \"subset_equal\": " << (subset_equal ? "true" : "false") << ", \"fid_last\": " << fids.back()
      << ", \"mid\": [";
    for (size_t t = 0; t < mid.size(); ++t) o << (t ? ", " : "") << mid[t];
    o << "]}";
    std::printf("%s\n", o.str().c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
