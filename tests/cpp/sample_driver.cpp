// TEST DRIVER — quantum-gas-microscope snapshots of psi_t, drawn both ways on the
// same device trajectory:
//   device: OptimalControl::samplePsit(ts, nshots, seed)  (ocg_sample: nothing but
//           the shots leaves the GPU)
//   host:   sampleFock(psi_t[e], nshots, seed, e) over getPsit()
// and the Mott-state probability along the ramp, getPsitFockProbability, against
// |<1..1|psi_t>|^2 / <psi_t|psi_t> contracted on the host from getPsit().
// Built by tests/test_sample_facade_gpu.py with g++ against
// liboptimalcontrolmps_amd.so.  Usage: sample_driver <state-dir>; prints one
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

// <n|psi> by the chain of site matrices of the dense tensors
static Cplx host_amplitude(const MPS& psi, const std::vector<int>& n) {
  const obs::Dense D = obs::dense(psi);
  obs::cmat v(1, Cplx(1, 0));
  for (int k = 1; k <= psi.L; ++k) {
    obs::cmat w(D.chi[k], Cplx(0, 0));
    for (int a = 0; a < D.chi[k - 1]; ++a)
      for (int c = 0; c < D.chi[k]; ++c) w[c] += v[a] * D.A[k][(size_t(a) * psi.p + n[k - 1]) * D.chi[k] + c];
    v = w;
  }
  return v[0];
}

// every completion of the first k - 1 sites of cf to Q particles, entries below p
static void completions(std::vector<signed char>& cur, int k, int L, int p, int left, std::vector<signed char>& out) {
  if (k == L) {
    if (left == 0) out.insert(out.end(), cur.begin(), cur.end());
    return;
  }
  for (int n = 0; n < p && n <= left; ++n) {
    cur[k] = (signed char)n;
    completions(cur, k + 1, L, p, left - n, out);
  }
}

// The distance of the u of decision (t, shot, site k) to the nearest normalised CDF
// boundary, the CDF taken from the device amplitudes of all completions of the prefix.
template <class Engine>
static double boundary_distance(Engine& eng, int t, const TrajectorySnapshots& s, size_t e, int shot, int k, int p,
                                int Q, unsigned long long seed) {
  const int L = s.L;
  std::vector<signed char> cur(L, 0), all;
  int used = 0;
  for (int j = 1; j < k; ++j) {
    cur[j - 1] = (signed char)s.config(e, shot, j);
    used += s.config(e, shot, j);
  }
  completions(cur, k - 1, L, p, Q - used, all);
  const std::vector<Cplx> amp = eng.fockAmplitudes(0, {t}, all);
  std::vector<double> c(p, 0.0);
  for (size_t j = 0; j < amp.size(); ++j) c[all[j * L + (k - 1)]] += std::norm(amp[j]);
  for (int n = 1; n < p; ++n) c[n] += c[n - 1];
  const unsigned long long h = obs::sampleMix(
      obs::sampleMix(obs::sampleMix(obs::sampleMix(seed) ^ (unsigned long long)t) ^ (unsigned long long)shot) ^
      (unsigned long long)k);
  const double u = double(h >> 11) * 0x1.0p-53;
  double d = 1.0;
  for (int n = 0; n + 1 < p; ++n) d = std::min(d, std::fabs(u - c[n] / c[p - 1]));
  return d;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <state-dir>\n", argv[0]);
    return 2;
  }
  try {
    const int L = 5, d = 4, Nt = 21, nshots = 256;
    const unsigned long long seed = 20261015ull;
    BoseHubbard sites(L, d);
    MPS psi_i = load_state(argv[1], "L5_p5_N5_J1_U2.5"), psi_f = load_state(argv[1], "L5_p5_N5_J1_U50");
    GpuTDMRG stepper(sites, 1.0, 0.01, Args(1e-8, 80));
    OptimalControl<GpuTDMRG> OC(psi_f, psi_i, stepper, Nt, 0);
    stdvec control(Nt);
    for (int i = 0; i < Nt; ++i) control[i] = 2.5 + (50.0 - 2.5) * i / (Nt - 1);
    const stdvec fids = OC.getFidelityForAllT(control);

    const TrajectorySnapshots dev = OC.samplePsit({}, nshots, seed);
    const std::vector<MPS> psi_t = OC.getPsit();
    if (dev.size() != psi_t.size() || dev.shots() != nshots) throw std::runtime_error("entry count");
    int differ = 0, unexplained = 0, bad = 0;
    double dev_logp = 0;
    std::vector<int> hist_dev(L + 1, 0), hist_host(L + 1, 0);
    for (size_t t = 0; t < psi_t.size(); ++t) {
      const TrajectorySnapshots host = sampleFock(psi_t[t], nshots, seed, int(t));
      for (int s = 0; s < nshots; ++s) {
        int first = 0, sum = 0, def_dev = 0, def_host = 0;
        for (int k = 1; k <= L; ++k) {
          const int n = dev.config(t, s, k);
          if (n < 0 || n > d) ++bad;
          sum += n;
          def_dev += n != 1;
          def_host += host.config(0, s, k) != 1;
          if (!first && n != host.config(0, s, k)) first = k;
        }
        if (sum != L) ++bad;
        if (t + 1 == psi_t.size()) {
          ++hist_dev[def_dev];
          ++hist_host[def_host];
        }
        if (first) {
          ++differ;
          if (boundary_distance(OC.getEngine(), int(t), dev, t, s, first, d + 1, L, seed) >= 1e-9) ++unexplained;
        } else {
          dev_logp = std::max(dev_logp, std::fabs(dev.logp(t, s) - host.logp(0, s)));
        }
      }
    }
    // a subset of times, repeated: the same shots
    const TrajectorySnapshots sub = OC.samplePsit({20, 3, 3}, 64, seed);
    bool subset_equal = sub.size() == 3 && sub.shots() == 64;
    for (int e = 0; e < 3 && subset_equal; ++e)
      for (int s = 0; s < 64; ++s) {
        const size_t t = e == 0 ? 20 : 3;
        if (sub.logp(e, s) != dev.logp(t, s)) subset_equal = false;
        for (int k = 1; k <= L; ++k)
          if (sub.config(e, s, k) != dev.config(t, s, k)) subset_equal = false;
      }
    // the Mott-state probability along the ramp
    const std::vector<int> mott(L, 1);
    const stdvec pm = OC.getPsitFockProbability({}, mott);
    if (pm.size() != psi_t.size()) throw std::runtime_error("probability count");
    double dev_mott = 0;
    for (size_t t = 0; t < psi_t.size(); ++t) {
      const obs::Envs V = obs::envs(obs::dense(psi_t[t]));
      const double host = std::norm(host_amplitude(psi_t[t], mott)) / V.Renv[0][0].real();
      dev_mott = std::max(dev_mott, std::fabs(pm[t] - host));
    }

    std::ostringstream o;
    o.precision(17);
    o << "{\"shots\": " << nshots * int(psi_t.size()) << ", \"differ\": " << differ
      << ", \"unexplained\": " << unexplained << ", \"bad\": " << bad << ", \"dev_logp\": " << dev_logp << ", \"dev_mott\": " << dev_mott
      << ", \"subset_equal\": " << (subset_equal ? "true" : "false") << ", \"fid_last\": " << fids.back()
      << ", \"mott_first\": " << pm.front() << ", \"mott_last\": " << pm.back() << ", \"hist_dev\": [";
    for (int i = 0; i <= L; ++i) o << (i ? ", " : "") << hist_dev[i];
    o << "], \"hist_host\": [";
    for (int i = 0; i <= L; ++i) o << (i ? ", " : "") << hist_host[i];
    o << "]}";
    std::printf("%s\n", o.str().c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
