// Times the host path of one state on one thread: sampleFock(psi, nshots, seed, id)
// of correlations.hpp ("seconds": the whole call, which forms the environments and
// then draws; "environments_seconds": a call with no shots) on a state read from a
// file (header L p Q ndims ndata, int32 dims, complex128 data).  Built and run by
// observe_timing.py.  Usage: host_sample_timing <state> [nshots]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../include/optimalcontrolmps/correlations.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const int nshots = argc > 2 ? std::atoi(argv[2]) : 1024;
  std::ifstream f(argv[1], std::ios::binary);
  int h[5];
  f.read(reinterpret_cast<char*>(h), sizeof h);
  std::vector<int> dims(h[3]);
  f.read(reinterpret_cast<char*>(dims.data()), sizeof(int) * h[3]);
  std::vector<ocmps::Cplx> data(h[4]);
  f.read(reinterpret_cast<char*>(data.data()), sizeof(double) * 2 * h[4]);
  const ocmps::MPS psi(h[0], h[1], h[2], dims, data);
  const auto t0 = std::chrono::steady_clock::now();
  const ocmps::TrajectorySnapshots none = ocmps::sampleFock(psi, 0, 1, 0);  // the environments alone
  const auto t1 = std::chrono::steady_clock::now();
  const ocmps::TrajectorySnapshots s = ocmps::sampleFock(psi, nshots, 1, 0);
  const auto t2 = std::chrono::steady_clock::now();
  double lp = 0;
  for (int i = 0; i < s.shots(); ++i) lp += s.logp(0, i);
  std::printf("{\"seconds\": %.6f, \"environments_seconds\": %.6f, \"nshots\": %d, \"mean_logp\": %.12f, "
              "\"entries\": %zu}\n",
              std::chrono::duration<double>(t2 - t1).count(), std::chrono::duration<double>(t1 - t0).count(), nshots,
              s.shots() ? lp / s.shots() : 0.0, none.size());
  return 0;
}
