// Times the host path of one state: entanglementEntropy(sites, psi) of
// correlations.hpp on a state read from a file (header L p Q ndims ndata, int32
// dims, complex128 data).  Built and run by observe_timing.py.
#include <chrono>
#include <cstdio>
#include <fstream>
#include <vector>

#include "../include/optimalcontrolmps/correlations.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int h[5];
  f.read(reinterpret_cast<char*>(h), sizeof h);
  std::vector<int> dims(h[3]);
  f.read(reinterpret_cast<char*>(dims.data()), sizeof(int) * h[3]);
  std::vector<ocmps::Cplx> data(h[4]);
  f.read(reinterpret_cast<char*>(data.data()), sizeof(double) * 2 * h[4]);
  const ocmps::MPS psi(h[0], h[1], h[2], dims, data);
  const ocmps::BoseHubbard sites(h[0], h[1] - 1);
  const auto t0 = std::chrono::steady_clock::now();
  const auto S = ocmps::entanglementEntropy(sites, psi);
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  double mx = 0;
  for (double v : S) mx = v > mx ? v : mx;
  std::printf("{\"seconds\": %.6f, \"max_entropy\": %.12f}\n", s, mx);
  return 0;
}
