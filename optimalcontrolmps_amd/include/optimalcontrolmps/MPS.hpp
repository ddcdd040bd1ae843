// Host-side value types of the optimalcontrolmps_amd C++ facade.
//
// ocmps::MPS replaces ITensor's IQMPS at the OptimalControl boundary
// (reference include/OptimalControl.hpp:23-27 stores IQMPS psi_target /
// psi_init / psi_t).  It holds a particle-number (U(1) "Nb") conserving
// matrix-product state in the engine's compact interchange format, defined
// in include/ocmps.h: per-bond sector dimensions plus the non-zero
// (sector, occupation) blocks of every site tensor, row-major.
//
// Args replaces itensor::Args{"Cutoff=", c, "Maxm=", m}
// (main/OptimizeRamp.cpp:88, tests/GradientTests.cpp:41); BoseHubbard
// replaces the SiteSet built by BoseHubbard(L, d) (include/BH_sites.h:57-112):
// L sites with occupations 0..d, i.e. local dimension p = d + 1.
#pragma once

#include <complex>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

namespace ocmps {

using Cplx = std::complex<double>;
using stdvec = std::vector<double>;
using rowmat = std::vector<std::vector<double>>;

struct Args {
  double cutoff = 1e-8;  // relative truncation error per decomposition ("Cutoff=")
  int maxm = 0;          // bond-dimension cap ("Maxm="); <= 0 selects ITensor's default (5000)
  Args() = default;
  Args(double cutoff_, int maxm_ = 0) : cutoff(cutoff_), maxm(maxm_) {}
};

struct BoseHubbard {
  int L = 0;  // sites
  int d = 0;  // maximal occupation per site
  BoseHubbard() = default;
  BoseHubbard(int L_, int d_) : L(L_), d(d_) {
    if (L_ < 2 || d_ < 1) throw std::invalid_argument("BoseHubbard: need L >= 2 and d >= 1");
  }
  int N() const { return L; }
  int localDim() const { return d + 1; }
};

struct MPS {
  int L = 0, p = 0, Q = 0;  // sites, local dimension, particle number
  std::vector<int> dims;    // dims[b*(Q+1) + q], bonds b = 0..L
  std::vector<Cplx> data;   // compact blocks (include/ocmps.h)

  MPS() = default;
  MPS(int L_, int p_, int Q_, std::vector<int> dims_, std::vector<Cplx> data_)
      : L(L_), p(p_), Q(Q_), dims(std::move(dims_)), data(std::move(data_)) {
    if (dims.size() != size_t(L + 1) * size_t(Q + 1)) throw std::invalid_argument("MPS: dims has the wrong size");
    if (data.size() != nelem(L, p, Q, dims.data())) throw std::invalid_argument("MPS: data has the wrong size");
  }
  bool empty() const { return L == 0; }
  int dim(int b, int q) const { return (q < 0 || q > Q) ? 0 : dims[size_t(b) * (Q + 1) + q]; }
  int bondDim(int b) const {
    int s = 0;
    for (int q = 0; q <= Q; ++q) s += dim(b, q);
    return s;
  }
  // complex elements of the compact format for the given sector dims
  static size_t nelem(int L, int p, int Q, const int* d) {
    size_t s = 0;
    for (int k = 1; k <= L; ++k)
      for (int q = 0; q <= Q; ++q)
        for (int n = 0; n < p && q + n <= Q; ++n) s += size_t(d[(k - 1) * (Q + 1) + q]) * d[k * (Q + 1) + q + n];
    return s;
  }
  const double* raw() const { return reinterpret_cast<const double*>(data.data()); }
};

// Energy moments of stored states (ocg_observe_moments): for H(J, U) = -J K + U D with
// K the hopping sum and D = sum_i n_i (n_i - 1) / 2, per entry e the raw numbers
// norm2, <K>, <D>, <K K>, <D D>, Re <K D>, Im <K D> (none divided by norm2).
struct TrajectoryMoments {
  std::vector<int> ts;      // [e] state index
  std::vector<double> mom;  // [e][7]
  size_t size() const { return ts.size(); }
  const double* at(size_t e) const { return mom.data() + 7 * e; }
  double norm2(size_t e) const { return at(e)[0]; }
  double k1(size_t e) const { return at(e)[1]; }
  double d1(size_t e) const { return at(e)[2]; }
  // <H(J, U)> = (-J k1 + U d1) / norm2
  double energy(size_t e, double J, double U) const { return (-J * at(e)[1] + U * at(e)[2]) / at(e)[0]; }
  // <H^2> - <H>^2
  double energyVariance(size_t e, double J, double U) const {
    const double* m = at(e);
    const double en = energy(e, J, U);
    return (J * J * m[3] - 2 * J * U * m[5] + U * U * m[4]) / m[0] - en * en;
  }
};
// E_t = <H(u_t)> and Var_t of the stored psi_t (OptimalControl::getPsitEnergies)
struct TrajectoryEnergies {
  TrajectoryMoments moments;
  std::vector<double> energy, variance;  // [e]
};

// Transition matrix elements between stored states (ocg_observe_pairs): per pair e of a bra x
// (state tx[e]) and a ket y (state ty[e]) the raw numbers <x|y>, <x|P_k(n)|y> and the hopping
// elements <x|a+_b a_{b+1}|y>, <x|a_b a+_{b+1}|y> (none divided by a norm).
struct PairObservables {
  int L = 0, p = 0;
  std::vector<int> tx, ty;  // [e] state indices
  std::vector<Cplx> ovl;    // [e]
  std::vector<Cplx> occ;    // [e][L][p]
  std::vector<Cplx> hop;    // [e][L-1][2]
  size_t size() const { return tx.size(); }
  // <x|n_k|y>, k = 1..L
  Cplx number(size_t e, int k) const {
    Cplx s = 0;
    for (int n = 0; n < p; ++n) s += double(n) * occ[(e * L + (k - 1)) * p + n];
    return s;
  }
  // <x|D|y>, D = sum_k n_k (n_k - 1) / 2
  Cplx interaction(size_t e) const {
    Cplx s = 0;
    for (int k = 0; k < L; ++k)
      for (int n = 0; n < p; ++n) s += 0.5 * n * (n - 1.0) * occ[(e * L + k) * p + n];
    return s;
  }
  // <x|K|y>, K = sum_b (a+_b a_{b+1} + a_b a+_{b+1})
  Cplx hopping(size_t e) const {
    Cplx s = 0;
    for (int j = 0; j < 2 * (L - 1); ++j) s += hop[e * 2 * (L - 1) + j];
    return s;
  }
};
// First-order sensitivities of the cost to the controls on the time grid
// (OptimalControl::getControlSensitivities): tstep Re(i <xi_t|dH/dlambda|psi_t> F) for
// lambda = U (dH = D, the fidelity gradient), J (dH = -K) and a site potential eps_k (dH = n_k);
// overlap[t] = <xi_t|psi_t>, constant in t for exact unitary evolution.  A total over t takes
// trapezoid weights (1/2 at t = 0 and t = N - 1).
struct ControlSensitivities {
  stdvec dU, dJ;              // [t]
  rowmat dEps;                // [t][k]
  std::vector<Cplx> overlap;  // [t]
};

// Observables of nt trajectory states evaluated on the device (ocg_observe,
// ocg_observe_spectrum, include/ocmps.h): what GpuTDMRG::Engine::observe and
// OptimalControl::getPsitObservables return and the overloads of
// correlations.hpp read.  Entry e belongs to trajectory state ts[e].
struct TrajectoryObservables {
  int L = 0, p = 0;
  std::vector<int> ts;        // [e] state index
  std::vector<int> rows;      // start sites (1..L) of the correlation rows
  std::vector<double> norm2;  // [e] <psi|psi>
  std::vector<double> occ;    // [e][L][p] occupation distribution (raw: sums to norm2 per site)
  std::vector<int> bond;      // [e][L+1] bond dimensions
  std::vector<Cplx> ada;      // [e][row][L] <a+_i a_j>, j >= i (0 for j < i)
  std::vector<double> nn;     // [e][row][L] <n_i n_j>, j >= i
  // entanglement spectra (ocg_observe_spectrum); empty unless asked for
  std::vector<double> entropy;  // [e][L-1] von Neumann entropy of the bonds b = 1..L-1
  std::vector<double> schmidt;  // [e][L-1][wcap] raw Schmidt weights, descending, 0 past the bond dimension
  std::vector<int> sector;      // [e][L-1][wcap] left particle count of each weight, -1 past the bond dimension
  int wcap = 0;
  size_t size() const { return ts.size(); }
  bool hasEntropy() const { return L > 1 && entropy.size() == ts.size() * size_t(L - 1) && !ts.empty(); }
  double entropyAt(size_t e, int b) const { return entropy[e * (L - 1) + (b - 1)]; }
  double schmidtAt(size_t e, int b, int j) const { return schmidt[(e * (L - 1) + (b - 1)) * wcap + j]; }
  int sectorAt(size_t e, int b, int j) const { return sector[(e * (L - 1) + (b - 1)) * wcap + j]; }
  double occAt(size_t e, int site, int n) const { return occ[(e * L + (site - 1)) * p + n]; }
  int bondDim(size_t e, int b) const { return bond[e * (L + 1) + b]; }
  int maxBondDim(size_t e) const {
    int m = 0;
    for (int b = 0; b <= L; ++b) m = m < bondDim(e, b) ? bondDim(e, b) : m;
    return m;
  }
  // index of start site i among rows, -1 if it was not requested
  int rowOf(int i) const {
    for (size_t r = 0; r < rows.size(); ++r)
      if (rows[r] == i) return int(r);
    return -1;
  }
};

// Fock-state snapshots of nt trajectory states drawn on the device (ocg_sample,
// include/ocmps.h): what GpuTDMRG::Engine::sample, OptimalControl::samplePsit and
// the host sampleFock (correlations.hpp) return.  Entry e belongs to trajectory
// state ts[e]; a shot of a zero state has -1 at every site and logp = -inf.
struct TrajectorySnapshots {
  int L = 0, nshots = 0;
  std::vector<int> ts;               // [e] state index (the id mixed into the random numbers)
  std::vector<signed char> configs;  // [e][shot][L] occupations
  std::vector<double> logps;         // [e][shot] ln(|<n|psi>|^2 / <psi|psi>)
  size_t size() const { return ts.size(); }
  int shots() const { return nshots; }
  // occupation of site k = 1..L in shot s of entry e
  int config(size_t e, int s, int k) const { return configs[(e * nshots + s) * L + (k - 1)]; }
  double logp(size_t e, int s) const { return logps[e * nshots + s]; }
};

}  // namespace ocmps
