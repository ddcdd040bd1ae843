// Ground-state preparation, the reference's InitializeState
// (include/InitializeState.hpp:18-117), on the MI355X: same signatures and
// starting guess, ITensor's DMRG replaced by imaginary-time evolution on the
// device (ocg_imag_steps: the BH_tDMRG sweep with exp(-tau h) gates and
// exp(-tau U n(n-1)/4) phases, normalised and truncated with the given
// threshold / maxBondDim).
//
//   starting guess  "Occ1" on the Npart right-most sites, "Emp" elsewhere
//                   (:26-40); Npart > N is refused like the reference
//   H               -J sum (a_i a^dag_{i+1} + h.c.) + U/2 sum n(n-1) (:42-51)
//   schedule        tau = 0.05, 0.01, 0.002, 0.001, 0.0005, each run in
//                   blocks of 25 steps until 1 - |<prev|new>| < 1e-13 (the
//                   tau^2 Trotter fixed-point infidelity: 6e-8 at L=5, U=2.5)
//   defaults        maxBondDim 200, threshold 1e-9 (the overload without
//                   them, :18-60: sweeps.maxm() up to 200, cutoff 1e-9)
//   certificate     optional out-parameters: the energy <H(J, U)> of the returned
//                   state, its variance <H^2> - <H>^2 (0 for an eigenstate) and the
//                   seven raw moments behind them (ocg_observe_moments_states)
//   site potential  the overload with site energies eps adds sum_k eps_k n_k to H
//                   (ocg_set_potential).  Its energy / variance out-parameters
//                   throw std::invalid_argument when eps is not zero: they describe
//                   the homogeneous H, and the variance with a potential needs
//                   <K V> and <D V>, which ocg_observe_moments does not return
#pragma once

#include <cmath>
#include <complex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/ocmps.h"
#include "MPS.hpp"

namespace ocmps {

// product state with Npart bosons on the right-most sites, all bonds 1
inline MPS productState(int L, int p, int Npart) {
  if (Npart > L) throw std::invalid_argument("Npart > N not supported");
  const int Q1 = Npart + 1;
  std::vector<int> dims(size_t(L + 1) * Q1, 0);
  int q = 0;
  dims[0] = 1;
  for (int b = 1; b <= L; ++b) {
    if (b > L - Npart) ++q;
    dims[size_t(b) * Q1 + q] = 1;
  }
  return MPS(L, p, Npart, dims, std::vector<Cplx>(size_t(L), Cplx(1.0, 0.0)));
}

namespace detail_gs {
inline void check(int rc, const ocg_ctx* c, const char* what) {
  if (rc != OCG_OK) {
    const char* m = ocg_last_error(c);
    throw std::runtime_error(std::string(what) + ": " + (m ? m : "error"));
  }
}
}  // namespace detail_gs

// the ground state in the static site potential sum_k eps_k n_k (eps: L site energies, site 1 first)
inline MPS InitializeState(const BoseHubbard& sites, const int Npart, const double J, const double U,
                           const std::vector<double>& eps, const int maxBondDim = 200, const double threshold = 1e-9,
                           bool /*silent*/ = true, int device = 0, double* energy = nullptr,
                           double* variance = nullptr, double* moments7 = nullptr) {
  const int L = sites.N(), p = sites.localDim();
  if (!eps.empty() && eps.size() != size_t(L)) throw std::invalid_argument("InitializeState: eps must have L entries");
  bool trapped = false;
  for (double e : eps) trapped = trapped || e != 0.0;
  if (trapped && (energy || variance))
    throw std::invalid_argument(
        "InitializeState: the energy and variance out-parameters describe the homogeneous Hamiltonian; with a "
        "site potential they need <K V> and <D V>, which ocg_observe_moments does not return");
  MPS psi = productState(L, p, Npart);
  ocg_ctx* c = nullptr;
  detail_gs::check(ocg_create(device, L, p, Npart, J, 0.01, threshold, maxBondDim, &c), nullptr, "ocg_create");
  try {
    if (trapped) detail_gs::check(ocg_set_potential(c, eps.data()), c, "ocg_set_potential");
    ocg_info info;
    detail_gs::check(ocg_get_info(c, &info), c, "ocg_get_info");
    std::vector<int> od(psi.dims.size());
    std::vector<Cplx> out(info.mps_max_nelem);
    const double taus[] = {0.05, 0.01, 0.002, 0.001, 0.0005};
    const int block = 25, max_steps = 8000;
    for (double tau : taus) {
      for (int done = 0; done < max_steps; done += block) {
        size_t n = 0;
        detail_gs::check(ocg_imag_steps(c, psi.dims.data(), psi.raw(), U, tau, block, od.data(),
                                        reinterpret_cast<double*>(out.data()), out.size(), &n),
                         c, "ocg_imag_steps");
        MPS nw(L, p, Npart, od, std::vector<Cplx>(out.begin(), out.begin() + n));
        double ov[2];
        detail_gs::check(ocg_overlap(c, psi.dims.data(), psi.raw(), nw.dims.data(), nw.raw(), 0, ov), c,
                         "ocg_overlap");
        psi = std::move(nw);
        if (1.0 - std::hypot(ov[0], ov[1]) < 1e-13) break;
      }
    }
    if (energy || variance || moments7) {
      double m[7];
      const double* data[1] = {psi.raw()};
      detail_gs::check(ocg_observe_moments_states(c, 1, psi.dims.data(), data, m), c, "ocg_observe_moments_states");
      const double e = (-J * m[1] + U * m[2]) / m[0];
      if (energy) *energy = e;
      if (variance) *variance = (J * J * m[3] - 2 * J * U * m[5] + U * U * m[4]) / m[0] - e * e;
      if (moments7)
        for (int j = 0; j < 7; ++j) moments7[j] = m[j];
    }
  } catch (...) {
    ocg_destroy(c);
    throw;
  }
  ocg_destroy(c);
  return psi;
}

inline MPS InitializeState(const BoseHubbard& sites, const int Npart, const double J, const double U,
                           const int maxBondDim, const double threshold, bool silent = true, int device = 0,
                           double* energy = nullptr, double* variance = nullptr, double* moments7 = nullptr) {
  return InitializeState(sites, Npart, J, U, std::vector<double>(), maxBondDim, threshold, silent, device, energy,
                         variance, moments7);
}

inline MPS InitializeState(const BoseHubbard& sites, const int Npart, const double J, const double U,
                           bool silent = true) {
  return InitializeState(sites, Npart, J, U, 200, 1e-9, silent);
}

}  // namespace ocmps
