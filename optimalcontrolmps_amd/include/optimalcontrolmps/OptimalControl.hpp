// OptimalControl<TimeStepper>: the IPOPT-facing surface of the reference
// (include/OptimalControl.hpp:17-75, src/OptimalControl.cpp:1-592) with the
// same names, signatures and new_control caching semantics, over a
// TimeStepper whose Engine keeps the trajectories (psi_t, xi_t, xiHlist) and
// runs the hot path: GpuTDMRG::Engine (HBM-resident, HIP) in the product;
// the CPU restatement in tests/ (tests/cpp/oracle_stepper.hpp).
//
// TimeStepper concept (reference include/BH_tDMRG.hpp:34-39 plus the engine):
//   double getTstep() const;  Args getArgs() const;
//   void step(MPS&, double from, double to, bool forward = true) const;
//   std::unique_ptr<Engine> makeEngine(const MPS& target, const MPS& init, size_t N) const;
//   Engine: setShards(n), propagate(u, which), divT(), overlapFactor(),
//           fidelities(), precomputeXiH(), hessianRows(u, F, divT, H),
//           hessianFresh(u, F&, divT&, H) (all of the above for a new control), psiTrajectory(),
//           observe(which, ts, rows), observeSpectrum(which, ts, weights) (optional: getPsitObservables
//           needs the first, and the second when entropies are asked for),
//           sample(which, ts, nshots, seed), fockAmplitudes(which, ts, configs) (optional: samplePsit,
//           getPsitFockProbability),
//           observeMoments(which, ts) (optional: getPsitEnergies, with the stepper's hopping()),
//           observePairs(which_x, tx, which_y, ty) (optional: getControlSensitivities),
//           observeStrings(which, ts, tables), sites(), levels(), particles() (optional:
//           getPsitStringExpectations, getPsitParityOrder, getPsitCountingStatistics),
//           convertHessian(basis, Hu) (ControlBasis::convertHessian, src/ControlBasis.cpp:91-116).
//
// Host-side arithmetic kept verbatim from the reference: the regularisation
// terms (:88-143), the gradient assembly g_i = dt Re(divT_i F i) (:240-246),
// the GROUP conversions (ControlBasis.hpp) and the caching flags.
// Threading: setThreadCount(n) selects the number of row shards (GPUs for
// GpuTDMRG); psi_t and xi_t always propagate concurrently on the device.
#pragma once

#include <cmath>
#include <complex>
#include <memory>
#include <stdexcept>
#include <vector>

#include "ControlBasis.hpp"
#include "MPS.hpp"

template <class TimeStepper>
class OptimalControl {
 public:
  using MPS = ocmps::MPS;
  using Cplx = ocmps::Cplx;
  using stdvec = ocmps::stdvec;
  using rowmat = ocmps::rowmat;
  using Engine = typename TimeStepper::Engine;

  // GRAPE constructor (src/OptimalControl.cpp:7-27)
  OptimalControl(MPS& psi_target_, MPS& psi_init_, TimeStepper& stepper_, size_t N_, double gamma_,
                 bool BFGS_ = false)
      : timeStepper(stepper_), gamma(gamma_), tstep(stepper_.getTstep()), N(N_), M(0),
        psi_target(psi_target_), psi_init(psi_init_), GRAPE(true), BFGS(BFGS_) {
    init();
  }
  // GROUP constructor (:30-50)
  OptimalControl(MPS& psi_target_, MPS& psi_init_, TimeStepper& stepper_, ControlBasis& basis_, double gamma_,
                 bool BFGS_ = false)
      : timeStepper(stepper_), basis(basis_), gamma(gamma_), tstep(stepper_.getTstep()), N(basis_.getN()),
        M(basis_.getM()), psi_target(psi_target_), psi_init(psi_init_), GRAPE(false), BFGS(BFGS_) {
    init();
  }

  std::vector<MPS> getPsit() const { return engine->psiTrajectory(); }
  // The drivers' loops over getPsit() without the states leaving the device:
  // occupation distributions, bond dimensions and a+a / nn correlation rows of
  // psi_t for t in ts (empty: all), rows = start sites 1..L (correlations.hpp
  // has the reference-named overloads that read the result).  Only for
  // steppers whose Engine has observe() (GpuTDMRG).  entropy: also the
  // entanglement entropy of every bond (AnalyzeQuench's entanglementEntropy
  // loop; Engine::observeSpectrum), read by entanglementEntropy(obs, e).
  ocmps::TrajectoryObservables getPsitObservables(const std::vector<int>& ts = {},
                                                  const std::vector<int>& rows = {}, bool entropy = false) const {
    ocmps::TrajectoryObservables o = engine->observe(0, ts, rows);
    if (entropy) o.entropy = engine->observeSpectrum(0, ts, false).entropy;
    return o;
  }
  // Projective occupation snapshots of psi_t for t in ts (empty: all), drawn on
  // the device (Engine::sample; the host counterpart for one state is sampleFock of
  // correlations.hpp, with the same random numbers): what a quantum-gas
  // microscope records.  Only for steppers whose Engine has sample() (GpuTDMRG).
  ocmps::TrajectorySnapshots samplePsit(const std::vector<int>& ts, int nshots, unsigned long long seed) const {
    return engine->sample(0, ts, nshots, seed);
  }
  // |<config|psi_t>|^2 / <psi_t|psi_t> for t in ts (empty: all), e.g. the
  // Mott-state probability along the ramp (Engine::fockAmplitudes + the norms of observe()).
  stdvec getPsitFockProbability(const std::vector<int>& ts, const std::vector<int>& config) const {
    const std::vector<signed char> cf(config.begin(), config.end());
    const std::vector<Cplx> amp = engine->fockAmplitudes(0, ts, cf);
    const ocmps::TrajectoryObservables o = engine->observe(0, ts, {});
    stdvec pr(amp.size());
    for (size_t e = 0; e < amp.size(); ++e) pr[e] = o.norm2[e] > 0 ? std::norm(amp[e]) / o.norm2[e] : 0.0;
    return pr;
  }
  // <psi_t|O_m|psi_t> for t in ts (empty: all) of products of diagonal one-site operators, [e][m], raw:
  // tables[m] is L x p, row k - 1 the diagonal of operator m on site k (all 1: outside its support).
  // Reads the device trajectory (Engine::observeStrings); nothing is propagated.  The host counterpart for
  // one state is stringExpectation of correlations.hpp.  Only for steppers whose Engine has observeStrings().
  std::vector<std::vector<Cplx>> getPsitStringExpectations(const std::vector<int>& ts,
                                                           const std::vector<std::vector<Cplx>>& tables) const {
    return engine->observeStrings(0, ts, tables);
  }
  // The parity (string) order of psi_t from site i: [e][j - 1] = <prod_{k=i..j} (-1)^(n_k - nbar)> / norm2
  // for j >= i, entries below i are 0: the Mott insulator's order parameter as a quantum-gas microscope
  // measures it.
  rowmat getPsitParityOrder(const std::vector<int>& ts, int i, int nbar) const {
    const int L = engine->sites(), p = engine->levels();
    if (i < 1 || i > L) throw std::invalid_argument("getPsitParityOrder: site out of range");
    std::vector<std::vector<Cplx>> tables(size_t(L - i + 2), std::vector<Cplx>(size_t(L) * p, Cplx(1, 0)));
    for (int j = i; j <= L; ++j)
      for (int k = i; k <= j; ++k)
        for (int n = 0; n < p; ++n) tables[j - i][size_t(k - 1) * p + n] = ((n - nbar) % 2 == 0) ? 1.0 : -1.0;
    const std::vector<std::vector<Cplx>> v = engine->observeStrings(0, ts, tables);  // (the last table: norm2)
    rowmat out;
    for (const std::vector<Cplx>& r : v) {
      stdvec row(size_t(L), 0.0);
      for (int j = i; j <= L; ++j) row[j - 1] = r[j - i].real() / r.back().real();
      out.push_back(row);
    }
    return out;
  }
  // The counting statistics of the block of sites i..j in psi_t: [e][m] = P(N_A = m), m = 0..Q, from the
  // Q + 1 generating-function values <exp(i theta_r N_A)>, theta_r = 2 pi r / (Q + 1), of the device and a
  // discrete Fourier transform on the host (exact, since N_A <= Q).
  rowmat getPsitCountingStatistics(const std::vector<int>& ts, int i, int j) const {
    const int L = engine->sites(), p = engine->levels(), Q1 = engine->particles() + 1;
    if (i < 1 || j < i || j > L) throw std::invalid_argument("getPsitCountingStatistics: block out of range");
    const double two_pi = 2 * std::acos(-1.0);
    std::vector<std::vector<Cplx>> tables(size_t(Q1), std::vector<Cplx>(size_t(L) * p, Cplx(1, 0)));
    for (int r = 0; r < Q1; ++r)
      for (int k = i; k <= j; ++k)
        for (int n = 0; n < p; ++n) tables[r][size_t(k - 1) * p + n] = std::polar(1.0, two_pi * r * n / Q1);
    const std::vector<std::vector<Cplx>> G = engine->observeStrings(0, ts, tables);  // (r = 0: norm2)
    rowmat out;
    for (const std::vector<Cplx>& g : G) {
      stdvec row(size_t(Q1), 0.0);
      for (int m = 0; m < Q1; ++m) {
        Cplx s = 0;
        for (int r = 0; r < Q1; ++r) s += std::polar(1.0, -two_pi * r * m / Q1) * g[r];
        row[m] = s.real() / Q1 / g[0].real();
      }
      out.push_back(row);
    }
    return out;
  }
  // E_t = <psi_t|H(u_t)|psi_t> / <psi_t|psi_t> and Var_t = <H(u_t)^2> - E_t^2 of the stored
  // psi_t with u = the control as given to the last propagation (GROUP coefficients are
  // converted) and the stepper's J: the drift of E over stretches of constant u measures
  // Trotter plus truncation error, E_T - E_0(u_T) is the residual energy of a ramp.  Reads the
  // device trajectory (Engine::observeMoments); nothing is propagated.  Only for steppers
  // whose Engine has observeMoments() and that have hopping() (GpuTDMRG).  H here is the
  // homogeneous chain's: with a non-zero site potential on the stepper this throws
  // std::invalid_argument (the variance would need <K V> and <D V>, which the moments lack).
  ocmps::TrajectoryEnergies getPsitEnergies(const stdvec& control) {
    const stdvec u = GRAPE ? control : basis.convertControl(control);
    if (u.size() != N) throw std::invalid_argument("getPsitEnergies: control has the wrong length");
    if (engine->hasPotential())
      throw std::invalid_argument(
          "getPsitEnergies: the energies describe the homogeneous Hamiltonian; with a site potential the energy "
          "and its variance need <K V> and <D V>, which ocg_observe_moments does not return");
    ocmps::TrajectoryEnergies r;
    r.moments = engine->observeMoments(0, {});
    const double J = timeStepper.hopping();
    for (size_t t = 0; t < r.moments.size(); ++t) {
      r.energy.push_back(r.moments.energy(t, J, u[t]));
      r.variance.push_back(r.moments.energyVariance(t, J, u[t]));
    }
    return r;
  }
  // First-order sensitivities of the fidelity cost to U(t) (the fidelity gradient itself), to the
  // hopping J(t) and to a site potential eps_k(t), and the overlap <xi_t|psi_t>, on the time grid:
  // tstep Re(i <xi_t|dH/dlambda|psi_t> F), the reference's gradient formula (:240-246) with
  // dH/dJ = -K and dH/deps_k = n_k, so with its time discretisation: a total over t takes trapezoid
  // weights.  GROUP coefficients are converted to the time grid first and the results are not
  // projected back onto the basis.  Makes psi, xi and divT available exactly as the non-BFGS gradient
  // does (new_control = false after a gradient propagates nothing), then reads the device
  // trajectories (Engine::observePairs).  Only for steppers whose Engine has observePairs() (GpuTDMRG).
  ocmps::ControlSensitivities getControlSensitivities(const stdvec& control, const bool new_control = true) {
    const stdvec u = GRAPE ? control : basis.convertControl(control, new_control);
    if (u.size() != N) throw std::invalid_argument("getControlSensitivities: control has the wrong length");
    if (new_control) {
      calculatedXi = false;
      calcPsiXiDivT(u);
    }
    if (!calculatedXi) {
      calcXi(u);
      calcDivT();
    }
    const Cplx F = engine->overlapFactor(), I(0, 1);
    const ocmps::PairObservables pr = engine->observePairs(1, {}, 0, {});
    ocmps::ControlSensitivities s;
    for (size_t t = 0; t < N; ++t) {
      s.dU.push_back(tstep * (I * pr.interaction(t) * F).real());
      s.dJ.push_back(tstep * (I * (-pr.hopping(t)) * F).real());
      stdvec e;
      for (int k = 1; k <= pr.L; ++k) e.push_back(tstep * (I * pr.number(t, k) * F).real());
      s.dEps.push_back(e);
      s.overlap.push_back(pr.ovl[t]);
    }
    return s;
  }
  size_t getM() const { return M; }
  size_t getN() const { return N; }
  stdvec getControl(const stdvec& control) { return GRAPE ? control : basis.convertControl(control); }
  // t = 0, dt, ... accumulated like the reference (:183-197)
  stdvec getTimeAxis() const {
    stdvec t;
    const double h = timeStepper.getTstep();
    for (double x = 0; std::fabs(x - N * h) > 1e-2 * h; x += h) t.push_back(x);
    return t;
  }
  void setGamma(double g) { gamma = g; }
  void setThreadCount(const size_t n) {
    if (n < 1) throw std::invalid_argument("Mininum threadCount is 1.");
    threadCount = n;
    engine->setShards(n);
  }
  void setGRAPE(const bool useGRAPE) {
    GRAPE = useGRAPE;
    calculatedXi = false;
  }
  void setBFGS(const bool useBFGS) {
    BFGS = useBFGS;
    calculatedXi = false;
  }
  bool useBFGS() const { return BFGS; }

  void propagatePsi(const stdvec& control) { calcPsi(GRAPE ? control : basis.convertControl(control)); }
  double getCost(const stdvec& control, const bool new_control = true) {
    return GRAPE ? calcCost(control, new_control) : calcCost(basis.convertControl(control, new_control), new_control);
  }
  stdvec getAnalyticGradient(const stdvec& control, const bool new_control = true) {
    if (GRAPE) return calcAnalyticGradient(control, new_control);
    return basis.convertGradient(calcAnalyticGradient(basis.convertControl(control, new_control), new_control));
  }
  // one code path for any threadCount: the rows are sharded by the engine
  rowmat getHessian(const stdvec& control, const bool new_control = true) {
    if (GRAPE) return calcHessian(control, new_control);
    // ControlBasis::convertHessian by the engine (the GPU engine projects on the device)
    return engine->convertHessian(basis, calcHessian(basis.convertControl(control, new_control), new_control));
  }
  stdvec getFidelityForAllT(const stdvec& control, const bool new_control = true) {
    return GRAPE ? calcFidelityForAllT(control, new_control)
                 : calcFidelityForAllT(basis.convertControl(control, new_control), new_control);
  }
  rowmat getControlJacobian() const {
    if (!GRAPE) return basis.getControlJacobian();
    rowmat I(N, stdvec(N, 0.0));
    for (size_t i = 0; i < N; ++i) I[i][i] = 1;
    return I;
  }

  // engine access (benchmarks, diagnostics)
  Engine& getEngine() { return *engine; }

 private:
  void init() {
    if (N < 4) throw std::invalid_argument("OptimalControl: N must be >= 4 (regularisation stencils)");
    threadCount = 1;
    calculatedXi = false;
    engine = timeStepper.makeEngine(psi_target, psi_init, N);
    divT.assign(N, Cplx(0, 0));
  }
  // ---- trajectories (:374-438)
  void calcPsi(const stdvec& u) {
    engine->propagate(u, 1);
    calculatedXi = false;
  }
  void calcXi(const stdvec& u) {
    engine->propagate(u, 2);
    calculatedXi = true;
  }
  void calcDivT() { divT = engine->divT(); }
  void calcPsiXiDivT(const stdvec& u) {
    engine->propagate(u, 3);
    calculatedXi = true;
    calcDivT();
  }
  // ---- regularisation (:88-143)
  double calcRegularization(const stdvec& u) const {
    double s = 0;
    for (size_t i = 0; i + 1 < N; ++i) {
      const double d = u[i + 1] - u[i];
      s += d * d / tstep;
    }
    return gamma / 2.0 * s;
  }
  stdvec calcRegularizationGrad(const stdvec& u) const {
    stdvec g(N);
    g[0] = -gamma * (-5.0 * u[1] + 4.0 * u[2] - u[3] + 2.0 * u[0]) / tstep;
    for (size_t i = 1; i + 1 < N; ++i) g[i] = -gamma * (u[i + 1] + u[i - 1] - 2.0 * u[i]) / tstep;
    g[N - 1] = -gamma * (-5.0 * u[N - 2] + 4.0 * u[N - 3] - u[N - 4] + 2.0 * u[N - 1]) / tstep;
    return g;
  }
  rowmat calcRegularizationHessian() const {
    rowmat H(N, stdvec(N, 0.0));
    const double g = gamma / tstep;
    for (size_t i = 1; i + 1 < N; ++i) {
      H[i][i - 1] = -g;
      H[i][i + 1] = -g;
      H[i][i] = 2.0 * g;
    }
    H[1][0] = 0;  // control endpoints are fixed
    H[N - 2][N - 1] = 0;
    return H;
  }
  // ---- cost / gradient / Hessian (:204-249, :281-372, :440-490)
  double calcCost(const stdvec& u, const bool new_control) {
    if (new_control) calcPsi(u);
    const double f = std::norm(engine->overlapFactor());  // |<target|psi_T>|^2
    return 0.5 * (1.0 - f) + calcRegularization(u);
  }
  stdvec calcFidelityGrad(const stdvec& u, const bool new_control) {
    if (new_control) {
      calculatedXi = false;
      if (BFGS) {
        // calcPsi + the inline xi propagation of the BFGS path (:210-229): xi
        // never reads psi, so both chains run concurrently in one launch
        engine->propagate(u, 3);
        calcDivT();
      } else {
        calcPsiXiDivT(u);
      }
    } else if (BFGS) {
      // the reference re-propagates xi inline on every BFGS gradient (:217-229)
      engine->propagate(u, 2);
      calcDivT();
    }
    if (!BFGS && !calculatedXi) {
      calcXi(u);
      calcDivT();
    }
    const Cplx F = engine->overlapFactor();
    stdvec g(N);
    for (size_t i = 0; i < N; ++i) g[i] = tstep * (divT[i] * F * Cplx(0, 1)).real();
    return g;
  }
  stdvec calcAnalyticGradient(const stdvec& u, const bool new_control) {
    stdvec g = calcFidelityGrad(u, new_control);
    const stdvec r = calcRegularizationGrad(u);
    for (size_t i = 0; i < N; ++i) g[i] += r[i];
    return g;
  }
  rowmat calcHessian(const stdvec& u, const bool new_control) {
    if (new_control) {
      // psi, xi, divT, xiHlist and the rows in one pipelined engine call
      rowmat H = calcRegularizationHessian();
      Cplx F;
      engine->hessianFresh(u, F, divT, H);
      calculatedXi = true;
      return H;
    }
    if (!calculatedXi) {
      calcXi(u);
      calcDivT();
    }
    rowmat H = calcRegularizationHessian();
    const Cplx F = engine->overlapFactor();
    engine->precomputeXiH();  // xiHlist (:300-303), recomputed on every call like the reference
    engine->hessianRows(u, F, divT, H);
    return H;
  }
  stdvec calcFidelityForAllT(const stdvec& u, const bool new_control) {
    if (new_control) calcPsi(u);
    return engine->fidelities();
  }

  TimeStepper timeStepper;
  ControlBasis basis;
  double gamma, tstep;
  size_t N, M, threadCount = 1;
  MPS psi_target, psi_init;
  std::vector<Cplx> divT;
  bool GRAPE, BFGS, calculatedXi = false;
  std::unique_ptr<Engine> engine;
};
