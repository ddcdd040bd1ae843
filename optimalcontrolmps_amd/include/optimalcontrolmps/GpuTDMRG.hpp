// GpuTDMRG: the MI355X TimeStepper behind the reference's stepper concept
// (reference include/BH_tDMRG.hpp:17-40, src/BH_tDMRG.cpp), implemented over
// the C-ABI of liboptimalcontrolmps_amd.so (include/ocmps.h).
//
// Stepper members kept with the reference's names and meaning:
//   GpuTDMRG(sites, J, tstep, args)          BH_tDMRG(sites, J, tstep, args)  (:34)
//   setTstep / getTstep / getArgs            (:35, :38, :39)
//   step(psi, from, to, propagateForward)    (:36; src/BH_tDMRG.cpp:111-230)
//   propagatorDeriv(u)                       (:37; src/BH_tDMRG.cpp:238-241)
// Beyond the reference: setPotential(eps) / getPotential(), the static site
// potential sum_k eps_k n_k of every step (ocg_set_potential); propagatorDeriv
// is unchanged by it.
// The particle number is taken from the states (ITensor infers it from the
// IQMPS quantum numbers), so device contexts are created on first use.
//
// OptimalControl<GpuTDMRG> drives the batched device paths through
// GpuTDMRG::Engine: psi_t / xi_t / xiHlist stay resident in HBM, and the
// Hessian rows are sharded zig-zag over the devices selected by
// setThreadCount (one context, stream and host thread per device).
#pragma once

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/ocmps.h"
#include "ControlBasis.hpp"
#include "MPS.hpp"

namespace ocmps {

namespace detail {
inline void check(int rc, const ocg_ctx* ctx, const char* what) {
  if (rc != OCG_OK) {
    const char* msg = ocg_last_error(ctx);
    throw std::runtime_error(std::string(what) + ": " + (msg ? msg : "error"));
  }
}
struct CtxDeleter {
  void operator()(ocg_ctx* c) const {
    if (c) ocg_destroy(c);
  }
};
using CtxPtr = std::unique_ptr<ocg_ctx, CtxDeleter>;

inline CtxPtr make_ctx(int dev, int L, int p, int Q, double J, double dt, const Args& a) {
  ocg_ctx* c = nullptr;
  check(ocg_create(dev, L, p, Q, J, dt, a.cutoff, a.maxm, &c), nullptr, "ocg_create");
  return CtxPtr(c);
}
inline MPS fetch_state(ocg_ctx* c, int L, int p, int Q, int which, int t) {
  ocg_info info;
  check(ocg_get_info(c, &info), c, "ocg_get_info");
  std::vector<int> dims(size_t(L + 1) * (Q + 1));
  std::vector<Cplx> data(info.mps_max_nelem);
  size_t n = 0;
  check(ocg_get_state(c, which, t, dims.data(), reinterpret_cast<double*>(data.data()), data.size(), &n), c,
        "ocg_get_state");
  data.resize(n);
  return MPS(L, p, Q, std::move(dims), std::move(data));
}
}  // namespace detail

// propagatorDeriv: the constant on-site MPO dH = sum_k 0.5 n_k (n_k - 1)
// (src/BH_tDMRG.cpp:10-14, :238-241); the control argument is ignored.
struct DerivMPO {
  int L = 0, p = 0;
  std::vector<double> onsite;  // 0.5 n (n-1), n = 0..p-1
};

class GpuTDMRG {
 public:
  class Engine;

  GpuTDMRG() = default;
  GpuTDMRG(const BoseHubbard& sites, double J_, double tstep_, const Args& args_ = Args())
      : L(sites.L), p(sites.localDim()), J(J_), tstep(tstep_), args(args_), scratch(std::make_shared<Scratch>()) {}

  void setTstep(double t) {
    tstep = t;
    scratch = std::make_shared<Scratch>();  // contexts carry dt-dependent gates
  }
  double getTstep() const { return tstep; }
  // static site potential sum_k eps_k n_k (L site energies, site 1 first; empty or all zeros: none).
  // Every context created afterwards carries it: single steps, and the shards of an
  // OptimalControl constructed from this stepper afterwards (like setTstep).
  void setPotential(std::vector<double> e) {
    if (!e.empty() && e.size() != size_t(L)) throw std::invalid_argument("setPotential: eps must have L entries");
    eps = std::move(e);
    scratch = std::make_shared<Scratch>();
  }
  std::vector<double> getPotential() const { return eps.empty() ? std::vector<double>(size_t(L), 0.0) : eps; }
  bool hasPotential() const {
    for (double e : eps)
      if (e != 0.0) return true;
    return false;
  }
  Args getArgs() const { return args; }
  DerivMPO propagatorDeriv(const double& /*control_n*/) const {
    DerivMPO m{L, p, std::vector<double>(p)};
    for (int n = 0; n < p; ++n) m.onsite[n] = 0.5 * n * (n - 1);
    return m;
  }
  // one Trotter step of psi in place (src/BH_tDMRG.cpp:111-125)
  void step(MPS& psi, double from, double to, bool propagateForward = true) const {
    ocg_ctx* c = scratch_ctx(psi.Q);
    std::vector<int> od(psi.dims.size());
    ocg_info info;
    detail::check(ocg_get_info(c, &info), c, "ocg_get_info");
    std::vector<Cplx> out(info.mps_max_nelem);
    size_t n = 0;
    detail::check(ocg_step(c, psi.dims.data(), psi.raw(), from, to, propagateForward ? 1 : 0, od.data(),
                           reinterpret_cast<double*>(out.data()), out.size(), &n),
                  c, "ocg_step");
    out.resize(n);
    psi = MPS(L, p, psi.Q, std::move(od), std::move(out));
  }
  // device used for single steps / the first shard (default 0)
  void setDevice(int dev) {
    device = dev;
    scratch = std::make_shared<Scratch>();
  }
  int getDevice() const { return device; }

  // trajectory engine owned by one OptimalControl (see OptimalControl.hpp)
  std::unique_ptr<Engine> makeEngine(const MPS& target, const MPS& init, size_t N) const;

  int sitesL() const { return L; }
  int localDim() const { return p; }
  double hopping() const { return J; }

 private:
  struct Scratch {
    std::mutex mu;
    std::map<int, detail::CtxPtr> byQ;
  };
  // a context of this stepper's chain on device dev with its site potential set
  detail::CtxPtr new_ctx(int dev, int Q) const {
    detail::CtxPtr c = detail::make_ctx(dev, L, p, Q, J, tstep, args);
    if (!eps.empty()) detail::check(ocg_set_potential(c.get(), eps.data()), c.get(), "ocg_set_potential");
    return c;
  }
  ocg_ctx* scratch_ctx(int Q) const {
    std::lock_guard<std::mutex> lk(scratch->mu);
    auto& c = scratch->byQ[Q];
    if (!c) c = new_ctx(device, Q);
    return c.get();
  }
  std::vector<double> eps;
  int L = 0, p = 0, device = 0;
  double J = 1.0, tstep = 0.01;
  Args args;
  std::shared_ptr<Scratch> scratch;  // step() is const in the reference; the context cache is shared by copies
};

// Device-resident trajectories of one OptimalControl instance.  Shard s owns
// a context on device (first + s); every shard recomputes psi_t / xi_t /
// xiHlist itself (2(N-1) steps, small next to the (N-2)(N-3)/2 row steps).
class GpuTDMRG::Engine {
 public:
  Engine(const GpuTDMRG& st, const MPS& target, const MPS& init, size_t N_)
      : stepper(st), tgt(target), ini(init), N(N_) {
    if (target.Q != init.Q || target.L != st.L || init.L != st.L || target.p != st.p || init.p != st.p)
      throw std::invalid_argument("OptimalControl: target/init states do not match the stepper's sites");
    setShards(1);
  }
  // setThreadCount: number of GPUs (shards) the Hessian rows are spread over.
  // Existing shards keep their trajectories; new shards replay the controls
  // of the current psi_t / xi_t before their first use.
  void setShards(size_t n) {
    if (n < 1) throw std::invalid_argument("Mininum threadCount is 1.");
    while (shards.size() > n) shards.pop_back();
    const size_t kept = shards.size();
    int ndev = 0;
    detail::check(ocg_device_count(&ndev), nullptr, "ocg_device_count");
    while (shards.size() < n) {
      // shard s on device (first + s) mod #devices: more shards than GPUs run
      // concurrently on separate streams of the same device
      const int dev = (stepper.device + int(shards.size())) % ndev;
      detail::CtxPtr c = stepper.new_ctx(dev, tgt.Q);  // (with the stepper's site potential)
      detail::check(ocg_set_states(c.get(), tgt.dims.data(), tgt.raw(), ini.dims.data(), ini.raw()), c.get(),
                    "ocg_set_states");
      shards.push_back(std::move(c));
    }
    // shards created by this call replay shard 0's controls before first use;
    // existing shards keep their trajectories (and their flags)
    fresh.resize(shards.size(), 1);
    xih_done.resize(shards.size(), 0);
    if (kept == 0) fresh[0] = 0;  // shard 0 is the reference copy
    for (size_t s = kept; s < shards.size(); ++s) xih_done[s] = 0;
  }
  size_t nShards() const { return shards.size(); }
  // which: 1 psi_t (calcPsi), 2 xi_t (calcXi), 3 both concurrently
  void propagate(const stdvec& u, int which) {
    check_len(u);
    on_all([&](ocg_ctx* c) { detail::check(ocg_propagate(c, u.data(), int(N), which), c, "ocg_propagate"); });
    if (which & 1) u_psi = u;
    if (which & 2) u_xi = u;
    for (size_t s = 0; s < shards.size(); ++s) xih_done[s] = 0;
  }
  std::vector<Cplx> divT() {
    std::vector<Cplx> d(N);
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_div_t(c, reinterpret_cast<double*>(d.data())), c, "ocg_div_t");
    return d;
  }
  Cplx overlapFactor() {
    double F[2];
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_overlap_factor(c, F), c, "ocg_overlap_factor");
    return Cplx(F[0], F[1]);
  }
  stdvec fidelities() {
    stdvec f(N);
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_fidelities(c, f.data()), c, "ocg_fidelities");
    return f;
  }
  void precomputeXiH() {
    replay_fresh();
    on_all([&](ocg_ctx* c) { detail::check(ocg_xi_dH(c), c, "ocg_xi_dH"); });
  }
  // calcHessianRow for rows 1..N-2 (zig-zag over shards), added into H
  void hessianRows(const stdvec& u, Cplx F, const std::vector<Cplx>& dT, rowmat& H) {
    check_len(u);
    const size_t G = shards.size();
    std::vector<std::vector<int>> rows(G);
    replay_fresh();
    for (size_t i = 1, k = 0; i + 1 < N; ++i, ++k) {
      const size_t r = k % (2 * G);
      rows[r < G ? r : 2 * G - 1 - r].push_back(int(i));
    }
    std::vector<std::vector<double>> part(G, std::vector<double>(N * N, 0.0));
    const double Fv[2] = {F.real(), F.imag()};
    on_all_indexed([&](size_t s, ocg_ctx* c) {
      if (rows[s].empty()) return;
      detail::check(ocg_hessian_rows(c, u.data(), int(N), rows[s].data(), int(rows[s].size()), Fv,
                                     reinterpret_cast<const double*>(dT.data()), part[s].data()),
                    c, "ocg_hessian_rows");
    });
    gather_rows(rows, part, H);
  }
  // getHessian(u, new_control = true) fidelity part in one pipelined call per
  // shard (ocg_hessian): trajectories, xiHlist and the shard's rows overlap
  void hessianFresh(const stdvec& u, Cplx& F, std::vector<Cplx>& dT, rowmat& H) {
    check_len(u);
    const size_t G = shards.size();
    std::vector<std::vector<int>> rows(G);
    for (size_t i = 1, k = 0; i + 1 < N; ++i, ++k) {
      const size_t r = k % (2 * G);
      rows[r < G ? r : 2 * G - 1 - r].push_back(int(i));
    }
    std::vector<std::vector<double>> part(G, std::vector<double>(N * N, 0.0));
    std::vector<double> dv(2 * N);
    double Fv[2] = {0, 0};
    on_all_indexed([&](size_t s, ocg_ctx* c) {
      std::vector<double> dvs(2 * N);
      double Fs[2];
      detail::check(ocg_hessian(c, u.data(), int(N), rows[s].data(), int(rows[s].size()), part[s].data(), dvs.data(),
                                Fs),
                    c, "ocg_hessian");
      if (s == 0) {
        dv = dvs;
        Fv[0] = Fs[0];
        Fv[1] = Fs[1];
      }
    });
    for (size_t s = 0; s < G; ++s) fresh[s] = 0;
    u_psi = u;
    u_xi = u;
    F = Cplx(Fv[0], Fv[1]);
    dT.resize(N);
    for (size_t i = 0; i < N; ++i) dT[i] = Cplx(dv[2 * i], dv[2 * i + 1]);
    gather_rows(rows, part, H);
  }
  // ControlBasis::convertHessian (src/ControlBasis.cpp:91-116) on shard 0's
  // device: bit-identical to the host restatement (ocg_convert_hessian)
  rowmat convertHessian(const ControlBasis& basis, const rowmat& Hu) {
    const rowmat& V = basis.basisMatrix();
    const size_t M = V.size(), n = Hu.size();
    if (M == 0 || n != N) return basis.convertHessian(Hu);
    std::vector<double> h(n * n), v(M * n), hc(M * M);
    for (size_t i = 0; i < n; ++i) std::copy(Hu[i].begin(), Hu[i].end(), h.begin() + i * n);
    for (size_t j = 0; j < M; ++j) std::copy(V[j].begin(), V[j].end(), v.begin() + j * n);
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_convert_hessian(c, h.data(), int(n), v.data(), int(M), hc.data()), c, "ocg_convert_hessian");
    rowmat Hc(M, stdvec(M));
    for (size_t i = 0; i < M; ++i) std::copy(hc.begin() + i * M, hc.begin() + (i + 1) * M, Hc[i].begin());
    return Hc;
  }
  // Observables of the device-resident trajectory (ocg_observe): which 0 psi_t,
  // 1 xi_t, 2 xiHlist; ts the state indices (empty: all N), rows the start
  // sites (1..L) of the correlation rows (empty: none).  Nothing but the
  // results leaves the device.
  TrajectoryObservables observe(int which = 0, const std::vector<int>& ts = {}, const std::vector<int>& rows = {}) {
    TrajectoryObservables o;
    o.L = stepper.L;
    o.p = stepper.p;
    o.ts = ts;
    if (ts.empty())
      for (size_t t = 0; t < N; ++t) o.ts.push_back(int(t));
    o.rows = rows;
    const size_t nt = o.ts.size(), nr = rows.size(), L = size_t(o.L);
    o.norm2.assign(nt, 0.0);
    o.occ.assign(nt * L * o.p, 0.0);
    o.bond.assign(nt * (L + 1), 0);
    o.ada.assign(nt * nr * L, Cplx(0, 0));
    o.nn.assign(nt * nr * L, 0.0);
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_observe(c, which, o.ts.data(), int(nt), rows.data(), int(nr), o.norm2.data(), o.occ.data(),
                              o.bond.data(), nr ? reinterpret_cast<double*>(o.ada.data()) : nullptr,
                              nr ? o.nn.data() : nullptr),
                  c, "ocg_observe");
    return o;
  }
  // Entanglement spectra of the device-resident trajectory (ocg_observe_spectrum):
  // the entropy of every bond b = 1..L-1 of the states ts (empty: all N) and,
  // with weights, the Schmidt weights and their sectors (wcap = the largest
  // bond dimension of the request).  The result carries ts, the bond dimensions
  // and the spectrum fields; the other observables are those of observe().
  TrajectoryObservables observeSpectrum(int which = 0, const std::vector<int>& ts = {}, bool weights = false) {
    TrajectoryObservables o;
    o.L = stepper.L;
    o.p = stepper.p;
    o.ts = ts;
    if (ts.empty())
      for (size_t t = 0; t < N; ++t) o.ts.push_back(int(t));
    const size_t nt = o.ts.size(), L = size_t(o.L), nb = L - 1;
    o.bond.assign(nt * (L + 1), 0);
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_observe(c, which, o.ts.data(), int(nt), nullptr, 0, nullptr, nullptr, o.bond.data(), nullptr,
                              nullptr),
                  c, "ocg_observe");
    if (weights) {
      for (int b : o.bond) o.wcap = std::max(o.wcap, b);
      o.schmidt.assign(nt * nb * o.wcap, 0.0);
      o.sector.assign(nt * nb * o.wcap, -1);
    }
    o.entropy.assign(nt * nb, 0.0);
    detail::check(ocg_observe_spectrum(c, which, o.ts.data(), int(nt), o.wcap, o.entropy.data(),
                                       weights ? o.schmidt.data() : nullptr, weights ? o.sector.data() : nullptr),
                  c, "ocg_observe_spectrum");
    return o;
  }
  // Fock-state snapshots of the device-resident trajectory (ocg_sample): nshots
  // occupation configurations of each state ts (empty: all N) drawn from
  // |<n|s>|^2 / <s|s>, with their log-probabilities.  The random numbers depend on
  // (seed, t, shot, site) alone; which is not mixed in.
  TrajectorySnapshots sample(int which, const std::vector<int>& ts, int nshots, unsigned long long seed) {
    TrajectorySnapshots o;
    o.L = stepper.L;
    o.nshots = nshots < 0 ? 0 : nshots;
    o.ts = ts;
    if (ts.empty())
      for (size_t t = 0; t < N; ++t) o.ts.push_back(int(t));
    const size_t nt = o.ts.size();
    o.configs.assign(nt * o.nshots * o.L, (signed char)-1);
    o.logps.assign(nt * o.nshots, 0.0);
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_sample(c, which, o.ts.data(), int(nt), nshots, seed, o.configs.data(), o.logps.data()), c,
                  "ocg_sample");
    return o;
  }
  // <n|s> of the configurations (nconf x L occupations, row after row) for the
  // states ts (empty: all N) of the device-resident trajectory (ocg_fock_amplitudes):
  // [e][conf], raw (not divided by the norm).
  std::vector<Cplx> fockAmplitudes(int which, const std::vector<int>& ts, const std::vector<signed char>& configs) {
    std::vector<int> tt = ts;
    if (ts.empty())
      for (size_t t = 0; t < N; ++t) tt.push_back(int(t));
    const size_t nconf = configs.size() / size_t(stepper.L);
    if (nconf * size_t(stepper.L) != configs.size())
      throw std::invalid_argument("fockAmplitudes: configs is not a multiple of L long");
    std::vector<Cplx> amp(tt.size() * nconf, Cplx(0, 0));
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_fock_amplitudes(c, which, tt.data(), int(tt.size()), configs.data(), int(nconf),
                                      reinterpret_cast<double*>(amp.data())),
                  c, "ocg_fock_amplitudes");
    return amp;
  }
  // Energy moments of the device-resident trajectory (ocg_observe_moments): norm2,
  // <K>, <D>, <K K>, <D D>, <K D> of the states ts (empty: all N), from which
  // TrajectoryMoments gives <H(J, U)> and its variance for any (J, U).
  TrajectoryMoments observeMoments(int which = 0, const std::vector<int>& ts = {}) {
    TrajectoryMoments o;
    o.ts = ts;
    if (ts.empty())
      for (size_t t = 0; t < N; ++t) o.ts.push_back(int(t));
    o.mom.assign(7 * o.ts.size(), 0.0);
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_observe_moments(c, which, o.ts.data(), int(o.ts.size()), o.mom.data()), c,
                  "ocg_observe_moments");
    return o;
  }
  // Transition matrix elements between states of the device-resident trajectories
  // (ocg_observe_pairs): pair e has the bra state tx[e] of which_x and the ket state ty[e] of
  // which_y (0 psi_t, 1 xi_t, 2 xiH_t; both empty: all N times, t with t).
  PairObservables observePairs(int which_x, const std::vector<int>& tx, int which_y, const std::vector<int>& ty) {
    PairObservables o;
    o.L = stepper.L;
    o.p = stepper.p;
    o.tx = tx;
    o.ty = ty;
    if (tx.empty() && ty.empty())
      for (size_t t = 0; t < N; ++t) {
        o.tx.push_back(int(t));
        o.ty.push_back(int(t));
      }
    if (o.tx.size() != o.ty.size()) throw std::invalid_argument("observePairs: tx and ty differ in length");
    const size_t n = o.tx.size();
    o.ovl.assign(n, Cplx(0, 0));
    o.occ.assign(n * o.L * o.p, Cplx(0, 0));
    o.hop.assign(n * 2 * (o.L - 1), Cplx(0, 0));
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_observe_pairs(c, which_x, o.tx.data(), which_y, o.ty.data(), int(n),
                                    reinterpret_cast<double*>(o.ovl.data()), reinterpret_cast<double*>(o.occ.data()),
                                    reinterpret_cast<double*>(o.hop.data())),
                  c, "ocg_observe_pairs");
    return o;
  }
  // Expectations of products of diagonal one-site operators in the states ts (empty: all N) of a
  // device-resident trajectory (ocg_observe_strings): tables[m] is L x p, row k - 1 the diagonal
  // f[n] of operator m on site k (all 1: the site is outside its support).  Returns [e][m] =
  // <s|O_m|s>, raw (not divided by the norm).
  std::vector<std::vector<Cplx>> observeStrings(int which, const std::vector<int>& ts,
                                                const std::vector<std::vector<Cplx>>& tables) {
    std::vector<int> tt = ts;
    if (ts.empty())
      for (size_t t = 0; t < N; ++t) tt.push_back(int(t));
    const size_t per = size_t(stepper.L) * stepper.p, nops = tables.size();
    std::vector<Cplx> f;
    for (const std::vector<Cplx>& t : tables) {
      if (t.size() != per) throw std::invalid_argument("observeStrings: a table is not L x p");
      f.insert(f.end(), t.begin(), t.end());
    }
    std::vector<Cplx> flat(tt.size() * nops, Cplx(0, 0));
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_observe_strings(c, which, tt.data(), int(tt.size()), reinterpret_cast<const double*>(f.data()),
                                      int(nops), reinterpret_cast<double*>(flat.data())),
                  c, "ocg_observe_strings");
    std::vector<std::vector<Cplx>> out(tt.size());
    for (size_t e = 0; e < tt.size(); ++e) out[e].assign(flat.begin() + e * nops, flat.begin() + (e + 1) * nops);
    return out;
  }
  // the chain length, the levels per site and the particle number of the trajectories
  int sites() const { return stepper.L; }
  int levels() const { return stepper.p; }
  int particles() const { return tgt.Q; }
  // a non-zero site potential is in force on every shard
  bool hasPotential() const { return stepper.hasPotential(); }
  // launches of one ocg_kernel_stats kind on shard 0 since the context was created (diagnostics: kind 0
  // counts the trajectory propagations)
  long kernelLaunches(int kind) {
    long n = 0;
    ocg_ctx* c = shards[0].get();
    detail::check(ocg_kernel_stats(c, kind, nullptr, &n, nullptr, nullptr, nullptr), c, "ocg_kernel_stats");
    return n;
  }
  std::vector<MPS> psiTrajectory() {
    std::vector<MPS> out;
    for (size_t t = 0; t < N; ++t)
      out.push_back(detail::fetch_state(shards[0].get(), stepper.L, stepper.p, tgt.Q, 0, int(t)));
    return out;
  }

 private:
  // Shard s wrote the entries (i, j >= i) of its rows and their mirrors; the
  // entry sets of different shards are disjoint, so adding only those is the
  // exact sum of the partial matrices (O(N^2) in total instead of G N^2).
  void gather_rows(const std::vector<std::vector<int>>& rows, const std::vector<std::vector<double>>& part,
                   rowmat& H) const {
    for (size_t s = 0; s < rows.size(); ++s)
      for (int i : rows[s])
        for (size_t j = size_t(i); j + 1 < N; ++j) {
          H[i][j] += part[s][size_t(i) * N + j];
          if (j > size_t(i)) H[j][i] += part[s][j * N + size_t(i)];
        }
  }
  // bring shards created after the last propagation up to shard 0's state
  void replay_fresh() {
    for (size_t s = 0; s < shards.size(); ++s) {
      if (!fresh[s]) continue;
      ocg_ctx* c = shards[s].get();
      if (!u_psi.empty()) detail::check(ocg_propagate(c, u_psi.data(), int(N), 1), c, "ocg_propagate");
      if (!u_xi.empty()) detail::check(ocg_propagate(c, u_xi.data(), int(N), 2), c, "ocg_propagate");
      fresh[s] = 0;
    }
  }
  void check_len(const stdvec& u) const {
    if (u.size() != N) throw std::invalid_argument("control has length " + std::to_string(u.size()) +
                                                   ", expected N = " + std::to_string(N));
  }
  template <class F>
  void on_all(F f) {
    on_all_indexed([&](size_t, ocg_ctx* c) { f(c); });
  }
  template <class F>
  void on_all_indexed(F f) {
    if (shards.size() == 1) { f(0, shards[0].get()); return; }
    std::vector<std::thread> th;
    std::vector<std::string> err(shards.size());
    for (size_t s = 0; s < shards.size(); ++s)
      th.emplace_back([&, s]() {
        try { f(s, shards[s].get()); } catch (const std::exception& e) { err[s] = e.what(); }
      });
    for (auto& t : th) t.join();
    for (auto& e : err)
      if (!e.empty()) throw std::runtime_error(e);
  }
  GpuTDMRG stepper;
  MPS tgt, ini;
  size_t N;
  std::vector<detail::CtxPtr> shards;
  std::vector<char> fresh, xih_done;
  stdvec u_psi, u_xi;  // controls of the current device trajectories
};

inline std::unique_ptr<GpuTDMRG::Engine> GpuTDMRG::makeEngine(const MPS& target, const MPS& init, size_t N) const {
  return std::unique_ptr<Engine>(new Engine(*this, target, init, N));
}

}  // namespace ocmps
