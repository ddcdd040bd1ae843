// The front end of the device-side observables, once for both engines: the argument checks, the
// chunking of a request against the workspace budget, the staging of caller-supplied states and the
// bodies of the ocg_observe* / ocg_sample* / ocg_fock_amplitudes* entry points (include/ocmps.h).
// Failures leave as obs::Error; the entry points of ocmps.hip and hbm.hip turn them into a status.
//
// An engine is seen through an adapter A:
//   int L, p, Q;  int N() const;  hipStream_t stream() const;
//   bool have(int which) const;  int base(int which) const;    a trajectory is stored / its first slot
//   void describe(slots, out0, bond, desc);   the block descriptors of state slots (and, with bond, the
//                                             bond dimensions into entry out0 + i of it)
//   void chunk(bytes, mid);   workspace of `bytes`, the kind-9 timing and statistics around mid(run) and the
//                             sync behind it; run.be is the backend of obs::run_chunk, run.tr the traffic
//                             it counts into, run.note(hipError_t) takes the status of a queued copy and
//                             run.ok() says whether to queue more
//   auto stage(n, what);      a device buffer .p of n complex elements for the call `what`; its destructor
//                             drains the stream and frees it
#pragma once

#include "observe.hpp"

namespace obs {

// ------------------------------------------------------------------ argument checks
template <class A>
void observe_check_rows(const A& a, const int* rows, int nrows) {
  if (nrows < 0 || (nrows > 0 && !rows)) throw Error(1, "bad rows");
  for (int i = 0; i < nrows; ++i)
    if (rows[i] < 1 || rows[i] > a.L) throw Error(1, "row (start site) out of 1..L");
}

// n caller-supplied states and the pointers that must come with them
inline void check_given(int n, bool pointers) {
  if (n < 0 || (n > 0 && !pointers)) throw Error(1, "bad argument");
}

// the dims of caller-supplied states, before anything is written (wcap >= 0: the
// bond dimensions must fit it)
template <class A>
void staged_check(const A& a, int n, const int* dims, int wcap) {
  const int Q1 = a.Q + 1, nsq = (a.L + 1) * Q1;
  for (int i = 0; i < n; ++i) {
    const int* d = dims + size_t(i) * nsq;
    for (int j = 0; j < nsq; ++j)
      if (d[j] < 0) throw Error(1, "negative bond dimension");
    for (int q = 0; q < Q1; ++q)
      if (d[q] != (q == 0 ? 1 : 0) || d[a.L * Q1 + q] != (q == a.Q ? 1 : 0))
        throw Error(1, "bond 0 / bond L must be one state with q = 0 / q = Q");
    for (int b = 1; b < a.L && wcap >= 0; ++b) {
      long sum = 0;
      for (int q = 0; q < Q1; ++q) sum += d[size_t(b) * Q1 + q];
      if (sum > wcap) throw Error(2, "wcap below the largest bond dimension of the states");
    }
  }
}

// every configuration has entries in 0..p-1 that add up to Q
template <class A>
void check_configs(const A& a, const signed char* configs, int nconf, double* amp) {
  if (nconf < 0 || (nconf > 0 && (!configs || !amp))) throw Error(1, "bad configurations / outputs");
  for (int j = 0; j < nconf; ++j) {
    int sum = 0;
    for (int k = 0; k < a.L; ++k) {
      const int v = configs[size_t(j) * a.L + k];
      if (v < 0 || v >= a.p) throw Error(1, "a configuration entry outside 0..p-1");
      sum += v;
    }
    if (sum != a.Q) throw Error(1, "a configuration that does not hold Q particles");
  }
}

// the operators of a string request (f[nops][L][p][2], all finite) with their supports
template <class A>
void string_request(const A& a, const double* f, int nops, Strings& sr) {
  if (nops < 0 || (nops > 0 && !f)) throw Error(1, "bad operator tables");
  const size_t nf = 2 * size_t(nops) * a.L * a.p;
  for (size_t j = 0; j < nf; ++j)
    if (!std::isfinite(f[j])) throw Error(1, "a table entry is not finite");
  sr.nops = nops;
  sr.f = f;
  sr.prepare(a.L, a.p);
}

// a request names a stored trajectory (which 0 psi_t, 1 xi_t, 2 xiH_t)
template <class A>
void check_trajectory(const A& a, int which, int nt) {
  if (which < 0 || which > 2 || nt < 0) throw Error(1, "bad which / count");
  if (!a.have(which)) throw Error(4, "requested trajectory not available");
}
// the slots of its times ts (null: 0..nt-1), and with ids the times themselves
template <class A>
std::vector<int> time_slots(const A& a, int which, const int* ts, int nt,
                            std::vector<unsigned long long>* ids = nullptr) {
  std::vector<int> slots(nt);
  if (ids) ids->resize(nt);
  for (int i = 0; i < nt; ++i) {
    const int t = ts ? ts[i] : i;
    if (t < 0 || t >= a.N()) throw Error(1, "t out of range");
    slots[i] = a.base(which) + t;
    if (ids) (*ids)[i] = (unsigned long long)t;
  }
  return slots;
}
// the trajectory slots of a request (which / ts as ocg_observe)
template <class A>
std::vector<int> trajectory_slots(const A& a, int which, const int* ts, int nt,
                                  std::vector<unsigned long long>* ids = nullptr) {
  check_trajectory(a, which, nt);
  return time_slots(a, which, ts, nt, ids);
}

// ------------------------------------------------------------------ requests
template <class A>
Outputs no_outputs(const A& a) {
  return Outputs{nullptr, nullptr, nullptr, nullptr, a.L, a.p, 0, nullptr};
}
inline Snap draw_request(int nshots, unsigned long long seed, const unsigned long long* ids, signed char* config,
                         double* logp) {
  Snap sn;
  sn.nper = nshots;
  sn.seed = seed;
  sn.ids = ids;
  sn.config = config;
  sn.val = logp;
  return sn;
}
inline Snap amplitude_request(const signed char* configs, int nconf, double* amp) {
  Snap sn;
  sn.nper = nconf;
  sn.given = configs;
  sn.val = amp;
  return sn;
}

// zero the row outputs (entries j < i stay 0) and pick the occupation buffer
inline double* observe_prepare(const Outputs& o, size_t n, std::vector<double>& tmp) {
  if (o.ada) std::fill(o.ada, o.ada + 2 * n * o.nrows * o.L, 0.0);
  if (o.nn) std::fill(o.nn, o.nn + n * o.nrows * o.L, 0.0);
  if (o.occ || !want_of(o).occ) return o.occ;
  tmp.assign(n * o.L * o.p, 0.0);
  return tmp.data();
}

// ------------------------------------------------------------------ chunks
// The chunks of observe.hpp's driver over states described on the device (with kets: over the pairs
// bra desc[i], ket (*kets)[i]), each of at most chunk_budget() bytes of workspace, results into entry
// out0 + i of the outputs.  With so the spectrum stages run too and their results go to *so; with sn
// the snapshot launch follows the right sweep instead and its results go to sn's outputs.
template <class A>
void observe_descs(A& a, const std::vector<StateDesc>& desc, size_t out0, const Outputs& o, double* occ_buf,
                   const SpecOutputs* so = nullptr, Snap* sn = nullptr,
                   const std::vector<StateDesc>* kets = nullptr) {
  const int L = a.L, Q1 = a.Q + 1, nst = int(desc.size());
  Want want = want_of(o);
  want.spec = so != nullptr;
  if (!want.norm && !want.env() && !want.spec && !want.mom && !want.pair && !want.str && !sn) return;
  int wb = 0, wo = 0;
  for (int i = 0; i < nst; ++i) {
    widest(desc[i], L, Q1, wb, wo);
    if (kets) widest((*kets)[i], L, Q1, wb, wo);
  }
  if (want.str && wo > kStringMaxOrder) throw Error(2, "strings: a bond sector above order 512");
  if (sn && wo > kSampleMaxOrder) throw Error(2, "snapshots: a bond sector above order 512");
  if (want.pair && wo > kPairMaxOrder) throw Error(2, "pairs: a bond sector above order 512");
  if (want.mom && wo > kEnergyMaxOrder) throw Error(2, "moments: a bond sector above order 512");
  if (so) {
    if (so->weights() && so->wcap < wb)
      throw Error(2, "wcap " + std::to_string(so->wcap) + " below the largest bond dimension " + std::to_string(wb));
    if (wo > kEigMaxOrder) throw Error(2, "spectrum: a bond sector above order 512");
  }
  const std::vector<int> rows(o.rows, o.rows + o.nrows);
  const std::vector<size_t> need = workspace_needs(L, a.p, a.Q, desc, rows, want, sn, kets);
  const size_t budget = chunk_budget();
  for (int i0 = 0; i0 < nst;) {
    int i1 = i0;
    size_t sum = 0;
    while (i1 < nst && (i1 == i0 || sum + need[i1] <= budget)) sum += need[i1++];
    if ((sn || want.mom || want.pair || want.str) && sum > budget)  // (the older calls leave a single state above the budget to the allocation)
      throw Error(6, std::string(sn ? "snapshots" : want.pair ? "pairs" : want.str ? "strings" : "moments") +
                         ": the workspace of one " + (want.pair ? "pair" : "state") + " (" + std::to_string(sum) +
                         " B) exceeds the chunk budget");
    std::vector<const StateDesc*> S, SY;
    std::vector<size_t> os;
    for (int i = i0; i < i1; ++i) {
      S.push_back(&desc[i]);
      if (kets) SY.push_back(&(*kets)[i]);
      os.push_back(out0 + i);
    }
    std::vector<Dest> dests;
    std::vector<double> res, ent, wts;
    std::vector<int> status;
    Spec sp;
    a.chunk(sum, [&](auto& run) {
      const double* d_out = run_chunk(run.be, L, a.p, a.Q, S, os, rows, want, dests, run.tr, so ? &sp : nullptr, sn,
                                      kets ? &SY : nullptr);
      if (sn && run.ok()) run.note(sn->fetch(out0 + i0, S.size(), L, a.stream()));
      res.resize(2 * std::max<size_t>(dests.size(), 1));
      if (run.ok() && !dests.empty())
        run.note(hipMemcpyAsync(res.data(), d_out, sizeof(double) * 2 * dests.size(), hipMemcpyDeviceToHost,
                                a.stream()));
      if (so && run.ok()) {  // only results leave the device: the weights when they are asked for
        ent.resize(std::max<size_t>(S.size() * (L - 1), 1));
        status.resize(std::max<size_t>(sp.nstatus, 1));
        wts.resize(so->weights() ? std::max<size_t>(sp.nw, 1) : 0);
        if (L > 1)
          run.note(hipMemcpyAsync(ent.data(), sp.d_ent, sizeof(double) * S.size() * (L - 1), hipMemcpyDeviceToHost,
                                  a.stream()));
        if (sp.nstatus)
          run.note(hipMemcpyAsync(status.data(), sp.d_status, sizeof(int) * sp.nstatus, hipMemcpyDeviceToHost,
                                  a.stream()));
        if (so->weights() && sp.nw)
          run.note(hipMemcpyAsync(wts.data(), sp.d_w, sizeof(double) * sp.nw, hipMemcpyDeviceToHost, a.stream()));
      }
    });
    if (so) {
      for (size_t j = 0; j < sp.nstatus; ++j)
        if (status[j]) throw Error(5, "spectrum: a Jacobi eigen block did not converge");
      scatter_spectrum(sp, S, os, L, Q1, ent.data(), wts.data(), *so);
    }
    scatter(dests, res.data(), o, occ_buf);
    if (o.nrows > 0 && (o.ada || o.nn))
      for (int i = i0; i < i1; ++i) diagonals(out0 + i, o, occ_buf);
    i0 = i1;
  }
}

// the same over state slots of the engine
template <class A>
void observe_slots(A& a, const std::vector<int>& slots, size_t out0, const Outputs& o, int* bond, double* occ_buf,
                   const SpecOutputs* so = nullptr, Snap* sn = nullptr) {
  std::vector<StateDesc> desc;
  a.describe(slots, out0, bond, desc);
  observe_descs(a, desc, out0, o, occ_buf, so, sn);
}

// Caller-supplied states staged a batch at a time in the compact interchange format
// itself: its blocks are the contiguous row-major matrices the descriptors want, and a
// sector may be larger than the bound of the engine's state slots (a padded or
// over-parametrised state).
// With dims_y / data_y the states are the bras of pairs and those the kets, staged behind them.
template <class A>
void observe_staged(A& a, int n, const int* dims, const double* const* data, const Outputs& o, const SpecOutputs* so,
                    Snap* sn, const char* what, const int* dims_y = nullptr, const double* const* data_y = nullptr) {
  const int nsq = (a.L + 1) * (a.Q + 1);
  const int B = std::min(n, 64);
  for (int i0 = 0; i0 < n; i0 += B) {
    const int nb0 = std::min(B, n - i0), nb = dims_y ? 2 * nb0 : nb0;
    // entry i of the batch: state i0 + i, or for i >= nb0 the ket i0 + i - nb0
    auto dims_of = [&](int i) { return i < nb0 ? dims + size_t(i0 + i) * nsq : dims_y + size_t(i0 + i - nb0) * nsq; };
    auto data_of = [&](int i) { return i < nb0 ? data[i0 + i] : data_y[i0 + i - nb0]; };
    std::vector<StateDesc> desc(nb);
    std::vector<size_t> at(nb + 1, 0);
    for (int i = 0; i < nb; ++i) at[i + 1] = at[i] + compact_desc(a.L, a.p, a.Q, dims_of(i), nullptr, desc[i]);
    auto stage = a.stage(std::max<size_t>(at[nb], 1), what);
    for (int i = 0; i < nb; ++i) {
      if (at[i + 1] > at[i]) {
        const hipError_t e = hipMemcpyAsync(stage.p + 2 * at[i], data_of(i), 16 * (at[i + 1] - at[i]),
                                            hipMemcpyHostToDevice, a.stream());
        if (e != hipSuccess) throw Error(3, std::string(what) + ": " + hipGetErrorString(e));
      }
      compact_desc(a.L, a.p, a.Q, dims_of(i), stage.p + 2 * at[i], desc[i]);
    }
    std::vector<StateDesc> kets;
    if (dims_y) {
      kets.assign(desc.begin() + nb0, desc.end());
      desc.resize(nb0);
    }
    observe_descs(a, desc, size_t(i0), o, nullptr, so, sn, dims_y ? &kets : nullptr);
  }
}

// ------------------------------------------------------------------ entry points
// (ocg_observe_states stages through the engine's own state slots and stays with the engines)
template <class A>
void observe(A& a, int which, const int* ts, int nt, const int* rows, int nrows, double* norm2, double* occ, int* bond,
             double* ada, double* nn) {
  check_trajectory(a, which, nt);
  observe_check_rows(a, rows, nrows);
  const std::vector<int> slots = time_slots(a, which, ts, nt);
  if (nt == 0) return;
  const Outputs o{norm2, occ, ada, nn, a.L, a.p, nrows, rows};
  std::vector<double> tmp;
  double* occ_buf = observe_prepare(o, size_t(nt), tmp);
  observe_slots(a, slots, 0, o, bond, occ_buf);
}

template <class A>
void observe_spectrum(A& a, int which, const int* ts, int nt, int wcap, double* entropy, double* schmidt,
                      int* sector) {
  const std::vector<int> slots = trajectory_slots(a, which, ts, nt);
  if (nt == 0 || (!entropy && !schmidt && !sector)) return;
  const SpecOutputs so{entropy, schmidt, sector, wcap};
  observe_slots(a, slots, 0, no_outputs(a), nullptr, nullptr, &so);
}

template <class A>
void observe_spectrum_states(A& a, int n, const int* dims, const double* const* data, int wcap, double* entropy,
                             double* schmidt, int* sector) {
  check_given(n, dims && data);
  if (n == 0 || (!entropy && !schmidt && !sector)) return;
  const SpecOutputs so{entropy, schmidt, sector, wcap};
  staged_check(a, n, dims, so.weights() ? std::max(wcap, 0) : -1);
  observe_staged(a, n, dims, data, no_outputs(a), &so, nullptr, "spectrum");
}

template <class A>
void sample(A& a, int which, const int* ts, int nt, int nshots, unsigned long long seed, signed char* config,
            double* logp) {
  if (nshots < 0 || (nshots > 0 && nt > 0 && !config)) throw Error(1, "bad shots / outputs");
  std::vector<unsigned long long> ids;
  const std::vector<int> slots = trajectory_slots(a, which, ts, nt, &ids);
  if (nt == 0 || nshots == 0) return;
  Snap sn = draw_request(nshots, seed, ids.data(), config, logp);
  observe_slots(a, slots, 0, no_outputs(a), nullptr, nullptr, nullptr, &sn);
}

template <class A>
void sample_states(A& a, int n, const int* dims, const double* const* data, int nshots, unsigned long long seed,
                   signed char* config, double* logp) {
  check_given(n, dims && data);
  if (nshots < 0 || (nshots > 0 && n > 0 && !config)) throw Error(1, "bad shots / outputs");
  if (n == 0 || nshots == 0) return;
  staged_check(a, n, dims, -1);
  std::vector<unsigned long long> ids(n);
  for (int i = 0; i < n; ++i) ids[i] = (unsigned long long)i;
  Snap sn = draw_request(nshots, seed, ids.data(), config, logp);
  observe_staged(a, n, dims, data, no_outputs(a), nullptr, &sn, "snapshots");
}

template <class A>
void fock_amplitudes(A& a, int which, const int* ts, int nt, const signed char* configs, int nconf, double* amp) {
  const std::vector<int> slots = trajectory_slots(a, which, ts, nt);
  check_configs(a, configs, nconf, amp);
  if (nt == 0 || nconf == 0) return;
  Snap sn = amplitude_request(configs, nconf, amp);
  observe_slots(a, slots, 0, no_outputs(a), nullptr, nullptr, nullptr, &sn);
}

template <class A>
void fock_amplitudes_states(A& a, int n, const int* dims, const double* const* data, const signed char* configs,
                            int nconf, double* amp) {
  check_given(n, dims && data);
  check_configs(a, configs, nconf, amp);
  if (n == 0 || nconf == 0) return;
  staged_check(a, n, dims, -1);
  Snap sn = amplitude_request(configs, nconf, amp);
  observe_staged(a, n, dims, data, no_outputs(a), nullptr, &sn, "amplitudes");
}

template <class A>
void observe_moments(A& a, int which, const int* ts, int nt, double* mom) {
  const std::vector<int> slots = trajectory_slots(a, which, ts, nt);
  if (nt == 0) return;
  if (!mom) throw Error(1, "bad output");
  Outputs o = no_outputs(a);
  o.mom = mom;
  observe_slots(a, slots, 0, o, nullptr, nullptr);
}

template <class A>
void observe_moments_states(A& a, int n, const int* dims, const double* const* data, double* mom) {
  check_given(n, dims && data && mom);
  if (n == 0) return;
  staged_check(a, n, dims, -1);
  Outputs o = no_outputs(a);
  o.mom = mom;
  observe_staged(a, n, dims, data, o, nullptr, nullptr, "moments");
}

template <class A>
void observe_pairs(A& a, int which_x, const int* tx, int which_y, const int* ty, int npairs, double* ovl, double* occ,
                   double* hop) {
  const std::vector<int> sx = trajectory_slots(a, which_x, tx, npairs);
  const std::vector<int> sy = trajectory_slots(a, which_y, ty, npairs);
  if (npairs == 0 || (!ovl && !occ && !hop)) return;
  Outputs o = no_outputs(a);
  o.povl = ovl;
  o.pocc = occ;
  o.phop = hop;
  std::vector<StateDesc> dx, dy;
  a.describe(sx, 0, nullptr, dx);
  a.describe(sy, 0, nullptr, dy);
  observe_descs(a, dx, 0, o, nullptr, nullptr, nullptr, &dy);
}

template <class A>
void observe_pairs_states(A& a, int n, const int* dims_x, const double* const* x, const int* dims_y,
                          const double* const* y, double* ovl, double* occ, double* hop) {
  check_given(n, dims_x && x && dims_y && y);
  if (n == 0 || (!ovl && !occ && !hop)) return;
  staged_check(a, n, dims_x, -1);
  staged_check(a, n, dims_y, -1);
  Outputs o = no_outputs(a);
  o.povl = ovl;
  o.pocc = occ;
  o.phop = hop;
  observe_staged(a, n, dims_x, x, o, nullptr, nullptr, "pairs", dims_y, y);
}

template <class A>
void observe_strings(A& a, int which, const int* ts, int nt, const double* f, int nops, double* out) {
  const std::vector<int> slots = trajectory_slots(a, which, ts, nt);
  Strings sr;
  string_request(a, f, nops, sr);
  if (nt == 0 || nops == 0) return;
  if (!out) throw Error(1, "bad output");
  Outputs o = no_outputs(a);
  o.str = &sr;
  o.sout = out;
  observe_slots(a, slots, 0, o, nullptr, nullptr);
}

template <class A>
void observe_strings_states(A& a, int n, const int* dims, const double* const* data, const double* f, int nops,
                            double* out) {
  check_given(n, dims && data);
  Strings sr;
  string_request(a, f, nops, sr);
  if (n == 0 || nops == 0) return;
  if (!out) throw Error(1, "bad output");
  staged_check(a, n, dims, -1);
  Outputs o = no_outputs(a);
  o.str = &sr;
  o.sout = out;
  observe_staged(a, n, dims, data, o, nullptr, nullptr, "strings");
}

}  // namespace obs
