// Device-side observables of stored MPS (ocg_observe / ocg_observe_states):
// norm, occupation distribution per site and correlation rows <a+_i a_j>,
// <n_i n_j> from a start site, for a chunk of states in one set of launches.
//
// Both engines describe a state by its compact U(1) blocks: block (q, n) of
// site k is a contiguous row-major dims[k-1][q] x dims[k][q+n] complex matrix
// (DESIGN.md §4), so one host driver (run_chunk) builds the task lists from
// (pointer, rows, cols) descriptors and a backend launches them:
//   * a right sweep stores Renv_k for every bond,
//   * a left sweep carries Lenv and the open correlation environments C (bra
//     one sector above the ket) and N, and closes every site as it is reached.
// A site round is three launches for the whole chunk: the products E·A and
// A·Renv^H, the new environments sum_n A^H·(E·A), and the closes
// sum conj(X)∘Y.  Every dependency is a kernel boundary on one stream.
//
// With Want::mom the chunk runs observe_energy.hpp's moment sweep instead
// (ocg_observe_moments).
//
// With Want::pair the chunk is a list of (bra, ket) pairs and runs observe_pair.hpp's
// transition sweeps (ocg_observe_pairs).
//
// With Want::str the chunk runs observe_string.hpp's string-operator sweeps (ocg_observe_strings).
//
// With a Spec the spectrum stages follow the sweeps (ocg_observe_spectrum):
// the Schmidt weights and entropies of every bond from Lenv_b and Renv_b on
// observe_eig.hpp's batched Jacobi eigensolver (see run_chunk).
//
// Determinism: an output element is computed by one wave (GEMM tile) or one
// workgroup (close) from that state's operands alone, in an order fixed by the
// block shapes: results do not depend on what else is in the chunk.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "observe_eig.hpp"
#include "observe_sample.hpp"

namespace obs {

// a failed call: a status code of include/ocmps.h (OCG_EINVAL = 1 .. OCG_ENOMEM = 6) and its message
struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

struct Blk {
  const double* p = nullptr;  // interleaved (re, im); null: block absent
  int r = 0, c = 0;
};
// one state: bond-sector dims and the device address of every block
struct StateDesc {
  std::vector<int> dims;  // (L+1) * Q1
  std::vector<Blk> blk;   // [(k * Q1 + q) * p + n], k = 1..L
};

// alpha * op(A)[m x k] * op(B)[k x n]; ops bit 0: A conj-transposed, bit 1: B
struct Seg {
  const double* A;
  const double* B;
  int lda, ldb, k, ops;
  double alpha;
};
// C[m x n] (ld ldc) = sum of its segments (none: C = 0)
struct Task {
  double* C;
  int ldc, m, n, seg0, nseg, tile0;
};
// w * sum_e conj(X[e]) * Y[e] over n complex elements
struct Pair {
  const double* X;
  const double* Y;
  long long n;
  double w;
};
// out[task] = sum of its pairs, in list order
struct CTask {
  int pair0, npair;
};

struct Want {
  bool norm = false, occ = false, ada = false, nn = false;
  bool spec = false;  // Schmidt weights and entropies of every bond (run_chunk's Spec argument)
  bool mom = false;   // the energy moments alone (observe_energy.hpp)
  bool pair = false, pair_occ = false, pair_hop = false;  // transition elements of pairs alone (observe_pair.hpp)
  const struct Strings* str = nullptr;                    // string-operator expectations alone (observe_string.hpp)
  bool env() const { return occ || ada || nn; }
};
// the spectrum results of one chunk (device addresses, valid until the chunk's sync)
struct Spec {
  double* d_ent = nullptr;   // [state][L-1] entropies
  double* d_w = nullptr;     // per state and bond b = 1..L-1 its bond[b] weights, sector after sector
  int* d_status = nullptr;   // one word per eigen block, nonzero: not converged
  size_t nw = 0, nstatus = 0;
  std::vector<size_t> woff;  // [state * (L-1) + b-1]: where bond b's weights start in d_w
};
// a snapshot request (ocg_sample: draw nper shots per state; ocg_fock_amplitudes: the
// amplitudes of the nper given configurations) and the results of one chunk
struct Snap {
  int nper = 0;
  bool amp() const { return given != nullptr; }
  // queue the copies of a chunk's results (states out0..out0+nst of the request) to the host
  hipError_t fetch(size_t out0, size_t nst, int L, hipStream_t st) const {
    const size_t items = nst * nper, at = out0 * nper;
    hipError_t e = hipSuccess;
    if (!amp() && items)
      e = hipMemcpyAsync(config + at * L, d_config, items * L, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && val && items)
      e = hipMemcpyAsync(val + at * (amp() ? 2 : 1), d_val, sizeof(double) * items * (amp() ? 2 : 1),
                         hipMemcpyDeviceToHost, st);
    return e;
  }
  unsigned long long seed = 0;
  const unsigned long long* ids = nullptr;  // [out slot]: the id mixed into a state's random numbers
  const signed char* given = nullptr;       // host [nper][L]: amplitude mode (no right sweep)
  signed char* config = nullptr;            // host outputs by out slot: [nper][L] each (draw mode),
  double* val = nullptr;                    // logp [nper] (may be null) or amplitudes [nper][2] each
  signed char* d_config = nullptr;          // device [state][nper][L] (draw mode)
  double* d_val = nullptr;                  // device: logp [state][nper], or amplitudes [state][nper][2]
};
// where a close result goes: kind 0 norm2, 1 occ, 2 ada (complex), 3 nn, 4 a real moment, 5 <K D> (complex),
// 6 / 7 / 8 a pair's ovl / occ / hop (complex), 9 a string-operator expectation (complex)
struct Dest {
  int kind;
  size_t idx;
};
struct Traffic {
  double bytes = 0, flops = 0;
  long launches = 0;
};

}  // namespace obs

#include "observe_energy.hpp"
#include "observe_pair.hpp"
#include "observe_string.hpp"

namespace obs {

// ------------------------------------------------------------------ kernels
namespace {

constexpr int kGemmTile = 16;
constexpr int kCloseNT = 256;

typedef double obs_d4 __attribute__((ext_vector_type(4)));

// One wave = one 16x16 tile of one task, operands straight from global memory
// (the LDS engine's blocks are a few dozen rows: they live in L2), k in steps
// of 4 on v_mfma_f64_16x16x4f64: lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15]; results col = l & 15, row = (l >> 4) + 4 r.
__global__ __launch_bounds__(64) void k_obs_gemm(const Task* __restrict__ tasks, const int* __restrict__ tile_task,
                                                 const Seg* __restrict__ segs) {
  const int lane = threadIdx.x;
  const Task T = tasks[tile_task[blockIdx.x]];
  const int tl = int(blockIdx.x) - T.tile0;
  const int ntn = (T.n + kGemmTile - 1) / kGemmTile;
  const int m0 = (tl / ntn) * kGemmTile, n0 = (tl % ntn) * kGemmTile;
  const int ar = m0 + (lane & 15), bc = n0 + (lane & 15), kl = lane >> 4;
  obs_d4 cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
  for (int s = 0; s < T.nseg; ++s) {
    const Seg S = segs[T.seg0 + s];
    const bool ca = S.ops & 1, cb = (S.ops >> 1) & 1;
    for (int k0 = 0; k0 < S.k; k0 += 4) {
      const int kk = k0 + kl;
      double are = 0, aim = 0, bre = 0, bim = 0;
      if (kk < S.k && ar < T.m) {
        const double* a = S.A + 2 * (ca ? size_t(kk) * S.lda + ar : size_t(ar) * S.lda + kk);
        are = a[0] * S.alpha;
        aim = (ca ? -a[1] : a[1]) * S.alpha;
      }
      if (kk < S.k && bc < T.n) {
        const double* b = S.B + 2 * (cb ? size_t(bc) * S.ldb + kk : size_t(kk) * S.ldb + bc);
        bre = b[0];
        bim = cb ? -b[1] : b[1];
      }
      cr = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bre, cr, 0, 0, 0);
      cr = __builtin_amdgcn_mfma_f64_16x16x4f64(-aim, bim, cr, 0, 0, 0);
      ci = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bim, ci, 0, 0, 0);
      ci = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, bre, ci, 0, 0, 0);
    }
  }
  if (bc >= T.n) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = m0 + kl + 4 * r;
    if (row < T.m) {
      double* c = T.C + 2 * (size_t(row) * T.ldc + bc);
      c[0] = cr[r];
      c[1] = ci[r];
    }
  }
}

// One workgroup = one output: its pairs in list order, each thread a fixed
// stride of the elements, then a shuffle tree per wave and the four wave sums
// added in wave order.  No atomics: the order depends on the shapes alone.
__global__ __launch_bounds__(kCloseNT) void k_obs_close(const CTask* __restrict__ tasks,
                                                        const Pair* __restrict__ pairs, double* __restrict__ out) {
  __shared__ double red[2 * (kCloseNT / 64)];
  const int tid = threadIdx.x;
  const CTask T = tasks[blockIdx.x];
  double re = 0, im = 0;
  for (int i = 0; i < T.npair; ++i) {
    const Pair P = pairs[T.pair0 + i];
    double pr = 0, pi = 0;
    for (long long e = tid; e < P.n; e += kCloseNT) {
      const double xr = P.X[2 * e], xi = P.X[2 * e + 1], yr = P.Y[2 * e], yi = P.Y[2 * e + 1];
      pr += xr * yr + xi * yi;
      pi += xr * yi - xi * yr;
    }
    re += P.w * pr;
    im += P.w * pi;
  }
  for (int o = 32; o > 0; o >>= 1) {
    re += __shfl_down(re, o, 64);
    im += __shfl_down(im, o, 64);
  }
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = re;
    red[2 * (tid >> 6) + 1] = im;
  }
  __syncthreads();
  if (tid == 0) {
    double sr = 0, si = 0;
    for (int w = 0; w < kCloseNT / 64; ++w) {
      sr += red[2 * w];
      si += red[2 * w + 1];
    }
    out[2 * size_t(blockIdx.x)] = sr;
    out[2 * size_t(blockIdx.x) + 1] = si;
  }
}

}  // namespace

// ------------------------------------------------------------------ backends
// A backend provides:
//   double* alloc(size_t ncomplex)        chunk workspace (valid until the chunk's sync)
//   const double* one()                   a device complex 1
//   void gemm(std::vector<Task>&, std::vector<Seg>&)
//   void close(std::vector<CTask>&, std::vector<Pair>&, double* out)
//   int eig(std::vector<ETask>&, int* status)     one eigen stage; returns its launches
//   void entropy(std::vector<STask>&, double* out)
//   void sample(SampleTable&, const SArgs&)          the snapshot launch of the chunk
//   void energy(EnergyTable&, const EArgs&, std::vector<double>& coef)   the moment chain launch
//   void pair(PairTable&, const PArgs&)              the pair chain launch
//   const double* consts(std::vector<double>&)       doubles placed on the device (valid until the chunk's sync)
//   void string(StringTable&, const StrArgs&)        the two string chain launches

// dry run: the workspace a chunk would take (256-byte granules, as the arenas)
struct CountBackend {
  size_t bytes = 0;
  static size_t al(size_t b) { return (b + 255) & ~size_t(255); }
  double* alloc(size_t n) {
    bytes += al(16 * (n ? n : 1));
    return reinterpret_cast<double*>(size_t(256));  // never dereferenced
  }
  const double* one() { return alloc(1); }
  void gemm(std::vector<Task>& t, std::vector<Seg>& s) {
    size_t tiles = 0;
    for (auto& x : t) tiles += size_t((x.m + kGemmTile - 1) / kGemmTile) * ((x.n + kGemmTile - 1) / kGemmTile);
    bytes += al(sizeof(Task) * t.size()) + al(sizeof(Seg) * s.size()) + al(sizeof(int) * 2 * tiles);
    t.clear();
    s.clear();
  }
  void close(std::vector<CTask>& t, std::vector<Pair>& p, double*) {
    bytes += al(sizeof(CTask) * t.size()) + al(sizeof(Pair) * p.size());
    t.clear();
    p.clear();
  }
  int eig(std::vector<ETask>& t, int*) {
    std::vector<ETask> g[2];
    eig_split(t, g[0], g[1]);
    for (auto& x : g)
      if (!x.empty()) bytes += al(sizeof(ETask) * x.size());
    t.clear();
    return int(!g[0].empty()) + int(!g[1].empty());
  }
  void entropy(std::vector<STask>& t, double*) {
    bytes += al(sizeof(STask) * t.size());
    t.clear();
  }
  void sample(SampleTable& tb, const SArgs&) {
    bytes += al(sizeof(SBlk) * tb.blk.size()) + al(sizeof(double*) * tb.renv.size()) +
             al(sizeof(SState) * tb.st.size()) + al(tb.given.size());
  }
  void energy(EnergyTable& tb, const EArgs&, std::vector<double>& coef) {
    bytes += al(sizeof(EBlk) * tb.blk.size()) + al(sizeof(int) * tb.dims.size()) + al(sizeof(double) * coef.size());
  }
  void pair(PairTable& tb, const PArgs&) { bytes += al(sizeof(EBlk) * tb.blk.size()) + al(sizeof(int) * tb.dims.size()); }
  const double* consts(std::vector<double>& v) {
    bytes += al(sizeof(double) * v.size());
    return reinterpret_cast<const double*>(size_t(256));
  }
  void string(StringTable& tb, const StrArgs&) {
    bytes += al(sizeof(EBlk) * tb.blk.size()) + al(sizeof(int) * tb.dims.size()) + al(sizeof(double) * tb.f.size()) +
             al(sizeof(int) * tb.sup.size());
  }
};

// everything in one raw device buffer on one stream (the LDS engine's context)
struct RawBackend {
  char* base = nullptr;
  size_t cap = 0, top = 0;
  hipStream_t st = nullptr;
  hipError_t err = hipSuccess;
  bool overflow = false;
  std::vector<std::shared_ptr<void>> keep;  // the host side of queued uploads, until the chunk's sync
  char* raw(size_t bytes) {
    bytes = CountBackend::al(bytes ? bytes : 1);
    if (top + bytes > cap) {
      overflow = true;
      return nullptr;
    }
    char* r = base + top;
    top += bytes;
    return r;
  }
  double* alloc(size_t n) { return reinterpret_cast<double*>(raw(16 * (n ? n : 1))); }
  // takes the vector (left empty): the copy is queued from its storage
  template <class T>
  const T* upload(std::vector<T>& v) {
    char* d = raw(sizeof(T) * v.size());
    if (!d || v.empty()) return reinterpret_cast<const T*>(d);
    auto h = std::make_shared<std::vector<T>>(std::move(v));
    v.clear();
    keep.push_back(h);
    // in pieces: one copy of a large pageable list takes the runtime tens of milliseconds of host time
    // (measured: a flat 28 ms once the task lists of a launch pass roughly 0.6 MiB), pieces of this size do not
    const size_t bytes = sizeof(T) * h->size(), piece = size_t(256) << 10;
    for (size_t o = 0; o < bytes; o += piece)
      note(hipMemcpyAsync(d + o, reinterpret_cast<const char*>(h->data()) + o, std::min(piece, bytes - o),
                          hipMemcpyHostToDevice, st));
    return reinterpret_cast<const T*>(d);
  }
  void note(hipError_t e) {
    if (err == hipSuccess && e != hipSuccess) err = e;
  }
  bool ok() const { return err == hipSuccess && !overflow; }
  const double* one() {
    std::vector<double> v{1.0, 0.0};
    return upload(v);
  }
  void gemm(std::vector<Task>& t, std::vector<Seg>& s) {
    std::vector<int> map;
    for (size_t i = 0; i < t.size(); ++i) {
      t[i].tile0 = int(map.size());
      const int nt = ((t[i].m + kGemmTile - 1) / kGemmTile) * ((t[i].n + kGemmTile - 1) / kGemmTile);
      map.insert(map.end(), size_t(nt), int(i));
    }
    if (!map.empty()) {
      const unsigned ntile = unsigned(map.size());
      const Task* dt = upload(t);
      const Seg* ds = upload(s);
      const int* dm = upload(map);
      if (ok()) {
        hipLaunchKernelGGL(k_obs_gemm, dim3(ntile), dim3(64), 0, st, dt, dm, ds);
        note(hipGetLastError());
      }
    }
    t.clear();
    s.clear();
  }
  void close(std::vector<CTask>& t, std::vector<Pair>& p, double* out) {
    if (!t.empty()) {
      const unsigned ntask = unsigned(t.size());
      const CTask* dt = upload(t);
      const Pair* dp = upload(p);
      if (ok() && out) {
        hipLaunchKernelGGL(k_obs_close, dim3(ntask), dim3(kCloseNT), 0, st, dt, dp, out);
        note(hipGetLastError());
      }
    }
    t.clear();
    p.clear();
  }
  int eig(std::vector<ETask>& t, int* status) {
    std::vector<ETask> g[2];
    eig_split(t, g[0], g[1]);
    int launches = 0;
    size_t done = 0;
    for (int i = 0; i < 2; ++i) {
      if (g[i].empty()) continue;
      const size_t cnt = g[i].size();
      ++launches;
      if (ok())
        note(eig_launch(g[i], status ? status + done : nullptr, i == 0 ? 64 : 256, st,
                        [&](std::vector<ETask>& v) { return upload(v); }));
      done += cnt;
    }
    t.clear();
    return launches;
  }
  void entropy(std::vector<STask>& t, double* out) {
    if (!t.empty()) {
      const unsigned ntask = unsigned(t.size());
      const STask* dt = upload(t);
      if (ok() && out) {
        hipLaunchKernelGGL(k_obs_entropy, dim3(ntask), dim3(64), 0, st, dt, out);
        note(hipGetLastError());
      }
    }
    t.clear();
  }
  void sample(SampleTable& tb, const SArgs& a) {
    if (ok()) note(sample_launch(tb, a, st, [&](auto& v) { return upload(v); }));
  }
  void energy(EnergyTable& tb, const EArgs& a, std::vector<double>& coef) {
    std::vector<double> cf = coef;  // (upload takes its vector)
    if (ok()) note(energy_launch(tb, a, cf, st, [&](auto& v) { return upload(v); }));
  }
  void pair(PairTable& tb, const PArgs& a) {
    if (ok()) note(pair_launch(tb, a, st, [&](auto& v) { return upload(v); }));
  }
  const double* consts(std::vector<double>& v) { return upload(v); }
  void string(StringTable& tb, const StrArgs& a) {
    if (ok()) note(string_launch(tb, a, st, [&](auto& v) { return upload(v); }));
  }
};

// ------------------------------------------------------------------ driver
// whether a backend has the pair chain launch
template <class BE, class = void>
struct has_pair : std::false_type {};
template <class BE>
struct has_pair<BE, std::void_t<decltype(std::declval<BE&>().pair(std::declval<PairTable&>(), std::declval<const PArgs&>()))>>
    : std::true_type {};

// whether a backend has the string chain launches
template <class BE, class = void>
struct has_string : std::false_type {};
template <class BE>
struct has_string<BE, std::void_t<decltype(std::declval<BE&>().string(std::declval<StringTable&>(), std::declval<const StrArgs&>()))>>
    : std::true_type {};

// close outputs one state can produce (sizes its slice of the result buffer)
inline size_t max_outputs(int L, int p, int nrows, Want w) {
  return 1 + (w.env() ? size_t(L) * p : 0) + 2 * size_t(nrows) * L + (w.mom ? size_t(kEnergyOut) : 0) +
         (w.pair ? pair_outputs(L, p) : 0) + (w.str ? size_t(w.str->nops) : 0);
}

// Queue every launch of one chunk.  out_slot[i] is state i's index in the
// caller's outputs; rows are start sites (1..L).  Close task j of the chunk
// writes complex j of d_out and belongs to dests[j].  Returns d_out.
// With spec (want.spec) the Lenv of every bond is kept and, after the sweeps,
// the spectrum stages run over the whole chunk: stage A eigen-decomposes every
// Lenv_b[q] = V diag(lambda) V^H into S = V diag(sqrt(max(lambda, 0))), two GEMM
// launches form Y = Renv_b[q] S and X = S^H Y, stage B takes the eigenvalues of
// X (the Schmidt weights of the sector) and one wave per (state, bond) reduces
// the entropy.  A sector without an Lenv or Renv block gets zero weights.
// With want.pair S are the bras and kets the kets of the chunk's pairs.
template <class BE>
double* run_chunk(BE& be, int L, int p, int Q, const std::vector<const StateDesc*>& S,
                  const std::vector<size_t>& out_slot, const std::vector<int>& rows, Want want,
                  std::vector<Dest>& dests, Traffic& tr, Spec* spec = nullptr, Snap* snap = nullptr,
                  const std::vector<const StateDesc*>* kets = nullptr) {
  const int Q1 = Q + 1, B = int(S.size()), R = int(rows.size());
  const bool ada = want.ada && R > 0, nn = want.nn && R > 0, env = want.occ || ada || nn;
  const bool renv = env || spec != nullptr || (snap && !snap->given);
  dests.clear();
  double* d_out = be.alloc(size_t(B) * max_outputs(L, p, R, want));
  const double* one = be.one();
  if (want.mom) {
    energy_chunk(be, L, p, Q, S, out_slot, d_out, one, dests, tr);
    return d_out;
  }
  if (want.pair) {
    if constexpr (has_pair<BE>::value)  // (a backend without the pair launch is never asked for pairs)
      pair_chunk(be, L, p, Q, S, *kets, out_slot, want.pair_occ, want.pair_hop, d_out, one, dests, tr);
    return d_out;
  }
  if (want.str) {
    if constexpr (has_string<BE>::value)  // (a backend without the string launches is never asked for strings)
      string_chunk(be, L, p, Q, S, out_slot, *want.str, d_out, one, dests, tr);
    return d_out;
  }
  auto D = [&](int i, int b, int q) { return (q < 0 || q > Q) ? 0 : S[i]->dims[size_t(b) * Q1 + q]; };
  auto A = [&](int i, int k, int q, int n) -> Blk {
    if (q < 0 || n < 0 || n >= p || q + n > Q) return Blk{};
    return S[i]->blk[(size_t(k) * Q1 + q) * p + n];
  };
  std::vector<Task> gt;
  std::vector<Seg> gs;
  auto seg = [&](const double* a, int lda, const double* b, int ldb, int k, int ops, double alpha) {
    gs.push_back(Seg{a, b, lda, ldb, k, ops, alpha});
  };
  // a task over the segments pushed since s0 (m x n, k per segment as pushed)
  auto task = [&](double* C, int m, int n, int s0) {
    const int ns = int(gs.size()) - s0;
    gt.push_back(Task{C, n, m, n, s0, ns, 0});
    for (int s = s0; s < s0 + ns; ++s) {
      tr.flops += 8.0 * m * n * gs[s].k;
      tr.bytes += 16.0 * (double(m) * gs[s].k + double(gs[s].k) * n);
    }
    tr.bytes += 16.0 * m * n;
  };
  auto launch_gemm = [&] {
    if (!gt.empty()) ++tr.launches;
    be.gemm(gt, gs);
  };

  // ---- right sweep: Renv[i][b * Q1 + q], b = 1..L
  std::vector<std::vector<const double*>> Renv(B);
  if (renv) {
    for (int i = 0; i < B; ++i) {
      Renv[i].assign(size_t(L + 1) * Q1, nullptr);
      Renv[i][size_t(L) * Q1 + Q] = one;
    }
    std::vector<std::vector<double*>> W(B);
    for (int k = L; k >= 2; --k) {
      for (int i = 0; i < B; ++i) {
        W[i].assign(size_t(Q1) * p, nullptr);
        for (int q = 0; q <= Q; ++q)
          for (int n = 0; n < p && q + n <= Q; ++n) {
            const Blk a = A(i, k, q, n);
            const double* r = Renv[i][size_t(k) * Q1 + q + n];
            if (!a.p || !r) continue;
            double* w = be.alloc(size_t(a.r) * a.c);
            const int s0 = int(gs.size());
            seg(a.p, a.c, r, a.c, a.c, 0, 1.0);
            task(w, a.r, a.c, s0);
            W[i][size_t(q) * p + n] = w;
          }
      }
      launch_gemm();
      for (int i = 0; i < B; ++i)
        for (int q = 0; q <= Q; ++q) {
          const int dq = D(i, k - 1, q);
          if (dq == 0) continue;
          const int s0 = int(gs.size());
          for (int n = 0; n < p && q + n <= Q; ++n) {
            const double* w = W[i][size_t(q) * p + n];
            if (!w) continue;
            const Blk a = A(i, k, q, n);
            seg(w, a.c, a.p, a.c, a.c, 2, 1.0);
          }
          if (int(gs.size()) == s0) continue;
          double* r = be.alloc(size_t(dq) * dq);
          task(r, dq, dq, s0);
          Renv[i][size_t(k - 1) * Q1 + q] = r;
        }
      launch_gemm();
    }
  }

  // ---- snapshots: the table of every block and right environment, then one launch
  if (snap) {
    SampleTable tb;
    const bool amp = snap->given != nullptr;
    int vmax = 1;
    double work = 0;  // complex multiply-adds of one shot along the widest sectors
    for (int i = 0; i < B; ++i) {
      tb.st.push_back(SState{snap->ids ? snap->ids[out_slot[i]] : 0ull, (long long)tb.blk.size(),
                             (long long)tb.renv.size()});
      for (int k = 1; k <= L; ++k) {
        double site = 0;
        for (int q = 0; q <= Q; ++q) {
          double sec = 0;
          for (int n = 0; n < p; ++n) {
            const Blk a = A(i, k, q, n);
            tb.blk.push_back(SBlk{a.p, a.r, a.c});
            if (!a.p) continue;
            vmax = std::max(vmax, std::max(a.r, a.c));
            const double rc = double(a.r) * a.c, cc = double(a.c) * a.c;
            sec = amp ? std::max(sec, rc) : sec + rc + cc + rc / p;
          }
          site = std::max(site, sec);
        }
        work += site;
        for (int q = 0; q <= Q; ++q) tb.renv.push_back(amp ? nullptr : Renv[i][size_t(k) * Q1 + q]);
      }
    }
    const size_t items = size_t(B) * snap->nper;
    snap->d_config = amp ? nullptr : reinterpret_cast<signed char*>(be.alloc((items * L + 15) / 16));
    snap->d_val = be.alloc(amp ? items : (items + 1) / 2);
    if (amp) tb.given.assign(snap->given, snap->given + size_t(snap->nper) * L);
    tr.flops += 8.0 * work / B * double(items);
    tr.bytes += 16.0 * work / B * double(items) + (amp ? 16.0 : 8.0 + L) * double(items);
    ++tr.launches;
    be.sample(tb, SArgs{nullptr, nullptr, nullptr, nullptr, snap->d_config, snap->d_val, snap->seed, L, p, Q,
                        snap->nper, vmax});
    return d_out;
  }

  // ---- left sweep
  struct Open {
    std::vector<const double*> C, N;  // [q] on the current bond (C[s]: d[s+1] x d[s])
  };
  std::vector<std::vector<const double*>> Lenv(B), Lall(B);  // Lall[i][b * Q1 + q]: every bond's, for the spectra
  std::vector<std::vector<Open>> open(B, std::vector<Open>(R));
  for (int i = 0; i < B; ++i) {
    Lenv[i].assign(Q1, nullptr);
    Lenv[i][0] = one;
    if (spec) Lall[i].assign(size_t(L + 1) * Q1, nullptr);
  }
  std::vector<CTask> ct;
  std::vector<Pair> cp;
  auto close_task = [&](int p0, Dest d) {
    ct.push_back(CTask{p0, int(cp.size()) - p0});
    for (size_t j = size_t(p0); j < cp.size(); ++j) {
      tr.bytes += 32.0 * double(cp[j].n);
      tr.flops += 8.0 * double(cp[j].n);
    }
    dests.push_back(d);
  };
  const size_t QP = size_t(Q1) * p;
  for (int k = 1; k <= L; ++k) {
    // products with the site's blocks: T = Lenv A, X = A Renv^H, TC = C A, TN = N A
    std::vector<std::vector<double*>> T(B), X(B);
    std::vector<std::vector<std::vector<double*>>> TC(B), TN(B);
    for (int i = 0; i < B; ++i) {
      T[i].assign(QP, nullptr);
      X[i].assign(QP, nullptr);
      TC[i].assign(R, std::vector<double*>());
      TN[i].assign(R, std::vector<double*>());
      for (int q = 0; q <= Q; ++q)
        for (int n = 0; n < p && q + n <= Q; ++n) {
          const Blk a = A(i, k, q, n);
          if (!a.p) continue;
          if (const double* l = Lenv[i][q]) {
            double* t = be.alloc(size_t(a.r) * a.c);
            const int s0 = int(gs.size());
            seg(l, a.r, a.p, a.c, a.r, 0, 1.0);
            task(t, a.r, a.c, s0);
            T[i][size_t(q) * p + n] = t;
          }
          const double* r = env ? Renv[i][size_t(k) * Q1 + q + n] : nullptr;
          if (r) {
            double* x = be.alloc(size_t(a.r) * a.c);
            const int s0 = int(gs.size());
            seg(a.p, a.c, r, a.c, a.c, 2, 1.0);
            task(x, a.r, a.c, s0);
            X[i][size_t(q) * p + n] = x;
          }
        }
      for (int ri = 0; ri < R; ++ri) {
        if (rows[ri] >= k) continue;
        const Open& o = open[i][ri];
        if (ada) {
          TC[i][ri].assign(QP, nullptr);
          for (int s = 0; s <= Q; ++s) {
            if (!o.C[s]) continue;
            const int m = D(i, k - 1, s + 1), kk = D(i, k - 1, s);
            for (int n = 0; n < p && s + n <= Q; ++n) {
              const Blk a = A(i, k, s, n);
              if (!a.p) continue;
              double* t = be.alloc(size_t(m) * a.c);
              const int s0 = int(gs.size());
              seg(o.C[s], kk, a.p, a.c, kk, 0, 1.0);
              task(t, m, a.c, s0);
              TC[i][ri][size_t(s) * p + n] = t;
            }
          }
        }
        if (nn) {
          TN[i][ri].assign(QP, nullptr);
          for (int q = 0; q <= Q; ++q) {
            if (!o.N[q]) continue;
            for (int n = 0; n < p && q + n <= Q; ++n) {
              const Blk a = A(i, k, q, n);
              if (!a.p) continue;
              double* t = be.alloc(size_t(a.r) * a.c);
              const int s0 = int(gs.size());
              seg(o.N[q], a.r, a.p, a.c, a.r, 0, 1.0);
              task(t, a.r, a.c, s0);
              TN[i][ri][size_t(q) * p + n] = t;
            }
          }
        }
      }
    }
    launch_gemm();

    // the environments of bond k
    for (int i = 0; i < B; ++i) {
      std::vector<const double*> Ln(Q1, nullptr);
      for (int qq = 0; qq <= Q; ++qq) {
        const int c = D(i, k, qq);
        if (c == 0) continue;
        const int s0 = int(gs.size());
        for (int n = 0; n < p && qq - n >= 0; ++n) {
          const double* t = T[i][size_t(qq - n) * p + n];
          if (!t) continue;
          const Blk a = A(i, k, qq - n, n);
          seg(a.p, a.c, t, a.c, a.r, 1, 1.0);
        }
        if (int(gs.size()) == s0) continue;
        double* l = be.alloc(size_t(c) * c);
        task(l, c, c, s0);
        Ln[qq] = l;
      }
      for (int ri = 0; ri < R && k < L; ++ri) {
        if (rows[ri] > k) continue;
        const bool opening = rows[ri] == k;
        Open nx;
        if (ada) {
          nx.C.assign(Q1, nullptr);
          for (int sp = 0; sp + 1 <= Q; ++sp) {  // C[sp]: d(k, sp+1) x d(k, sp)
            const int m = D(i, k, sp + 1), nc = D(i, k, sp);
            if (m == 0 || nc == 0) continue;
            const int s0 = int(gs.size());
            for (int n = 0; n < p && sp - n >= 0; ++n) {
              const int s = sp - n;
              if (opening) {
                const double* t = T[i][size_t(s) * p + n];
                const Blk a1 = A(i, k, s, n + 1);
                if (t && a1.p) seg(a1.p, a1.c, t, nc, a1.r, 1, std::sqrt(double(n + 1)));
              } else {
                const double* t = TC[i][ri][size_t(s) * p + n];
                const Blk a1 = A(i, k, s + 1, n);
                if (t && a1.p) seg(a1.p, a1.c, t, nc, a1.r, 1, 1.0);
              }
            }
            if (int(gs.size()) == s0) continue;
            double* cn = be.alloc(size_t(m) * nc);
            task(cn, m, nc, s0);
            nx.C[sp] = cn;
          }
        }
        if (nn) {
          nx.N.assign(Q1, nullptr);
          for (int qq = 0; qq <= Q; ++qq) {
            const int c = D(i, k, qq);
            if (c == 0) continue;
            const int s0 = int(gs.size());
            for (int n = opening ? 1 : 0; n < p && qq - n >= 0; ++n) {
              const double* t = opening ? T[i][size_t(qq - n) * p + n] : TN[i][ri][size_t(qq - n) * p + n];
              if (!t) continue;
              const Blk a = A(i, k, qq - n, n);
              seg(a.p, a.c, t, a.c, a.r, 1, opening ? double(n) : 1.0);
            }
            if (int(gs.size()) == s0) continue;
            double* nq = be.alloc(size_t(c) * c);
            task(nq, c, c, s0);
            nx.N[qq] = nq;
          }
        }
        // closes below still read the products of the old environments (TC, TN), not these
        open[i][ri] = std::move(nx);
      }
      if (spec) std::copy(Ln.begin(), Ln.end(), Lall[i].begin() + size_t(k) * Q1);
      Lenv[i] = std::move(Ln);
    }
    launch_gemm();

    // closes of site k
    for (int i = 0; i < B; ++i) {
      const size_t o = out_slot[i];
      if (env)
        for (int n = 0; n < p; ++n) {
          const int p0 = int(cp.size());
          for (int q = 0; q + n <= Q; ++q) {
            const double *x = X[i][size_t(q) * p + n], *t = T[i][size_t(q) * p + n];
            if (!x || !t) continue;
            const Blk a = A(i, k, q, n);
            cp.push_back(Pair{x, t, (long long)a.r * a.c, 1.0});
          }
          close_task(p0, Dest{1, (o * L + (k - 1)) * p + n});
        }
      for (int ri = 0; ri < R; ++ri) {
        if (rows[ri] >= k) continue;
        if (ada) {
          const int p0 = int(cp.size());
          for (int s = 0; s + 1 <= Q; ++s)
            for (int n = 1; n < p && s + n <= Q; ++n) {
              const double *x = X[i][size_t(s + 1) * p + n - 1], *t = TC[i][ri][size_t(s) * p + n];
              if (!x || !t) continue;
              const Blk a = A(i, k, s + 1, n - 1);
              cp.push_back(Pair{x, t, (long long)a.r * a.c, std::sqrt(double(n))});
            }
          close_task(p0, Dest{2, (o * R + ri) * L + (k - 1)});
        }
        if (nn) {
          const int p0 = int(cp.size());
          for (int q = 0; q <= Q; ++q)
            for (int n = 1; n < p && q + n <= Q; ++n) {
              const double *x = X[i][size_t(q) * p + n], *t = TN[i][ri][size_t(q) * p + n];
              if (!x || !t) continue;
              const Blk a = A(i, k, q, n);
              cp.push_back(Pair{x, t, (long long)a.r * a.c, double(n)});
            }
          close_task(p0, Dest{3, (o * R + ri) * L + (k - 1)});
        }
      }
      if (k == L && want.norm) {
        const int p0 = int(cp.size());
        if (Lenv[i][Q]) cp.push_back(Pair{one, Lenv[i][Q], 1, 1.0});
        close_task(p0, Dest{0, o});
      }
    }
    if (!ct.empty()) {
      ++tr.launches;
      const size_t first = dests.size() - ct.size();
      be.close(ct, cp, d_out ? d_out + 2 * first : nullptr);
    }
  }

  // ---- spectra of the bonds 1..L-1
  if (spec) {
    const int NB = L - 1, lds_max = eig_lds_max();
    spec->woff.assign(size_t(B) * NB, 0);
    spec->nw = spec->nstatus = 0;
    for (int i = 0; i < B; ++i)
      for (int b = 1; b < L; ++b) {
        spec->woff[size_t(i) * NB + b - 1] = spec->nw;
        for (int q = 0; q <= Q; ++q) {
          const int d = D(i, b, q);
          spec->nw += size_t(d);
          if (d > 0) spec->nstatus += (Lall[i][size_t(b) * Q1 + q] && Renv[i][size_t(b) * Q1 + q]) ? 2 : 1;
        }
      }
    // doubles and ints out of the complex-granular workspace
    spec->d_w = be.alloc((spec->nw + 1) / 2);
    spec->d_ent = be.alloc((size_t(B) * NB + 1) / 2);
    spec->d_status = reinterpret_cast<int*>(be.alloc((spec->nstatus + 3) / 4));
    std::vector<ETask> ea, eb;
    std::vector<STask> es;
    auto eig_traffic = [&](const ETask& t) {
      if (!t.A) return;
      tr.bytes += 16.0 * t.n * t.n * (t.S ? 2 : 1) + (t.w ? 8.0 * t.n : 0.0);
      tr.flops += eig_flops(t.n, t.S != nullptr);
    };
    struct Sec {
      const double* r;
      double *s, *y, *x;
      int n;
    };
    std::vector<Sec> secs;
    for (int i = 0; i < B; ++i)
      for (int b = 1; b < L; ++b) {
        double* w = spec->d_w ? spec->d_w + spec->woff[size_t(i) * NB + b - 1] : nullptr;
        int nb = 0;
        for (int q = 0; q <= Q; ++q) {
          const int d = D(i, b, q);
          if (d == 0) continue;
          const double *l = Lall[i][size_t(b) * Q1 + q], *r = Renv[i][size_t(b) * Q1 + q];
          double* wq = w ? w + nb : nullptr;
          nb += d;
          if (!l || !r) {
            eb.push_back(ETask{nullptr, nullptr, wq, nullptr, d});
            continue;
          }
          const size_t dd = size_t(d) * d;
          Sec sc{r, be.alloc(dd), be.alloc(dd), be.alloc(dd), d};
          const size_t wa = eig_work(d, true, lds_max), wb = eig_work(d, false, lds_max);
          ea.push_back(ETask{l, sc.s, nullptr, wa ? be.alloc(wa) : nullptr, d});
          eb.push_back(ETask{sc.x, nullptr, wq, wb ? be.alloc(wb) : nullptr, d});
          secs.push_back(sc);
        }
        es.push_back(STask{w, nb});
      }
    for (const ETask& t : ea) eig_traffic(t);
    for (const ETask& t : eb) eig_traffic(t);
    const size_t na = ea.size();
    tr.launches += be.eig(ea, spec->d_status);
    for (const Sec& sc : secs) {
      const int s0 = int(gs.size());
      seg(sc.r, sc.n, sc.s, sc.n, sc.n, 0, 1.0);
      task(sc.y, sc.n, sc.n, s0);
    }
    launch_gemm();
    for (const Sec& sc : secs) {
      const int s0 = int(gs.size());
      seg(sc.s, sc.n, sc.y, sc.n, sc.n, 1, 1.0);
      task(sc.x, sc.n, sc.n, s0);
    }
    launch_gemm();
    tr.launches += be.eig(eb, spec->d_status ? spec->d_status + na : nullptr);
    if (!es.empty()) {
      ++tr.launches;
      tr.bytes += 8.0 * double(spec->nw + es.size());
      tr.flops += 4.0 * double(spec->nw);
      be.entropy(es, spec->d_ent);
    }
  }
  return d_out;
}

// workspace bytes of every state alone (a chunk of several takes at most the
// sum), by a dry run per distinct set of bond-sector dims (with kets: of every pair, per distinct dims of both;
// the operators of want.str, and so their supports, are those of the whole request)
inline std::vector<size_t> workspace_needs(int L, int p, int Q, const std::vector<StateDesc>& desc,
                                           const std::vector<int>& rows, Want want, const Snap* snap = nullptr,
                                           const std::vector<StateDesc>* kets = nullptr) {
  std::map<std::vector<int>, size_t> seen;
  std::vector<size_t> need(desc.size());
  for (size_t i = 0; i < desc.size(); ++i) {
    std::vector<int> key = desc[i].dims;
    if (kets) key.insert(key.end(), (*kets)[i].dims.begin(), (*kets)[i].dims.end());
    auto it = seen.find(key);
    if (it == seen.end()) {
      CountBackend cb;
      std::vector<Dest> dd;
      Traffic tt;
      Spec sp;
      Snap sn;
      if (snap) {
        sn = *snap;
        sn.ids = nullptr;
      }
      std::vector<const StateDesc*> ky;
      if (kets) ky.push_back(&(*kets)[i]);
      run_chunk(cb, L, p, Q, {&desc[i]}, {0}, rows, want, dd, tt, want.spec ? &sp : nullptr, snap ? &sn : nullptr,
                kets ? &ky : nullptr);
      it = seen.emplace(key, cb.bytes).first;
    }
    need[i] = it->second;
  }
  return need;
}

// workspace bytes one chunk may take: half the free device memory, as the
// engines' row batches (OCG_OBS_BUDGET=bytes overrides: tests of the chunking)
inline size_t chunk_budget() {
  if (const char* e = std::getenv("OCG_OBS_BUDGET")) return size_t(std::atoll(e));
  size_t fr = 0, tot = 0;
  (void)hipMemGetInfo(&fr, &tot);
  return fr / 2;
}

// host outputs of ocg_observe (null: not wanted); nt states, nrows rows
struct Outputs {
  double* norm2 = nullptr;
  double* occ = nullptr;
  double* ada = nullptr;
  double* nn = nullptr;
  int L = 0, p = 0, nrows = 0;
  const int* rows = nullptr;
  double* mom = nullptr;  // [nt][7]: alone (ocg_observe_moments)
  // alone (ocg_observe_pairs), complex: [n] <x|y>, [n][L][p] <x|P_k(n)|y>, [n][L-1][2] the hopping elements
  double* povl = nullptr;
  double* pocc = nullptr;
  double* phop = nullptr;
  // alone (ocg_observe_strings), complex: [nt][nops] <s|O_m|s> of the operators *str
  const Strings* str = nullptr;
  double* sout = nullptr;
};

// what the kernels must compute for the requested outputs (the diagonal of a
// correlation row comes from the occupations)
inline Want want_of(const Outputs& o) {
  Want w;
  w.norm = o.norm2 != nullptr;
  w.ada = o.ada != nullptr && o.nrows > 0;
  w.nn = o.nn != nullptr && o.nrows > 0;
  w.occ = o.occ != nullptr || w.ada || w.nn;
  w.mom = o.mom != nullptr;
  w.pair_occ = o.pocc != nullptr;
  w.pair_hop = o.phop != nullptr && o.L > 1;
  w.pair = o.povl != nullptr || w.pair_occ || w.pair_hop;
  w.str = o.sout ? o.str : nullptr;
  return w;
}

// scatter a chunk's close results; occ_tmp ([nt][L][p]) receives the
// occupations when the caller did not ask for them but the rows need them
inline void scatter(const std::vector<Dest>& dests, const double* res, const Outputs& o, double* occ_buf) {
  for (size_t j = 0; j < dests.size(); ++j) {
    const Dest d = dests[j];
    switch (d.kind) {
      case 0: o.norm2[d.idx] = res[2 * j]; break;
      case 1: occ_buf[d.idx] = res[2 * j]; break;
      case 2:
        o.ada[2 * d.idx] = res[2 * j];
        o.ada[2 * d.idx + 1] = res[2 * j + 1];
        break;
      case 3: o.nn[d.idx] = res[2 * j]; break;
      case 4: o.mom[d.idx] = res[2 * j]; break;
      case 5:
        o.mom[d.idx] = res[2 * j];
        o.mom[d.idx + 1] = res[2 * j + 1];
        break;
      case 6:
      case 7:
      case 8:
        if (double* dst = d.kind == 6 ? o.povl : d.kind == 7 ? o.pocc : o.phop) {
          dst[2 * d.idx] = res[2 * j];
          dst[2 * d.idx + 1] = res[2 * j + 1];
        }
        break;
      case 9:
        o.sout[2 * d.idx] = res[2 * j];
        o.sout[2 * d.idx + 1] = res[2 * j + 1];
        break;
    }
  }
}

// the j = i entries of the rows of state slot s from its occupations
inline void diagonals(size_t s, const Outputs& o, const double* occ_buf) {
  for (int ri = 0; ri < o.nrows; ++ri) {
    const int i = o.rows[ri] - 1;
    const double* oc = occ_buf + (s * o.L + i) * o.p;
    double n1 = 0, n2 = 0;
    for (int n = 0; n < o.p; ++n) {
      n1 += n * oc[n];
      n2 += double(n) * n * oc[n];
    }
    const size_t at = (s * o.nrows + ri) * o.L + i;
    if (o.ada) {
      o.ada[2 * at] = n1;
      o.ada[2 * at + 1] = 0.0;
    }
    if (o.nn) o.nn[at] = n2;
  }
}

// the descriptor of a state held on the device in the compact interchange format
// itself (include/ocmps.h: sites 1..L, per site the blocks (q, n) in order, each a
// contiguous row-major matrix) at d_data; returns its complex elements
inline size_t compact_desc(int L, int p, int Q, const int* dims, const double* d_data, StateDesc& out) {
  const int Q1 = Q + 1;
  out.dims.assign(dims, dims + size_t(L + 1) * Q1);
  out.blk.assign(size_t(L + 1) * Q1 * p, Blk{});
  size_t off = 0;
  for (int k = 1; k <= L; ++k)
    for (int q = 0; q <= Q; ++q)
      for (int n = 0; n < p && q + n <= Q; ++n) {
        const int r = dims[(k - 1) * Q1 + q], c = dims[k * Q1 + q + n];
        if (r <= 0 || c <= 0) continue;
        out.blk[(size_t(k) * Q1 + q) * p + n] = Blk{d_data ? d_data + 2 * off : nullptr, r, c};  // (null: counting)
        off += size_t(r) * c;
      }
  return off;
}

// host outputs of ocg_observe_spectrum (null: not wanted)
struct SpecOutputs {
  double* entropy = nullptr;  // [nt][L-1]
  double* schmidt = nullptr;  // [nt][L-1][wcap]
  int* sector = nullptr;      // [nt][L-1][wcap]
  int wcap = 0;
  bool weights() const { return schmidt || sector; }
};

// the largest bond dimension and sector order of a state
inline void widest(const StateDesc& d, int L, int Q1, int& bond, int& order) {
  for (int b = 1; b < L; ++b) {
    int sum = 0;
    for (int q = 0; q < Q1; ++q) {
      sum += d.dims[size_t(b) * Q1 + q];
      order = std::max(order, d.dims[size_t(b) * Q1 + q]);
    }
    bond = std::max(bond, sum);
  }
}

// a chunk's spectrum results (host copies of Spec's buffers; w may be null when
// no weights are wanted) into the outputs: the weights of a bond descending,
// ties by sector ascending, padded with 0 / -1 up to wcap
inline void scatter_spectrum(const Spec& sp, const std::vector<const StateDesc*>& S,
                             const std::vector<size_t>& out_slot, int L, int Q1, const double* ent,
                             const double* w, const SpecOutputs& o) {
  const int NB = L - 1;
  std::vector<std::pair<double, int>> ws;
  for (size_t i = 0; i < S.size(); ++i)
    for (int b = 1; b < L; ++b) {
      const size_t at = out_slot[i] * NB + (b - 1);
      if (o.entropy) o.entropy[at] = ent[i * NB + (b - 1)];
      if (!o.weights()) continue;
      ws.clear();
      const double* wb = w + sp.woff[i * NB + (b - 1)];
      for (int q = 0; q < Q1; ++q)
        for (int j = 0; j < S[i]->dims[size_t(b) * Q1 + q]; ++j) ws.emplace_back(*wb++, q);
      std::stable_sort(ws.begin(), ws.end(), [](const std::pair<double, int>& x, const std::pair<double, int>& y) {
        return x.first > y.first || (x.first == y.first && x.second < y.second);
      });
      for (int j = 0; j < o.wcap; ++j) {
        const bool in = size_t(j) < ws.size();
        if (o.schmidt) o.schmidt[at * o.wcap + j] = in ? ws[j].first : 0.0;
        if (o.sector) o.sector[at * o.wcap + j] = in ? ws[j].second : -1;
      }
    }
}

}  // namespace obs
