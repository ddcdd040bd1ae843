// Expectations of products of diagonal one-site operators in stored MPS (ocg_observe_strings /
// ocg_observe_strings_states): for every state s of a chunk and every operator m of the request
//   O_m = (x)_k F_{m,k},   F_{m,k} = sum_n f[m][k-1][n] P_k(n)      (P_k(n): projector on occupation n of site k)
// the raw complex number <s|O_m|s>.  The support [a, b] of an operator runs from its first to its last
// site whose table is not exactly (1, 0) for every n; an empty support is treated as the support [1, 1]
// (the table of site 1 is the identity then, so the result is norm2).  With Lenv / Renv the
// environments of ocg_observe
//   E_{a-1}[q] = Lenv_{a-1}[q]
//   E_k[q + n] += f[k][n] A_k(q, n)^H E_{k-1}[q] A_k(q, n)           k = a..b
//   out = sum_q tr(E_b[q] Renv_b[q]).
// A block that does not exist, and a level whose f is exactly 0, contribute nothing.
//
// Two paths, chosen per state by its widest bond sector (so a state's numbers do not depend on what
// else is in the chunk):
//   * string_lists: L - 1 rounds of two GEMM launches form Lenv of the bonds 1..L-1 and Renv of the bonds
//     L-1..1 together (round j: site j from the left, site L+1-j from the right); then all operators of all
//     states advance together, one support site per round of two GEMM launches (T = E A, then
//     E' = sum_n f A^H T); one close launch at the end takes sum conj(Renv_b) . E_b (Renv is Hermitian).
//     Launches of one chunk: 2 (L - 1) + 2 M + 1, M the longest support (at least 1).
//     The segment scale of the GEMM backends is real.  An operator with a non-real table carries
//     F = i E beside E (from J = i Lenv, swept from an uploaded constant i):
//       E' = sum_n Re f A^H (E A) + Im f A^H (F A),   F' = sum_n Re f A^H (F A) - Im f A^H (E A),
//     so the backends and every existing caller's segments stay as they are.
//   * k_obs_string_env + k_obs_string: states whose sectors are all at most 16 wide.  Two launches per
//     chunk: a workgroup per state writes the Lenv / Renv tiles of every bond to the workspace, then a
//     workgroup per (state, operator) sweeps the support and closes it.  Every block is one 16 x 16 MFMA
//     tile in k_obs_pair's operand layout; sector q belongs to wave q % 4; the per-sector partial closes
//     are added in sector order by one thread after a __syncthreads().
// The two paths sum in different orders: they agree to rounding, not bit for bit.
// Included by observe.hpp after observe_pair.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace obs {

constexpr int kStringMaxOrder = 512;   // the sector orders the list path is offered
constexpr int kStringChainOrder = 16;  // states up to this order run on k_obs_string

// the operators of one request (host)
struct Strings {
  int nops = 0;
  const double* f = nullptr;  // [nops][L][p][2]
  std::vector<int> a, b;      // the support of every operator, 1 <= a <= b <= L
  std::vector<char> cplx;     // a table entry on the support has a nonzero imaginary part
  int longest = 0;            // the longest support
  void prepare(int L, int p) {
    a.assign(nops, 1);
    b.assign(nops, 1);
    cplx.assign(nops, 0);
    longest = 0;
    for (int m = 0; m < nops; ++m) {
      int lo = 0, hi = 0;
      for (int k = 1; k <= L; ++k) {
        bool id = true;
        for (int n = 0; n < p; ++n) {
          const double* e = f + 2 * ((size_t(m) * L + (k - 1)) * p + n);
          if (e[0] != 1.0 || e[1] != 0.0) id = false;
        }
        if (!id) {
          if (!lo) lo = k;
          hi = k;
        }
      }
      if (lo) {
        a[m] = lo;
        b[m] = hi;
      }
      for (int k = a[m]; k <= b[m]; ++k)
        for (int n = 0; n < p; ++n)
          if (f[2 * ((size_t(m) * L + (k - 1)) * p + n) + 1] != 0.0) cplx[m] = 1;
      longest = std::max(longest, b[m] - a[m] + 1);
    }
  }
};

// OCG_OBS_STRING_CHAIN=0: every state on the list path
inline bool string_chain_enabled() {
  const char* e = std::getenv("OCG_OBS_STRING_CHAIN");
  return !(e && e[0] == '0');
}

// ------------------------------------------------------------------ chain kernels
struct StrArgs {
  const EBlk* blk;   // [state][site k - 1][q][n]
  const int* dims;   // [state][bond 0..L][q]
  const double* f;   // [nops][L][p][2]
  const int* sup;    // [nops][2]: a, b
  double* env;       // [state]: Renv of the bonds 0..L, then Lenv of the bonds 0..L; tiles of 16 x 16 complex (ld 16)
  double* sweep;     // [state][op][2][q]: the E tiles of two bonds
  double* out;       // [state][op] complex
  int L, p, Q, nops;
};
struct StringTable {
  std::vector<EBlk> blk;
  std::vector<int> dims;
  std::vector<double> f;
  std::vector<int> sup;
};
__host__ __device__ inline size_t string_env_complex(int L, int Q1) { return size_t(2) * (L + 1) * Q1 * (kPairTile / 2); }  // per state
__host__ __device__ inline size_t string_sweep_complex(int Q1) { return size_t(2) * Q1 * (kPairTile / 2); }  // per (state, operator)
inline size_t string_lds_bytes(int Q1) { return sizeof(double) * 2 * size_t(Q1); }  // the partial closes (dynamic)
constexpr size_t kStringLdsStatic = 4 * kPairTile * sizeof(double);                // the four T tiles
// the chain kernels can take a state: every sector fits a tile and the partial closes fit the LDS
inline bool string_chain_fits(int widest, int Q1) {
  return widest <= kStringChainOrder && kStringLdsStatic + string_lds_bytes(Q1) <= kEnergyLdsLimit;
}

namespace {

// the tile products of both kernels, on the wave's LDS tile T (k_obs_pair's operand layout)
struct StrWave {
  double* T;
  int li, kl;
  __device__ void put_T(const pr_d4& tr, const pr_d4& ti) const {
    energy_wave_order();  // the loads of the previous T are done
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T[2 * ((kl + 4 * r) * 16 + li)] = tr[r];
      T[2 * ((kl + 4 * r) * 16 + li) + 1] = ti[r];
    }
    energy_wave_order();
  }
  __device__ void put_env(double* o, int m, int n, const pr_d4& cr, const pr_d4& ci) const {
    if (li >= n) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = kl + 4 * r;
      if (row < m) {
        o[2 * (row * 16 + li)] = cr[r];
        o[2 * (row * 16 + li) + 1] = ci[r];
      }
    }
  }
  // C += (fr + i fi) A^H T: A a stored r x c block, T the wave's tile (r x n)
  __device__ void add_AhT(pr_d4& cr, pr_d4& ci, const EBlk A, int n, double fr, double fi) const {
    const double* t = T;
    const int l = li;
    pair_mma(cr, ci, A.r, kl,
             [&](int kk, double& re, double& im) {
               if (l < A.c) {
                 const double ar = A.a[2 * (size_t(kk) * A.c + l)], ai = A.a[2 * (size_t(kk) * A.c + l) + 1];
                 re = ar * fr + ai * fi;
                 im = ar * fi - ai * fr;
               }
             },
             [&](int kk, double& re, double& im) {
               if (l < n) {
                 re = t[2 * (kk * 16 + l)];
                 im = t[2 * (kk * 16 + l) + 1];
               }
             });
  }
  // C = E A: E a tile (m x A.r), A a stored block
  __device__ void mul_EA(pr_d4& cr, pr_d4& ci, const double* E, int m, const EBlk A) const {
    const int l = li;
    pair_mma(cr, ci, A.r, kl,
             [&](int kk, double& re, double& im) {
               if (l < m) {
                 re = E[2 * (l * 16 + kk)];
                 im = E[2 * (l * 16 + kk) + 1];
               }
             },
             [&](int kk, double& re, double& im) {
               if (l < A.c) {
                 re = A.a[2 * (size_t(kk) * A.c + l)];
                 im = A.a[2 * (size_t(kk) * A.c + l) + 1];
               }
             });
  }
  // C = A R: A a stored block, R a tile (A.c x n)
  __device__ void mul_AR(pr_d4& cr, pr_d4& ci, const EBlk A, const double* R, int n) const {
    const int l = li;
    pair_mma(cr, ci, A.c, kl,
             [&](int kk, double& re, double& im) {
               if (l < A.r) {
                 re = A.a[2 * (size_t(l) * A.c + kk)];
                 im = A.a[2 * (size_t(l) * A.c + kk) + 1];
               }
             },
             [&](int kk, double& re, double& im) {
               if (l < n) {
                 re = R[2 * (kk * 16 + l)];
                 im = R[2 * (kk * 16 + l) + 1];
               }
             });
  }
  // C += T A^H: T the wave's tile (m x A.c), A a stored r x c block
  __device__ void add_TAh(pr_d4& cr, pr_d4& ci, int m, const EBlk A) const {
    const double* t = T;
    const int l = li;
    pair_mma(cr, ci, A.c, kl,
             [&](int kk, double& re, double& im) {
               if (l < m) {
                 re = t[2 * (l * 16 + kk)];
                 im = t[2 * (l * 16 + kk) + 1];
               }
             },
             [&](int kk, double& re, double& im) {
               if (l < A.r) {
                 re = A.a[2 * (size_t(l) * A.c + kk)];
                 im = -A.a[2 * (size_t(l) * A.c + kk) + 1];
               }
             });
  }
};

// One workgroup of four waves = one state: step j forms Renv of bond L - j and Lenv of bond j, each
// sector by wave q % 4, with one barrier per step.  A tile is written over the sector's extent whenever
// the sector exists (zeros where nothing contributes); a sector that does not exist is never read.
__global__ __launch_bounds__(256) void k_obs_string_env(const StrArgs a) {
  __shared__ double tt[4][kPairTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = a.L, p = a.p, Q1 = a.Q + 1;
  const size_t si = blockIdx.x;
  const size_t nblk = size_t(L) * Q1 * p, ndim = size_t(L + 1) * Q1;
  const EBlk* blk = a.blk + si * nblk;
  const int* dims = a.dims + si * ndim;
  double* renv = a.env + si * 2 * string_env_complex(L, Q1);
  double* lenv = renv + ndim * kPairTile;
  const StrWave W{tt[wave], lane & 15, lane >> 4};
  if (tid == 0) {
    double* r = renv + (size_t(L) * Q1 + a.Q) * kPairTile;
    r[0] = 1.0;
    r[1] = 0.0;
    lenv[0] = 1.0;
    lenv[1] = 0.0;
  }
  __syncthreads();
  for (int j = 1; j < L; ++j) {
    const int kr = L + 1 - j, kl = j;  // the sites absorbed from the right and from the left
    for (int q = wave; q < Q1; q += 4) {
      const int r = dims[size_t(kr - 1) * Q1 + q];
      if (r > 0) {
        pr_d4 cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        for (int n = 0; n < p && q + n < Q1; ++n) {
          const EBlk A = blk[(size_t(kr - 1) * Q1 + q) * p + n];
          if (!A.a) continue;
          pr_d4 wr = {0, 0, 0, 0}, wi = {0, 0, 0, 0};
          W.mul_AR(wr, wi, A, renv + (size_t(kr) * Q1 + q + n) * kPairTile, A.c);
          W.put_T(wr, wi);
          W.add_TAh(cr, ci, r, A);
        }
        W.put_env(renv + (size_t(kr - 1) * Q1 + q) * kPairTile, r, r, cr, ci);
      }
      const int c = dims[size_t(kl) * Q1 + q];
      if (c > 0) {
        pr_d4 cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        for (int n = 0; n < p && q - n >= 0; ++n) {
          const EBlk A = blk[(size_t(kl - 1) * Q1 + q - n) * p + n];
          if (!A.a) continue;
          pr_d4 tr = {0, 0, 0, 0}, ti = {0, 0, 0, 0};
          W.mul_EA(tr, ti, lenv + (size_t(kl - 1) * Q1 + q - n) * kPairTile, A.r, A);
          W.put_T(tr, ti);
          W.add_AhT(cr, ci, A, c, 1.0, 0.0);
        }
        W.put_env(lenv + (size_t(kl) * Q1 + q) * kPairTile, c, c, cr, ci);
      }
    }
    __syncthreads();
  }
}

// One workgroup of four waves = one (state, operator): E of bond k, sector by sector on wave q % 4, from E
// of bond k - 1 (Lenv of bond a - 1 at the first site), alternating between two sets of tiles with one
// barrier per site; at the last site the product stays in the accumulators and is closed with Renv.
__global__ __launch_bounds__(256) void k_obs_string(const StrArgs a) {
  __shared__ double tt[4][kPairTile];
  extern __shared__ double string_part[];  // [q] complex
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = a.L, p = a.p, Q1 = a.Q + 1;
  const size_t si = blockIdx.x / unsigned(a.nops);
  const int m = int(blockIdx.x % unsigned(a.nops));
  const size_t nblk = size_t(L) * Q1 * p, ndim = size_t(L + 1) * Q1;
  const EBlk* blk = a.blk + si * nblk;
  const int* dims = a.dims + si * ndim;
  const double* renv = a.env + si * 2 * string_env_complex(L, Q1);
  const double* lenv = renv + ndim * kPairTile;
  double* sweep = a.sweep + size_t(blockIdx.x) * 2 * string_sweep_complex(Q1);
  const double* f = a.f + 2 * size_t(m) * L * p;
  const int s0 = a.sup[2 * m], s1 = a.sup[2 * m + 1];
  const StrWave W{tt[wave], lane & 15, lane >> 4};
  for (int k = s0; k <= s1; ++k) {
    const double* Ein = k == s0 ? lenv + size_t(k - 1) * Q1 * kPairTile : sweep + size_t((k - 1) & 1) * Q1 * kPairTile;
    double* Eout = sweep + size_t(k & 1) * Q1 * kPairTile;
    const int *d0 = dims + size_t(k - 1) * Q1, *d1 = dims + size_t(k) * Q1;
    for (int qq = wave; qq < Q1; qq += 4) {
      const int c = d1[qq];
      pr_d4 cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
      if (c > 0)
        for (int n = 0; n < p && qq - n >= 0; ++n) {
          const int q = qq - n;
          const EBlk A = blk[(size_t(k - 1) * Q1 + q) * p + n];
          const double fr = f[2 * (size_t(k - 1) * p + n)], fi = f[2 * (size_t(k - 1) * p + n) + 1];
          if (!A.a || d0[q] == 0 || (fr == 0.0 && fi == 0.0)) continue;
          pr_d4 tr = {0, 0, 0, 0}, ti = {0, 0, 0, 0};
          W.mul_EA(tr, ti, Ein + size_t(q) * kPairTile, A.r, A);
          W.put_T(tr, ti);
          W.add_AhT(cr, ci, A, c, fr, fi);
        }
      if (k < s1) {
        if (c > 0) W.put_env(Eout + size_t(qq) * kPairTile, c, c, cr, ci);
      } else {
        // tr(E Renv): this lane's E[row][col] with Renv[col][row], inside the sector's extent
        double sr = 0, sim = 0;
        if (c > 0) {
          const double* R = renv + (size_t(k) * Q1 + qq) * kPairTile;
          const int col = W.li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = W.kl + 4 * r;
            if (row < c && col < c) {
              const double rr = R[2 * (col * 16 + row)], ri = R[2 * (col * 16 + row) + 1];
              sr += cr[r] * rr - ci[r] * ri;
              sim += cr[r] * ri + ci[r] * rr;
            }
          }
        }
        for (int o = 32; o > 0; o >>= 1) {
          sr += __shfl_xor(sr, o, 64);
          sim += __shfl_xor(sim, o, 64);
        }
        if (lane == 0) {
          string_part[2 * qq] = sr;
          string_part[2 * qq + 1] = sim;
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    double sr = 0, sim = 0;
    for (int q = 0; q < Q1; ++q) {
      sr += string_part[2 * q];
      sim += string_part[2 * q + 1];
    }
    a.out[2 * size_t(blockIdx.x)] = sr;
    a.out[2 * size_t(blockIdx.x) + 1] = sim;
  }
}

}  // namespace

// Queue the two chain launches of a chunk's narrow states on st; up(list) places a list on the
// device (null: it did not fit, nothing is launched).  a.env, a.sweep and a.out are set by the caller.
template <class Up>
inline hipError_t string_launch(StringTable& tb, StrArgs a, hipStream_t st, Up&& up) {
  const size_t nst = tb.dims.size() / (size_t(a.L + 1) * (a.Q + 1));
  a.blk = up(tb.blk);
  a.dims = up(tb.dims);
  a.f = up(tb.f);
  a.sup = up(tb.sup);
  if (nst == 0 || a.nops == 0 || !a.blk || !a.dims || !a.f || !a.sup || !a.env || !a.sweep || !a.out) return hipSuccess;
  hipLaunchKernelGGL(k_obs_string_env, dim3(unsigned(nst)), dim3(256), 0, st, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(k_obs_string, dim3(unsigned(nst * a.nops)), dim3(256), string_lds_bytes(a.Q + 1), st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ host driver
// Queue the launches of one chunk (called by run_chunk).  Result j of the chunk (complex j of d_out)
// belongs to dests[j]: kind 9, idx = out slot * nops + operator.  The chain states' results come first,
// then the list states' closes.
template <class BE>
void string_chunk(BE& be, int L, int p, int Q, const std::vector<const StateDesc*>& S,
                  const std::vector<size_t>& out_slot, const Strings& sr, double* d_out, const double* one,
                  std::vector<Dest>& dests, Traffic& tr) {
  const int Q1 = Q + 1, B = int(S.size()), nops = sr.nops;
  auto D = [&](int i, int b, int q) { return (q < 0 || q > Q) ? 0 : S[i]->dims[size_t(b) * Q1 + q]; };
  auto A = [&](int i, int k, int q, int n) -> Blk {
    if (q < 0 || n < 0 || n >= p || q + n > Q) return Blk{};
    return S[i]->blk[(size_t(k) * Q1 + q) * p + n];
  };
  auto F = [&](int m, int k, int n) { return sr.f + 2 * ((size_t(m) * L + (k - 1)) * p + n); };
  const bool chain_on = string_chain_enabled();
  std::vector<int> chain, lists;
  for (int i = 0; i < B; ++i) {
    const int widest = *std::max_element(S[i]->dims.begin(), S[i]->dims.end());
    (chain_on && string_chain_fits(widest, Q1) ? chain : lists).push_back(i);
  }

  // ---- narrow states: the tables and two launches
  if (!chain.empty()) {
    StringTable tb;
    double work = 0, elems = 0;
    for (int i : chain) {
      for (int m = 0; m < nops; ++m) dests.push_back(Dest{9, out_slot[i] * nops + m});
      tb.dims.insert(tb.dims.end(), S[i]->dims.begin(), S[i]->dims.end());
      for (int k = 1; k <= L; ++k) {
        int uses = 2;  // a model, not a count: every block in two products per sweep and per operator over it
        for (int m = 0; m < nops; ++m) uses += (sr.a[m] <= k && k <= sr.b[m]) ? 2 : 0;
        for (int q = 0; q <= Q; ++q)
          for (int n = 0; n < p; ++n) {
            const Blk b = A(i, k, q, n);
            tb.blk.push_back(EBlk{b.p, b.r, b.c});
            if (b.p) {
              work += double(b.r) * b.c * (b.r + b.c) * 0.5 * uses;
              elems += double(b.r) * b.c * uses;
            }
          }
      }
    }
    tb.f.assign(sr.f, sr.f + 2 * size_t(nops) * L * p);
    for (int m = 0; m < nops; ++m) {
      tb.sup.push_back(sr.a[m]);
      tb.sup.push_back(sr.b[m]);
    }
    StrArgs a{nullptr, nullptr, nullptr, nullptr, be.alloc(chain.size() * string_env_complex(L, Q1)),
              be.alloc(chain.size() * nops * string_sweep_complex(Q1)), d_out, L, p, Q, nops};
    tr.flops += 8.0 * work;
    tr.bytes += 16.0 * elems;
    tr.launches += 2;
    be.string(tb, a);
  }
  if (lists.empty()) return;

  // ---- the other states: task lists
  std::vector<Task> gt;
  std::vector<Seg> gs;
  auto seg = [&](const double* a, int lda, const double* b, int ldb, int k, int ops, double alpha) {
    gs.push_back(Seg{a, b, lda, ldb, k, ops, alpha});
  };
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
  // C (a.r x a.c) = E (a.r x a.r) A
  auto times = [&](const double* e, const Blk a) {
    double* t = be.alloc(size_t(a.r) * a.c);
    const int s0 = int(gs.size());
    seg(e, a.r, a.p, a.c, a.r, 0, 1.0);
    task(t, a.r, a.c, s0);
    return t;
  };
  const size_t QP = size_t(Q1) * p;
  bool need_i = false;
  for (int m = 0; m < nops; ++m) need_i = need_i || sr.cplx[m];
  const double* ii = nullptr;
  if (need_i) {
    std::vector<double> v{0.0, 1.0};
    ii = be.consts(v);
  }

  // the environments of every bond: Lenv (and J = i Lenv) of the bonds 0..L-1, Renv of the bonds 1..L
  std::vector<std::vector<const double*>> Le(B), Je(B), Re(B);
  for (int i : lists) {
    Le[i].assign(size_t(L + 1) * Q1, nullptr);
    Je[i].assign(size_t(L + 1) * Q1, nullptr);
    Re[i].assign(size_t(L + 1) * Q1, nullptr);
    Le[i][0] = one;
    Je[i][0] = ii;
    Re[i][size_t(L) * Q1 + Q] = one;
  }
  {
    std::vector<std::vector<double*>> T(B), TJ(B), W(B);
    for (int j = 1; j < L; ++j) {
      const int kl = j, kr = L + 1 - j;
      for (int i : lists) {
        T[i].assign(QP, nullptr);
        TJ[i].assign(QP, nullptr);
        W[i].assign(QP, nullptr);
        for (int q = 0; q <= Q; ++q)
          for (int n = 0; n < p && q + n <= Q; ++n) {
            const Blk al = A(i, kl, q, n);
            if (al.p) {
              if (const double* l = Le[i][size_t(kl - 1) * Q1 + q]) T[i][size_t(q) * p + n] = times(l, al);
              if (const double* l = Je[i][size_t(kl - 1) * Q1 + q]) TJ[i][size_t(q) * p + n] = times(l, al);
            }
            const Blk ar = A(i, kr, q, n);
            const double* r = Re[i][size_t(kr) * Q1 + q + n];
            if (ar.p && r) {
              double* w = be.alloc(size_t(ar.r) * ar.c);
              const int s0 = int(gs.size());
              seg(ar.p, ar.c, r, ar.c, ar.c, 0, 1.0);
              task(w, ar.r, ar.c, s0);
              W[i][size_t(q) * p + n] = w;
            }
          }
      }
      launch_gemm();
      for (int i : lists)
        for (int q = 0; q <= Q; ++q) {
          if (const int c = D(i, kl, q)) {
            for (int w = 0; w < 2; ++w) {
              const std::vector<double*>& src = w ? TJ[i] : T[i];
              const int s0 = int(gs.size());
              for (int n = 0; n < p && q - n >= 0; ++n) {
                const double* t = src[size_t(q - n) * p + n];
                if (!t) continue;
                const Blk a = A(i, kl, q - n, n);
                seg(a.p, a.c, t, a.c, a.r, 1, 1.0);
              }
              if (int(gs.size()) == s0) continue;
              double* l = be.alloc(size_t(c) * c);
              task(l, c, c, s0);
              (w ? Je[i] : Le[i])[size_t(kl) * Q1 + q] = l;
            }
          }
          if (const int r = D(i, kr - 1, q)) {
            const int s0 = int(gs.size());
            for (int n = 0; n < p && q + n <= Q; ++n) {
              const double* w = W[i][size_t(q) * p + n];
              if (!w) continue;
              const Blk a = A(i, kr, q, n);
              seg(w, a.c, a.p, a.c, a.c, 2, 1.0);
            }
            if (int(gs.size()) == s0) continue;
            double* rr = be.alloc(size_t(r) * r);
            task(rr, r, r, s0);
            Re[i][size_t(kr - 1) * Q1 + q] = rr;
          }
        }
      launch_gemm();
    }
  }

  // the supports: every operator of every state one site per round
  struct Cur {
    std::vector<const double*> E, F;  // [q] on the bond behind the site; F = i E (non-real tables)
  };
  std::vector<std::vector<Cur>> cur(B, std::vector<Cur>(nops));
  for (int i : lists)
    for (int m = 0; m < nops; ++m) {
      const size_t at = size_t(sr.a[m] - 1) * Q1;
      cur[i][m].E.assign(Le[i].begin() + at, Le[i].begin() + at + Q1);
      if (sr.cplx[m]) cur[i][m].F.assign(Je[i].begin() + at, Je[i].begin() + at + Q1);
    }
  std::vector<std::vector<std::vector<double*>>> T1(B, std::vector<std::vector<double*>>(nops)), T2 = T1;
  for (int r = 1; r <= sr.longest; ++r) {
    for (int i : lists)
      for (int m = 0; m < nops; ++m) {
        const int k = sr.a[m] + r - 1;
        if (k > sr.b[m]) continue;
        T1[i][m].assign(QP, nullptr);
        T2[i][m].assign(QP, nullptr);
        for (int q = 0; q <= Q; ++q)
          for (int n = 0; n < p && q + n <= Q; ++n) {
            const Blk a = A(i, k, q, n);
            const double* f = F(m, k, n);
            if (!a.p || (f[0] == 0.0 && f[1] == 0.0)) continue;
            if (const double* e = cur[i][m].E[q]) T1[i][m][size_t(q) * p + n] = times(e, a);
            if (sr.cplx[m])
              if (const double* e = cur[i][m].F[q]) T2[i][m][size_t(q) * p + n] = times(e, a);
          }
      }
    launch_gemm();
    for (int i : lists)
      for (int m = 0; m < nops; ++m) {
        const int k = sr.a[m] + r - 1;
        if (k > sr.b[m]) continue;
        Cur nx;
        nx.E.assign(Q1, nullptr);
        if (sr.cplx[m]) nx.F.assign(Q1, nullptr);
        for (int w = 0; w < (sr.cplx[m] && k < sr.b[m] ? 2 : 1); ++w)  // (F is not needed behind the last site)
          for (int qq = 0; qq <= Q; ++qq) {
            const int c = D(i, k, qq);
            if (c == 0) continue;
            const int s0 = int(gs.size());
            for (int n = 0; n < p && qq - n >= 0; ++n) {
              const double* f = F(m, k, n);
              const Blk a = A(i, k, qq - n, n);
              const double *t1 = T1[i][m][size_t(qq - n) * p + n], *t2 = T2[i][m][size_t(qq - n) * p + n];
              // E' takes Re f of E A and Im f of F A; F' takes Re f of F A and -Im f of E A
              const double* ta = w ? t2 : t1;
              const double* tb = w ? t1 : t2;
              if (ta && f[0] != 0.0) seg(a.p, a.c, ta, a.c, a.r, 1, f[0]);
              if (tb && f[1] != 0.0) seg(a.p, a.c, tb, a.c, a.r, 1, w ? -f[1] : f[1]);
            }
            if (int(gs.size()) == s0) continue;
            double* e = be.alloc(size_t(c) * c);
            task(e, c, c, s0);
            (w ? nx.F : nx.E)[qq] = e;
          }
        cur[i][m] = std::move(nx);
      }
    launch_gemm();
  }

  // the closes: sum_q tr(E_b[q] Renv_b[q]) = sum conj(Renv_b[q]) . E_b[q]
  std::vector<CTask> ct;
  std::vector<Pair> cp;
  for (int i : lists)
    for (int m = 0; m < nops; ++m) {
      const int p0 = int(cp.size());
      for (int q = 0; q <= Q; ++q) {
        const double *e = cur[i][m].E[q], *rr = Re[i][size_t(sr.b[m]) * Q1 + q];
        if (!e || !rr) continue;
        const long long n = (long long)D(i, sr.b[m], q) * D(i, sr.b[m], q);
        cp.push_back(Pair{rr, e, n, 1.0});
        tr.bytes += 32.0 * double(n);
        tr.flops += 8.0 * double(n);
      }
      ct.push_back(CTask{p0, int(cp.size()) - p0});
      dests.push_back(Dest{9, out_slot[i] * nops + m});
    }
  if (!ct.empty()) {
    ++tr.launches;
    const size_t first = dests.size() - ct.size();
    be.close(ct, cp, d_out ? d_out + 2 * first : nullptr);
  }
}

}  // namespace obs
