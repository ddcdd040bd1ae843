// Energy moments of stored MPS (ocg_observe_moments / ocg_observe_moments_states):
// with H(J, U) = -J K + U D, K = sum_i (a+_i a_{i+1} + a_i a+_{i+1}) and
// D = sum_i n_i (n_i - 1) / 2, the raw numbers
//   norm2 = <s|s>, k1 = <s|K|s>, d1 = <s|D|s>, kk = <s|K K|s>, dd = <s|D D|s>, kd = <s|K D|s>
// of every state of a chunk, from which the caller forms <H>, <H^2> - <H>^2 and
// d<D>/dt for any (J, U).
//
// One left-to-right sweep (no right environments, so any gauge and norm) of the
// environments E[alpha][beta] of two copies of the operator automaton
//   0 nothing yet, 1 a+ placed (a owed), 2 a placed (a+ owed), 3 a K term done, 4 a D term done
// alpha for the left operator of the product, beta for the right one.  E is block
// sparse: block q (the ket sector) is d[q + c] x d[q], c = charge(alpha) + charge(beta).
// At site k
//   E'[alpha'][beta'][q + n] += <m| W[alpha -> alpha'] W[beta -> beta'] |n> A(q + c, m)^H E[alpha][beta][q] A(q, n)
// and after site L the 1 x 1 blocks are the results.  Every W is a monomial: n fixes m.
//
// Two paths, chosen per state by its widest bond sector and the context's Q (so a state's
// numbers do not depend on what else is in the chunk):
//   * energy_lists: two task lists per site, T = E A and E' = sum coef A^H T, on the
//     backend's GEMM, the matrix element on Seg::alpha; environments ping-pong between
//     two buffers per state.
//   * k_obs_energy: states whose sectors are all at most 16 wide (and Q + 1 <= 245, so that
//     the kernel's flags fit the LDS beside its tiles).  One launch per chunk,
//     one workgroup per state, all L sites in the kernel, every block one 16 x 16 MFMA
//     tile, from a per-chunk table of block addresses and dims (no per-site lists).
// Included by observe.hpp after its list types.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace obs {

constexpr int kEnergyMaxOrder = 512;   // the sector orders the list path is offered (as the spectrum's)
constexpr int kEnergyChainOrder = 16;  // states up to this order run on k_obs_energy
constexpr int kEnergyNA = 5;           // automaton states
constexpr int kEnergyNCh = kEnergyNA * kEnergyNA;
constexpr int kEnergyNT = 8;           // transitions
constexpr int kEnergyOut = 6;          // complex results per state: norm2, k1, d1, kk, dd, kd

// site operators: 0 identity, 1 a+, 2 a, 3 n (n - 1) / 2
struct ETrans {
  signed char from, to, op;
};
// the one transition table both paths read
constexpr ETrans kEnergyTrans[kEnergyNT] = {{0, 0, 0}, {0, 1, 1}, {0, 2, 2}, {0, 4, 3},
                                            {1, 3, 2}, {2, 3, 1}, {3, 3, 0}, {4, 4, 0}};
constexpr signed char kEnergyCharge[kEnergyNA] = {0, 1, -1, 0, 0};  // bra sector - ket sector
constexpr signed char kEnergyShift[4] = {0, 1, -1, 0};              // level shift of a site operator
// the channels alpha * 5 + beta of the results, in output order
constexpr signed char kEnergyFinal[kEnergyOut] = {0, 15, 20, 18, 24, 19};

// a channel some result can still be reached from (left D with a right K in progress is never asked for)
__host__ __device__ constexpr bool energy_live(int ch) { return !(ch / kEnergyNA == 4 && ch % kEnergyNA >= 1 && ch % kEnergyNA <= 3); }

inline double energy_op(int op, int n) {
  return op == 0 ? 1.0 : op == 1 ? std::sqrt(double(n + 1)) : op == 2 ? std::sqrt(double(n)) : 0.5 * n * (n - 1.0);
}
// coef[(ta * 8 + tb) * p + n] = <m| W[ta] W[tb] |n>, m = n + shift(ta) + shift(tb); 0: a level leaves 0..p-1
inline std::vector<double> energy_coefs(int p) {
  std::vector<double> c(size_t(kEnergyNT) * kEnergyNT * p, 0.0);
  for (int ta = 0; ta < kEnergyNT; ++ta)
    for (int tb = 0; tb < kEnergyNT; ++tb)
      for (int n = 0; n < p; ++n) {
        const int n1 = n + kEnergyShift[kEnergyTrans[tb].op], m = n1 + kEnergyShift[kEnergyTrans[ta].op];
        if (n1 < 0 || n1 >= p || m < 0 || m >= p) continue;
        c[(size_t(ta) * kEnergyNT + tb) * p + n] = energy_op(kEnergyTrans[tb].op, n) * energy_op(kEnergyTrans[ta].op, n1);
      }
  return c;
}

// OCG_OBS_ENERGY_CHAIN=0: every state on the list path
inline bool energy_chain_enabled() {
  const char* e = std::getenv("OCG_OBS_ENERGY_CHAIN");
  return !(e && e[0] == '0');
}

// ------------------------------------------------------------------ chain kernel
struct EBlk {
  const double* a;  // row-major r x c, interleaved (re, im); null: absent
  int r, c;
};
struct EArgs {
  const EBlk* blk;     // [state][site k - 1][q][n]
  const int* dims;     // [state][bond 0..L][q]
  const double* coef;  // energy_coefs(p)
  double* env;         // [state][2][channel][q] tiles of 16 x 16 complex (ld 16)
  double* out;         // [state][kEnergyOut] complex
  int L, p, Q;
};
struct EnergyTable {
  std::vector<EBlk> blk;
  std::vector<int> dims;
};
constexpr size_t kEnergyTile = 2 * 16 * 16;  // doubles
__host__ __device__ inline size_t energy_env_complex(int Q1) { return size_t(2) * kEnergyNCh * Q1 * (kEnergyTile / 2); }  // per state
inline size_t energy_lds_bytes(int Q1) { return sizeof(int) * 2 * kEnergyNCh * size_t(Q1); }  // the flags (dynamic)
constexpr size_t kEnergyLdsStatic = 4 * kEnergyTile * sizeof(double);                             // the four T tiles
constexpr size_t kEnergyLdsLimit = size_t(64) << 10;  // what a launch may take without opting in to more
// the chain kernel can take a state: every sector fits a tile and the flags of its Q + 1 sectors fit the LDS
inline bool energy_chain_fits(int widest, int Q1) {
  return widest <= kEnergyChainOrder && kEnergyLdsStatic + energy_lds_bytes(Q1) <= kEnergyLdsLimit;
}
inline int energy_live_channels() {
  int n = 0;
  for (int ch = 0; ch < kEnergyNCh; ++ch) n += energy_live(ch) ? 1 : 0;
  return n;
}

namespace {

typedef double en_d4 __attribute__((ext_vector_type(4)));

// a wave's own LDS tile: its stores before, its loads after
__device__ inline void energy_wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One workgroup of four waves = one state.  Output channel ch' belongs to wave ch' % 4.
// Per output block the wave walks the transitions into it in table order; for each it
// forms T = E A (operands from the workspace and the state, v_mfma_f64_16x16x4f64 as
// k_obs_gemm: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], results col l & 15,
// rows (l >> 4) + 4 r), passes T through its LDS tile and accumulates coef A^H T.  Which
// blocks of a bond exist is kept in LDS flags; the barrier at the end of a site is the
// only synchronisation between waves.
__global__ __launch_bounds__(256) void k_obs_energy(const EArgs a) {
  __shared__ double tt[4][kEnergyTile];
  extern __shared__ int energy_flags[];  // [2][channel][q]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Q1 = a.Q + 1, li = lane & 15, kl = lane >> 4;
  const size_t si = blockIdx.x;
  const EBlk* blk = a.blk + si * size_t(a.L) * Q1 * a.p;
  const int* dims = a.dims + si * size_t(a.L + 1) * Q1;
  double* env = a.env + si * 2 * energy_env_complex(Q1);
  double* T = tt[wave];
  const int nfl = kEnergyNCh * Q1;
  for (int j = tid; j < 2 * nfl; j += 256) energy_flags[j] = 0;
  __syncthreads();
  if (tid == 0) {  // E[0][0][q = 0] of bond 0 is [1]
    env[0] = 1.0;
    env[1] = 0.0;
    energy_flags[0] = 1;
  }
  __syncthreads();
  for (int k = 1; k <= a.L; ++k) {
    const int cur = (k - 1) & 1, nxt = k & 1;
    const int* fcur = energy_flags + cur * nfl;
    int* fnxt = energy_flags + nxt * nfl;
    const double* ecur = env + size_t(cur) * kEnergyNCh * Q1 * kEnergyTile;
    double* enxt = env + size_t(nxt) * kEnergyNCh * Q1 * kEnergyTile;
    const int* d0 = dims + size_t(k - 1) * Q1;
    const int* d1 = dims + size_t(k) * Q1;
    const EBlk* bk = blk + size_t(k - 1) * Q1 * a.p;
    for (int cho = wave; cho < kEnergyNCh; cho += 4) {
      const int alo = cho / kEnergyNA, beo = cho % kEnergyNA;
      const int co = kEnergyCharge[alo] + kEnergyCharge[beo];
      for (int qko = 0; qko < Q1; ++qko) {
        const int qbo = qko + co;
        const int ck = d1[qko], cb = (qbo >= 0 && qbo < Q1) ? d1[qbo] : 0;
        bool any = false;
        en_d4 cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        if (energy_live(cho) && ck > 0 && cb > 0) {
          for (int ta = 0; ta < kEnergyNT; ++ta) {
            if (kEnergyTrans[ta].to != alo) continue;
            for (int tb = 0; tb < kEnergyNT; ++tb) {
              if (kEnergyTrans[tb].to != beo) continue;
              const int al = kEnergyTrans[ta].from, be = kEnergyTrans[tb].from, ch = al * kEnergyNA + be;
              const int c0 = kEnergyCharge[al] + kEnergyCharge[be];
              const int sh = kEnergyShift[kEnergyTrans[ta].op] + kEnergyShift[kEnergyTrans[tb].op];
              for (int n = 0; n < a.p; ++n) {
                const double coef = a.coef[(size_t(ta) * kEnergyNT + tb) * a.p + n];
                const int qk = qko - n, qb = qk + c0, m = n + sh;
                if (coef == 0.0 || qk < 0 || qb < 0 || qb >= Q1 || m < 0 || m >= a.p) continue;
                if (!fcur[ch * Q1 + qk]) continue;
                const EBlk Ak = bk[size_t(qk) * a.p + n], Ab = bk[size_t(qb) * a.p + m];
                if (!Ak.a || !Ab.a) continue;
                const int rk = d0[qk], rb = d0[qb];
                // T = E (rb x rk) Ak (rk x ck)
                const double* e = ecur + (size_t(ch) * Q1 + qk) * kEnergyTile;
                en_d4 tr = {0, 0, 0, 0}, ti = {0, 0, 0, 0};
                for (int k0 = 0; k0 < rk; k0 += 4) {
                  const int kk = k0 + kl;
                  double are = 0, aim = 0, bre = 0, bim = 0;
                  if (kk < rk && li < rb) {
                    are = e[2 * (li * 16 + kk)];
                    aim = e[2 * (li * 16 + kk) + 1];
                  }
                  if (kk < rk && li < ck) {
                    bre = Ak.a[2 * (size_t(kk) * ck + li)];
                    bim = Ak.a[2 * (size_t(kk) * ck + li) + 1];
                  }
                  tr = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bre, tr, 0, 0, 0);
                  tr = __builtin_amdgcn_mfma_f64_16x16x4f64(-aim, bim, tr, 0, 0, 0);
                  ti = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bim, ti, 0, 0, 0);
                  ti = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, bre, ti, 0, 0, 0);
                }
                energy_wave_order();  // the loads of the previous T are done
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  T[2 * ((kl + 4 * r) * 16 + li)] = tr[r];
                  T[2 * ((kl + 4 * r) * 16 + li) + 1] = ti[r];
                }
                energy_wave_order();
                // E' += coef Ab^H (cb x rb) T (rb x ck)
                for (int k0 = 0; k0 < rb; k0 += 4) {
                  const int kk = k0 + kl;
                  double are = 0, aim = 0, bre = 0, bim = 0;
                  if (kk < rb) {
                    if (li < cb) {
                      are = Ab.a[2 * (size_t(kk) * cb + li)] * coef;
                      aim = -Ab.a[2 * (size_t(kk) * cb + li) + 1] * coef;
                    }
                    bre = T[2 * (kk * 16 + li)];
                    bim = T[2 * (kk * 16 + li) + 1];
                  }
                  cr = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bre, cr, 0, 0, 0);
                  cr = __builtin_amdgcn_mfma_f64_16x16x4f64(-aim, bim, cr, 0, 0, 0);
                  ci = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bim, ci, 0, 0, 0);
                  ci = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, bre, ci, 0, 0, 0);
                }
                any = true;
              }
            }
          }
        }
        if (any && li < ck) {
          double* o = enxt + (size_t(cho) * Q1 + qko) * kEnergyTile;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = kl + 4 * r;
            if (row < cb) {
              o[2 * (row * 16 + li)] = cr[r];
              o[2 * (row * 16 + li) + 1] = ci[r];
            }
          }
        }
        if (lane == 0) fnxt[cho * Q1 + qko] = any ? 1 : 0;
      }
    }
    __syncthreads();
  }
  if (tid < kEnergyOut) {
    const int ch = kEnergyFinal[tid], buf = a.L & 1;
    const bool have = energy_flags[buf * nfl + ch * Q1 + a.Q] != 0;
    const double* e = env + (size_t(buf) * kEnergyNCh * Q1 + size_t(ch) * Q1 + a.Q) * kEnergyTile;
    double* o = a.out + 2 * (si * kEnergyOut + tid);
    o[0] = have ? e[0] : 0.0;
    o[1] = have ? e[1] : 0.0;
  }
}

}  // namespace

// Queue the chain launch of a chunk's narrow states on st; up(list) places a list on the
// device (null: it did not fit, nothing is launched).  a.env and a.out are set by the caller.
template <class Up>
inline hipError_t energy_launch(EnergyTable& tb, EArgs a, std::vector<double>& coef, hipStream_t st, Up&& up) {
  const size_t nst = tb.dims.size() / (size_t(a.L + 1) * (a.Q + 1));
  a.blk = up(tb.blk);
  a.dims = up(tb.dims);
  a.coef = up(coef);
  if (nst == 0 || !a.blk || !a.dims || !a.coef || !a.env || !a.out) return hipSuccess;
  hipLaunchKernelGGL(k_obs_energy, dim3(unsigned(nst)), dim3(256), energy_lds_bytes(a.Q + 1), st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ host driver
// Queue the moment launches of one chunk (called by run_chunk).
// Result j of the chunk (complex j of d_out) belongs to dests[j]: kind 4 a real moment,
// kind 5 <K D>, idx into the [nt][7] output.  The chain states' results come first, then
// the list states' closes.
template <class BE>
void energy_chunk(BE& be, int L, int p, int Q, const std::vector<const StateDesc*>& S,
                  const std::vector<size_t>& out_slot, double* d_out, const double* one, std::vector<Dest>& dests,
                  Traffic& tr) {
  const int Q1 = Q + 1, B = int(S.size());
  auto D = [&](int i, int b, int q) { return (q < 0 || q > Q) ? 0 : S[i]->dims[size_t(b) * Q1 + q]; };
  auto A = [&](int i, int k, int q, int n) -> Blk {
    if (q < 0 || n < 0 || n >= p || q + n > Q) return Blk{};
    return S[i]->blk[(size_t(k) * Q1 + q) * p + n];
  };
  auto push_dests = [&](size_t o) {
    for (int j = 0; j < kEnergyOut; ++j) dests.push_back(Dest{j < 5 ? 4 : 5, o * 7 + size_t(j)});
  };
  std::vector<double> coef = energy_coefs(p);
  const bool chain_on = energy_chain_enabled();
  std::vector<int> chain, lists;
  for (int i = 0; i < B; ++i) {
    const int widest = *std::max_element(S[i]->dims.begin(), S[i]->dims.end());
    (chain_on && energy_chain_fits(widest, Q1) ? chain : lists).push_back(i);
  }

  // ---- narrow states: the table and one launch
  if (!chain.empty()) {
    EnergyTable tb;
    double work = 0, elems = 0;
    for (int i : chain) {
      push_dests(out_slot[i]);
      tb.dims.insert(tb.dims.end(), S[i]->dims.begin(), S[i]->dims.end());
      for (int k = 1; k <= L; ++k)
        for (int q = 0; q <= Q; ++q)
          for (int n = 0; n < p; ++n) {
            const Blk b = A(i, k, q, n);
            tb.blk.push_back(EBlk{b.p, b.r, b.c});
            if (b.p) {
              work += double(b.r) * b.c * (b.r + b.c);
              elems += double(b.r) * b.c;
            }
          }
    }
    EArgs a{nullptr, nullptr, nullptr, be.alloc(chain.size() * energy_env_complex(Q1)), d_out, L, p, Q};
    // a model, not a count (the host builds no lists here): every block as the ket and as the bra operand of
    // one transition per live channel
    const int nlive = energy_live_channels();
    tr.flops += 8.0 * work * nlive;
    tr.bytes += 16.0 * 2 * elems * nlive;
    ++tr.launches;
    be.energy(tb, a, coef);
  }
  if (lists.empty()) return;

  // ---- the other states: two task lists per site
  const size_t first = dests.size();
  struct Per {
    double *e[2], *t;
    std::vector<double*> cur, nxt;  // [channel * Q1 + ket sector]
  };
  std::vector<Per> per(B);
  for (int i : lists) {
    size_t ecap = 1, tcap = 1;
    for (int b = 0; b <= L; ++b) {
      size_t es = 0, ts = 0;
      for (int ch = 0; ch < kEnergyNCh; ++ch) {
        if (!energy_live(ch)) continue;
        const int c = kEnergyCharge[ch / kEnergyNA] + kEnergyCharge[ch % kEnergyNA];
        for (int q = 0; q <= Q; ++q) {
          es += size_t(D(i, b, q + c)) * D(i, b, q);
          for (int n = 0; n < p && b < L; ++n) ts += size_t(D(i, b, q + c)) * D(i, b + 1, q + n);
        }
      }
      ecap = std::max(ecap, es);
      tcap = std::max(tcap, ts);
    }
    Per& P = per[i];
    P.e[0] = be.alloc(2 * ecap + tcap);
    P.e[1] = P.e[0] + 2 * ecap;
    P.t = P.e[1] + 2 * ecap;
    P.cur.assign(size_t(kEnergyNCh) * Q1, nullptr);
    P.cur[0] = const_cast<double*>(one);
  }
  std::vector<Task> gt1, gt2;
  std::vector<Seg> gs1, gs2;
  auto task = [&](std::vector<Task>& gt, const std::vector<Seg>& gs, double* C, int m, int n, int s0) {
    const int ns = int(gs.size()) - s0;
    gt.push_back(Task{C, n, m, n, s0, ns, 0});
    for (int s = s0; s < s0 + ns; ++s) {
      tr.flops += 8.0 * m * n * gs[s].k;
      tr.bytes += 16.0 * (double(m) * gs[s].k + double(gs[s].k) * n);
    }
    tr.bytes += 16.0 * m * n;
  };
  std::vector<double*> T;  // [(channel * Q1 + ket sector) * p + n] of the state in hand
  for (int k = 1; k <= L; ++k) {
    for (int i : lists) {
      Per& P = per[i];
      size_t eoff = 0, toff = 0;
      double* ebuf = P.e[k & 1];
      T.assign(size_t(kEnergyNCh) * Q1 * p, nullptr);
      P.nxt.assign(size_t(kEnergyNCh) * Q1, nullptr);
      for (int cho = 0; cho < kEnergyNCh; ++cho) {
        if (!energy_live(cho)) continue;
        const int alo = cho / kEnergyNA, beo = cho % kEnergyNA;
        const int co = kEnergyCharge[alo] + kEnergyCharge[beo];
        for (int qko = 0; qko <= Q; ++qko) {
          const int ck = D(i, k, qko), cb = D(i, k, qko + co);
          if (ck == 0 || cb == 0) continue;
          const int s0 = int(gs2.size());
          for (int ta = 0; ta < kEnergyNT; ++ta) {
            if (kEnergyTrans[ta].to != alo) continue;
            for (int tb = 0; tb < kEnergyNT; ++tb) {
              if (kEnergyTrans[tb].to != beo) continue;
              const int al = kEnergyTrans[ta].from, bt = kEnergyTrans[tb].from, ch = al * kEnergyNA + bt;
              const int c0 = kEnergyCharge[al] + kEnergyCharge[bt];
              const int sh = kEnergyShift[kEnergyTrans[ta].op] + kEnergyShift[kEnergyTrans[tb].op];
              for (int n = 0; n < p; ++n) {
                const double cf = coef[(size_t(ta) * kEnergyNT + tb) * p + n];
                const int qk = qko - n, qb = qk + c0, m = n + sh;
                if (cf == 0.0 || qk < 0 || qb < 0 || qb > Q) continue;
                const double* e = P.cur[size_t(ch) * Q1 + qk];
                if (!e) continue;
                const Blk Ak = A(i, k, qk, n), Ab = A(i, k, qb, m);
                if (!Ak.p || !Ab.p) continue;
                double*& t = T[(size_t(ch) * Q1 + qk) * p + n];
                if (!t) {  // T = E (rb x rk) Ak (rk x ck), once for all that read it
                  t = P.t + 2 * toff;
                  toff += size_t(Ab.r) * Ak.c;
                  const int t0 = int(gs1.size());
                  gs1.push_back(Seg{e, Ak.p, Ak.r, Ak.c, Ak.r, 0, 1.0});
                  task(gt1, gs1, t, Ab.r, Ak.c, t0);
                }
                gs2.push_back(Seg{Ab.p, t, Ab.c, ck, Ab.r, 1, cf});
              }
            }
          }
          if (int(gs2.size()) == s0) continue;
          double* o = ebuf + 2 * eoff;
          eoff += size_t(cb) * ck;
          task(gt2, gs2, o, cb, ck, s0);
          P.nxt[size_t(cho) * Q1 + qko] = o;
        }
      }
      P.cur.swap(P.nxt);
    }
    if (!gt1.empty()) ++tr.launches;
    be.gemm(gt1, gs1);
    if (!gt2.empty()) ++tr.launches;
    be.gemm(gt2, gs2);
  }
  std::vector<CTask> ct;
  std::vector<Pair> cp;
  for (int i : lists) {
    push_dests(out_slot[i]);
    for (int j = 0; j < kEnergyOut; ++j) {
      const int p0 = int(cp.size());
      if (const double* e = per[i].cur[size_t(kEnergyFinal[j]) * Q1 + Q]) cp.push_back(Pair{one, e, 1, 1.0});
      ct.push_back(CTask{p0, int(cp.size()) - p0});
      tr.bytes += 32.0;
    }
  }
  ++tr.launches;
  be.close(ct, cp, d_out ? d_out + 2 * first : nullptr);
}

}  // namespace obs
