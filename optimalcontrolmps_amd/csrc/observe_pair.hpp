// Transition matrix elements between two stored MPS (ocg_observe_pairs /
// ocg_observe_pairs_states): for every pair (bra x, ket y) of a chunk the raw numbers
//   ovl = <x|y>,  occ[k][n] = <x|P_k(n)|y>  (P_k(n) the projector on occupation n of site k),
//   hop[b][0] = <x|a+_b a_{b+1}|y>,  hop[b][1] = <x|a_b a+_{b+1}|y>   (a, a+ cut at p levels),
// from which the caller forms <x|n_k|y>, <x|D|y> and <x|K|y>.
//
// Gauge free, environments from both ends, all rectangular (block q is d_x[b][q] x d_y[b][q]):
//   R_{k-1}[q] = sum_n Ax(q, n) R_k[q + n] Ay(q, n)^H          (the conjugate of the right environment)
//   L_k[q + n] = sum_n Ax(q, n)^H L_{k-1}[q] Ay(q, n)
// and with T(q, n) = L_{k-1}[q] Ay(q, n), X(q, n) = Ax(q, n) R_k[q + n]
//   occ[k][n]  = sum_q sum conj(X(q, n)) . T(q, n),     ovl = L_L[Q].
// A hopping term opens an environment at site k that lives for one site, kept by ket sector s:
//   C_k[s + n] = sum_n sqrt(n + 1) Ax(s, n + 1)^H T(s, n)     d_x[k][s + n + 1] x d_y[k][s + n]
//   G_k[s + n] = sum_n sqrt(n)     Ax(s, n - 1)^H T(s, n)     d_x[k][s + n - 1] x d_y[k][s + n]
// and closes at site k + 1:
//   hop[k][0] = sum sqrt(n)     conj(X(s + 1, n - 1)) . (C_k[s] Ay(s, n))
//   hop[k][1] = sum sqrt(n + 1) conj(X(s - 1, n + 1)) . (G_k[s] Ay(s, n)).
// A sector that only one of the two states has gives no block and so contributes nothing.
//
// Two paths, chosen per pair by the widest bond sector of both states and the context's p and Q
// (so a pair's numbers do not depend on what else is in the chunk):
//   * pair_lists: the right sweep (two GEMM launches per site k = L..2), then per site of the left sweep
//     the products (T, X and the open environments times Ay), the new environments, and the closes.
//     Launches of one chunk, for L >= 2: 5 L - 2 when occ or hop is wanted (2 (L - 1) + 3 L),
//     2 L + 1 for ovl alone (no right sweep; one close launch at site L).
//   * k_obs_pair: pairs whose sectors are all at most 16 wide (and whose per-sector partial closes,
//     2 (p + 2) (Q + 1) complex, fit the LDS beside the tiles).  One launch per chunk, one
//     workgroup per pair, both sweeps and all closes in the kernel, every block one 16 x 16 MFMA
//     tile, from a per-chunk table of block addresses and dims.  A block of an environment exists
//     where both states have the sector; one nothing contributes to is a zero tile.
// The two paths sum in different orders: they agree to rounding, not bit for bit.
// Included by observe.hpp after observe_energy.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace obs {

constexpr int kPairMaxOrder = 512;   // the sector orders the list path is offered
constexpr int kPairChainOrder = 16;  // pairs up to this order run on k_obs_pair
constexpr size_t kPairTile = 2 * 16 * 16;  // doubles

// complex results of one pair, in the order ovl, occ[L][p], hop[L - 1][2]
__host__ __device__ inline size_t pair_outputs(int L, int p) { return 1 + size_t(L) * p + 2 * size_t(L > 1 ? L - 1 : 0); }

// OCG_OBS_PAIR_CHAIN=0: every pair on the list path
inline bool pair_chain_enabled() {
  const char* e = std::getenv("OCG_OBS_PAIR_CHAIN");
  return !(e && e[0] == '0');
}

// ------------------------------------------------------------------ chain kernel
struct PArgs {
  const EBlk* blk;  // [pair][x, y][site k - 1][q][n]
  const int* dims;  // [pair][x, y][bond 0..L][q]
  double* env;      // [pair]: R of the bonds 0..L, then L, C, G of two bonds; tiles of 16 x 16 complex (ld 16)
  double* out;      // [pair][pair_outputs] complex
  int L, p, Q;
  int occ, hop;  // what is wanted beside ovl
};
struct PairTable {
  std::vector<EBlk> blk;
  std::vector<int> dims;
};
__host__ __device__ inline size_t pair_env_tiles(int L, int Q1) { return (size_t(L) + 1 + 6) * Q1; }  // per pair
__host__ __device__ inline size_t pair_env_complex(int L, int Q1) { return pair_env_tiles(L, Q1) * (kPairTile / 2); }
inline size_t pair_lds_bytes(int p, int Q1) { return sizeof(double) * 2 * 2 * size_t(p + 2) * Q1; }  // partial closes (dynamic)
constexpr size_t kPairLdsStatic = 4 * kPairTile * sizeof(double);                                    // the four T tiles
// the chain kernel can take a pair: every sector of both states fits a tile, the partial closes fit the LDS
// and a site's p + 2 results have a thread each
inline bool pair_chain_fits(int widest, int p, int Q1) {
  return widest <= kPairChainOrder && p + 2 <= 256 && kPairLdsStatic + pair_lds_bytes(p, Q1) <= kEnergyLdsLimit;
}

namespace {

typedef double pr_d4 __attribute__((ext_vector_type(4)));

// C += A B on v_mfma_f64_16x16x4f64 over K in steps of 4: fa(kk, re, im) gives this lane's A[lane & 15][kk],
// fb(kk, re, im) its B[kk][lane & 15] (both leave 0 outside the operand); results col lane & 15, rows (lane >> 4) + 4 r
template <class FA, class FB>
__device__ inline void pair_mma(pr_d4& cr, pr_d4& ci, int K, int kl, FA&& fa, FB&& fb) {
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int kk = k0 + kl;
    double are = 0, aim = 0, bre = 0, bim = 0;
    if (kk < K) {
      fa(kk, are, aim);
      fb(kk, bre, bim);
    }
    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bre, cr, 0, 0, 0);
    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(-aim, bim, cr, 0, 0, 0);
    ci = __builtin_amdgcn_mfma_f64_16x16x4f64(are, bim, ci, 0, 0, 0);
    ci = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, bre, ci, 0, 0, 0);
  }
}

// the wave's sum of w conj(x) . t over the tile, on every lane (a fixed shuffle tree)
__device__ inline void pair_dot(const pr_d4& xr, const pr_d4& xi, const pr_d4& tr, const pr_d4& ti, double w, double& re,
                                double& im) {
  double sr = 0, si = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sr += xr[r] * tr[r] + xi[r] * ti[r];
    si += xr[r] * ti[r] - xi[r] * tr[r];
  }
  for (int o = 32; o > 0; o >>= 1) {
    sr += __shfl_xor(sr, o, 64);
    si += __shfl_xor(si, o, 64);
  }
  re += w * sr;
  im += w * si;
}

// One workgroup of four waves = one pair.  Sector q of a bond belongs to wave q % 4: in the right sweep the
// block R_{k-1}[q], in the left sweep everything that ends in ket sector q of bond k: L_k[q], C_k[q], G_k[q]
// and the partial closes of site k.  A product that feeds a second one passes through the wave's LDS tile; a
// product that is closed stays in the accumulators (X and T have the same lane layout).  The partial closes
// of a site are summed over the sectors in sector order by one thread per result after the site's barrier,
// which is the only synchronisation between waves; the partials alternate between two buffers.
__global__ __launch_bounds__(256) void k_obs_pair(const PArgs a) {
  __shared__ double tt[4][kPairTile];
  extern __shared__ double pair_part[];  // [2][p + 2][q] complex
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = a.L, p = a.p, Q1 = a.Q + 1, li = lane & 15, kl = lane >> 4;
  const size_t si = blockIdx.x;
  const size_t nblk = size_t(L) * Q1 * p, ndim = size_t(L + 1) * Q1;
  const EBlk* bx = a.blk + si * 2 * nblk;
  const EBlk* by = bx + nblk;
  const int* dx = a.dims + si * 2 * ndim;
  const int* dy = dx + ndim;
  double* renv = a.env + si * 2 * pair_env_complex(L, Q1);
  double* lenv = renv + ndim * kPairTile;  // [L, C, G][bond parity][q]
  double* out = a.out + 2 * si * pair_outputs(L, p);
  double* T = tt[wave];
  const bool closes = a.occ || a.hop;
  const int npart = (p + 2) * Q1;

  auto tile_a = [&](const double* t, int m, double& re, double& im, int kk) {  // A = a tile (ld 16), m rows
    if (li < m) {
      re = t[2 * (li * 16 + kk)];
      im = t[2 * (li * 16 + kk) + 1];
    }
  };
  auto tile_b = [&](const double* t, int n, double& re, double& im, int kk) {  // B = a tile (ld 16), n cols
    if (li < n) {
      re = t[2 * (kk * 16 + li)];
      im = t[2 * (kk * 16 + li) + 1];
    }
  };
  auto put_T = [&](const pr_d4& tr, const pr_d4& ti) {
    energy_wave_order();  // the loads of the previous T are done
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T[2 * ((kl + 4 * r) * 16 + li)] = tr[r];
      T[2 * ((kl + 4 * r) * 16 + li) + 1] = ti[r];
    }
    energy_wave_order();
  };
  auto put_env = [&](double* o, int m, int n, const pr_d4& cr, const pr_d4& ci) {
    if (li >= n) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = kl + 4 * r;
      if (row < m) {
        o[2 * (row * 16 + li)] = cr[r];
        o[2 * (row * 16 + li) + 1] = ci[r];
      }
    }
  };
  // C += alpha A^H T: A a stored r x m block, T the wave's tile (r x n)
  auto add_AhT = [&](pr_d4& cr, pr_d4& ci, const EBlk A, int n, double alpha) {
    pair_mma(cr, ci, A.r, kl,
             [&](int kk, double& re, double& im) {
               if (li < A.c) {
                 re = A.a[2 * (size_t(kk) * A.c + li)] * alpha;
                 im = -A.a[2 * (size_t(kk) * A.c + li) + 1] * alpha;
               }
             },
             [&](int kk, double& re, double& im) { tile_b(T, n, re, im, kk); });
  };
  // C = E A: E a tile (m x A.r), A a stored block
  auto mul_EA = [&](pr_d4& cr, pr_d4& ci, const double* E, int m, const EBlk A) {
    pair_mma(cr, ci, A.r, kl, [&](int kk, double& re, double& im) { tile_a(E, m, re, im, kk); },
             [&](int kk, double& re, double& im) {
               if (li < A.c) {
                 re = A.a[2 * (size_t(kk) * A.c + li)];
                 im = A.a[2 * (size_t(kk) * A.c + li) + 1];
               }
             });
  };
  // C = A R: A a stored block, R a tile (A.c x n)
  auto mul_AR = [&](pr_d4& cr, pr_d4& ci, const EBlk A, const double* R, int n) {
    pair_mma(cr, ci, A.c, kl,
             [&](int kk, double& re, double& im) {
               if (li < A.r) {
                 re = A.a[2 * (size_t(li) * A.c + kk)];
                 im = A.a[2 * (size_t(li) * A.c + kk) + 1];
               }
             },
             [&](int kk, double& re, double& im) { tile_b(R, n, re, im, kk); });
  };

  // ---- right sweep: R of the bonds L..1
  if (closes) {
    if (tid == 0) {
      double* r = renv + (size_t(L) * Q1 + a.Q) * kPairTile;
      r[0] = 1.0;
      r[1] = 0.0;
    }
    __syncthreads();
    for (int k = L; k >= 2; --k) {
      const int *dx0 = dx + size_t(k - 1) * Q1, *dy0 = dy + size_t(k - 1) * Q1;
      for (int q = wave; q < Q1; q += 4) {
        const int rx = dx0[q], ry = dy0[q];
        if (rx == 0 || ry == 0) continue;
        pr_d4 cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        for (int n = 0; n < p && q + n < Q1; ++n) {
          const EBlk Ax = bx[(size_t(k - 1) * Q1 + q) * p + n], Ay = by[(size_t(k - 1) * Q1 + q) * p + n];
          if (!Ax.a || !Ay.a) continue;
          pr_d4 wr = {0, 0, 0, 0}, wi = {0, 0, 0, 0};
          mul_AR(wr, wi, Ax, renv + (size_t(k) * Q1 + q + n) * kPairTile, Ay.c);
          put_T(wr, wi);
          // R' += W (rx x cy) Ay^H (cy x ry)
          pair_mma(cr, ci, Ay.c, kl, [&](int kk, double& re, double& im) { tile_a(T, rx, re, im, kk); },
                   [&](int kk, double& re, double& im) {
                     if (li < ry) {
                       re = Ay.a[2 * (size_t(li) * Ay.c + kk)];
                       im = -Ay.a[2 * (size_t(li) * Ay.c + kk) + 1];
                     }
                   });
        }
        put_env(renv + (size_t(k - 1) * Q1 + q) * kPairTile, rx, ry, cr, ci);
      }
      __syncthreads();
    }
  }

  // ---- left sweep
  if (tid == 0) {  // L_0[0] = [1]
    lenv[0] = 1.0;
    lenv[1] = 0.0;
  }
  __syncthreads();
  for (int k = 1; k <= L; ++k) {
    const int cur = (k - 1) & 1, nxt = k & 1;
    const double *Lc = lenv + size_t(0 + cur) * Q1 * kPairTile, *Cc = lenv + size_t(2 + cur) * Q1 * kPairTile,
                 *Gc = lenv + size_t(4 + cur) * Q1 * kPairTile;
    double *Ln = lenv + size_t(0 + nxt) * Q1 * kPairTile, *Cn = lenv + size_t(2 + nxt) * Q1 * kPairTile,
           *Gn = lenv + size_t(4 + nxt) * Q1 * kPairTile;
    const int *dx0 = dx + size_t(k - 1) * Q1, *dy0 = dy + size_t(k - 1) * Q1;
    const int *dx1 = dx + size_t(k) * Q1, *dy1 = dy + size_t(k) * Q1;
    const EBlk *bkx = bx + size_t(k - 1) * Q1 * p, *bky = by + size_t(k - 1) * Q1 * p;
    double* part = pair_part + size_t(2) * nxt * npart;
    const bool open = a.hop && k < L, shut = a.hop && k >= 2;
    for (int qq = wave; qq < Q1; qq += 4) {
      const int cy = dy1[qq], cx = dx1[qq];
      const int cxp = qq + 1 < Q1 ? dx1[qq + 1] : 0, cxm = qq >= 1 ? dx1[qq - 1] : 0;
      const double* R = renv + (size_t(k) * Q1 + qq) * kPairTile;
      pr_d4 lr = {0, 0, 0, 0}, lim = {0, 0, 0, 0}, cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0}, gr = {0, 0, 0, 0},
            gi = {0, 0, 0, 0};
      double h0r = 0, h0i = 0, h1r = 0, h1i = 0;
      for (int n = 0; n < p; ++n) {
        const int q = qq - n;
        double ore = 0, oim = 0;
        if (q >= 0 && cy > 0) {
          const int rx = dx0[q], ry = dy0[q];
          const EBlk Ay = bky[size_t(q) * p + n];
          if (Ay.a && rx > 0) {
            pr_d4 tr = {0, 0, 0, 0}, ti = {0, 0, 0, 0};
            mul_EA(tr, ti, Lc + size_t(q) * kPairTile, rx, Ay);
            put_T(tr, ti);
            const EBlk Ax = bkx[size_t(q) * p + n];
            if (Ax.a) {
              add_AhT(lr, lim, Ax, cy, 1.0);
              if (a.occ) {
                pr_d4 xr = {0, 0, 0, 0}, xi = {0, 0, 0, 0};
                mul_AR(xr, xi, Ax, R, cy);
                pair_dot(xr, xi, tr, ti, 1.0, ore, oim);
              }
            }
            if (open && n + 1 < p) {
              const EBlk Axp = bkx[size_t(q) * p + n + 1];
              if (Axp.a) add_AhT(cr, ci, Axp, cy, sqrt(double(n + 1)));
            }
            if (open && n >= 1) {
              const EBlk Axm = bkx[size_t(q) * p + n - 1];
              if (Axm.a) add_AhT(gr, gi, Axm, cy, sqrt(double(n)));
            }
          }
          if (shut && Ay.a) {
            // a+ on the site before: the bra came in one sector above, its level here is n - 1
            if (n >= 1 && q + 1 < Q1 && dx0[q + 1] > 0) {
              const EBlk Ax = bkx[size_t(q + 1) * p + n - 1];
              if (Ax.a) {
                pr_d4 tr = {0, 0, 0, 0}, ti = {0, 0, 0, 0}, xr = {0, 0, 0, 0}, xi = {0, 0, 0, 0};
                mul_EA(tr, ti, Cc + size_t(q) * kPairTile, dx0[q + 1], Ay);
                mul_AR(xr, xi, Ax, R, cy);
                pair_dot(xr, xi, tr, ti, sqrt(double(n)), h0r, h0i);
              }
            }
            // a on the site before: the bra came in one sector below, its level here is n + 1
            if (n + 1 < p && q >= 1 && dx0[q - 1] > 0) {
              const EBlk Ax = bkx[size_t(q - 1) * p + n + 1];
              if (Ax.a) {
                pr_d4 tr = {0, 0, 0, 0}, ti = {0, 0, 0, 0}, xr = {0, 0, 0, 0}, xi = {0, 0, 0, 0};
                mul_EA(tr, ti, Gc + size_t(q) * kPairTile, dx0[q - 1], Ay);
                mul_AR(xr, xi, Ax, R, cy);
                pair_dot(xr, xi, tr, ti, sqrt(double(n + 1)), h1r, h1i);
              }
            }
          }
        }
        if (lane == 0) {
          part[2 * (n * Q1 + qq)] = ore;
          part[2 * (n * Q1 + qq) + 1] = oim;
        }
      }
      if (lane == 0) {
        part[2 * (p * Q1 + qq)] = h0r;
        part[2 * (p * Q1 + qq) + 1] = h0i;
        part[2 * ((p + 1) * Q1 + qq)] = h1r;
        part[2 * ((p + 1) * Q1 + qq) + 1] = h1i;
      }
      if (cy > 0) {
        if (cx > 0) put_env(Ln + size_t(qq) * kPairTile, cx, cy, lr, lim);
        if (open && cxp > 0) put_env(Cn + size_t(qq) * kPairTile, cxp, cy, cr, ci);
        if (open && cxm > 0) put_env(Gn + size_t(qq) * kPairTile, cxm, cy, gr, gi);
      }
    }
    __syncthreads();
    if (tid < p + 2) {
      double sr = 0, sim = 0;
      for (int q = 0; q < Q1; ++q) {
        sr += part[2 * (tid * Q1 + q)];
        sim += part[2 * (tid * Q1 + q) + 1];
      }
      double* o = nullptr;
      if (tid < p) {
        if (a.occ) o = out + 2 * (1 + size_t(k - 1) * p + tid);
      } else if (shut) {
        o = out + 2 * (1 + size_t(L) * p + 2 * size_t(k - 2) + (tid - p));
      }
      if (o) {
        o[0] = sr;
        o[1] = sim;
      }
    }
  }
  if (tid == 0) {
    const double* l = lenv + (size_t(L & 1) * Q1 + a.Q) * kPairTile;
    out[0] = l[0];
    out[1] = l[1];
  }
}

}  // namespace

// Queue the chain launch of a chunk's narrow pairs on st; up(list) places a list on the
// device (null: it did not fit, nothing is launched).  a.env and a.out are set by the caller.
template <class Up>
inline hipError_t pair_launch(PairTable& tb, PArgs a, hipStream_t st, Up&& up) {
  const size_t npair = tb.dims.size() / (2 * size_t(a.L + 1) * (a.Q + 1));
  a.blk = up(tb.blk);
  a.dims = up(tb.dims);
  if (npair == 0 || !a.blk || !a.dims || !a.env || !a.out) return hipSuccess;
  hipLaunchKernelGGL(k_obs_pair, dim3(unsigned(npair)), dim3(256), pair_lds_bytes(a.p, a.Q + 1), st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ host driver
// Queue the launches of one chunk of pairs (called by run_chunk): bra X[i], ket Y[i].
// Result j of the chunk (complex j of d_out) belongs to dests[j]: kind 6 ovl, 7 occ, 8 hop, idx the
// complex index in that output.  The chain pairs' results come first, then the list pairs' closes.
template <class BE>
void pair_chunk(BE& be, int L, int p, int Q, const std::vector<const StateDesc*>& X,
                const std::vector<const StateDesc*>& Y, const std::vector<size_t>& out_slot, bool want_occ,
                bool want_hop, double* d_out, const double* one, std::vector<Dest>& dests, Traffic& tr) {
  const int Q1 = Q + 1, B = int(X.size()), NB = L > 1 ? L - 1 : 0;
  const bool renv = want_occ || want_hop;
  auto DX = [&](int i, int b, int q) { return (q < 0 || q > Q) ? 0 : X[i]->dims[size_t(b) * Q1 + q]; };
  auto DY = [&](int i, int b, int q) { return (q < 0 || q > Q) ? 0 : Y[i]->dims[size_t(b) * Q1 + q]; };
  auto blk_of = [&](const StateDesc* s, int k, int q, int n) -> Blk {
    if (q < 0 || n < 0 || n >= p || q + n > Q) return Blk{};
    return s->blk[(size_t(k) * Q1 + q) * p + n];
  };
  auto AX = [&](int i, int k, int q, int n) { return blk_of(X[i], k, q, n); };
  auto AY = [&](int i, int k, int q, int n) { return blk_of(Y[i], k, q, n); };
  const bool chain_on = pair_chain_enabled();
  std::vector<int> chain, lists;
  for (int i = 0; i < B; ++i) {
    const int widest = std::max(*std::max_element(X[i]->dims.begin(), X[i]->dims.end()),
                                *std::max_element(Y[i]->dims.begin(), Y[i]->dims.end()));
    (chain_on && pair_chain_fits(widest, p, Q1) ? chain : lists).push_back(i);
  }

  // ---- narrow pairs: the table and one launch
  if (!chain.empty()) {
    PairTable tb;
    double work = 0, elems = 0;
    for (int i : chain) {
      const size_t o = out_slot[i];
      dests.push_back(Dest{6, o});
      for (size_t j = 0; j < size_t(L) * p; ++j) dests.push_back(Dest{7, o * L * p + j});
      for (size_t j = 0; j < 2 * size_t(NB); ++j) dests.push_back(Dest{8, o * 2 * NB + j});
      for (const StateDesc* s : {X[i], Y[i]}) {
        tb.dims.insert(tb.dims.end(), s->dims.begin(), s->dims.end());
        for (int k = 1; k <= L; ++k)
          for (int q = 0; q <= Q; ++q)
            for (int n = 0; n < p; ++n) {
              const Blk b = blk_of(s, k, q, n);
              tb.blk.push_back(EBlk{b.p, b.r, b.c});
              if (b.p) {
                work += double(b.r) * b.c * (b.r + b.c);
                elems += double(b.r) * b.c;
              }
            }
      }
    }
    PArgs a{nullptr, nullptr, be.alloc(chain.size() * pair_env_complex(L, Q1)), d_out, L, p, Q, want_occ ? 1 : 0,
            want_hop ? 1 : 0};
    // a model, not a count (the host builds no lists here): every block in one product per sweep and use
    const int uses = 1 + (renv ? 1 : 0) + (want_occ ? 1 : 0) + (want_hop ? 4 : 0);
    tr.flops += 8.0 * work * uses;
    tr.bytes += 16.0 * 2 * elems * uses;
    ++tr.launches;
    be.pair(tb, a);
  }
  if (lists.empty()) return;

  // ---- the other pairs: task lists
  std::vector<Task> gt;
  std::vector<Seg> gs;
  auto seg = [&](const double* A, int lda, const double* Bm, int ldb, int k, int ops, double alpha) {
    gs.push_back(Seg{A, Bm, lda, ldb, k, ops, alpha});
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
  const size_t QP = size_t(Q1) * p;

  // right sweep: R[i][b * Q1 + q] (d_x x d_y), b = 1..L
  std::vector<std::vector<const double*>> R(B);
  if (renv) {
    for (int i : lists) {
      R[i].assign(size_t(L + 1) * Q1, nullptr);
      R[i][size_t(L) * Q1 + Q] = one;
    }
    std::vector<std::vector<double*>> W(B);
    for (int k = L; k >= 2; --k) {
      for (int i : lists) {
        W[i].assign(QP, nullptr);
        for (int q = 0; q <= Q; ++q)
          for (int n = 0; n < p && q + n <= Q; ++n) {
            const Blk ax = AX(i, k, q, n), ay = AY(i, k, q, n);
            const double* r = R[i][size_t(k) * Q1 + q + n];
            if (!ax.p || !ay.p || !r) continue;
            double* w = be.alloc(size_t(ax.r) * ay.c);
            const int s0 = int(gs.size());
            seg(ax.p, ax.c, r, ay.c, ax.c, 0, 1.0);
            task(w, ax.r, ay.c, s0);
            W[i][size_t(q) * p + n] = w;
          }
      }
      launch_gemm();
      for (int i : lists)
        for (int q = 0; q <= Q; ++q) {
          const int rx = DX(i, k - 1, q), ry = DY(i, k - 1, q);
          if (rx == 0 || ry == 0) continue;
          const int s0 = int(gs.size());
          for (int n = 0; n < p && q + n <= Q; ++n) {
            const double* w = W[i][size_t(q) * p + n];
            if (!w) continue;
            const Blk ay = AY(i, k, q, n);
            seg(w, ay.c, ay.p, ay.c, ay.c, 2, 1.0);
          }
          if (int(gs.size()) == s0) continue;
          double* r = be.alloc(size_t(rx) * ry);
          task(r, rx, ry, s0);
          R[i][size_t(k - 1) * Q1 + q] = r;
        }
      launch_gemm();
    }
  }

  // left sweep
  std::vector<std::vector<const double*>> Lenv(B), Cenv(B), Genv(B);  // [ket sector] on the bond behind the site
  for (int i : lists) {
    Lenv[i].assign(Q1, nullptr);
    Cenv[i].assign(Q1, nullptr);
    Genv[i].assign(Q1, nullptr);
    Lenv[i][0] = one;
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
  std::vector<std::vector<double*>> T(B), Xp(B), TC(B), TG(B);
  for (int k = 1; k <= L; ++k) {
    const bool open = want_hop && k < L, shut = want_hop && k >= 2;
    // products with the ket's blocks: T = L Ay, TC = C Ay, TG = G Ay; with the bra's: X = Ax R
    for (int i : lists) {
      T[i].assign(QP, nullptr);
      Xp[i].assign(QP, nullptr);
      TC[i].assign(QP, nullptr);
      TG[i].assign(QP, nullptr);
      for (int q = 0; q <= Q; ++q)
        for (int n = 0; n < p && q + n <= Q; ++n) {
          const Blk ay = AY(i, k, q, n), ax = AX(i, k, q, n);
          auto times_ay = [&](const double* e, int m) {
            double* t = be.alloc(size_t(m) * ay.c);
            const int s0 = int(gs.size());
            seg(e, ay.r, ay.p, ay.c, ay.r, 0, 1.0);
            task(t, m, ay.c, s0);
            return t;
          };
          if (ay.p) {
            if (const double* l = Lenv[i][q]) T[i][size_t(q) * p + n] = times_ay(l, DX(i, k - 1, q));
            if (shut && Cenv[i][q]) TC[i][size_t(q) * p + n] = times_ay(Cenv[i][q], DX(i, k - 1, q + 1));
            if (shut && Genv[i][q]) TG[i][size_t(q) * p + n] = times_ay(Genv[i][q], DX(i, k - 1, q - 1));
          }
          const double* r = renv ? R[i][size_t(k) * Q1 + q + n] : nullptr;
          if (ax.p && r) {
            const int cy = DY(i, k, q + n);
            double* x = be.alloc(size_t(ax.r) * cy);
            const int s0 = int(gs.size());
            seg(ax.p, ax.c, r, cy, ax.c, 0, 1.0);
            task(x, ax.r, cy, s0);
            Xp[i][size_t(q) * p + n] = x;
          }
        }
    }
    launch_gemm();

    // the environments of bond k
    for (int i : lists) {
      std::vector<const double*> Ln(Q1, nullptr), Cn(Q1, nullptr), Gn(Q1, nullptr);
      for (int qq = 0; qq <= Q; ++qq) {
        const int cy = DY(i, k, qq);
        if (cy == 0) continue;
        // sum over n of alpha(n) Ax(qq - n, n + dn)^H T(qq - n, n) into an m x cy block
        auto env = [&](int dn, int m, std::vector<const double*>& dst) {
          if (m == 0) return;
          const int s0 = int(gs.size());
          for (int n = 0; n < p && qq - n >= 0; ++n) {
            const double* t = T[i][size_t(qq - n) * p + n];
            const Blk ax = AX(i, k, qq - n, n + dn);
            if (!t || !ax.p) continue;
            seg(ax.p, ax.c, t, cy, ax.r, 1, dn == 0 ? 1.0 : dn > 0 ? std::sqrt(double(n + 1)) : std::sqrt(double(n)));
          }
          if (int(gs.size()) == s0) return;
          double* e = be.alloc(size_t(m) * cy);
          task(e, m, cy, s0);
          dst[qq] = e;
        };
        env(0, DX(i, k, qq), Ln);
        if (open) {
          env(+1, DX(i, k, qq + 1), Cn);
          env(-1, DX(i, k, qq - 1), Gn);
        }
      }
      Lenv[i] = std::move(Ln);
      Cenv[i] = std::move(Cn);
      Genv[i] = std::move(Gn);
    }
    launch_gemm();

    // closes of site k
    for (int i : lists) {
      const size_t o = out_slot[i];
      if (want_occ)
        for (int n = 0; n < p; ++n) {
          const int p0 = int(cp.size());
          for (int q = 0; q + n <= Q; ++q) {
            const double *x = Xp[i][size_t(q) * p + n], *t = T[i][size_t(q) * p + n];
            if (!x || !t) continue;
            cp.push_back(Pair{x, t, (long long)DX(i, k - 1, q) * DY(i, k, q + n), 1.0});
          }
          close_task(p0, Dest{7, (o * L + (k - 1)) * p + n});
        }
      if (shut) {
        int p0 = int(cp.size());
        for (int s = 0; s + 1 <= Q; ++s)
          for (int n = 1; n < p && s + n <= Q; ++n) {
            const double *x = Xp[i][size_t(s + 1) * p + n - 1], *t = TC[i][size_t(s) * p + n];
            if (!x || !t) continue;
            cp.push_back(Pair{x, t, (long long)DX(i, k - 1, s + 1) * DY(i, k, s + n), std::sqrt(double(n))});
          }
        close_task(p0, Dest{8, (o * NB + (k - 2)) * 2});
        p0 = int(cp.size());
        for (int s = 1; s <= Q; ++s)
          for (int n = 0; n + 1 < p && s + n <= Q; ++n) {
            const double *x = Xp[i][size_t(s - 1) * p + n + 1], *t = TG[i][size_t(s) * p + n];
            if (!x || !t) continue;
            cp.push_back(Pair{x, t, (long long)DX(i, k - 1, s - 1) * DY(i, k, s + n), std::sqrt(double(n + 1))});
          }
        close_task(p0, Dest{8, (o * NB + (k - 2)) * 2 + 1});
      }
      if (k == L) {
        const int p0 = int(cp.size());
        if (Lenv[i][Q]) cp.push_back(Pair{one, Lenv[i][Q], 1, 1.0});
        close_task(p0, Dest{6, o});
      }
    }
    if (!ct.empty()) {
      ++tr.launches;
      const size_t first = dests.size() - ct.size();
      be.close(ct, cp, d_out ? d_out + 2 * first : nullptr);
    }
  }
}

}  // namespace obs
