// Batched small Hermitian eigensolver and entropy reduction of the spectrum
// observables (ocg_observe_spectrum / ocg_observe_spectrum_states): the kernel
// family observe.hpp's run_chunk launches over the per-bond, per-sector
// environment blocks of a whole chunk.
//
// k_obs_eig: one workgroup per block of order n, cyclic Jacobi with the
// round-robin ordering (n/2 disjoint rotations per round, a bye for odd n).
// The matrix (and in stage A the vectors) live in LDS up to the switch-over
// order and in the chunk's global workspace above it; the code is the same.
// The rotation schedule, the convergence rule (off-diagonal Frobenius norm
// <= kEigTol * ||A||_F, tested before every sweep, at most kEigSweeps sweeps)
// and the reduction orders depend on n alone, so a block's result depends on
// that block alone.  Jacobi because stage A needs vectors and eigenvalues far
// below ||A|| must be right to ~1e-16 ||A|| absolute (the Schmidt weights at
// the truncation edge), which hbm_eig.hpp's cutoff contract does not promise.
// No atomics, no cross-workgroup synchronisation; a block that does not
// converge writes 1 to its own status word with an ordinary store.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace obs {

struct ETask {
  const double* A;  // n x n complex, Hermitian up to rounding; null: block absent, w = 0
  double* S;        // stage A: V diag(sqrt(max(lambda, 0))), n x n complex; null: values only
  double* w;        // n eigenvalues (in the order Jacobi leaves them); null: not kept
  double* work;     // orders above the LDS switch-over: n * n complex (twice that with S); else null
  int n;
};
// entropy of the n weights at w
struct STask {
  const double* w;
  int n;
};

constexpr int kEigMaxOrder = 512;
constexpr int kEigLdsMax = 64;    // 32 n^2 bytes with vectors: 128 KiB of the CU's 160 KiB
constexpr int kEigSmall = 16;     // orders up to this run on one wave
constexpr int kEigSweeps = 30;
constexpr double kEigTol = 1e-14;
constexpr int kEigNominalSweeps = 6;  // Traffic's flop count (the sweeps taken are known on the device only)

// the switch-over order (OCG_OBS_EIG_LDS_MAX=n overrides, 0: every block on the global path; tests)
inline int eig_lds_max() {
  if (const char* e = std::getenv("OCG_OBS_EIG_LDS_MAX")) return std::max(0, std::min(kEigLdsMax, std::atoi(e)));
  return kEigLdsMax;
}
// complex elements of global workspace a block of order n takes
inline size_t eig_work(int n, bool vectors, int lds_max) {
  return n > lds_max ? size_t(n) * n * (vectors ? 2 : 1) : 0;
}
inline double eig_flops(int n, bool vectors) {
  return double(kEigNominalSweeps) * (0.5 * n * (n - 1)) * (vectors ? 3.0 : 2.0) * n * 20.0;
}

namespace {

// pair k of round r of the round-robin schedule over m = n rounded up to even
// players (player m - 1 stays, the others rotate); false: the pair holds the bye
__device__ __forceinline__ bool eig_pair(int n, int m, int r, int k, int& a, int& b) {
  const int x = k == 0 ? m - 1 : (r + k) % (m - 1);
  const int y = k == 0 ? r : (r - k + m - 1) % (m - 1);
  a = x < y ? x : y;
  b = x < y ? y : x;
  return b < n;
}

// sum over the workgroup in a fixed order; every thread gets the same value
__device__ __forceinline__ double eig_block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int nw = int(blockDim.x) >> 6;
  if (nw == 1) return v;
  __syncthreads();  // red may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0;
  for (int w = 0; w < nw; ++w) s += red[w];
  return s;
}

// blockDim.x = 64 (orders <= kEigSmall) or 256; dynamic LDS: the largest LDS-resident block of the launch
__global__ __launch_bounds__(256) void k_obs_eig(const ETask* __restrict__ tasks, int* __restrict__ status) {
  extern __shared__ double obs_eig_lds[];
  __shared__ double rot[3 * (kEigMaxOrder / 2)];  // per pair: c, s cos(phi), s sin(phi)
  __shared__ double red[4];
  const int tid = threadIdx.x, nt = blockDim.x;
  const ETask T = tasks[blockIdx.x];
  const int n = T.n, nn = n * n;
  if (!T.A) {
    if (T.w)
      for (int j = tid; j < n; j += nt) T.w[j] = 0.0;
    if (tid == 0) status[blockIdx.x] = 0;
    return;
  }
  double* M = T.work ? T.work : obs_eig_lds;
  double* V = T.S ? M + 2 * size_t(nn) : nullptr;
  // one triangle's worth: the Hermitian part (the input is Hermitian only up to rounding)
  for (int e = tid; e < nn; e += nt) {
    const int i = e / n, j = e - i * n;
    const double* x = T.A + 2 * size_t(e);
    const double* y = T.A + 2 * (size_t(j) * n + i);
    M[2 * e] = 0.5 * (x[0] + y[0]);
    M[2 * e + 1] = 0.5 * (x[1] - y[1]);
    if (V) {
      V[2 * e] = i == j ? 1.0 : 0.0;
      V[2 * e + 1] = 0.0;
    }
  }
  __syncthreads();
  const int m = n + (n & 1), npair = m / 2;
  int st = 1;
  for (int sweep = 0;; ++sweep) {
    double off = 0, dia = 0;
    for (int e = tid; e < nn; e += nt) {
      const int i = e / n, j = e - i * n;
      const double v = M[2 * e] * M[2 * e] + M[2 * e + 1] * M[2 * e + 1];
      if (i == j)
        dia += v;
      else
        off += v;
    }
    off = eig_block_sum(off, red);
    dia = eig_block_sum(dia, red);
    if (sqrt(off) <= kEigTol * sqrt(off + dia)) {
      st = 0;
      break;
    }
    if (sweep == kEigSweeps) break;
    for (int r = 0; r < m - 1; ++r) {
      for (int k = tid; k < npair; k += nt) {
        int a, b;
        double c = 1.0, sr = 0.0, si = 0.0;
        if (eig_pair(n, m, r, k, a, b)) {
          const double xr = M[2 * (a * n + b)], xi = M[2 * (a * n + b) + 1];
          const double ab2 = xr * xr + xi * xi;
          if (ab2 >= 1e-300) {
            const double ab = sqrt(ab2);
            const double tau = (M[2 * (b * n + b)] - M[2 * (a * n + a)]) / (2.0 * ab);
            const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            const double s = t * c;
            sr = s * (xr / ab);
            si = s * (xi / ab);
          }
        }
        rot[3 * k] = c;
        rot[3 * k + 1] = sr;
        rot[3 * k + 2] = si;
      }
      __syncthreads();
      // columns: M <- M J, V <- V J; (x_a, x_b) <- (c x_a - conj(se) x_b, se x_a + c x_b), se = s e^{i phi}
      for (int it = tid; it < npair * n; it += nt) {
        const int row = it / npair, k = it - row * npair;
        const double c = rot[3 * k], sr = rot[3 * k + 1], si = rot[3 * k + 2];
        int a, b;
        if ((sr == 0.0 && si == 0.0) || !eig_pair(n, m, r, k, a, b)) continue;
        for (double* X = M; X; X = (X == M ? V : nullptr)) {
          double* pa = X + 2 * (row * n + a);
          double* pb = X + 2 * (row * n + b);
          const double ar = pa[0], ai = pa[1], br = pb[0], bi = pb[1];
          pa[0] = c * ar - (sr * br + si * bi);
          pa[1] = c * ai - (sr * bi - si * br);
          pb[0] = (sr * ar - si * ai) + c * br;
          pb[1] = (sr * ai + si * ar) + c * bi;
        }
      }
      __syncthreads();
      // rows: M <- J^H M; (x_a, x_b) <- (c x_a - se x_b, conj(se) x_a + c x_b)
      for (int it = tid; it < npair * n; it += nt) {
        const int k = it / n, col = it - k * n;
        const double c = rot[3 * k], sr = rot[3 * k + 1], si = rot[3 * k + 2];
        int a, b;
        if ((sr == 0.0 && si == 0.0) || !eig_pair(n, m, r, k, a, b)) continue;
        double* pa = M + 2 * (a * n + col);
        double* pb = M + 2 * (b * n + col);
        const double ar = pa[0], ai = pa[1], br = pb[0], bi = pb[1];
        pa[0] = c * ar - (sr * br - si * bi);
        pa[1] = c * ai - (sr * bi + si * br);
        pb[0] = (sr * ar + si * ai) + c * br;
        pb[1] = (sr * ai - si * ar) + c * bi;
      }
      __syncthreads();
    }
  }
  if (T.w)
    for (int j = tid; j < n; j += nt) T.w[j] = M[2 * (j * n + j)];
  if (T.S)
    for (int e = tid; e < nn; e += nt) {
      const int j = e % n;
      const double lam = M[2 * (j * n + j)];
      const double f = lam > 0.0 ? sqrt(lam) : 0.0;
      T.S[2 * size_t(e)] = V[2 * e] * f;
      T.S[2 * size_t(e) + 1] = V[2 * e + 1] * f;
    }
  if (tid == 0) status[blockIdx.x] = st;
}

// One wave per (state, bond): S = -sum_{p > 1e-12} p ln p over p = max(w, 0) / sum max(w, 0), 0 for a zero sum;
// every lane a fixed stride of the weights, then a butterfly: the order depends on n alone.
__global__ __launch_bounds__(64) void k_obs_entropy(const STask* __restrict__ tasks, double* __restrict__ out) {
  const STask T = tasks[blockIdx.x];
  const int lane = threadIdx.x;
  double s = 0;
  for (int j = lane; j < T.n; j += 64) s += fmax(T.w[j], 0.0);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  double h = 0;
  if (s > 0)
    for (int j = lane; j < T.n; j += 64) {
      const double p = fmax(T.w[j], 0.0) / s;
      if (p > 1e-12) h -= p * log(p);
    }
  for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
  if (lane == 0) out[blockIdx.x] = h;
}

}  // namespace

// the two launches of an eigen stage: orders <= kEigSmall on one wave, the rest on four
inline void eig_split(const std::vector<ETask>& t, std::vector<ETask>& small, std::vector<ETask>& big) {
  for (const ETask& x : t) (x.n <= kEigSmall ? small : big).push_back(x);
}

// Queue one group of an eigen stage on st; up(list) places the list on the device
// (null: it did not fit, nothing is launched).  Task j writes status[j].
template <class Up>
inline hipError_t eig_launch(std::vector<ETask>& t, int* status, int threads, hipStream_t st, Up&& up) {
  if (t.empty()) return hipSuccess;
  size_t lds = 0;
  for (const ETask& x : t)
    if (x.A && !x.work) lds = std::max(lds, size_t(16) * x.n * x.n * (x.S ? 2 : 1));
  const unsigned ntask = unsigned(t.size());
  const ETask* dt = up(t);
  if (!dt || !status) return hipSuccess;
  if (lds > 48 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute((const void*)k_obs_eig, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_obs_eig, dim3(ntask), dim3(threads), lds, st, dt, status);
  return hipGetLastError();
}

}  // namespace obs
