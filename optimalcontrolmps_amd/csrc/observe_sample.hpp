// Fock-state snapshots and amplitudes of stored MPS (ocg_sample /
// ocg_fock_amplitudes and their _states variants): the kernel observe.hpp's
// run_chunk launches once per chunk after its right sweep, over all (state,
// shot) or (state, configuration) pairs.
//
// One wave carries one shot through the sites k = 1..L with the row vector
// v (1 x dims[k-1][q]) in LDS.  Per candidate n it forms w = v A_k(q, n) and
// pr_n = max(Re sum_c (w Renv_k[q+n])[c] conj(w[c]), 0) (Renv is Hermitian: both
// products read rows), draws n from the running sums with a counter-based
// random number, recomputes the chosen w into the other LDS buffer and swaps.
// With the occupations given (amplitudes) only the chosen product runs and no
// Renv is read.  Every sum is a fixed stride per lane and a butterfly over the
// wave: a result depends on its state, shot index and seed alone.  Chunks whose
// sectors are all at most 16 wide run four shots per wave (k_obs_sample16), with
// the same sums bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace obs {

constexpr int kSampleMaxOrder = 512;  // the sector orders v and w are sized for (as the spectrum's)
constexpr int kSamplePackOrder = 16;  // chunks up to this order run four shots per wave (k_obs_sample16)

// block (k, q, n) of a state: row-major r x c, interleaved (re, im); a null: absent
struct SBlk {
  const double* a;
  int r, c;
};
// one state of the chunk: where its L * Q1 * p blocks and L * Q1 right environments
// (Renv_k[q], k = 1..L) start in the tables, and the id mixed into the random numbers
struct SState {
  unsigned long long id;
  long long blk0, renv0;
};
struct SArgs {
  const SBlk* blk;
  const double* const* renv;
  const SState* st;
  const signed char* given;  // [nper][L] occupations (amplitude mode); null: draw
  signed char* config;       // [state][nper][L] (draw mode)
  double* val;               // draw: logp [state][nper]; amplitudes: [state][nper][2]
  unsigned long long seed;
  int L, p, Q, nper, vmax;
};
// the host side of a launch's tables
struct SampleTable {
  std::vector<SBlk> blk;
  std::vector<const double*> renv;
  std::vector<SState> st;
  std::vector<signed char> given;
};

// the splitmix64 step and the random number of (seed, id, shot, site)
__host__ __device__ inline unsigned long long sample_mix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__host__ __device__ inline unsigned long long sample_hash(unsigned long long seed, unsigned long long id,
                                                          unsigned long long shot, unsigned long long k) {
  return sample_mix(sample_mix(sample_mix(sample_mix(seed) ^ id) ^ shot) ^ k);
}
__host__ __device__ inline double sample_uniform(unsigned long long h) { return double(h >> 11) * 0x1.0p-53; }

inline size_t sample_lds_bytes(int vmax, int p) { return sizeof(double) * (4 * size_t(vmax) + 2 * size_t(p)); }
// four shots per wave when the chunk's largest order allows it (OCG_OBS_SAMPLE_PACK=0: never; the
// results do not depend on it, tested)
inline bool sample_packed(int vmax) {
  const char* e = std::getenv("OCG_OBS_SAMPLE_PACK");
  return vmax <= kSamplePackOrder && !(e && e[0] == '0');
}

namespace {

// out[j] = (v[0..r) * A)[j] (A r x c row-major) for the columns j = lane, lane + 64, ... below cend
__device__ inline void sample_row_times(const double* v, const double* __restrict__ A, int r, int cend, int c,
                                        double* out, int lane) {
  for (int j = lane; j < cend; j += 64) {
    double re = 0, im = 0;
    for (int i = 0; i < r; ++i) {
      const double vr = v[2 * i], vi = v[2 * i + 1];
      const double ar = A[2 * (size_t(i) * c + j)], ai = A[2 * (size_t(i) * c + j) + 1];
      re += vr * ar - vi * ai;
      im += vr * ai + vi * ar;
    }
    out[2 * j] = re;
    out[2 * j + 1] = im;
  }
}

__global__ __launch_bounds__(64) void k_obs_sample(const SArgs a) {
  extern __shared__ double sample_lds[];
  const int lane = threadIdx.x;
  const int Q1 = a.Q + 1;
  const int si = __builtin_amdgcn_readfirstlane(int(blockIdx.x / unsigned(a.nper)));
  const int shot = __builtin_amdgcn_readfirstlane(int(blockIdx.x % unsigned(a.nper)));
  const SState S = a.st[si];
  double* v = sample_lds;
  double* w = sample_lds + 2 * size_t(a.vmax);
  double* prs = sample_lds + 4 * size_t(a.vmax);  // pr_n, then the running sums c_n
  double* cs = prs + a.p;
  const size_t item = size_t(si) * a.nper + shot;
  const bool draw = a.given == nullptr;
  if (lane == 0) {
    v[0] = 1.0;
    v[1] = 0.0;
  }
  __syncthreads();
  const unsigned long long h0 = sample_mix(sample_mix(sample_mix(a.seed) ^ S.id) ^ (unsigned long long)shot);
  int q = 0, r = 1;
  bool dead = false;
  double norm2 = 0.0;
  for (int k = 1; k <= a.L; ++k) {
    const SBlk* B = a.blk + S.blk0 + (size_t(k - 1) * Q1 + q) * a.p;
    const double* const* R = a.renv + S.renv0 + size_t(k - 1) * Q1;
    int pick = -1;
    if (draw) {
      double run = 0.0;
      for (int n = 0; n < a.p; ++n) {
        double pr = 0.0;
        const double* rn = q + n <= a.Q ? R[q + n] : nullptr;
        if (rn && B[n].a) {
          const int c = B[n].c;
          sample_row_times(v, B[n].a, r, c, c, w, lane);
          __syncthreads();
          for (int j = lane; j < c; j += 64) {
            double yr = 0, yi = 0;
            for (int i = 0; i < c; ++i) {
              const double wr = w[2 * i], wi = w[2 * i + 1];
              const double rr = rn[2 * (size_t(i) * c + j)], ri = rn[2 * (size_t(i) * c + j) + 1];
              yr += wr * rr - wi * ri;
              yi += wr * ri + wi * rr;
            }
            pr += yr * w[2 * j] + yi * w[2 * j + 1];
          }
          for (int o = 32; o > 0; o >>= 1) pr += __shfl_xor(pr, o, 64);
          pr = pr > 0.0 ? pr : 0.0;  // (a NaN counts as 0)
          __syncthreads();           // w is rewritten by the next candidate
        }
        run += pr;
        if (lane == 0) {
          prs[n] = pr;
          cs[n] = run;
        }
      }
      __syncthreads();
      const double tot = cs[a.p - 1];
      if (k == 1) norm2 = tot;
      if (!(tot > 0.0)) {
        dead = true;
        break;
      }
      const double u = sample_uniform(sample_mix(h0 ^ (unsigned long long)k));
      int last = -1;
      for (int n = 0; n < a.p; ++n) {
        if (prs[n] > 0.0) last = n;
        if (pick < 0 && u * tot < cs[n]) pick = n;
      }
      if (pick < 0) pick = last;
      pick = __builtin_amdgcn_readfirstlane(pick);
      __syncthreads();  // prs / cs are rewritten at the next site
    } else {
      pick = a.given[size_t(shot) * a.L + (k - 1)];
      if (pick < 0 || pick >= a.p || q + pick > a.Q || !B[pick].a) {
        dead = true;
        break;
      }
    }
    const SBlk P = B[pick];
    sample_row_times(v, P.a, r, P.c, P.c, w, lane);
    __syncthreads();
    double* t = v;
    v = w;
    w = t;
    r = __builtin_amdgcn_readfirstlane(P.c);
    q = __builtin_amdgcn_readfirstlane(q + pick);
    if (draw && lane == 0) a.config[item * a.L + (k - 1)] = (signed char)pick;
  }
  if (draw) {
    if (lane == 0) {  // (the lane that wrote the sites before a dead end)
      if (dead)
        for (int k = 0; k < a.L; ++k) a.config[item * a.L + k] = (signed char)-1;
      a.val[item] = dead ? -__builtin_inf() : log(v[0] * v[0] + v[1] * v[1]) - log(norm2);
    }
  } else if (lane == 0) {
    a.val[2 * item] = dead ? 0.0 : v[0];
    a.val[2 * item + 1] = dead ? 0.0 : v[1];
  }
}

// Four shots per wave, 16 lanes each, for chunks whose largest sector order is at most
// kSamplePackOrder (config 1: every sector is a few states wide and 60 of 64 lanes would
// idle).  The groups of a wave differ in state, q and n, so control flow is kept
// wave-uniform: every candidate and every barrier is visited by all groups and a group
// without a block (or past a dead end, or past the last item) is predicated off.  The
// sums are those of k_obs_sample bit for bit: a lane holds the same column, and the
// 64-lane butterfly only adds the zeros of the lanes above 16 first.
__global__ __launch_bounds__(64) void k_obs_sample16(const SArgs a, const unsigned items) {
  extern __shared__ double sample_lds[];
  const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
  const int Q1 = a.Q + 1;
  const size_t item = size_t(blockIdx.x) * 4 + g;
  const bool live = item < items;
  const size_t it = live ? item : 0;
  const int si = int(it / unsigned(a.nper)), shot = int(it % unsigned(a.nper));
  const SState S = a.st[si];
  double* v = sample_lds + size_t(g) * (4 * kSamplePackOrder + 2 * a.p);
  double* w = v + 2 * kSamplePackOrder;
  double* prs = v + 4 * kSamplePackOrder;
  double* cs = prs + a.p;
  const bool draw = a.given == nullptr;
  if (l == 0) {
    v[0] = 1.0;
    v[1] = 0.0;
  }
  __syncthreads();
  const unsigned long long h0 = sample_mix(sample_mix(sample_mix(a.seed) ^ S.id) ^ (unsigned long long)shot);
  int q = 0, r = 1;
  bool dead = !live;
  double norm2 = 0.0;
  for (int k = 1; k <= a.L; ++k) {
    const SBlk* B = a.blk + S.blk0 + (size_t(k - 1) * Q1 + q) * a.p;
    const double* const* R = a.renv + S.renv0 + size_t(k - 1) * Q1;
    int pick = -1;
    if (draw) {
      double run = 0.0;
      for (int n = 0; n < a.p; ++n) {
        const double* rn = (!dead && q + n <= a.Q) ? R[q + n] : nullptr;
        const SBlk b = B[n];
        const bool on = rn && b.a && l < b.c;
        const int c = b.c;
        if (on) sample_row_times(v, b.a, r, l + 1, c, w, l);
        __syncthreads();
        double pr = 0.0;
        if (on) {
          double yr = 0, yi = 0;
          for (int i = 0; i < c; ++i) {
            const double wr = w[2 * i], wi = w[2 * i + 1];
            const double rr = rn[2 * (size_t(i) * c + l)], ri = rn[2 * (size_t(i) * c + l) + 1];
            yr += wr * rr - wi * ri;
            yi += wr * ri + wi * rr;
          }
          pr = yr * w[2 * l] + yi * w[2 * l + 1];
        }
        for (int o = 8; o > 0; o >>= 1) pr += __shfl_xor(pr, o, 64);
        pr = pr > 0.0 ? pr : 0.0;
        __syncthreads();
        run += pr;
        if (l == 0) {
          prs[n] = pr;
          cs[n] = run;
        }
      }
      __syncthreads();
      const double tot = cs[a.p - 1];
      if (k == 1) norm2 = tot;
      if (!(tot > 0.0)) dead = true;
      if (!dead) {
        const double u = sample_uniform(sample_mix(h0 ^ (unsigned long long)k));
        int last = -1;
        for (int n = 0; n < a.p; ++n) {
          if (prs[n] > 0.0) last = n;
          if (pick < 0 && u * tot < cs[n]) pick = n;
        }
        if (pick < 0) pick = last;
      }
      __syncthreads();
    } else if (!dead) {
      pick = a.given[size_t(shot) * a.L + (k - 1)];
      if (pick < 0 || pick >= a.p || q + pick > a.Q || !B[pick].a) dead = true;
    }
    SBlk P{nullptr, 0, 0};
    if (!dead) {
      P = B[pick];
      if (l < P.c) sample_row_times(v, P.a, r, l + 1, P.c, w, l);
    }
    __syncthreads();
    double* t = v;
    v = w;
    w = t;
    if (!dead) {
      r = P.c;
      q += pick;
      if (draw && l == 0) a.config[item * a.L + (k - 1)] = (signed char)pick;
    }
  }
  if (!live || l != 0) return;
  if (draw) {
    if (dead)
      for (int k = 0; k < a.L; ++k) a.config[item * a.L + k] = (signed char)-1;
    a.val[item] = dead ? -__builtin_inf() : log(v[0] * v[0] + v[1] * v[1]) - log(norm2);
  } else {
    a.val[2 * item] = dead ? 0.0 : v[0];
    a.val[2 * item + 1] = dead ? 0.0 : v[1];
  }
}

}  // namespace

// Queue the launch of one chunk on st; up(list) places a list on the device (null:
// it did not fit, nothing is launched).  a's table pointers are filled in here.
template <class Up>
inline hipError_t sample_launch(SampleTable& tb, SArgs a, hipStream_t st, Up&& up) {
  const size_t items = tb.st.size() * size_t(a.nper);
  const bool amp = !tb.given.empty();
  if (items > size_t(0x7fffffff)) return hipErrorInvalidValue;
  a.blk = up(tb.blk);
  a.renv = up(tb.renv);
  a.st = up(tb.st);
  a.given = amp ? up(tb.given) : nullptr;
  if (items == 0 || !a.blk || !a.renv || !a.st || (amp && !a.given) || !a.val || (!amp && !a.config))
    return hipSuccess;
  if (sample_packed(a.vmax))
    hipLaunchKernelGGL(k_obs_sample16, dim3(unsigned((items + 3) / 4)), dim3(64),
                       4 * sample_lds_bytes(kSamplePackOrder, a.p), st, a, unsigned(items));
  else
    hipLaunchKernelGGL(k_obs_sample, dim3(unsigned(items)), dim3(64), sample_lds_bytes(a.vmax, a.p), st, a);
  return hipGetLastError();
}

}  // namespace obs
