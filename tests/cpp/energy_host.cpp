// TEST INFRASTRUCTURE ONLY: the host driver of ocg_observe_moments
// (observe_energy.hpp's energy_chunk through observe.hpp's run_chunk: table and
// list building, workspace sizing, output indexing) over a CPU backend, as a
// stand-alone program for the sanitizers.  The backend executes the task lists
// with plain loops and restates k_obs_energy's walk over its table in scalar
// code; every workspace block is a NaN-filled heap block of its exact size, and their
// sum is held to what the dry run counted.
//
//   energy_host STATES   (text: "L p Q n", then per state its (L+1)(Q+1) dims and
//                         its 2 * nelem doubles)
// prints "chain i m0 .. m6" and "list i m0 .. m6" per state and checks that a
// state alone gives the bits it gives in the chunk.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../../optimalcontrolmps_amd/csrc/observe.hpp"

using cd = std::complex<double>;

struct CpuBackend {
  // every allocation a heap block of its exact size (an overrun meets a redzone), NaN-filled; the sum of
  // the granules must stay within what the dry run counted
  std::vector<std::unique_ptr<double[]>> blocks;
  size_t cap, top = 0;
  explicit CpuBackend(size_t bytes) : cap(bytes) {}
  double* alloc(size_t n) {
    n = n ? n : 1;
    top += obs::CountBackend::al(16 * n);
    if (top > cap) {
      std::fprintf(stderr, "workspace beyond the dry run's count\n");
      std::exit(2);
    }
    blocks.emplace_back(new double[2 * n]);
    std::fill(blocks.back().get(), blocks.back().get() + 2 * n, std::numeric_limits<double>::quiet_NaN());
    return blocks.back().get();
  }
  const double* one() {
    double* o = alloc(1);
    o[0] = 1.0;
    o[1] = 0.0;
    return o;
  }
  static cd at(const double* M, size_t i) { return cd(M[2 * i], M[2 * i + 1]); }
  void gemm(std::vector<obs::Task>& t, std::vector<obs::Seg>& s) {
    for (const obs::Task& T : t)
      for (int i = 0; i < T.m; ++i)
        for (int j = 0; j < T.n; ++j) {
          cd acc = 0;
          for (int x = T.seg0; x < T.seg0 + T.nseg; ++x) {
            const obs::Seg& S = s[x];
            for (int k = 0; k < S.k; ++k) {
              const cd a = (S.ops & 1) ? std::conj(at(S.A, size_t(k) * S.lda + i)) : at(S.A, size_t(i) * S.lda + k);
              const cd b = (S.ops & 2) ? std::conj(at(S.B, size_t(j) * S.ldb + k)) : at(S.B, size_t(k) * S.ldb + j);
              acc += S.alpha * a * b;
            }
          }
          T.C[2 * (size_t(i) * T.ldc + j)] = acc.real();
          T.C[2 * (size_t(i) * T.ldc + j) + 1] = acc.imag();
        }
    t.clear();
    s.clear();
  }
  void close(std::vector<obs::CTask>& t, std::vector<obs::Pair>& p, double* out) {
    for (size_t j = 0; j < t.size(); ++j) {
      cd acc = 0;
      for (int x = t[j].pair0; x < t[j].pair0 + t[j].npair; ++x)
        for (long long e = 0; e < p[x].n; ++e) acc += p[x].w * std::conj(at(p[x].X, e)) * at(p[x].Y, e);
      out[2 * j] = acc.real();
      out[2 * j + 1] = acc.imag();
    }
    t.clear();
    p.clear();
  }
  int eig(std::vector<obs::ETask>&, int*) { std::abort(); }
  void entropy(std::vector<obs::STask>&, double*) { std::abort(); }
  void sample(obs::SampleTable&, const obs::SArgs&) { std::abort(); }
  // k_obs_energy's walk in scalar code: the same table, flags, tiles and order of transitions
  void energy(obs::EnergyTable& tb, const obs::EArgs& a0, std::vector<double>& coef) {
    using namespace obs;
    EArgs a = a0;
    a.blk = tb.blk.data();
    a.dims = tb.dims.data();
    a.coef = coef.data();
    const int Q1 = a.Q + 1, nfl = kEnergyNCh * Q1;
    const size_t nst = tb.dims.size() / (size_t(a.L + 1) * Q1);
    for (size_t si = 0; si < nst; ++si) {
      const EBlk* blk = a.blk + si * size_t(a.L) * Q1 * a.p;
      const int* dims = a.dims + si * size_t(a.L + 1) * Q1;
      double* env = a.env + si * 2 * energy_env_complex(Q1);
      std::vector<int> flags(2 * size_t(nfl), 0);
      env[0] = 1.0;
      env[1] = 0.0;
      flags[0] = 1;
      for (int k = 1; k <= a.L; ++k) {
        const int cur = (k - 1) & 1, nxt = k & 1;
        const double* ecur = env + size_t(cur) * kEnergyNCh * Q1 * kEnergyTile;
        double* enxt = env + size_t(nxt) * kEnergyNCh * Q1 * kEnergyTile;
        const int *d0 = dims + size_t(k - 1) * Q1, *d1 = dims + size_t(k) * Q1;
        const EBlk* bk = blk + size_t(k - 1) * Q1 * a.p;
        for (int cho = 0; cho < kEnergyNCh; ++cho) {
          const int alo = cho / kEnergyNA, beo = cho % kEnergyNA, co = kEnergyCharge[alo] + kEnergyCharge[beo];
          for (int qko = 0; qko < Q1; ++qko) {
            const int qbo = qko + co;
            const int ck = d1[qko], cb = (qbo >= 0 && qbo < Q1) ? d1[qbo] : 0;
            bool any = false;
            std::vector<cd> acc(256, cd(0));
            if (energy_live(cho) && ck > 0 && cb > 0)
              for (int ta = 0; ta < kEnergyNT; ++ta)
                for (int tb2 = 0; tb2 < kEnergyNT; ++tb2) {
                  if (kEnergyTrans[ta].to != alo || kEnergyTrans[tb2].to != beo) continue;
                  const int al = kEnergyTrans[ta].from, be = kEnergyTrans[tb2].from, ch = al * kEnergyNA + be;
                  const int c0 = kEnergyCharge[al] + kEnergyCharge[be];
                  const int sh = kEnergyShift[kEnergyTrans[ta].op] + kEnergyShift[kEnergyTrans[tb2].op];
                  for (int n = 0; n < a.p; ++n) {
                    const double cf = a.coef[(size_t(ta) * kEnergyNT + tb2) * a.p + n];
                    const int qk = qko - n, qb = qk + c0, m = n + sh;
                    if (cf == 0.0 || qk < 0 || qb < 0 || qb >= Q1 || m < 0 || m >= a.p) continue;
                    if (!flags[size_t(cur) * nfl + ch * Q1 + qk]) continue;
                    const EBlk Ak = bk[size_t(qk) * a.p + n], Ab = bk[size_t(qb) * a.p + m];
                    if (!Ak.a || !Ab.a) continue;
                    const int rk = d0[qk], rb = d0[qb];
                    if (Ak.r != rk || Ak.c != ck || Ab.r != rb || Ab.c != cb || rk > 16 || rb > 16 || ck > 16 || cb > 16) {
                      std::fprintf(stderr, "table shapes disagree\n");
                      std::exit(3);
                    }
                    const double* e = ecur + (size_t(ch) * Q1 + qk) * kEnergyTile;
                    std::vector<cd> T(size_t(rb) * ck, cd(0));
                    for (int i = 0; i < rb; ++i)
                      for (int j = 0; j < ck; ++j)
                        for (int x = 0; x < rk; ++x) T[size_t(i) * ck + j] += at(e, size_t(i) * 16 + x) * at(Ak.a, size_t(x) * ck + j);
                    for (int i = 0; i < cb; ++i)
                      for (int j = 0; j < ck; ++j)
                        for (int x = 0; x < rb; ++x)
                          acc[size_t(i) * 16 + j] += cf * std::conj(at(Ab.a, size_t(x) * cb + i)) * T[size_t(x) * ck + j];
                    any = true;
                  }
                }
            if (any) {
              double* o = enxt + (size_t(cho) * Q1 + qko) * kEnergyTile;
              for (int i = 0; i < cb; ++i)
                for (int j = 0; j < ck; ++j) {
                  o[2 * (i * 16 + j)] = acc[size_t(i) * 16 + j].real();
                  o[2 * (i * 16 + j) + 1] = acc[size_t(i) * 16 + j].imag();
                }
            }
            flags[size_t(nxt) * nfl + cho * Q1 + qko] = any ? 1 : 0;
          }
        }
      }
      for (int j = 0; j < kEnergyOut; ++j) {
        const int ch = kEnergyFinal[j], buf = a.L & 1;
        const bool have = flags[size_t(buf) * nfl + ch * Q1 + a.Q] != 0;
        const double* e = env + (size_t(buf) * kEnergyNCh * Q1 + size_t(ch) * Q1 + a.Q) * kEnergyTile;
        a.out[2 * (si * kEnergyOut + j)] = have ? e[0] : 0.0;
        a.out[2 * (si * kEnergyOut + j) + 1] = have ? e[1] : 0.0;
      }
    }
  }
};

// the moments of the states idx (one chunk) into mom[slot of the request]
static void run(int L, int p, int Q, const std::vector<obs::StateDesc>& desc, const std::vector<int>& idx,
                std::vector<double>& mom) {
  obs::Want want;
  want.mom = true;
  std::vector<obs::StateDesc> sub;
  for (int i : idx) sub.push_back(desc[i]);
  const std::vector<size_t> need = obs::workspace_needs(L, p, Q, sub, {}, want);
  size_t sum = 0;
  for (size_t b : need) sum += b;
  CpuBackend be(sum);
  std::vector<const obs::StateDesc*> S;
  std::vector<size_t> os;
  for (size_t i = 0; i < sub.size(); ++i) {
    S.push_back(&sub[i]);
    os.push_back(i);
  }
  std::vector<obs::Dest> dests;
  obs::Traffic tr;
  const double* d_out = obs::run_chunk(be, L, p, Q, S, os, {}, want, dests, tr);
  if (dests.size() != sub.size() * obs::kEnergyOut || tr.launches <= 0 || !(tr.flops >= 0)) {
    std::fprintf(stderr, "bad result list\n");
    std::exit(4);
  }
  mom.assign(sub.size() * 7, std::numeric_limits<double>::quiet_NaN());
  obs::Outputs o;
  o.mom = mom.data();
  obs::scatter(dests, d_out, o, nullptr);
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 1;
  int L, p, Q, n;
  if (std::fscanf(f, "%d %d %d %d", &L, &p, &Q, &n) != 4) return 1;
  const int nsq = (L + 1) * (Q + 1);
  std::vector<std::vector<int>> dims(n, std::vector<int>(nsq));
  std::vector<std::vector<double>> data(n);
  std::vector<obs::StateDesc> desc(n);
  for (int i = 0; i < n; ++i) {
    for (int& d : dims[i])
      if (std::fscanf(f, "%d", &d) != 1) return 1;
    obs::StateDesc tmp;
    data[i].resize(2 * obs::compact_desc(L, p, Q, dims[i].data(), nullptr, tmp));
    for (double& x : data[i])
      if (std::fscanf(f, "%lf", &x) != 1) return 1;
    obs::compact_desc(L, p, Q, dims[i].data(), data[i].data(), desc[i]);
  }
  std::fclose(f);
  std::vector<int> all(n), rev(n);
  for (int i = 0; i < n; ++i) {
    all[i] = i;
    rev[i] = n - 1 - i;
  }
  for (int path = 0; path < 2; ++path) {
    setenv("OCG_OBS_ENERGY_CHAIN", path == 0 ? "1" : "0", 1);
    std::vector<double> mom, one, back;
    run(L, p, Q, desc, all, mom);
    run(L, p, Q, desc, rev, back);
    for (int i = 0; i < n; ++i) {
      run(L, p, Q, desc, {i}, one);
      if (std::memcmp(one.data(), mom.data() + 7 * i, 7 * sizeof(double)) != 0 ||
          std::memcmp(one.data(), back.data() + 7 * (n - 1 - i), 7 * sizeof(double)) != 0) {
        std::fprintf(stderr, "state %d: alone and in the chunk differ\n", i);
        return 5;
      }
      int wide = 0;
      for (int d : dims[i]) wide = std::max(wide, d);
      std::printf("%s %d", path == 0 && wide <= obs::kEnergyChainOrder ? "chain" : "list", i);
      for (int j = 0; j < 7; ++j) std::printf(" %.17g", mom[7 * i + j]);
      std::printf("\n");
    }
  }
  return 0;
}
