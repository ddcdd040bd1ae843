// TEST INFRASTRUCTURE ONLY: the host driver of ocg_observe_pairs
// (observe_pair.hpp's pair_chunk through observe.hpp's run_chunk: table and list
// building, workspace sizing, output indexing) over a CPU backend, as a stand-alone
// program for the sanitizers.  The backend executes the task lists with plain loops
// and restates k_obs_pair's walk over its table in scalar code; every workspace
// block is a NaN-filled heap block of its exact size, and their sum is held to what
// the dry run counted.
//
//   pairs_host PAIRS   (text: "L p Q n", then per pair the (L+1)(Q+1) dims and the
//                       2 * nelem doubles of the bra, then those of the ket)
// prints "chain i v.." and "list i v.." per pair (v: ovl, occ[L][p], hop[L-1][2],
// each re im) and checks that a pair alone gives the bits it gives in the chunk.
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
  void energy(obs::EnergyTable&, const obs::EArgs&, std::vector<double>&) { std::abort(); }

  // a 16 x 16 tile of the workspace as a matrix of the given shape, and back
  using Mat = std::vector<cd>;
  static Mat tile(const double* t, int m, int n) {
    Mat M(size_t(m) * n);
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < n; ++j) M[size_t(i) * n + j] = at(t, size_t(i) * 16 + j);
    return M;
  }
  static void put(double* t, int m, int n, const Mat& M) {
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < n; ++j) {
        t[2 * (i * 16 + j)] = M[size_t(i) * n + j].real();
        t[2 * (i * 16 + j) + 1] = M[size_t(i) * n + j].imag();
      }
  }
  static Mat blk(const obs::EBlk& b) {
    Mat M(size_t(b.r) * b.c);
    for (size_t i = 0; i < M.size(); ++i) M[i] = at(b.a, i);
    return M;
  }
  // C (m x n) = op(A) B with A m x k (or, h: its conjugate transpose stored k x m), B k x n (or, bh: stored n x k)
  static Mat mul(const Mat& A, const Mat& B, int m, int k, int n, bool h = false, bool bh = false) {
    Mat C(size_t(m) * n, cd(0));
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < n; ++j)
        for (int x = 0; x < k; ++x)
          C[size_t(i) * n + j] += (h ? std::conj(A[size_t(x) * m + i]) : A[size_t(i) * k + x]) *
                                  (bh ? std::conj(B[size_t(j) * k + x]) : B[size_t(x) * n + j]);
    return C;
  }
  static cd dot(const Mat& X, const Mat& T) {
    cd s = 0;
    for (size_t i = 0; i < X.size(); ++i) s += std::conj(X[i]) * T[i];
    return s;
  }
  // k_obs_pair's walk in scalar code: the same table, tiles, ownership of the sectors and order of the sums
  void pair(obs::PairTable& tb, const obs::PArgs& a) {
    using namespace obs;
    const int L = a.L, p = a.p, Q1 = a.Q + 1;
    const size_t nblk = size_t(L) * Q1 * p, ndim = size_t(L + 1) * Q1;
    const size_t npair = tb.dims.size() / (2 * ndim);
    auto check = [](bool ok) {
      if (!ok) {
        std::fprintf(stderr, "table shapes disagree\n");
        std::exit(3);
      }
    };
    for (size_t si = 0; si < npair; ++si) {
      const EBlk *bx = tb.blk.data() + si * 2 * nblk, *by = bx + nblk;
      const int *dx = tb.dims.data() + si * 2 * ndim, *dy = dx + ndim;
      double* renv = a.env + si * 2 * pair_env_complex(L, Q1);
      double* lenv = renv + ndim * kPairTile;
      double* out = a.out + 2 * si * pair_outputs(L, p);
      for (size_t j = 0; j < 2 * nblk; ++j)
        if (bx[j].a) check(bx[j].r >= 1 && bx[j].c >= 1 && bx[j].r <= 16 && bx[j].c <= 16);
      if (a.occ || a.hop) {
        renv[(size_t(L) * Q1 + a.Q) * kPairTile] = 1.0;
        renv[(size_t(L) * Q1 + a.Q) * kPairTile + 1] = 0.0;
        for (int k = L; k >= 2; --k)
          for (int q = 0; q < Q1; ++q) {
            const int rx = dx[size_t(k - 1) * Q1 + q], ry = dy[size_t(k - 1) * Q1 + q];
            if (rx == 0 || ry == 0) continue;
            Mat acc(size_t(rx) * ry, cd(0));
            for (int n = 0; n < p && q + n < Q1; ++n) {
              const EBlk Ax = bx[(size_t(k - 1) * Q1 + q) * p + n], Ay = by[(size_t(k - 1) * Q1 + q) * p + n];
              if (!Ax.a || !Ay.a) continue;
              check(Ax.r == rx && Ay.r == ry && Ax.c == dx[size_t(k) * Q1 + q + n] && Ay.c == dy[size_t(k) * Q1 + q + n]);
              const Mat W = mul(blk(Ax), tile(renv + (size_t(k) * Q1 + q + n) * kPairTile, Ax.c, Ay.c), rx, Ax.c, Ay.c);
              const Mat R = mul(W, blk(Ay), rx, Ay.c, ry, false, true);
              for (size_t j = 0; j < acc.size(); ++j) acc[j] += R[j];
            }
            put(renv + (size_t(k - 1) * Q1 + q) * kPairTile, rx, ry, acc);
          }
      }
      lenv[0] = 1.0;
      lenv[1] = 0.0;
      for (int k = 1; k <= L; ++k) {
        const int cur = (k - 1) & 1, nxt = k & 1;
        const double *Lc = lenv + size_t(0 + cur) * Q1 * kPairTile, *Cc = lenv + size_t(2 + cur) * Q1 * kPairTile,
                     *Gc = lenv + size_t(4 + cur) * Q1 * kPairTile;
        double *Ln = lenv + size_t(0 + nxt) * Q1 * kPairTile, *Cn = lenv + size_t(2 + nxt) * Q1 * kPairTile,
               *Gn = lenv + size_t(4 + nxt) * Q1 * kPairTile;
        const int *dx0 = dx + size_t(k - 1) * Q1, *dy0 = dy + size_t(k - 1) * Q1;
        const int *dx1 = dx + size_t(k) * Q1, *dy1 = dy + size_t(k) * Q1;
        const EBlk *bkx = bx + size_t(k - 1) * Q1 * p, *bky = by + size_t(k - 1) * Q1 * p;
        const bool open = a.hop && k < L, shut = a.hop && k >= 2;
        std::vector<cd> part(size_t(p + 2) * Q1, cd(0));
        for (int qq = 0; qq < Q1; ++qq) {
          const int cy = dy1[qq], cx = dx1[qq];
          const int cxp = qq + 1 < Q1 ? dx1[qq + 1] : 0, cxm = qq >= 1 ? dx1[qq - 1] : 0;
          if (cy == 0) continue;
          Mat la(size_t(cx) * cy, cd(0)), ca(size_t(cxp) * cy, cd(0)), ga(size_t(cxm) * cy, cd(0));
          auto add = [&](Mat& dst, const EBlk A, const Mat& T, double alpha) {
            const Mat M = mul(blk(A), T, A.c, A.r, cy, true);
            check(M.size() == dst.size());
            for (size_t j = 0; j < dst.size(); ++j) dst[j] += alpha * M[j];
          };
          for (int n = 0; n < p && qq - n >= 0; ++n) {
            const int q = qq - n, rx = dx0[q], ry = dy0[q];
            const EBlk Ay = bky[size_t(q) * p + n];
            if (Ay.a) check(Ay.r == ry && Ay.c == cy);
            const Mat R = cx > 0 && (a.occ || a.hop) ? tile(renv + (size_t(k) * Q1 + qq) * kPairTile, cx, cy) : Mat();
            if (Ay.a && rx > 0) {
              const Mat T = mul(tile(Lc + size_t(q) * kPairTile, rx, ry), blk(Ay), rx, ry, cy);
              const EBlk Ax = bkx[size_t(q) * p + n];
              if (Ax.a) {
                check(Ax.r == rx && Ax.c == cx);
                add(la, Ax, T, 1.0);
                if (a.occ) part[size_t(n) * Q1 + qq] += dot(mul(blk(Ax), R, rx, cx, cy), T);
              }
              if (open && n + 1 < p && bkx[size_t(q) * p + n + 1].a) add(ca, bkx[size_t(q) * p + n + 1], T, std::sqrt(double(n + 1)));
              if (open && n >= 1 && bkx[size_t(q) * p + n - 1].a) add(ga, bkx[size_t(q) * p + n - 1], T, std::sqrt(double(n)));
            }
            if (shut && Ay.a) {
              if (n >= 1 && q + 1 < Q1 && dx0[q + 1] > 0) {
                const EBlk Ax = bkx[size_t(q + 1) * p + n - 1];
                if (Ax.a) {
                  check(Ax.c == cx);
                  const Mat T = mul(tile(Cc + size_t(q) * kPairTile, dx0[q + 1], ry), blk(Ay), dx0[q + 1], ry, cy);
                  part[size_t(p) * Q1 + qq] += std::sqrt(double(n)) * dot(mul(blk(Ax), R, Ax.r, cx, cy), T);
                }
              }
              if (n + 1 < p && q >= 1 && dx0[q - 1] > 0) {
                const EBlk Ax = bkx[size_t(q - 1) * p + n + 1];
                if (Ax.a) {
                  check(Ax.c == cx);
                  const Mat T = mul(tile(Gc + size_t(q) * kPairTile, dx0[q - 1], ry), blk(Ay), dx0[q - 1], ry, cy);
                  part[size_t(p + 1) * Q1 + qq] += std::sqrt(double(n + 1)) * dot(mul(blk(Ax), R, Ax.r, cx, cy), T);
                }
              }
            }
          }
          if (cx > 0) put(Ln + size_t(qq) * kPairTile, cx, cy, la);
          if (open && cxp > 0) put(Cn + size_t(qq) * kPairTile, cxp, cy, ca);
          if (open && cxm > 0) put(Gn + size_t(qq) * kPairTile, cxm, cy, ga);
        }
        for (int j = 0; j < p + 2; ++j) {
          cd s = 0;
          for (int q = 0; q < Q1; ++q) s += part[size_t(j) * Q1 + q];
          double* o = nullptr;
          if (j < p) {
            if (a.occ) o = out + 2 * (1 + size_t(k - 1) * p + j);
          } else if (shut) {
            o = out + 2 * (1 + size_t(L) * p + 2 * size_t(k - 2) + (j - p));
          }
          if (o) {
            o[0] = s.real();
            o[1] = s.imag();
          }
        }
      }
      const double* l = lenv + (size_t(L & 1) * Q1 + a.Q) * kPairTile;
      out[0] = l[0];
      out[1] = l[1];
    }
  }
};

// the outputs of the pairs idx (one chunk), pair_outputs complex per pair in the order ovl, occ, hop
static void run(int L, int p, int Q, const std::vector<obs::StateDesc>& dx, const std::vector<obs::StateDesc>& dy,
                const std::vector<int>& idx, bool occ, bool hop, std::vector<double>& res) {
  obs::Want want;
  want.pair = true;
  want.pair_occ = occ;
  want.pair_hop = hop && L > 1;
  std::vector<obs::StateDesc> sx, sy;
  for (int i : idx) {
    sx.push_back(dx[i]);
    sy.push_back(dy[i]);
  }
  const std::vector<size_t> need = obs::workspace_needs(L, p, Q, sx, {}, want, nullptr, &sy);
  size_t sum = 0;
  for (size_t b : need) sum += b;
  CpuBackend be(sum);
  std::vector<const obs::StateDesc*> X, Y;
  std::vector<size_t> os;
  for (size_t i = 0; i < sx.size(); ++i) {
    X.push_back(&sx[i]);
    Y.push_back(&sy[i]);
    os.push_back(i);
  }
  std::vector<obs::Dest> dests;
  obs::Traffic tr;
  const double* d_out = obs::run_chunk(be, L, p, Q, X, os, {}, want, dests, tr, nullptr, nullptr, &Y);
  if (dests.empty() || tr.launches <= 0 || !(tr.flops >= 0)) {
    std::fprintf(stderr, "bad result list\n");
    std::exit(4);
  }
  const size_t no = obs::pair_outputs(L, p), n = sx.size(), NB = L > 1 ? L - 1 : 0;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> ovl(2 * n, nan), po(2 * n * L * p, occ ? nan : 0.0), ph(2 * n * 2 * NB + 2, want.pair_hop ? nan : 0.0);
  obs::Outputs o;
  o.L = L;
  o.p = p;
  o.povl = ovl.data();
  o.pocc = occ ? po.data() : nullptr;
  o.phop = want.pair_hop ? ph.data() : nullptr;
  obs::scatter(dests, d_out, o, nullptr);
  res.clear();
  for (size_t i = 0; i < n; ++i) {
    res.insert(res.end(), ovl.begin() + 2 * i, ovl.begin() + 2 * (i + 1));
    res.insert(res.end(), po.begin() + 2 * i * L * p, po.begin() + 2 * (i + 1) * L * p);
    res.insert(res.end(), ph.begin() + 2 * i * 2 * NB, ph.begin() + 2 * (i + 1) * 2 * NB);
  }
  if (res.size() != 2 * no * n) std::exit(4);
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 1;
  int L, p, Q, n;
  if (std::fscanf(f, "%d %d %d %d", &L, &p, &Q, &n) != 4) return 1;
  const int nsq = (L + 1) * (Q + 1);
  std::vector<std::vector<int>> dims(2 * n, std::vector<int>(nsq));
  std::vector<std::vector<double>> data(2 * n);
  std::vector<obs::StateDesc> dx(n), dy(n);
  for (int i = 0; i < 2 * n; ++i) {  // bra, ket, bra, ket, ..
    for (int& d : dims[i])
      if (std::fscanf(f, "%d", &d) != 1) return 1;
    obs::StateDesc tmp;
    data[i].resize(2 * obs::compact_desc(L, p, Q, dims[i].data(), nullptr, tmp));
    for (double& x : data[i])
      if (std::fscanf(f, "%lf", &x) != 1) return 1;
    obs::compact_desc(L, p, Q, dims[i].data(), data[i].data(), (i & 1) ? dy[i / 2] : dx[i / 2]);
  }
  std::fclose(f);
  std::vector<int> all(n), rev(n);
  for (int i = 0; i < n; ++i) {
    all[i] = i;
    rev[i] = n - 1 - i;
  }
  const size_t no = 2 * obs::pair_outputs(L, p);
  for (int path = 0; path < 2; ++path) {
    setenv("OCG_OBS_PAIR_CHAIN", path == 0 ? "1" : "0", 1);
    std::vector<double> res, one, back, part;
    run(L, p, Q, dx, dy, all, true, true, res);
    run(L, p, Q, dx, dy, rev, true, true, back);
    for (int i = 0; i < n; ++i) {
      run(L, p, Q, dx, dy, {i}, true, true, one);
      if (std::memcmp(one.data(), res.data() + no * i, no * sizeof(double)) != 0 ||
          std::memcmp(one.data(), back.data() + no * (n - 1 - i), no * sizeof(double)) != 0) {
        std::fprintf(stderr, "pair %d: alone and in the chunk differ\n", i);
        return 5;
      }
      // what is asked for does not change the numbers: ovl alone, and occ without hop
      run(L, p, Q, dx, dy, {i}, false, false, part);
      if (std::memcmp(one.data(), part.data(), 2 * sizeof(double)) != 0) return 6;
      run(L, p, Q, dx, dy, {i}, true, false, part);
      if (std::memcmp(one.data(), part.data(), 2 * (1 + size_t(L) * p) * sizeof(double)) != 0) return 6;
      int wide = 0;
      for (int d : dims[2 * i]) wide = std::max(wide, d);
      for (int d : dims[2 * i + 1]) wide = std::max(wide, d);
      std::printf("%s %d", path == 0 && wide <= obs::kPairChainOrder ? "chain" : "list", i);
      for (size_t j = 0; j < no; ++j) std::printf(" %.17g", res[no * i + j]);
      std::printf("\n");
    }
  }
  return 0;
}
