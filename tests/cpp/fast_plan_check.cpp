// TEST INFRASTRUCTURE ONLY: a verifier of the one-wave padded chain's host plans (csrc/fast_plan.hpp:
// build_fast_plan, build_overlap_plan), as a stand-alone program for the sanitizers.
//
// For every chain shape of L = 2..8, p = 2..7, Q = 1..8 (Q <= L (p - 1)) it builds the step plan and the
// overlap plan and walks every table with a decoder written from fast.hpp's layout comments.  What a field
// must hold is recomputed here from (L, p, Q) alone: the rank bounds, the padded layout, the operations of
// a step, the matricisation of each and its sectors.  Checked:
//   * every packed field decodes back to the value it stands for (so no field overflowed its bits);
//   * every source and destination offset lies inside its LDS region or is exactly that region's zero
//     slot: MPS <= np, matricisation / gated Θ <= kHThZ, scratch <= kHXsZ, eigenvectors <= 64;
//   * the factor destinations of an operation are pairwise distinct and cover whole padded sites (or the
//     whole scratch block), the gauge product's cover the neighbour site;
//   * the eigen slots of an operation are a permutation of 0..T-1;
//   * every table offset is 16-byte aligned and every table ends inside the image; kHNint / kOvNint is the
//     image size;
//   * fast_lds_bytes / overlap_lds_bytes cover the furthest byte a descriptor can address.
// fast_plan.hpp is plain host C++ (engine.hpp, fast.hpp): no HIP declaration is needed to include it.
//
//   fast_plan_check        one line per shape: "L p Q accepted <sizes>" or "L p Q rejected <why_not>";
//                          "VIOLATION ..." lines and exit status 1 if a check fails
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../optimalcontrolmps_amd/csrc/params.hpp"
#include "../../optimalcontrolmps_amd/csrc/fast_plan.hpp"

using namespace ocg::fastp;

static int g_bad = 0;
static int gL, gp, gQ;
static void bad(const char* fmt, ...) {
  if (++g_bad > 200) return;
  std::printf("VIOLATION %d %d %d: ", gL, gp, gQ);
  va_list ap;
  va_start(ap, fmt);
  std::vprintf(fmt, ap);
  va_end(ap);
  std::printf("\n");
}
#define CHECK(c, ...) do { if (!(c)) bad(__VA_ARGS__); } while (0)

// configurations of m sites with 0..p-1 bosons each that hold q bosons
static long long configs(int m, int p, int q) {
  if (q < 0) return 0;
  if (m == 0) return q == 0;
  static std::map<std::vector<int>, long long> memo;
  auto it = memo.find({m, p, q});
  if (it != memo.end()) return it->second;
  long long s = 0;
  for (int n = 0; n < p && n <= q; ++n) s += configs(m - 1, p, q - n);
  return memo[{m, p, q}] = s;
}

struct Elem { int k, q, n, a, c; };

// the padded layout recomputed from the rank bounds
struct Layout {
  int L, p, Q, Q1, np = 0;
  std::vector<int> D;                  // [(L+1) * Q1]
  std::map<std::vector<int>, int> po;  // (k, q, n) -> first padded element
  std::vector<Elem> el;                // padded element -> its indices
  std::vector<int> site;               // [k] first element, k = 1..L+1
  struct Blk { int k, q, n, first; };
  std::vector<Blk> blk;
  int d(int b, int q) const { return (b < 0 || b > L || q < 0 || q > Q) ? 0 : D[b * Q1 + q]; }
  int at(int k, int q, int n, int a, int c) const {  // padded index of A_k[(q, n)][a][c], -1: none
    auto it = po.find({k, q, n});
    if (it == po.end() || a < 0 || c < 0 || a >= d(k - 1, q) || c >= d(k, q + n)) return -1;
    return it->second + a * d(k, q + n) + c;
  }
  Layout(int L_, int p_, int Q_) : L(L_), p(p_), Q(Q_), Q1(Q_ + 1), D(size_t(L_ + 1) * (Q_ + 1)), site(L_ + 2, 0) {
    for (int b = 0; b <= L; ++b)
      for (int q = 0; q <= Q; ++q)
        D[b * Q1 + q] = int(std::min<long long>(std::min(configs(b, p, q), configs(L - b, p, Q - q)), 1 << 30));
    for (int k = 1; k <= L; ++k) {
      site[k] = np;
      const int first = int(blk.size());
      for (int q = 0; q <= Q; ++q)
        for (int n = 0; n < p && q + n <= Q; ++n) {
          const int dl = d(k - 1, q), dr = d(k, q + n);
          if (!dl || !dr) continue;
          po[{k, q, n}] = np;
          blk.push_back({k, q, n, first});
          for (int a = 0; a < dl; ++a)
            for (int c = 0; c < dr; ++c) el.push_back({k, q, n, a, c});
          np += dl * dr;
        }
    }
    site[L + 1] = np;
  }
};

struct Op { int kind, k, dir, closing; };
// the operations of a step (BH_tDMRG::doStep): the gates on the odd bonds ascending, then on the even
// bonds descending, each leaving the centre towards the next gate, the gauge moves to the next gate's
// near site between them, and the closing moves to site 1
static std::vector<Op> step_ops(int L) {
  std::vector<int> g;
  for (int i = 1; i < L; i += 2) g.push_back(i);
  for (int i = (L % 2 ? L - 1 : L - 2); i >= 2; i -= 2) g.push_back(i);
  std::vector<Op> ops;
  for (size_t x = 0; x < g.size(); ++x) {
    const bool last = x + 1 == g.size();
    const bool right = !last && g[x + 1] > g[x];  // the next gate lies to the right
    ops.push_back({kOpGate, g[x], right ? 0 : 1, 0});
    int c = right ? g[x] + 1 : g[x];
    const int to = last ? 1 : (right ? g[x + 1] : g[x + 1] + 1);
    for (; c < to; ++c) ops.push_back({kOpGaugeR, c, 0, last ? 1 : 0});
    for (; c > to; --c) ops.push_back({kOpGaugeL, c, 1, last ? 1 : 0});
  }
  return ops;
}

// a table of `count` entries of `width` ints at offset `off`: aligned and inside the image
static bool table_ok(const std::vector<int>& I, int off, long long count, int width, const char* what) {
  const bool ok = off >= 0 && off % 4 == 0 && off + count * width <= (long long)I.size();
  CHECK(ok, "%s: table at %d (%lld x %d ints) misaligned or outside the image of %zu", what, off, count, width,
        I.size());
  return ok;
}

static void check_step_plan(const OcgParams& P, const std::vector<int>& I, const Layout& Y) {
  const int L = Y.L, p = Y.p, Q = Y.Q, Q1 = Y.Q1, np = Y.np;
  CHECK(int(I.size()) >= kHdrInts && I[kHNint] == int(I.size()) && I.size() % 4 == 0, "kHNint %d, image %zu",
        I[kHNint], I.size());
  CHECK(I[kHNp] == np && np <= 64 * kItMps, "np %d, recomputed %d", I[kHNp], np);
  const int nblk = int(Y.blk.size());
  CHECK(I[kHNblk] == nblk, "nblk %d, recomputed %d", I[kHNblk], nblk);
  // ---- block table, element table, site ranges, site 1's physical indices
  if (table_ok(I, I[kHBlk], nblk, 4, "blocks"))
    for (int b = 0; b < nblk; ++b) {
      const int* t = &I[I[kHBlk] + 4 * b];
      const auto& B = Y.blk[b];
      CHECK((t[0] & 255) == B.k && ((t[0] >> 8) & 255) == B.q && (t[0] >> 16) == B.n && t[1] == (B.k - 1) * Q1 + B.q &&
                t[2] == B.k * Q1 + B.q + B.n && t[3] == B.first,
            "block %d decodes to k %d q %d n %d rows %d cols %d first %d", b, t[0] & 255, (t[0] >> 8) & 255, t[0] >> 16,
            t[1], t[2], t[3]);
    }
  if (table_ok(I, I[kHLs], np, 4, "elements")) {
    int b = -1;
    for (int x = 0; x < np; ++x) {
      const int* t = &I[I[kHLs] + 4 * x];
      const Elem& e = Y.el[x];
      if (e.a == 0 && e.c == 0) ++b;
      const unsigned w0 = t[0], w1 = t[1], w2 = t[2];
      CHECK(int(w0 & 0xffff) == (e.k - 1) * Q1 + e.q && int(w0 >> 16) == e.k * Q1 + e.q + e.n, "element %d: dims indices", x);
      CHECK(int(w1 & 0xffff) == b && int(w1 >> 16) == Y.blk[b].first, "element %d: block %d first %d", x, w1 & 0xffff,
            w1 >> 16);
      CHECK(int(w2 & 0xff) == e.a && int(w2 >> 8) == e.c, "element %d: a %d c %d", x, w2 & 0xff, w2 >> 8);
      CHECK(t[3] == P.site_base[e.k], "element %d: slot base %d", x, t[3]);
    }
  }
  if (table_ok(I, I[kHSite], L + 2, 1, "site ranges"))
    for (int k = 1; k <= L + 1; ++k) CHECK(I[I[kHSite] + k] == Y.site[k], "site %d starts at %d", k, I[I[kHSite] + k]);
  if (table_ok(I, I[kHSiteN], Y.site[2], 1, "site 1 physical indices"))
    for (int x = 0; x < Y.site[2]; ++x) CHECK(I[I[kHSiteN] + x] == Y.el[x].n, "site-1 element %d: n %d", x, I[I[kHSiteN] + x]);
  // ---- operations
  const std::vector<Op> ops = step_ops(L);
  CHECK(I[kHNops] == int(ops.size()) && int(ops.size()) <= kMaxOps, "%d operations, recomputed %zu", I[kHNops], ops.size());
  if (I[kHNops] != int(ops.size())) return;
  int last_gate = 0, thmax = 1, xsmax = 1;
  const int thz = I[kHThZ], xsz = I[kHXsZ];
  std::vector<int> goff(2 * p, 0);  // gate blocks per n1 + n2: lo, size, offset
  auto glo = [&](int s) { return std::max(0, s - (p - 1)); };
  auto gsz = [&](int s) { return std::min(p - 1, s) - glo(s) + 1; };
  for (int s = 1; s <= 2 * (p - 1); ++s) goff[s] = goff[s - 1] + gsz(s - 1) * gsz(s - 1);
  const int gtotal = goff[2 * (p - 1)] + 1;
  CHECK(gtotal == P.gtotal, "gate table of %d entries, recomputed %d", P.gtotal, gtotal);
  for (size_t oi = 0; oi < ops.size(); ++oi) {
    const Op& o = ops[oi];
    const int hp = I[kHOps + int(oi)];
    if (!table_ok(I, hp, 1, kOpHdr, "op header")) continue;
    const int* h = &I[hp];
    const bool gate = o.kind == kOpGate;
    if (gate) last_gate = o.k;
    const bool first_layer = gate && o.k % 2 == 1;
    const int mode = gate ? (first_layer ? 0 : 1) : 0;
    const int lonely = !gate || o.k + 1 != L ? 0 : (first_layer ? (L % 2 == 0 ? 1 : 0) : (L % 2 ? 2 : 0));
    const int newb = o.kind == kOpGaugeL ? o.k - 1 : o.k;
    CHECK(h[kOhKind] == o.kind && h[kOhK] == o.k && h[kOhDir] == o.dir && h[kOhClosing] == o.closing &&
              h[kOhMode] == mode && h[kOhLonely] == lonely && h[kOhNewBond] == newb,
          "op %zu header: kind %d k %d dir %d mode %d lonely %d closing %d bond %d", oi, h[kOhKind], h[kOhK], h[kOhDir],
          h[kOhMode], h[kOhLonely], h[kOhClosing], h[kOhNewBond]);
    // the matricisation: sector q has rows (nr, a) and cols (nc, c)
    const int bl = o.k - 1, br = gate ? o.k + 1 : o.k;
    const int prow = o.kind == kOpGaugeL ? 1 : p, pcol = o.kind == kOpGaugeR ? 1 : p;
    struct Rc { int n, i; };  // physical index and bond index of a row / column
    std::vector<std::vector<Rc>> rows(Q1), cols(Q1);
    std::vector<int> tho(Q1 + 1, 0);
    for (int q = 0; q <= Q; ++q) {
      for (int n = 0; n < prow; ++n)
        for (int a = 0; a < Y.d(bl, q - n); ++a) rows[q].push_back({n, a});
      for (int n = 0; n < pcol; ++n)
        for (int c = 0; c < Y.d(br, q + n); ++c) cols[q].push_back({n, c});
      if (rows[q].empty() || cols[q].empty()) { rows[q].clear(); cols[q].clear(); }
      tho[q + 1] = tho[q] + int(rows[q].size() * cols[q].size());
    }
    const int nth = tho[Q1];
    thmax = std::max(thmax, nth);
    CHECK(h[kOhNth] == nth && nth <= 64 * kItTh && nth <= thz, "op %zu: nth %d, recomputed %d, zero slot %d", oi,
          h[kOhNth], nth, thz);
    // TH index of (q, row (nr, a), col (nc, c)), -1: none
    auto th = [&](int q, int nr, int a, int nc, int c) {
      if (q < 0 || q > Q) return -1;
      int r = -1, cc = -1;
      for (size_t x = 0; x < rows[q].size(); ++x) if (rows[q][x].n == nr && rows[q][x].i == a) r = int(x);
      for (size_t x = 0; x < cols[q].size(); ++x) if (cols[q][x].n == nc && cols[q][x].i == c) cc = int(x);
      return (r < 0 || cc < 0) ? -1 : tho[q] + r * int(cols[q].size()) + cc;
    };
    // -- M's elements
    if (table_ok(I, h[kOhMat], nth, gate ? 2 : 1, "matricisation")) {
      int e = 0;
      for (int q = 0; q <= Q; ++q)
        for (const Rc& r : rows[q])
          for (const Rc& c : cols[q]) {
            if (gate) {
              const unsigned w0 = I[h[kOhMat] + 2 * e], w1 = I[h[kOhMat] + 2 * e + 1];
              const int x1 = w0 & 0xffff, x2 = w0 >> 16, dm = w1 & 0xff, drc = w1 >> 8;
              CHECK(dm == Y.d(o.k, q) && dm <= kMaxDm, "op %zu Θ %d: middle dimension %d", oi, e, dm);
              for (int b = 0; b < dm && b < kMaxDm; ++b)  // Θ = sum_b A_k[(q - nr, nr)][a][b] A_{k+1}[(q, nc)][b][c]
                CHECK(x1 + b == Y.at(o.k, q - r.n, r.n, r.i, b) && x2 + b * drc == Y.at(o.k + 1, q, c.n, b, c.i) &&
                          x1 + b < np && x2 + b * drc < np,
                      "op %zu Θ %d term %d: reads MPS %d and %d", oi, e, b, x1 + b, x2 + b * drc);
              CHECK(x2 <= np, "op %zu Θ %d: x2 %d outside the MPS", oi, e, x2);
            } else {
              const int s = I[h[kOhMat] + e];
              const int want = o.kind == kOpGaugeR ? Y.at(o.k, q - r.n, r.n, r.i, c.i) : Y.at(o.k, q, c.n, r.i, c.i);
              CHECK(s == want && s >= 0 && s < np, "op %zu M %d: source %d, recomputed %d", oi, e, s, want);
            }
            ++e;
          }
    }
    // -- gate descriptors
    if (gate && table_ok(I, h[kOhGate], nth, 4, "gate descriptors")) {
      int e = 0;
      for (int q = 0; q <= Q; ++q)
        for (const Rc& r : rows[q])
          for (const Rc& c : cols[q]) {
            const int* t = &I[h[kOhGate] + 4 * e];
            const unsigned w = t[0];
            const int row = w & 0xffff, sz = (w >> 16) & 15, lo = (w >> 20) & 15, a1 = (w >> 24) & 15, a2 = w >> 28;
            const int s = r.n + c.n;
            CHECK(a1 == r.n && a2 == c.n && lo == glo(s) && sz == gsz(s) && sz <= 6 &&
                      row == goff[s] + (a1 - lo) * sz && row + sz <= gtotal,
                  "op %zu gate %d: row %d sz %d lo %d a1 %d a2 %d", oi, e, row, sz, lo, a1, a2);
            for (int x = 0; x < sz && x < 6; ++x) {  // input (n1, n2) = (lo + x, s - n1) of the same bond indices
              const int ad = (unsigned(t[1 + x / 2]) >> (16 * (x & 1))) & 0xffff, n1 = lo + x;
              const int want = th(q - r.n + n1, n1, r.i, s - n1, c.i);
              CHECK(ad == want && ad >= 0 && ad < nth, "op %zu gate %d input %d: Θ %d, recomputed %d", oi, e, x, ad, want);
            }
            ++e;
          }
    }
    // -- sectors of the decomposition
    std::vector<int> sq, secn(Q1, 0), side(Q1, 0), grp(Q1, -1), eoff(Q1, 0), sidx(Q1, -1);
    int ngrp = 0, T = 0, maxn = 0, dot = 1;
    for (int q = 0; q <= Q; ++q) {
      const int R = int(rows[q].size()), C = int(cols[q].size());
      if (!R) continue;
      secn[q] = std::min(R, C);
      // the Gram on the smaller side; on a tie, the side of the bond a gauge move does not rewrite
      side[q] = R < C ? 0 : (R > C ? 1 : (o.kind == kOpGaugeR ? 1 : 0));
      if (secn[q] >= 2) grp[q] = ngrp++;
      eoff[q] = T;
      sidx[q] = int(sq.size());
      sq.push_back(q);
      T += secn[q];
      maxn = std::max(maxn, secn[q]);
      dot = std::max(dot, std::max(R, C));
      CHECK(secn[q] <= kMaxGram && std::max(R, C) <= kMaxDot, "op %zu sector %d: %d x %d", oi, q, R, C);
      CHECK(Y.d(newb, q) <= secn[q] && Y.d(newb, q) <= kMaxDm, "op %zu sector %d: bound %d above its order %d", oi, q,
            Y.d(newb, q), secn[q]);
    }
    const int nsec = int(sq.size());
    CHECK(h[kOhNsec] == nsec && nsec <= 15 && h[kOhT] == T && T <= 64 && h[kOhNgrp] == ngrp && ngrp <= 4 &&
              h[kOhMaxr] == (maxn >= 3 ? 3 : maxn == 2 ? 1 : 0) && h[kOhDot] == dot,
          "op %zu: nsec %d T %d ngrp %d maxr %d dot %d, recomputed %d %d %d (order %d) %d", oi, h[kOhNsec], h[kOhT],
          h[kOhNgrp], h[kOhMaxr], h[kOhDot], nsec, T, ngrp, maxn, dot);
    std::vector<int> slots(T, 0);  // eigen slots claimed by the Jacobi groups and the order-1 sectors
    {
      int g = 0;
      for (int q : sq) {
        if (grp[q] < 0) continue;
        const int* G = &h[kOhGrp + 8 * g++];
        const int R = int(rows[q].size()), C = int(cols[q].size());
        CHECK(G[0] == sidx[q] && G[1] == secn[q] && G[2] == side[q] && G[3] == tho[q] && G[4] == R && G[5] == C &&
                  G[6] == eoff[q],
              "op %zu group %d: s %d n %d side %d tho %d R %d C %d eoff %d", oi, g - 1, G[0], G[1], G[2], G[3], G[4], G[5], G[6]);
        // the Gram dots of rows / columns i < n stay inside the block
        const int len = side[q] == 0 ? C : R, st = side[q] == 0 ? 1 : C, step = side[q] == 0 ? C : 1;
        CHECK(tho[q] + (secn[q] - 1) * step + (len - 1) * st < tho[q + 1], "op %zu group %d: dots leave the block", oi, g - 1);
        for (int i = 0; i < secn[q]; ++i) if (eoff[q] + i < T) ++slots[eoff[q] + i];
      }
      for (; g < 4; ++g) CHECK(h[kOhGrp + 8 * g] == -1, "op %zu: unused group %d marked %d", oi, g, h[kOhGrp + 8 * g]);
    }
    int no1 = 0;
    for (int q : sq) no1 += secn[q] == 1;
    CHECK(h[kOhNo1] == no1 && no1 <= 64, "op %zu: %d order-1 sectors, recomputed %d", oi, h[kOhNo1], no1);
    if (table_ok(I, h[kOhO1], no1, 4, "order-1 sectors")) {
      int x = 0;
      for (int q : sq) {
        if (secn[q] != 1) continue;
        const int* t = &I[h[kOhO1] + 4 * x++];
        const int R = int(rows[q].size()), C = int(cols[q].size());
        CHECK(t[0] == tho[q] && t[1] == R * C && t[1] <= kMaxDot && t[2] == (side[q] == 0 ? 1 : C) &&
                  t[0] + (t[1] - 1) * t[2] < tho[q + 1] && t[3] == eoff[q],
              "op %zu order-1 sector %d: M %d len %d stride %d slot %d", oi, q, t[0], t[1], t[2], t[3]);
        if (t[3] >= 0 && t[3] < T) ++slots[t[3]];
      }
    }
    for (int e = 0; e < T; ++e) CHECK(slots[e] == 1, "op %zu: eigen slot %d claimed %d times", oi, e, slots[e]);
    if (table_ok(I, h[kOhEq], T, 4, "eigen slots")) {
      std::vector<int> seen(T, 0);
      int e = 0;
      for (int q : sq)
        for (int i = 0; i < secn[q]; ++i, ++e) {
          const int* t = &I[h[kOhEq] + 4 * e];
          CHECK(t[0] == sidx[q] && t[1] == i && t[2] == eoff[q] && (t[3] & 255) == secn[q] &&
                    int(unsigned(t[3]) >> 8) == Y.d(newb, q),
                "op %zu eigen slot %d: s %d i %d eoff %d n %d bound %d", oi, e, t[0], t[1], t[2], t[3] & 255, unsigned(t[3]) >> 8);
          if (t[2] + t[1] >= 0 && t[2] + t[1] < T) ++seen[t[2] + t[1]];
        }
      for (int x = 0; x < T; ++x) CHECK(seen[x] == 1, "op %zu: eigen slots are no permutation (slot %d: %d)", oi, x, seen[x]);
    }
    if (table_ok(I, h[kOhSecQ], nsec, 1, "sector table"))
      for (int s = 0; s < nsec; ++s) {
        const int w = I[h[kOhSecQ] + s], q = sq[s];
        CHECK((w & 255) == q && ((w >> 8) & 255) == eoff[q] && ((w >> 16) & 15) == secn[q] && (w >> 20) == 0,
              "op %zu sector %d: q %d eoff %d n %d", oi, s, w & 255, (w >> 8) & 255, w >> 16);
      }
    // -- factor elements
    std::vector<int> xs_off(Q1, 0), ys_off(Q1, 0);
    int xs_tot = 0, ys_tot = 0;
    for (int q : sq) {
      xs_off[q] = xs_tot;
      ys_off[q] = ys_tot;
      if (o.kind == kOpGaugeL) xs_tot += int(rows[q].size()) * Y.d(newb, q);  // X: R x D(newb, q)
      if (o.kind == kOpGaugeR) ys_tot += Y.d(newb, q) * int(cols[q].size());  // Y: D(newb, q) x C
    }
    const int scr_tot = std::max(xs_tot, ys_tot);
    xsmax = std::max(xsmax, scr_tot);
    CHECK(scr_tot <= xsz, "op %zu: scratch %d beyond its zero slot %d", oi, scr_tot, xsz);
    const int nf = h[kOhNf];
    CHECK(nf <= 64 * kItF, "op %zu: %d factor elements", oi, nf);
    std::set<int> fmps, fscr;
    if (table_ok(I, h[kOhF], nf, 4, "factor elements"))
      for (int e = 0; e < nf; ++e) {
        const int* t = &I[h[kOhF] + 4 * e];
        const unsigned w0 = t[0], w1 = t[1], w2 = t[2];
        const int dest = w0 & 0xffff, s = (w0 >> 16) & 15, j = (w0 >> 20) & 15;
        const bool isx = (w0 >> 24) & 1, scr = (w0 >> 25) & 1;
        CHECK((w0 >> 26) == 0 && s < nsec, "op %zu factor %d: sector %d", oi, e, s);
        if (s >= nsec) continue;
        const int q = sq[s], n = secn[q], R = int(rows[q].size()), C = int(cols[q].size());
        const bool exact = (w2 >> 12) & 1;
        CHECK(int(w2 & 255) == eoff[q] && int((w2 >> 8) & 15) == n && (w2 >> 13) == 0 && j < Y.d(newb, q) && j < n,
              "op %zu factor %d: eoff %d n %d j %d", oi, e, w2 & 255, (w2 >> 8) & 15, j);
        CHECK(exact == (isx ? side[q] == 0 : side[q] == 1), "op %zu factor %d: exact %d on side %d", oi, e, int(exact), side[q]);
        CHECK(t[3] == (grp[q] >= 0 ? 16 * grp[q] : 64), "op %zu factor %d: eigenvector block %d", oi, e, t[3]);
        // which row (X) or column (Y) of the sector the destination is
        int idx = -1;
        if (scr) {
          CHECK(isx ? o.kind == kOpGaugeL : o.kind == kOpGaugeR, "op %zu factor %d: scratch destination", oi, e);
          const int jb = Y.d(newb, q), rel = dest - (isx ? xs_off[q] : ys_off[q]);
          if (isx && rel >= 0 && rel < R * jb && rel % jb == j) idx = rel / jb;
          if (!isx && rel >= 0 && rel < jb * C && rel / C == j) idx = rel % C;
          CHECK(dest < scr_tot && dest < xsz && fscr.insert(dest).second, "op %zu factor %d: scratch destination %d", oi, e, dest);
        } else {
          CHECK(isx ? o.kind != kOpGaugeL : o.kind != kOpGaugeR, "op %zu factor %d: MPS destination", oi, e);
          CHECK(dest < np && fmps.insert(dest).second, "op %zu factor %d: MPS destination %d", oi, e, dest);
          if (dest < np) {
            const Elem& d = Y.el[dest];
            if (isx && d.k == o.k && d.q + d.n == q && d.c == j)  // row (nr, a) of sector q: block (q - nr, nr), row a
              for (size_t x = 0; x < rows[q].size(); ++x) if (rows[q][x].n == d.n && rows[q][x].i == d.a) idx = int(x);
            if (!isx && d.k == (gate ? o.k + 1 : o.k) && d.q == q && d.a == j)  // col (nc, c): block (q, nc), col c
              for (size_t x = 0; x < cols[q].size(); ++x) if (cols[q][x].n == d.n && cols[q][x].i == d.c) idx = int(x);
          }
        }
        CHECK(idx >= 0, "op %zu factor %d: destination %d is no %s element of sector %d, column %d", oi, e, dest,
              isx ? "X" : "Y", q, j);
        if (idx < 0) continue;
        if (exact) {  // W[idx][.] of the group, or the unit slot
          CHECK(int(w1) == t[3] + (grp[q] >= 0 ? 4 * idx : 0) && idx < n && int(w1) + n - 1 <= 64,
                "op %zu factor %d: eigenvector row at %d", oi, e, int(w1));
        } else {      // X[idx][j] = sum_c M[idx][c] W[c][.], Y[j][idx] = sum_r conj(W[r][.]) M[r][idx]
          const int mb = w1 & 0xffff, terms = (w1 >> 16) & 31, ms = w1 >> 21;
          CHECK(mb == (isx ? tho[q] + idx * C : tho[q] + idx) && terms == n && terms <= kMaxGram && ms == (isx ? 1 : C) &&
                    mb + (terms - 1) * ms < tho[q + 1] && mb + (terms - 1) * ms < nth,
                "op %zu factor %d: M %d terms %d stride %d", oi, e, mb, terms, ms);
        }
      }
    {  // whole padded sites (and the whole scratch block)
      std::set<int> want;
      auto whole = [&](int k) { for (int x = Y.site[k]; x < Y.site[k + 1]; ++x) want.insert(x); };
      if (o.kind != kOpGaugeL) whole(o.k);
      if (gate) whole(o.k + 1);
      if (o.kind == kOpGaugeL) whole(o.k);
      CHECK(fmps == want, "op %zu: the factors write %zu MPS elements, the whole sites have %zu", oi, fmps.size(), want.size());
      CHECK(int(fscr.size()) == (gate ? 0 : scr_tot), "op %zu: the factors write %zu scratch elements of %d", oi, fscr.size(), scr_tot);
    }
    // -- gauge product: every element of the neighbour site
    if (!gate) {
      const int nb = o.kind == kOpGaugeR ? o.k + 1 : o.k - 1;
      const int ns = h[kOhNs];
      CHECK(nb >= 1 && nb <= L && ns == Y.site[nb + 1] - Y.site[nb] && ns <= 64 * kItS, "op %zu: %d product elements", oi, ns);
      std::set<int> dests;
      if (nb >= 1 && nb <= L && table_ok(I, h[kOhS], ns, 4, "gauge product"))
        for (int e = 0; e < ns; ++e) {
          const int* t = &I[h[kOhS] + 4 * e];
          const unsigned w0 = t[0], w1 = t[1];
          const int x1 = w0 & 0xffff, x2 = w0 >> 16, len = w1 & 0xffff, s2 = w1 >> 16, dest = t[2];
          CHECK(dest >= Y.site[nb] && dest < Y.site[nb + 1] && dests.insert(dest).second && t[3] == 0,
                "op %zu product %d: destination %d", oi, e, dest);
          if (dest < 0 || dest >= np) continue;
          const Elem& d = Y.el[dest];
          const int qq = o.kind == kOpGaugeR ? d.q : d.q + d.n;  // the sector of the rewritten bond
          const int want_len = sidx[qq] >= 0 ? Y.d(newb, qq) : 0;
          CHECK(len == want_len && len <= kMaxDm, "op %zu product %d: %d terms, recomputed %d", oi, e, len, want_len);
          for (int b = 0; b < len && b < kMaxDm; ++b) {
            if (o.kind == kOpGaugeR)  // S[(q, n)][j][c] = sum_b Y_q[j][b] A_{k+1}[(q, n)][b][c]
              CHECK(x1 + b == ys_off[qq] + d.a * int(cols[qq].size()) + b && x1 + b < scr_tot &&
                        x2 + b * s2 == Y.at(nb, d.q, d.n, b, d.c) && x2 + b * s2 < np,
                    "op %zu product %d term %d: scratch %d, MPS %d", oi, e, b, x1 + b, x2 + b * s2);
            else                      // S[(q, n)][a][j] = sum_b A_{k-1}[(q, n)][a][b] X_qq[b][j]
              CHECK(x1 + b == Y.at(nb, d.q, d.n, d.a, b) && x1 + b < np &&
                        x2 + b * s2 == xs_off[qq] + b * Y.d(newb, qq) + d.c && x2 + b * s2 < scr_tot,
                    "op %zu product %d term %d: MPS %d, scratch %d", oi, e, b, x1 + b, x2 + b * s2);
          }
          // a product without terms still reads its second operand once, at x2
          CHECK(x2 <= (o.kind == kOpGaugeR ? np : xsz), "op %zu product %d: x2 %d outside its region", oi, e, x2);
        }
      CHECK(int(dests.size()) == ns, "op %zu: the product writes %zu of %d elements", oi, dests.size(), ns);
    }
  }
  // ---- zero slots and the LDS map (complex units), then the bytes behind it
  CHECK(thz == thmax && xsz == xsmax, "zero slots %d / %d, recomputed %d / %d", thz, xsz, thmax, xsmax);
  CHECK(I[kHCentre] == last_gate, "open centre %d, recomputed %d", I[kHCentre], last_gate);
  const int zo[8] = {I[kHZMps], I[kHZTh], I[kHZTg], I[kHZW], I[kHZX], I[kHZGt], I[kHZPh], I[kHZTot]};
  const int need[7] = {np + 1, thz + 1, thz + 1, 65, xsz + 1, 2 * gtotal, 2 * p + 2 * p * p};
  CHECK(zo[0] == 0, "the MPS region starts at %d", zo[0]);
  for (int r = 0; r < 7; ++r)
    CHECK(zo[r] >= 0 && zo[r + 1] >= zo[r] + need[r], "LDS region %d: [%d, %d) holds fewer than %d elements", r, zo[r], zo[r + 1], need[r]);
  auto al = [](int x) { return (x + 3) & ~3; };
  // complex buffers; LAM, SIG, 1 / SIG (64 each), 8 spare, the model cache (2 kMaxOps) as doubles; the model
  // cache epochs, dims, block offsets, kept counts, eigenvector indices (64 each), 4 flags, the image as ints
  const long long furthest = 16LL * zo[7] + 8LL * (3 * 64 + 8 + 2 * kMaxOps) +
                             4LL * (kMaxOps + al(P.nsq) + al(nblk) + 64 + 64 + 4 + I[kHNint]);
  CHECK(ocg_host::fast_lds_bytes(I, P) >= furthest, "fast_lds_bytes %d below the furthest byte %lld",
        ocg_host::fast_lds_bytes(I, P), furthest);
}

static void check_overlap_plan(const OcgParams& P, const std::vector<int>& I, const Layout& Y) {
  const int L = Y.L, p = Y.p, Q = Y.Q, Q1 = Y.Q1, np = Y.np, nblk = int(Y.blk.size());
  CHECK(int(I.size()) >= kOvHdr && I[kOvNint] == int(I.size()) && I.size() % 4 == 0, "overlap: kOvNint %d, image %zu",
        I[kOvNint], I.size());
  CHECK(I[kOvL] == L && I[kOvQ1] == Q1 && I[kOvP] == p && p <= kOvMaxP && I[kOvNp] == np && I[kOvNblk] == nblk,
        "overlap header: L %d Q1 %d p %d np %d nblk %d", I[kOvL], I[kOvQ1], I[kOvP], I[kOvNp], I[kOvNblk]);
  std::vector<int> eo(size_t(L + 1) * Q1, 0), en(L + 1, 0);
  int maxen = 1, maxsite = 1;
  for (int b = 0; b <= L; ++b)
    for (int q = 0; q <= Q; ++q) {
      eo[b * Q1 + q] = en[b];
      en[b] += Y.d(b, q) * Y.d(b, q);
      maxen = std::max(maxen, en[b]);
    }
  for (int k = 1; k <= L; ++k) maxsite = std::max(maxsite, Y.site[k + 1] - Y.site[k]);
  CHECK(I[kOvMaxSite] == maxsite && I[kOvMaxEn] == maxen && maxen <= kOvMaxE && en[0] == 1 && en[L] == 1,
        "overlap: largest site %d (%d), environment %d (%d)", I[kOvMaxSite], maxsite, I[kOvMaxEn], maxen);
  if (table_ok(I, I[kOvD], (L + 1) * Q1, 1, "overlap bounds") && table_ok(I, I[kOvEo], (L + 1) * Q1, 1, "overlap eo"))
    for (int x = 0; x < (L + 1) * Q1; ++x)
      CHECK(I[I[kOvD] + x] == Y.D[x] && I[I[kOvEo] + x] == eo[x], "overlap: bound / offset %d: %d / %d", x, I[I[kOvD] + x], I[I[kOvEo] + x]);
  if (table_ok(I, I[kOvEn], L + 1, 1, "overlap en"))
    for (int b = 0; b <= L; ++b) CHECK(I[I[kOvEn] + b] == en[b], "overlap: environment %d has %d", b, I[I[kOvEn] + b]);
  if (table_ok(I, I[kOvPo], (long long)(L + 2) * Q1 * p, 1, "overlap po"))
    for (int k = 0; k <= L + 1; ++k)
      for (int q = 0; q <= Q; ++q)
        for (int n = 0; n < p; ++n) {
          const int first = Y.at(k, q, n, 0, 0), got = I[I[kOvPo] + (k * Q1 + q) * p + n];
          CHECK(got == (first < 0 ? -1 : first - Y.site[k]), "overlap: block (%d, %d, %d) at %d", k, q, n, got);
        }
  if (table_ok(I, I[kOvSb], L + 2, 1, "overlap sb"))
    for (int k = 1; k <= L + 1; ++k) CHECK(I[I[kOvSb] + k] == Y.site[k], "overlap: site %d starts at %d", k, I[I[kOvSb] + k]);
  if (table_ok(I, I[kOvElo], L + 2, 1, "overlap elo")) {
    int tot = 0;
    for (int b = 0; b <= L + 1; ++b) {
      CHECK(I[I[kOvElo] + b] == tot, "overlap: element list %d at %d", b, I[I[kOvElo] + b]);
      if (b <= L) tot += en[b];
    }
    if (table_ok(I, I[kOvEl], tot, 1, "overlap el")) {
      int x = 0;
      for (int b = 0; b <= L; ++b)
        for (int q = 0; q <= Q; ++q)
          for (int c = 0; c < Y.d(b, q); ++c)
            for (int d = 0; d < Y.d(b, q); ++d, ++x) {
              const unsigned w = I[I[kOvEl] + x];
              CHECK(int(w & 255) == q && int((w >> 8) & 15) == c && int((w >> 12) & 15) == d && int(w >> 16) == Y.d(b, q),
                    "overlap: environment element %d", x);
            }
    }
  }
  if (table_ok(I, I[kOvLs], np, 4, "overlap elements")) {
    int b = -1;
    for (int x = 0; x < np; ++x) {
      const int* t = &I[I[kOvLs] + 4 * x];
      const Elem& e = Y.el[x];
      if (e.a == 0 && e.c == 0) ++b;
      const unsigned w0 = t[0], w1 = t[1], w2 = t[2];
      CHECK(int(w0 & 0xffff) == (e.k - 1) * Q1 + e.q && int(w0 >> 16) == e.k * Q1 + e.q + e.n &&
                int(w1 & 0xffff) == b && int(w1 >> 16) == Y.blk[b].first && int(w2 & 15) == e.a &&
                int((w2 >> 4) & 15) == e.c && int((w2 >> 8) & 15) == Y.d(e.k - 1, e.q) &&
                int((w2 >> 12) & 15) == Y.d(e.k, e.q + e.n) && int(w2 >> 16) == eo[(e.k - 1) * Q1 + e.q] &&
                t[3] == P.site_base[e.k],
            "overlap: padded element %d", x);
      // stage 1 reads E_(k-1)[q][., a] and Y_(q, n)[., c]: inside the environment and the site
      CHECK(eo[(e.k - 1) * Q1 + e.q] + Y.d(e.k - 1, e.q) * Y.d(e.k - 1, e.q) <= en[e.k - 1], "overlap: element %d leaves E", x);
    }
  }
  if (table_ok(I, I[kOvBlk], nblk, 1, "overlap blocks"))
    for (int b = 0; b < nblk; ++b) {
      const unsigned w = I[I[kOvBlk] + b];
      const auto& B = Y.blk[b];
      CHECK(int(w & 0xffff) == (B.k - 1) * Q1 + B.q && int(w >> 16) == B.k * Q1 + B.q + B.n, "overlap: block %d", b);
    }
  // the plan, two dims and two block-offset arrays as ints; both padded states, T and two environments, each
  // with its zero slot (with dH: another T and two more environments)
  auto al = [](int x) { return (x + 3) & ~3; };
  const long long ints = I[kOvNint] + 2LL * al(P.nsq) + 2LL * al(nblk + 1);
  const long long zs = 2LL * (np + 1) + (maxsite + 1) + 2LL * (maxen + 1), zd = (maxsite + 1) + 2LL * (maxen + 1);
  CHECK(ocg_host::overlap_lds_bytes(I, P) >= 4 * ints + 16 * zs &&
            ocg_host::overlap_lds_bytes(I, P, true) >= ocg_host::overlap_lds_bytes(I, P) + 16 * zd,
        "overlap_lds_bytes %d / %d below the furthest byte %lld / +%lld", ocg_host::overlap_lds_bytes(I, P),
        ocg_host::overlap_lds_bytes(I, P, true), 4 * ints + 16 * zs, 16 * zd);
}

int main() {
  int naccepted = 0, nshapes = 0;
  for (int L = 2; L <= 8; ++L)
    for (int p = 2; p <= 7; ++p)
      for (int Q = 1; Q <= 8 && Q <= L * (p - 1); ++Q) {
        gL = L; gp = p; gQ = Q;
        ++nshapes;
        OcgParams P;
        std::vector<int> md;
        std::vector<double> gf, gb;
        const std::string err = ocg_host::build_params(P, md, L, p, Q, 0.01, 1e-8, 5000);
        if (!err.empty()) { bad("no parameter block: %s", err.c_str()); continue; }
        ocg_host::gate_tables(P, 1.0, gf, gb);
        const Layout Y(L, p, Q);
        for (int x = 0; x < (L + 1) * (Q + 1); ++x) CHECK(md[x] == Y.D[x], "rank bound %d: %d, recomputed %d", x, md[x], Y.D[x]);
        const ocg_host::FastPlanBuild fb = ocg_host::build_fast_plan(P, md);
        const std::vector<int> ov = ocg_host::build_overlap_plan(P, md);
        if (!fb.why_not.empty()) {
          CHECK(fb.plan.empty(), "a rejected shape has a plan image");
          std::printf("%d %d %d rejected %s\n", L, p, Q, fb.why_not.c_str());
        } else {
          ++naccepted;
          const int before = g_bad;
          check_step_plan(P, fb.plan, Y);
          CHECK(!ov.empty(), "an accepted shape has no overlap plan");
          std::printf("%d %d %d accepted np %d ops %d ints %zu ovl %zu lds %d %s\n", L, p, Q, fb.plan[kHNp], fb.plan[kHNops],
                      fb.plan.size(), ov.size(), ocg_host::fast_lds_bytes(fb.plan, P), g_bad == before ? "ok" : "BAD");
        }
        // the overlap plan has its own eligibility (p <= 6, bounds <= 4, environments <= 128)
        if (!ov.empty()) check_overlap_plan(P, ov, Y);
      }
  std::printf("%d shapes, %d accepted, %d violations\n", nshapes, naccepted, g_bad);
  return g_bad ? 1 : 0;
}
