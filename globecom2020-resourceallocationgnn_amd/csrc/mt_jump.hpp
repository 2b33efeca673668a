// Jump-ahead polynomials of MT19937 over GF(2): host arithmetic for v2x_mt_jump_polys (v2xsimdev.hip), plain C++, no GPU call.
// The identity they serve is in include/v2xgnn.h.  Polynomials are bit vectors in 64-bit words, coefficient i in bit i & 63 of
// word i >> 6.
//   phi        Berlekamp-Massey on bit 0 of w[1], w[2], ... of the word stream the caller's twist makes from a fixed key array:
//              the connection polynomial C of the shortest recurrence s[n] = XOR_i C_i s[n - i], reversed (phi_j = C_(L - j)).
//              Any stream whose bit 0 has full linear complexity gives the same phi; the degree is checked against 19937.
//   reduce     a product of degree < 2 x 19937 modulo phi, a 64-bit word at a time from the top: the bits of a word at or above
//              x^19937 are XORed back at every lower term of phi.  phi's second term lies 227 below its first (more than a word),
//              so a word never folds into itself or a higher one; that gap is checked, not assumed.
//   square     bit spreading; x^J by square-and-shift from J's top bit down.
//   multiply   g h: the 64 shifts of h are made once, every set bit of g XORs one of them in at a word offset.
#pragma once
#include <cstdint>
#include <vector>

namespace mtjump {

constexpr int DEG = 19937, N = 624, M = 397;
constexpr int W = (DEG + 63) / 64;                   /* 312 words hold a reduced polynomial */
typedef std::vector<uint64_t> Poly;

struct Field {
  Poly phi;                                          /* W words, bit DEG set */
  std::vector<int> low;                              /* the exponents of phi's terms below x^DEG */
  bool ok = false;
};

inline int bit(const Poly& p, int64_t i) { return (int)((p[(size_t)(i >> 6)] >> (i & 63)) & 1u); }

// the 64 bits of r from bit `at` on (r has a spare word at the top)
inline uint64_t window(const Poly& r, int64_t at) {
  const size_t w = (size_t)(at >> 6);
  const int sh = (int)(at & 63);
  return sh ? (r[w] >> sh) | (r[w + 1] << (64 - sh)) : r[w];
}

// p ^= v << at, v a 64-bit piece
inline void xor_at(Poly& p, int64_t at, uint64_t v) {
  const size_t w = (size_t)(at >> 6);
  const int sh = (int)(at & 63);
  p[w] ^= v << sh;
  if (sh && (v >> (64 - sh))) p[w + 1] ^= v >> (64 - sh);
}

// Berlekamp-Massey over GF(2) on s[0 .. len): -> L, the connection polynomial in c (c_0 = 1).  The sequence is kept reversed
// (rev bit len - 1 - n = s[n]), so the discrepancy at n is the parity of c AND the window of rev from len - 1 - n on.
inline int berlekamp_massey(const std::vector<uint8_t>& s, Poly& c) {
  const int64_t len = (int64_t)s.size();
  const size_t words = (size_t)(len / 64 + 2);
  Poly rev(words + 1, 0), b(words, 0), t;
  for (int64_t n = 0; n < len; ++n)
    if (s[(size_t)n]) rev[(size_t)((len - 1 - n) >> 6)] |= 1ull << ((len - 1 - n) & 63);
  c.assign(words, 0);
  c[0] = b[0] = 1;
  int64_t L = 0, m = 1;
  for (int64_t n = 0; n < len; ++n) {
    uint64_t d = 0;
    const int64_t at = len - 1 - n;
    for (int64_t w = 0; w <= L >> 6; ++w) d ^= c[(size_t)w] & window(rev, at + 64 * w);
    if (!(__builtin_popcountll(d) & 1)) { ++m; continue; }
    const bool grow = 2 * L <= n;
    if (grow) t = c;
    for (int64_t w = 0; w <= (n >> 6); ++w)          /* c ^= b x^m: b's degree is at most n - m, so nothing passes bit n */
      if (b[(size_t)w]) xor_at(c, 64 * w + m, b[(size_t)w]);
    if (grow) { L = n + 1 - L; b.swap(t); m = 1; } else ++m;
  }
  return (int)L;
}

// phi of the recurrence word[i + 624] = twist(word[i], word[i + 1], word[i + 397]).  false: the stream did not give a
// polynomial of degree 19937 with a second term more than a word below the first (a bug, never an input).
inline bool make_field(uint32_t (*twist)(uint32_t, uint32_t, uint32_t), Field& f) {
  const int len = 2 * DEG + 256;
  std::vector<uint32_t> w((size_t)len + 2);
  uint32_t x = 19650218u;                            /* any key array that is not all zero: the generator's own seeding rule */
  for (int i = 0; i < N; ++i) { w[(size_t)i] = x; x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)(i + 1); }
  for (int i = 0; i + N < len + 2; ++i) w[(size_t)(i + N)] = twist(w[(size_t)i], w[(size_t)(i + 1)], w[(size_t)(i + M)]);
  std::vector<uint8_t> s((size_t)len);
  for (int i = 0; i < len; ++i) s[(size_t)i] = (uint8_t)(w[(size_t)(i + 1)] & 1u);
  Poly c;
  if (berlekamp_massey(s, c) != DEG) return false;
  f.phi.assign((size_t)W, 0);
  f.low.clear();
  for (int j = 0; j <= DEG; ++j)
    if (bit(c, DEG - j)) {
      f.phi[(size_t)(j >> 6)] |= 1ull << (j & 63);
      if (j < DEG) f.low.push_back(j);
    }
  if (!bit(f.phi, DEG) || f.low.empty() || f.low.back() > DEG - 64) return false;
  f.ok = true;
  return true;
}

// p (2 W words, degree < 2 DEG) modulo phi, in place; the words from W on end up zero
inline void reduce(const Field& f, Poly& p) {
  const int64_t edge = DEG >> 6;                     /* the word x^DEG lies in */
  for (int64_t w = (int64_t)p.size() - 1; w >= edge; --w) {
    uint64_t v = p[(size_t)w];
    int64_t at = 64 * w - DEG;                       /* v x^(64 w) = v x^at x^DEG */
    if (w == edge) { v >>= (DEG & 63); at = 0; }
    if (!v) continue;
    if (w == edge) p[(size_t)w] &= (1ull << (DEG & 63)) - 1; else p[(size_t)w] = 0;
    for (int t : f.low) xor_at(p, at + t, v);
  }
}

inline void square(const Field& f, Poly& g) {
  Poly p((size_t)(2 * W), 0);
  for (int w = 0; w < W; ++w) {
    uint64_t lo = g[(size_t)w] & 0xffffffffull, hi = g[(size_t)w] >> 32;
    for (uint64_t* h : { &lo, &hi }) {               /* spread 32 bits to the even positions of 64 */
      uint64_t v = *h;
      v = (v | (v << 16)) & 0x0000ffff0000ffffull;
      v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
      v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
      v = (v | (v << 2)) & 0x3333333333333333ull;
      v = (v | (v << 1)) & 0x5555555555555555ull;
      *h = v;
    }
    p[(size_t)(2 * w)] = lo;
    p[(size_t)(2 * w + 1)] = hi;
  }
  reduce(f, p);
  g.assign(p.begin(), p.begin() + W);
}

// g = x^J mod phi
inline void power_of_x(const Field& f, int64_t J, Poly& g) {
  g.assign((size_t)W, 0);
  g[0] = 1;
  int top = 62;
  while (top > 0 && !((J >> top) & 1)) --top;
  for (int b = top; b >= 0; --b) {
    square(f, g);
    if ((J >> b) & 1) {                              /* times x */
      Poly p((size_t)(2 * W), 0);
      uint64_t carry = 0;
      for (int w = 0; w < W; ++w) {
        p[(size_t)w] = (g[(size_t)w] << 1) | carry;
        carry = g[(size_t)w] >> 63;
      }
      reduce(f, p);
      g.assign(p.begin(), p.begin() + W);
    }
  }
}

// the 64 shifts of h, each W + 1 words: shifts[s] = h << s
inline void make_shifts(const Poly& h, std::vector<Poly>& shifts) {
  shifts.assign(64, Poly((size_t)(W + 1), 0));
  for (int s = 0; s < 64; ++s)
    for (int w = 0; w < W; ++w) xor_at(shifts[(size_t)s], 64 * w + s, h[(size_t)w]);
}

// g = g h mod phi, h given by its shifts
inline void multiply(const Field& f, Poly& g, const std::vector<Poly>& shifts) {
  Poly p((size_t)(2 * W + 1), 0);
  for (int w = 0; w < W; ++w) {
    uint64_t v = g[(size_t)w];
    while (v) {
      const int b = __builtin_ctzll(v);
      v &= v - 1;
      const uint64_t* src = shifts[(size_t)b].data();
      uint64_t* dst = p.data() + w;
      for (int k = 0; k <= W; ++k) dst[k] ^= src[k];
    }
  }
  reduce(f, p);
  g.assign(p.begin(), p.begin() + W);
}

// out[624] (32-bit words): coefficient i in bit i & 31 of word i >> 5
inline void store32(const Poly& g, uint32_t* out) {
  for (int w = 0; w < W; ++w) {
    out[2 * w] = (uint32_t)g[(size_t)w];
    out[2 * w + 1] = (uint32_t)(g[(size_t)w] >> 32);
  }
}

// out [count][624]: x^(J0 + p stride) mod phi, p = 0 .. count - 1
inline void jump_polys(const Field& f, int64_t J0, int64_t stride, int32_t count, uint32_t* out) {
  Poly g, h;
  power_of_x(f, J0, g);
  store32(g, out);
  if (count < 2) return;
  power_of_x(f, stride, h);
  std::vector<Poly> shifts;
  make_shifts(h, shifts);
  for (int32_t p = 1; p < count; ++p) {
    multiply(f, g, shifts);
    store32(g, out + (int64_t)p * N);
  }
}

}  // namespace mtjump
