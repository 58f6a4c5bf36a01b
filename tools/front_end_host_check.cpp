// front_end_host_check.cpp -- the partition front end's word arithmetic, old form against new form, on the CPU,
// outside pytest.  Built and run as the other *_host_check.cpp programs are:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o front_end_host_check tools/front_end_host_check.cpp
//   ./front_end_host_check
//
// Three pieces of the front end were rewritten for fewer vector instructions and must give the same words:
//
//   B  dev_load_chunk32 (common.h), full-chunk branch: 32 code bytes -> two words of packed bases and the invalid mask.
//      Old: dev_pack4 / dev_bad4 per word, shifted and or-ed into place.  New: the products' top bytes through two
//      v_perm_b32 per 16 bases, the flag gathers through a chain of v_alignbit by 4.  Both against the byte-wise
//      definition (the loader's tail branch) as well.
//   A  msp_minimizers (msp_dev.h): the canonical m-mer of each of a lane's 32 positions.  Old: forward m-mer = top bits
//      of a window shifted down, reverse complement = low bits of a window masked, minimum of the two.  New: the
//      reverse-complemented string moved left by 32 - 2m bits once, both windows top-aligned, the minimum shifted down.
//   C  the validity smear of p1_tile (msp.hip): old on two 64-bit words, new on three 32-bit words with v_alignbit.
//
// v_alignbit_b32, v_perm_b32 and v_mul_hi_u32 are emulated below as the ISA defines them.  Inputs: triples of 32-byte
// chunks (a lane's, the next lane's, the one after) -- random with invalid bytes of every value 4..255 mixed in at
// several densities, all one base, period 2, period 4, and strings followed by their reverse complement (palindromic
// m-mers at every even m) -- with m in {12, 13, 14, 16} and k = 16..32.  Prints one summary line; exit status 1 on the
// first difference.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

// ---- the three instructions
static uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t s) {          // ({hi, lo} >> s[4:0])[31:0]
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31u));
}
static uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {            // byte select from {s0, s1}
  const uint64_t both = ((uint64_t)s0 << 32) | s1;
  uint32_t out = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t c = (sel >> (8 * i)) & 255u;
    uint32_t b;
    if (c <= 7) b = (uint32_t)(both >> (8 * c)) & 255u;
    else if (c <= 11) b = ((both >> (16 * (c - 8) + 15)) & 1u) ? 255u : 0u;   // sign of a 16-bit half
    else if (c == 12) b = 0;
    else b = 255u;
    out |= b << (8 * i);
  }
  return out;
}
static uint32_t umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

static int fail(const char *what, long long at, int p0, int p1, unsigned long long a, unsigned long long b) {
  printf("DIFFERENCE in %s: input %lld, parameters %d %d: old %llx new %llx\n", what, at, p0, p1, a, b);
  return 1;
}

// ---- B: the loader
static uint32_t pack4(uint32_t w) { return ((w & 0x03030303u) * 0x40100401u) >> 24; }
static uint32_t bad4(uint32_t w) {
  const uint32_t f = (((w & 0x7C7C7C7Cu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
  return umulhi(f, 0x10080402u) & 15u;
}
static void pack16(const uint32_t *v, uint32_t &bases, uint32_t &bad) {
  bases = (pack4(v[0]) << 24) | (pack4(v[1]) << 16) | (pack4(v[2]) << 8) | pack4(v[3]);
  bad = (bad4(v[0]) << 12) | (bad4(v[1]) << 8) | (bad4(v[2]) << 4) | bad4(v[3]);
}
static void load_old(const uint32_t *w, uint32_t &b0, uint32_t &b1, uint32_t &bad) {
  uint32_t m0, m1;
  pack16(w, b0, m0);
  pack16(w + 4, b1, m1);
  bad = (m0 << 16) | m1;
}
static void load_new(const uint32_t *w, uint32_t &b0, uint32_t &b1, uint32_t &bad) {
  uint32_t pr[8];
  for (int i = 0; i < 8; ++i) pr[i] = (w[i] & 0x03030303u) * 0x40100401u;
  b0 = perm(pr[0], pr[1], 0x07030c0cu) | perm(pr[2], pr[3], 0x0c0c0703u);
  b1 = perm(pr[4], pr[5], 0x07030c0cu) | perm(pr[6], pr[7], 0x0c0c0703u);
  uint32_t acc = 0;
  for (int i = 7; i >= 0; --i) {
    const uint32_t f = (((w[i] & 0x7C7C7C7Cu) + 0x7F7F7F7Fu) | w[i]) & 0x80808080u;
    acc = alignbit(umulhi(f, 0x10080402u), acc, 4);
  }
  bad = acc;
}
// the definition, byte by byte.  (An invalid byte packs as its low two bits here and as 0 in the loader's tail branch:
// the bases of an invalid position are never used.)
static void load_bytes(const uint8_t *c, uint32_t &b0, uint32_t &b1, uint32_t &bad) {
  b0 = b1 = bad = 0;
  for (int j = 0; j < 32; ++j) {
    const bool inv = c[j] > 3;
    const uint32_t v = c[j] & 3u;
    if (j < 16) b0 |= v << (30 - 2 * j); else b1 |= v << (30 - 2 * (j - 16));
    if (inv) bad |= 1u << (31 - j);
  }
}

// ---- A: the canonical m-mers of a lane's 32 positions (before the multiply: the hash is a function of the value)
static void revcomp_words(const uint32_t *D, uint32_t *R) {               // R[1..3]; the caller sets R[0] (and R[4])
  for (int i = 0; i < 3; ++i) {
    uint32_t x = D[i];                                                    // v_bfrev_b32
    x = (x >> 16) | (x << 16);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    R[3 - i] = ~x;
  }
}
static void mmers_old(const uint32_t *D, int m, uint32_t *out) {
  uint32_t R[5];
  revcomp_words(D, R);
  R[0] = 0; R[4] = 0;                                                      // (R[4]: never read, as in the kernel)
  const uint32_t mmask = (m == 16) ? 0xFFFFFFFFu : ((1u << (2 * m)) - 1u);
  const int fsh = 32 - 2 * m;
  for (int j = 0; j < 32; ++j) {
    const int o = 2 * j, q = o >> 5, r = o & 31;
    const uint32_t X = r ? alignbit(D[q], D[q + 1], 32 - r) : D[q];
    const int o2 = 96 - 2 * j, q2 = o2 >> 5, r2 = o2 & 31;
    const uint32_t Y = r2 ? alignbit(R[q2], R[q2 + 1], 32 - r2) : R[q2];
    const uint32_t fm = X >> fsh, rm = Y & mmask;
    out[j] = fm < rm ? fm : rm;
  }
}
static void mmers_new(const uint32_t *D, int m, uint32_t *out) {
  uint32_t R[5], RS[5];
  revcomp_words(D, R);
  R[0] = 0; R[4] = 0;
  const int fsh = 32 - 2 * m;
  RS[0] = 0; RS[4] = 0;
  for (int i = 1; i < 4; ++i) RS[i] = fsh ? alignbit(R[i], R[i + 1], 32 - fsh) : R[i];
  for (int j = 0; j < 32; ++j) {
    const int o = 2 * j, q = o >> 5, r = o & 31;
    const uint32_t X = r ? alignbit(D[q], D[q + 1], 32 - r) : D[q];
    const int o2 = 96 - 2 * j, q2 = o2 >> 5, r2 = o2 & 31;
    const uint32_t Y = r2 ? alignbit(RS[q2], RS[q2 + 1], 32 - r2) : RS[q2];
    out[j] = (X < Y ? X : Y) >> fsh;
  }
}
// the definition, base by base: the smaller of the m-mer at position j and its reverse complement
static uint32_t mmer_plain(const uint8_t *codes, int j, int m) {
  uint32_t f = 0, r = 0;
  for (int i = 0; i < m; ++i) {
    f = (f << 2) | codes[j + i];
    r |= (uint32_t)(3 - codes[j + i]) << (2 * i);
  }
  return f < r ? f : r;
}

// ---- C: the validity words of a lane from the invalid masks of its chunk and the next two
static uint64_t smear_old(uint32_t bad, uint32_t nbad, uint32_t nnbad, int k) {
  uint64_t Yh = ((uint64_t)bad << 32) | nbad, Yl = (uint64_t)nnbad << 32;
  int w = 1;
  for (int st = 0; st < 5; ++st) {
    if (2 * w <= k) {
      Yh |= (Yh << w) | (Yl >> (64 - w));
      Yl |= Yl << w;
      w *= 2;
    }
  }
  if (k > w) {
    Yh |= (Yh << (k - w)) | (Yl >> (64 - (k - w)));
    Yl |= Yl << (k - w);
  }
  return ~Yh;
}
static uint64_t smear_new(uint32_t bad, uint32_t nbad, uint32_t nnbad, int k) {
  uint32_t Q0 = bad, Q1 = nbad, Q2 = nnbad;
  int w = 1;
  for (int st = 0; st < 5; ++st) {
    if (2 * w <= k) {
      Q0 |= alignbit(Q0, Q1, 32 - w);
      Q1 |= alignbit(Q1, Q2, 32 - w);
      Q2 |= Q2 << w;
      w *= 2;
    }
  }
  if (k > w) {
    Q0 |= alignbit(Q0, Q1, 32 - (k - w));
    Q1 |= alignbit(Q1, Q2, 32 - (k - w));
  }
  return ~(((uint64_t)Q0 << 32) | Q1);
}
// the definition: position p (0..63) is valid when none of the bases p .. p+k-1 is invalid
static uint64_t smear_plain(const uint8_t *codes, int k) {
  uint64_t v = 0;
  for (int p = 0; p < 64; ++p) {
    bool ok = true;
    for (int i = 0; i < k; ++i) ok = ok && codes[p + i] <= 3;
    if (ok) v |= 1ull << (63 - p);
  }
  return v;
}

static const int MS[4] = {12, 13, 14, 16};
static size_t n_chunks = 0, n_mmers = 0, n_ties = 0, n_smears = 0, n_invalid = 0;
static bool seen_value[256];

// one triple of chunks through B, A and C; 0 when everything agrees.  Old against new on every input; the base-wise
// definitions of A and C, which cost many times more, on the constructed inputs and on every eighth random one.
static int check(const uint8_t *codes /* 96 bytes */, long long at, bool plain) {
  uint32_t b[3][2], bad[3];
  for (int c = 0; c < 3; ++c) {
    uint32_t w[8];
    memcpy(w, codes + 32 * c, 32);                                        // first base in the lowest byte, as on the device
    uint32_t o0, o1, ob, p0, p1, pb;
    load_old(w, o0, o1, ob);
    load_new(w, b[c][0], b[c][1], bad[c]);
    load_bytes(codes + 32 * c, p0, p1, pb);
    if (o0 != b[c][0]) return fail("B bases 0..15", at, c, 0, o0, b[c][0]);
    if (o1 != b[c][1]) return fail("B bases 16..31", at, c, 0, o1, b[c][1]);
    if (ob != bad[c]) return fail("B invalid mask", at, c, 0, ob, bad[c]);
    if (p0 != o0 || p1 != o1 || pb != ob) return fail("B against the byte-wise definition", at, c, 0, pb, ob);
    ++n_chunks;
  }
  for (int j = 0; j < 96; ++j) { seen_value[codes[j]] = true; n_invalid += codes[j] > 3; }
  const uint32_t D[3] = {b[0][0], b[0][1], b[1][0]};
  uint8_t clean[96];
  for (int j = 0; j < 96; ++j) clean[j] = codes[j] & 3;                  // (what the full-chunk loader packs)
  for (int mi = 0; mi < 4; ++mi) {
    uint32_t a[32], n[32];
    mmers_old(D, MS[mi], a);
    mmers_new(D, MS[mi], n);
    for (int j = 0; j < 32; ++j) {
      if (a[j] != n[j]) return fail("A canonical m-mer", at, MS[mi], j, a[j], n[j]);
      // (the words hold 48 bases: the plain form is defined while the m-mer lies inside them)
      if (plain && j + MS[mi] <= 48 && mmer_plain(clean, j, MS[mi]) != n[j]) return fail("A against the base-wise definition", at, MS[mi], j, mmer_plain(clean, j, MS[mi]), n[j]);
      ++n_mmers;
    }
    // how many positions tie in the top bits (the case the rewrite has to get right)
    for (int j = 0; plain && j + MS[mi] <= 48 && j < 32; ++j) {
      uint32_t f = 0, r = 0;
      for (int i = 0; i < MS[mi]; ++i) { f = (f << 2) | clean[j + i]; r |= (uint32_t)(3 - clean[j + i]) << (2 * i); }
      n_ties += f == r;
    }
  }
  for (int k = 16; k <= 32; ++k) {
    const uint64_t a = smear_old(bad[0], bad[1], bad[2], k), n = smear_new(bad[0], bad[1], bad[2], k);
    if (a != n) return fail("C validity", at, k, 0, a, n);
    if (plain && smear_plain(codes, k) != n) return fail("C against the base-wise definition", at, k, 0, smear_plain(codes, k), n);
    ++n_smears;
  }
  return 0;
}

int main() {
  uint8_t codes[96];
  long long at = 0;
  // all one base; period 2 and period 4 at every phase and every choice of bases
  for (int a = 0; a < 4; ++a) {
    memset(codes, a, sizeof codes);
    if (check(codes, at++, true)) return 1;
    for (int b = 0; b < 4; ++b) {
      for (int j = 0; j < 96; ++j) codes[j] = (uint8_t)((j & 1) ? b : a);
      if (check(codes, at++, true)) return 1;
    }
  }
  for (int q = 0; q < 256; ++q) {
    const uint8_t unit[4] = {(uint8_t)(q & 3), (uint8_t)((q >> 2) & 3), (uint8_t)((q >> 4) & 3), (uint8_t)(q >> 6)};
    for (int ph = 0; ph < 4; ++ph) {
      for (int j = 0; j < 96; ++j) codes[j] = unit[(j + ph) & 3];
      if (check(codes, at++, true)) return 1;
    }
  }
  // a random string followed by its reverse complement, the joint at every place of the first 48 bases: palindromic
  // m-mers (even m) at the joint, and windows that tie in their top bits with different neighbours below
  for (int round = 0; round < 20000; ++round) {
    const int joint = 1 + (int)(rnd() % 47), off = (int)(rnd() % 3);
    for (int j = 0; j < 96; ++j) codes[j] = (uint8_t)(rnd() & 3);
    for (int i = 0; joint + i < 96 && joint - 1 - i >= 0; ++i) codes[joint + i] = (uint8_t)(3 - codes[joint - 1 - i]);
    if (off == 1) codes[rnd() % 96] = (uint8_t)(4 + rnd() % 252);          // sometimes an invalid byte beside it
    if (check(codes, at++, true)) return 1;
  }
  // random triples, invalid bytes of every value mixed in at densities from none to most
  uint32_t next_value = 4;
  for (int round = 0; round < 400000; ++round) {
    const uint64_t density = (round % 8 == 0) ? 0 : (round % 8 == 7) ? 2 : (uint64_t)(4 << (round % 8));   // 1 in `density`
    for (int j = 0; j < 96; ++j) {
      codes[j] = (uint8_t)(rnd() & 3);
      if (density && rnd() % density == 0) {
        codes[j] = (uint8_t)next_value;                                      // every value 4..255 in turn
        next_value = next_value == 255 ? 4 : next_value + 1;
      }
    }
    if (check(codes, at++, round % 8 == 0)) return 1;
  }
  for (int v = 0; v < 256; ++v)
    if (!seen_value[v]) { printf("byte value %d never seen\n", v); return 1; }
  if (n_chunks < 1000000 || n_ties < 10000) { printf("too few inputs: %zu chunks, %zu ties\n", n_chunks, n_ties); return 1; }
  printf("old and new front end agree: %zu chunks (%zu invalid bytes, every value seen), %zu m-mers (%zu palindromic) at m = 12, 13, 14, 16, "
         "%zu validity words at k = 16..32\n", n_chunks, n_invalid, n_mmers, n_ties, n_smears);
  return 0;
}
