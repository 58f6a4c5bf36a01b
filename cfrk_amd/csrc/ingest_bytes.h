// ingest_bytes.h -- byte twiddling shared by the text parsers (ingest.hip: FASTA, ingest_fastq.hip: FASTQ): 16 bytes
// of text per lane as four words, byte tests as 16-bit masks (bit j = byte j), the base codes four to a word.
#pragma once
#include "common.h"

// 4 bytes -> 4 bits (bit j = byte j equals the pattern byte); exact: no carries between bytes
__device__ __forceinline__ uint32_t fa_eq4(uint32_t w, uint32_t pat) {
  const uint32_t x = w ^ pat;
  const uint32_t f = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
  return ((f >> 7) * 0x01020408u) >> 24;      // bits 0, 8, 16, 24 -> 24..27: every partial product has a bit of its own
}
__device__ __forceinline__ uint32_t fa_eq16(uint4 v, uint32_t pat) {
  return fa_eq4(v.x, pat) | (fa_eq4(v.y, pat) << 4) | (fa_eq4(v.z, pat) << 8) | (fa_eq4(v.w, pat) << 12);
}
// aA cC gG tT -> 0 1 2 3, anything else -> 0xFF (the host parser's encode_avx2, four bytes to a word)
__device__ __forceinline__ uint32_t fa_code4(uint32_t w) {
  const uint32_t u = w & 0xDFDFDFDFu;
  auto zero = [](uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; };
  const uint32_t ok = zero(u ^ 0x41414141u) | zero(u ^ 0x43434343u) | zero(u ^ 0x47474747u) | zero(u ^ 0x54545454u);
  const uint32_t x = (u >> 1) & 0x03030303u;
  const uint32_t code = x ^ ((x >> 1) & 0x01010101u);
  return code | ~((ok >> 7) * 0xFFu);
}

// a lane's 16 bytes at p0 (a multiple of 16; the text is 16-byte aligned); bytes at or behind n read 0
__device__ __forceinline__ uint4 fa_load(const uint8_t *__restrict__ text, uint64_t p0, uint64_t n, uint32_t &valid) {
  if (p0 + 16 <= n) {
    valid = 0xFFFFu;
    return *reinterpret_cast<const uint4 *>(text + p0);
  }
  uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
  valid = 0;
  if (p0 < n) {
    const int m = (int)(n - p0);
    valid = (1u << m) - 1u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t c = (j < m) ? (uint32_t)text[p0 + j] : 0u;
      if (j < 4) w0 |= c << (8 * (j & 3));
      else if (j < 8) w1 |= c << (8 * (j & 3));
      else if (j < 12) w2 |= c << (8 * (j & 3));
      else w3 |= c << (8 * (j & 3));
    }
  }
  return make_uint4(w0, w1, w2, w3);
}
