// Host core of the MX load self-test: the OCP e4m3 and e2m1 element formats,
// the E8M0 scale, the operand generator, the bounds on K and the checksum of
// the golden product. No HIP and no pybind includes, so
// mxtest_core_selftest.cpp can drive it under AddressSanitizer and UBSan
// without a GPU; mxtest_kernels.hpp includes it for the device build, where
// LT_HD makes the formats and the generator callable from a kernel.
//
// An MX operand is [rows][K] elements with one E8M0 scale per 32 consecutive
// k of a row; the value of an element is decode(code) * 2^(scale - 127).
// Generated values, per format:
//
//   mxfp8  element an integer v in [-8, 8] as e4m3, scale 2^e, e in {-1,0,1}
//   mxfp4  element any of the 16 e2m1 codes (a multiple of 2^-1, |x| <= 6),
//          scale 2^e, e in {-1, 0, 1}
//
// Every scaled element is a multiple of 2^-2 and is kept here as that
// multiple ("quarter units"); every product is a whole number of units of
// 2^-4. tests/mxtest_reference.py mirrors all of this in numpy.

#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "loadtest_core.hpp"  // LT_HD, lt_mix, LtChecksum, kLtMaxMN

enum MxFormat { kMxFp8 = 0, kMxFp4 = 1 };
constexpr int kMxFormats = 2;

constexpr int kMxTile = 128;   // output tile edge: M and N are multiples of it
constexpr int kMxBK = 128;     // K-step, the K of one scaled MFMA
constexpr int kMxBlock = 32;   // consecutive k that share one scale
constexpr int kMxScaleBias = 127;

// Largest magnitude of a scaled element in quarter units: 8 * 2^1 = 16 for
// mxfp8, 6 * 2^1 = 12 for mxfp4.
constexpr long long kMxFp8MaxQuarter = 64;
constexpr long long kMxFp4MaxQuarter = 48;

// Why K stops where it does. A product of two scaled elements is a whole
// number of units of 2^-4. A sum of up to K of them, taken in any order and
// grouped in any way, is a whole number of units of magnitude at most
// (largest product) * K; while that is at most 2^24 it fits fp32's 24-bit
// significand and no addition ever rounds, so the MFMA's adder tree and the
// golden kernel's k-ordered fmaf chain must agree bit for bit.
//   mxfp4: the largest product is 48 * 48 = 2304 units (144.0);
//          2304 * K <= 2^24 gives K <= 7281, so 7168 in multiples of 128.
//   mxfp8: scaled elements are multiples of 2^-1, so a product is a multiple
//          of 4 units of magnitude at most 64 * 64 = 4096 (256.0): the same
//          bounds as the bf16 load test, and the same cap with the same
//          spare bit: 4096 / 4 * K <= 2^23 gives K <= 8192.
constexpr int kMxFp8MaxK = 8192;
constexpr int kMxFp4MaxK = 7168;
static_assert(kMxFp8MaxQuarter * kMxFp8MaxQuarter / 4 * kMxFp8MaxK <=
                  (1ll << 24) / 2,
              "mxfp8 partial sums in units of 2^-2 stay inside 24 bits");
static_assert(kMxFp4MaxQuarter * kMxFp4MaxQuarter * kMxFp4MaxK <= (1ll << 24),
              "mxfp4 partial sums in units of 2^-4 stay inside 24 bits");
static_assert(kMxFp8MaxK % kMxBK == 0 && kMxFp4MaxK % kMxBK == 0 &&
                  kMxFp8MaxK >= 4096 && kMxFp4MaxK >= 4096,
              "caps are whole K-steps and admit the default K");

LT_HD inline int mx_max_k(int format) {
  return format == kMxFp4 ? kMxFp4MaxK : kMxFp8MaxK;
}

inline const char* mx_format_name(int format) {
  return format == kMxFp4 ? "mxfp4" : "mxfp8";
}

// kMxFp8, kMxFp4 or throws std::invalid_argument.
inline int mx_format_from_name(const std::string& name) {
  if (name == "mxfp8") return kMxFp8;
  if (name == "mxfp4") return kMxFp4;
  throw std::invalid_argument("format must be mxfp8 or mxfp4, got '" + name +
                              "'");
}

// Bytes of `k` elements of one row: one per element for e4m3, two elements
// per byte for e2m1 (the even k in the low nibble).
LT_HD inline size_t mx_row_bytes(int format, size_t k) {
  return format == kMxFp4 ? k / 2 : k;
}

// ---------------------------------------------------------------------------
// formats
// ---------------------------------------------------------------------------
LT_HD inline float mx_bits_to_float(uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(bits);
#else
  float f;
  std::memcpy(&f, &bits, sizeof f);
  return f;
#endif
}

// 2^e for e in [-126, 127].
LT_HD inline float mx_pow2(int e) {
  return mx_bits_to_float((uint32_t)(e + 127) << 23);
}

// E8M0: byte b is 2^(b - 127); 0xFF is NaN. Byte 0 is 2^-127, an fp32
// subnormal.
LT_HD inline float mx_e8m0_to_float(uint8_t b) {
  if (b == 0xFF) return mx_bits_to_float(0x7FC00000u);
  if (b == 0) return mx_bits_to_float(0x00400000u);
  return mx_bits_to_float((uint32_t)b << 23);
}

// OCP e4m3fn: sign, 4 exponent bits of bias 7, 3 mantissa bits; no
// infinities, S.1111.111 is NaN, the largest finite value is 448.
LT_HD inline float mx_e4m3_to_float(uint8_t code) {
  int e = (code >> 3) & 15, m = code & 7;
  float mag;
  if (e == 15 && m == 7)
    return mx_bits_to_float(0x7FC00000u);
  else if (e == 0)
    mag = (float)m * mx_pow2(-9);  // subnormal: m / 8 * 2^-6
  else
    mag = (float)(8 + m) * mx_pow2(e - 10);  // (1 + m / 8) * 2^(e - 7)
  return (code & 0x80) ? -mag : mag;
}

// OCP e2m1: sign, 2 exponent bits of bias 1, 1 mantissa bit:
// 0, 0.5, 1, 1.5, 2, 3, 4, 6.
LT_HD inline float mx_e2m1_to_float(uint8_t code) {
  int e = (code >> 1) & 3, m = code & 1;
  float mag = e == 0 ? (float)m * 0.5f : (float)(2 + m) * mx_pow2(e - 2);
  return (code & 8) ? -mag : mag;
}

// e2m1 code in half units (multiples of 2^-1), sign included; -0 is 0.
LT_HD inline int mx_e2m1_half_units(uint8_t code) {
  int e = (code >> 1) & 3, m = code & 1;
  int mag = e == 0 ? m : (2 + m) << (e - 1);
  return (code & 8) ? -mag : mag;
}

// e4m3 code of the integer v, |v| <= 15: exact, since v has at most four
// significant bits.
LT_HD inline uint8_t mx_e4m3_from_int(int v) {
  int mag = v < 0 ? -v : v;
  if (mag == 0) return 0;
  int p = 0;
  while ((mag >> (p + 1)) != 0) ++p;  // mag = 1.xxx * 2^p
  int m = ((mag << 3) >> p) & 7;
  return (uint8_t)((v < 0 ? 0x80 : 0) | ((p + 7) << 3) | m);
}

// ---------------------------------------------------------------------------
// generator
// ---------------------------------------------------------------------------
// Key spaces: bits 60.. hold the format + 1 (the bf16 load test's keys have
// them clear), bit 57 tells scales from elements, bit 56 B^T from A.
LT_HD inline uint64_t mx_key(int format, int scale, int which, uint64_t row,
                             uint64_t col) {
  return ((uint64_t)(format + 1) << 60) | ((uint64_t)scale << 57) |
         ((uint64_t)which << 56) | (row << 28) | col;
}

// Element (row, k) of operand `which` as its code: an e4m3 byte or an e2m1
// nibble.
LT_HD inline uint8_t mx_element_code(uint64_t seed, int format, int which,
                                     uint64_t row, uint64_t k) {
  uint64_t r = lt_mix(seed + mx_key(format, 0, which, row, k));
  if (format == kMxFp4) return (uint8_t)(r % 16);
  return mx_e4m3_from_int((int)(r % 17) - 8);
}

// Scale byte of block `kb` (k = 32 * kb ... 32 * kb + 31) of row `row`:
// 2^-1, 2^0 or 2^1.
LT_HD inline uint8_t mx_scale_byte(uint64_t seed, int format, int which,
                                   uint64_t row, uint64_t kb) {
  uint64_t r = lt_mix(seed + mx_key(format, 1, which, row, kb));
  return (uint8_t)(kMxScaleBias - 1 + (int)((r >> 32) % 3));
}

// The scaled element in quarter units (multiples of 2^-2), from the
// generator alone: |q| <= 64 for mxfp8, 48 for mxfp4.
LT_HD inline int mx_quarter_units(uint64_t seed, int format, int which,
                                  uint64_t row, uint64_t k) {
  uint64_t r = lt_mix(seed + mx_key(format, 0, which, row, k));
  int e = (int)mx_scale_byte(seed, format, which, row, k / kMxBlock) -
          kMxScaleBias;  // -1, 0, 1
  if (format == kMxFp4)
    return mx_e2m1_half_units((uint8_t)(r % 16)) * (1 << (e + 1));
  return ((int)(r % 17) - 8) * (1 << (e + 2));
}

// Throws std::invalid_argument unless (m, n, k) is a shape the kernels take
// for this format. Called before any allocation or launch.
inline void mx_check_shape(int format, long long m, long long n,
                           long long k) {
  auto bad = [](const std::string& what) {
    throw std::invalid_argument(what);
  };
  if (format != kMxFp8 && format != kMxFp4)
    bad("unknown MX format " + std::to_string(format));
  if (m < kMxTile || m > kLtMaxMN || m % kMxTile != 0)
    bad("m must be a multiple of 128 in [128, 16384], got " +
        std::to_string(m));
  if (n < kMxTile || n > kLtMaxMN || n % kMxTile != 0)
    bad("n must be a multiple of 128 in [128, 16384], got " +
        std::to_string(n));
  const int cap = mx_max_k(format);
  if (k < kMxBK || k > cap || k % kMxBK != 0)
    bad(std::string(mx_format_name(format)) +
        ": k must be a multiple of 128 in [128, " + std::to_string(cap) +
        "] (above it a partial sum may not be exact in fp32), got " +
        std::to_string(k));
}

// Packed elements of one operand: [rows][k] bytes for mxfp8, [rows][k / 2]
// for mxfp4 with the even k in the low nibble.
inline std::vector<uint8_t> mx_generate(uint64_t seed, int format, int which,
                                        int rows, int k) {
  const size_t rb = mx_row_bytes(format, (size_t)k);
  std::vector<uint8_t> out((size_t)rows * rb, 0);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < k; ++c) {
      uint8_t code = mx_element_code(seed, format, which, r, c);
      if (format == kMxFp4)
        out[(size_t)r * rb + c / 2] |= (uint8_t)(code << (4 * (c & 1)));
      else
        out[(size_t)r * rb + c] = code;
    }
  return out;
}

// Scale bytes of one operand, [rows][k / 32].
inline std::vector<uint8_t> mx_generate_scales(uint64_t seed, int format,
                                               int which, int rows, int k) {
  const int kb = k / kMxBlock;
  std::vector<uint8_t> out((size_t)rows * kb);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < kb; ++c)
      out[(size_t)r * kb + c] = mx_scale_byte(seed, format, which, r, c);
  return out;
}

// Row sums and column sums of `golden` ([m][n] fp32) against A * (B * 1) and
// (1^T * A) * B, in int64 units of 2^-4, from this file's generator alone:
// O(mk + nk + mn) work. An element that is not a whole number of units makes
// its row offend. The report has the shape of lt_checksum's.
inline LtChecksum mx_checksum(uint64_t seed, int format, int m, int n, int k,
                              const float* golden) {
  std::vector<int8_t> a((size_t)m * k), b((size_t)n * k);
  std::vector<long long> asum(k, 0), bsum(k, 0);
  for (int i = 0; i < m; ++i)
    for (int c = 0; c < k; ++c) {
      int q = mx_quarter_units(seed, format, kLtA, i, c);
      a[(size_t)i * k + c] = (int8_t)q;
      asum[c] += q;
    }
  for (int j = 0; j < n; ++j)
    for (int c = 0; c < k; ++c) {
      int q = mx_quarter_units(seed, format, kLtB, j, c);
      b[(size_t)j * k + c] = (int8_t)q;
      bsum[c] += q;
    }
  std::vector<long long> col_got(n, 0);
  LtChecksum res;
  for (int i = 0; i < m; ++i) {
    long long want = 0, got = 0;
    for (int c = 0; c < k; ++c) want += a[(size_t)i * k + c] * bsum[c];
    bool whole = true;
    for (int j = 0; j < n; ++j) {
      float q = golden[(size_t)i * n + j] * 16.0f;
      // |q| <= 2^25 for a correct product (mxfp8 at its cap; multiples of
      // 4 there); anything else offends
      if (!(q >= -33554432.0f && q <= 33554432.0f) ||
          (float)(long long)q != q) {
        whole = false;
        continue;
      }
      got += (long long)q;
      col_got[j] += (long long)q;
    }
    if ((!whole || got != want) && res.ok) {
      res.ok = false;
      res.is_row = true;
      res.index = i;
    }
  }
  if (!res.ok) return res;
  for (int j = 0; j < n; ++j) {
    long long want = 0;
    for (int c = 0; c < k; ++c) want += asum[c] * b[(size_t)j * k + c];
    if (col_got[j] != want) {
      res.ok = false;
      res.is_row = false;
      res.index = j;
      return res;
    }
  }
  return res;
}
