// Host core of the load self-test: the operand generator, the bound on K
// and the checksum of the golden product. No HIP and no pybind includes, so
// loadtest_core_selftest.cpp can drive it under AddressSanitizer and UBSan
// without a GPU; loadtest_kernels.hpp includes it for the device build, where
// LT_HD makes the generator callable from a kernel.
//
// Operand values are v * 2^e with integer v in [-8, 8] and e in {-1, 0, 1}:
// every one is a multiple of 2^-1 of magnitude at most 16, and is kept here
// as that multiple ("half units", an integer in [-32, 32]). tests/
// loadtest_reference.py mirrors the generator in numpy.

#pragma once

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define LT_HD __host__ __device__
#else
#define LT_HD
#endif

constexpr int kLtTile = 128;  // output tile edge: M and N are multiples of it
constexpr int kLtBK = 64;     // K-step: K is a multiple of it
constexpr int kLtMinK = 64;
// Why K stops here. A product of two operands is a multiple of 2^-2 of
// magnitude at most 16 * 16 = 256. A sum of up to K of them, taken in any
// order and grouped in any way, is a multiple of 2^-2 of magnitude at most
// 256 * K. At K = 8192 that is 2^21, which is 2^23 units of 2^-2: every
// partial sum is an integer number of units below 2^24, so it fits fp32's
// 24-bit significand and no addition ever rounds. The kernel under load and
// the golden kernel add in different orders and must still agree bit for bit.
constexpr int kLtMaxK = 8192;
static_assert(256ll * kLtMaxK * 4 <= (1ll << 24) / 2,
              "partial sums in units of 2^-2 stay inside 24 bits");
constexpr int kLtMaxMN = 16384;  // 1 GiB of fp32 C at the most

enum LtOperand { kLtA = 0, kLtB = 1 };

// splitmix64 finaliser, the same function as st_mix of selftest_kernels.hpp;
// mix(0) = 0xE220A8397B1DCDAF.
LT_HD inline uint64_t lt_mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Element (row, k) of operand `which` (A is [M][K], B is kept as B^T [N][K])
// in half units: v * 2^(e + 1).
LT_HD inline int lt_half_units(uint64_t seed, int which, uint64_t row,
                               uint64_t k) {
  uint64_t key = ((uint64_t)which << 56) | (row << 28) | k;
  uint64_t r = lt_mix(seed + key);
  int v = (int)(r % 17) - 8;
  int e = (int)((r >> 32) % 3) - 1;
  return v * (1 << (e + 1));
}

// bf16 bit pattern of h half units, |h| <= 32: at most six significant bits,
// so the low half of the fp32 pattern is zero and the shift drops nothing.
LT_HD inline uint16_t lt_bf16_bits(int h) {
  float f = (float)h * 0.5f;
  uint32_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
  bits = __float_as_uint(f);
#else
  std::memcpy(&bits, &f, sizeof bits);
#endif
  return (uint16_t)(bits >> 16);
}

// Throws std::invalid_argument unless (m, n, k) is a shape the kernels take.
// Called before any allocation or launch.
inline void lt_check_shape(long long m, long long n, long long k) {
  auto bad = [](const std::string& what) {
    throw std::invalid_argument(what);
  };
  if (m < kLtTile || m > kLtMaxMN || m % kLtTile != 0)
    bad("m must be a multiple of 128 in [128, 16384], got " +
        std::to_string(m));
  if (n < kLtTile || n > kLtMaxMN || n % kLtTile != 0)
    bad("n must be a multiple of 128 in [128, 16384], got " +
        std::to_string(n));
  if (k < kLtMinK || k > kLtMaxK || k % kLtBK != 0)
    bad("k must be a multiple of 64 in [64, 8192] (above 8192 a partial sum "
        "may not be exact in fp32), got " +
        std::to_string(k));
}

inline std::vector<uint16_t> lt_generate(uint64_t seed, int which, int rows,
                                         int k) {
  std::vector<uint16_t> out((size_t)rows * k);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < k; ++c)
      out[(size_t)r * k + c] = lt_bf16_bits(lt_half_units(seed, which, r, c));
  return out;
}

struct LtChecksum {
  bool ok = true;
  bool is_row = false;   // what `index` counts when !ok
  long long index = -1;  // the lowest offending row, else the lowest column
};

// Row sums and column sums of `golden` ([m][n] fp32) against A * (B * 1) and
// (1^T * A) * B, in int64 units of 2^-2, from this file's generator alone:
// O(mk + nk + mn) work. An element that is not a whole number of units makes
// its row offend.
inline LtChecksum lt_checksum(uint64_t seed, int m, int n, int k,
                              const float* golden) {
  std::vector<int8_t> a((size_t)m * k), b((size_t)n * k);
  std::vector<long long> asum(k, 0), bsum(k, 0);
  for (int i = 0; i < m; ++i)
    for (int c = 0; c < k; ++c) {
      int h = lt_half_units(seed, kLtA, i, c);
      a[(size_t)i * k + c] = (int8_t)h;
      asum[c] += h;
    }
  for (int j = 0; j < n; ++j)
    for (int c = 0; c < k; ++c) {
      int h = lt_half_units(seed, kLtB, j, c);
      b[(size_t)j * k + c] = (int8_t)h;
      bsum[c] += h;
    }
  std::vector<long long> col_got(n, 0);
  LtChecksum res;
  for (int i = 0; i < m; ++i) {
    long long want = 0, got = 0;
    for (int c = 0; c < k; ++c) want += a[(size_t)i * k + c] * bsum[c];
    bool whole = true;
    for (int j = 0; j < n; ++j) {
      float q = golden[(size_t)i * n + j] * 4.0f;
      // |q| <= 2^23 for a correct product; anything else offends
      if (!(q >= -16777216.0f && q <= 16777216.0f) ||
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
