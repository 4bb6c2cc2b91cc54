// Stand-alone driver of loadtest_core.hpp: its own main, no Python, no HIP.
// Built with -fsanitize=address,undefined by
// build_native.build_loadtest_core_selftest and run directly. Exit 0 when
// every check holds; the first failed check is printed and exits 1.

#include "loadtest_core.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__,     \
                   __LINE__, #cond);                                  \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static float bf16_to_float(uint16_t bits) {
  uint32_t w = (uint32_t)bits << 16;
  float f;
  std::memcpy(&f, &w, sizeof f);
  return f;
}

static bool shape_ok(long long m, long long n, long long k) {
  try {
    lt_check_shape(m, n, k);
    return true;
  } catch (const std::invalid_argument&) {
    return false;
  }
}

// C = A * B from the generated bf16 bits, accumulated in fp32 in k order.
static std::vector<float> product(const std::vector<uint16_t>& a,
                                  const std::vector<uint16_t>& bt, int m,
                                  int n, int k) {
  std::vector<float> c((size_t)m * n);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) {
      float s = 0.f;
      for (int x = 0; x < k; ++x)
        s = std::fmaf(bf16_to_float(a[(size_t)i * k + x]),
                      bf16_to_float(bt[(size_t)j * k + x]), s);
      c[(size_t)i * n + j] = s;
    }
  return c;
}

int main() {
  CHECK(lt_mix(0) == 0xE220A8397B1DCDAFull);

  // the generator: range, exactness in bf16, every value and exponent used
  const uint64_t seed = 0x0123456789ABCDEFull;
  bool seen[65] = {false};
  for (int which = 0; which < 2; ++which)
    for (int row = 0; row < 64; ++row)
      for (int k = 0; k < 256; ++k) {
        int h = lt_half_units(seed, which, row, k);
        CHECK(h >= -32 && h <= 32);
        seen[h + 32] = true;
        CHECK(bf16_to_float(lt_bf16_bits(h)) == (float)h * 0.5f);
      }
  for (int v = -8; v <= 8; ++v)
    for (int e = 0; e <= 2; ++e) CHECK(seen[v * (1 << e) + 32]);
  CHECK(lt_half_units(seed, kLtA, 3, 5) == lt_half_units(seed, kLtA, 3, 5));
  {
    int same = 0;
    for (int k = 0; k < 256; ++k)
      same += lt_half_units(seed, kLtA, 0, k) == lt_half_units(seed, kLtB, 0, k);
    CHECK(same < 64);  // A and B^T are different streams
  }

  // shapes: validated before anything is allocated
  CHECK(shape_ok(128, 128, 64));
  CHECK(shape_ok(4096, 4096, 4096));
  CHECK(shape_ok(128, 128, kLtMaxK));
  CHECK(shape_ok(kLtMaxMN, 128, 64));
  CHECK(!shape_ok(128, 128, kLtMaxK + 64));
  CHECK(!shape_ok(128, 128, 32));
  CHECK(!shape_ok(128, 128, 96));
  CHECK(!shape_ok(0, 128, 64));
  CHECK(!shape_ok(-128, 128, 64));
  CHECK(!shape_ok(192, 128, 64));
  CHECK(!shape_ok(128, 64, 64));
  CHECK(!shape_ok(128, kLtMaxMN + 128, 64));
  CHECK(!shape_ok(1ll << 40, 128, 64));

  // the checksum accepts the true product and names what is wrong otherwise
  const int m = 128, n = 256, k = 192;
  std::vector<uint16_t> a = lt_generate(seed, kLtA, m, k);
  std::vector<uint16_t> bt = lt_generate(seed, kLtB, n, k);
  CHECK(a.size() == (size_t)m * k && bt.size() == (size_t)n * k);
  std::vector<float> c = product(a, bt, m, n, k);
  LtChecksum sum = lt_checksum(seed, m, n, k, c.data());
  CHECK(sum.ok && sum.index == -1);

  std::vector<float> wrong = c;
  wrong[(size_t)77 * n + 200] += 0.25f;  // one unit, one element
  sum = lt_checksum(seed, m, n, k, wrong.data());
  CHECK(!sum.ok && sum.is_row && sum.index == 77);

  wrong = c;  // two errors that cancel in their row show in the columns
  wrong[(size_t)5 * n + 9] += 1.0f;
  wrong[(size_t)5 * n + 30] -= 1.0f;
  sum = lt_checksum(seed, m, n, k, wrong.data());
  CHECK(!sum.ok && !sum.is_row && sum.index == 9);

  wrong = c;
  wrong[(size_t)100 * n + 1] += 0.125f;  // not a whole number of units
  sum = lt_checksum(seed, m, n, k, wrong.data());
  CHECK(!sum.ok && sum.is_row && sum.index == 100);

  wrong = c;
  wrong[3] = std::nanf("");
  sum = lt_checksum(seed, m, n, k, wrong.data());
  CHECK(!sum.ok && sum.is_row && sum.index == 0);

  sum = lt_checksum(seed + 1, m, n, k, c.data());  // another seed's product
  CHECK(!sum.ok);

  std::puts("loadtest_core_selftest: ok");
  return 0;
}
