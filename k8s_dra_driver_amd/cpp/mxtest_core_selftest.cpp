// Stand-alone driver of mxtest_core.hpp: its own main, no Python, no HIP.
// Built with -fsanitize=address,undefined by
// build_native.build_mxtest_core_selftest and run directly. Exit 0 when
// every check holds; the first failed check is printed and exits 1.

#include "mxtest_core.hpp"

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

static bool shape_ok(int format, long long m, long long n, long long k) {
  try {
    mx_check_shape(format, m, n, k);
    return true;
  } catch (const std::invalid_argument&) {
    return false;
  }
}

static float element(int format, const std::vector<uint8_t>& packed,
                     const std::vector<uint8_t>& scales, int row, int x,
                     int k) {
  size_t rb = mx_row_bytes(format, (size_t)k);
  float v = format == kMxFp4
                ? mx_e2m1_to_float(
                      (packed[row * rb + x / 2] >> (4 * (x & 1))) & 15)
                : mx_e4m3_to_float(packed[row * rb + x]);
  return v * mx_e8m0_to_float(scales[(size_t)row * (k / kMxBlock) +
                                     x / kMxBlock]);
}

// C = A * B from the generated codes and scales, accumulated in fp32 in k
// order.
static std::vector<float> product(int format, uint64_t seed, int m, int n,
                                  int k) {
  std::vector<uint8_t> a = mx_generate(seed, format, kLtA, m, k);
  std::vector<uint8_t> as = mx_generate_scales(seed, format, kLtA, m, k);
  std::vector<uint8_t> bt = mx_generate(seed, format, kLtB, n, k);
  std::vector<uint8_t> bs = mx_generate_scales(seed, format, kLtB, n, k);
  std::vector<float> fa((size_t)m * k), fb((size_t)n * k);
  for (int i = 0; i < m; ++i)
    for (int x = 0; x < k; ++x)
      fa[(size_t)i * k + x] = element(format, a, as, i, x, k);
  for (int j = 0; j < n; ++j)
    for (int x = 0; x < k; ++x)
      fb[(size_t)j * k + x] = element(format, bt, bs, j, x, k);
  std::vector<float> c((size_t)m * n);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) {
      float s = 0.f;
      for (int x = 0; x < k; ++x)
        s = std::fmaf(fa[(size_t)i * k + x], fb[(size_t)j * k + x], s);
      c[(size_t)i * n + j] = s;
    }
  return c;
}

int main() {
  // e4m3fn: the OCP values
  CHECK(mx_e4m3_to_float(0x00) == 0.f && !std::signbit(mx_e4m3_to_float(0)));
  CHECK(mx_e4m3_to_float(0x80) == 0.f && std::signbit(mx_e4m3_to_float(0x80)));
  CHECK(mx_e4m3_to_float(0x01) == 0.001953125f);  // 2^-9, smallest subnormal
  CHECK(mx_e4m3_to_float(0x07) == 7 * 0.001953125f);
  CHECK(mx_e4m3_to_float(0x08) == 0.015625f);  // 2^-6, smallest normal
  CHECK(mx_e4m3_to_float(0x38) == 1.f);
  CHECK(mx_e4m3_to_float(0x3C) == 1.5f);
  CHECK(mx_e4m3_to_float(0x7E) == 448.f);
  CHECK(mx_e4m3_to_float(0xFE) == -448.f);
  CHECK(std::isnan(mx_e4m3_to_float(0x7F)));
  CHECK(std::isnan(mx_e4m3_to_float(0xFF)));
  for (int code = 0; code < 256; ++code) {
    if ((code & 0x7F) == 0x7F) continue;
    float v = mx_e4m3_to_float((uint8_t)code);
    CHECK(std::isfinite(v) && std::fabs(v) <= 448.f);
    if (code & 0x7F)  // strictly increasing in the code
      CHECK(std::fabs(v) > std::fabs(mx_e4m3_to_float((uint8_t)(code - 1))));
  }
  for (int v = -15; v <= 15; ++v)
    CHECK(mx_e4m3_to_float(mx_e4m3_from_int(v)) == (float)v);

  // e2m1
  const float e2m1[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
  for (int code = 0; code < 16; ++code) {
    float v = mx_e2m1_to_float((uint8_t)code);
    CHECK(std::fabs(v) == e2m1[code & 7]);
    CHECK(std::signbit(v) == (code >= 8));
    CHECK(mx_e2m1_half_units((uint8_t)code) == (int)(v * 2));
  }

  // E8M0
  CHECK(mx_e8m0_to_float(127) == 1.f);
  CHECK(mx_e8m0_to_float(126) == 0.5f);
  CHECK(mx_e8m0_to_float(137) == 1024.f);
  CHECK(mx_e8m0_to_float(254) == std::ldexp(1.f, 127));
  CHECK(mx_e8m0_to_float(1) == std::ldexp(1.f, -126));
  CHECK(mx_e8m0_to_float(0) == std::ldexp(1.f, -127));
  CHECK(std::isnan(mx_e8m0_to_float(255)));

  // the generator: fixed vectors that tests/mxtest_reference.py also gives
  const uint64_t seed = 0x0123456789ABCDEFull;
  {
    const int codes[2][2][8] = {
        {{202, 202, 204, 196, 192, 74, 56, 78},
         {206, 200, 192, 184, 202, 64, 72, 206}},
        {{9, 8, 15, 10, 11, 4, 4, 9}, {11, 5, 1, 14, 15, 5, 4, 3}}};
    const int scales[2][2][2] = {{{128, 128}, {126, 127}},
                                 {{126, 127}, {126, 128}}};
    const int quarter[2][2][4] = {{{32, -56, -8, -64}, {-6, 10, -12, -32}},
                                  {{-8, 4, -12, -16}, {4, -12, 32, 0}}};
    for (int f = 0; f < kMxFormats; ++f)
      for (int w = 0; w < 2; ++w) {
        for (int x = 0; x < 8; ++x)
          CHECK(mx_element_code(seed, f, w, 3, x) == codes[f][w][x]);
        for (int b = 0; b < 2; ++b)
          CHECK(mx_scale_byte(seed, f, w, 3, b) == scales[f][w][b]);
        for (int x = 0; x < 4; ++x)
          CHECK(mx_quarter_units(seed, f, w, 3, 30 + x) == quarter[f][w][x]);
      }
  }

  // the generator: ranges, every value used, quarter units agree with the
  // decoded codes and scales, packing
  for (int f = 0; f < kMxFormats; ++f) {
    const int rows = 32, k = 256;
    const int maxq = f == kMxFp4 ? kMxFp4MaxQuarter : kMxFp8MaxQuarter;
    bool code_seen[256] = {false}, scale_seen[3] = {false};
    for (int w = 0; w < 2; ++w) {
      std::vector<uint8_t> packed = mx_generate(seed, f, w, rows, k);
      std::vector<uint8_t> scales = mx_generate_scales(seed, f, w, rows, k);
      CHECK(packed.size() == (size_t)rows * mx_row_bytes(f, k));
      CHECK(scales.size() == (size_t)rows * k / kMxBlock);
      for (int r = 0; r < rows; ++r)
        for (int x = 0; x < k; ++x) {
          uint8_t code = mx_element_code(seed, f, w, r, x);
          uint8_t sb = mx_scale_byte(seed, f, w, r, x / kMxBlock);
          CHECK(sb >= 126 && sb <= 128);
          CHECK(scales[(size_t)r * (k / kMxBlock) + x / kMxBlock] == sb);
          code_seen[code] = true;
          scale_seen[sb - 126] = true;
          int q = mx_quarter_units(seed, f, w, r, x);
          CHECK(q >= -maxq && q <= maxq);
          CHECK(element(f, packed, scales, r, x, k) == (float)q * 0.25f);
          if (f == kMxFp8) {
            float v = mx_e4m3_to_float(code);
            CHECK(v == std::rint(v) && std::fabs(v) <= 8.f);
          } else {
            CHECK(code < 16);
          }
        }
    }
    CHECK(scale_seen[0] && scale_seen[1] && scale_seen[2]);
    if (f == kMxFp4)
      for (int c = 0; c < 16; ++c) CHECK(code_seen[c]);
    else
      for (int v = -8; v <= 8; ++v) CHECK(code_seen[mx_e4m3_from_int(v)]);
    int same = 0;
    for (int x = 0; x < 256; ++x)
      same += mx_element_code(seed, f, kLtA, 0, x) ==
              mx_element_code(seed, f, kLtB, 0, x);
    CHECK(same < 96);  // A and B^T are different streams
  }
  {
    int same = 0;  // scales and elements are different streams
    for (int x = 0; x < 256; ++x)
      same += lt_mix(seed + mx_key(kMxFp4, 0, kLtA, 0, x)) ==
              lt_mix(seed + mx_key(kMxFp4, 1, kLtA, 0, x));
    CHECK(same == 0);
    CHECK(mx_key(kMxFp8, 0, kLtA, 0, 0) >> 60 != 0);  // off the bf16 keys
  }

  // names
  CHECK(mx_format_from_name("mxfp8") == kMxFp8);
  CHECK(mx_format_from_name("mxfp4") == kMxFp4);
  CHECK(std::string(mx_format_name(kMxFp4)) == "mxfp4");
  try {
    mx_format_from_name("mxfp6");
    CHECK(false);
  } catch (const std::invalid_argument&) {
  }

  // shapes: validated before anything is allocated
  for (int f = 0; f < kMxFormats; ++f) {
    const int cap = mx_max_k(f);
    CHECK(shape_ok(f, 128, 128, 128));
    CHECK(shape_ok(f, 4096, 4096, 4096));
    CHECK(shape_ok(f, 128, 128, cap));
    CHECK(shape_ok(f, kLtMaxMN, 128, 128));
    CHECK(!shape_ok(f, 128, 128, cap + 128));
    CHECK(!shape_ok(f, 128, 128, 64));
    CHECK(!shape_ok(f, 128, 128, 192));
    CHECK(!shape_ok(f, 128, 128, 0));
    CHECK(!shape_ok(f, 0, 128, 128));
    CHECK(!shape_ok(f, -128, 128, 128));
    CHECK(!shape_ok(f, 192, 128, 128));
    CHECK(!shape_ok(f, 128, 64, 128));
    CHECK(!shape_ok(f, 128, kLtMaxMN + 128, 128));
    CHECK(!shape_ok(f, 1ll << 40, 128, 128));
  }
  CHECK(mx_max_k(kMxFp8) == 8192 && mx_max_k(kMxFp4) == 7168);
  CHECK(shape_ok(kMxFp8, 128, 128, 8192) && !shape_ok(kMxFp4, 128, 128, 8192));
  CHECK(!shape_ok(2, 128, 128, 128));

  // the checksum accepts the true product and names what is wrong otherwise
  for (int f = 0; f < kMxFormats; ++f) {
    const int m = 128, n = 256, k = 128;
    std::vector<float> c = product(f, seed, m, n, k);
    LtChecksum sum = mx_checksum(seed, f, m, n, k, c.data());
    CHECK(sum.ok && sum.index == -1);

    std::vector<float> wrong = c;
    wrong[(size_t)77 * n + 200] += 0.0625f;  // one unit, one element
    sum = mx_checksum(seed, f, m, n, k, wrong.data());
    CHECK(!sum.ok && sum.is_row && sum.index == 77);

    wrong = c;  // two errors that cancel in their row show in the columns
    wrong[(size_t)5 * n + 9] += 1.0f;
    wrong[(size_t)5 * n + 30] -= 1.0f;
    sum = mx_checksum(seed, f, m, n, k, wrong.data());
    CHECK(!sum.ok && !sum.is_row && sum.index == 9);

    wrong = c;
    wrong[(size_t)100 * n + 1] += 0.03125f;  // not a whole number of units
    sum = mx_checksum(seed, f, m, n, k, wrong.data());
    CHECK(!sum.ok && sum.is_row && sum.index == 100);

    wrong = c;
    wrong[3] = std::nanf("");
    sum = mx_checksum(seed, f, m, n, k, wrong.data());
    CHECK(!sum.ok && sum.is_row && sum.index == 0);

    sum = mx_checksum(seed + 1, f, m, n, k, c.data());  // another seed's
    CHECK(!sum.ok);
    sum = mx_checksum(seed, 1 - f, m, n, k, c.data());  // another format's
    CHECK(!sum.ok);
  }

  std::puts("mxtest_core_selftest: ok");
  return 0;
}
