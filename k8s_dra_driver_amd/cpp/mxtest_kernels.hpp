// MX load self-test of _hiphealth: a tiled GEMM on the block-scaled MFMA
// (v_mfma_scale_f32_16x16x128_f8f6f4) with OCP e4m3 (mxfp8) or e2m1 (mxfp4)
// elements and E8M0 scales, on exact data, run for a time budget with every
// element of every iteration compared bit for bit with an answer computed
// without MFMA. Included by hiphealth.hip inside its anonymous namespace,
// after loadtest_kernels.hpp (c_verify, LoadReport, LoadOutcome, LoadBuffers,
// run_load_loop, load_dict and everything that header names).
//
//   mx_selftest()        - production path: generate, golden product, host
//                          checksum of the golden product, then
//                          mx_gemm -> c_verify until the time is up
//   mx_gemm_probe()      - test hook: the same kernels between guards on the
//                          caller's operands, scales, expectation and flips
//   mx_operands_probe()  - test hook: the generated operands and scales
//   mx_mfma_probe()      - test hook: one scaled MFMA on one wave from
//                          operands in matrix form; pins the lane map
//
// Operand lane map of the instruction, as measured through mx_mfma_probe
// (profiles/mx_selftest.md) and pinned by its tests. With r = l & 15 and
// q = l >> 4, lane l holds of row r of A
//   e2m1: k = 32 q + j, j = 0..31, in its low 4 VGPRs (the upper four are
//         ignored), ascending from the low nibble of the first;
//   e4m3: k = 16 q + j, j = 0..15, in VGPRs 0-3 and k = 64 + 16 q + j in
//         VGPRs 4-7, ascending from the low byte: a lane's 32 elements lie
//         in two k-blocks, not one.
// B^T likewise with the column on r. For both formats the scale of row r
// and k-block b (k = 32 b .. 32 b + 31) is read from lane 16 b + r, from the
// byte of the scale VGPR that op_sel names. C/D is col = l & 15,
// row = 4 * (l >> 4) + register.

#pragma once

#include <functional>

#include "mxtest_core.hpp"

typedef int mx_i32x8 __attribute__((ext_vector_type(8)));

constexpr int kMxThreads = 256;
// cbsz / blgp of the scaled MFMA: the element format of A / B
constexpr int kMxFmtE4m3 = 0;
constexpr int kMxFmtE2m1 = 4;

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// Packed elements and scale bytes of A ([m] rows) and B^T ([n] rows). One
// thread per byte of output, so an e2m1 byte's two nibbles have one writer.
__global__ void __launch_bounds__(256) mx_operands(
    unsigned char* __restrict__ a, unsigned char* __restrict__ as,
    unsigned char* __restrict__ bt, unsigned char* __restrict__ bs, int format,
    int m, int n, int k, u64 seed) {
  const size_t rb = mx_row_bytes(format, (size_t)k);
  const size_t kb = (size_t)k / kMxBlock;
  const size_t ne = ((size_t)m + n) * rb, total = ne + ((size_t)m + n) * kb;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    if (i < ne) {
      bool is_b = i >= (size_t)m * rb;
      size_t e = is_b ? i - (size_t)m * rb : i;
      size_t row = e / rb, c = e % rb;
      int which = is_b ? kLtB : kLtA;
      unsigned char v;
      if (format == kMxFp4)
        v = (unsigned char)(mx_element_code(seed, format, which, row, 2 * c) |
                            (mx_element_code(seed, format, which, row,
                                             2 * c + 1)
                             << 4));
      else
        v = mx_element_code(seed, format, which, row, c);
      (is_b ? bt : a)[e] = v;
    } else {
      size_t s = i - ne;
      bool is_b = s >= (size_t)m * kb;
      size_t e = is_b ? s - (size_t)m * kb : s;
      (is_b ? bs : as)[e] = mx_scale_byte(seed, format, is_b ? kLtB : kLtA,
                                          e / kb, e % kb);
    }
  }
}

// The golden path: one thread per element of C. Every element is decoded in
// plain C++, multiplied by its power-of-two scale (exact: the product of a
// finite element and a scale in this test's range is a normal fp32 number
// with the element's significand) and accumulated with a k-ordered fmaf
// chain on the vector ALUs. No LDS, no MFMA, no tiling shared with mx_gemm.
template <int kFormat>
__global__ void __launch_bounds__(256) mx_gemm_ref(
    const unsigned char* __restrict__ a, const unsigned char* __restrict__ as,
    const unsigned char* __restrict__ bt,
    const unsigned char* __restrict__ bs, float* __restrict__ c, int m, int n,
    int k) {
  int col = blockIdx.x * 16 + (threadIdx.x & 15);
  int row = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (row >= m || col >= n) return;
  const size_t rb = mx_row_bytes(kFormat, (size_t)k);
  const int kb = k / kMxBlock;
  const unsigned char* pa = a + (size_t)row * rb;
  const unsigned char* pb = bt + (size_t)col * rb;
  const unsigned char* sa = as + (size_t)row * kb;
  const unsigned char* sb = bs + (size_t)col * kb;
  float s = 0.f;
  for (int blk = 0; blk < kb; ++blk) {
    float fa = mx_e8m0_to_float(sa[blk]), fb = mx_e8m0_to_float(sb[blk]);
    for (int j = 0; j < kMxBlock; ++j) {
      int x = blk * kMxBlock + j;
      float va, vb;
      if constexpr (kFormat == kMxFp4) {
        va = mx_e2m1_to_float((pa[x >> 1] >> (4 * (x & 1))) & 15);
        vb = mx_e2m1_to_float((pb[x >> 1] >> (4 * (x & 1))) & 15);
      } else {
        va = mx_e4m3_to_float(pa[x]);
        vb = mx_e4m3_to_float(pb[x]);
      }
      s = fmaf(va * fa, vb * fb, s);
    }
  }
  c[(size_t)row * n + col] = s;
}

// Byte offset of 16-byte chunk `c16` of row `row` in an operand's LDS image
// of one K-step: [128] rows of kRowBytes = 128 (e4m3) or 64 (e2m1) bytes.
//
// A lane's fragment is chunk q of row r (q = lane >> 4, r = lane & 15) and,
// for e4m3, chunk 4 + q as well, one ds_read_b128 each. That instruction
// serves lanes {0-3, 12-15, 20-27} in one cycle (and three groups like it):
// eight rows at chunk c and the other eight at chunk c ^ 1.
//
// e4m3: rows are 128 bytes, two to a 256-byte bank row, so unswizzled the
// eight rows at one chunk share two 16-byte slots: an 8-way conflict. As in
// lt_lds_off the chunk is XORed with the row's low three bits: the four even
// rows of each half then take four different slots of one parity, the half
// at chunk c ^ 1 the other parity, and the odd rows the upper half of the
// bank row: 16 lanes, 16 different slots.
//
// e2m1: rows are 64 bytes, four to a bank row, so the two rows of a half
// that share row & 3 meet in one quarter of the bank row. The chunk is
// XORed with v = row >> 2, and with 2 more where v is odd, which sends the
// four rows of a quarter (two at chunk c, two at c ^ 1) to its four slots.
template <int kFormat>
__device__ inline int mx_lds_off(int row, int c16) {
  if constexpr (kFormat == kMxFp4) {
    int v = (row >> 2) & 3;
    return row * 64 + ((c16 ^ v ^ ((v & 1) << 1)) << 4);
  } else {
    return row * 128 + ((c16 ^ (row & 7)) << 4);
  }
}

// One scaled MFMA; kCode is cbsz and blgp, kSelA / kSelB the byte of the
// scale VGPRs that applies.
template <int kCode, int kSelA, int kSelB>
__device__ inline f32x4 mx_mfma(mx_i32x8 a, mx_i32x8 b, f32x4 c, int sa,
                                int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, c, kCode, kCode, kSelA, sa, kSelB, sb);
}

// C[M][N] = A[M][K] * B, B given as B^T [N][K], both MX operands. One
// 128 x 128 tile of C per block, tiles numbered row-major as in load_gemm.
// Four waves as 2 x 2, each 64 x 64 as 4 x 4 scaled MFMAs of K = 128. A
// K-step of 128 (elements and the four scale bytes of each row) is fetched
// into registers while the step before it is computed, and written to LDS
// between two barriers.
//
// Scales: the instruction takes one VGPR per operand and a byte selector
// that is the same for every lane, and reads the scale of row r and k-block
// q from lane 16 q + r. The LDS scale image is therefore kept transposed: word
// [q][h][r] (q = k-block, h = 64-row half, r = row & 15) holds in byte i the
// scale of row 64 h + 16 i + r, so one ds_read_b32 per operand and K-step
// gives a lane the scales of all four of its 16-row sub-tiles and op_sel
// picks sub-tile i's.
template <int kFormat>
__global__ void __launch_bounds__(kMxThreads) mx_gemm(
    const unsigned char* __restrict__ a, const unsigned char* __restrict__ as,
    const unsigned char* __restrict__ bt,
    const unsigned char* __restrict__ bs, float* __restrict__ c, int m, int n,
    int k, FootRecord* __restrict__ tile_rec) {
  constexpr int kRowBytes = kFormat == kMxFp4 ? 64 : 128;  // of one K-step
  constexpr int kChunks = kRowBytes / 16;                   // per row
  constexpr int kTileBytes = kMxTile * kRowBytes;
  constexpr int kStage = kMxTile * kChunks / kMxThreads;  // chunks per thread
  constexpr int kFrag = kFormat == kMxFp4 ? 1 : 2;  // chunks per fragment
  constexpr int kCode = kFormat == kMxFp4 ? kMxFmtE2m1 : kMxFmtE4m3;
  constexpr int kScaleBytes = 4 * 2 * 16 * 4;  // one operand's scale image
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kTileBytes];
  __shared__ __attribute__((aligned(16))) unsigned char lds_s[2 * kScaleBytes];
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int tiles_n = n / kMxTile;
  const int tile = blockIdx.x;
  const size_t brow = (size_t)(tile / tiles_n) * kMxTile;
  const size_t bcol = (size_t)(tile % tiles_n) * kMxTile;
  const size_t rb = mx_row_bytes(kFormat, (size_t)k);
  const int kb = k / kMxBlock;

  // staging: chunk q = t + 256 * i of an operand's tile is row q / kChunks,
  // chunk q % kChunks: kChunks lanes fetch one row's bytes of the K-step
  const unsigned char* ga[kStage];
  const unsigned char* gb[kStage];
  int soff[kStage];
#pragma unroll
  for (int i = 0; i < kStage; ++i) {
    int q = t + kMxThreads * i;
    int row = q / kChunks, c16 = q % kChunks;
    ga[i] = a + (brow + row) * rb + c16 * 16;
    gb[i] = bt + (bcol + row) * rb + c16 * 16;
    soff[i] = mx_lds_off<kFormat>(row, c16);
  }
  // scales: thread t fetches the four bytes of row t & 127 of A (t < 128)
  // or B^T, and scatters them to the transposed image
  const int srow = t & 127;
  const unsigned char* gs =
      t < 128 ? as + (brow + srow) * kb : bs + (bcol + srow) * kb;
  const int ssoff = (t < 128 ? 0 : kScaleBytes) +
                    (((srow >> 6) * 16 + (srow & 15)) << 2) +
                    ((srow >> 4) & 3);

  u32x4 ra[kStage], rb4[kStage];
  unsigned rs;
#pragma unroll
  for (int i = 0; i < kStage; ++i) {
    ra[i] = *reinterpret_cast<const u32x4*>(ga[i]);
    rb4[i] = *reinterpret_cast<const u32x4*>(gb[i]);
  }
  rs = *reinterpret_cast<const unsigned*>(gs);

  f32x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < k; k0 += kMxBK) {
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      *reinterpret_cast<u32x4*>(lds + soff[i]) = ra[i];
      *reinterpret_cast<u32x4*>(lds + kTileBytes + soff[i]) = rb4[i];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)  // k-block q of the step: word [q][h][r]
      lds_s[ssoff + q * 128] = (unsigned char)(rs >> (8 * q));
    __syncthreads();
    if (k0 + kMxBK < k) {  // the next step's operands, all inside [.][K]
      const size_t step = (size_t)(k0 + kMxBK);
#pragma unroll
      for (int i = 0; i < kStage; ++i) {
        ra[i] = *reinterpret_cast<const u32x4*>(
            ga[i] + mx_row_bytes(kFormat, step));
        rb4[i] = *reinterpret_cast<const u32x4*>(
            gb[i] + mx_row_bytes(kFormat, step));
      }
      rs = *reinterpret_cast<const unsigned*>(gs + step / kMxBlock);
    }
    {
      mx_i32x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        u32x4 pa[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        u32x4 pb[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
        for (int h = 0; h < kFrag; ++h) {
          // e4m3: k = 16 q .. in VGPRs 0-3, k = 64 + 16 q .. in VGPRs 4-7
          pa[h] = *reinterpret_cast<const u32x4*>(
              lds + mx_lds_off<kFormat>(wr * 64 + i * 16 + fr, fq + 4 * h));
          pb[h] = *reinterpret_cast<const u32x4*>(
              lds + kTileBytes +
              mx_lds_off<kFormat>(wc * 64 + i * 16 + fr, fq + 4 * h));
        }
        fa[i] = {(int)pa[0][0], (int)pa[0][1], (int)pa[0][2], (int)pa[0][3],
                 (int)pa[1][0], (int)pa[1][1], (int)pa[1][2], (int)pa[1][3]};
        fb[i] = {(int)pb[0][0], (int)pb[0][1], (int)pb[0][2], (int)pb[0][3],
                 (int)pb[1][0], (int)pb[1][1], (int)pb[1][2], (int)pb[1][3]};
      }
      const int sca = *reinterpret_cast<const int*>(
          lds_s + (((fq * 2 + wr) * 16 + fr) << 2));
      const int scb = *reinterpret_cast<const int*>(
          lds_s + kScaleBytes + (((fq * 2 + wc) * 16 + fr) << 2));
#define MX_ROW(mi)                                                          \
  acc[mi][0] = mx_mfma<kCode, mi, 0>(fa[mi], fb[0], acc[mi][0], sca, scb);  \
  acc[mi][1] = mx_mfma<kCode, mi, 1>(fa[mi], fb[1], acc[mi][1], sca, scb);  \
  acc[mi][2] = mx_mfma<kCode, mi, 2>(fa[mi], fb[2], acc[mi][2], sca, scb);  \
  acc[mi][3] = mx_mfma<kCode, mi, 3>(fa[mi], fb[3], acc[mi][3], sca, scb);
      MX_ROW(0)
      MX_ROW(1)
      MX_ROW(2)
      MX_ROW(3)
#undef MX_ROW
    }
    __syncthreads();  // the next step's writes replace what was just read
  }

  // register j of lane l: C[4 * (l >> 4) + j][l & 15] of each 16 x 16 tile
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        c[(brow + wr * 64 + mi * 16 + fq * 4 + j) * n + bcol + wc * 64 +
          ni * 16 + fr] = acc[mi][ni][j];

  if (t == 0) {
    unsigned hw = __builtin_amdgcn_s_getreg(foot_getreg(32, 0, kRegHwId));
    unsigned xcc = __builtin_amdgcn_s_getreg(foot_getreg(4, 0, kRegXccId));
    u32x4 rec = {hw, xcc, (unsigned)tile, 0u};
    *reinterpret_cast<u32x4*>(&tile_rec[tile]) = rec;
  }
}

// Test hook only: one wave, one scaled MFMA. Lane l is handed its fragments
// (8 dwords of a and b), its two scale VGPRs and its 4 floats of c; which
// matrix element each slot holds is the binding's business.
template <int kCode>
__global__ void __launch_bounds__(64) mx_mfma_one(
    const mx_i32x8* __restrict__ a, const mx_i32x8* __restrict__ b,
    const int* __restrict__ sa, const int* __restrict__ sb,
    const f32x4* __restrict__ c, f32x4* __restrict__ d, int sel) {
  int lane = threadIdx.x;
  mx_i32x8 fa = a[lane], fb = b[lane];
  int va = sa[lane], vb = sb[lane];
  f32x4 acc = c[lane];
  switch (sel) {  // op_sel is an immediate
    case 0: acc = mx_mfma<kCode, 0, 0>(fa, fb, acc, va, vb); break;
    case 1: acc = mx_mfma<kCode, 1, 1>(fa, fb, acc, va, vb); break;
    case 2: acc = mx_mfma<kCode, 2, 2>(fa, fb, acc, va, vb); break;
    default: acc = mx_mfma<kCode, 3, 3>(fa, fb, acc, va, vb); break;
  }
  d[lane] = acc;
}

// Test hook only: one thread XORs 8-bit masks into bytes of A's element
// buffer the host has already checked to lie inside it.
__global__ void mx_u8_xor(unsigned char* __restrict__ a,
                          const u64* __restrict__ flips, int count) {
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int i = 0; i < count; ++i)
      a[flips[2 * i]] ^= (unsigned char)flips[2 * i + 1];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct MxOperands {
  const unsigned char* a;
  const unsigned char* as;
  const unsigned char* bt;
  const unsigned char* bs;
};

void launch_mx_gemm_ref(int format, const MxOperands& op, float* c, int m,
                        int n, int k) {
  auto kernel = format == kMxFp4 ? mx_gemm_ref<kMxFp4> : mx_gemm_ref<kMxFp8>;
  hipLaunchKernelGGL(kernel, dim3(n / 16, m / 16), dim3(256), 0, 0, op.a,
                     op.as, op.bt, op.bs, c, m, n, k);
  HIP_CHECK(hipGetLastError());
}

void launch_mx_gemm(int format, const MxOperands& op, float* c, int m, int n,
                    int k, FootRecord* tile_rec) {
  int tiles = (m / kMxTile) * (n / kMxTile);
  auto kernel = format == kMxFp4 ? mx_gemm<kMxFp4> : mx_gemm<kMxFp8>;
  hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kMxThreads), 0, 0, op.a, op.as,
                     op.bt, op.bs, c, m, n, k, tile_rec);
  HIP_CHECK(hipGetLastError());
}

py::dict mx_selftest(int device, const std::string& format_name,
                     double seconds, int m, int n, int k, u64 seed) {
  const int format = mx_format_from_name(format_name);
  mx_check_shape(format, m, n, k);
  if (!(seconds > 0.0) || seconds > kLtMaxSeconds)
    throw std::invalid_argument("seconds must be in (0, 600], got " +
                                std::to_string(seconds));
  probe_device(device);

  const int tiles = (m / kMxTile) * (n / kMxTile);
  const size_t c_bytes = (size_t)m * n * sizeof(float);
  const size_t rb = mx_row_bytes(format, (size_t)k), kb = (size_t)k / kMxBlock;
  DevBuf a(m * rb), as(m * kb), bt(n * rb), bs(n * kb);
  DevBuf c(c_bytes), golden(c_bytes);
  hipLaunchKernelGGL(mx_operands, dim3(1024), dim3(256), 0, 0,
                     a.as<unsigned char>(), as.as<unsigned char>(),
                     bt.as<unsigned char>(), bs.as<unsigned char>(), format, m,
                     n, k, seed);
  HIP_CHECK(hipGetLastError());
  MxOperands op = {a.as<const unsigned char>(), as.as<const unsigned char>(),
                   bt.as<const unsigned char>(),
                   bs.as<const unsigned char>()};
  auto t0 = std::chrono::steady_clock::now();
  launch_mx_gemm_ref(format, op, golden.as<float>(), m, n, k);
  HIP_CHECK(hipMemset(c.as<void>(), 0xFF, c_bytes));
  HIP_CHECK(hipDeviceSynchronize());
  LtChecksum sum;
  {
    std::vector<float> host((size_t)m * n);
    HIP_CHECK(hipMemcpy(host.data(), golden.as<void>(), c_bytes,
                        hipMemcpyDeviceToHost));
    sum = mx_checksum(seed, format, m, n, k, host.data());
  }
  double golden_s = std::chrono::duration<double>(
                        std::chrono::steady_clock::now() - t0)
                        .count();

  GuardedBuf tile_rec((size_t)kLtBatch * tiles * sizeof(FootRecord));
  GuardedBuf tile_bad((size_t)kLtBatch * tiles * sizeof(unsigned));
  HIP_CHECK(hipMemset(tile_bad.payload<void>(), 0,
                      (size_t)kLtBatch * tiles * sizeof(unsigned)));
  LoadReport zero;
  std::memset(&zero, 0, sizeof zero);
  GuardedBuf report(sizeof zero, &zero);
  LoadBuffers buf = {c.as<float>(), golden.as<const float>(), &tile_rec,
                     &tile_bad,     &report,                  kLtBatch};
  LoadOutcome out;
  run_load_loop(
      buf,
      [&](FootRecord* rec) {
        launch_mx_gemm(format, op, c.as<float>(), m, n, k, rec);
      },
      m, n, k, seconds, -1, "mx_selftest", &out);
  py::dict d = load_dict(device, seed, m, n, k, out, sum);
  d["format"] = format_name;
  // generating nothing, the golden kernel and the host checksum: what the
  // child's time limit allows for, informative only
  d["golden_seconds"] = golden_s;
  return d;
}

py::tuple mx_gemm_probe(
    int device, const std::string& format_name, const py::bytes& a_bytes,
    const py::bytes& as_bytes, const py::bytes& bt_bytes,
    const py::bytes& bs_bytes, int m, int n, int k,
    const py::bytes& want_bytes, int iterations,
    const std::vector<std::pair<long long, long long>>& flips,
    const std::string& stage) {
  const int format = mx_format_from_name(format_name);
  std::string a = a_bytes, as = as_bytes, bt = bt_bytes, bs = bs_bytes,
              want = want_bytes;
  mx_check_shape(format, m, n, k);
  const size_t c_bytes = (size_t)m * n * sizeof(float);
  const size_t rb = mx_row_bytes(format, (size_t)k), kb = (size_t)k / kMxBlock;
  if (a.size() != m * rb)
    throw std::invalid_argument("a must be m rows of packed elements");
  if (bt.size() != n * rb)
    throw std::invalid_argument("b_t must be n rows of packed elements");
  if (as.size() != m * kb)
    throw std::invalid_argument("a_scales must be m x k/32 bytes");
  if (bs.size() != n * kb)
    throw std::invalid_argument("b_t_scales must be n x k/32 bytes");
  if (!want.empty() && want.size() != c_bytes)
    throw std::invalid_argument("want must be empty or m x n float32");
  probe_range("operand and result bytes",
              (long long)(a.size() + bt.size() + as.size() + bs.size() +
                          2 * c_bytes),
              0, kProbeMaxBytes);
  probe_range("iterations", iterations, 1, kLtProbeMaxIters);
  probe_range("len(flips)", (long long)flips.size(), 0, kMaxFlips);
  if (stage != "ref" && stage != "gemm" && stage != "verify")
    throw std::invalid_argument("stage must be ref, gemm or verify, got '" +
                                stage + "'");
  std::vector<u64> flat;
  flat.reserve(2 * flips.size());
  for (const auto& f : flips) {
    if (f.first < 0 || f.first >= (long long)a.size())
      throw std::invalid_argument("flip index " + std::to_string(f.first) +
                                  " outside A of " + std::to_string(a.size()) +
                                  " bytes");
    if (f.second < 0 || f.second > 0xFF)
      throw std::invalid_argument("flip mask must fit 8 bits, got " +
                                  std::to_string(f.second));
    flat.push_back((u64)f.first);
    flat.push_back((u64)f.second);
  }
  probe_device(device);

  const int tiles = (m / kMxTile) * (n / kMxTile);
  GuardedBuf da(a.size(), a.data(), kInputGuard);
  GuardedBuf das(as.size(), as.data(), kInputGuard);
  GuardedBuf dbt(bt.size(), bt.data(), kInputGuard);
  GuardedBuf dbs(bs.size(), bs.data(), kInputGuard);
  MxOperands op = {
      da.payload<const unsigned char>(), das.payload<const unsigned char>(),
      dbt.payload<const unsigned char>(), dbs.payload<const unsigned char>()};
  // written by mx_gemm_ref when the caller brings no expectation
  GuardedBuf golden(c_bytes, want.empty() ? nullptr : want.data(),
                    want.empty() ? kCanary : kInputGuard);
  GuardedBuf dc(c_bytes);
  if (want.empty())
    launch_mx_gemm_ref(format, op, golden.payload<float>(), m, n, k);
  HIP_CHECK(hipDeviceSynchronize());
  if (stage == "ref")
    return py::make_tuple(golden.download(), py::none(), py::none());

  if (!flat.empty()) {
    DevBuf dflips(flat.size() * sizeof(u64), flat.data());
    hipLaunchKernelGGL(mx_u8_xor, dim3(1), dim3(64), 0, 0,
                       da.payload<unsigned char>(), dflips.as<const u64>(),
                       (int)flips.size());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());  // dflips is freed here
  }
  GuardedBuf tile_rec((size_t)iterations * tiles * sizeof(FootRecord));
  if (stage == "gemm") {
    launch_mx_gemm(format, op, dc.payload<float>(), m, n, k,
                   tile_rec.payload<FootRecord>());
    HIP_CHECK(hipDeviceSynchronize());
    return py::make_tuple(dc.download(), py::none(), tile_rec.download());
  }

  GuardedBuf tile_bad((size_t)iterations * tiles * sizeof(unsigned));
  HIP_CHECK(hipMemset(tile_bad.payload<void>(), 0,
                      (size_t)iterations * tiles * sizeof(unsigned)));
  LoadReport zero;
  std::memset(&zero, 0, sizeof zero);
  GuardedBuf report(sizeof zero, &zero);
  LoadBuffers buf = {dc.payload<float>(), golden.payload<const float>(),
                     &tile_rec,           &tile_bad,
                     &report,             iterations};
  LoadOutcome out;
  run_load_loop(
      buf,
      [&](FootRecord* rec) {
        launch_mx_gemm(format, op, dc.payload<float>(), m, n, k, rec);
      },
      m, n, k, 0.0, iterations, "mx_gemm_probe", &out);
  // the caller's operands have no seed: nothing to check a checksum against
  py::dict d = load_dict(device, 0, m, n, k, out, LtChecksum());
  d["format"] = format_name;
  return py::make_tuple(dc.download(), d, tile_rec.download());
}

py::tuple mx_operands_probe(int device, const std::string& format_name, int m,
                            int n, int k, u64 seed) {
  const int format = mx_format_from_name(format_name);
  mx_check_shape(format, m, n, k);
  const size_t rb = mx_row_bytes(format, (size_t)k), kb = (size_t)k / kMxBlock;
  probe_range("operand bytes", (long long)(((size_t)m + n) * (rb + kb)), 0,
              kProbeMaxBytes);
  probe_device(device);
  GuardedBuf a(m * rb), as(m * kb), bt(n * rb), bs(n * kb);
  hipLaunchKernelGGL(mx_operands, dim3(1024), dim3(256), 0, 0,
                     a.payload<unsigned char>(), as.payload<unsigned char>(),
                     bt.payload<unsigned char>(), bs.payload<unsigned char>(),
                     format, m, n, k, seed);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  return py::make_tuple(a.download(), as.download(), bt.download(),
                        bs.download());
}

// a, b_t: [16][128] elements packed as the format packs them; a_scales,
// b_t_scales: [16][4] bytes; c: [16][16] float32. The lane map of this
// file's head is applied here. `opsel` names the byte of the scale VGPRs
// that carries the scales; the other three bytes hold `other_scale`.
py::bytes mx_mfma_probe(int device, const std::string& format_name,
                        const py::bytes& a_bytes, const py::bytes& as_bytes,
                        const py::bytes& bt_bytes, const py::bytes& bs_bytes,
                        const py::bytes& c_bytes, int opsel, int other_scale) {
  const int format = mx_format_from_name(format_name);
  std::string a = a_bytes, as = as_bytes, bt = bt_bytes, bs = bs_bytes,
              c = c_bytes;
  const size_t rb = mx_row_bytes(format, 128);
  if (a.size() != 16 * rb || bt.size() != 16 * rb)
    throw std::invalid_argument(
        "a and b_t must be 16 rows of 128 packed elements");
  if (as.size() != 64 || bs.size() != 64)
    throw std::invalid_argument("a_scales and b_t_scales must be 16 x 4 bytes");
  if (c.size() != 256 * sizeof(float))
    throw std::invalid_argument("c must be 16 x 16 float32");
  probe_range("opsel", opsel, 0, 3);
  probe_range("other_scale", other_scale, 0, 254);
  probe_device(device);

  std::vector<int> fa(64 * 8, 0), fb(64 * 8, 0), sa(64), sb(64);
  std::vector<float> fc(64 * 4);
  for (int l = 0; l < 64; ++l) {
    int r = l & 15, q = l >> 4;
    // e2m1: 16 bytes, k = 32 q ..; e4m3: 16 bytes of k = 16 q .. and 16 of
    // k = 64 + 16 q ..
    for (int h = 0; h < (format == kMxFp4 ? 1 : 2); ++h) {
      std::memcpy(&fa[l * 8 + 4 * h], a.data() + r * rb + (q + 4 * h) * 16, 16);
      std::memcpy(&fb[l * 8 + 4 * h], bt.data() + r * rb + (q + 4 * h) * 16, 16);
    }
    unsigned fill = (unsigned)other_scale * 0x01010101u;
    unsigned keep = ~(0xFFu << (8 * opsel));
    sa[l] = (int)((fill & keep) |
                  ((unsigned)(unsigned char)as[r * 4 + q] << (8 * opsel)));
    sb[l] = (int)((fill & keep) |
                  ((unsigned)(unsigned char)bs[r * 4 + q] << (8 * opsel)));
    for (int j = 0; j < 4; ++j)
      std::memcpy(&fc[l * 4 + j], c.data() + ((4 * q + j) * 16 + r) * 4, 4);
  }
  GuardedBuf da(fa.size() * 4, fa.data(), kInputGuard);
  GuardedBuf db(fb.size() * 4, fb.data(), kInputGuard);
  GuardedBuf dsa(sa.size() * 4, sa.data(), kInputGuard);
  GuardedBuf dsb(sb.size() * 4, sb.data(), kInputGuard);
  GuardedBuf dc(fc.size() * 4, fc.data(), kInputGuard);
  GuardedBuf dd(fc.size() * 4);
  auto kernel =
      format == kMxFp4 ? mx_mfma_one<kMxFmtE2m1> : mx_mfma_one<kMxFmtE4m3>;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, 0,
                     da.payload<const mx_i32x8>(), db.payload<const mx_i32x8>(),
                     dsa.payload<const int>(), dsb.payload<const int>(),
                     dc.payload<const f32x4>(), dd.payload<f32x4>(), opsel);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  // back to matrix form, guards kept: guard + D[16][16] float32 + guard
  std::string raw = dd.download();
  std::string out = raw;
  for (int l = 0; l < 64; ++l)
    for (int j = 0; j < 4; ++j)
      std::memcpy(&out[kGuard + ((4 * (l >> 4) + j) * 16 + (l & 15)) * 4],
                  &raw[kGuard + (l * 4 + j) * 4], 4);
  return py::bytes(out);
}
