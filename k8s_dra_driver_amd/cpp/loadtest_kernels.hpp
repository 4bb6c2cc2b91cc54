// Load self-test of _hiphealth: a tiled bf16 GEMM on exact data, run for a
// time budget with every element of every iteration compared bit for bit
// with an independently computed answer. Included by hiphealth.hip inside
// its anonymous namespace, after cutest_kernels.hpp (GuardedBuf, DevBuf,
// Events, require_guards, FootRecord, CuKey, foot_decode, foot_getreg,
// probe_range, probe_device, bf16x8, f32x4, u32x4, u64, kMaxRecords,
// kMaxFlips).
//
//   load_selftest()        - production path: generate, golden product,
//                            host checksum of the golden product, then
//                            load_gemm -> c_verify until the time is up
//   load_gemm_probe()      - test hook: the same kernels between guards on
//                            the caller's operands, expectation and flips
//   load_operands_probe()  - test hook: the generated operands
//
// The two stages before it test a quiet chip. Here every CU streams operands
// from HBM, stages them through LDS and issues MFMAs back to back, and a
// wrong element is named by iteration, element, tile and CU.

#pragma once

#include <chrono>
#include <functional>
#include <set>

#include "loadtest_core.hpp"

constexpr int kLtThreads = 256;
constexpr int kLtTileBytes = kLtTile * kLtBK * 2;  // one operand's LDS image
constexpr unsigned kLtPoison = 0xFFFFFFFFu;
// load_gemm -> c_verify pairs between two synchronisations: long enough that
// the chip does not idle between batches for a noticeable share of the time,
// short enough that a bad GPU is stopped within milliseconds.
constexpr int kLtBatch = 8;
constexpr int kLtProbeMaxIters = 64;
constexpr double kLtMaxSeconds = 600.0;

typedef unsigned short lt_bf16;

struct LoadRecord {
  unsigned iteration, row, col, got, want, hw_id, xcc_id;
};
struct LoadReport {
  u64 count;
  LoadRecord rec[kMaxRecords];
};

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) load_operands(
    lt_bf16* __restrict__ a, lt_bf16* __restrict__ bt, int m, int n, int k,
    u64 seed) {
  size_t na = (size_t)m * k, total = na + (size_t)n * k;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    bool is_b = i >= na;
    size_t e = is_b ? i - na : i;
    lt_bf16 bits = lt_bf16_bits(
        lt_half_units(seed, is_b ? kLtB : kLtA, e / k, e % k));
    (is_b ? bt : a)[e] = bits;
  }
}

__device__ inline float lt_bf16_to_f32(lt_bf16 bits) {
  return __uint_as_float((unsigned)bits << 16);
}

// The golden path: one thread per element of C, a k-ordered fmaf chain on
// the vector ALUs. No LDS, no MFMA, no tiling shared with load_gemm.
__global__ void __launch_bounds__(256) gemm_ref(
    const lt_bf16* __restrict__ a, const lt_bf16* __restrict__ bt,
    float* __restrict__ c, int m, int n, int k) {
  int col = blockIdx.x * 16 + (threadIdx.x & 15);
  int row = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (row >= m || col >= n) return;
  const bf16x8* pa = reinterpret_cast<const bf16x8*>(a + (size_t)row * k);
  const bf16x8* pb = reinterpret_cast<const bf16x8*>(bt + (size_t)col * k);
  float s = 0.f;
  for (int x = 0; x < k / 8; ++x) {  // 8 consecutive k are one 16-byte load
    bf16x8 va = pa[x], vb = pb[x];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      s = fmaf(lt_bf16_to_f32((lt_bf16)va[j]), lt_bf16_to_f32((lt_bf16)vb[j]),
               s);
  }
  c[(size_t)row * n + col] = s;
}

// Byte offset of 16-byte chunk `c16` (8 consecutive k) of row `row` in an
// operand's [128][64] bf16 LDS image. Rows are 128 bytes, two to a 256-byte
// bank row, and a wave's fragment read has 16 rows on one chunk: unswizzled
// that is an 8-way conflict for ds_read_b128. XORing the chunk with the
// row's low three bits puts the 16 lanes of each of that instruction's lane
// groups (8 rows at chunk c, 8 at chunk c ^ 1) on 16 different slots.
__device__ inline int lt_lds_off(int row, int c16) {
  return row * (kLtBK * 2) + ((c16 ^ (row & 7)) << 4);
}

// C[M][N] = A[M][K] * B, B given as B^T [N][K]. One 128x128 tile of C per
// block, tiles numbered row-major: tile t is rows 128 * (t / (N / 128)) and
// columns 128 * (t % (N / 128)). Four waves as 2 x 2, each 64 x 64 as 4 x 4
// MFMA tiles. A K-step of 64 is fetched into registers while the step
// before it is computed, and written to LDS between two barriers.
__global__ void __launch_bounds__(kLtThreads) load_gemm(
    const lt_bf16* __restrict__ a, const lt_bf16* __restrict__ bt,
    float* __restrict__ c, int m, int n, int k,
    FootRecord* __restrict__ tile_rec) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kLtTileBytes];
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int tiles_n = n / kLtTile;
  const int tile = blockIdx.x;
  const size_t brow = (size_t)(tile / tiles_n) * kLtTile;
  const size_t bcol = (size_t)(tile % tiles_n) * kLtTile;

  // staging: chunk q = t + 256 * i of the 1024 in an operand's tile is
  // row q >> 3, chunk q & 7: eight lanes fetch one row's 128 bytes
  const lt_bf16* ga[4];
  const lt_bf16* gb[4];
  int soff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int q = t + kLtThreads * i;
    int row = q >> 3, c16 = q & 7;
    ga[i] = a + (brow + row) * k + c16 * 8;
    gb[i] = bt + (bcol + row) * k + c16 * 8;
    soff[i] = lt_lds_off(row, c16);
  }
  u32x4 ra[4], rb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = *reinterpret_cast<const u32x4*>(ga[i]);
    rb[i] = *reinterpret_cast<const u32x4*>(gb[i]);
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < k; k0 += kLtBK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4*>(lds + soff[i]) = ra[i];
      *reinterpret_cast<u32x4*>(lds + kLtTileBytes + soff[i]) = rb[i];
    }
    __syncthreads();
    if (k0 + kLtBK < k) {  // the next step's operands, all inside [.][K]
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = *reinterpret_cast<const u32x4*>(ga[i] + k0 + kLtBK);
        rb[i] = *reinterpret_cast<const u32x4*>(gb[i] + k0 + kLtBK);
      }
    }
#pragma unroll
    for (int kk = 0; kk < kLtBK / 32; ++kk) {
      // lane l: A[row l & 15][k = 8 * (l >> 4) + j], B[k][col l & 15]
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fa[i] = *reinterpret_cast<const bf16x8*>(
            lds + lt_lds_off(wr * 64 + i * 16 + fr, kk * 4 + fq));
        fb[i] = *reinterpret_cast<const bf16x8*>(
            lds + kLtTileBytes +
            lt_lds_off(wc * 64 + i * 16 + fr, kk * 4 + fq));
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
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

// Compares C with the golden copy, four elements per lane per trip, and
// leaves poison behind: an iteration that does not write a tile finds
// 0xFFFFFFFF there and not the last iteration's answer. tile_rec holds the
// records of the load_gemm launched just before on the same stream.
__global__ void __launch_bounds__(256) c_verify(
    u32x4* __restrict__ c, const u32x4* __restrict__ golden, int m, int n,
    unsigned iteration, const FootRecord* __restrict__ tile_rec,
    unsigned* __restrict__ tile_bad, LoadReport* __restrict__ report) {
  size_t n4 = (size_t)m * n / 4;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  const u32x4 poison = {kLtPoison, kLtPoison, kLtPoison, kLtPoison};
  for (; i < n4; i += stride) {
    u32x4 got = c[i];
    u32x4 want = golden[i];
    c[i] = poison;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (got[r] == want[r]) continue;
      size_t e = 4 * i + r;
      unsigned row = (unsigned)(e / n), col = (unsigned)(e % n);
      unsigned tile = (row / kLtTile) * (n / kLtTile) + col / kLtTile;
      u64 slot = atomicAdd(&report->count, 1ull);
      if (slot < (u64)kMaxRecords) {
        LoadRecord rec = {iteration, row,    col,
                          got[r],    want[r], tile_rec[tile].hw_id,
                          tile_rec[tile].xcc_id};
        report->rec[slot] = rec;
      }
      atomicAdd(&tile_bad[tile], 1u);
    }
  }
}

// Test hook only: one thread XORs 16-bit masks into elements of A the host
// has already checked to lie inside it. flips holds (index, mask) pairs.
__global__ void bf16_xor(lt_bf16* __restrict__ a,
                         const u64* __restrict__ flips, int count) {
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int i = 0; i < count; ++i)
      a[flips[2 * i]] ^= (lt_bf16)flips[2 * i + 1];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
void launch_load_operands(lt_bf16* a, lt_bf16* bt, int m, int n, int k,
                          u64 seed) {
  hipLaunchKernelGGL(load_operands, dim3(1024), dim3(256), 0, 0, a, bt, m, n,
                     k, seed);
  HIP_CHECK(hipGetLastError());
}

void launch_gemm_ref(const lt_bf16* a, const lt_bf16* bt, float* c, int m,
                     int n, int k) {
  hipLaunchKernelGGL(gemm_ref, dim3(n / 16, m / 16), dim3(256), 0, 0, a, bt,
                     c, m, n, k);
  HIP_CHECK(hipGetLastError());
}

void launch_load_gemm(const lt_bf16* a, const lt_bf16* bt, float* c, int m,
                      int n, int k, FootRecord* tile_rec) {
  int tiles = (m / kLtTile) * (n / kLtTile);
  hipLaunchKernelGGL(load_gemm, dim3(tiles), dim3(kLtThreads), 0, 0, a, bt, c,
                     m, n, k, tile_rec);
  HIP_CHECK(hipGetLastError());
}

struct LoadBuffers {
  float* c;
  const float* golden;
  // `slots` iterations' worth of per-tile records and mismatch counters;
  // iteration i uses slot i % slots
  GuardedBuf* tile_rec;
  GuardedBuf* tile_bad;
  GuardedBuf* report;
  int slots;
};

struct LoadOutcome {
  u64 iterations = 0;
  LoadReport report;
  std::map<int, u64> bad_tiles;
  std::map<CuKey, u64> bad_cus;
  std::set<CuKey> cus;
  double gemm_loop_ms = 0;
  double seconds = 0;
};

// Launches the GEMM under test once: it writes all of buf.c and one record
// per tile to the slot it is handed.
typedef std::function<void(FootRecord*)> LoadGemm;

// gemm -> c_verify in batches of kLtBatch, one synchronisation per batch,
// until `seconds` of wall time have passed (max_iters < 0) or max_iters
// iterations ran; always at least one batch, and none after a batch that
// recorded a mismatch.
void run_load_loop(const LoadBuffers& buf, const LoadGemm& gemm, int m, int n,
                   int k, double seconds, long long max_iters,
                   const char* what, LoadOutcome* out) {
  const int tiles = (m / kLtTile) * (n / kLtTile);
  const int verify_blocks =
      (int)std::min<size_t>(1024, ((size_t)m * n / 4 + 255) / 256);
  FootRecord* rec_dev = buf.tile_rec->payload<FootRecord>();
  unsigned* bad_dev = buf.tile_bad->payload<unsigned>();
  LoadReport* report_dev = buf.report->payload<LoadReport>();
  std::vector<FootRecord> rec(tiles);
  std::vector<unsigned> bad(tiles);
  std::memset(&out->report, 0, sizeof out->report);
  Events ev(2);
  auto t0 = std::chrono::steady_clock::now();
  auto elapsed = [&t0]() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() -
                                         t0)
        .count();
  };
  HIP_CHECK(hipEventRecord(ev[0]));
  for (;;) {
    long long batch = kLtBatch;
    if (max_iters >= 0)
      batch = std::min<long long>(batch, max_iters - (long long)out->iterations);
    for (long long b = 0; b < batch; ++b) {
      u64 it = out->iterations + b;
      size_t slot = (size_t)(it % buf.slots) * tiles;
      gemm(rec_dev + slot);
      hipLaunchKernelGGL(c_verify, dim3(verify_blocks), dim3(256), 0, 0,
                         reinterpret_cast<u32x4*>(buf.c),
                         reinterpret_cast<const u32x4*>(buf.golden), m, n,
                         (unsigned)it, rec_dev + slot, bad_dev + slot,
                         report_dev);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipDeviceSynchronize());
    for (long long b = 0; b < batch; ++b) {
      u64 it = out->iterations + b;
      size_t slot = (size_t)(it % buf.slots) * tiles;
      HIP_CHECK(hipMemcpy(rec.data(), rec_dev + slot,
                          tiles * sizeof(FootRecord), hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(bad.data(), bad_dev + slot,
                          tiles * sizeof(unsigned), hipMemcpyDeviceToHost));
      for (int t = 0; t < tiles; ++t) {
        if (rec[t].block != (unsigned)t || rec[t].pad != 0u)
          throw std::runtime_error(std::string(what) + ": tile " +
                                   std::to_string(t) + " of iteration " +
                                   std::to_string(it) + " left no record");
        CuKey cu = foot_decode(rec[t].hw_id, rec[t].xcc_id);
        out->cus.insert(cu);
        if (bad[t]) {
          out->bad_tiles[t] += bad[t];
          out->bad_cus[cu] += bad[t];
        }
      }
    }
    out->iterations += (u64)batch;
    HIP_CHECK(hipMemcpy(&out->report, report_dev, sizeof out->report,
                        hipMemcpyDeviceToHost));
    if (out->report.count) break;
    if (max_iters >= 0 ? (long long)out->iterations >= max_iters
                       : elapsed() >= seconds)
      break;
    if (max_iters < 0) {
      // the slots are used again: a tile that does not run must not find
      // the records of the batch before
      HIP_CHECK(hipMemset(rec_dev, 0xFF,
                          (size_t)buf.slots * tiles * sizeof(FootRecord)));
      HIP_CHECK(hipMemset(bad_dev, 0,
                          (size_t)buf.slots * tiles * sizeof(unsigned)));
    }
  }
  HIP_CHECK(hipEventRecord(ev[1]));
  HIP_CHECK(hipEventSynchronize(ev[1]));
  out->gemm_loop_ms = ev.ms(0, 1);
  out->seconds = elapsed();
  require_guards(*buf.tile_rec, what);
  require_guards(*buf.tile_bad, what);
  require_guards(*buf.report, what);
}

py::dict load_dict(int device, u64 seed, int m, int n, int k,
                   const LoadOutcome& o, const LtChecksum& sum) {
  py::list records, bad_tiles, bad_cus;
  u64 kept = std::min<u64>(o.report.count, kMaxRecords);
  for (u64 i = 0; i < kept; ++i) {
    const LoadRecord& r = o.report.rec[i];
    records.append(py::make_tuple(r.iteration, r.row, r.col, r.got, r.want));
  }
  const int tiles_n = n / kLtTile;
  for (const auto& kv : o.bad_tiles)
    bad_tiles.append(
        py::make_tuple(kv.first / tiles_n, kv.first % tiles_n, kv.second));
  for (const auto& kv : o.bad_cus) {  // std::map iterates in sorted order
    py::dict bad;
    bad["xcc"] = kv.first.xcc;
    bad["se"] = kv.first.se;
    bad["sh"] = kv.first.sh;
    bad["cu"] = kv.first.cu;
    bad["mismatches"] = kv.second;
    bad_cus.append(bad);
  }
  py::dict d;
  d["ok"] = o.report.count == 0 && sum.ok;
  d["device"] = device;
  d["seed"] = seed;
  d["m"] = m;
  d["n"] = n;
  d["k"] = k;
  d["iterations"] = o.iterations;
  d["seconds"] = o.seconds;
  d["checksum_ok"] = sum.ok;
  // "" or the first row or column of the golden copy whose sum is wrong
  d["checksum_first_bad"] =
      sum.ok ? std::string()
             : std::string(sum.is_row ? "row " : "column ") +
                   std::to_string(sum.index);
  d["mismatches"] = o.report.count;
  d["records"] = records;
  d["bad_tiles"] = bad_tiles;
  d["bad_cus"] = bad_cus;
  d["cus_seen"] = o.cus.size();
  // the whole loop, its c_verify launches included: informative only
  d["tflops"] = o.gemm_loop_ms > 0
                    ? 2.0 * m * n * k * (double)o.iterations /
                          (o.gemm_loop_ms / 1e3) / 1e12
                    : 0.0;
  return d;
}

py::dict load_selftest(int device, double seconds, int m, int n, int k,
                       u64 seed) {
  lt_check_shape(m, n, k);
  if (!(seconds > 0.0) || seconds > kLtMaxSeconds)
    throw std::invalid_argument("seconds must be in (0, 600], got " +
                                std::to_string(seconds));
  probe_device(device);

  const int tiles = (m / kLtTile) * (n / kLtTile);
  const size_t c_bytes = (size_t)m * n * sizeof(float);
  DevBuf a((size_t)m * k * 2), bt((size_t)n * k * 2);
  DevBuf c(c_bytes), golden(c_bytes);
  launch_load_operands(a.as<lt_bf16>(), bt.as<lt_bf16>(), m, n, k, seed);
  launch_gemm_ref(a.as<const lt_bf16>(), bt.as<const lt_bf16>(),
                  golden.as<float>(), m, n, k);
  HIP_CHECK(hipMemset(c.as<void>(), 0xFF, c_bytes));
  HIP_CHECK(hipDeviceSynchronize());
  LtChecksum sum;
  {
    std::vector<float> host((size_t)m * n);
    HIP_CHECK(hipMemcpy(host.data(), golden.as<void>(), c_bytes,
                        hipMemcpyDeviceToHost));
    sum = lt_checksum(seed, m, n, k, host.data());
  }

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
        launch_load_gemm(a.as<const lt_bf16>(), bt.as<const lt_bf16>(),
                         c.as<float>(), m, n, k, rec);
      },
      m, n, k, seconds, -1, "load_selftest", &out);
  return load_dict(device, seed, m, n, k, out, sum);
}

py::tuple load_gemm_probe(
    int device, const py::bytes& a_bytes, const py::bytes& bt_bytes, int m,
    int n, int k, const py::bytes& want_bytes, int iterations,
    const std::vector<std::pair<long long, long long>>& flips,
    const std::string& stage) {
  std::string a = a_bytes, bt = bt_bytes, want = want_bytes;
  lt_check_shape(m, n, k);
  const size_t c_bytes = (size_t)m * n * sizeof(float);
  if (a.size() != (size_t)m * k * 2)
    throw std::invalid_argument("a must be m x k uint16");
  if (bt.size() != (size_t)n * k * 2)
    throw std::invalid_argument("b_t must be n x k uint16");
  if (!want.empty() && want.size() != c_bytes)
    throw std::invalid_argument("want must be empty or m x n float32");
  probe_range("operand and result bytes",
              (long long)(a.size() + bt.size() + 2 * c_bytes), 0,
              kProbeMaxBytes);
  probe_range("iterations", iterations, 1, kLtProbeMaxIters);
  probe_range("len(flips)", (long long)flips.size(), 0, kMaxFlips);
  if (stage != "ref" && stage != "gemm" && stage != "verify")
    throw std::invalid_argument("stage must be ref, gemm or verify, got '" +
                                stage + "'");
  std::vector<u64> flat;
  flat.reserve(2 * flips.size());
  for (const auto& f : flips) {
    if (f.first < 0 || f.first >= (long long)m * k)
      throw std::invalid_argument("flip index " + std::to_string(f.first) +
                                  " outside A of " +
                                  std::to_string((long long)m * k) +
                                  " elements");
    if (f.second < 0 || f.second > 0xFFFF)
      throw std::invalid_argument("flip mask must fit 16 bits, got " +
                                  std::to_string(f.second));
    flat.push_back((u64)f.first);
    flat.push_back((u64)f.second);
  }
  probe_device(device);

  const int tiles = (m / kLtTile) * (n / kLtTile);
  GuardedBuf da(a.size(), a.data(), kInputGuard);
  GuardedBuf dbt(bt.size(), bt.data(), kInputGuard);
  // written by gemm_ref when the caller brings no expectation
  GuardedBuf golden(c_bytes, want.empty() ? nullptr : want.data(),
                    want.empty() ? kCanary : kInputGuard);
  GuardedBuf dc(c_bytes);
  if (want.empty())
    launch_gemm_ref(da.payload<const lt_bf16>(), dbt.payload<const lt_bf16>(),
                    golden.payload<float>(), m, n, k);
  HIP_CHECK(hipDeviceSynchronize());
  if (stage == "ref")
    return py::make_tuple(golden.download(), py::none(), py::none());

  if (!flat.empty()) {
    DevBuf dflips(flat.size() * sizeof(u64), flat.data());
    hipLaunchKernelGGL(bf16_xor, dim3(1), dim3(64), 0, 0,
                       da.payload<lt_bf16>(), dflips.as<const u64>(),
                       (int)flips.size());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());  // dflips is freed here
  }
  GuardedBuf tile_rec((size_t)iterations * tiles * sizeof(FootRecord));
  if (stage == "gemm") {
    launch_load_gemm(da.payload<const lt_bf16>(),
                     dbt.payload<const lt_bf16>(), dc.payload<float>(), m, n,
                     k, tile_rec.payload<FootRecord>());
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
        launch_load_gemm(da.payload<const lt_bf16>(),
                         dbt.payload<const lt_bf16>(), dc.payload<float>(), m,
                         n, k, rec);
      },
      m, n, k, 0.0, iterations, "load_gemm_probe", &out);
  // the caller's operands have no seed: nothing to check a checksum against
  py::dict d = load_dict(device, 0, m, n, k, out, LtChecksum());
  return py::make_tuple(dc.download(), d, tile_rec.download());
}

py::tuple load_operands_probe(int device, int m, int n, int k, u64 seed) {
  lt_check_shape(m, n, k);
  probe_range("operand bytes", ((long long)m + n) * k * 2, 0, kProbeMaxBytes);
  probe_device(device);
  GuardedBuf a((size_t)m * k * 2), bt((size_t)n * k * 2);
  launch_load_operands(a.payload<lt_bf16>(), bt.payload<lt_bf16>(), m, n, k,
                       seed);
  HIP_CHECK(hipDeviceSynchronize());
  return py::make_tuple(a.download(), bt.download());
}
