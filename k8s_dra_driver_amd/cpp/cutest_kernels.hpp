// Per-CU self-test of _hiphealth: an LDS pattern test and the MFMA
// known-answer table, reported under the name of the compute unit that ran
// them. Included by hiphealth.hip inside its anonymous namespace, after
// footprint_kernels.hpp (st_word, KatTable, make_kat_table, GuardedBuf,
// DevBuf, Events, require_guards, foot_decode, foot_getreg, probe_range,
// probe_device).
//
//   cu_selftest()        - production path: one launch over all of LDS on
//                          8 blocks per CU, aggregated per CU
//   cu_selftest_probe()  - test hook: the same kernel between guards on the
//                          caller's table, LDS size and wrong data
//
// A block of cu_test declares all 160 KiB of LDS, so no second block shares
// its CU while it runs: its four waves and its LDS belong to the CU that
// HW_REG_HW_ID names. The selftest() stage before it can say that a GPU
// computes wrong answers; this one says which CUs do.

#pragma once

#include <map>

constexpr int kCuLdsElems = 10240;  // 16-byte elements: all of a CU's LDS
constexpr int kCuLdsBytes = kCuLdsElems * 16;
static_assert(kCuLdsBytes == 163840, "160 KiB of LDS per CU on gfx950");
// Default grid of cu_selftest. An unmasked MI355X reported every CU with
// this grid (profiles/cu_selftest.md).
constexpr int kCuBlocksPerCu = 8;
constexpr int kCuThreads = 256;
constexpr int kCuWaves = kCuThreads / 64;

// One block's answer, 32 bytes, written as two 16-byte stores.
struct alignas(16) CuRecord {
  unsigned hw_id;   // HW_REG_HW_ID of the wave that holds thread 0
  unsigned xcc_id;  // HW_REG_XCC_ID, bits 3:0
  unsigned block;   // blockIdx.x
  unsigned simd_mask;  // OR of 1 << SIMD_ID over the block's four waves
  unsigned lds_mismatches;
  unsigned mfma_mismatches;
  unsigned pad[2];  // 0
};
static_assert(sizeof(CuRecord) == 32, "CuRecord is two 16-byte stores");

struct CuLdsRecord {
  unsigned block, pattern;
  u64 word, got, want;
};
struct CuMfmaRecord {
  unsigned block, wave, vector, lane, slot, got, want;
};
// Same discipline as MemReport and KatReport: an exact counter per kind,
// the first kMaxRecords records of each in the slot the atomic returned.
struct CuReport {
  u64 lds_count, mfma_count;
  CuLdsRecord lds[kMaxRecords];
  CuMfmaRecord mfma[kMaxRecords];
};

// Test hook only: XOR mask into LDS word `word` of block `block` while it
// holds pattern `pattern`. The host has checked every field.
struct CuFlip {
  unsigned block, pattern;
  u64 word, mask;
};

// One pattern over the first n16 elements of LDS. Thread t fills elements
// t, t+256, ... and verifies 255-t, 511-t, ...: element i is written by
// thread i % 256 and read by thread 255 - i % 256, which is another lane
// (63 - l) of another wave (3 - w). Returns this thread's mismatches.
template <int P>
__device__ inline unsigned cu_lds_pass(u64x2* lds, int n16, u64 seed,
                                       CuReport* __restrict__ report,
                                       const CuFlip* __restrict__ flips,
                                       int nflips) {
  const int t = threadIdx.x;
  for (int i = t; i < n16; i += kCuThreads) {
    u64x2 v = {st_word<P>(2 * (u64)i, seed), st_word<P>(2 * (u64)i + 1, seed)};
    lds[i] = v;
  }
  __syncthreads();
  if (t == 0) {
    for (int k = 0; k < nflips; ++k) {
      CuFlip f = flips[k];
      if (f.block != blockIdx.x || f.pattern != (unsigned)P) continue;
      u64x2 v = lds[f.word >> 1];  // word < 2 * n16, checked by the host
      if (f.word & 1)
        v.y ^= f.mask;
      else
        v.x ^= f.mask;
      lds[f.word >> 1] = v;
    }
  }
  __syncthreads();
  unsigned bad = 0;
  for (int base = 0; base < n16; base += kCuThreads) {
    int i = base + (kCuThreads - 1) - t;
    if (i >= n16) continue;
    u64x2 v = lds[i];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      u64 want = st_word<P>(2 * (u64)i + k, seed);
      if (v[k] != want) {
        ++bad;
        u64 slot = atomicAdd(&report->lds_count, 1ull);
        if (slot < (u64)kMaxRecords) {
          CuLdsRecord rec = {blockIdx.x, (unsigned)P, 2 * (u64)i + k, v[k],
                             want};
          report->lds[slot] = rec;
        }
      }
    }
  }
  __syncthreads();  // the next pattern's fill overwrites what was verified
  return bad;
}

__global__ void __launch_bounds__(kCuThreads) cu_test(
    const bf16x8* __restrict__ a_tab, const bf16x8* __restrict__ b_tab,
    const f32x4* __restrict__ c_tab, const f32x4* __restrict__ want_tab,
    u64 seed, int n16, CuRecord* __restrict__ records,
    CuReport* __restrict__ report, const CuFlip* __restrict__ flips,
    int nflips) {
  __shared__ u64x2 lds[kCuLdsElems];
  const unsigned lane = threadIdx.x & 63;
  const unsigned wave = threadIdx.x >> 6;

  // a. LDS, four patterns; block b's words are those of seed + b
  const u64 block_seed = seed + blockIdx.x;
  unsigned lds_bad = 0;
  lds_bad += cu_lds_pass<kPatAddr>(lds, n16, block_seed, report, flips, nflips);
  lds_bad +=
      cu_lds_pass<kPatAddrInv>(lds, n16, block_seed, report, flips, nflips);
  lds_bad += cu_lds_pass<kPatHash>(lds, n16, block_seed, report, flips, nflips);
  lds_bad +=
      cu_lds_pass<kPatHashInv>(lds, n16, block_seed, report, flips, nflips);

  // b. every wave takes the whole known-answer table
  unsigned mfma_bad = 0;
  for (int v = 0; v < kKatVectors; ++v) {
    unsigned idx = v * 64 + lane;
    bf16x8 fa = a_tab[idx], fb = b_tab[idx];
    f32x4 acc = c_tab[idx];
#pragma unroll
    for (int i = 0; i < kKatChain; ++i)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc, 0, 0, 0);
    f32x4 want = want_tab[idx];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned got_bits = __float_as_uint(acc[r]);
      unsigned want_bits = __float_as_uint(want[r]);
      if (got_bits != want_bits) {
        ++mfma_bad;
        u64 slot = atomicAdd(&report->mfma_count, 1ull);
        if (slot < (u64)kMaxRecords) {
          CuMfmaRecord rec = {blockIdx.x, wave,     (unsigned)v, lane,
                              (unsigned)r, got_bits, want_bits};
          report->mfma[slot] = rec;
        }
      }
    }
  }

  // c. where it ran. The last pass ended on a barrier, so the first words
  // of LDS are free to hold the block's three totals.
  unsigned hw = __builtin_amdgcn_s_getreg(foot_getreg(32, 0, kRegHwId));
  unsigned* total = reinterpret_cast<unsigned*>(lds);
  if (threadIdx.x < 3) total[threadIdx.x] = 0u;
  __syncthreads();
  if (lds_bad) atomicAdd(&total[0], lds_bad);
  if (mfma_bad) atomicAdd(&total[1], mfma_bad);
  if (lane == 0) atomicOr(&total[2], 1u << ((hw >> 4) & 0x3u));
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned xcc = __builtin_amdgcn_s_getreg(foot_getreg(4, 0, kRegXccId));
    u32x4 lo = {hw, xcc, blockIdx.x, total[2]};
    u32x4 hi = {total[0], total[1], 0u, 0u};
    u32x4* out = reinterpret_cast<u32x4*>(&records[blockIdx.x]);
    out[0] = lo;
    out[1] = hi;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct CuRun {
  int device, blocks, n16, multi_processor_count;
  u64 seed;
  double kernel_ms;
};

// The per-block records and the shared report as the dict both entry points
// return. Coverage and SIMD figures are reported, never judged: under an
// HSA_CU_MASK an incomplete footprint is the expected result.
py::dict aggregate(const CuRun& run, const std::vector<CuRecord>& records,
                   const CuReport& report) {
  struct PerCu {
    int blocks = 0;
    unsigned simd_mask = 0;
    u64 lds = 0, mfma = 0;
  };
  std::map<CuKey, PerCu> per_cu;
  for (int b = 0; b < run.blocks; ++b) {
    const CuRecord& r = records[b];
    if (r.block != (unsigned)b || r.pad[0] != 0u || r.pad[1] != 0u)
      throw std::runtime_error("cu_selftest: block " + std::to_string(b) +
                               " left no record");
    PerCu& c = per_cu[foot_decode(r.hw_id, r.xcc_id)];
    ++c.blocks;
    c.simd_mask |= r.simd_mask;
    c.lds += r.lds_mismatches;
    c.mfma += r.mfma_mismatches;
  }
  std::map<unsigned, int> xcc_count;
  int lo = run.blocks, hi = 0, simds = 4;
  py::list bad_cus;
  for (const auto& kv : per_cu) {  // std::map iterates in sorted order
    const CuKey& k = kv.first;
    const PerCu& c = kv.second;
    ++xcc_count[k.xcc];
    lo = std::min(lo, c.blocks);
    hi = std::max(hi, c.blocks);
    simds = std::min(simds, __builtin_popcount(c.simd_mask));
    if (c.lds || c.mfma) {
      py::dict bad;
      bad["xcc"] = k.xcc;
      bad["se"] = k.se;
      bad["sh"] = k.sh;
      bad["cu"] = k.cu;
      bad["blocks"] = c.blocks;
      bad["lds_mismatches"] = c.lds;
      bad["mfma_mismatches"] = c.mfma;
      bad_cus.append(bad);
    }
  }
  py::dict per_xcc;
  for (const auto& kv : xcc_count) per_xcc[py::int_(kv.first)] = kv.second;

  py::list lds_records, mfma_records;
  u64 m = std::min<u64>(report.lds_count, kMaxRecords);
  for (u64 i = 0; i < m; ++i) {
    const CuLdsRecord& r = report.lds[i];
    lds_records.append(py::make_tuple(r.block, kPatternNames[r.pattern & 3u],
                                      r.word, r.got, r.want));
  }
  m = std::min<u64>(report.mfma_count, kMaxRecords);
  for (u64 i = 0; i < m; ++i) {
    const CuMfmaRecord& r = report.mfma[i];
    mfma_records.append(py::make_tuple(r.block, r.wave, r.vector, r.lane,
                                       r.slot, r.got, r.want));
  }
  py::dict lds, mfma;
  lds["checked_words"] = (size_t)run.blocks * 4 * 2 * (size_t)run.n16;
  lds["mismatches"] = report.lds_count;
  lds["records"] = lds_records;
  mfma["checked"] = (size_t)run.blocks * kCuWaves * kKatVectors * 64 * 4;
  mfma["mismatches"] = report.mfma_count;
  mfma["records"] = mfma_records;

  py::dict d;
  d["ok"] = report.lds_count == 0 && report.mfma_count == 0;
  d["device"] = run.device;
  d["seed"] = run.seed;
  d["blocks"] = run.blocks;
  d["lds_bytes"] = (size_t)run.n16 * 16;
  d["multi_processor_count"] = run.multi_processor_count;
  d["covered"] = per_cu.size();
  d["per_xcc"] = per_xcc;
  d["blocks_per_cu_min"] = lo;
  d["blocks_per_cu_max"] = hi;
  d["simds_per_cu_min"] = simds;
  d["lds"] = lds;
  d["mfma"] = mfma;
  d["bad_cus"] = bad_cus;
  d["kernel_ms"] = run.kernel_ms;
  return d;
}

// One timed launch of cu_test; the records and the report come back to the
// host, `raw` (when asked for) with the records' guards.
py::dict run_cu_test(CuRun run, const bf16x8* a, const bf16x8* b,
                     const f32x4* c, const f32x4* want,
                     const CuFlip* flips, int nflips, const char* what,
                     py::bytes* raw) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, run.device));
  run.multi_processor_count = prop.multiProcessorCount;

  GuardedBuf records((size_t)run.blocks * sizeof(CuRecord));
  CuReport host;
  std::memset(&host, 0, sizeof host);
  GuardedBuf report(sizeof host, &host);
  Events ev(2);
  HIP_CHECK(hipEventRecord(ev[0]));
  hipLaunchKernelGGL(cu_test, dim3(run.blocks), dim3(kCuThreads), 0, 0, a, b,
                     c, want, run.seed, run.n16, records.payload<CuRecord>(),
                     report.payload<CuReport>(), flips, nflips);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(ev[1]));
  HIP_CHECK(hipEventSynchronize(ev[1]));
  run.kernel_ms = ev.ms(0, 1);
  require_guards(records, what);
  require_guards(report, what);
  std::vector<CuRecord> rec(run.blocks);
  HIP_CHECK(hipMemcpy(rec.data(), records.payload<void>(),
                      rec.size() * sizeof(CuRecord), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(&host, report.payload<void>(), sizeof host,
                      hipMemcpyDeviceToHost));
  if (raw) *raw = records.download();
  return aggregate(run, rec, host);
}

py::dict cu_selftest(int device, u64 seed, int blocks) {
  probe_range("blocks", blocks, 0, kProbeMaxBlocks);
  probe_device(device);
  if (blocks == 0) {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    blocks = std::min(kCuBlocksPerCu * prop.multiProcessorCount,
                      kProbeMaxBlocks);
  }
  KatTable t = make_kat_table(seed);
  DevBuf a(kKatFragBytes, t.a.data()), b(kKatFragBytes, t.b.data());
  DevBuf c(kKatFragBytes, t.c.data()), want(kKatFragBytes, t.want.data());
  CuRun run = {device, blocks, kCuLdsElems, 0, seed, 0.0};
  return run_cu_test(run, a.as<const bf16x8>(), b.as<const bf16x8>(),
                     c.as<const f32x4>(), want.as<const f32x4>(), nullptr, 0,
                     "cu_selftest", nullptr);
}

py::tuple cu_selftest_probe(
    int device, const py::bytes& a_bytes, const py::bytes& b_bytes,
    const py::bytes& c_bytes, const py::bytes& want_bytes, u64 seed,
    int blocks, long long lds_bytes,
    const std::vector<std::tuple<long long, std::string, long long, u64>>&
        flips) {
  std::string a = a_bytes, b = b_bytes, c = c_bytes, want = want_bytes;
  if (a.size() != kKatFragBytes)
    throw std::invalid_argument("a_tab must be 16x64x8 uint16 (16384 bytes)");
  if (b.size() != kKatFragBytes)
    throw std::invalid_argument("b_tab must be 16x64x8 uint16 (16384 bytes)");
  if (c.size() != kKatFragBytes)
    throw std::invalid_argument("c_tab must be 16x64x4 float32 (16384 bytes)");
  if (want.size() != kKatFragBytes)
    throw std::invalid_argument(
        "want_tab must be 16x64x4 float32 (16384 bytes)");
  probe_range("blocks", blocks, 1, kProbeMaxBlocks);
  probe_range("lds_bytes", lds_bytes, 16, kCuLdsBytes);
  if (lds_bytes % 16 != 0)
    throw std::invalid_argument("lds_bytes must be a multiple of 16");
  probe_range("len(flips)", (long long)flips.size(), 0, kMaxFlips);
  int n16 = (int)(lds_bytes / 16);
  std::vector<CuFlip> flat;
  flat.reserve(flips.size());
  for (const auto& f : flips) {
    long long block = std::get<0>(f), word = std::get<2>(f);
    int p = pattern_from_name(std::get<1>(f));
    if (block < 0 || block >= blocks)
      throw std::invalid_argument("flip block " + std::to_string(block) +
                                  " outside the grid of " +
                                  std::to_string(blocks) + " blocks");
    if (word < 0 || word >= 2 * (long long)n16)
      throw std::invalid_argument(
          "flip word index " + std::to_string(word) +
          " outside the region of " + std::to_string(2 * n16) + " words");
    flat.push_back({(unsigned)block, (unsigned)p, (u64)word, std::get<3>(f)});
  }
  probe_device(device);

  GuardedBuf da(a.size(), a.data(), kInputGuard);
  GuardedBuf db(b.size(), b.data(), kInputGuard);
  GuardedBuf dc(c.size(), c.data(), kInputGuard);
  GuardedBuf dw(want.size(), want.data(), kInputGuard);
  GuardedBuf df(flat.size() * sizeof(CuFlip), flat.data(), kInputGuard);
  CuRun run = {device, blocks, n16, 0, seed, 0.0};
  py::bytes raw;
  py::dict d = run_cu_test(run, da.payload<const bf16x8>(),
                           db.payload<const bf16x8>(),
                           dc.payload<const f32x4>(),
                           dw.payload<const f32x4>(),
                           df.payload<const CuFlip>(), (int)flat.size(),
                           "cu_selftest_probe", &raw);
  return py::make_tuple(raw, d);
}
