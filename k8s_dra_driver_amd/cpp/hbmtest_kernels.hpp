// HBM march self-test of _hiphealth. Included by hiphealth.hip inside its
// anonymous namespace, after selftest_kernels.hpp (st_word, mem_xor, DevBuf,
// Events, require_guards) and the probe helpers (GuardedBuf, probe_range).
//
//   hbm_selftest()     - production path: all free memory less a reserve (or
//                        the MiB asked for) in 1 GiB chunks, marched for a
//                        time budget
//   hbm_march_probe()  - test hook: the same host loop on small guarded
//                        chunks, with wrong data injected by the caller
//
// hbmtest_core.hpp has the plan, the schedule and the aggregation. Every pass
// goes over every chunk before the next pass starts, so a word is read back
// only after the whole coverage went through the memory system; the march
// passes read and write each element in place, which gives HBM mixed traffic
// at the full rate. In odd cycles the chunks are launched last to first and a
// lane takes its elements from the top; inside a launch the order is only as
// strict as the hardware's dispatch of blocks, so "downwards" is approximate.

#pragma once

#include "hbmtest_core.hpp"

struct HbReport {
  u64 count;
  u64 flipped_or;  // OR of got ^ want over every mismatch
  HbRecord rec[kHbMaxRecords];
};

// One mismatch: exact counts by plain global atomics, the first
// kHbMaxRecords records in the slots the counter handed out. `e` is the
// element inside the chunk; a chunk has at most 2^30 bytes, so its page
// number stays inside the bitmap.
__device__ inline void hb_mismatch(HbReport* __restrict__ report,
                                   HbChunkCount* __restrict__ chunk, u64 pass,
                                   u64 word, size_t e, u64 got, u64 want) {
  u64 slot = atomicAdd(&report->count, 1ull);
  atomicOr(&report->flipped_or, got ^ want);
  atomicAdd(&chunk->count, 1ull);
  unsigned page = (unsigned)((e * sizeof(u64x2)) >> kHbPageShift);
  atomicOr(&chunk->bitmap[page >> 6], 1ull << (page & 63));
  if (slot < (u64)kHbMaxRecords) {
    report->rec[slot].pass = pass;
    report->rec[slot].word = word;
    report->rec[slot].got = got;
    report->rec[slot].want = want;
  }
}

// The launch shape of mem_fill: 256 threads, grid-stride, one 16-byte
// non-temporal access per lane per trip. `word0` is the global index of the
// chunk's first word; with `down` the lane that would take element i takes
// n - 1 - i.
template <int P>
__global__ void __launch_bounds__(256) hbm_fill(u64x2* __restrict__ region,
                                                size_t n, u64 word0, u64 seed,
                                                int down) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    size_t e = down ? n - 1 - i : i;
    u64 w = word0 + 2 * e;
    u64x2 v = {st_word<P>(w, seed), st_word<P>(w + 1, seed)};
    __builtin_nontemporal_store(v, &region[e]);
  }
}

template <int P>
__global__ void __launch_bounds__(256) hbm_verify(
    const u64x2* __restrict__ region, size_t n, u64 word0, u64 seed, int down,
    u64 pass, HbReport* __restrict__ report,
    HbChunkCount* __restrict__ chunk) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    size_t e = down ? n - 1 - i : i;
    u64 w = word0 + 2 * e;
    u64x2 v = __builtin_nontemporal_load(&region[e]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      u64 want = st_word<P>(w + k, seed);
      if (v[k] != want) hb_mismatch(report, chunk, pass, w + k, e, v[k], want);
    }
  }
}

// The word after `want` of pattern P: the next pattern of the cycle, or addr
// with the next cycle's seed after hash_inv. The complement of the expected
// word is free, so an element costs two splitmix64 at the most, and none on
// the way from addr to addr_inv.
template <int P>
__device__ inline u64 hb_next_word(u64 w, u64 want, u64 seed, u64 next_seed) {
  if constexpr (P == kPatAddr || P == kPatHash) return ~want;
  if constexpr (P == kPatAddrInv) return st_mix(w + seed);
  return w ^ next_seed;
}

// A march pass: read an element, compare both words with pattern P, write the
// next round to the same place. One thread owns the element for the whole
// pass, so the update in place has no race. Not unrolled: four loads in
// flight per lane before the first compare were measured against this loop
// (profiles/hbm_selftest.md).
template <int P>
__global__ void __launch_bounds__(256) hbm_march(
    u64x2* __restrict__ region, size_t n, u64 word0, u64 seed, u64 next_seed,
    int down, u64 pass, HbReport* __restrict__ report,
    HbChunkCount* __restrict__ chunk) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    size_t e = down ? n - 1 - i : i;
    u64 w = word0 + 2 * e;
    u64x2 v = __builtin_nontemporal_load(&region[e]);
    u64x2 next;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      u64 want = st_word<P>(w + k, seed);
      if (v[k] != want) hb_mismatch(report, chunk, pass, w + k, e, v[k], want);
      next[k] = hb_next_word<P>(w + k, want, seed, next_seed);
    }
    __builtin_nontemporal_store(next, &region[e]);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr double kHbMaxSeconds = 600.0;
constexpr int kHbProbeMaxChunks = 64;
constexpr int kHbProbeMaxRounds = 64;
constexpr int kHbDefaultBlocks = 1024;  // the grid bandwidth_gbs settled on

#define HB_LAUNCH_BY_PATTERN(pattern, KERNEL, ...)                            \
  switch (pattern) {                                                          \
    case kPatAddr:                                                            \
      hipLaunchKernelGGL(KERNEL(kPatAddr), grid, block, 0, 0, __VA_ARGS__);   \
      break;                                                                  \
    case kPatAddrInv:                                                         \
      hipLaunchKernelGGL(KERNEL(kPatAddrInv), grid, block, 0, 0,              \
                         __VA_ARGS__);                                        \
      break;                                                                  \
    case kPatHash:                                                            \
      hipLaunchKernelGGL(KERNEL(kPatHash), grid, block, 0, 0, __VA_ARGS__);   \
      break;                                                                  \
    default:                                                                  \
      hipLaunchKernelGGL(KERNEL(kPatHashInv), grid, block, 0, 0,              \
                         __VA_ARGS__);                                        \
  }

#define HB_FILL(P) hbm_fill<P>
#define HB_VERIFY(P) hbm_verify<P>
#define HB_MARCH(P) hbm_march<P>

struct HbDevChunk {
  u64x2* ptr;
  HbChunk plan;
};

// What the loop needs besides the chunks: the two report buffers (between
// guards) and, for the test hook, the flips of every pass.
struct HbFlip {
  u64 pass, word, mask;
};

struct HbOutcome {
  u64 rounds = 0;  // rounds written
  u64 passes = 0;  // passes run
  HbReport report;
  std::vector<HbChunkCount> chunks;
  double seconds = 0;
  // event-timed milliseconds and bytes moved per kind of pass
  double ms[4] = {0, 0, 0, 0};
  double bytes[4] = {0, 0, 0, 0};
};
enum HbKind { kHbFill = 0, kHbMarchAddr, kHbMarchHash, kHbVerify };

// XORs the flips of `pass` into the chunks, each through mem_xor with word
// indices inside its chunk. The flips were checked against the plan before
// the first launch.
void hb_apply_flips(const std::vector<HbDevChunk>& chunks,
                    const std::vector<HbChunk>& plan,
                    const std::vector<HbFlip>& flips, u64 pass) {
  for (size_t c = 0; c < chunks.size(); ++c) {
    std::vector<u64> flat;
    for (const HbFlip& f : flips)
      if (f.pass == pass && hb_chunk_of(plan, f.word) == (int)c) {
        flat.push_back(f.word - plan[c].word0);
        flat.push_back(f.mask);
      }
    if (flat.empty()) continue;
    DevBuf dflips(flat.size() * sizeof(u64), flat.data());
    hipLaunchKernelGGL(mem_xor, dim3(1), dim3(64), 0, 0,
                       reinterpret_cast<u64*>(chunks[c].ptr),
                       dflips.as<const u64>(), (int)(flat.size() / 2));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());  // dflips is freed here
  }
}

// Pass 0 fills, passes 1 .. R-1 march, pass R verifies; the host syncs and
// reads the count after every pass, and a pass with a mismatch is the last.
// R is `fixed_rounds` when positive; else passes run until `seconds` have
// passed, always to the end of a cycle of four, and at least one cycle.
void run_hbm_loop(const std::vector<HbDevChunk>& chunks, u64 seed, int blocks,
                  double seconds, u64 fixed_rounds,
                  const std::vector<HbFlip>& flips, const GuardedBuf& report,
                  const GuardedBuf& counts, const char* what, HbOutcome* out) {
  std::vector<HbChunk> plan;
  for (const HbDevChunk& c : chunks) plan.push_back(c.plan);
  const double total = (double)hb_total(plan);
  HbReport* report_dev = report.payload<HbReport>();
  HbChunkCount* counts_dev = counts.payload<HbChunkCount>();
  dim3 grid(blocks), block(256);
  Events ev(2);
  auto t0 = std::chrono::steady_clock::now();
  auto elapsed = [&t0]() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() -
                                         t0)
        .count();
  };
  u64 rounds = fixed_rounds;  // 0: not known yet
  for (u64 pass = 0;; ++pass) {
    if (!fixed_rounds && hb_timed_run_ends(pass, elapsed() >= seconds))
      rounds = pass;
    const bool closing = rounds && pass == rounds;
    // the closing verify goes the way of the round it reads
    const bool down = hb_descending(pass, closing ? rounds : pass + 1);
    if (pass) hb_apply_flips(chunks, plan, flips, pass);
    HbRound now = hb_round(seed, pass);             // written by this pass
    HbRound before = hb_round(seed, pass ? pass - 1 : 0);  // read by it
    int kind = !pass ? kHbFill
               : closing ? kHbVerify
               : before.pattern == kPatAddr ? kHbMarchAddr
                                            : kHbMarchHash;
    HIP_CHECK(hipEventRecord(ev[0]));
    for (size_t k = 0; k < chunks.size(); ++k) {
      size_t c = down ? chunks.size() - 1 - k : k;
      u64x2* ptr = chunks[c].ptr;
      size_t n = (size_t)(plan[c].bytes / sizeof(u64x2));
      u64 word0 = plan[c].word0;
      if (!pass) {
        HB_LAUNCH_BY_PATTERN(now.pattern, HB_FILL, ptr, n, word0, now.seed,
                             (int)down)
      } else if (closing) {
        HB_LAUNCH_BY_PATTERN(before.pattern, HB_VERIFY, (const u64x2*)ptr, n,
                             word0, before.seed, (int)down, pass, report_dev,
                             counts_dev + c)
      } else {
        HB_LAUNCH_BY_PATTERN(before.pattern, HB_MARCH, ptr, n, word0,
                             before.seed, now.seed, (int)down, pass,
                             report_dev, counts_dev + c)
      }
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(ev[1]));
    HIP_CHECK(hipEventSynchronize(ev[1]));
    out->ms[kind] += ev.ms(0, 1);
    out->bytes[kind] +=
        (kind == kHbMarchAddr || kind == kHbMarchHash) ? 2 * total : total;
    out->passes = pass + 1;
    if (!closing) out->rounds = pass + 1;
    HIP_CHECK(hipMemcpy(&out->report, report_dev, sizeof out->report,
                        hipMemcpyDeviceToHost));
    if (out->report.count || closing) break;
  }
  out->seconds = elapsed();
  out->chunks.resize(chunks.size());
  HIP_CHECK(hipMemcpy(out->chunks.data(), counts_dev,
                      chunks.size() * sizeof(HbChunkCount),
                      hipMemcpyDeviceToHost));
  require_guards(report, what);
  require_guards(counts, what);
}

py::dict hbm_dict(int device, u64 seed, const std::vector<HbChunk>& plan,
                  size_t free_bytes, size_t total_bytes, bool alloc_short,
                  double alloc_seconds, const HbOutcome& o) {
  HbSummary s = hb_summarise(o.report.count, o.report.flipped_or, o.report.rec,
                             o.chunks, plan);
  py::list records, bad_chunks, bad_pages_first, chunk_bytes;
  for (const HbRecord& r : s.records)
    records.append(py::make_tuple(r.pass, r.word, r.got, r.want));
  for (const auto& c : s.bad_chunks)
    bad_chunks.append(py::make_tuple(c.first, c.second));
  for (const auto& p : s.bad_pages_first)
    bad_pages_first.append(py::make_tuple(p.first, p.second));
  for (const HbChunk& c : plan) chunk_bytes.append(c.bytes);
  py::dict gbs;
  const char* kinds[4] = {"fill", "march_addr", "march_hash", "verify"};
  for (int k = 0; k < 4; ++k)
    gbs[kinds[k]] = o.ms[k] > 0 ? o.bytes[k] / 1e9 / (o.ms[k] / 1e3) : 0.0;
  py::dict d;
  d["ok"] = s.mismatches == 0;
  d["device"] = device;
  d["seed"] = seed;
  d["seconds"] = o.seconds;
  d["alloc_seconds"] = alloc_seconds;
  d["bytes"] = hb_total(plan);
  d["chunks"] = plan.size();
  d["chunk_bytes"] = chunk_bytes;
  d["free_bytes"] = free_bytes;
  d["total_bytes"] = total_bytes;
  d["alloc_short"] = alloc_short;
  d["rounds"] = o.rounds;
  d["passes"] = o.passes;
  d["mismatches"] = s.mismatches;
  d["flipped_or"] = s.flipped_or;
  d["bad_chunks"] = bad_chunks;
  d["bad_pages"] = s.bad_pages;
  d["bad_pages_first"] = bad_pages_first;
  d["records"] = records;
  // read + write counted for the march passes; march_addr is the pass from
  // addr to addr_inv, which hashes nothing, march_hash the other three, which
  // hash each word once. Event-timed and informative only.
  d["gbs"] = gbs;
  return d;
}

// The production chunks: plain allocations, freed on scope exit.
class HbAllocation {
 public:
  HbAllocation() = default;
  HbAllocation(const HbAllocation&) = delete;
  HbAllocation& operator=(const HbAllocation&) = delete;
  ~HbAllocation() {
    for (void* p : ptrs_) (void)hipFree(p);
  }
  // false when the device has no room for it: the test goes on with what
  // it has
  bool add(size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();  // the error is answered here
      return false;
    }
    HIP_CHECK(e);
    ptrs_.push_back(p);
    return true;
  }
  void* operator[](size_t i) const { return ptrs_[i]; }
  size_t size() const { return ptrs_.size(); }

 private:
  std::vector<void*> ptrs_;
};

void hb_zero_reports(const GuardedBuf& report, const GuardedBuf& counts,
                     size_t chunks) {
  HIP_CHECK(hipMemset(report.payload<void>(), 0, sizeof(HbReport)));
  HIP_CHECK(hipMemset(counts.payload<void>(), 0,
                      chunks * sizeof(HbChunkCount)));
}

py::dict hbm_selftest(int device, double seconds, long long mib, u64 seed,
                      int blocks) {
  if (!(seconds > 0.0) || seconds > kHbMaxSeconds)
    throw std::invalid_argument("seconds must be in (0, 600], got " +
                                std::to_string(seconds));
  if (mib != 0)
    probe_range("mib", mib, (long long)(kHbMinBytes >> 20), kSelftestMaxMib);
  probe_range("blocks", blocks, 0, kProbeMaxBlocks);
  probe_device(device);
  if (blocks == 0) blocks = kHbDefaultBlocks;

  size_t free_bytes = 0, total_bytes = 0;
  HIP_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
  std::vector<HbChunk> plan =
      hb_plan(hb_target(free_bytes, total_bytes, (u64)mib), kHbChunkBytes);
  auto t0 = std::chrono::steady_clock::now();
  HbAllocation alloc;
  bool alloc_short = false;
  for (const HbChunk& c : plan)
    if (!alloc.add((size_t)c.bytes)) {
      alloc_short = true;
      break;
    }
  plan.resize(alloc.size());  // word0 of the chunks that stay is unchanged
  if (hb_total(plan) < kHbMinBytes)
    throw std::runtime_error(
        "hbm march: " + std::to_string(hb_total(plan) >> 20) + " MiB of " +
        std::to_string(free_bytes >> 20) +
        " MiB free could be covered; below 1024 MiB the test would run in "
        "the Infinity Cache");
  std::vector<HbDevChunk> chunks;
  for (size_t c = 0; c < plan.size(); ++c)
    chunks.push_back({reinterpret_cast<u64x2*>(alloc[c]), plan[c]});
  GuardedBuf report(sizeof(HbReport));
  GuardedBuf counts(plan.size() * sizeof(HbChunkCount));
  hb_zero_reports(report, counts, plan.size());
  double alloc_seconds = std::chrono::duration<double>(
                             std::chrono::steady_clock::now() - t0)
                             .count();
  HbOutcome out;
  run_hbm_loop(chunks, seed, blocks, seconds, 0, {}, report, counts,
               "hbm_selftest", &out);
  return hbm_dict(device, seed, plan, free_bytes, total_bytes, alloc_short,
                  alloc_seconds, out);
}

py::tuple hbm_march_probe(
    int device, long long nbytes, u64 seed, int rounds, int blocks,
    long long chunk_bytes,
    const std::vector<std::tuple<long long, long long, u64>>& flips) {
  probe_range("nbytes", nbytes, 16, kProbeMaxBytes);
  if (nbytes % (long long)sizeof(u64x2) != 0)
    throw std::invalid_argument("nbytes must be a multiple of 16");
  probe_range("chunk_bytes", chunk_bytes, 16, kProbeMaxBytes);
  if (chunk_bytes % (long long)sizeof(u64x2) != 0)
    throw std::invalid_argument("chunk_bytes must be a multiple of 16");
  probe_range("rounds", rounds, 1, kHbProbeMaxRounds);
  probe_range("blocks", blocks, 1, kProbeMaxBlocks);
  probe_range("len(flips)", (long long)flips.size(), 0, kMaxFlips);
  std::vector<HbChunk> plan = hb_plan((u64)nbytes, (u64)chunk_bytes);
  probe_range("chunks", (long long)plan.size(), 1, kHbProbeMaxChunks);
  std::vector<HbFlip> checked;
  for (const auto& f : flips) {
    hb_check_flip(plan, (u64)rounds, std::get<0>(f), std::get<1>(f));
    checked.push_back(
        {(u64)std::get<0>(f), (u64)std::get<1>(f), std::get<2>(f)});
  }
  probe_device(device);

  size_t free_bytes = 0, total_bytes = 0;
  HIP_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
  std::vector<std::unique_ptr<GuardedBuf>> bufs;
  std::vector<HbDevChunk> chunks;
  for (const HbChunk& c : plan) {
    bufs.emplace_back(new GuardedBuf((size_t)c.bytes));
    chunks.push_back({bufs.back()->payload<u64x2>(), c});
  }
  GuardedBuf report(sizeof(HbReport));
  GuardedBuf counts(plan.size() * sizeof(HbChunkCount));
  hb_zero_reports(report, counts, plan.size());
  HbOutcome out;
  run_hbm_loop(chunks, seed, blocks, 0.0, (u64)rounds, checked, report, counts,
               "hbm_march_probe", &out);
  py::list raw;
  for (const auto& b : bufs) raw.append(b->download());
  return py::make_tuple(raw, hbm_dict(device, seed, plan, free_bytes,
                                      total_bytes, false, 0.0, out));
}
