// Host core of the HBM march self-test: the chunk plan, the round schedule,
// the expected word and the aggregation of a raw report. No HIP and no
// pybind includes, so hbmtest_core_selftest.cpp can drive it under
// AddressSanitizer and UBSan without a GPU; hbmtest_kernels.hpp includes it
// for the host loop. tests/hbmtest_reference.py mirrors it in numpy.
//
// The coverage is one array of little-endian 64-bit words with a global index
// w, cut into chunks of kHbChunkBytes (the last may be shorter). Round r
// leaves pattern r % 4 (addr, addr_inv, hash, hash_inv of
// selftest_kernels.hpp) with seed hb_mix(seed + r / 4) in every word, so a
// bit holds both values in consecutive rounds and every cycle of four rounds
// has a seed of its own. Pass 0 writes round 0; pass p, 1 <= p < R, reads
// round p - 1 and writes round p in place; pass R reads round R - 1.

#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

constexpr uint64_t kHbChunkBytes = 1ull << 30;
constexpr uint64_t kHbPageBytes = 2ull << 20;  // the blocks a mismatch is named by
constexpr int kHbPageShift = 21;
static_assert(1ull << kHbPageShift == kHbPageBytes, "page shift");
constexpr int kHbBitmapWords = 8;  // 512 pages of a chunk, one bit each
static_assert(kHbChunkBytes / kHbPageBytes == 64ull * kHbBitmapWords,
              "the bitmap has a bit for every page of a full chunk");
// below this the region would sit in the 256 MiB Infinity Cache, not in HBM
constexpr uint64_t kHbMinBytes = 1ull << 30;
// what the default coverage leaves free: max(2 GiB, 2 % of the total)
constexpr uint64_t kHbReserveMinBytes = 2ull << 30;
constexpr int kHbReservePercent = 2;
constexpr int kHbMaxRecords = 64;
constexpr int kHbPagesFirst = 8;  // bad pages a result names
constexpr int kHbPatterns = 4;

// splitmix64 finaliser, the same function as st_mix of selftest_kernels.hpp;
// mix(0) = 0xE220A8397B1DCDAF.
inline uint64_t hb_mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---------------------------------------------------------------------------
// chunk plan
// ---------------------------------------------------------------------------
inline uint64_t hb_reserve(uint64_t total_bytes) {
  return std::max<uint64_t>(kHbReserveMinBytes,
                            total_bytes / 100 * kHbReservePercent);
}

// Bytes to cover: mib MiB when asked for, else what is free less the reserve;
// rounded down to whole pages.
inline uint64_t hb_target(uint64_t free_bytes, uint64_t total_bytes,
                          uint64_t mib) {
  uint64_t target = mib << 20;
  if (mib == 0) {
    uint64_t reserve = hb_reserve(total_bytes);
    target = free_bytes > reserve ? free_bytes - reserve : 0;
  }
  return target / kHbPageBytes * kHbPageBytes;
}

struct HbChunk {
  uint64_t bytes;  // a multiple of 16
  uint64_t word0;  // global index of its first word
};

// `total` bytes as chunks of `chunk_bytes`, the last one shorter when total
// is no multiple. Both are multiples of 16.
inline std::vector<HbChunk> hb_plan(uint64_t total, uint64_t chunk_bytes) {
  if (chunk_bytes == 0 || chunk_bytes % 16 != 0 || chunk_bytes > kHbChunkBytes)
    throw std::invalid_argument(
        "chunk_bytes must be a multiple of 16 in [16, 2^30], got " +
        std::to_string(chunk_bytes));
  if (total % 16 != 0)
    throw std::invalid_argument("the coverage must be a multiple of 16, got " +
                                std::to_string(total));
  std::vector<HbChunk> plan;
  for (uint64_t at = 0; at < total; at += chunk_bytes)
    plan.push_back({std::min(chunk_bytes, total - at), at / 8});
  return plan;
}

inline uint64_t hb_total(const std::vector<HbChunk>& plan) {
  return plan.empty() ? 0 : plan.back().word0 * 8 + plan.back().bytes;
}

// The chunk that holds global word w, -1 when none does.
inline int hb_chunk_of(const std::vector<HbChunk>& plan, uint64_t w) {
  for (size_t c = 0; c < plan.size(); ++c)
    if (w >= plan[c].word0 && w - plan[c].word0 < plan[c].bytes / 8)
      return (int)c;
  return -1;
}

// ---------------------------------------------------------------------------
// round schedule
// ---------------------------------------------------------------------------
struct HbRound {
  int pattern;    // MemPattern of selftest_kernels.hpp
  uint64_t seed;  // of its cycle of four
};

inline HbRound hb_round(uint64_t seed, uint64_t r) {
  return {(int)(r % kHbPatterns), hb_mix(seed + r / kHbPatterns)};
}

inline uint64_t hb_word(int pattern, uint64_t w, uint64_t seed) {
  switch (pattern) {
    case 0:
      return w ^ seed;
    case 1:
      return ~(w ^ seed);
    case 2:
      return hb_mix(w + seed);
    default:
      return ~hb_mix(w + seed);
  }
}

// What round r leaves in global word w.
inline uint64_t hb_expected(uint64_t seed, uint64_t r, uint64_t w) {
  HbRound round = hb_round(seed, r);
  return hb_word(round.pattern, w, round.seed);
}

// Pass p of a run of `rounds` rounds goes downwards (chunks last to first,
// elements from the top) in the odd cycles of the round it writes; the
// closing verify writes none and goes the way of the round it reads.
inline bool hb_descending(uint64_t pass, uint64_t rounds) {
  uint64_t r = std::min(pass, rounds - 1);
  return (r / kHbPatterns) & 1;
}

// Rounds of a timed run after `done` rounds were written: it ends at the
// first whole cycle at which the time is up.
inline bool hb_timed_run_ends(uint64_t done, bool time_is_up) {
  return done >= kHbPatterns && done % kHbPatterns == 0 && time_is_up;
}

// ---------------------------------------------------------------------------
// report
// ---------------------------------------------------------------------------
struct HbRecord {
  uint64_t pass, word, got, want;
};

struct HbChunkCount {  // per chunk, as the kernels keep it
  uint64_t count;
  uint64_t bitmap[kHbBitmapWords];  // bit p: page p held a mismatch
};

struct HbSummary {
  uint64_t mismatches = 0;
  uint64_t flipped_or = 0;
  std::vector<HbRecord> records;                      // sorted, at most 64
  std::vector<std::pair<int, uint64_t>> bad_chunks;   // (chunk, mismatches)
  uint64_t bad_pages = 0;
  std::vector<std::pair<int, int>> bad_pages_first;   // (chunk, page)
};

inline bool hb_record_less(const HbRecord& a, const HbRecord& b) {
  if (a.pass != b.pass) return a.pass < b.pass;
  if (a.word != b.word) return a.word < b.word;
  if (a.got != b.got) return a.got < b.got;
  return a.want < b.want;
}

// The raw counters as the result's fields; `rec` holds min(count,
// kHbMaxRecords) records. Throws std::runtime_error when
// they contradict each other: that is a fault of the test, not a finding.
inline HbSummary hb_summarise(uint64_t count, uint64_t flipped_or,
                              const HbRecord* rec,
                              const std::vector<HbChunkCount>& chunks,
                              const std::vector<HbChunk>& plan) {
  if (chunks.size() != plan.size())
    throw std::runtime_error("hbm march: a count for every chunk is needed");
  HbSummary s;
  s.mismatches = count;
  s.flipped_or = flipped_or;
  uint64_t kept = std::min<uint64_t>(count, kHbMaxRecords);
  s.records.assign(rec, rec + kept);
  std::sort(s.records.begin(), s.records.end(), hb_record_less);
  uint64_t in_chunks = 0;
  for (size_t c = 0; c < chunks.size(); ++c) {
    const HbChunkCount& cc = chunks[c];
    uint64_t pages = (plan[c].bytes + kHbPageBytes - 1) / kHbPageBytes;
    uint64_t bits = 0;
    for (int p = 0; p < 64 * kHbBitmapWords; ++p) {
      if (!(cc.bitmap[p / 64] >> (p % 64) & 1)) continue;
      if ((uint64_t)p >= pages)
        throw std::runtime_error("hbm march: chunk " + std::to_string(c) +
                                 " marks a page it does not have");
      ++bits;
      if ((int)s.bad_pages_first.size() < kHbPagesFirst)
        s.bad_pages_first.push_back({(int)c, p});
    }
    if ((cc.count != 0) != (bits != 0) || bits > cc.count)
      throw std::runtime_error("hbm march: count and page bitmap of chunk " +
                               std::to_string(c) + " disagree");
    s.bad_pages += bits;
    in_chunks += cc.count;
    if (cc.count) s.bad_chunks.push_back({(int)c, cc.count});
  }
  if (in_chunks != count)
    throw std::runtime_error(
        "hbm march: the per-chunk counts do not add up to the count");
  if ((count != 0) != (flipped_or != 0))
    throw std::runtime_error(
        "hbm march: the count and the flipped bits disagree");
  for (const HbRecord& r : s.records)
    if (hb_chunk_of(plan, r.word) < 0 || r.got == r.want ||
        ((r.got ^ r.want) & ~flipped_or))
      throw std::runtime_error("hbm march: a record names word " +
                               std::to_string(r.word) +
                               " that cannot have mismatched");
  return s;
}

// A flip of the test hook: `mask` is XORed into global word `word` before
// pass `pass` reads. Throws std::invalid_argument on one that is outside the
// coverage or the passes that read.
inline void hb_check_flip(const std::vector<HbChunk>& plan, uint64_t rounds,
                          long long pass, long long word) {
  if (pass < 1 || (uint64_t)pass > rounds)
    throw std::invalid_argument("flip pass must be in [1, " +
                                std::to_string(rounds) + "], got " +
                                std::to_string(pass));
  if (word < 0 || hb_chunk_of(plan, (uint64_t)word) < 0)
    throw std::invalid_argument(
        "flip word index " + std::to_string(word) +
        " outside the coverage of " + std::to_string(hb_total(plan) / 8) +
        " words");
}
