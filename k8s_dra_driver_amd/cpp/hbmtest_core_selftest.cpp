// Stand-alone driver of hbmtest_core.hpp: its own main, no Python, no HIP.
// Built with -fsanitize=address,undefined by
// build_native.build_hbmtest_core_selftest and run directly. Exit 0 when
// every check holds; the first failed check is printed and exits 1.

#include "hbmtest_core.hpp"

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

template <typename F>
static bool throws_invalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

template <typename F>
static bool throws_runtime(F f) {
  try {
    f();
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

int main() {
  const uint64_t GiB = 1ull << 30, MiB = 1ull << 20;
  CHECK(hb_mix(0) == 0xE220A8397B1DCDAFull);
  CHECK(hb_mix(1) == 0x910A2DEC89025CC1ull);

  // the reserve and the target
  CHECK(hb_reserve(64 * GiB) == 2 * GiB);
  CHECK(hb_reserve(100 * GiB) == 2 * GiB);
  CHECK(hb_reserve(288000000000ull) == 5760000000ull);
  CHECK(hb_target(10 * GiB, 16 * GiB, 0) == 8 * GiB);
  CHECK(hb_target(10 * GiB + 3 * MiB + 5, 16 * GiB, 0) == 8 * GiB + 2 * MiB);
  CHECK(hb_target(GiB, 16 * GiB, 0) == 0);  // less free than the reserve
  CHECK(hb_target(0, 0, 0) == 0);
  CHECK(hb_target(5, 16 * GiB, 1024) == GiB);  // asked for: free is not used
  CHECK(hb_target(5, 16 * GiB, 1025) == GiB);  // rounded down to a page
  CHECK(hb_target(5, 16 * GiB, 1026) == GiB + 2 * MiB);

  // the plan: word0 continues from chunk to chunk, the last one is shorter
  std::vector<HbChunk> plan = hb_plan(2 * GiB + 6 * MiB, kHbChunkBytes);
  CHECK(plan.size() == 3);
  CHECK(plan[0].bytes == GiB && plan[0].word0 == 0);
  CHECK(plan[1].bytes == GiB && plan[1].word0 == GiB / 8);
  CHECK(plan[2].bytes == 6 * MiB && plan[2].word0 == 2 * GiB / 8);
  CHECK(hb_total(plan) == 2 * GiB + 6 * MiB);
  CHECK(hb_plan(0, 4096).empty() && hb_total(hb_plan(0, 4096)) == 0);
  CHECK(hb_plan(GiB, kHbChunkBytes).size() == 1);
  plan = hb_plan(3 * 4096 + 1024, 4096);
  CHECK(plan.size() == 4 && plan[3].bytes == 1024 && plan[3].word0 == 1536);
  CHECK(hb_chunk_of(plan, 0) == 0 && hb_chunk_of(plan, 511) == 0);
  CHECK(hb_chunk_of(plan, 512) == 1 && hb_chunk_of(plan, 1535) == 2);
  CHECK(hb_chunk_of(plan, 1536 + 127) == 3 && hb_chunk_of(plan, 1536 + 128) < 0);
  CHECK(hb_chunk_of(plan, ~0ull) < 0);
  CHECK(throws_invalid([] { hb_plan(4096, 0); }));
  CHECK(throws_invalid([] { hb_plan(4096, 24); }));
  CHECK(throws_invalid([] { hb_plan(4100, 4096); }));
  CHECK(throws_invalid([] { hb_plan(4096, kHbChunkBytes + 16); }));
  // a short allocation keeps the chunks it has, word0 unchanged
  plan = hb_plan(3 * GiB, kHbChunkBytes);
  plan.resize(2);
  CHECK(hb_total(plan) == 2 * GiB);

  // the schedule
  const uint64_t seed = 0x0123456789ABCDEFull;
  for (uint64_t r = 0; r < 12; ++r) {
    HbRound round = hb_round(seed, r);
    CHECK(round.pattern == (int)(r % 4));
    CHECK(round.seed == hb_mix(seed + r / 4));
  }
  CHECK(hb_round(0, 0).seed == 0xE220A8397B1DCDAFull);
  CHECK(hb_round(~0ull, 4).seed == 0xE220A8397B1DCDAFull);  // wraps
  CHECK(hb_expected(0, 0, 5) == (5 ^ 0xE220A8397B1DCDAFull));
  for (uint64_t w : {0ull, 1ull, 77ull, ~0ull}) {
    CHECK(hb_expected(seed, 1, w) == ~hb_expected(seed, 0, w));
    CHECK(hb_expected(seed, 3, w) == ~hb_expected(seed, 2, w));
    CHECK(hb_expected(seed, 6, w) == hb_mix(w + hb_mix(seed + 1)));
    CHECK(hb_expected(seed, 4, w) != hb_expected(seed, 0, w));
  }
  // direction: by the cycle of the round a pass writes; the closing verify
  // goes the way of the round it reads
  for (uint64_t p = 0; p < 4; ++p) CHECK(!hb_descending(p, 9));
  for (uint64_t p = 4; p < 8; ++p) CHECK(hb_descending(p, 9));
  CHECK(!hb_descending(8, 9) && !hb_descending(9, 9));
  CHECK(!hb_descending(4, 4) && hb_descending(5, 5) && hb_descending(8, 8));
  CHECK(!hb_descending(1, 1));
  // a timed run ends only at the end of a cycle, and not before the first
  CHECK(!hb_timed_run_ends(0, true) && !hb_timed_run_ends(3, true));
  CHECK(hb_timed_run_ends(4, true) && !hb_timed_run_ends(4, false));
  CHECK(!hb_timed_run_ends(6, true) && hb_timed_run_ends(8, true));

  // flips are checked against the plan and the passes
  plan = hb_plan(3 * 4096 + 1024, 4096);
  hb_check_flip(plan, 5, 1, 0);
  hb_check_flip(plan, 5, 5, 1536 + 127);
  CHECK(throws_invalid([&] { hb_check_flip(plan, 5, 0, 0); }));
  CHECK(throws_invalid([&] { hb_check_flip(plan, 5, 6, 0); }));
  CHECK(throws_invalid([&] { hb_check_flip(plan, 5, -1, 0); }));
  CHECK(throws_invalid([&] { hb_check_flip(plan, 5, 1, -1); }));
  CHECK(throws_invalid([&] { hb_check_flip(plan, 5, 1, 1536 + 128); }));

  // aggregation
  std::vector<HbChunkCount> counts(plan.size());
  for (auto& c : counts) c = HbChunkCount{};
  HbRecord none[1] = {{0, 0, 0, 0}};
  HbSummary s = hb_summarise(0, 0, none, counts, plan);
  CHECK(s.mismatches == 0 && s.records.empty() && s.bad_chunks.empty());
  CHECK(s.bad_pages == 0 && s.bad_pages_first.empty());

  HbRecord two[2] = {{3, 600, 0xF1, 0xF0}, {3, 5, 0x8000000000000000ull, 0}};
  counts[0].count = 1;
  counts[0].bitmap[0] = 1;
  counts[1].count = 1;
  counts[1].bitmap[0] = 1;
  s = hb_summarise(2, 0x8000000000000001ull, two, counts, plan);
  CHECK(s.mismatches == 2 && s.flipped_or == 0x8000000000000001ull);
  CHECK(s.records.size() == 2 && s.records[0].word == 5);  // sorted
  CHECK(s.bad_chunks.size() == 2 && s.bad_chunks[1].first == 1);
  CHECK(s.bad_pages == 2 && s.bad_pages_first[1].first == 1 &&
        s.bad_pages_first[1].second == 0);
  // more mismatches than records: the first 64 are kept
  {
    std::vector<HbRecord> many(kHbMaxRecords);
    for (int i = 0; i < kHbMaxRecords; ++i)
      many[i] = {1, (uint64_t)(kHbMaxRecords - i), 1, 0};
    std::vector<HbChunkCount> c2(plan.size());
    for (auto& c : c2) c = HbChunkCount{};
    c2[0].count = 100;
    c2[0].bitmap[0] = 1;
    s = hb_summarise(100, 1, many.data(), c2, plan);
    CHECK(s.mismatches == 100 && s.records.size() == 64);
    CHECK(s.records.front().word == 1 && s.records.back().word == 64);
  }
  // pages of a full chunk, and more bad pages than a result names
  {
    std::vector<HbChunk> big = hb_plan(2 * GiB, kHbChunkBytes);
    std::vector<HbChunkCount> c2(2);
    for (auto& c : c2) c = HbChunkCount{};
    c2[1].count = 12;
    c2[1].bitmap[0] = 0xFF;
    c2[1].bitmap[7] = 0xF000000000000000ull;
    std::vector<HbRecord> twelve(12);  // the caller hands min(count, 64)
    for (int i = 0; i < 12; ++i) twelve[i] = {2, GiB / 8 + i, 1, 0};
    s = hb_summarise(12, 1, twelve.data(), c2, big);
    CHECK(s.bad_pages == 12 && s.bad_pages_first.size() == kHbPagesFirst);
    CHECK(s.bad_pages_first[7].first == 1 && s.bad_pages_first[7].second == 7);
    CHECK(s.bad_chunks.size() == 1 && s.bad_chunks[0].second == 12);
  }
  // counters that contradict each other are a fault of the test
  HbRecord three[3] = {two[0], two[1], {3, 6, 1, 0}};
  CHECK(throws_runtime([&] {  // the chunks count 2
    hb_summarise(3, 0x8000000000000001ull, three, counts, plan);
  }));
  CHECK(throws_runtime([&] { hb_summarise(2, 0, two, counts, plan); }));
  CHECK(throws_runtime([&] { hb_summarise(2, 1, two, counts, plan); }));
  {
    std::vector<HbChunkCount> c2 = counts;
    c2[1].bitmap[0] = 0;  // a count without a page
    CHECK(throws_runtime(
        [&] { hb_summarise(2, 0x8000000000000001ull, two, c2, plan); }));
    c2 = counts;
    c2[1].bitmap[0] = 2;  // page 1 of a 4 KiB chunk
    CHECK(throws_runtime(
        [&] { hb_summarise(2, 0x8000000000000001ull, two, c2, plan); }));
    c2 = counts;
    c2.pop_back();
    CHECK(throws_runtime(
        [&] { hb_summarise(2, 0x8000000000000001ull, two, c2, plan); }));
    HbRecord outside[2] = {{3, 99999, 1, 0}, {3, 5, 1, 0}};
    CHECK(throws_runtime([&] { hb_summarise(2, 1, outside, counts, plan); }));
  }

  std::puts("hbmtest_core_selftest: ok");
  return 0;
}
