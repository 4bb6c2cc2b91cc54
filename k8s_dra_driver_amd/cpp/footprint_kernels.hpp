// CU footprint of _hiphealth: which compute units a process's blocks run on.
// Included by hiphealth.hip inside its anonymous namespace, after
// selftest_kernels.hpp (HIP_CHECK, probe_device, probe_range, GuardedBuf,
// Events, require_guards, kCanary, kGuard, kProbeMaxBlocks).
//
//   cu_footprint()        - production path: one launch, the distinct
//                           (xcc, se, sh, cu) the blocks reported
//   cu_footprint_probe()  - test hook: one launch between guards, the raw
//                           records returned
//
// A SharedCompute share is an HSA_CU_MASK bit range (sharing/shared.py).
// How the kernel driver spreads those bits over XCDs and shader engines is
// its own business, so the only way to know where a share runs is to ask
// the waves: every block stores the hardware id registers of the wave that
// holds its thread 0. The kernel stores the raw words; decoding is the
// host's job (here and in sharing/footprint.py, which mirrors it).

#pragma once

#include <map>
#include <tuple>

// One block's answer, 16 bytes, stored whole.
struct alignas(16) FootRecord {
  unsigned hw_id;   // HW_REG_HW_ID, all 32 bits
  unsigned xcc_id;  // HW_REG_XCC_ID, bits 3:0
  unsigned block;   // blockIdx.x
  unsigned pad;     // 0
};
static_assert(sizeof(FootRecord) == 16, "FootRecord is one 16-byte store");
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// s_getreg_b32 immediate: SIZE-1 in 15:11, OFFSET in 10:6, register in 5:0.
constexpr int foot_getreg(int size, int offset, int reg) {
  return ((size - 1) << 11) | (offset << 6) | reg;
}
constexpr int kRegHwId = 4;    // HW_REG_HW_ID
constexpr int kRegXccId = 20;  // HW_REG_XCC_ID (gfx942, gfx950)

// Fields of HW_ID on CDNA with four shader engines per XCC, as HIP's own
// __smid() reads them (hip/amd_detail/amd_device_functions.h):
//   CU_ID 11:8, SH_ID 12, SE_ID 14:13; XCC_ID 3:0 of its own register.
// WAVE_ID 3:0, SIMD_ID 5:4, PIPE_ID 7:6, bit 15 and everything above say
// which wave slot and queue, not which CU, and are dropped.
struct CuKey {
  unsigned xcc, se, sh, cu;
  bool operator<(const CuKey& o) const {
    return std::tie(xcc, se, sh, cu) < std::tie(o.xcc, o.se, o.sh, o.cu);
  }
};
inline CuKey foot_decode(unsigned hw_id, unsigned xcc_id) {
  return {xcc_id & 0xFu, (hw_id >> 13) & 0x3u, (hw_id >> 12) & 0x1u,
          (hw_id >> 8) & 0xFu};
}

constexpr int kFootThreads = 1024;  // 16 waves: at most two blocks fit on a CU
constexpr int kFootMaxSpin = 1 << 20;
constexpr int kFootBlocksPerCu = 8;
// Default spin of cu_footprint: four times the smallest power of two at
// which an unmasked MI355X reported all of its CUs with the default grid.
// That power is 1: the dispatcher deals blocks over the enabled CUs however
// briefly they stay (profiles/cu_footprint.md has the sweep).
constexpr int kFootDefaultSpin = 4;

// Every thread runs exactly `spin` dependent FMAs (a fixed count, as in
// valu_burn: nothing here waits on a clock or a flag), which keeps the block
// resident while the dispatcher places the blocks behind it. Thread 0 then
// stores where its wave is running.
__global__ void __launch_bounds__(kFootThreads) cu_where(
    FootRecord* __restrict__ out, int spin) {
  float x = 1.0f + threadIdx.x * 1e-6f;
  for (int i = 0; i < spin; ++i) x = fmaf(x, 1.0000001f, 1e-7f);
  asm volatile("" ::"v"(x));  // the chain has no other use
  if (threadIdx.x == 0) {
    unsigned hw = __builtin_amdgcn_s_getreg(foot_getreg(32, 0, kRegHwId));
    unsigned xcc = __builtin_amdgcn_s_getreg(foot_getreg(4, 0, kRegXccId));
    u32x4 rec = {hw, xcc, blockIdx.x, 0u};
    *reinterpret_cast<u32x4*>(&out[blockIdx.x]) = rec;
  }
}

void launch_cu_where(FootRecord* out, int blocks, int spin) {
  hipLaunchKernelGGL(cu_where, dim3(blocks), dim3(kFootThreads), 0, 0, out,
                     spin);
  HIP_CHECK(hipGetLastError());
}

py::bytes cu_footprint_probe(int device, int blocks, int spin) {
  probe_range("blocks", blocks, 1, kProbeMaxBlocks);
  probe_range("spin", spin, 0, kFootMaxSpin);
  probe_device(device);
  GuardedBuf out((size_t)blocks * sizeof(FootRecord));
  launch_cu_where(out.payload<FootRecord>(), blocks, spin);
  HIP_CHECK(hipDeviceSynchronize());
  return out.download();
}

py::dict cu_footprint(int device, int blocks, int spin) {
  probe_range("blocks", blocks, 0, kProbeMaxBlocks);
  probe_range("spin", spin, 0, kFootMaxSpin);
  probe_device(device);
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  if (blocks == 0)
    blocks = std::min(kFootBlocksPerCu * prop.multiProcessorCount,
                      kProbeMaxBlocks);
  if (spin == 0) spin = kFootDefaultSpin;

  GuardedBuf out((size_t)blocks * sizeof(FootRecord));
  Events ev(2);
  HIP_CHECK(hipEventRecord(ev[0]));
  launch_cu_where(out.payload<FootRecord>(), blocks, spin);
  HIP_CHECK(hipEventRecord(ev[1]));
  HIP_CHECK(hipEventSynchronize(ev[1]));
  double kernel_ms = ev.ms(0, 1);
  require_guards(out, "cu_footprint");
  std::vector<FootRecord> host(blocks);
  HIP_CHECK(hipMemcpy(host.data(), out.payload<void>(),
                      host.size() * sizeof(FootRecord),
                      hipMemcpyDeviceToHost));

  std::map<CuKey, int> per_cu;
  for (int b = 0; b < blocks; ++b) {
    const FootRecord& r = host[b];
    if (r.block != (unsigned)b || r.pad != 0u)
      throw std::runtime_error("cu_footprint: block " + std::to_string(b) +
                               " left no record");
    ++per_cu[foot_decode(r.hw_id, r.xcc_id)];
  }
  py::list cus;
  std::map<unsigned, int> xcc_count;
  int lo = blocks, hi = 0;
  for (const auto& kv : per_cu) {  // std::map iterates in sorted order
    const CuKey& k = kv.first;
    cus.append(py::make_tuple(k.xcc, k.se, k.sh, k.cu));
    ++xcc_count[k.xcc];
    lo = std::min(lo, kv.second);
    hi = std::max(hi, kv.second);
  }
  py::dict per_xcc;
  for (const auto& kv : xcc_count) per_xcc[py::int_(kv.first)] = kv.second;

  py::dict d;
  d["cus"] = cus;
  d["count"] = per_cu.size();
  d["per_xcc"] = per_xcc;
  d["blocks_per_cu_min"] = lo;
  d["blocks_per_cu_max"] = hi;
  d["blocks"] = blocks;
  d["spin"] = spin;
  d["multi_processor_count"] = prop.multiProcessorCount;
  d["kernel_ms"] = kernel_ms;
  return d;
}
