// Startup self-test of _hiphealth: HBM pattern test and MFMA known-answer
// test. Included by hiphealth.hip inside its anonymous namespace, after the
// probe helpers it uses (HIP_CHECK, probe_device, probe_range, GuardedBuf,
// bf16x8, f32x4).
//
//   selftest()        - production path: four fill/verify passes over one
//                       region, then the MFMA known-answer test
//   memtest_probe()   - test hook: one fill (and verify) between guards,
//                       with wrong data injected by the caller
//   mfma_kat_probe()  - test hook: the known-answer kernel on the caller's
//                       table, so a wrong expectation exercises the comparator
//   pci_bus_id()      - which physical GPU a HIP ordinal is
//
// Both tests report the same way: an exact mismatch counter (one ordinary
// global atomicAdd per mismatch) and the first kMaxRecords mismatches, each
// stored in the slot the atomicAdd returned. The count is exact; the order
// of the records is whatever order the waves arrived in.

#pragma once

#include <cstdint>
#include <cstring>
#include <utility>

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr int kMaxRecords = 64;
constexpr int kMaxFlips = 4096;
constexpr int kSelftestMaxMib = 1 << 18;  // 256 GiB: below the HBM size

// ---------------------------------------------------------------------------
// memory patterns. The region is n 16-byte elements = 2n little-endian
// 64-bit words; word w is an index inside the region, not an address, so
// the host (and numpy) can reproduce every pattern.
// ---------------------------------------------------------------------------
enum MemPattern { kPatAddr = 0, kPatAddrInv, kPatHash, kPatHashInv };
constexpr const char* kPatternNames[4] = {"addr", "addr_inv", "hash",
                                          "hash_inv"};

// splitmix64 finaliser; mix(0) = 0xE220A8397B1DCDAF.
__host__ __device__ inline u64 st_mix(u64 x) {
  u64 z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <int P>
__host__ __device__ inline u64 st_word(u64 w, u64 seed) {
  if constexpr (P == kPatAddr) return w ^ seed;
  if constexpr (P == kPatAddrInv) return ~(w ^ seed);
  if constexpr (P == kPatHash) return st_mix(w + seed);
  return ~st_mix(w + seed);
}

struct MemRecord {
  u64 word, got, want;
};
struct MemReport {
  u64 count;
  MemRecord rec[kMaxRecords];
};

// Same launch shape as copy_f4_nt: 256 threads, grid-stride, one 16-byte
// non-temporal access per lane per trip. The data is written once and read
// once, so neither pass asks the caches to keep it.
template <int P>
__global__ void __launch_bounds__(256) mem_fill(u64x2* __restrict__ region,
                                                size_t n, u64 seed) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    u64x2 v = {st_word<P>(2 * i, seed), st_word<P>(2 * i + 1, seed)};
    __builtin_nontemporal_store(v, &region[i]);
  }
}

// Reads the region and nothing else of it: the pointer is const, every
// store goes to the report.
template <int P>
__global__ void __launch_bounds__(256) mem_verify(
    const u64x2* __restrict__ region, size_t n, u64 seed,
    MemReport* __restrict__ report) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    u64x2 v = __builtin_nontemporal_load(&region[i]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      u64 want = st_word<P>(2 * i + k, seed);
      if (v[k] != want) {
        u64 slot = atomicAdd(&report->count, 1ull);
        if (slot < (u64)kMaxRecords) {
          report->rec[slot].word = 2 * i + k;
          report->rec[slot].got = v[k];
          report->rec[slot].want = want;
        }
      }
    }
  }
}

// Test hook only: one thread XORs masks into words the host has already
// checked to lie inside the region (wrong data, never a wrong address).
__global__ void mem_xor(u64* __restrict__ words, const u64* __restrict__ flips,
                        int count) {
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int k = 0; k < count; ++k) words[flips[2 * k]] ^= flips[2 * k + 1];
}

void launch_mem_fill(int pattern, int blocks, u64x2* region, size_t n,
                     u64 seed) {
  dim3 grid(blocks), block(256);
  switch (pattern) {
    case kPatAddr:
      hipLaunchKernelGGL(mem_fill<kPatAddr>, grid, block, 0, 0, region, n, seed);
      break;
    case kPatAddrInv:
      hipLaunchKernelGGL(mem_fill<kPatAddrInv>, grid, block, 0, 0, region, n,
                         seed);
      break;
    case kPatHash:
      hipLaunchKernelGGL(mem_fill<kPatHash>, grid, block, 0, 0, region, n, seed);
      break;
    default:
      hipLaunchKernelGGL(mem_fill<kPatHashInv>, grid, block, 0, 0, region, n,
                         seed);
  }
  HIP_CHECK(hipGetLastError());
}

void launch_mem_verify(int pattern, int blocks, const u64x2* region, size_t n,
                       u64 seed, MemReport* report) {
  dim3 grid(blocks), block(256);
  switch (pattern) {
    case kPatAddr:
      hipLaunchKernelGGL(mem_verify<kPatAddr>, grid, block, 0, 0, region, n,
                         seed, report);
      break;
    case kPatAddrInv:
      hipLaunchKernelGGL(mem_verify<kPatAddrInv>, grid, block, 0, 0, region, n,
                         seed, report);
      break;
    case kPatHash:
      hipLaunchKernelGGL(mem_verify<kPatHash>, grid, block, 0, 0, region, n,
                         seed, report);
      break;
    default:
      hipLaunchKernelGGL(mem_verify<kPatHashInv>, grid, block, 0, 0, region, n,
                         seed, report);
  }
  HIP_CHECK(hipGetLastError());
}

int pattern_from_name(const std::string& name) {
  for (int p = 0; p < 4; ++p)
    if (name == kPatternNames[p]) return p;
  throw std::invalid_argument(
      "pattern must be addr, addr_inv, hash or hash_inv, got '" + name + "'");
}

// ---------------------------------------------------------------------------
// MFMA known-answer test. Wave g takes vector g % kKatVectors of the table:
// per lane 8 bf16 of A, 8 bf16 of B, 4 floats of C and the 4 floats that 4
// chained v_mfma_f32_16x16x32_bf16 must leave in its accumulator. The table
// values are m * 2^e, |m| <= 15, e in [-2, 2], and integer |C| <= 1000, so
// every partial sum is exact in fp32 in any order (tests/test_hip_kernels.py
// has the argument) and the comparison is of bits.
// ---------------------------------------------------------------------------
constexpr int kKatVectors = 16;
constexpr int kKatChain = 4;
constexpr size_t kKatFragBytes = (size_t)kKatVectors * 64 * 16;  // per table

struct KatRecord {
  unsigned wave, lane, slot, got, want;
};
struct KatReport {
  u64 count;
  KatRecord rec[kMaxRecords];
};

__global__ void __launch_bounds__(256) mfma_kat(
    const bf16x8* __restrict__ a_tab, const bf16x8* __restrict__ b_tab,
    const f32x4* __restrict__ c_tab, const f32x4* __restrict__ want_tab,
    KatReport* __restrict__ report) {
  unsigned lane = threadIdx.x & 63;
  unsigned wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  unsigned idx = (wave % kKatVectors) * 64 + lane;
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
      u64 slot = atomicAdd(&report->count, 1ull);
      if (slot < (u64)kMaxRecords) {
        KatRecord rec = {wave, lane, (unsigned)r, got_bits, want_bits};
        report->rec[slot] = rec;
      }
    }
  }
}

// Lane maps of v_mfma_f32_16x16x32_bf16, as tests/hip_reference.py writes
// them out and checks them on the CPU:
//   A slot j of lane l = A[l & 15][8 * (l >> 4) + j]
//   B slot j of lane l = B[8 * (l >> 4) + j][l & 15]
//   C/D register r of lane l = C[4 * (l >> 4) + r][l & 15]
struct KatTable {
  std::vector<uint16_t> a, b;  // kKatVectors x 64 x 8
  std::vector<float> c, want;  // kKatVectors x 64 x 4
};

inline uint16_t bf16_bits_exact(float v) {
  uint32_t bits;
  std::memcpy(&bits, &v, sizeof bits);
  return (uint16_t)(bits >> 16);  // 4 significant bits: the low half is 0
}

KatTable make_kat_table(u64 seed) {
  KatTable t;
  t.a.resize((size_t)kKatVectors * 64 * 8);
  t.b.resize(t.a.size());
  t.c.resize((size_t)kKatVectors * 64 * 4);
  t.want.resize(t.c.size());
  u64 state = seed;
  auto next = [&state]() { return st_mix(state++); };
  auto operand = [&next]() {  // m * 2^e
    u64 r = next();
    int m = (int)(r % 31) - 15;
    int e = (int)((r >> 32) % 5) - 2;
    return std::ldexp((double)m, e);
  };
  for (int v = 0; v < kKatVectors; ++v) {
    double A[16][32], B[32][16], C[16][16], D[16][16];
    for (auto& row : A)
      for (double& x : row) x = operand();
    for (auto& row : B)
      for (double& x : row) x = operand();
    for (auto& row : C)
      for (double& x : row) x = (double)((long long)(next() % 2001) - 1000);
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        double s = 0;
        for (int k = 0; k < 32; ++k) s += A[i][k] * B[k][j];
        D[i][j] = kKatChain * s + C[i][j];
      }
    for (int l = 0; l < 64; ++l) {
      size_t frag = ((size_t)v * 64 + l);
      for (int j = 0; j < 8; ++j) {
        t.a[frag * 8 + j] = bf16_bits_exact((float)A[l & 15][8 * (l >> 4) + j]);
        t.b[frag * 8 + j] = bf16_bits_exact((float)B[8 * (l >> 4) + j][l & 15]);
      }
      for (int r = 0; r < 4; ++r) {
        t.c[frag * 4 + r] = (float)C[4 * (l >> 4) + r][l & 15];
        t.want[frag * 4 + r] = (float)D[4 * (l >> 4) + r][l & 15];
      }
    }
  }
  return t;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Plain device allocation, freed on scope exit (the production region has
// no guards: it is as large as the operator asks).
class DevBuf {
 public:
  explicit DevBuf(size_t bytes, const void* init = nullptr) {
    HIP_CHECK(hipMalloc(&p_, bytes ? bytes : 1));
    if (init && bytes) {
      hipError_t e = hipMemcpy(p_, init, bytes, hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        (void)hipFree(p_);
        HIP_CHECK(e);
      }
    }
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)hipFree(p_); }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p_);
  }
 private:
  void* p_ = nullptr;
};

class Events {
 public:
  explicit Events(int n) : ev_(n, nullptr) {
    for (auto& e : ev_) HIP_CHECK(hipEventCreate(&e));
  }
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  ~Events() {
    for (auto e : ev_)
      if (e) (void)hipEventDestroy(e);
  }
  hipEvent_t operator[](int i) const { return ev_[i]; }
  double ms(int from, int to) const {
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, ev_[from], ev_[to]));
    return t;
  }

 private:
  std::vector<hipEvent_t> ev_;
};

py::list mem_records(const MemReport& r) {
  py::list out;
  u64 m = std::min<u64>(r.count, kMaxRecords);
  for (u64 i = 0; i < m; ++i)
    out.append(py::make_tuple(r.rec[i].word, r.rec[i].got, r.rec[i].want));
  return out;
}

py::list kat_records(const KatReport& r) {
  py::list out;
  u64 m = std::min<u64>(r.count, kMaxRecords);
  for (u64 i = 0; i < m; ++i)
    out.append(py::make_tuple(r.rec[i].wave, r.rec[i].lane, r.rec[i].slot,
                              r.rec[i].got, r.rec[i].want));
  return out;
}

// A report buffer's guards must come back untouched: the kernels index it
// with a slot number they were handed by an atomic.
void require_guards(const GuardedBuf& buf, const char* what) {
  std::string raw = buf.download();
  for (size_t i = 0; i < kGuard; ++i)
    if ((unsigned char)raw[i] != kCanary ||
        (unsigned char)raw[raw.size() - 1 - i] != kCanary)
      throw std::runtime_error(std::string(what) +
                               ": a guard of the report buffer changed");
}

// One launch of mfma_kat on a table already on the device.
void launch_mfma_kat(const bf16x8* a, const bf16x8* b, const f32x4* c,
                     const f32x4* want, int blocks, KatReport* report) {
  hipLaunchKernelGGL(mfma_kat, dim3(blocks), dim3(256), 0, 0, a, b, c, want,
                     report);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
}

py::dict selftest(int device, int mib, u64 seed, int blocks) {
  probe_range("mib", mib, 1, kSelftestMaxMib);
  probe_range("blocks", blocks, 0, kProbeMaxBlocks);
  probe_device(device);
  // 1024 workgroups: the grid bandwidth_gbs settled on from measurements
  if (blocks == 0) blocks = 1024;
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));

  size_t bytes = (size_t)mib << 20;
  size_t n = bytes / sizeof(u64x2);
  bool ok = true;
  py::list passes;
  {
    DevBuf region(bytes);
    DevBuf report(sizeof(MemReport));
    Events ev(3);
    MemReport host;
    for (int p = 0; p < 4; ++p) {
      HIP_CHECK(hipMemset(report.as<void>(), 0, sizeof(MemReport)));
      HIP_CHECK(hipEventRecord(ev[0]));
      launch_mem_fill(p, blocks, region.as<u64x2>(), n, seed);
      HIP_CHECK(hipEventRecord(ev[1]));
      launch_mem_verify(p, blocks, region.as<const u64x2>(), n, seed,
                        report.as<MemReport>());
      HIP_CHECK(hipEventRecord(ev[2]));
      HIP_CHECK(hipEventSynchronize(ev[2]));
      HIP_CHECK(hipMemcpy(&host, report.as<void>(), sizeof host,
                          hipMemcpyDeviceToHost));
      py::dict pass;
      pass["pattern"] = kPatternNames[p];
      pass["mismatches"] = host.count;
      pass["records"] = mem_records(host);
      pass["fill_gbs"] = (double)bytes / 1e9 / (ev.ms(0, 1) / 1e3);
      pass["verify_gbs"] = (double)bytes / 1e9 / (ev.ms(1, 2) / 1e3);
      passes.append(pass);
      if (host.count) ok = false;
    }
  }

  KatTable t = make_kat_table(seed);
  DevBuf a(kKatFragBytes, t.a.data()), b(kKatFragBytes, t.b.data());
  DevBuf c(kKatFragBytes, t.c.data()), want(kKatFragBytes, t.want.data());
  int kat_blocks = 4 * prop.multiProcessorCount;
  KatReport kat;
  std::memset(&kat, 0, sizeof kat);
  DevBuf kat_report(sizeof kat, &kat);
  launch_mfma_kat(a.as<const bf16x8>(), b.as<const bf16x8>(),
                  c.as<const f32x4>(), want.as<const f32x4>(), kat_blocks,
                  kat_report.as<KatReport>());
  HIP_CHECK(hipMemcpy(&kat, kat_report.as<void>(), sizeof kat,
                      hipMemcpyDeviceToHost));
  if (kat.count) ok = false;
  py::dict mfma;
  mfma["blocks"] = kat_blocks;
  mfma["checked"] = (size_t)kat_blocks * 256 * 4;
  mfma["mismatches"] = kat.count;
  mfma["records"] = kat_records(kat);

  py::dict out;
  out["ok"] = ok;
  out["device"] = device;
  out["seed"] = seed;
  out["bytes"] = bytes;
  out["memory"] = passes;
  out["mfma"] = mfma;
  return out;
}

py::tuple memtest_probe(
    int device, long long nbytes, const std::string& pattern, u64 seed,
    int blocks, const std::vector<std::pair<long long, u64>>& flips,
    const std::string& stage) {
  int p = pattern_from_name(pattern);
  if (stage != "fill" && stage != "verify")
    throw std::invalid_argument("stage must be fill or verify, got '" + stage +
                                "'");
  probe_range("nbytes", nbytes, 0, kProbeMaxBytes);
  if (nbytes % (long long)sizeof(u64x2) != 0)
    throw std::invalid_argument("nbytes must be a multiple of 16");
  probe_range("blocks", blocks, 1, kProbeMaxBlocks);
  probe_range("len(flips)", (long long)flips.size(), 0, kMaxFlips);
  size_t n = (size_t)nbytes / sizeof(u64x2);
  std::vector<u64> flat;
  flat.reserve(2 * flips.size());
  for (const auto& f : flips) {
    if (f.first < 0 || (u64)f.first >= 2 * (u64)n)
      throw std::invalid_argument(
          "flip word index " + std::to_string(f.first) +
          " outside the region of " + std::to_string(2 * n) + " words");
    flat.push_back((u64)f.first);
    flat.push_back(f.second);
  }
  probe_device(device);

  GuardedBuf region((size_t)nbytes);
  MemReport host;
  std::memset(&host, 0, sizeof host);
  GuardedBuf report(sizeof host, &host);
  launch_mem_fill(p, blocks, region.payload<u64x2>(), n, seed);
  if (stage == "verify") {
    if (!flat.empty()) {
      DevBuf dflips(flat.size() * sizeof(u64), flat.data());
      hipLaunchKernelGGL(mem_xor, dim3(1), dim3(64), 0, 0,
                         region.payload<u64>(), dflips.as<const u64>(),
                         (int)flips.size());
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());  // dflips is freed here
    }
    launch_mem_verify(p, blocks, region.payload<const u64x2>(), n, seed,
                      report.payload<MemReport>());
  }
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(&host, report.payload<void>(), sizeof host,
                      hipMemcpyDeviceToHost));
  require_guards(report, "memtest_probe");
  return py::make_tuple(region.download(), host.count, mem_records(host));
}

py::tuple mfma_kat_probe(int device, const py::bytes& a_bytes,
                         const py::bytes& b_bytes, const py::bytes& c_bytes,
                         const py::bytes& want_bytes, int blocks) {
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
  probe_device(device);
  GuardedBuf da(a.size(), a.data(), kInputGuard);
  GuardedBuf db(b.size(), b.data(), kInputGuard);
  GuardedBuf dc(c.size(), c.data(), kInputGuard);
  GuardedBuf dw(want.size(), want.data(), kInputGuard);
  KatReport r;
  std::memset(&r, 0, sizeof r);
  GuardedBuf report(sizeof r, &r);
  launch_mfma_kat(da.payload<const bf16x8>(), db.payload<const bf16x8>(),
                  dc.payload<const f32x4>(), dw.payload<const f32x4>(), blocks,
                  report.payload<KatReport>());
  HIP_CHECK(hipMemcpy(&r, report.payload<void>(), sizeof r,
                      hipMemcpyDeviceToHost));
  require_guards(report, "mfma_kat_probe");
  return py::make_tuple(r.count, kat_records(r), (size_t)blocks * 256 * 4);
}

std::string pci_bus_id(int device) {
  int count = 0;
  HIP_CHECK(hipGetDeviceCount(&count));
  if (device < 0 || device >= count)
    throw std::invalid_argument("device " + std::to_string(device) +
                                " out of range (" + std::to_string(count) +
                                " visible)");
  char buf[64] = {0};
  HIP_CHECK(hipDeviceGetPCIBusId(buf, (int)sizeof buf, device));
  return std::string(buf);
}
