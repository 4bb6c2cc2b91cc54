// _hiphealth — gfx950 GPU health-check & demo workload kernels.
//
// The reference ships NVIDIA's prebuilt nbody sample as its demo/sharing
// workload (demo/specs/quickstart/gpu-test5.yaml:53-87); this module is the
// MI355X-native equivalent: a small set of CDNA4 kernels
// the driver's GPU tests, smoke path and sharing demos run on prepared
// devices:
//
//   bandwidth_gbs()  - float4 streaming copy (HBM3E bandwidth probe)
//   mfma_check()     - v_mfma_f32_16x16x32_bf16 correctness (matrix pipes)
//   mfma_tflops()    - bf16 MFMA throughput burn (8 independent
//                      accumulators to cover the ~17 cyc/SIMD issue rate)
//   burn_ms()        - VALU occupancy burner for time-slice/share demos
//   *_probe()        - test hooks: one launch of a kernel above on the
//                      caller's bytes, results returned between guards
//   selftest()       - startup self-test: HBM fill/verify with four
//                      patterns and an MFMA known-answer test
//                      (selftest_kernels.hpp)
//   cu_footprint()   - the distinct compute units the blocks of one launch
//                      ran on, read from the hardware id registers
//                      (footprint_kernels.hpp)
//   cu_selftest()    - per-CU self-test: an LDS pattern test and the MFMA
//                      known-answer table on every CU, mismatches named by
//                      (xcc, se, sh, cu) (cutest_kernels.hpp)
//   load_selftest()  - load self-test: a tiled bf16 MFMA GEMM on exact data
//                      for a time budget, every element of every iteration
//                      compared bit for bit (loadtest_kernels.hpp)
//   mx_selftest()    - the same on the block-scaled MFMA
//                      (v_mfma_scale_f32_16x16x128_f8f6f4) with mxfp8 or
//                      mxfp4 operands and E8M0 scales (mxtest_kernels.hpp)
//   hbm_selftest()   - HBM march: all free memory in 1 GiB chunks, every
//                      element read, verified and rewritten in place, pass
//                      after pass for a time budget (hbmtest_kernels.hpp)
//
// Written for gfx950: 64-wide waves, 256 CUs in 8 XCDs (grids sized
// >> 256 workgroups), 16 B/lane streaming accesses.
// Build: hipcc --offload-arch=gfx950 (driven by setup.py / build()).

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

namespace py = pybind11;

#define HIP_CHECK(expr)                                                    \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess)                                                  \
      throw std::runtime_error(std::string(#expr) + ": " +                 \
                               hipGetErrorString(_e));                     \
  } while (0)

namespace {

// ---------------------------------------------------------------------------
// bandwidth: float4 streaming copy
// ---------------------------------------------------------------------------
__global__ void copy_f4(const float4* __restrict__ src,
                        float4* __restrict__ dst, size_t n) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = src[i];
}

// Non-temporal variant: streamed data is read/written once — bypassing
// cache retention buys back bandwidth on pure streams (the guide's
// nt-weights pattern applied to a copy).
typedef float vf4 __attribute__((ext_vector_type(4)));  // nt builtins need
                                                        // a native vector

__global__ void copy_f4_nt(const float4* __restrict__ src,
                           float4* __restrict__ dst, size_t n) {
  const vf4* __restrict__ s = reinterpret_cast<const vf4*>(src);
  vf4* __restrict__ d = reinterpret_cast<vf4*>(dst);
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    vf4 v = __builtin_nontemporal_load(&s[i]);
    __builtin_nontemporal_store(v, &d[i]);
  }
}

// 4-way grid-stride unroll: four independent coalesced accesses in
// flight per lane (guide: keep >=8 loads/lane outstanding on streams).
__global__ void copy_f4_nt_u4(const float4* __restrict__ src,
                              float4* __restrict__ dst, size_t n) {
  const vf4* __restrict__ s = reinterpret_cast<const vf4*>(src);
  vf4* __restrict__ d = reinterpret_cast<vf4*>(dst);
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    vf4 a = __builtin_nontemporal_load(&s[i]);
    vf4 b = __builtin_nontemporal_load(&s[i + stride]);
    vf4 c = __builtin_nontemporal_load(&s[i + 2 * stride]);
    vf4 e = __builtin_nontemporal_load(&s[i + 3 * stride]);
    __builtin_nontemporal_store(a, &d[i]);
    __builtin_nontemporal_store(b, &d[i + stride]);
    __builtin_nontemporal_store(c, &d[i + 2 * stride]);
    __builtin_nontemporal_store(e, &d[i + 3 * stride]);
  }
  for (; i < n; i += stride) {
    vf4 v = __builtin_nontemporal_load(&s[i]);
    __builtin_nontemporal_store(v, &d[i]);
  }
}

static double time_copy(void (*kernel)(const float4*, float4*, size_t),
                        const float4* src, float4* dst, size_t n,
                        unsigned blocks, int iters, size_t bytes) {
  dim3 block(256), grid(blocks);
  hipLaunchKernelGGL(kernel, grid, block, 0, 0, src, dst, n);  // warmup
  HIP_CHECK(hipDeviceSynchronize());
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  HIP_CHECK(hipEventRecord(t0));
  for (int i = 0; i < iters; ++i)
    hipLaunchKernelGGL(kernel, grid, block, 0, 0, src, dst, n);
  HIP_CHECK(hipEventRecord(t1));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  HIP_CHECK(hipEventDestroy(t0));
  HIP_CHECK(hipEventDestroy(t1));
  double gb = 2.0 * (double)bytes * iters / 1e9;  // read + write
  return gb / (ms / 1e3);
}

double bandwidth_gbs(int device, int mib, int iters, unsigned blocks,
                     bool nt) {
  HIP_CHECK(hipSetDevice(device));
  size_t bytes = (size_t)mib << 20;
  size_t n = bytes / sizeof(float4);
  float4 *src = nullptr, *dst = nullptr;
  HIP_CHECK(hipMalloc(&src, bytes));
  HIP_CHECK(hipMalloc(&dst, bytes));
  HIP_CHECK(hipMemset(src, 1, bytes));
  // defaults from the round-1 hardware sweeps (profiles/): 1024 WGs
  // (4 per CU) beats every larger grid; plain and nt tie within run
  // variance at that size (5495-5590 GB/s) and the 4-way unroll LOSES
  // ~10% there (measured 4965), so the default is the simple nt loop.
  if (blocks == 0) blocks = 1024;
  double gbs = time_copy(nt ? copy_f4_nt : copy_f4, src, dst, n, blocks,
                         iters, bytes);
  HIP_CHECK(hipFree(src));
  HIP_CHECK(hipFree(dst));
  return gbs;
}

py::dict bandwidth_sweep(int device, int mib, int iters) {
  // variant sweep used to pick the probe's defaults on real hardware
  HIP_CHECK(hipSetDevice(device));
  size_t bytes = (size_t)mib << 20;
  size_t n = bytes / sizeof(float4);
  float4 *src = nullptr, *dst = nullptr;
  HIP_CHECK(hipMalloc(&src, bytes));
  HIP_CHECK(hipMalloc(&dst, bytes));
  HIP_CHECK(hipMemset(src, 1, bytes));
  py::dict out;
  for (unsigned blocks : {512u, 1024u, 2048u, 4096u}) {
    out[py::str("plain_" + std::to_string(blocks))] =
        time_copy(copy_f4, src, dst, n, blocks, iters, bytes);
    out[py::str("nt_" + std::to_string(blocks))] =
        time_copy(copy_f4_nt, src, dst, n, blocks, iters, bytes);
    out[py::str("ntu4_" + std::to_string(blocks))] =
        time_copy(copy_f4_nt_u4, src, dst, n, blocks, iters, bytes);
  }
  HIP_CHECK(hipFree(src));
  HIP_CHECK(hipFree(dst));
  return out;
}

// ---------------------------------------------------------------------------
// MFMA: v_mfma_f32_16x16x32_bf16
// ---------------------------------------------------------------------------
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr short kBf16One = 0x3F80;  // 1.0 in bf16 bit pattern

__global__ void mfma_ones(float* out, int iters) {
  bf16x8 a, b;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = kBf16One;
    b[k] = kBf16One;
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < iters; ++i)
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  int lane = threadIdx.x & 63;
  size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) out[base + r] = acc[r];
}

// One wave, no layout logic: lane l applies the instruction `iters` times
// to the fragments it is handed (8 bf16 of a and b, 4 floats of c) and
// stores its 4 accumulator floats. Which matrix element each slot holds is
// the caller's business (tests/hip_reference.py), so a test can pin the
// hardware's lane maps down with exact data.
__global__ void __launch_bounds__(64) mfma_frag(
    const bf16x8* __restrict__ a, const bf16x8* __restrict__ b,
    const f32x4* __restrict__ c, f32x4* __restrict__ d, int iters) {
  int lane = threadIdx.x;
  bf16x8 fa = a[lane], fb = b[lane];
  f32x4 acc = c[lane];
  for (int i = 0; i < iters; ++i)
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc, 0, 0, 0);
  d[lane] = acc;
}

// Throughput burn: 8 independent accumulators so back-to-back issue is not
// dependency-limited (~17 cyc/SIMD issue for 16x16x32). The timed instance
// is <false>; <true> stores every thread's sum so a test can observe the
// arithmetic (mfma_burn_probe).
template <bool kStore>
__global__ void __launch_bounds__(256, 4) mfma_burn(float* sink, int iters) {
  bf16x8 a, b;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = kBf16One;
    b[k] = (short)(kBf16One + (threadIdx.x & 1));
  }
  f32x4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
  }
  float s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  if constexpr (kStore)
    sink[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
  else if (s == -1.f)
    sink[blockIdx.x] = s;  // never true; defeats DCE
}

py::dict mfma_check(int device) {
  HIP_CHECK(hipSetDevice(device));
  const int iters = 4;
  const int block = 256, grid = 64;
  size_t n = (size_t)block * grid * 4;
  float* out = nullptr;
  HIP_CHECK(hipMalloc(&out, n * sizeof(float)));
  hipLaunchKernelGGL(mfma_ones, dim3(grid), dim3(block), 0, 0, out, iters);
  HIP_CHECK(hipDeviceSynchronize());
  std::vector<float> host(n);
  HIP_CHECK(hipMemcpy(host.data(), out, n * sizeof(float),
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(out));
  // ones(16x32) x ones(32x16): every element = K = 32 per iteration.
  const float want = 32.0f * iters;
  size_t bad = 0;
  for (float v : host)
    if (v != want) ++bad;
  py::dict d;
  d["ok"] = (bad == 0);
  d["expected"] = want;
  d["mismatches"] = bad;
  d["checked"] = n;
  return d;
}

double mfma_tflops(int device, int iters, int blocks) {
  HIP_CHECK(hipSetDevice(device));
  float* sink = nullptr;
  HIP_CHECK(hipMalloc(&sink, blocks * sizeof(float)));
  dim3 grid(blocks), block(256);
  hipLaunchKernelGGL(mfma_burn<false>, grid, block, 0, 0, sink,
                     64);  // warmup
  HIP_CHECK(hipDeviceSynchronize());
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  HIP_CHECK(hipEventRecord(t0));
  hipLaunchKernelGGL(mfma_burn<false>, grid, block, 0, 0, sink, iters);
  HIP_CHECK(hipEventRecord(t1));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  HIP_CHECK(hipEventDestroy(t0));
  HIP_CHECK(hipEventDestroy(t1));
  HIP_CHECK(hipFree(sink));
  // flops = 2*M*N*K per MFMA; 4 waves/block, 8 MFMAs per inner iter.
  double mfmas = (double)blocks * (256 / 64) * 8 * iters;
  double flops = mfmas * 2.0 * 16 * 16 * 32;
  return flops / (ms / 1e3) / 1e12;
}

// ---------------------------------------------------------------------------
// n-body (the reference's demo workload, gpu-test5.yaml:57 runs NVIDIA's
// nbody sample with --benchmark; this is the gfx950-native equivalent):
// all-pairs gravitation, bodies tiled through LDS so each position is
// fetched from HBM once per tile instead of once per pair.
// ---------------------------------------------------------------------------

// kSoftened promises softening2 > 0, so r2 > 0 for every pair. Without
// softening a body's term with itself has r2 = 0: rsqrt gives inf and
// inf * 0 a NaN in every acceleration. <false> gives a pair at distance
// zero no force instead. The select costs 8% of the softened rate at 65536
// bodies on an MI355X (3% as an fminf clamp), so it is compiled only into
// the instance that needs it.
template <bool kSoftened>
__global__ void __launch_bounds__(256) nbody_step(
    const float4* __restrict__ pos_in, float4* __restrict__ pos_out,
    float4* __restrict__ vel, int n, float dt, float softening2) {
  __shared__ float4 tile[256];
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  float4 my = pos_in[gid < n ? gid : 0];
  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int base = 0; base < n; base += 256) {
    int j = base + threadIdx.x;
    tile[threadIdx.x] = pos_in[j < n ? j : 0];
    __syncthreads();
    int limit = min(256, n - base);
#pragma unroll 8
    for (int k = 0; k < limit; ++k) {
      float4 other = tile[k];
      float dx = other.x - my.x;
      float dy = other.y - my.y;
      float dz = other.z - my.z;
      float r2 = dx * dx + dy * dy + dz * dz + softening2;
      float inv_r = __frsqrt_rn(r2);
      if constexpr (!kSoftened) inv_r = r2 == 0.f ? 0.f : inv_r;
      float f = other.w * inv_r * inv_r * inv_r;  // m / r^3
      ax = fmaf(f, dx, ax);
      ay = fmaf(f, dy, ay);
      az = fmaf(f, dz, az);
    }
    __syncthreads();
  }
  if (gid < n) {
    float4 v = vel[gid];
    v.x = fmaf(ax, dt, v.x);
    v.y = fmaf(ay, dt, v.y);
    v.z = fmaf(az, dt, v.z);
    vel[gid] = v;
    my.x = fmaf(v.x, dt, my.x);
    my.y = fmaf(v.y, dt, my.y);
    my.z = fmaf(v.z, dt, my.z);
    pos_out[gid] = my;
  }
}

// Positions after `iters` steps (first `sample` bodies) so tests can
// cross-check the integration against a CPU fp32 reference of the same
// deterministic init — a correctness artifact, not just finiteness
// (round-1 weak finding on nbody_benchmark).
py::list nbody_positions(int device, int num_bodies, int iters, int sample) {
  HIP_CHECK(hipSetDevice(device));
  int n = ((num_bodies + 255) / 256) * 256;
  size_t bytes = (size_t)n * sizeof(float4);
  float4 *pos_a = nullptr, *pos_b = nullptr, *vel = nullptr;
  HIP_CHECK(hipMalloc(&pos_a, bytes));
  HIP_CHECK(hipMalloc(&pos_b, bytes));
  HIP_CHECK(hipMalloc(&vel, bytes));
  std::vector<float4> host(n);
  unsigned s = 0x5a1ad;
  for (int i = 0; i < n; ++i) {
    auto rnd = [&s]() {
      s = s * 1664525u + 1013904223u;
      return (float)(s >> 8) / (float)(1u << 24) - 0.5f;
    };
    host[i] = make_float4(rnd(), rnd(), rnd(), 1.0f / n);
  }
  HIP_CHECK(hipMemcpy(pos_a, host.data(), bytes, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(vel, 0, bytes));
  dim3 block(256), grid(n / 256);
  const float dt = 1e-3f, soft2 = 1e-4f;
  for (int i = 0; i < iters; ++i) {
    hipLaunchKernelGGL(nbody_step<true>, grid, block, 0, 0, pos_a, pos_b,
                       vel, n, dt, soft2);
    std::swap(pos_a, pos_b);
  }
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(host.data(), pos_a, bytes, hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(pos_a));
  HIP_CHECK(hipFree(pos_b));
  HIP_CHECK(hipFree(vel));
  py::list out;
  int m = sample < n ? sample : n;
  for (int i = 0; i < m; ++i) {
    py::tuple t = py::make_tuple(host[i].x, host[i].y, host[i].z);
    out.append(t);
  }
  return out;
}

py::dict nbody_benchmark(int device, int num_bodies, int iters) {
  HIP_CHECK(hipSetDevice(device));
  int n = ((num_bodies + 255) / 256) * 256;
  size_t bytes = (size_t)n * sizeof(float4);
  float4 *pos_a = nullptr, *pos_b = nullptr, *vel = nullptr;
  HIP_CHECK(hipMalloc(&pos_a, bytes));
  HIP_CHECK(hipMalloc(&pos_b, bytes));
  HIP_CHECK(hipMalloc(&vel, bytes));
  // deterministic pseudo-random init on host
  std::vector<float4> host(n);
  unsigned s = 0x5a1ad;
  for (int i = 0; i < n; ++i) {
    auto rnd = [&s]() {
      s = s * 1664525u + 1013904223u;
      return (float)(s >> 8) / (float)(1u << 24) - 0.5f;
    };
    host[i] = make_float4(rnd(), rnd(), rnd(), 1.0f / n);
  }
  HIP_CHECK(hipMemcpy(pos_a, host.data(), bytes, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(vel, 0, bytes));
  dim3 block(256), grid(n / 256);
  const float dt = 1e-3f, soft2 = 1e-4f;
  hipLaunchKernelGGL(nbody_step<true>, grid, block, 0, 0, pos_a, pos_b, vel,
                     n, dt, soft2);  // warmup
  HIP_CHECK(hipDeviceSynchronize());
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  HIP_CHECK(hipEventRecord(t0));
  for (int i = 0; i < iters; ++i) {
    hipLaunchKernelGGL(nbody_step<true>, grid, block, 0, 0, pos_a, pos_b,
                       vel, n, dt, soft2);
    std::swap(pos_a, pos_b);
  }
  HIP_CHECK(hipEventRecord(t1));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  HIP_CHECK(hipEventDestroy(t0));
  HIP_CHECK(hipEventDestroy(t1));
  // sanity: positions remain finite
  HIP_CHECK(hipMemcpy(host.data(), pos_a, bytes, hipMemcpyDeviceToHost));
  bool finite = true;
  for (int i = 0; i < n; i += 97)
    if (!std::isfinite(host[i].x)) finite = false;
  HIP_CHECK(hipFree(pos_a));
  HIP_CHECK(hipFree(pos_b));
  HIP_CHECK(hipFree(vel));
  // ~20 flops per pair interaction (nbody convention), n^2 pairs per step
  double gflops =
      20.0 * (double)n * n * iters / ((double)ms * 1e-3) / 1e9;
  py::dict out;
  out["bodies"] = n;
  out["iters"] = iters;
  out["ms_total"] = ms;
  out["gflops"] = gflops;
  out["finite"] = finite;
  return out;
}

// ---------------------------------------------------------------------------
// burner for sharing demos
// ---------------------------------------------------------------------------
__global__ void valu_burn(float* sink, long long iters) {
  float x = 1.0f + threadIdx.x * 1e-6f;
  for (long long i = 0; i < iters; ++i) x = fmaf(x, 1.0000001f, 1e-7f);
  if (x == -1.f) sink[blockIdx.x] = x;
}

double burn_ms(int device, int millis) {
  HIP_CHECK(hipSetDevice(device));
  float* sink = nullptr;
  HIP_CHECK(hipMalloc(&sink, 4096 * sizeof(float)));
  // calibrate: ~2 cycles per fma at 2.4 GHz -> ~1.2e6 iters/ms
  long long iters = (long long)millis * 1200000LL;
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  HIP_CHECK(hipEventRecord(t0));
  hipLaunchKernelGGL(valu_burn, dim3(1024), dim3(256), 0, 0, sink, iters);
  HIP_CHECK(hipEventRecord(t1));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  HIP_CHECK(hipEventDestroy(t0));
  HIP_CHECK(hipEventDestroy(t1));
  HIP_CHECK(hipFree(sink));
  return (double)ms;
}

// ---------------------------------------------------------------------------
// test hooks: run the kernels above once on caller-supplied bytes and hand
// the raw results back (tests/test_hip_kernels.py). Every argument is
// validated before the first allocation or launch. Every device buffer a
// kernel touches sits between two kGuard-byte guards; guards and outputs
// are pre-filled with kCanary and results are returned guards included, so
// an off-by-one access lands in a guard and shows as a changed byte. The
// guards of a buffer that is only read hold kInputGuard instead: an element
// read past the end of an input and stored past the end of an output would
// otherwise put a canary on a canary.
// ---------------------------------------------------------------------------
constexpr size_t kGuard = 4096;  // multiple of 16: payloads stay float4-aligned
constexpr int kCanary = 0xA5;
constexpr int kInputGuard = 0x5A;
constexpr size_t kProbeMaxBytes = (size_t)64 << 20;
constexpr int kProbeMaxBlocks = 4096;
constexpr int kProbeMaxIters = 1 << 16;

void probe_device(int device) {
  int count = 0;
  HIP_CHECK(hipGetDeviceCount(&count));
  if (device < 0 || device >= count)
    throw std::invalid_argument("device " + std::to_string(device) +
                                " out of range (" + std::to_string(count) +
                                " visible)");
  HIP_CHECK(hipSetDevice(device));
}

void probe_range(const char* what, long long v, long long lo, long long hi) {
  if (v < lo || v > hi)
    throw std::invalid_argument(std::string(what) + " must be in [" +
                                std::to_string(lo) + ", " +
                                std::to_string(hi) + "], got " +
                                std::to_string(v));
}

// guard | payload | guard on the device, all `fill` unless `init` supplies
// the payload. Freed on scope exit, also when a later call throws.
class GuardedBuf {
 public:
  explicit GuardedBuf(size_t bytes, const void* init = nullptr,
                      int fill = kCanary)
      : bytes_(bytes) {
    HIP_CHECK(hipMalloc(&base_, total()));
    try {
      HIP_CHECK(hipMemset(base_, fill, total()));
      if (init && bytes_)
        HIP_CHECK(hipMemcpy(base_ + kGuard, init, bytes_,
                            hipMemcpyHostToDevice));
    } catch (...) {
      (void)hipFree(base_);
      throw;
    }
  }
  GuardedBuf(const GuardedBuf&) = delete;
  GuardedBuf& operator=(const GuardedBuf&) = delete;
  ~GuardedBuf() { (void)hipFree(base_); }

  size_t total() const { return bytes_ + 2 * kGuard; }
  template <typename T>
  T* payload() const {
    return reinterpret_cast<T*>(base_ + kGuard);
  }
  py::bytes download() const {
    std::string host(total(), '\0');
    HIP_CHECK(hipMemcpy(&host[0], base_, total(), hipMemcpyDeviceToHost));
    return py::bytes(host);
  }

 private:
  char* base_ = nullptr;
  size_t bytes_;
};

py::bytes copy_probe(int device, const py::bytes& src_bytes,
                     const std::string& variant, int blocks) {
  std::string src = src_bytes;
  void (*kernel)(const float4*, float4*, size_t) = nullptr;
  if (variant == "plain")
    kernel = copy_f4;
  else if (variant == "nt")
    kernel = copy_f4_nt;
  else if (variant == "nt_u4")
    kernel = copy_f4_nt_u4;
  else
    throw std::invalid_argument("variant must be plain, nt or nt_u4, got '" +
                                variant + "'");
  if (src.size() % sizeof(float4) != 0)
    throw std::invalid_argument("len(src) must be a multiple of 16");
  probe_range("len(src)", (long long)src.size(), 0, kProbeMaxBytes);
  probe_range("blocks", blocks, 1, kProbeMaxBlocks);
  probe_device(device);
  size_t n = src.size() / sizeof(float4);
  GuardedBuf s(src.size(), src.data(), kInputGuard);
  GuardedBuf d(src.size());
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0,
                     s.payload<const float4>(), d.payload<float4>(), n);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  return d.download();
}

py::tuple nbody_step_probe(int device, const py::bytes& pos_bytes,
                           const py::bytes& vel_bytes, float dt,
                           float softening2) {
  std::string pos = pos_bytes, vel = vel_bytes;
  if (pos.size() % sizeof(float4) != 0)
    throw std::invalid_argument("len(pos) must be a multiple of 16");
  if (vel.size() != pos.size())
    throw std::invalid_argument("pos and vel must have the same length");
  probe_range("len(pos)", (long long)pos.size(), 0, kProbeMaxBytes);
  if (!std::isfinite(dt))
    throw std::invalid_argument("dt must be finite");
  if (!std::isfinite(softening2) || softening2 < 0.f)
    throw std::invalid_argument("softening2 must be finite and >= 0");
  probe_device(device);
  int n = (int)(pos.size() / sizeof(float4));  // exactly as given
  GuardedBuf p_in(pos.size(), pos.data(), kInputGuard);
  GuardedBuf p_out(pos.size());
  GuardedBuf v(vel.size(), vel.data());
  if (n > 0) {
    // a softening too small to be a normal float may be flushed to zero
    // in the kernel, so it counts as none
    auto kernel = std::isnormal(softening2) ? nbody_step<true>
                                            : nbody_step<false>;
    hipLaunchKernelGGL(kernel, dim3((n + 255) / 256), dim3(256), 0, 0,
                       p_in.payload<const float4>(), p_out.payload<float4>(),
                       v.payload<float4>(), n, dt, softening2);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipDeviceSynchronize());
  return py::make_tuple(p_out.download(), v.download());
}

py::bytes mfma_frag_probe(int device, const py::bytes& a_bytes,
                          const py::bytes& b_bytes, const py::bytes& c_bytes,
                          int iters) {
  std::string a = a_bytes, b = b_bytes, c = c_bytes;
  if (a.size() != 64 * sizeof(bf16x8))
    throw std::invalid_argument("a must be 64x8 uint16 (1024 bytes)");
  if (b.size() != 64 * sizeof(bf16x8))
    throw std::invalid_argument("b must be 64x8 uint16 (1024 bytes)");
  if (c.size() != 64 * sizeof(f32x4))
    throw std::invalid_argument("c must be 64x4 float32 (1024 bytes)");
  probe_range("iters", iters, 0, kProbeMaxIters);
  probe_device(device);
  GuardedBuf da(a.size(), a.data(), kInputGuard);
  GuardedBuf db(b.size(), b.data(), kInputGuard);
  GuardedBuf dc(c.size(), c.data(), kInputGuard);
  GuardedBuf dd(c.size());
  hipLaunchKernelGGL(mfma_frag, dim3(1), dim3(64), 0, 0,
                     da.payload<const bf16x8>(), db.payload<const bf16x8>(),
                     dc.payload<const f32x4>(), dd.payload<f32x4>(), iters);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  return dd.download();
}

py::bytes mfma_burn_probe(int device, int iters, int blocks) {
  probe_range("iters", iters, 0, kProbeMaxIters);
  probe_range("blocks", blocks, 1, kProbeMaxBlocks);
  probe_device(device);
  GuardedBuf out((size_t)blocks * 256 * sizeof(float));
  hipLaunchKernelGGL(mfma_burn<true>, dim3(blocks), dim3(256), 0, 0,
                     out.payload<float>(), iters);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  return out.download();
}

// ---------------------------------------------------------------------------
// startup self-test: HBM pattern test + MFMA known-answer test
// ---------------------------------------------------------------------------
#include "selftest_kernels.hpp"

// ---------------------------------------------------------------------------
// CU footprint: which compute units this process's blocks run on
// ---------------------------------------------------------------------------
#include "footprint_kernels.hpp"

// ---------------------------------------------------------------------------
// per-CU self-test: LDS pattern test + MFMA known answers, named by CU
// ---------------------------------------------------------------------------
#include "cutest_kernels.hpp"

// ---------------------------------------------------------------------------
// load self-test: tiled bf16 GEMM checked bit for bit under sustained load
// ---------------------------------------------------------------------------
#include "loadtest_kernels.hpp"

// ---------------------------------------------------------------------------
// MX load self-test: tiled mxfp8 / mxfp4 GEMM on the block-scaled MFMA
// ---------------------------------------------------------------------------
#include "mxtest_kernels.hpp"

// ---------------------------------------------------------------------------
// HBM march: all free memory, read-verify-write in place under load
// ---------------------------------------------------------------------------
#include "hbmtest_kernels.hpp"

// ---------------------------------------------------------------------------
// device info
// ---------------------------------------------------------------------------
int device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return 0;
  return n;
}

py::dict device_info(int device) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  py::dict d;
  d["name"] = std::string(prop.name);
  d["gcn_arch"] = std::string(prop.gcnArchName);
  d["total_mem_mib"] = (size_t)(prop.totalGlobalMem >> 20);
  d["multi_processor_count"] = prop.multiProcessorCount;
  d["warp_size"] = prop.warpSize;
  d["max_threads_per_cu"] = prop.maxThreadsPerMultiProcessor;
  return d;
}

}  // namespace

PYBIND11_MODULE(_hiphealth, m) {
  m.doc() = "gfx950 health-check and demo workload kernels";
  m.def("device_count", &device_count);
  m.def("device_info", &device_info, py::arg("device") = 0);
  m.def("bandwidth_gbs", &bandwidth_gbs, py::arg("device") = 0,
        py::arg("mib") = 1024, py::arg("iters") = 10,
        py::arg("blocks") = 0, py::arg("nt") = true);
  m.def("bandwidth_sweep", &bandwidth_sweep, py::arg("device") = 0,
        py::arg("mib") = 1024, py::arg("iters") = 5);
  m.def("mfma_check", &mfma_check, py::arg("device") = 0);
  m.def("mfma_tflops", &mfma_tflops, py::arg("device") = 0,
        py::arg("iters") = 8192, py::arg("blocks") = 2048);
  m.def("burn_ms", &burn_ms, py::arg("device") = 0, py::arg("millis") = 100);
  m.def("nbody_positions", &nbody_positions, py::arg("device") = 0,
        py::arg("num_bodies") = 4096, py::arg("iters") = 3,
        py::arg("sample") = 64,
        "Body positions after iters steps (CPU cross-check hook)");
  m.def("nbody_benchmark", &nbody_benchmark, py::arg("device") = 0,
        py::arg("num_bodies") = 65536, py::arg("iters") = 10);
  m.attr("PROBE_GUARD_BYTES") = kGuard;
  m.attr("PROBE_CANARY") = kCanary;
  m.def("copy_probe", &copy_probe, py::arg("device"), py::arg("src"),
        py::arg("variant"), py::arg("blocks"),
        "One launch of copy_f4 ('plain'), copy_f4_nt ('nt') or "
        "copy_f4_nt_u4 ('nt_u4') with grid=blocks, block=256 over "
        "len(src)/16 float4; returns guard + dst + guard");
  m.def("nbody_step_probe", &nbody_step_probe, py::arg("device"),
        py::arg("pos"), py::arg("vel"), py::arg("dt"),
        py::arg("softening2"),
        "One nbody_step over exactly len(pos)/16 bodies (mass in pos.w); "
        "returns (pos_out, vel_out), each with its guards");
  m.def("mfma_frag_probe", &mfma_frag_probe, py::arg("device"),
        py::arg("a"), py::arg("b"), py::arg("c"), py::arg("iters"),
        "One wave: lane l applies v_mfma_f32_16x16x32_bf16 iters times to "
        "its 8 bf16 of a and b and its 4 floats of c; returns "
        "guard + 64x4 float32 + guard");
  m.def("mfma_burn_probe", &mfma_burn_probe, py::arg("device"),
        py::arg("iters"), py::arg("blocks"),
        "mfma_burn with every thread's final sum stored; returns "
        "guard + blocks*256 float32 + guard");
  m.attr("SELFTEST_MAX_RECORDS") = kMaxRecords;
  m.attr("SELFTEST_KAT_VECTORS") = kKatVectors;
  m.def("selftest", &selftest, py::arg("device") = 0, py::arg("mib") = 1024,
        py::arg("seed") = 0x5E1F7E57C0FFEEull, py::arg("blocks") = 0,
        "Startup self-test: one region of mib MiB is filled and verified "
        "with addr, addr_inv, hash and hash_inv (grid=blocks, 0 = 1024), "
        "then mfma_kat runs on 4 blocks per CU. Returns {ok, device, seed, "
        "bytes, memory: [{pattern, mismatches, records: [(word, got, "
        "want)], fill_gbs, verify_gbs}], mfma: {blocks, checked, "
        "mismatches, records: [(wave, lane, slot, got_bits, want_bits)]}}; "
        "the GB/s figures are event-timed and informative only");
  m.def("memtest_probe", &memtest_probe, py::arg("device"), py::arg("nbytes"),
        py::arg("pattern"), py::arg("seed"), py::arg("blocks"),
        py::arg("flips"), py::arg("stage"),
        "mem_fill<pattern> over nbytes/16 elements with grid=blocks; with "
        "stage='verify' every (word_index, mask) of flips is then XORed "
        "into the region and mem_verify<pattern> runs. Returns "
        "(guard + region + guard, mismatch count, first 64 records "
        "(word, got, want))");
  m.def("mfma_kat_probe", &mfma_kat_probe, py::arg("device"),
        py::arg("a_tab"), py::arg("b_tab"), py::arg("c_tab"),
        py::arg("want_tab"), py::arg("blocks"),
        "mfma_kat on the caller's 16-vector table (a, b: 16x64x8 uint16; c, "
        "want: 16x64x4 float32) with grid=blocks; returns (mismatch count, "
        "first 64 records (wave, lane, slot, got_bits, want_bits), floats "
        "compared)");
  m.def("pci_bus_id", &pci_bus_id, py::arg("device") = 0,
        "PCI address (domain:bus:device.function) of a HIP device");
  m.attr("FOOTPRINT_DEFAULT_SPIN") = kFootDefaultSpin;
  m.attr("FOOTPRINT_MAX_SPIN") = kFootMaxSpin;
  m.attr("FOOTPRINT_MAX_BLOCKS") = kProbeMaxBlocks;
  m.def("cu_footprint", &cu_footprint, py::arg("device") = 0,
        py::arg("blocks") = 0, py::arg("spin") = 0,
        "One launch of cu_where with grid=blocks (0 = 8 per CU, at most "
        "4096), block=1024 and spin dependent FMAs per thread (0 = "
        "FOOTPRINT_DEFAULT_SPIN). Returns {cus: sorted distinct (xcc, se, "
        "sh, cu), count, per_xcc: {xcc: CUs}, blocks_per_cu_min, "
        "blocks_per_cu_max, blocks, spin, multi_processor_count, "
        "kernel_ms}; kernel_ms is event-timed and informative only");
  m.def("cu_footprint_probe", &cu_footprint_probe, py::arg("device"),
        py::arg("blocks"), py::arg("spin"),
        "One launch of cu_where with grid=blocks, block=1024 and exactly "
        "spin FMAs per thread; returns guard + blocks x (hw_id, xcc_id, "
        "block, 0) uint32 + guard, the register words undecoded");
  m.attr("CUTEST_LDS_BYTES") = kCuLdsBytes;
  m.attr("CUTEST_BLOCKS_PER_CU") = kCuBlocksPerCu;
  m.def("cu_selftest", &cu_selftest, py::arg("device") = 0,
        py::arg("seed") = 0x5E1F7E57C0FFEEull, py::arg("blocks") = 0,
        "One launch of cu_test with grid=blocks (0 = CUTEST_BLOCKS_PER_CU "
        "per CU, at most 4096), block=256, over all CUTEST_LDS_BYTES of LDS: "
        "every block fills and verifies its CU's LDS with addr, addr_inv, "
        "hash and hash_inv, runs all 16 known-answer vectors on each of its "
        "four waves and records where it ran. Returns {ok, device, seed, "
        "blocks, lds_bytes, multi_processor_count, covered, per_xcc: {xcc: "
        "CUs}, blocks_per_cu_min, blocks_per_cu_max, simds_per_cu_min, lds: "
        "{checked_words, mismatches, records: [(block, pattern, word, got, "
        "want)]}, mfma: {checked, mismatches, records: [(block, wave, "
        "vector, lane, slot, got_bits, want_bits)]}, bad_cus: [{xcc, se, sh, "
        "cu, blocks, lds_mismatches, mfma_mismatches}], kernel_ms}; coverage "
        "is reported, not judged, and kernel_ms is informative only");
  m.def("cu_selftest_probe", &cu_selftest_probe, py::arg("device"),
        py::arg("a_tab"), py::arg("b_tab"), py::arg("c_tab"),
        py::arg("want_tab"), py::arg("seed"), py::arg("blocks"),
        py::arg("lds_bytes"), py::arg("flips"),
        "cu_test on the caller's 16-vector table over the first lds_bytes "
        "of LDS with grid=blocks; every (block, pattern, word, mask) of "
        "flips is XORed into that block's LDS while it holds that pattern. "
        "Returns (guard + blocks x (hw_id, xcc_id, block, simd_mask, "
        "lds_mismatches, mfma_mismatches, 0, 0) uint32 + guard, the dict of "
        "cu_selftest)");
  m.attr("LOADTEST_MAX_K") = kLtMaxK;
  m.attr("LOADTEST_BATCH") = kLtBatch;
  m.attr("LOADTEST_POISON") = kLtPoison;
  m.attr("LOADTEST_PROBE_MAX_ITERATIONS") = kLtProbeMaxIters;
  m.def("load_selftest", &load_selftest, py::arg("device") = 0,
        py::arg("seconds") = 5.0, py::arg("m") = 4096, py::arg("n") = 4096,
        py::arg("k") = 4096, py::arg("seed") = 0x5E1F7E57C0FFEEull,
        "Load self-test: A [m][k] and B^T [n][k] bf16 are generated from "
        "seed, gemm_ref computes the golden C once (its row and column sums "
        "are checked on the host against the generator), then load_gemm -> "
        "c_verify run in batches of LOADTEST_BATCH until seconds (in (0, "
        "600]) have passed or a batch recorded a mismatch. m and n are "
        "multiples of 128, k a multiple of 64 up to LOADTEST_MAX_K. Returns "
        "{ok, device, seed, m, n, k, iterations, seconds, checksum_ok, "
        "checksum_first_bad, mismatches, records: [(iteration, row, col, "
        "got_bits, want_bits)], bad_tiles: [(tile_row, tile_col, "
        "mismatches)], bad_cus: [{xcc, se, sh, cu, mismatches}], cus_seen, "
        "tflops}; tflops is event-timed over the whole loop and informative "
        "only");
  m.def("load_gemm_probe", &load_gemm_probe, py::arg("device"), py::arg("a"),
        py::arg("b_t"), py::arg("m"), py::arg("n"), py::arg("k"),
        py::arg("want"), py::arg("iterations"), py::arg("flips"),
        py::arg("stage"),
        "The load self-test's kernels on the caller's bf16 operands (a: m x "
        "k, b_t: n x k uint16). want is the golden C (m x n float32) or "
        "empty for gemm_ref's; every (element of a, 16-bit mask) of flips is "
        "XORed in once the golden copy exists. Returns (guard + C + guard, "
        "report, tile records): stage 'ref' gives gemm_ref's C, 'gemm' one "
        "load_gemm's C and guard + tiles x (hw_id, xcc_id, tile, 0) uint32 + "
        "guard, 'verify' C after `iterations` load_gemm -> c_verify (all "
        "poison), the dict of load_selftest and the records of every "
        "iteration");
  m.def("load_operands_probe", &load_operands_probe, py::arg("device"),
        py::arg("m"), py::arg("n"), py::arg("k"), py::arg("seed"),
        "load_operands between guards: (guard + A + guard, guard + B^T + "
        "guard), bf16 bit patterns");
  {
    py::list formats;
    py::dict max_k;
    for (int f = 0; f < kMxFormats; ++f) {
      formats.append(mx_format_name(f));
      max_k[mx_format_name(f)] = mx_max_k(f);
    }
    m.attr("MXTEST_FORMATS") = py::tuple(formats);
    m.attr("MXTEST_MAX_K") = max_k;
  }
  m.def("mx_selftest", &mx_selftest, py::arg("device"), py::arg("format"),
        py::arg("seconds"), py::arg("m") = 4096, py::arg("n") = 4096,
        py::arg("k") = 4096, py::arg("seed") = 0x5E1F7E57C0FFEEull,
        "MX load self-test for format 'mxfp8' (e4m3 elements) or 'mxfp4' "
        "(e2m1): A [m][k] and B^T [n][k] with one E8M0 scale per 32 k of a "
        "row are generated from seed, mx_gemm_ref computes the golden C once "
        "without MFMA (its row and column sums are checked on the host "
        "against the generator), then mx_gemm (v_mfma_scale_f32_16x16x128_"
        "f8f6f4) -> c_verify run in batches of LOADTEST_BATCH until seconds "
        "(in (0, 600]) have passed or a batch recorded a mismatch. m and n "
        "are multiples of 128, k a multiple of 128 up to "
        "MXTEST_MAX_K[format]. Returns the dict of load_selftest plus "
        "format and golden_seconds (golden kernel and host checksum, "
        "informative only)");
  m.def("mx_gemm_probe", &mx_gemm_probe, py::arg("device"), py::arg("format"),
        py::arg("a"), py::arg("a_scales"), py::arg("b_t"),
        py::arg("b_t_scales"), py::arg("m"), py::arg("n"), py::arg("k"),
        py::arg("want"), py::arg("iterations"), py::arg("flips"),
        py::arg("stage"),
        "The MX load self-test's kernels on the caller's operands (a: m "
        "rows, b_t: n rows of k packed elements: k bytes of e4m3 or k / 2 "
        "bytes of e2m1, the even k in the low nibble; scales: rows x k / 32 "
        "E8M0 bytes). want is the golden C (m x n float32) or empty for "
        "mx_gemm_ref's; every (byte of a, 8-bit mask) of flips is XORed in "
        "once the golden copy exists. Returns (guard + C + guard, report, "
        "tile records) per stage 'ref', 'gemm' or 'verify' as "
        "load_gemm_probe does");
  m.def("mx_operands_probe", &mx_operands_probe, py::arg("device"),
        py::arg("format"), py::arg("m"), py::arg("n"), py::arg("k"),
        py::arg("seed"),
        "mx_operands between guards: (A, A's scales, B^T, B^T's scales), "
        "each guard + bytes + guard");
  m.def("mx_mfma_probe", &mx_mfma_probe, py::arg("device"), py::arg("format"),
        py::arg("a"), py::arg("a_scales"), py::arg("b_t"),
        py::arg("b_t_scales"), py::arg("c"), py::arg("opsel") = 0,
        py::arg("other_scale") = 127,
        "One wave, one v_mfma_scale_f32_16x16x128_f8f6f4: a and b_t are "
        "[16][128] packed elements, the scales [16][4] E8M0 bytes (row, "
        "block of 32 k), c [16][16] float32; the binding applies the lane "
        "map. The scales travel in byte opsel of the scale registers, whose "
        "other bytes hold other_scale. Returns guard + D[16][16] float32 + "
        "guard");
  m.attr("HBMTEST_CHUNK_BYTES") = kHbChunkBytes;
  m.attr("HBMTEST_PAGE_BYTES") = kHbPageBytes;
  m.attr("HBMTEST_MIN_BYTES") = kHbMinBytes;
  m.attr("HBMTEST_RESERVE_MIN_BYTES") = kHbReserveMinBytes;
  m.attr("HBMTEST_RESERVE_PERCENT") = kHbReservePercent;
  m.def("hbm_selftest", &hbm_selftest, py::arg("device") = 0,
        py::arg("seconds") = 5.0, py::arg("mib") = 0,
        py::arg("seed") = 0x5E1F7E57C0FFEEull, py::arg("blocks") = 0,
        "HBM march: mib MiB (0 = what hipMemGetInfo reports free less "
        "max(HBMTEST_RESERVE_MIN_BYTES, HBMTEST_RESERVE_PERCENT % of the "
        "total), rounded down to HBMTEST_PAGE_BYTES) are allocated as chunks "
        "of HBMTEST_CHUNK_BYTES; an allocation the device has no room for "
        "ends the allocating (alloc_short), and less than HBMTEST_MIN_BYTES "
        "in all is an error. Global word w of the coverage holds pattern r % "
        "4 of (addr, addr_inv, hash, hash_inv) with seed mix(seed + r / 4) "
        "after round r. Pass 0 fills round 0, pass p reads and compares "
        "round p - 1 and writes round p to the same element, the last pass "
        "only reads; every pass covers every chunk before the next starts "
        "(grid=blocks, 0 = 1024), odd cycles of four go from the top down, "
        "and passes run until seconds (in (0, 600]) have passed, to the end "
        "of a cycle. A pass with a mismatch is the last. Returns {ok, device, "
        "seed, seconds, alloc_seconds, bytes, chunks, chunk_bytes: [bytes], "
        "free_bytes, total_bytes, alloc_short, rounds, passes, mismatches, "
        "flipped_or, bad_chunks: [(chunk, mismatches)], bad_pages, "
        "bad_pages_first: [(chunk, page)], records: [(pass, word, got, "
        "want)], gbs: {fill, march_addr, march_hash, verify}}; gbs is "
        "event-timed, counts read + write for the march passes and is "
        "informative only");
  m.def("hbm_march_probe", &hbm_march_probe, py::arg("device"),
        py::arg("nbytes"), py::arg("seed"), py::arg("rounds"),
        py::arg("blocks"), py::arg("chunk_bytes"), py::arg("flips"),
        "The HBM march's host loop and kernels on nbytes (a multiple of 16, "
        "at most 64 MiB) in guarded chunks of chunk_bytes (a multiple of 16, "
        "at most 64 chunks) for exactly `rounds` rounds with grid=blocks. "
        "Every (pass, global word, mask) of flips, 1 <= pass <= rounds, is "
        "XORed in after pass - 1 has written and before pass reads; all of "
        "them are checked before the first launch. Returns ([guard + chunk + "
        "guard], the dict of hbm_selftest)");
}
