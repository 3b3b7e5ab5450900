// Device primitives shared by the MFMA kernels (gfx950): each defined here once.
#pragma once
#include "common.h"

#include <type_traits>

namespace tv {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kTileM = 128;
constexpr int kTileN = 128;
constexpr int kRowBytes = 128;                       // bytes of K per step, per row
constexpr int kStageBytes = (kTileM + kTileN) * kRowBytes;  // 32 KiB
constexpr int kStageRow = kTileN * 4 + 16;           // fp32 epilogue row stride (bytes)
constexpr int kLdsBytes = (2 * kStageBytes > kTileM * kStageRow) ? 2 * kStageBytes : kTileM * kStageRow;

// byte offset of 16-byte chunk `c` of row `r` in a [rows][128 B] swizzled image
__device__ __forceinline__ int swz(int r, int c) { return r * kRowBytes + ((c ^ ((r >> 1) & 7)) << 4); }

template <typename T> struct Mfma;
template <> struct Mfma<_Float16> {
  __device__ static void run(const uint4& a, const uint4& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b),
                                                 acc, 0, 0, 0);
  }
};
template <> struct Mfma<__bf16> {
  __device__ static void run(const uint4& a, const uint4& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                  acc, 0, 0, 0);
  }
};
template <> struct Mfma<float> {
  // lane half h holds k = 4*(2j+h) + e for e = 0..3: four K=2 steps per 16-byte chunk
  __device__ static void run(const uint4& a, const uint4& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
};

template <typename T> __device__ __forceinline__ float to_f(T v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f(float v) { return (T)v; }

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4 g_cu32x4;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;

// Global (not flat) 16-byte accesses: pointers read from the parameter block are generic.
__device__ __forceinline__ uint4 gload16(const void* ptr) {
  u32x4 v = *(g_cu32x4*)(ptr);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void gstore16(void* ptr, uint4 v) { *(g_u32x4*)(ptr) = u32x4{v.x, v.y, v.z, v.w}; }
// 8-byte accesses (whole 256-byte rows from 32 lanes)
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 gload8(const void* ptr) {
  u32x2_t v = *(const __attribute__((address_space(1))) u32x2_t*)(ptr);
  return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void gstore8(void* ptr, uint2 v) {
  *(__attribute__((address_space(1))) u32x2_t*)(ptr) = u32x2_t{v.x, v.y};
}

// ---- address spaces and raw buffer operations ------------------------------------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) char lds_char;
typedef const __attribute__((address_space(3))) u32x4 lds_u32x4;
typedef const __attribute__((address_space(1))) void gvoid;
typedef __attribute__((address_space(1))) unsigned gu32;  // global (never flat) agent-scope ticket words

__device__ u32x4 raw_buffer_load_v4(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4i32");
__device__ u32x2 raw_buffer_load_v2(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v2i32");
__device__ unsigned raw_buffer_load_u32(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.i32");
__device__ unsigned char raw_buffer_load_u8(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.i8");
__device__ void raw_buffer_store_v4(u32x4 data, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v4i32");
__device__ void raw_buffer_store_v2(u32x2 data, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v2i32");
__device__ void raw_buffer_load_lds(i32x4 rsrc, __attribute__((address_space(3))) void* lds, int size, int voffset,
                                    int soffset, int offset, int aux) __asm("llvm.amdgcn.raw.buffer.load.lds");

constexpr int kRsrcWord3 = 0x00020000;  // last dword of a raw (untyped, range-checked) buffer resource
constexpr int OOB = (int)0x80000000u;  // a buffer offset past every resource: loads 0, stores dropped
constexpr int SC1 = 16;  // aux cache bits: sc1 (write-through store / L1-bypassing load)

// buffer resource over [base, base + bytes): raw (untyped) accesses, range-checked against bytes
__device__ __forceinline__ i32x4 rsrc_of(const void* base, unsigned bytes) {
  const unsigned long long a = (unsigned long long)base;
  i32x4 r;
  r.x = (int)(unsigned)a;
  r.y = (int)(unsigned)(a >> 32);
  r.z = (int)bytes;
  r.w = kRsrcWord3;
  return r;
}

__device__ __forceinline__ uint4 to_u4(u32x4 v) { return make_uint4(v.x, v.y, v.z, v.w); }

template <typename T>
__device__ __forceinline__ unsigned pack2(float a, float b) {
  typedef T t2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, t2{(T)a, (T)b});
}

// ---- LDS ---------------------------------------------------------------------------------------
// 16 bytes per lane from global memory straight into LDS (the wave's 1 KiB piece at dst)
__device__ __forceinline__ void dma16(const void* src, lds_char* dst) {
  __builtin_amdgcn_global_load_lds((gvoid*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}
// 16-byte LDS reads the compiler does not track: the caller owns the lgkmcnt wait before the
// first use of the result (tools/check_lds_asm.py checks the hand-scheduled bodies)
__device__ __forceinline__ u32x4 ds_read16(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
template <int OFF>
__device__ __forceinline__ u32x4 ds_read16_off(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
// an LDS read the compiler tracks (it places the lgkmcnt waits before the MFMAs that consume it)
__device__ __forceinline__ u32x4 lds_load16(unsigned addr) { return *reinterpret_cast<lds_u32x4*>(addr); }

// Workgroup barrier for LDS hand-offs only. __syncthreads() also waits for every outstanding
// global store (vmcnt(0)), which would drain a tile's 128 KiB of stores before the next tile's
// work instead of letting them stream under it.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// the same, and nothing is scheduled across it either (stem_s2's hand-ordered blocks; the two
// endings give different code in each other's kernels)
__device__ __forceinline__ void lds_barrier_sched() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// ---- counted waits and compile-time loops ------------------------------------------------------
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// s_waitcnt takes an immediate: dispatch the (wave-uniform, exact) count
__device__ __forceinline__ void wait_vm_n(int n) {
  switch (n) {
    case 0: wait_vm<0>(); break;
    case 1: wait_vm<1>(); break;
    case 2: wait_vm<2>(); break;
    case 3: wait_vm<3>(); break;
    case 4: wait_vm<4>(); break;
    case 5: wait_vm<5>(); break;
    case 6: wait_vm<6>(); break;
    case 7: wait_vm<7>(); break;
    case 8: wait_vm<8>(); break;
    case 9: wait_vm<9>(); break;
    case 10: wait_vm<10>(); break;
    case 11: wait_vm<11>(); break;
    case 12: wait_vm<12>(); break;
    default: wait_vm<13>(); break;
  }
}

template <int V>
using IC = std::integral_constant<int, V>;

// f(IC<Q>{}), f(IC<Q + 1>{}), ..., f(IC<N - 1>{}): straight-line code with compile-time indices
template <int Q, int N, typename F>
__device__ __forceinline__ void unroll(F& f) {
  if constexpr (Q < N) {
    f(IC<Q>{});
    unroll<Q + 1, N>(f);
  }
}

// ---- XCD-aware work order: workgroup b runs on XCD b % 8 ----------------------------------------
// Bijective remap of workgroup bid of n: each XCD walks a contiguous run of the linear index, so
// neighbouring tiles (shared halo rows, the same weight panel) meet in one XCD's L2.
__device__ __forceinline__ int xcd_linear(int bid, int n) {
  const int q8 = n >> 3, r8 = n & 7, xcd = bid & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}
// This workgroup's items first, first + stride, ... < end of a persistent grid over n items: one
// contiguous range per XCD, or plain grid-stride order when the grid is no multiple of 8.
struct XcdRange {
  int first, stride, end;  // (in the order the kernels declared them: it reaches the generated code)
};
__device__ __forceinline__ XcdRange xcd_range(int n) {
  const int G = gridDim.x, bid = blockIdx.x;
  XcdRange r;
  if ((G & 7) == 0) {
    r.first = (int)((long long)n * (bid & 7) / 8) + (bid >> 3);
    r.end = (int)((long long)n * ((bid & 7) + 1) / 8);
    r.stride = G >> 3;
  } else {
    r.first = bid;
    r.end = n;
    r.stride = G;
  }
  return r;
}

// ---- split-K ticket (gfx950 only: common.h) ------------------------------------------------------
// Call after the workgroup's sc1 stores of its partial tile to the slab: every storing wave drains
// them (vmcnt(0)), the workgroup barrier orders that before ONE relaxed agent-scope ticket, and
// the workgroup drawing ksplit - 1 is the last: it alone goes on, and reads the other slices with
// sc1 loads (the acquire fence is compiler-only). Workgroup-uniform result; lds_flag is one LDS
// word nobody else touches across the call.
__device__ __forceinline__ bool splitk_arrive_is_last(gu32* ticket, int ksplit, unsigned* lds_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) *lds_flag = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (*lds_flag != (unsigned)(ksplit - 1)) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return true;
}
// the last workgroup re-arms the ticket for the next launch (the engine also zeroes the tickets
// before each forward)
__device__ __forceinline__ void splitk_reset(gu32* ticket) {
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename OutT>
__device__ __forceinline__ void store_chunk(OutT* dst, const float* v);
template <>
__device__ __forceinline__ void store_chunk<float>(float* dst, const float* v) {
  gstore16(dst, make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])));
}
template <typename OutT>
__device__ __forceinline__ void store_chunk(OutT* dst, const float* v) {
  uint32_t w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    OutT lo = (OutT)v[2 * e], hi = (OutT)v[2 * e + 1];
    w[e] = (uint32_t)__builtin_bit_cast(uint16_t, lo) | ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16);
  }
  gstore16(dst, make_uint4(w[0], w[1], w[2], w[3]));
}

}  // namespace tv
