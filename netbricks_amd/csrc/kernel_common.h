// Device helpers shared by the kernel files (hash, LUT and parse helpers, 16-B loads and stores, the
// wave and block scans, the ballot multisplit), and the two host helpers every launcher uses.
#pragma once

#include <hip/hip_runtime.h>

#include "nbgpu_internal.h"

namespace nbg {

namespace {

constexpr uint32_t kSentinel = NBG_SENTINEL;
constexpr uint32_t kEth = 14;

// LUT placement / width variants.
enum LutMode { kLdsU8 = 0, kLdsU16 = 1, kGlobalU8 = 2, kGlobalU16 = 3, kLdsU8Tail = 4, kIdx = 5 };
// kIdx (NBG_LUT_TILED): no lookup; the classify kernel emits the LUT index (bit 31 set, so it
// cannot be mistaken for the would-panic bin) and the tiled lookup resolves it later.

// Packet layouts: fixed slots (general), fixed slots known by the host to be 16-B aligned with
// owned windows, no length array and frames >= 48 B (every chunk readable, no per-lane
// predicates), and descriptors (offset + length arrays).
enum Layout { kFixed = 0, kLean = 1, kDesc = 2 };

// h = h ^ b; h *= 0x100000001b3 on (lo, hi) 32-bit halves:
// h * (2^40 + 0x1b3) = lo*0x1b3 + 2^32 * ((hi*0x1b3 mod 2^32) + (lo << 8))  (mod 2^64)
// -> one v_mad_u64_u32 (lo*0x1b3 + (hi*0x1b3) << 32), one v_mul_lo_u32, one shift-add.
__device__ __forceinline__ void fnv_step(uint32_t& lo, uint32_t& hi, uint32_t b) {
  lo ^= b;
  const uint64_t t = static_cast<uint64_t>(lo) * 0x1b3u + (static_cast<uint64_t>(hi * 0x1b3u) << 32);
  hi = static_cast<uint32_t>(t >> 32) + (lo << 8);
  lo = static_cast<uint32_t>(t);
}

// x mod 65537 with 2^16 == -1 (mod 65537): alternating 16-bit digit sum.
__device__ __forceinline__ uint32_t mod_f4(uint32_t lo, uint32_t hi) {
  uint32_t r = (lo & 0xffffu) + (hi & 0xffffu) + 131074u - (lo >> 16) - (hi >> 16);  // [4, 262144]
  r = (r & 0xffffu) + 65537u - (r >> 16);                                          // [65533, 131072]
  return r >= 65537u ? r - 65537u : r;
}

// Barrett: mu = floor(2^64 / m); q underestimates floor(h/m) by at most one.
__device__ __forceinline__ uint32_t mod_barrett(uint32_t lo, uint32_t hi, uint32_t m, uint64_t mu) {
  const uint64_t h = (static_cast<uint64_t>(hi) << 32) | lo;
  const uint64_t q = __umul64hi(h, mu);
  uint64_t r = h - q * m;
  if (r >= m) r -= m;
  return static_cast<uint32_t>(r);
}

// FNV over Flow{src_ip, dst_ip, src_port, dst_port, proto} (LE fields of BE-read values).
// src/dst/ports are the wire bytes packed little-endian (wire byte k at bits 8k), so the
// hashed byte order is src[3..0], dst[3..0], ports[1],ports[0], ports[3],ports[2], proto.
__device__ __forceinline__ void fnv_flow(uint32_t& lo, uint32_t& hi, uint32_t src, uint32_t dst, uint32_t ports,
                                         uint32_t proto) {
  lo = 0x84222325u;  // 0xcbf29ce484222325
  hi = 0xcbf29ce4u;
  fnv_step(lo, hi, src >> 24);
  fnv_step(lo, hi, (src >> 16) & 0xffu);
  fnv_step(lo, hi, (src >> 8) & 0xffu);
  fnv_step(lo, hi, src & 0xffu);
  fnv_step(lo, hi, dst >> 24);
  fnv_step(lo, hi, (dst >> 16) & 0xffu);
  fnv_step(lo, hi, (dst >> 8) & 0xffu);
  fnv_step(lo, hi, dst & 0xffu);
  fnv_step(lo, hi, (ports >> 8) & 0xffu);
  fnv_step(lo, hi, ports & 0xffu);
  fnv_step(lo, hi, ports >> 24);
  fnv_step(lo, hi, (ports >> 16) & 0xffu);
  fnv_step(lo, hi, proto);
}

template <int LUTM>
__device__ __forceinline__ uint32_t lut_get(const ClassifyArgs& a, const uint8_t* lut_lds, uint32_t idx) {
  if constexpr (LUTM == kLdsU8) return lut_lds[idx];
  if constexpr (LUTM == kLdsU16) return reinterpret_cast<const uint16_t*>(lut_lds)[idx];
  if constexpr (LUTM == kGlobalU8) return static_cast<const uint8_t*>(a.lut)[idx];
  if constexpr (LUTM == kLdsU8Tail) return idx < 65536u ? lut_lds[idx] : a.lut_tail;  // streaming kernel
  if constexpr (LUTM == kIdx) return idx | 0x80000000u;
  return static_cast<const uint16_t*>(a.lut)[idx];
}

template <int LUTM, bool F4>
__device__ __forceinline__ uint32_t lookup(const ClassifyArgs& a, const uint8_t* lut_lds, uint32_t lo, uint32_t hi) {
  const uint32_t idx = F4 ? mod_f4(lo, hi) : mod_barrett(lo, hi, a.m, a.mu);
  return lut_get<LUTM>(a, lut_lds, idx);
}

// DIR-24-8 lookup_entry (test/lpm/src/nf.rs:88-98) of a host-order IPv4 address.
__device__ __forceinline__ uint32_t lpm_lookup(const uint16_t* tbl24, const uint16_t* tbl_long, uint32_t ip) {
  const uint32_t t = tbl24[ip >> 8];
  return (t & 0x8000u) ? tbl_long[((t & 0x7fffu) << 8) + (ip & 0xffu)] : t;
}

// One byte of global memory, loaded and waited for inside one asm statement: the compiler's wait
// pass never sees it pending (see classify_slow's SYNC).
__device__ __forceinline__ uint32_t ld_byte_sync(const uint8_t* p) {
  uint32_t v;
  asm volatile(
      "global_load_ubyte %0, %1, off\n\t"
      "s_waitcnt vmcnt(0)"
      : "=v"(v)
      : "v"(p)
      : "memory");
  return v;
}

// Byte-wise path: any alignment, any length, any IHL.  Returns the bin (nb = sentinel);
// CHAIN also sets the lpm gate (sentinel when test/lpm cannot parse the packet).
// SYNC (the streaming kernels): every byte is read by ld_byte_sync.  Compiler-visible loads here
// would stay pending, as far as the compiler's wait pass knows, across the unit loop's back-edge,
// and it then puts vmcnt(0) waits on the main path wherever the register allocator reuses their
// VGPRs, draining the LDS-DMA tile ring every step (measured: 2x per-step time in the lagged-
// grouping kernel).  A synchronous byte load costs a full memory round trip, but only packets off
// the fast path (none in the C2/C3/C5 traces) take this path.
// WT (the persistent ring kernel): the MAC bytes are stored write-through (sc1), so that they are in
// HBM once the store retires (nbg_ring completion, no L2 write-back in a kernel that never ends).
template <int LUTM, bool F4, bool CHAIN, bool SYNC = false, bool WT = false>
__device__ __forceinline__ uint32_t classify_slow(const ClassifyArgs& a, const uint8_t* lut_lds, uint8_t* p,
                                                  uint32_t len, uint32_t pkt, uint32_t& gate) {
  auto rd = [](const uint8_t* x) -> uint32_t {
    if constexpr (SYNC) return ld_byte_sync(x);
    return *x;
  };
  auto wr = [](uint8_t* x, uint8_t v) {
    if constexpr (WT)  // global (not flat): a flat store would also count in lgkmcnt
      __hip_atomic_store((__attribute__((address_space(1))) uint8_t*)(x), v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    else *x = v;
  };
  gate = kSentinel;
  if (len < kEth) return a.nb;  // Packet::parse_header assert (interface/packet.rs:392-399)
  const uint8_t* q = p + kEth;
  const uint32_t plen = len - kEth;
  if constexpr (CHAIN) {
    // test/lpm: parse::<IpHeader> asserts payload_size >= 20 (packet.rs:392-399, ip.rs:53-56);
    // the gate is the group index of its group_by(lpm_groups) (test/lpm/src/nf.rs:216-221)
    if (plen < 20) return a.nb;
    const uint32_t ip = (rd(q + 12) << 24) | (rd(q + 13) << 16) | (rd(q + 14) << 8) | rd(q + 15);
    gate = lpm_lookup(a.tbl24, a.tbl_long, ip);
    if (gate >= a.lpm_groups) return a.nb;
  } else if (a.swap) {  // transform runs before group_by over the batch (chain: two swaps cancel)
    uint8_t* o = a.mac_out ? a.mac_out + static_cast<size_t>(pkt) * 12u : p;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const uint8_t d = static_cast<uint8_t>(rd(p + k)), s = static_cast<uint8_t>(rd(p + k + 6));
      wr(o + k, s);
      wr(o + k + 6, d);
    }
  }
  if (plen < 20) return a.nb;  // slice OOB in ipv4_extract_flow
  const uint32_t ps = (rd(q) & 0xfu) * 4u;
  if (plen < ps + 4) return a.nb;
  const uint32_t src = rd(q + 12) | (rd(q + 13) << 8) | (rd(q + 14) << 16) | (rd(q + 15) << 24);
  const uint32_t dst = rd(q + 16) | (rd(q + 17) << 8) | (rd(q + 18) << 16) | (rd(q + 19) << 24);
  const uint32_t ports = rd(q + ps) | (rd(q + ps + 1) << 8) | (rd(q + ps + 2) << 16) | (rd(q + ps + 3) << 24);
  uint32_t lo, hi;
  fnv_flow(lo, hi, src, dst, ports, rd(q + 9));
  return lookup<LUTM, F4>(a, lut_lds, lo, hi);
}

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
// Packet windows are read once: the streaming policy.  Round 1 measured it neutral on C2's 4-stream
// path (then served by this kernel); round 2, with C2 on the streaming kernel, it cut C3 from 48.9 to
// 44.8 us and C5 from 28.3 to 26.5 us per batch at 3 streams (profiles/r02_c3_c5_ntloads_ab.txt).
__device__ __forceinline__ uint4 ldg16(const uint8_t* p) {
  const u32x4_t w = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  return make_uint4(w.x, w.y, w.z, w.w);
}
// Non-temporal 16-B store: in-place window write-back streams ~10 % faster with nt (tools/membench).
__device__ __forceinline__ void stg16_nt(uint8_t* p, uint4 v) {
  const u32x4_t w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<u32x4_t*>(p));
}

// Write-through 16-B store (sc1: the line leaves L2 for HBM; MI355X_MICROARCH.md visibility table):
// the persistent ring kernel's outputs, visible to any later launch or copy once the store retires.
// Inline asm (the compiler cannot emit sc1 on a 64-bit-addressed 16-B store); s_nop 1 keeps the
// compiler's next instruction off the data VGPRs while the store reads them.
__device__ __forceinline__ void stg16_wt(void* p, uint4 v) {
  const u32x4_t w = {v.x, v.y, v.z, v.w};
  asm volatile(
      "global_store_dwordx4 %0, %1, off sc1\n\t"
      "s_nop 1"
      :
      : "v"(p), "v"(w)
      : "memory");
}

// Workgroup barrier for LDS-only hand-offs: wait for this wave's LDS operations, then s_barrier.
// Unlike __syncthreads() it does not wait for outstanding global stores (the release fence drains
// vmcnt), which would put HBM write latency on the group kernel's critical path.
__device__ __forceinline__ void lds_sync() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0) only
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Loads at a 32-bit byte offset from a kernel-argument base: the compiler can then use the
// SGPR-base + 32-bit VGPR-offset form (one VGPR per address instead of two).
__device__ __forceinline__ uint32_t ld_u32(const uint32_t* base, uint32_t byte_off) {
  return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(base) + byte_off);
}
// Raw buffer resource over `bytes` bytes at p (gfx9 descriptor word 3: CK_BUFFER_RESOURCE_3RD_DWORD):
// a load past `bytes` returns 0 without touching memory, so the group kernel's loads need neither an
// index clamp nor a 64-bit address per lane (one 32-bit offset, constant parts in the instruction).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, static_cast<int>(bytes), 0x00020000);
}
__device__ __forceinline__ uint32_t ld_u16(const uint16_t* base, uint32_t byte_off) {
  return *reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(base) + byte_off);
}

// Inclusive scan over the 64 lanes of a wave with DPP moves (no LDS round trips): shifts by
// 1, 2, 4, 8 inside each 16-lane row, then row 0's / rows 0-1's totals broadcast into the rows
// above (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3).  Lanes a move does not
// write keep the `old` operand, 0.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
  x += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x111, 0xf, 0xf, false));
  x += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x112, 0xf, 0xf, false));
  x += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x114, 0xf, 0xf, false));
  x += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x118, 0xf, 0xf, false));
  x += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x142, 0xa, 0xf, false));
  x += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x143, 0xc, 0xf, false));
  return x;
}

// Block-wide exclusive scan of one value per thread (blocks of NT threads); returns the
// exclusive prefix and the total.
template <uint32_t NT>
__device__ __forceinline__ uint32_t block_excl_scan_n(uint32_t v, uint32_t* s_wave, uint32_t& total) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t x = wave_incl_scan(v);
  if (lane == 63u) s_wave[wave] = x;
  lds_sync();
  uint32_t wpre = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < NT / 64; ++w) {
    const uint32_t t = s_wave[w];
    if (w < wave) wpre += t;
    tot += t;
  }
  lds_sync();
  total = tot;
  return wpre + x - v;
}

// Stable rank of this lane among the lanes of its wave with the same `bin` (valid lanes only), and
// how many lanes hold that bin: one ballot per bin bit plus one for validity, no loop over lanes.
template <int BITS>
__device__ __forceinline__ void wave_match_rank(uint32_t bin, bool valid, uint32_t lane, uint32_t& rank,
                                                uint32_t& count) {
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const uint32_t mv = valid ? ~0u : 0u;
  const unsigned long long bv = __builtin_amdgcn_ballot_w64(valid);
  uint32_t elo = ~(static_cast<uint32_t>(bv) ^ mv), ehi = ~(static_cast<uint32_t>(bv >> 32) ^ mv);
#pragma unroll
  for (int bit = 0; bit < BITS; ++bit) {
    const uint32_t m = static_cast<uint32_t>(__builtin_amdgcn_sbfe(static_cast<int>(bin), bit, 1));  // 0 or ~0
    const unsigned long long bb = __builtin_amdgcn_ballot_w64(m != 0);
    elo &= ~(static_cast<uint32_t>(bb) ^ m);
    ehi &= ~(static_cast<uint32_t>(bb >> 32) ^ m);
  }
  rank = __popc(elo & static_cast<uint32_t>(lt)) + __popc(ehi & static_cast<uint32_t>(lt >> 32));
  count = __popc(elo) + __popc(ehi);
}

// N (2..4) consecutive bin bits b .. b + N - 1 of a wave ballot multisplit, four VALU operations per
// bit: the lane's bit as 0 / ~0 (v_bfe), the wave's ballot of it (v_cmp into an SGPR pair), and per
// 32-lane half acc |= ballot ^ bit in one v_bitop3 (truth table 0xde over (ballot, acc, bit)).  The
// compiler's own form of the accumulation took ~6 operations per bit (v_lshlrev + v_cmp for the
// ballot, two v_xor, v_or3), and the group kernel's ranks are VALU-bound (profiles/r05_group_pmc.txt).
// The N compares are one asm statement and the bitop3s follow in others: a VALU read of an SGPR that a
// VALU just wrote needs wait states on gfx950, which the compiler's hazard pass inserts between
// statements (one s_nop per group instead of one per bit).
template <int N>
__device__ __forceinline__ void mismatch_bits(uint32_t bin, int b, uint32_t& mlo, uint32_t& mhi) {
  static_assert(N >= 2 && N <= 4, "2 to 4 bits per group");
  uint32_t m[4];
  unsigned long long q[4];
#pragma unroll
  for (int k = 0; k < N; ++k) m[k] = static_cast<uint32_t>(__builtin_amdgcn_sbfe(static_cast<int>(bin), b + k, 1));
  if constexpr (N == 4)
    asm("v_cmp_ne_u32_e64 %0, 0, %4\n\tv_cmp_ne_u32_e64 %1, 0, %5\n\t"
        "v_cmp_ne_u32_e64 %2, 0, %6\n\tv_cmp_ne_u32_e64 %3, 0, %7"
        : "=&s"(q[0]), "=&s"(q[1]), "=&s"(q[2]), "=&s"(q[3])
        : "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]));
  else if constexpr (N == 3)
    asm("v_cmp_ne_u32_e64 %0, 0, %3\n\tv_cmp_ne_u32_e64 %1, 0, %4\n\tv_cmp_ne_u32_e64 %2, 0, %5"
        : "=&s"(q[0]), "=&s"(q[1]), "=&s"(q[2])
        : "v"(m[0]), "v"(m[1]), "v"(m[2]));
  else
    asm("v_cmp_ne_u32_e64 %0, 0, %2\n\tv_cmp_ne_u32_e64 %1, 0, %3" : "=&s"(q[0]), "=&s"(q[1]) : "v"(m[0]), "v"(m[1]));
#pragma unroll
  for (int k = 0; k < N; ++k) {
    asm("v_bitop3_b32 %0, %1, %0, %2 bitop3:0xde" : "+v"(mlo) : "s"(static_cast<uint32_t>(q[k])), "v"(m[k]));
    asm("v_bitop3_b32 %0, %1, %0, %2 bitop3:0xde" : "+v"(mhi) : "s"(static_cast<uint32_t>(q[k] >> 32)), "v"(m[k]));
  }
}

// All BITS bin bits (7 or 10): groups of 4, then the remaining 3 or 2
template <int BITS>
__device__ __forceinline__ void mismatch_all(uint32_t bin, uint32_t& mlo, uint32_t& mhi) {
  static_assert(BITS % 4 >= 2 || BITS % 4 == 0, "groups of 2 to 4 bits");
#pragma unroll
  for (int b = 0; b + 4 <= BITS; b += 4) mismatch_bits<4>(bin, b, mlo, mhi);
  if constexpr (BITS % 4 == 3) mismatch_bits<3>(bin, BITS - 3, mlo, mhi);
  if constexpr (BITS % 4 == 2) mismatch_bits<2>(bin, BITS - 2, mlo, mhi);
}

// One kernel launch and its check: `what` is the launcher's "<kernel> launch: %s" (NBG_EIO, HIP's text).
template <typename Fn, typename... Args>
int launch_checked(const char* what, Fn fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args&... args) {
  hipLaunchKernelGGL(fn, grid, block, lds, s, args...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(NBG_EIO, what, hipGetErrorString(e));
  return NBG_OK;
}

// Raise fn's dynamic-LDS limit to `bytes`; `what` is the launcher's "<kernel>: LDS attribute: %s".
// once (a launcher's static flag): skip the call after the first success.
template <typename Fn>
int raise_lds_limit(const char* what, Fn fn, size_t bytes, bool* once = nullptr) {
  if (once && *once) return NBG_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(bytes)) != hipSuccess)
    return set_error(NBG_EIO, what, hipGetErrorString(hipGetLastError()));
  if (once) *once = true;
  return NBG_OK;
}
}  // namespace

}  // namespace nbg
