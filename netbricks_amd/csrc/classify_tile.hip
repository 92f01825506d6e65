// The tile-per-wave classify kernels, the LDS-tiled lookup, the stand-alone lpm lookup and zero_kernel.
//
// classify_kernel — per packet (test/maglev/src/nf.rs:92-106):
//   parse::<MacHeader>   offset 14 (framework/src/headers/mac.rs:96-106, feature "performance")
//   swap_addresses       headers/mac.rs:140-145
//   ipv4_extract_flow    utils/flow.rs:53-62
//   FNV-1a 64 over the packed little-endian Flow (utils/flow.rs:10-18,105-110)
//   lut[hash % M]        test/maglev/src/nf.rs:78-81
//   + a per-tile backend histogram for the group_by FIFO order (operators/group_by.rs:46-51).
//   Loads are cooperative: a wave reads 64 packets' 64-B header windows as 16-B chunks
//   (4 lanes per window, contiguous 1 KiB per instruction for the 64-B slot layout),
//   transposes them through LDS to one packet per lane, and the lane holding chunk 0
//   applies the MAC swap in registers and writes the window back with full-line stores.
//
// Integer/byte work only; no MFMA.  HBM-bound.
#include <algorithm>

#include "kernel_common.h"

namespace nbg {

namespace {

// One wave's 64-packet tile in registers: lane = (quad, part) holds 16-B chunk `part` of
// packet k*16+quad (k = 0..3) — for 64-B slots each wave-instruction reads 1 KiB contiguous.
// Every load is issued unconditionally (a lane with nothing to read loads 16 B at the batch
// base) and nothing selects on its value: a predicated load merged with a default forces the
// compiler to wait for it inside the branch, serialising the four loads.  The chunk of a lane
// whose cflag bit is clear is never used.
struct TileRegs {
  uint4 ch[4];
  uint32_t cflag;  // bit k: chunk k was really read and the packet is long enough for the fast path
};

// Per-lane metadata of its own packet (descriptor mode: offset + length; else fixed).
struct TileMeta {
  uint32_t off, len;
};

// DESC (descriptor mode): off[] and len[] are both present and read unconditionally (clamped
// index), so the loads can stay in flight; otherwise only len[] may be present.
template <int LAYOUT>
__device__ __forceinline__ TileMeta load_meta(const ClassifyArgs& a, uint32_t wbase, uint32_t lane) {
  const uint32_t p = min(wbase + lane, a.n_pkts - 1u);  // clamped: the value of a lane past the end is unused
  TileMeta m;
  if constexpr (LAYOUT == kLean) {
    m.off = 0u;
    m.len = a.fixed_len;
  } else if constexpr (LAYOUT == kDesc) {
    m.off = a.off[p];
    m.len = a.len[p];
  } else {
    m.off = 0u;
    m.len = a.len ? a.len[p] : a.fixed_len;
  }
  return m;
}

// Fixed slots: the wave's tile base is wave-uniform (scalar 64-bit math) and lane offsets are
// 32-bit (stride < 2^24 is checked on the host), keeping 64-bit multiplies out of the VALU path.
template <int LAYOUT>
__device__ __forceinline__ const uint8_t* pkt_addr(const ClassifyArgs& a, uint32_t wbase, uint32_t idx_in_tile,
                                                   uint32_t off) {
  if constexpr (LAYOUT == kDesc) return a.pkts + off;
  return a.pkts + static_cast<size_t>(wbase) * a.stride + __umul24(idx_in_tile, a.stride);
}

template <int LAYOUT>
__device__ __forceinline__ void load_tile(const ClassifyArgs& a, uint32_t wbase, const TileMeta& m, uint32_t part,
                                          uint32_t quad, TileRegs& t) {
  constexpr bool DESC = LAYOUT == kDesc;
  const uint8_t* addr[4];
  t.cflag = 0;
  if constexpr (LAYOUT == kLean) {
    // every chunk of every packet is readable; only the batch tail is masked
    const uint8_t* tb = a.pkts + static_cast<size_t>(wbase) * a.stride + __umul24(quad, a.stride) + part * 16u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool pv = wbase + k * 16u + quad < a.n_pkts;
      addr[k] = pv ? tb + k * 16u * a.stride : a.pkts;
      t.cflag |= static_cast<uint32_t>(pv) << k;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) t.ch[k] = ldg16(addr[k]);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t src = k * 16u + quad;
    const uint32_t p = wbase + src;
    const bool pv = p < a.n_pkts;
    const uint32_t o = DESC ? static_cast<uint32_t>(__shfl(static_cast<int>(m.off), src)) : 0u;
    const uint32_t l = a.len ? static_cast<uint32_t>(__shfl(static_cast<int>(m.len), src)) : a.fixed_len;
    const uint8_t* base = pkt_addr<LAYOUT>(a, wbase, src, o);
    const bool aligned = (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
    // chunk readable/writable: inside the frame, or the window is owned by this packet.  (Read only,
    // chunk 3 is unused, but skipping its load measured 0.7 us slower for C5: profiles/r04_c5_ablation.txt)
    const bool inwin = a.win_owned || (part * 16u + 16u <= l);
    const bool rd = pv && aligned && inwin;
    addr[k] = rd ? base + part * 16u : a.pkts;
    if (rd && l >= 48u) t.cflag |= 1u << k;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) t.ch[k] = ldg16(addr[k]);
}

// One transposed 64-packet tile of classify_kernel (its loads in `cur`, its chunks 0..2 in the
// wave's LDS rows `xp`): classify each lane's packet, write back, count.  Packets off the fast
// path are classified after this tile's loads, stores and gathers are all issued (`slow`): their
// byte-wise loads would otherwise make the compiler wait for every outstanding load.
template <int LUTM, bool F4, bool HIST, bool CHAIN, int LAYOUT>
__device__ __forceinline__ void classify_tile(const ClassifyArgs& a, const uint8_t* lut_lds, const uint8_t* xp,
                                              uint32_t* hist, uint32_t lane, uint32_t part, uint32_t quad,
                                              uint32_t wbase, const TileMeta& meta, const TileRegs& cur) {
  constexpr bool desc = LAYOUT == kDesc;
  const uint32_t p_own = wbase + lane;
  // compute lane: one packet (issues the LUT / LPM gathers)
  uint32_t bin = a.nb, gate = kSentinel, iplo = 0;
  bool resolve = false;  // CHAIN fast path: `gate` holds the raw tbl24 entry until consumed
  bool slow = false;
  uint8_t* pown = const_cast<uint8_t*>(pkt_addr<LAYOUT>(a, wbase, lane, meta.off));
  if (p_own < a.n_pkts) {
    const uint8_t* x = xp + lane * kXStride;
    const uint32_t w3 = *reinterpret_cast<const uint32_t*>(x + 12);
    const bool aligned = LAYOUT == kLean || (reinterpret_cast<uintptr_t>(pown) & 15u) == 0;
    const bool longf = LAYOUT == kLean || meta.len >= 48u;
    // same decision as the loader lanes: chunks 0..2 were loaded (and, if swapping, get written)
    if (aligned && longf && ((w3 >> 16) & 0xfu) == 5u) {
      const uint4 c1 = *reinterpret_cast<const uint4*>(x + 16);
      const uint2 c2 = *reinterpret_cast<const uint2*>(x + 32);
      // frame bytes: src 26..29, dst 30..33, ports 34..37, proto 23
      const uint32_t src = (c1.z >> 16) | (c1.w << 16);
      const uint32_t dst = (c1.w >> 16) | (c2.x << 16);
      const uint32_t ports = (c2.x >> 16) | (c2.y << 16);
      uint32_t lo, hi;
      if constexpr (CHAIN) {  // tbl24 gather issued here, resolved after the LUT gather
        const uint32_t ip = __builtin_bswap32(src);
        gate = a.tbl24[ip >> 8];
        iplo = ip & 0xffu;
        resolve = true;
      }
      fnv_flow(lo, hi, src, dst, ports, c1.y >> 24);
      bin = lookup<LUTM, F4>(a, lut_lds, lo, hi);
    } else {
      slow = true;
    }
  }
  // MAC swap in the loader lanes + window write-back (fast-path packets only).  Never in the chain
  // (lpm's and maglev's swaps cancel; the host clears a.swap): compiled out there, so the tile's
  // registers are dead after the transpose
  if (!CHAIN && a.swap) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // the quad's chunk-0 lane holds bytes 12..15 (IHL) of this packet
      const uint32_t w3 = static_cast<uint32_t>(__shfl(static_cast<int>(cur.ch[k].w), lane & ~3u));
      const bool fast = ((cur.cflag >> k) & 1u) && ((w3 >> 16) & 0xfu) == 5u;
      const uint32_t src = k * 16u + quad;
      const uint32_t o = desc ? static_cast<uint32_t>(__shfl(static_cast<int>(meta.off), src)) : 0u;
      if (!fast) continue;
      uint8_t* base = const_cast<uint8_t*>(pkt_addr<LAYOUT>(a, wbase, src, o));
      uint4 v = cur.ch[k];
      if (part == 0u) {
        const uint32_t w0 = v.x, w1 = v.y, w2 = v.z;
        // new bytes 0..5 = old 6..11, new 6..11 = old 0..5
        v = make_uint4((w1 >> 16) | (w2 << 16), (w2 >> 16) | (w0 << 16), (w0 >> 16) | (w1 << 16), v.w);
      }
      if (a.mac_out) {
        // egress rewrite record: the 12 swapped bytes, dense (packet bytes untouched)
        if (part == 0u) {
          uint32_t* mo = reinterpret_cast<uint32_t*>(a.mac_out + static_cast<size_t>(wbase + src) * 12u);
          mo[0] = v.x;
          mo[1] = v.y;
          mo[2] = v.z;
        }
      } else if (part == 0u || a.wb_full) {
        stg16_nt(base + part * 16u, v);  // chunks 1..3 unchanged: makes the write whole lines
      }
    }
  }
  // consume the gathers
  if (p_own < a.n_pkts) {
    if (slow) bin = classify_slow<LUTM, F4, CHAIN>(a, lut_lds, pown, meta.len, p_own, gate);
    if constexpr (CHAIN) {
      if (resolve && (gate & 0x8000u)) gate = a.tbl_long[((gate & 0x7fffu) << 8) + iplo];
      a.gate[p_own] = static_cast<uint16_t>(gate);
      if (gate >= a.lpm_groups) bin = a.nb;  // test/lpm would panic: never reaches maglev
    }
    if constexpr (LUTM == kIdx) {
      a.idx_out[p_own] = (bin & 0x80000000u) ? (bin & 0x7fffffffu) : 0xffffffffu;
    } else {
      a.backend[p_own] = static_cast<uint16_t>(bin == a.nb ? kSentinel : bin);
      if constexpr (HIST) atomicAdd(&hist[bin], 1u);
    }
  }
}

// classify_kernel: each wave walks `tiles_per_wave` consecutive 64-packet tiles.  L2-gathered LUT:
// 256-thread blocks, one tile per wave, 8 blocks per CU (occupancy hides the latency; a software
// pipeline measured no faster there and cost 18 VGPRs).  LDS-staged LUT: one
// 1024-thread block per CU, up to 4 tiles per wave with two tiles' loads in flight (below).  Per
// tile: loads, LDS transpose, hash + gathers, then the write-back stores (vmcnt retires in issue
// order: stores issued before the gathers would delay their use), then the slow-path packets.
// One LDS histogram per block (two barriers per launch) is flushed once into the block's partition
// row (the block's 64 * waves * tiles_per_wave packets divide part_pkts).
// The kernel body; `bid` is the block's index within its batch (classify_desc_multi_kernel runs
// several batches' blocks in one grid).
template <int LUTM, bool F4, bool HIST, bool CHAIN, int LAYOUT, int NT>
__device__ __forceinline__ void classify_body(const ClassifyArgs& a, const uint32_t bid) {
  extern __shared__ __align__(16) uint8_t smem[];  // classify_lds() (after this body) sizes this carve-up
  constexpr uint32_t kW = NT / 64u;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t part = lane & 3u, quad = lane >> 2;
  const uint32_t nbins = a.nb + 1;
  constexpr bool kLdsLut = LUTM == kLdsU8 || LUTM == kLdsU16;
  const uint32_t lut_bytes = kLdsLut ? a.lut_lds_bytes : 0u;
  uint8_t* lut_lds = smem;
  uint8_t* xp = smem + lut_bytes + wave * (64u * kXStride);
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + lut_bytes + kW * 64u * kXStride);  // per block
  const uint32_t tpw = a.tiles_per_wave;
  const uint32_t t0 = (bid * kW + wave) * tpw;  // first 64-packet tile of this wave

  // LDS-staged LUT: one 1024-thread block per CU (4 waves per SIMD) leaves VGPRs for kPf tiles'
  // loads in flight beside the tile being classified (a ring of kPf + 1 register tiles; the tile
  // loop is unrolled so that the ring stays in registers).  The first tiles' loads are issued
  // before the LUT staging, so that its latency hides under theirs.
  constexpr uint32_t kPf = kLdsLut ? 2u : 0u;
  constexpr uint32_t kRing = kPf + 1u;
  constexpr uint32_t kMaxTpw = kLdsLut ? kChunk / (64u * kW) : 1u;
  TileMeta rm[kRing];
  TileRegs rt[kRing];
  if constexpr (kLdsLut) {
#pragma unroll
    for (uint32_t j = 0; j < kPf; ++j) {
      const uint32_t wb = (t0 + j) * 64u;
      if (j < tpw && wb < a.n_pkts) {
        rm[j] = load_meta<LAYOUT>(a, wb, lane);
        load_tile<LAYOUT>(a, wb, rm[j], part, quad, rt[j]);
      }
    }
    constexpr int kS = 8;  // 16 B per thread per slot: up to 128 KiB per 1024-thread block
    const uint32_t nvec = lut_bytes / 16u;
    const uint4* src = static_cast<const uint4*>(a.lut);
    uint4 lt[kS];
#pragma unroll
    for (int j = 0; j < kS; ++j) {
      const uint32_t k = j * NT + tid;
      lt[j] = k < nvec ? src[k] : make_uint4(0, 0, 0, 0);
    }
    uint4* dst = reinterpret_cast<uint4*>(lut_lds);
#pragma unroll
    for (int j = 0; j < kS; ++j) {
      const uint32_t k = j * NT + tid;
      if (k < nvec) dst[k] = lt[j];
    }
  }
  if constexpr (HIST) {
    for (uint32_t b = tid; b < nbins; b += NT) hist[b] = 0;
  }
  if constexpr (HIST || kLdsLut) lds_sync();

  // transpose: chunks 0..2 of each packet of a tile -> LDS [packet][kXStride B]
  auto transpose = [&](const TileRegs& cur) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (part < 3u) *reinterpret_cast<uint4*>(xp + (k * 16u + quad) * kXStride + part * 16u) = cur.ch[k];
    }
  };


  if constexpr (kPf > 0) {
    // tile i sits in ring slot i % kRing; after its transpose, tile i + kPf is loaded into the
    // slot tile i - 1 used
#pragma unroll
    for (uint32_t i = 0; i < kMaxTpw; ++i) {
      const uint32_t wbase = (t0 + i) * 64u;
      if (i >= tpw || wbase >= a.n_pkts) break;  // wave-uniform
      transpose(rt[i % kRing]);
      const uint32_t j = i + kPf, wb = (t0 + j) * 64u;
      if (j < tpw && wb < a.n_pkts) {
        rm[j % kRing] = load_meta<LAYOUT>(a, wb, lane);
        load_tile<LAYOUT>(a, wb, rm[j % kRing], part, quad, rt[j % kRing]);
      }
      classify_tile<LUTM, F4, HIST, CHAIN, LAYOUT>(a, lut_lds, xp, hist, lane, part, quad, wbase, rm[i % kRing],
                                                           rt[i % kRing]);
    }
  } else if (LAYOUT == kDesc && tpw > 1u && tpw <= 4u) {
    // descriptor layouts, 2..4 tiles per wave (NBG_TPW, measurement): the descriptors of all of the
    // wave's tiles are loaded up front (measured no faster than one tile per wave for C3 / C5:
    // profiles/r04_c5_ablation.txt), unconditionally (clamped), so every tile after the first
    // issues its window loads at once instead of after a descriptor round trip of its own
    constexpr uint32_t kMetaTiles = 4;
    TileMeta mq[kMetaTiles];
#pragma unroll
    for (uint32_t j = 0; j < kMetaTiles; ++j) mq[j] = load_meta<LAYOUT>(a, (t0 + j) * 64u, lane);
#pragma unroll
    for (uint32_t i = 0; i < kMetaTiles; ++i) {
      const uint32_t wbase = (t0 + i) * 64u;
      if (i >= tpw || wbase >= a.n_pkts) break;  // wave-uniform
      __builtin_amdgcn_s_setprio(kLoadPrio);
      TileRegs cur;
      load_tile<LAYOUT>(a, wbase, mq[i], part, quad, cur);
      __builtin_amdgcn_s_setprio(0);
      transpose(cur);
      classify_tile<LUTM, F4, HIST, CHAIN, LAYOUT>(a, lut_lds, xp, hist, lane, part, quad, wbase, mq[i], cur);
    }
  } else {
    for (uint32_t i = 0; i < tpw; ++i) {
      const uint32_t wbase = (t0 + i) * 64u;
      if (wbase >= a.n_pkts) break;  // wave-uniform
      // The tile's loads are issued at raised wave priority, so a newly started wave gets its HBM
      // requests out ahead of resident waves' hash/gather work (bench +2 % in place, +4 % records).
      __builtin_amdgcn_s_setprio(kLoadPrio);
      const TileMeta meta = load_meta<LAYOUT>(a, wbase, lane);
      TileRegs cur;
      load_tile<LAYOUT>(a, wbase, meta, part, quad, cur);
      __builtin_amdgcn_s_setprio(0);
      transpose(cur);
      classify_tile<LUTM, F4, HIST, CHAIN, LAYOUT>(a, lut_lds, xp, hist, lane, part, quad, wbase, meta, cur);
    }
  }

  if constexpr (HIST) {
    // one flush per block into its partition row (the block's packets never straddle two):
    // 4096-packet rows take ~16 blocks' adds, so they rarely contend
    lds_sync();
    const uint32_t p = bid * kW * tpw * 64u / a.part_pkts;
    if (a.hist16) {  // two bins per word: half the atomics, and half the rows' bytes for the group kernel
      const uint32_t hw = (nbins + 1) >> 1;
      uint32_t* row = a.part_hist + static_cast<size_t>(p) * hw;
      for (uint32_t w = tid; w < hw; w += NT) {
        const uint32_t h = hist[2 * w] | (2 * w + 1 < nbins ? hist[2 * w + 1] << 16 : 0u);
        if (h) atomicAdd(&row[w], h);
      }
    } else {
      uint32_t* row = a.part_hist + static_cast<size_t>(p) * nbins;
      for (uint32_t b = tid; b < nbins; b += NT) {
        const uint32_t h = hist[b];
        if (h) atomicAdd(&row[b], h);
      }
    }
  }
}

// classify_body's dynamic LDS as it is carved up at its top (LUT, one transpose area per wave, hist).
// The block histogram is allocated only when the kernel keeps one (HIST): C3's 1001 bins would
// otherwise cost every 256-thread block 4 KB of the LDS a co-resident group block needs.
size_t classify_lds(uint32_t nb, uint32_t lut_lds_bytes, bool hist = true) {
  const uint32_t waves = (lut_lds_bytes ? kLdsBlock : kBlock) / 64;
  return static_cast<size_t>(lut_lds_bytes) + waves * 64u * kXStride + (hist ? static_cast<size_t>(nb + 1) * 4 : 0u);
}


template <int LUTM, bool F4, bool HIST, bool CHAIN, int LAYOUT, int NT = kBlock>
__global__ __launch_bounds__(NT, CHAIN ? 1 : 2048 / NT) void classify_kernel(ClassifyArgs a) {
  classify_body<LUTM, F4, HIST, CHAIN, LAYOUT, NT>(a, blockIdx.x);
}

// Several descriptor batches in one grid (several RX queues' bursts per launch): the launch's ramp
// and tail are paid once for all of them.  The batch of a block is found by a wave-uniform scan of
// blk_base (monotone; an empty batch owns no block).
template <int LUTM, bool F4, bool HIST, bool CHAIN>
__global__ __launch_bounds__(kBlock, CHAIN ? 1 : 2048 / kBlock) void classify_desc_multi_kernel(ClassifyArgs a,
                                                                                                 DescBatches db) {
  uint32_t j = 0;
#pragma unroll
  for (uint32_t k = 1; k < kMaxMulti; ++k) j = (k < db.n && blockIdx.x >= db.blk_base[k]) ? k : j;
  ClassifyArgs b = a;
  b.pkts = db.pkts[j];
  b.off = db.off[j];
  b.len = db.len[j];
  b.backend = db.backend[j];
  b.gate = db.gate[j];
  b.part_hist = db.part_hist[j];
  b.n_pkts = db.n_pkts[j];
  classify_body<LUTM, F4, HIST, CHAIN, kDesc, kBlock>(b, blockIdx.x - db.blk_base[j]);
}

// ---- LDS-tiled lookup (NBG_LUT_TILED; config C3's named variant) --------------------------------
// A u16 LUT larger than LDS (C3: 655373 entries = 1.25 MiB) is split into 64-KiB tiles of 32768
// entries.  After the classify kernel has written each packet's LUT index (kIdx):
//   tile_bucket_kernel  appends (packet, index in tile) to its tile's bucket: counts per tile in
//                       LDS, one global reservation per tile per block, then the scatter;
//   tile_lookup_kernel  one block per (tile, chunk of its bucket) stages the tile in LDS and
//                       resolves its chunk: backend[packet] = tile[index].
// Would-panic packets (index 0xffffffff) get the sentinel in the bucket kernel.  The measured
// alternative to the L2 gather that BASELINE config C3 names.
constexpr uint32_t kTileEntries = 32768;  // u16 entries per 64-KiB LUT tile
constexpr uint32_t kBucketNT = 256, kBucketPkts = 4096, kLookupNT = 512, kLookupChunk = 8192;

__global__ __launch_bounds__(kBucketNT) void tile_bucket_kernel(TileArgs a) {
  extern __shared__ __align__(16) uint32_t tcnt[];  // [n_tiles] counts, then reserved bases
  const uint32_t tid = threadIdx.x, p0 = blockIdx.x * kBucketPkts;
  for (uint32_t t = tid; t < a.n_tiles; t += kBucketNT) tcnt[t] = 0;
  __syncthreads();
  constexpr uint32_t kPer = kBucketPkts / kBucketNT;
  uint32_t idx[kPer], slot[kPer];
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const uint32_t p = p0 + k * kBucketNT + tid;
    idx[k] = a.idx[min(p, a.n_pkts - 1u)];
  }
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const uint32_t p = p0 + k * kBucketNT + tid;
    slot[k] = 0;
    if (p < a.n_pkts) {
      if (idx[k] == 0xffffffffu) a.backend[p] = static_cast<uint16_t>(kSentinel);
      else slot[k] = atomicAdd(&tcnt[idx[k] / kTileEntries], 1u);
    }
  }
  __syncthreads();
  for (uint32_t t = tid; t < a.n_tiles; t += kBucketNT)
    tcnt[t] = tcnt[t] ? atomicAdd(&a.cursor[t], tcnt[t]) : 0u;
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const uint32_t p = p0 + k * kBucketNT + tid;
    if (p < a.n_pkts && idx[k] != 0xffffffffu) {
      const uint32_t t = idx[k] / kTileEntries;
      a.bucket[static_cast<size_t>(t) * a.bucket_cap + tcnt[t] + slot[k]] =
          (static_cast<uint64_t>(p) << 32) | (idx[k] - t * kTileEntries);
    }
  }
}

__global__ __launch_bounds__(kLookupNT) void tile_lookup_kernel(TileArgs a) {
  extern __shared__ __align__(16) uint16_t tlut[];  // one LUT tile
  const uint32_t t = blockIdx.y, tid = threadIdx.x;
  const uint32_t cnt = a.cursor[t];
  const uint32_t c0 = blockIdx.x * kLookupChunk;
  if (c0 >= cnt) return;  // block-uniform
  const uint32_t entries = min(kTileEntries, a.m - t * kTileEntries);
  const uint4* src = reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(a.lut) + t * kTileEntries);
  for (uint32_t v = tid; v < (entries + 7) / 8; v += kLookupNT) reinterpret_cast<uint4*>(tlut)[v] = src[v];
  __syncthreads();
  const uint64_t* b = a.bucket + static_cast<size_t>(t) * a.bucket_cap;
  const uint32_t c1 = min(c0 + kLookupChunk, cnt);
  for (uint32_t i = c0 + tid; i < c1; i += kLookupNT) {
    const uint64_t e = b[i];
    a.backend[static_cast<uint32_t>(e >> 32)] = tlut[static_cast<uint32_t>(e)];
  }
}

template <int LUTM, bool F4, bool HIST, bool CHAIN>
int launch_one(const ClassifyArgs& a, int grid, size_t lds, hipStream_t s) {
  constexpr int NT = (LUTM == kLdsU8 || LUTM == kLdsU16) ? kLdsBlock : kBlock;
  auto fn = a.off ? classify_kernel<LUTM, F4, HIST, CHAIN, kDesc, NT>
                  : (a.lean ? classify_kernel<LUTM, F4, HIST, CHAIN, kLean, NT>
                            : classify_kernel<LUTM, F4, HIST, CHAIN, kFixed, NT>);
  return launch_checked("classify launch: %s", fn, dim3(grid), dim3(NT), lds, s, a);
}

template <int LUTM, bool F4, bool HIST>
int launch_v(const ClassifyArgs& a, int grid, size_t lds, hipStream_t s) {
  if (a.tbl24) return launch_one<LUTM, F4, HIST, true>(a, grid, lds, s);
  return launch_one<LUTM, F4, HIST, false>(a, grid, lds, s);
}

template <int LUTM>
int launch_mode(const ClassifyArgs& a, bool hist, int grid, size_t lds, hipStream_t s) {
  if (a.m == 65537u)
    return hist ? launch_v<LUTM, true, true>(a, grid, lds, s) : launch_v<LUTM, true, false>(a, grid, lds, s);
  return hist ? launch_v<LUTM, false, true>(a, grid, lds, s) : launch_v<LUTM, false, false>(a, grid, lds, s);
}

}  // namespace

int launch_classify(const ClassifyArgs& a, bool wide_lut, bool lds_lut, int grid, void* stream) {
  const bool hist = a.part_hist != nullptr;
  const size_t lds = classify_lds(a.nb, lds_lut ? a.lut_lds_bytes : 0, hist);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (lds_lut)
    return wide_lut ? launch_mode<kLdsU16>(a, hist, grid, lds, s) : launch_mode<kLdsU8>(a, hist, grid, lds, s);
  return wide_lut ? launch_mode<kGlobalU16>(a, hist, grid, lds, s) : launch_mode<kGlobalU8>(a, hist, grid, lds, s);
}

__global__ __launch_bounds__(kBlock) void lpm_lookup_kernel(const uint16_t* __restrict__ tbl24,
                                                            const uint16_t* __restrict__ tbl_long,
                                                            const uint32_t* __restrict__ ips, uint32_t n,
                                                            uint16_t* __restrict__ gate) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) gate[i] = static_cast<uint16_t>(lpm_lookup(tbl24, tbl_long, ips[i]));
}

int launch_lpm_lookup(const uint16_t* tbl24, const uint16_t* tbl_long, const uint32_t* ips, uint64_t n,
                      uint16_t* gate, void* stream) {
  const uint32_t grid = static_cast<uint32_t>((n + kBlock - 1) / kBlock);
  return launch_checked("lpm lookup launch: %s", lpm_lookup_kernel, dim3(grid), dim3(kBlock), 0,
                        static_cast<hipStream_t>(stream), tbl24, tbl_long, ips, static_cast<uint32_t>(n), gate);
}

__global__ __launch_bounds__(kBlock) void zero_kernel(uint32_t* p, uint32_t words) {
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < words; i += gridDim.x * kBlock) p[i] = 0;
}

int launch_zero(uint32_t* p, size_t words, void* stream) {
  if (words == 0) return NBG_OK;
  const uint32_t grid = static_cast<uint32_t>(std::min<size_t>((words + kBlock - 1) / kBlock, 1024));
  return launch_checked("zero launch: %s", zero_kernel, dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), p,
                        static_cast<uint32_t>(words));
}

uint32_t classify_block_pkts() { return kBlock; }  // per tile per wave (64 packets x 4 waves)

template <int LUTM, bool F4, bool HIST>
int launch_desc_multi_v(const ClassifyArgs& a, const DescBatches& db, size_t lds, hipStream_t s) {
  auto fn = a.tbl24 ? classify_desc_multi_kernel<LUTM, F4, HIST, true> : classify_desc_multi_kernel<LUTM, F4, HIST, false>;
  return launch_checked("classify launch (descriptor multi): %s", fn, dim3(db.blk_base[db.n]), dim3(kBlock), lds, s, a, db);
}

int launch_classify_desc_multi(const ClassifyArgs& a, const DescBatches& db, bool wide_lut, void* stream) {
  if (db.n == 0 || db.n > kMaxMulti || (a.tiles_per_wave != 1u && a.tiles_per_wave != 2u && a.tiles_per_wave != 4u))
    return set_error(NBG_EINVAL, "classify (descriptor multi): %u batches, %u tiles per wave", db.n, a.tiles_per_wave);
  if (db.blk_base[db.n] == 0) return NBG_OK;
  const bool hist = db.part_hist[0] != nullptr;
  const size_t lds = classify_lds(a.nb, 0, hist);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (wide_lut) {
    if (a.m == 65537u)
      return hist ? launch_desc_multi_v<kGlobalU16, true, true>(a, db, lds, s) : launch_desc_multi_v<kGlobalU16, true, false>(a, db, lds, s);
    return hist ? launch_desc_multi_v<kGlobalU16, false, true>(a, db, lds, s) : launch_desc_multi_v<kGlobalU16, false, false>(a, db, lds, s);
  }
  if (a.m == 65537u)
    return hist ? launch_desc_multi_v<kGlobalU8, true, true>(a, db, lds, s) : launch_desc_multi_v<kGlobalU8, true, false>(a, db, lds, s);
  return hist ? launch_desc_multi_v<kGlobalU8, false, true>(a, db, lds, s) : launch_desc_multi_v<kGlobalU8, false, false>(a, db, lds, s);
}

int launch_classify_idx(const ClassifyArgs& a, int grid, void* stream) {
  const size_t lds = classify_lds(a.nb, 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto fn = a.off ? classify_kernel<kIdx, false, false, false, kDesc>
                  : (a.lean ? classify_kernel<kIdx, false, false, false, kLean>
                            : classify_kernel<kIdx, false, false, false, kFixed>);
  return launch_checked("classify (index) launch: %s", fn, dim3(grid), dim3(kBlock), lds, s, a);
}

int launch_tiled_lookup(const TileArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = launch_checked("tile bucket launch: %s", tile_bucket_kernel, dim3((a.n_pkts + kBucketPkts - 1) / kBucketPkts),
                          dim3(kBucketNT), a.n_tiles * 4, s, a);
  if (rc) return rc;
  static bool attr = false;
  if ((rc = raise_lds_limit("tile lookup: LDS attribute: %s", tile_lookup_kernel, kTileEntries * 2, &attr))) return rc;
  return launch_checked("tile lookup launch: %s", tile_lookup_kernel,
                        dim3((a.n_pkts + kLookupChunk - 1) / kLookupChunk, a.n_tiles), dim3(kLookupNT), kTileEntries * 2, s, a);
}

uint32_t lut_tiles(uint64_t m) { return static_cast<uint32_t>((m + kTileEntries - 1) / kTileEntries); }

// Grid for the classify kernel: resident blocks (CUs x blocks/CU by LDS), so that the
// LDS-staged LUT is loaded once per resident block and amortised over its tiles.
int classify_grid(bool lds_lut, uint32_t lut_bytes, uint32_t nb, int device, int* grid) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
    return set_error(NBG_ENODEV, "hipDeviceGetAttribute(CU count) failed");
  const size_t lds = classify_lds(nb, lds_lut ? lut_bytes : 0);
  int per_cu = static_cast<int>((160 * 1024) / lds);
  per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
  *grid = cus * per_cu;
  return NBG_OK;
}

}  // namespace nbg
