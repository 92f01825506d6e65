// The streaming classify kernels (one persistent block per CU, tiles through LDS by LDS-DMA): fixed
// slots with the lagged grouping, the persistent RX ring with its gate, and descriptor layouts.
#include "kernel_common.h"

namespace nbg {

namespace {

// ---- streaming classify (fixed 64-B-aligned slots, u8 LUT <= 65537 entries) -------------------
//
// One 512-thread block per CU (persistent).  The block stages the LUT in LDS once with LDS-DMA
// (entries 0..65535; entry 65536 of a 65537-slot table is the kernel argument lut_tail), so the
// per-packet lookup is an LDS read instead of an L2 gather (a 1M-packet batch of L2 gathers costs
// ~3.3 us of L2 request throughput).  Each wave then streams 64-packet tiles through a
// private ring of kRing LDS buffers: every packet's row lands packet-major by global_load_lds_dwordx4
// straight from HBM — no VGPRs held by loads in flight, no transpose — while the wave classifies the
// tile kStreamAhead tiles behind.  Tiles are interleaved so that the whole grid sweeps the batch
// sequentially; the block's backend histogram is flushed once per unit of W tiles.
//
// LDS-DMA writes are ordered for the issuing wave's ds_read only by its own covering vmcnt
// (MI355X_MICROARCH.md item 7).  hipcc does not count the inline-asm loads, so each tile is waited
// for with a counted s_waitcnt vmcnt(4 * tiles issued after it): other VM operations issued in
// between (stores, flush atomics, the compiler's slow-path loads) only make that wait conservative.
constexpr int kStreamNT = 512;                 // threads per block (8 waves)
constexpr int kStreamW = kStreamNT / 64;
constexpr int kRing = 2;                       // LDS tile buffers per wave
[[maybe_unused]] constexpr int kStreamAhead = kRing - 1;  // tiles in flight while one is classified
static_assert(kRing >= 2 && kRing <= 3, "classify_stream_kernel tracks the counts of three tiles at most");
// LDS bytes per packet: 48 (chunks 0..2, all the classify reads) for read-only and records; 64 (the
// whole slot) for the in-place swap, which then writes every line back whole from LDS (measured:
// 48-B rows read faster, whole-line write-back beats 16-B partial-line stores)
template <int MODE>
constexpr uint32_t row_of() { return MODE == 1 ? 64u : 48u; }
template <int MODE>
constexpr uint32_t stream_row_of() { return row_of<MODE>(); }
constexpr uint32_t kLutLds = 65536;            // LUT bytes staged in LDS

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return static_cast<uint32_t>(
      reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) void*)(p)));
}

// 16 B per active lane from `src` into LDS at m0 + lane * 16 (lds_base wave-uniform).
__device__ __forceinline__ void glds16(const void* src, uint32_t lds_base) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_base))
      : "memory");
}

// The same with the streaming (non-temporal) policy, for packet windows (read once).  Measured on
// classify_stream_kernel, 1M packets, one MI355X (tools/runs/gpu_ab_ms.sh, profiles/r02_tile_nt_ab.txt):
// one stream, read-only 14.6 -> 13.5 us, in place 27.5 -> 25.5, records 17.0 -> 16.6; three streams
// with grouping, read-only 16.1 -> 15.8, in place neutral, records 17.8 -> 18.9 (slower).  So nt for
// read-only and in place (NT = true), the default policy for records.  The LUT pieces keep the
// default policy: every CU of an XCD re-reads them from L2.
template <bool NT>
__device__ __forceinline__ void glds16_tile(const void* src, uint32_t lds_base) {
  if constexpr (NT) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off nt\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_base))
        : "memory");
  } else {
    glds16(src, lds_base);
  }
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

// Wait until tile i's four LDS-DMA loads landed: `ahead` tiles (0..5) were issued after it.
__device__ __forceinline__ void wait_tile(uint32_t ahead) {
  if (ahead >= 5) wait_vm<20>();
  else if (ahead == 4) wait_vm<16>();
  else if (ahead == 3) wait_vm<12>();
  else if (ahead == 2) wait_vm<8>();
  else if (ahead == 1) wait_vm<4>();
  else wait_vm<0>();
}

// Wait until at most n VM operations are outstanding (n above 31 waits for 31: stricter, still right).
__device__ __forceinline__ void wait_vm_n(uint32_t n) {
#define NBG_VMC(i) \
  case i:          \
    wait_vm<i>();  \
    break;
  switch (n) {
    NBG_VMC(0) NBG_VMC(1) NBG_VMC(2) NBG_VMC(3) NBG_VMC(4) NBG_VMC(5) NBG_VMC(6) NBG_VMC(7)
    NBG_VMC(8) NBG_VMC(9) NBG_VMC(10) NBG_VMC(11) NBG_VMC(12) NBG_VMC(13) NBG_VMC(14) NBG_VMC(15)
    NBG_VMC(16) NBG_VMC(17) NBG_VMC(18) NBG_VMC(19) NBG_VMC(20) NBG_VMC(21) NBG_VMC(22) NBG_VMC(23)
    NBG_VMC(24) NBG_VMC(25) NBG_VMC(26) NBG_VMC(27) NBG_VMC(28) NBG_VMC(29) NBG_VMC(30)
    default:
      wait_vm<31>();
      break;
  }
#undef NBG_VMC
}

// Issue tile `t` (64 packets from tile base `tb`) into the LDS buffer at `buf`: instruction k
// covers packets 16k..16k+15.  48-B rows: lane l < 48 fetches chunk l % 3 of packet 16k + l / 3;
// 64-B rows: lane l fetches chunk l % 4 of packet 16k + l / 4 (1 KiB contiguous).  Lanes past the
// batch end fetch the batch base (their rows are never read).
template <uint32_t kRow, bool NT>
__device__ __forceinline__ void issue_tile(const ClassifyArgs& a, uint32_t tb, uint32_t buf, uint32_t lane) {
  constexpr uint32_t kCh = kRow / 16u;
  if (kCh == 4u || lane < 16u * kCh) {
    const uint32_t pk = lane / kCh, ch = lane - pk * kCh;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t p = tb + k * 16u + pk;
      const uint8_t* src = p < a.n_pkts ? a.pkts + static_cast<size_t>(p) * a.stride + ch * 16u : a.pkts;
      glds16_tile<NT>(src, buf + k * (16u * kRow));
    }
  }
}

template <bool HIST>
__device__ __forceinline__ void stream_flush(const ClassifyArgs& a, uint32_t* hist, uint32_t nbins, uint32_t part,
                                             uint32_t lane) {
  if constexpr (HIST) {
    if (a.hist16) {
      const uint32_t hw = (nbins + 1) >> 1;
      uint32_t* row = a.part_hist + static_cast<size_t>(part) * hw;
      for (uint32_t w = lane; w < hw; w += 64) {
        const uint32_t h = hist[2 * w] | (2 * w + 1 < nbins ? hist[2 * w + 1] << 16 : 0u);
        if (h) atomicAdd(&row[w], h);
      }
    } else {
      uint32_t* row = a.part_hist + static_cast<size_t>(part) * nbins;
      for (uint32_t b = lane; b < nbins; b += 64) {
        const uint32_t h = hist[b];
        if (h) atomicAdd(&row[b], h);
      }
    }
    for (uint32_t b = lane; b < nbins; b += 64) hist[b] = 0;
  }
}

// Classify one tile from its LDS ring buffer `x` (row of this lane's packet) and write the results.
// Returns the bin to count (histogram) through `bin`; false when the lane has no packet.
template <bool F4, int MODE, uint32_t kRow = row_of<MODE>(), bool WT = false>
__device__ __forceinline__ bool stream_classify(const ClassifyArgs& a, const uint8_t* lut, const uint8_t* x,
                                                uint32_t p, uint32_t& bin_out, bool& slow_out) {
  const bool valid = p < a.n_pkts;
  const uint4 c0 = *reinterpret_cast<const uint4*>(x);
  const uint4 c1 = *reinterpret_cast<const uint4*>(x + 16);
  const uint2 c2 = *reinterpret_cast<const uint2*>(x + 32);
  const bool fast = valid && ((c0.w >> 16) & 0xfu) == 5u;  // lean layout: aligned, frames >= 48 B
  // frame bytes: src 26..29, dst 30..33, ports 34..37, proto 23
  const uint32_t src = (c1.z >> 16) | (c1.w << 16);
  const uint32_t dst = (c1.w >> 16) | (c2.x << 16);
  const uint32_t ports = (c2.x >> 16) | (c2.y << 16);
  uint32_t lo, hi;
  fnv_flow(lo, hi, src, dst, ports, c1.y >> 24);
  const uint32_t idx = F4 ? mod_f4(lo, hi) : mod_barrett(lo, hi, a.m, a.mu);
  const uint32_t e = lut[idx & 0xffffu];
  bin_out = (idx >> 16) ? a.lut_tail : e;
  if constexpr (MODE == 1) {
    static_assert(kRow == 64, "the in-place swap writes whole slots back from 64-B rows");
    // whole-line write-back from the tile's LDS rows: lane (quad, part) stores chunk `part` of packet
    // 16k + quad (1 KiB contiguous per instruction), chunk 0 with the MACs swapped; a packet off
    // the fast path keeps its chunk 0 for the byte-wise path
    const uint8_t* tile = x - (p & 63u) * kRow;
    const uint32_t part = p & 3u, quad = (p & 63u) >> 2;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t q = (p & ~63u) + k * 16u + quad;
      uint4 v = *reinterpret_cast<const uint4*>(tile + (k * 16u + quad) * kRow + part * 16u);
      // the quad's chunk-0 lane holds bytes 12..15 (IHL)
      const uint32_t w3 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(v.w), 0x00, 0xf, 0xf, false));
      const bool qfast = q < a.n_pkts && ((w3 >> 16) & 0xfu) == 5u;
      if (part == 0u)
        v = make_uint4((v.y >> 16) | (v.z << 16), (v.z >> 16) | (v.x << 16), (v.x >> 16) | (v.y << 16), v.w);
      if (qfast) {
        if constexpr (WT) stg16_wt(a.pkts + static_cast<size_t>(q) * a.stride + part * 16u, v);
        else stg16_nt(a.pkts + static_cast<size_t>(q) * a.stride + part * 16u, v);
      }
    }
  } else if constexpr (MODE == 2) {
    if (fast) {
      uint32_t* mo = reinterpret_cast<uint32_t*>(a.mac_out + static_cast<size_t>(p) * 12u);
      mo[0] = (c0.y >> 16) | (c0.z << 16);
      mo[1] = (c0.z >> 16) | (c0.x << 16);
      mo[2] = (c0.x >> 16) | (c0.y << 16);
    }
  }
  slow_out = valid && !fast;
  return valid;
}

// The packet's backend (and its slow path, after the tile's next loads are issued).
template <bool F4>
__device__ __forceinline__ uint32_t stream_finish(const ClassifyArgs& a, const uint8_t* lut, uint32_t p, uint32_t bin,
                                                  bool slow) {
  if (slow) {
    uint32_t gate;
    bin = classify_slow<kLdsU8Tail, F4, false, true>(a, lut, a.pkts + static_cast<size_t>(p) * a.stride, a.fixed_len,
                                                     p, gate);
  }
  a.backend[p] = static_cast<uint16_t>(bin == a.nb ? kSentinel : bin);
  return bin;
}

// 4 or 2 B per lane from `src` into LDS at m0 + lane * 4.
__device__ __forceinline__ void glds4(const void* src, uint32_t lds_base) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_base))
      : "memory");
}
__device__ __forceinline__ void glds2(const void* src, uint32_t lds_base) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_ushort %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_base))
      : "memory");
}


// Lagged grouping (NBG_GROUP_LAG, GB > 0: the multisplit's bin bits): besides classifying its batch,
// the launch groups the handle's pending batch `lg` (classified by the previous launch, whose
// partition rows are complete).  Block c owns partition c: a prologue sums the rows into the
// partition's per-bin perm bases (group base + prefix over earlier partitions, as group_kernel's),
// then at every unit step each wave ranks 64 packets of the next 512-packet piece of the partition
// (ballot multisplit), the unit's existing LDS barrier publishes the per-wave bin counts, and every
// lane stores perm[base + run + earlier waves' counts + rank] = its packet: the stable per-group FIFO
// order of group_by.rs:46-51.  Pieces beyond the unit steps run after them.  A piece's backends
// arrive by LDS-DMA with the tile of its step (counted in `seq`), so grouping never drains the tile
// ring.  The launch then zeroes the lag histogram buffer the launch after next accumulates into
// (three buffers rotate: classify into one, group from the previous one, zero the third).
constexpr uint32_t kLagPiece = 64u * kStreamW;  // packets per piece (one 64-packet rank per wave)
constexpr uint32_t kLagSlots = 3;                // backend pieces per wave: steps k, k+1, k+2

// LDS words of the lag state past the block histograms (hstride = (nbins + 3) & ~3):
// base[hs], tot[hs], run[2][hs], cnt[2][kStreamW][hs], pbs[2][hs] (a piece's bin starts),
// kStreamW * kLagSlots pieces of 64 dwords, the block scan's per-wave sums, and srt[2][kLagPiece]
// (pos, packet) pairs of a piece sorted by bin (dynamic LDS only: the kernel may take all 160 KiB)
__host__ __device__ constexpr uint32_t lag_lds_words(uint32_t hstride) {
  return hstride * (6u + 2u * kStreamW) + kStreamW * kLagSlots * 64u + kStreamW + 2u * kLagPiece * 2u;
}

// MODE: 0 = read only, 1 = MAC swap in place, 2 = swapped MACs as 12-B records (a.mac_out)
// sb: the batches of this launch (one for nbg_maglev_classify_device; up to kMaxMulti for
// nbg_maglev_classify_device_multi).  `a` carries what they share; per unit, the unit's batch
// supplies pkts, n_pkts, backend, mac_out and part_hist (a view of `a`).  GB > 0: one batch, plus
// the lagged grouping of lg (above).
template <bool F4, bool HIST, int MODE, int GB = 0>
__global__ __launch_bounds__(kStreamNT, 1) void classify_stream_kernel(ClassifyArgs a, StreamBatches sb, LagGroup lg) {
  constexpr uint32_t kRow = stream_row_of<MODE>(), kTileLds = 64u * kRow;
  static_assert(GB == 0 || HIST, "lagged grouping runs on the per-unit histogram barrier");
  extern __shared__ __align__(16) uint8_t smem[];  // stream_lds() (after the kernel) sizes this carve-up
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t nbins = a.nb + 1;
  uint8_t* lut = smem;
  uint8_t* ring = smem + kLutLds + wave * (kRing * kTileLds);
  const uint32_t hstride = (nbins + 3) & ~3u;
  uint32_t* hist_base = reinterpret_cast<uint32_t*>(smem + kLutLds + kStreamW * kRing * kTileLds);
  const uint32_t ring_lds = __builtin_amdgcn_readfirstlane(lds_addr(ring));
  const uint32_t lut_lds = __builtin_amdgcn_readfirstlane(lds_addr(lut));
  // Interleaved units: unit u = tiles [u*W, u*W + W), one per wave; block b takes units b, b + G,
  // b + 2G, ...  At any moment the grid reads consecutive units: one sequential sweep of the batch
  // (contiguous per-wave runs read ~3k streams at a fixed stride and measured 10 % slower:
  // HBM channel imbalance).  The block's histogram is double-buffered per unit and flushed by one
  // wave behind one LDS-only barrier; a unit (W tiles = 512 packets) never straddles a partition.
  const uint32_t n_units = sb.unit_base[sb.n];
  const uint32_t G = gridDim.x, b = blockIdx.x;
  const uint32_t nt = b < n_units ? (n_units - b + G - 1) / G : 0u;  // units of this block (block-uniform)
  // position k: global unit b + k*G; its batch j (scalar search, block-uniform) and the unit's
  // first packet within the batch
  // A cursor over the batches: units [lo, hi) are batch j's.  Positions visit increasing units, so
  // a cursor only moves forward, at most n - 1 times per block: the kernel arguments are read at a
  // batch change only.  Measured (rocprof, 4 x 1M per launch, profiles/r02_multi_batch_rocprof.txt):
  // read-only 45.7 us with the cursor against 52.7 us with a per-unit search of the argument arrays.
  struct Cursor {
    uint32_t j, lo, hi;
    ClassifyArgs v;
  };
  auto load = [&](Cursor& c, uint32_t j) {
    c.j = j;
    c.lo = sb.unit_base[j];
    c.hi = sb.unit_base[j + 1];
    c.v = a;
    c.v.pkts = sb.pkts[j];
    c.v.n_pkts = sb.n_pkts[j];
    c.v.backend = sb.backend[j];
    c.v.mac_out = sb.mac_out[j];
    c.v.part_hist = sb.part_hist[j];
  };
  auto seek = [&](Cursor& c, uint32_t u) {
    if (u < c.hi) return;
    uint32_t jj = c.j + 1;
    while (jj + 1 < sb.n && u >= sb.unit_base[jj + 1]) ++jj;
    load(c, jj);
  };
  auto first_pkt = [&](const Cursor& c, uint32_t u) { return ((u - c.lo) * kStreamW + wave) * 64u; };
  Cursor cur, nxt;  // the unit being classified; the unit whose tile is issued
  load(cur, 0);
  load(nxt, 0);
  uint32_t* hist = hist_base;  // [2][hstride]
  // GB == 0: the wave's 64 backend words for the packed backend[] stores, past the histograms
  uint16_t* rep = reinterpret_cast<uint16_t*>(hist_base + 2u * hstride) + wave * 64u;

  // lagged grouping state (GB > 0): this block's partition [pbeg, pend) of the pending batch, its
  // 512-packet pieces, and the LDS words past the block histograms
  uint32_t* g_base = hist_base + 2 * hstride;   // [hstride] perm base of every bin for this partition
  uint32_t* g_tot = g_base + hstride;           // [hstride] prologue scratch: bin totals
  uint32_t* g_run = g_tot + hstride;            // [2][hstride] bin counts of earlier pieces
  uint32_t* g_cnt = g_run + 2 * hstride;        // [2][kStreamW][hstride] per-wave counts of a piece
  uint32_t* g_pbs = g_cnt + 2 * kStreamW * hstride;  // [2][hstride] where each bin starts in a sorted piece
  uint32_t* g_bk = g_pbs + 2 * hstride;         // [kStreamW][kLagSlots][64] backends (one dword per lane)
  uint32_t* s_wave = g_bk + kStreamW * kLagSlots * 64u;  // [kStreamW] block scan
  uint2* g_srt = reinterpret_cast<uint2*>(s_wave + kStreamW);  // [2][kLagPiece] (perm position, packet)
  const uint32_t bk_lds = GB > 0 ? __builtin_amdgcn_readfirstlane(lds_addr(g_bk + wave * kLagSlots * 64u)) : 0u;
  const bool g_own = GB > 0 && b < lg.n_parts;  // block-uniform
  const uint32_t pbeg = g_own ? b * lg.part_pkts : 0u;
  const uint32_t pend = g_own ? min(pbeg + lg.part_pkts, lg.n_pkts) : 0u;
  const uint32_t pieces = g_own && lg.perm ? (pend - pbeg + kLagPiece - 1) / kLagPiece : 0u;
  const bool pro = g_own && (lg.perm || b == 0);  // block-uniform; counts from block 0

  // Prologue loads (GB > 0): this partition's per-bin perm base (group base + prefix over earlier
  // partitions) is summed straight from the pending batch's partition rows (group_kernel's direct
  // scan): L threads per row word, each over rows j, j + L, ...  The first kPU rows of every thread
  // are loaded here, before the LUT pieces and the first tiles, so they retire first: the compiler's
  // waits for them (it does not see the LDS-DMA loads) never wait for the tile ring.
  constexpr uint32_t kPU = GB > 0 ? 32u : 1u;
  const uint32_t rw = lg.hist16 ? (nbins + 1) >> 1 : nbins;  // words per row
  const uint32_t pL = rw >= kStreamNT ? 1u : kStreamNT / rw;
  const uint32_t pw = tid % rw, pj = tid / rw;
  const bool pthr = pro && tid < rw * pL;
  uint32_t ph[kPU];
  if constexpr (GB > 0) {
    if (pthr) {
#pragma unroll
      for (uint32_t k = 0; k < kPU; ++k) ph[k] = ld_u32(lg.part_hist, (min(pj + k * pL, lg.n_parts - 1u) * rw + pw) * 4u);
    }
  }

  // LUT staging: lut_lds_bytes (a multiple of 1 KiB, <= 64 KiB) in 1-KiB pieces over the block's
  // waves (the device LUT is padded to whole pieces); the first tiles go out behind them
  const uint32_t pieces_lut = a.lut_lds_bytes >> 10;
  const uint32_t first = min(nt, static_cast<uint32_t>(kRing));
  // the LUT pieces first, then the first tiles (measured: tiles first, or the LUT through registers
  // off the LDS-DMA path, are both ~0.8 us slower per launch)
  for (uint32_t q = wave; q < pieces_lut; q += kStreamW)
    glds16(static_cast<const uint8_t*>(a.lut) + q * 1024u + lane * 16u, lut_lds + q * 1024u);
  // VM operations this wave issued after the LUT pieces (tile loads, and a lower bound of its
  // stores): waiting for tile k is vmcnt(seq - its count), so the stores issued after a tile do not
  // make the wait for it stricter (vmcnt counts stores too)
  uint32_t seq = 0, sA = 0, sB = 0, sC = 0;  // counts after tiles k, k+1, k+2
  // lagged grouping: piece q's 64 backends of this wave, one dword per lane (a 2-B LDS-DMA fills a
  // dword), into slot q % kLagSlots; issued just before the tile of step q, so waiting for that
  // tile covers it.  One instruction (counted) when the wave has packets in the piece.
  auto issue_piece = [&](uint32_t q) {
    if constexpr (GB > 0) {
      const uint32_t i0 = pbeg + q * kLagPiece + wave * 64u;
      if (q < pieces && i0 < pend) {
        const uint32_t i = min(i0 + lane, pend - 1u);
        glds2(lg.backend + i, bk_lds + (q % kLagSlots) * 256u);
        ++seq;
      }
    }
  };
  for (uint32_t k = 0; k < first; ++k) {
    const uint32_t u = b + k * G;
    seek(nxt, u);
    issue_piece(k);
    issue_tile<kRow, MODE != 2>(nxt.v, first_pkt(nxt, u), ring_lds + k * kTileLds, lane);
    seq += 4;
    (k == 0 ? sA : (k == 1 ? sB : sC)) = seq;
  }
  if constexpr (HIST)
    for (uint32_t i = tid; i < 2 * hstride; i += kStreamNT) hist[i] = 0;
  if constexpr (GB > 0) {
    if (pro) {  // the sums, while the LUT pieces and the first tiles are in flight
      for (uint32_t i = tid; i < hstride; i += kStreamNT) {
        g_base[i] = 0;
        g_tot[i] = 0;
        g_run[i] = 0;
      }
      lds_sync();
      const uint32_t c = b;
      if (pthr) {
        uint32_t pre_lo = 0, pre_hi = 0, all_lo = 0, all_hi = 0;
        auto add = [&](uint32_t q, uint32_t h) {
          const uint32_t lo = !lg.hist16 ? h : (h & 0xffffu), hi = lg.hist16 ? h >> 16 : 0u;
          const bool in = q < lg.n_parts;
          all_lo += in ? lo : 0u;
          all_hi += in ? hi : 0u;
          pre_lo += in && q < c ? lo : 0u;
          pre_hi += in && q < c ? hi : 0u;
        };
#pragma unroll
        for (uint32_t k = 0; k < kPU; ++k) add(pj + k * pL, ph[k]);
        for (uint32_t q = pj + kPU * pL; q < lg.n_parts; q += pL)  // rows past the first kPU (rare)
          add(q, ld_u32(lg.part_hist, (q * rw + pw) * 4u));
        const uint32_t b0 = lg.hist16 ? 2 * pw : pw;
        if (pre_lo) atomicAdd(&g_base[b0], pre_lo);
        if (all_lo) atomicAdd(&g_tot[b0], all_lo);
        if (lg.hist16 && b0 + 1 < nbins) {
          if (pre_hi) atomicAdd(&g_base[b0 + 1], pre_hi);
          if (all_hi) atomicAdd(&g_tot[b0 + 1], all_hi);
        }
      }
      lds_sync();
      // group bases: exclusive scan of the totals over bins (<= 2^GB bins: <= 512 = one per thread)
      static_assert((1u << GB) <= kStreamNT, "one bin per thread in the group-base scan");
      const uint32_t t = tid < nbins ? g_tot[tid] : 0u;
      uint32_t all;
      const uint32_t gb = block_excl_scan_n<kStreamNT>(t, s_wave, all);
      if (tid < nbins) {
        if (c == 0 && lg.counts) lg.counts[tid] = t;
        g_base[tid] += gb;
      }
    }
  }
  // this wave's LUT pieces are in when at most its tile loads are outstanding; then the barrier
  // makes every wave's pieces visible to every wave
  wait_tile(first);
  lds_sync();

  // Lagged grouping of piece q runs across three barriers, so that every barrier the unit loop already
  // has carries it (sync point s = the loop step, then tail barriers):
  //   before barrier q:  rank the wave's 64 packets (ballot multisplit), publish the wave's bin counts
  //   after barrier q:   each packet's perm position (base + earlier pieces + earlier waves + rank);
  //                      one wave: the next piece's running counts and this piece's bin starts (pbs)
  //   after barrier q+1: each packet's slot in the piece sorted by bin (pbs + earlier waves + rank)
  //   after barrier q+2: thread t stores sorted slot t: consecutive threads write consecutive perm
  //                      entries of one bin (coalesced), where lane-order stores scattered every lane
  uint32_t g_bin = 0, g_rank = 0;    // piece q (ranked, before barrier q)
  bool g_valid = false;
  uint32_t p_pos = 0, p_bin = 0, p_pre = 0;  // piece q-1 (positioned, after barrier q-1)
  bool p_valid = false;
  auto piece_rank = [&](uint32_t q) {  // before barrier q
    if constexpr (GB > 0) {
      const uint32_t i = pbeg + q * kLagPiece + wave * 64u + lane;
      g_valid = i < pend;
      const uint32_t raw = g_bk[(wave * kLagSlots + q % kLagSlots) * 64u + lane] & 0xffffu;
      g_bin = g_valid ? (raw == NBG_SENTINEL ? a.nb : raw) : 0u;
      uint32_t count;
      wave_match_rank<GB>(g_bin, g_valid, lane, g_rank, count);
      uint32_t* row = g_cnt + ((q & 1u) * kStreamW + wave) * hstride;
      for (uint32_t j = lane; j < hstride; j += 64) row[j] = 0;
      __builtin_amdgcn_wave_barrier();
      if (g_valid) row[g_bin] = count;  // every lane of a bin stores the same count
    }
  };
  auto piece_sync = [&](uint32_t s) {  // after barrier s
    if constexpr (GB > 0) {
      // piece s-2: coalesced stores of its sorted slots
      if (s >= 2 && s - 2 < pieces) {
        const uint32_t q = s - 2, n_q = min(pend - (pbeg + q * kLagPiece), kLagPiece);
        const uint2 e = g_srt[(q & 1u) * kLagPiece + tid];
        if (tid < n_q && e.x < lg.n_pkts) lg.perm[e.x] = e.y;
        if (wave * 64u < n_q) ++seq;  // lane 0 stored
      }
      // piece s-1: its sorted slot
      if (s >= 1 && s - 1 < pieces && p_valid) {
        const uint32_t q = s - 1;
        const uint32_t slot = g_pbs[(q & 1u) * hstride + p_bin] + p_pre;
        g_srt[(q & 1u) * kLagPiece + slot] = make_uint2(p_pos, pbeg + q * kLagPiece + wave * 64u + lane);
      }
      // piece s: perm positions; one wave: running counts and bin starts
      if (s < pieces) {
        const uint32_t* cq = g_cnt + (s & 1u) * kStreamW * hstride;
        uint32_t pre = g_rank;
#pragma unroll
        for (uint32_t w = 0; w < kStreamW; ++w)
          if (w < wave) pre += cq[w * hstride + g_bin];
        p_pos = g_base[g_bin] + g_run[(s & 1u) * hstride + g_bin] + pre;
        p_bin = g_bin;
        p_pre = pre;
        p_valid = g_valid;
        if (wave == (s + kStreamW / 2) % kStreamW) {
          constexpr uint32_t kB = (1u << GB) / 64u;  // consecutive bins per lane
          uint32_t pc[kB], tot = 0;
#pragma unroll
          for (uint32_t i = 0; i < kB; ++i) {
            const uint32_t bn = lane * kB + i;
            uint32_t v = 0;
            if (bn < nbins) {
#pragma unroll
              for (uint32_t w = 0; w < kStreamW; ++w) v += cq[w * hstride + bn];
              g_run[((s + 1) & 1u) * hstride + bn] = g_run[(s & 1u) * hstride + bn] + v;
            }
            pc[i] = v;
            tot += v;
          }
          uint32_t st = wave_incl_scan(tot) - tot;
#pragma unroll
          for (uint32_t i = 0; i < kB; ++i) {
            const uint32_t bn = lane * kB + i;
            if (bn < nbins) g_pbs[(s & 1u) * hstride + bn] = st;
            st += pc[i];
          }
        }
      } else {
        p_valid = false;
      }
    }
  };

  for (uint32_t k = 0; k < nt; ++k) {
    const uint32_t u = b + k * G;
    seek(cur, u);
    const ClassifyArgs& aj = cur.v;
    const uint32_t tb = first_pkt(cur, u);
    wait_vm_n(seq - sA);  // kStreamAhead tiles (and their stores) stay in flight
    const uint32_t p = tb + lane;
    uint32_t bin = 0;
    bool slow = false;
    const bool valid = tb < aj.n_pkts && stream_classify<F4, MODE, kRow>(aj, lut, ring + (k % kRing) * kTileLds + lane * kRow,
                                                                    p, bin, slow);
    // tile k + kRing into the buffer just read (its ds_reads are consumed above): while the next
    // tile is classified, kStreamAhead tiles stay in flight
    uint32_t sN = 0;
    if (k + kRing < nt) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const uint32_t u2 = u + kRing * G;
      seek(nxt, u2);
      issue_piece(k + kRing);
      issue_tile<kRow, MODE != 2>(nxt.v, first_pkt(nxt, u2), ring_lds + (k % kRing) * kTileLds, lane);
      seq += 4;
      sN = seq;
    }
    if constexpr (GB == 0) {
      // backend[]: a whole tile's 128 B go out as 16-B stores of lanes 0..7 (through the wave's LDS
      // words, as the ring kernel does) instead of 64 2-B stores: in place 93.2-93.8 against
      // 94.0-94.5 us per 4 x 1M launch (profiles/r05_stream_pack_ab.txt)
      uint32_t be = 0;
      if (valid) {
        if (slow) {
          uint32_t gate;
          bin = classify_slow<kLdsU8Tail, F4, false, true>(aj, lut, aj.pkts + static_cast<size_t>(p) * aj.stride,
                                                           aj.fixed_len, p, gate);
        }
        be = bin == aj.nb ? kSentinel : bin;
        if constexpr (HIST) atomicAdd(&hist[(k & 1u) * hstride + bin], 1u);
      }
      if (tb + 64u <= aj.n_pkts && (reinterpret_cast<uintptr_t>(aj.backend) & 15u) == 0) {
        rep[lane] = static_cast<uint16_t>(be);
        asm volatile("" ::: "memory");  // the u16 writes before the 16-B reads of the same words
        __builtin_amdgcn_wave_barrier();
        const uint4 w = reinterpret_cast<const uint4*>(rep)[lane & 7u];
        if (lane < 8u) *reinterpret_cast<uint4*>(aj.backend + tb + lane * 8u) = w;
      } else if (valid) {
        aj.backend[p] = static_cast<uint16_t>(be);
      }
    } else if (valid) {
      bin = stream_finish<F4>(aj, lut, p, bin, slow);
      if constexpr (HIST) atomicAdd(&hist[(k & 1u) * hstride + bin], 1u);
    }
    if (tb < aj.n_pkts) ++seq;  // the backend store (one instruction; lane 0 has a packet)
    if (k < pieces) piece_rank(k);
    sA = sB;
    if constexpr (kRing == 2) {
      sB = sN;
    } else {
      sB = sC;
      sC = sN;
    }
    if constexpr (HIST) {
      // every wave's counts of unit k are in hist[k & 1]; one wave flushes it into the unit's
      // partition row and zeroes it.  The next barrier (unit k + 1) orders that before unit k + 2
      // counts into the same buffer.
      lds_sync();
      if (wave == k % kStreamW) {
        uint32_t* h = hist + (k & 1u) * hstride;
        stream_flush<HIST>(aj, h, nbins, ((u - cur.lo) * kStreamW * 64u) / a.part_pkts, lane);
      }
    }
    piece_sync(k);
  }
  if constexpr (GB > 0) {
    // sync points past the unit steps: pieces beyond them (a pending batch larger than this one),
    // then the last two pieces' sorted slots and stores
    {
      for (uint32_t s = nt; s < pieces + 2; ++s) {
        if (s < pieces) {
          issue_piece(s);
          wait_vm<0>();
          piece_rank(s);
        }
        lds_sync();
        piece_sync(s);
      }
    }
    for (uint32_t i = b * kStreamNT + tid; i < lg.zero_words; i += G * kStreamNT) lg.zero[i] = 0;
  }
}

}  // namespace

// classify_stream_kernel's dynamic LDS as it is carved up at its top: the LUT, kRing tile buffers per
// wave, two block histograms, then the lag state (lag_lds_words) or the waves' backend words.
size_t stream_lds(uint32_t nb, int mode, bool lag) {
  const uint32_t hstride = ((nb + 1) + 3) & ~3u;
  const size_t tile = 64u * (mode == 1 ? stream_row_of<1>() : stream_row_of<0>());
  // past the histograms: the lag state, or the waves' backend words (64 x 2 B each)
  const size_t words = 2 * hstride + (lag ? lag_lds_words(hstride) : kStreamW * 32u);
  return kLutLds + static_cast<size_t>(kStreamW) * kRing * tile + words * 4u;
}

int stream_waves_per_block() { return kStreamW; }

namespace {

// ---- persistent RX-ring classify (nbg_ring_*) ----------------------------------------------------
//
// One launch per ring for the whole run: the RX ring that never stops (ReceiveBatch polling its port,
// framework/src/operators/receive_batch.rs:26,52-61).  Same blocks, LUT staging, LDS-DMA tile ring
// and interleaved 512-packet units as classify_stream_kernel, but the unit sequence is open-ended:
// batch j covers units [ulo_j, uhi_j) of one sequence, block b takes units b, b + G, b + 2G, ... of
// it, and batches arrive through a descriptor ring in pinned host memory while the kernel runs.  So
// the LUT is staged once per ring and the tile pipeline runs across batch boundaries without a
// ramp.
//
//   Descriptors.  The control wave (the ninth) of every block keeps up to kRingCache batch
//   descriptors in LDS.  It prefetches the next kRingFetch slots of its replica of the device ring
//   (uncached HBM, filled from the host's ring by the relay block, ring_relay) by LDS-DMA; a slot is taken
//   once its seq and check match (a read that overlaps the relay rewriting the slot fails the check
//   and is retried).  The count of known batches is published through a step-parity LDS word behind
//   the unit barrier, so every wave sees the same count.  When the block has no tile to classify
//   (the next unit is in no known batch) it drains and the control wave polls the slot (and the
//   device stop word) with s_sleep between polls: the idle path.  No classify CU reads host memory.
//   Exit: stop set and nothing posted, or idle_ticks without a new batch (the exit condition every
//   wave reaches when the host goes away).
//
//   Completion.  Outputs are stored write-through (sc1: backend[] packed 16 B per lane, the in-place
//   windows 16 B per lane), so a store that retired is in HBM.  In-order vmcnt: once every wave has
//   waited for tile k (the unit barrier of step k), the stores of steps <= k - 3 retired.  The
//   control wave then publishes, per block, the count of batches all of whose units of this block
//   are complete (to uncached HBM, when the count changes); the relay reports the minimum to the host.
constexpr uint32_t kRingCache = 4;  // batch descriptors in LDS (from the current unit's batch on)
constexpr uint32_t kRingFetch = 2;  // ring slots per prefetch (one LDS-DMA dword load, 32 lanes)
constexpr uint32_t kRingCtlWords = kRingCache * 16u + kRingFetch * 16u + 4u + kStreamW * 32u + 16u;

__device__ __forceinline__ void glds4_sys(const void* src, uint32_t lds_base) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %1, off sc0 sc1\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_base))
      : "memory");
}

__device__ __forceinline__ uint32_t rfl(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }


// The ring kernel's cursor over the known batches (block-uniform; loaded from the LDS descriptor cache)
struct RingCursor {
  uint32_t j;  // batch index (0xffffffff: none yet)
  uint64_t lo, hi;
  uint8_t* pkts;
  uint16_t* backend;
  uint32_t n;
};

__device__ __forceinline__ void ring_load(RingCursor& c, const uint32_t* cache, uint32_t j) {
  const uint32_t* e = cache + (j % kRingCache) * 16u;
  c.j = j;
  c.pkts = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(rfl(e[0])) | static_cast<uintptr_t>(rfl(e[1])) << 32);
  c.backend = reinterpret_cast<uint16_t*>(static_cast<uintptr_t>(rfl(e[2])) | static_cast<uintptr_t>(rfl(e[3])) << 32);
  c.lo = static_cast<uint64_t>(rfl(e[4])) | static_cast<uint64_t>(rfl(e[5])) << 32;
  c.hi = static_cast<uint64_t>(rfl(e[6])) | static_cast<uint64_t>(rfl(e[7])) << 32;
  c.n = rfl(e[8]);
}

// Move c forward to the batch holding unit u; false when u lies past the known batches.
__device__ __forceinline__ bool ring_seek(RingCursor& c, const uint32_t* cache, uint64_t u, uint32_t known) {
  while (u >= c.hi) {
    const uint32_t nj = c.j + 1u;
    if (static_cast<int32_t>(nj - known) >= 0) return false;
    ring_load(c, cache, nj);
  }
  return true;
}

// Take the staged descriptor d (every lane reads its 16 words) as batch known_w if it is that batch
// (seq and check match) and the cache has room past `base` (the oldest batch a cursor may still load).
__device__ __forceinline__ bool ring_take(const uint32_t* d, uint32_t* cache, uint32_t& known_w, uint32_t base,
                                          uint32_t lane) {
  const uint4 w0 = *reinterpret_cast<const uint4*>(d), w1 = *reinterpret_cast<const uint4*>(d + 4);
  const uint4 w2 = *reinterpret_cast<const uint4*>(d + 8), w3 = *reinterpret_cast<const uint4*>(d + 12);
  const uint64_t pk = w0.x | static_cast<uint64_t>(w0.y) << 32, be = w0.z | static_cast<uint64_t>(w0.w) << 32;
  const uint64_t lo = w1.x | static_cast<uint64_t>(w1.y) << 32, hi = w1.z | static_cast<uint64_t>(w1.w) << 32;
  const uint64_t ck = w3.z | static_cast<uint64_t>(w3.w) << 32;
  const bool ok = w2.y == known_w + 1u && ck == ring_check(pk, be, lo, hi, w2.x, w2.y) && known_w - base < kRingCache;
  if (!rfl(ok ? 1u : 0u)) return false;
  // copy the words just checked (d may be rewritten by a landing prefetch meanwhile)
  const uint4 q = (lane >> 2) == 0 ? w0 : ((lane >> 2) == 1 ? w1 : ((lane >> 2) == 2 ? w2 : w3));
  const uint32_t x = (lane & 3u) == 0 ? q.x : ((lane & 3u) == 1 ? q.y : ((lane & 3u) == 2 ? q.z : q.w));
  if (lane < 16) cache[(known_w % kRingCache) * 16u + lane] = x;
  ++known_w;
  return true;
}

// Batch j's descriptor in this block's replica of the ring.
__device__ __forceinline__ const RingDesc* ring_slot(const RingArgs& r, uint32_t j) {
  return r.desc + (blockIdx.x & (r.reps - 1u)) * r.slots + (j & (r.slots - 1u));
}

// Wave 0, idle: read ring slots (and the stop word) until a new batch is taken; true = exit (stop
// with nothing posted, or idle_ticks without a batch: then the error word is set).
__device__ __forceinline__ bool ring_poll(const RingArgs& r, uint32_t* stage, uint32_t* cache, uint32_t& known_w,
                                          uint32_t base, uint32_t lane) {
  const uint64_t t0 = wall_clock64();
  const uint32_t known0 = known_w;
  for (uint32_t nap = 1;; nap = min(2u * nap, 16u)) {
    for (;;) {  // every consecutive batch that is posted (and fits)
      const uint32_t* slot = reinterpret_cast<const uint32_t*>(ring_slot(r, known_w));
      if (lane < 16) stage[lane] = __hip_atomic_load(slot + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __builtin_amdgcn_wave_barrier();
      if (!ring_take(stage, cache, known_w, base, lane)) break;
    }
    if (known_w != known0) return false;
    if (rfl(__hip_atomic_load(r.dstop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))) {
      // a batch posted before the stop is in its slot by now: look once more
      const uint32_t* slot = reinterpret_cast<const uint32_t*>(ring_slot(r, known_w));
      if (lane < 16) stage[lane] = __hip_atomic_load(slot + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __builtin_amdgcn_wave_barrier();
      return !ring_take(stage, cache, known_w, base, lane);
    }
    if (static_cast<uint64_t>(wall_clock64()) - t0 > r.idle_ticks) {
      if (lane == 0) __hip_atomic_store(&r.ctl->error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return true;
    }
    // back off to 16 x 512 clocks (~3.5 us) between polls of the (uncached) device ring
    for (uint32_t i = 0; i < nap; ++i) __builtin_amdgcn_s_sleep(8);
  }
}

// The ring's relay: wave 0 of the classify kernel's last block (the other waves of that block exit),
// so its PCIe reads of the host ring hold no classify CU.  (A separate one-wave kernel measured no
// good: blocks go to XCDs round-robin and never move, so the XCD that hosted it had one classify
// block too many for its CUs, and that block never became resident.)
// Loop: copy every newly posted host slot (seq and check match) into each replica of the uncached
// device ring; report the minimum of the blocks' completion counts to the host when it moves; on
// the host's stop, relay what was posted before it, then raise the device stop word and exit once
// every relayed batch is complete; on idle_ticks without a post or a completion, raise the device
// stop word and the host error word and exit (the exit every path reaches when the host goes away).
__device__ __forceinline__ void ring_relay(const RingArgs& r, uint32_t lane) {
  uint32_t known = 0, done = 0, nap = 1;
  bool stopping = false, stopped = false;
  uint64_t t_act = wall_clock64();
  for (;;) {
    bool moved = false;
    for (;;) {  // every consecutive posted slot
      const uint32_t* hs = reinterpret_cast<const uint32_t*>(r.hdesc + (known & (r.slots - 1u)));
      const uint32_t x = lane < 16u ? __hip_atomic_load(hs + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
      uint32_t w[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) w[i] = __shfl(x, i);
      const uint64_t pk = w[0] | static_cast<uint64_t>(w[1]) << 32, be = w[2] | static_cast<uint64_t>(w[3]) << 32;
      const uint64_t lo = w[4] | static_cast<uint64_t>(w[5]) << 32, hi = w[6] | static_cast<uint64_t>(w[7]) << 32;
      const uint64_t ck = w[14] | static_cast<uint64_t>(w[15]) << 32;
      if (!(w[9] == known + 1u && ck == ring_check(pk, be, lo, hi, w[8], w[9]))) break;
      for (uint32_t q = lane >> 4; q < r.reps; q += 4u) {
        uint32_t* d = reinterpret_cast<uint32_t*>(r.desc + q * r.slots + (known & (r.slots - 1u)));
        __hip_atomic_store(d + (lane & 15u), __shfl(x, static_cast<int>(lane & 15u)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
      }
      ++known;
      moved = true;
    }
    // completion: the slowest block
    uint32_t lag = 0;
    for (uint32_t b = lane; b < r.grid; b += 64u)
      lag = max(lag, known - __hip_atomic_load(r.prog + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lag = max(lag, static_cast<uint32_t>(__shfl_xor(static_cast<int>(lag), o)));
    const uint32_t c = known - rfl(lag);
    if (c != done) {
      done = c;
      if (lane == 0) {
        __hip_atomic_store(r.dcomp, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // the gate kernels
        __hip_atomic_store(&r.ctl->completed, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      moved = true;
    }
    if (moved) {
      t_act = wall_clock64();
      nap = 1;
      continue;
    }
    if (stopped) {
      if (done == known) break;  // every relayed batch is complete; the blocks exit on the stop word
    } else if (rfl(__hip_atomic_load(&r.ctl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))) {
      if (stopping) {
        // the slots were read once more after the stop was seen: everything posted before it is
        // relayed; the descriptors are in memory before the stop word
        wait_vm<0>();
        if (lane == 0) __hip_atomic_store(r.dstop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        stopped = true;
        continue;
      }
      stopping = true;
      continue;
    }
    if (static_cast<uint64_t>(wall_clock64()) - t_act > r.idle_ticks) {
      if (lane == 0) {
        __hip_atomic_store(r.dstop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (done != known || !stopped) __hip_atomic_store(&r.ctl->error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      break;
    }
    for (uint32_t i = 0; i < nap; ++i) __builtin_amdgcn_s_sleep(4);
    nap = min(2u * nap, 8u);
  }
}

constexpr int kRingNT = kStreamNT + 64;  // the tile waves plus the control wave

template <bool F4, int MODE>
__global__ __launch_bounds__(kRingNT, 1) void classify_ring_kernel(ClassifyArgs a, RingArgs r) {
  static_assert(MODE == 0 || MODE == 1, "the ring classifies read only or in place");
  constexpr uint32_t kRow = stream_row_of<MODE>(), kTileLds = 64u * kRow;
  extern __shared__ __align__(16) uint8_t smem[];  // ring_lds() (after the kernel) sizes this carve-up
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = rfl(tid >> 6);
  // the control wave (the last) fetches descriptors, publishes completion and polls when idle: its
  // PCIe reads are in no tile wave's vmcnt, so a slow read never holds a tile wait
  const bool ctl = wave == static_cast<uint32_t>(kStreamW);
  uint8_t* lut = smem;
  uint8_t* ring = smem + kLutLds + (ctl ? 0u : wave) * (kRing * kTileLds);
  uint32_t* cache = reinterpret_cast<uint32_t*>(smem + kLutLds + kStreamW * kRing * kTileLds);  // [kRingCache][16]
  uint32_t* stage = cache + kRingCache * 16u;   // [kRingFetch][16] the control wave's prefetch landing area
  uint32_t* known_l = stage + kRingFetch * 16u;  // [2] known batches, by step parity; [2] exit
  uint16_t* rep = reinterpret_cast<uint16_t*>(known_l + 4) + (ctl ? 0u : wave) * 64u;  // a tile wave's 64 backends
  const uint32_t ring_lds = rfl(lds_addr(ring)), lut_lds = rfl(lds_addr(lut)), stage_lds = rfl(lds_addr(stage));
  if (blockIdx.x == r.grid) {  // the relay block
    if (wave == 0) ring_relay(r, lane);
    return;
  }
  const uint32_t G = r.grid, b = blockIdx.x;
  const uint32_t pieces_lut = ctl ? 0u : a.lut_lds_bytes >> 10;
  for (uint32_t q = wave; q < pieces_lut; q += kStreamW)
    glds16(static_cast<const uint8_t*>(a.lut) + q * 1024u + lane * 16u, lut_lds + q * 1024u);
  if (tid < 4) known_l[tid] = 0;
  wait_vm<0>();
  lds_sync();

  // cursors (every wave keeps them): the unit being classified, and the unit whose tile is issued
  RingCursor cur{0xffffffffu, 0, 0, nullptr, nullptr, 0}, nxt = cur;
  const uint64_t Gu = G;
  uint32_t k = 0, iss = 0;                   // unit steps of this block classified / issued
  uint32_t seq = 0, sA = 0, sB = 0, sC = 0;  // VM operations issued; counts after tiles k, k+1, k+2
  // the control wave's descriptor state
  uint32_t known_w = 0, pf_base = 0, last_pf = 0, pub = 0;
  bool pf = false;
  uint32_t hA = 0xffffffffu, hB = 0xffffffffu, hC = 0xffffffffu;  // batch of the unit of steps k - 1, k - 2, k - 3
  // a step's backends are stored one step late, behind the next tile issue: the wait for a tile then
  // covers the write-through stores of four steps back, not three, so their longer acks stay off the
  // critical path
  uint4 pw = make_uint4(0, 0, 0, 0);
  uint16_t* pp = nullptr;
  bool pend = false;

// the tile of unit step `t` into ring buffer t % kRing (the issue cursor moves to its batch; the
// control wave only moves its cursor)
#define RING_ISSUE(t, ok)                                                                                    \
  {                                                                                                         \
    const uint64_t u_ = b + static_cast<uint64_t>(t) * Gu;                                                  \
    ok = ring_seek(nxt, cache, u_, known);                                                                  \
    if (ok) {                                                                                               \
      if (!ctl) {                                                                                           \
        ClassifyArgs v_ = a;                                                                                \
        v_.pkts = nxt.pkts;                                                                                 \
        v_.n_pkts = nxt.n;                                                                                  \
        issue_tile<kRow, true>(v_, static_cast<uint32_t>(((u_ - nxt.lo) * kStreamW + wave) * 64u),         \
                               ring_lds + (rfl(t) % kRing) * kTileLds, lane);                               \
        seq += 4;                                                                                           \
        const uint32_t d_ = (t) - k;                                                                        \
        if (d_ == 0) sA = seq;                                                                              \
        else if (d_ == 1) sB = seq;                                                                         \
        else sC = seq;                                                                                      \
      }                                                                                                     \
      ++iss;                                                                                                \
    }                                                                                                       \
  }
// batches < v complete for this block (the control wave; one system-scope store when the count moves)
#define RING_PUBLISH(v)                                                                                      \
  {                                                                                                         \
    const uint32_t v_ = (v);                                                                                \
    if (static_cast<int32_t>(v_ - pub) > 0) {                                                               \
      pub = v_;                                                                                             \
      if (lane == 0) __hip_atomic_store(r.prog + b, v_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);       \
    }                                                                                                       \
  }
// take what has landed of the control wave's prefetch (the LDS-DMA may still be in flight: a slot not
// yet landed, torn, or not yet posted fails ring_take's seq / check test and is fetched again)
#define RING_TAKE_STAGED(base)                                                                               \
  {                                                                                                         \
    uint32_t i_ = 0;                                                                                        \
    for (; i_ < kRingFetch && pf_base + i_ == known_w; ++i_)                                                \
      if (!ring_take(stage + i_ * 16u, cache, known_w, (base), lane)) break;                               \
    if (i_ == kRingFetch) pf = false;                                                                       \
  }

  for (;;) {
    const uint32_t known = rfl(known_l[k & 1u]);  // block-uniform: written before the last barrier
    for (bool ok = true; ok && iss < k + kRing;) RING_ISSUE(iss, ok)
    if (iss == k) {
      // nothing to classify: drain, then the control wave fetches descriptors (polling while none is
      // posted).  No issued unit waits for cur, so it takes nxt's place: the descriptor cache then
      // only keeps batches past the issue cursor (which has walked every known batch), and a block
      // with no unit in several small batches still gets room to take the next ones.
      cur = nxt;
      if (pend) {
        if (lane < 8u) stg16_wt(pp, pw);
        pend = false;
      }
      wait_vm<0>();
      lds_sync();
      if (ctl) {
        const uint32_t base = cur.j == 0xffffffffu ? 0u : cur.j;
        if (pf) {  // landed (vmcnt(0) above)
          RING_TAKE_STAGED(base)
          pf = false;
        }
        RING_PUBLISH(known)  // every unit of this block in batches < known is complete
        const bool ex = known_w == known && ring_poll(r, stage, cache, known_w, base, lane);
        if (lane == 0) {
          known_l[k & 1u] = known_w;
          known_l[2] = ex ? 1u : 0u;
        }
      }
      lds_sync();
      if (rfl(known_l[2])) break;
      continue;
    }
    const uint64_t u = b + static_cast<uint64_t>(k) * Gu;
    ring_seek(cur, cache, u, known);
    const uint32_t h0 = cur.j;
    if (ctl) {
      // descriptor prefetch: take what has landed, then fetch the next slots when the issue cursor
      // is within two batches of the known ones (again after 6 steps when they were not posted yet)
      if (pf) {
        const uint32_t kw0 = known_w;
        RING_TAKE_STAGED(cur.j)
        if (known_w == kw0 && k - last_pf >= 6u) {
          pf = false;
        }
      }
      if (!pf && known_w - cur.j < kRingCache && known_w - nxt.j <= 2u) {
        if (lane < 16u * kRingFetch) stage[lane] = 0u;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pf_base = known_w;
        if (lane < 16u * kRingFetch)
          glds4_sys(reinterpret_cast<const uint32_t*>(ring_slot(r, known_w + lane / 16u)) + (lane & 15u), stage_lds);
        pf = true;
        last_pf = k;
      }
      if (lane == 0) known_l[(k + 1u) & 1u] = known_w;
    } else {
      wait_vm_n(seq - sA);
      ClassifyArgs v = a;
      v.pkts = cur.pkts;
      v.n_pkts = cur.n;
      v.backend = cur.backend;
      const uint32_t tb = static_cast<uint32_t>(((u - cur.lo) * kStreamW + wave) * 64u);
      const uint32_t p = tb + lane;
      uint32_t bin = 0;
      bool slow = false;
      const bool valid = tb < v.n_pkts && stream_classify<F4, MODE, kRow, true>(
                                              v, lut, ring + (k % kRing) * kTileLds + lane * kRow, p, bin, slow);
      if (iss == k + kRing) {  // the next tile into the buffer just read
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        bool ok;
        RING_ISSUE(iss, ok)
      }
      if (pend) {  // the previous step's backends
        if (lane < 8u) stg16_wt(pp, pw);
        ++seq;
        pend = false;
      }
      if (valid && slow) {
        uint32_t gate;
        bin = classify_slow<kLdsU8Tail, F4, false, true, true>(v, lut, v.pkts + static_cast<size_t>(p) * v.stride,
                                                               v.fixed_len, p, gate);
      }
      if (tb < v.n_pkts) {
        const uint16_t be = static_cast<uint16_t>(bin == a.nb ? kSentinel : bin);
        const uint32_t cnt = min(64u, v.n_pkts - tb);
        if (cnt == 64u) {  // 16 B per lane: lanes 0..7 store the wave's 128 B (next step)
          rep[lane] = be;
          asm volatile("" ::: "memory");  // the u16 writes before the 16-B reads of the same words
          __builtin_amdgcn_wave_barrier();
          pw = reinterpret_cast<const uint4*>(rep)[lane & 7u];
          pp = v.backend + tb + (lane & 7u) * 8u;
          pend = true;
        } else {
          if (valid)
            __hip_atomic_store((__attribute__((address_space(1))) uint16_t*)(v.backend + p), be, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
          ++seq;
        }
      }
    }
    lds_sync();
    // every tile wave has waited for tile k: the stores of steps <= k - 4 retired (the backends of
    // step k - 3 went out behind tile k's issue)
    if (ctl && hC != 0xffffffffu) RING_PUBLISH(hC)
    hC = hB;
    hB = hA;
    hA = h0;
    sA = sB;
    sB = sC;
    ++k;
  }
#undef RING_ISSUE
#undef RING_PUBLISH
#undef RING_TAKE_STAGED
  // the block's exit, once every wave's stores have retired: a gate kernel waiting for a batch this
  // ring will never complete (stop, idle exit) returns when every classify block has exited
  wait_vm<0>();
  lds_sync();
  if (tid == 0) __hip_atomic_fetch_add(r.dexit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

// classify_ring_kernel's dynamic LDS as it is carved up at its top: the LUT, kRing tile buffers per tile
// wave, then kRingCtlWords (descriptor cache, prefetch stage, the known / exit words, the waves' backends).
size_t ring_lds(int mode) {
  const size_t tile = 64u * (mode == 1 ? stream_row_of<1>() : stream_row_of<0>());
  return kLutLds + static_cast<size_t>(kStreamW) * kRing * tile + kRingCtlWords * 4u;
}

namespace {

// The gate of a ring batch's grouping (nbg_ring_group before the batch is complete): one wave that
// polls the relay's completion word in uncached HBM and returns once batch target - 1 is complete,
// or once every classify block has exited (the ring ended; the grouping then reads what backend[]
// holds, which no kernel writes any more).  Every path ends: the ring itself always ends (stop or
// idle_ms).  Launched ahead of the batch's hist / group kernels on the caller's stream, so the
// producer needs no host poll between the ring's completion and the grouping.
__global__ __launch_bounds__(64) void ring_gate_kernel(const uint32_t* dcomp, const uint32_t* dexit, uint32_t target,
                                                       uint32_t grid) {
  for (uint32_t nap = 1;; nap = min(2u * nap, 4u)) {
    const uint32_t c = rfl(__hip_atomic_load(dcomp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
    if (static_cast<int32_t>(c - target) >= 0) return;
    if (rfl(__hip_atomic_load(dexit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) >= grid) return;
    for (uint32_t i = 0; i < nap; ++i) __builtin_amdgcn_s_sleep(2);
  }
}

// ---- streaming classify for descriptor layouts (IMIX: u32 offsets + u16 lengths, owned windows) ----
//
// Configs C5 (the lpm -> maglev chain: u8 LUT in LDS, tbl24 gathered) and the IMIX read-only /
// record layouts (u8 LUT in LDS or the u16 LUT gathered).  Same block structure as
// classify_stream_kernel (one block per CU, interleaved units, per-unit block histogram).  Per wave,
// everything global arrives by LDS-DMA: the descriptors of a tile (off[64], len[64]) issued four
// tiles ahead, the packet windows of a tile from its descriptors three tiles ahead, and the per-packet
// gather (tbl24 or LUT entry, 2 B per lane) one tile ahead — so iteration k hashes tile k+1 and
// issues its gather, then finishes tile k, whose gather had a whole iteration to land.  The chain's
// second, dependent gather (tbl_long, routes longer than /24) is issued at the start of iteration k
// and waited for after tile k+1's hash and prefetches, so it never drains them.  Opt-in
// (NBG_STREAM_DESC): one block per CU holds all LDS, so several streams' kernels cannot co-run.
//
// vmcnt retires in issue order and hipcc does not count these loads, so the kernel keeps its own
// wave-uniform count of issued VM operations (`seq`): each load group records the count after it,
// and waiting for one is vmcnt(seq - recorded).  Every store instruction is issued by every lane
// (lanes with nothing to store write to a scratch sink), so the count of stores per tile is a
// known lower bound; uncounted operations (byte-wise path, histogram flush) only ever make a wait
// stricter.
// A 1- or 2-B LDS-DMA load still fills one dword per lane (measured: lane i's value at 4i), so the
// u16 lengths and gathered entries take 4 B of LDS per lane.
constexpr uint32_t kDescRing = 4;                   // descriptor slots per wave: tiles k .. k+3, then k+4 into k's
constexpr uint32_t kDescLds = 64u * 4u + 64u * 4u;  // off[64] then len[64] (dword per lane)
constexpr uint32_t kGatherLds = 64u * 4u;           // one dword per lane, two tiles

template <int MODE>
__host__ __device__ constexpr uint32_t desc_ring_tiles() { return MODE == 1 ? 4u : 3u; }

template <int MODE>
__host__ __device__ constexpr uint32_t desc_wave_lds() {
  return desc_ring_tiles<MODE>() * 64u * row_of<MODE>() + kDescRing * kDescLds + 3u * kGatherLds;
}

// A hashed tile waiting for its gather.
struct DescTile {
  uint32_t fast;   // packet on the fast path (valid, 16-B aligned, >= 48 B, IHL 5)
  uint32_t bin;    // u8 LUT: the entry (LDS lookup)
  uint32_t iplo;   // chain: low byte of the source address (tbl_long index)
  uint32_t r0, r1, r2;  // records: the swapped MAC words
};


// LUTM: kLdsU8Tail (u8 LUT staged in LDS) or kGlobalU16 (u16 LUT gathered from L2).
// MODE: 0 = read only (always with CHAIN), 1 = in place (whole owned windows), 2 = 12-B records.
template <int LUTM, bool F4, bool HIST, int MODE, bool CHAIN>
__global__ __launch_bounds__(kStreamNT, 1) void classify_stream_desc_kernel(ClassifyArgs a) {
  constexpr uint32_t kRow = row_of<MODE>(), kTileLds = 64u * kRow;
  constexpr uint32_t kLut = LUTM == kLdsU8Tail ? kLutLds : 0u;
  constexpr uint32_t kPR = desc_ring_tiles<MODE>();
  constexpr bool kG = (CHAIN || LUTM == kGlobalU16) ;  // one 2-B gather per packet
  // store instructions per tile (a lower bound: the compiler may not split them further)
  constexpr uint32_t kS = 1u + (CHAIN ? 1u : 0u) + (MODE == 1 ? 4u : 0u) + (MODE == 2 ? 1u : 0u);
  extern __shared__ __align__(16) uint8_t smem[];  // stream_desc_lds() (after the kernel) sizes this carve-up
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t nbins = a.nb + 1;
  uint8_t* lut = smem;
  uint8_t* wbase = smem + kLut + wave * desc_wave_lds<MODE>();
  uint8_t* ring = wbase;
  uint8_t* dring = wbase + kPR * kTileLds;
  uint8_t* gbuf = dring + kDescRing * kDescLds;
  uint8_t* tlbuf = gbuf + 2u * kGatherLds;  // chain: tbl_long entries of the tile being finished
  const uint32_t hstride = (nbins + 3) & ~3u;
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + kLut + kStreamW * desc_wave_lds<MODE>());
  const uint32_t ring_lds = __builtin_amdgcn_readfirstlane(lds_addr(ring));
  const uint32_t dring_lds = __builtin_amdgcn_readfirstlane(lds_addr(dring));
  const uint32_t gbuf_lds = __builtin_amdgcn_readfirstlane(lds_addr(gbuf));
  const uint32_t tl_lds = __builtin_amdgcn_readfirstlane(lds_addr(tlbuf));
  const uint32_t lut_lds = __builtin_amdgcn_readfirstlane(lds_addr(lut));
  const uint32_t n_tiles = (a.n_pkts + 63u) >> 6;
  const uint32_t n_units = (n_tiles + kStreamW - 1) / kStreamW;
  const uint32_t G = gridDim.x, b = blockIdx.x;
  const uint32_t nt = b < n_units ? (n_units - b + G - 1) / G : 0u;
  auto tile_of = [&](uint32_t k) { return (b + k * G) * kStreamW + wave; };
  auto doff = [&](uint32_t k) {
    return reinterpret_cast<const uint32_t*>(dring + (k % kDescRing) * kDescLds);
  };
  auto dlen = [&](uint32_t k) {
    return reinterpret_cast<const uint32_t*>(dring + (k % kDescRing) * kDescLds + 256u);
  };
  uint8_t* sink = a.sink + lane * 16u;
  uint32_t seq = 0;  // VM operations this wave issued (counted ones)
  auto wait_seq = [&](uint32_t after) { wait_vm_n(seq - after); };
  // descriptors of step k: lane i fetches off/len of packet tile_of(k)*64 + i (clamped)
  auto issue_desc = [&](uint32_t k) {
    const uint32_t p = min(tile_of(k) * 64u + lane, a.n_pkts - 1u);
    const uint32_t d = dring_lds + (k % kDescRing) * kDescLds;
    glds4(a.off + p, d);
    glds2(a.len + p, d + 256u);
    seq += 2;
    return seq;
  };
  // packet windows of step k from its landed descriptors; a window off the 16-B grid is fetched
  // from the batch base (its lane takes the byte-wise path)
  auto issue_pk = [&](uint32_t k) {
    constexpr uint32_t kCh = kRow / 16u;
    const uint32_t* o = doff(k);
    const uint32_t buf = ring_lds + (k % kPR) * kTileLds;
    const uint32_t tb = tile_of(k) * 64u;
    if (kCh == 4u || lane < 16u * kCh) {
      const uint32_t pk = lane / kCh, ch = lane - pk * kCh;
      uint32_t off[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) off[j] = o[j * 16u + pk];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t q = j * 16u + pk;
        const uint8_t* src = (tb + q < a.n_pkts && (off[j] & 15u) == 0) ? a.pkts + off[j] + ch * 16u : a.pkts;
        glds16_tile<MODE != 2>(src, buf + j * (16u * kRow));
      }
    }
    seq += 4;
    return seq;
  };
  // hash step k's packets (landed) and issue their gather; returns the count after the gather
  auto hash = [&](uint32_t k, DescTile& st) {
    const uint32_t p = tile_of(k) * 64u + lane;
    const uint8_t* x = ring + (k % kPR) * kTileLds + lane * kRow;
    const uint4 c0 = *reinterpret_cast<const uint4*>(x);
    const uint4 c1 = *reinterpret_cast<const uint4*>(x + 16);
    const uint2 c2 = *reinterpret_cast<const uint2*>(x + 32);
    const uint32_t off = doff(k)[lane], len = dlen(k)[lane] & 0xffffu;
    const bool fast = p < a.n_pkts && (off & 15u) == 0 && len >= 48u && ((c0.w >> 16) & 0xfu) == 5u;
    st.fast = fast;
    // frame bytes: src 26..29, dst 30..33, ports 34..37, proto 23
    const uint32_t src = (c1.z >> 16) | (c1.w << 16);
    const uint32_t dst = (c1.w >> 16) | (c2.x << 16);
    const uint32_t ports = (c2.x >> 16) | (c2.y << 16);
    uint32_t lo, hi;
    fnv_flow(lo, hi, src, dst, ports, c1.y >> 24);
    const uint32_t idx = F4 ? mod_f4(lo, hi) : mod_barrett(lo, hi, a.m, a.mu);
    if constexpr (LUTM == kLdsU8Tail) st.bin = (idx >> 16) ? a.lut_tail : lut[idx & 0xffffu];
    if constexpr (MODE == 2) {
      st.r0 = (c0.y >> 16) | (c0.z << 16);
      st.r1 = (c0.z >> 16) | (c0.x << 16);
      st.r2 = (c0.x >> 16) | (c0.y << 16);
    }
    const uint32_t g = gbuf_lds + (k & 1u) * kGatherLds;
    if constexpr (CHAIN) {
      const uint32_t ip = __builtin_bswap32(src);
      st.iplo = ip & 0xffu;
      if (kG) glds2(a.tbl24 + (fast ? (ip >> 8) : 0u), g);
    } else if constexpr (LUTM == kGlobalU16 && kG) {
      glds2(static_cast<const uint16_t*>(a.lut) + (fast ? idx : 0u), g);
    }
    if constexpr (kG) ++seq;
    return seq;
  };

  if constexpr (kLut) {
    const uint32_t pieces = a.lut_lds_bytes >> 10;
    for (uint32_t q = wave; q < pieces; q += kStreamW)
      glds16(static_cast<const uint8_t*>(a.lut) + q * 1024u + lane * 16u, lut_lds + q * 1024u);
  }
  if constexpr (HIST)
    for (uint32_t i = tid; i < 2 * hstride; i += kStreamNT) hist[i] = 0;
  // prologue: D(0..2) landed, P(0..2) and D(3) in flight
  uint32_t sP1 = 0, sP2 = 0, sP3 = 0, sD3 = 0, sD4 = 0, sG0 = 0, sG1 = 0, sP0 = 0;
  if (nt > 0) {
    for (uint32_t j = 0; j < 3 && j < nt; ++j) issue_desc(j);
    wait_vm<0>();  // the LUT pieces too
    sP0 = issue_pk(0);
    if (nt > 1) sP1 = issue_pk(1);
    if (nt > 2) sP2 = issue_pk(2);
    if (nt > 3) sD3 = issue_desc(3);
  }
  lds_sync();  // LUT and zeroed histograms visible to every wave
  DescTile cur{}, nxt{};
  if (nt > 0) {
    wait_seq(sP0);
    sG0 = hash(0, cur);
  }
  for (uint32_t k = 0; k < nt; ++k) {
    const uint32_t tb = tile_of(k) * 64u;
    const uint32_t p = tb + lane;
    const bool valid = p < a.n_pkts;
    // tile k's gather (issued one iteration ago)
    uint32_t gv = 0;
    if constexpr (kG) {
      wait_seq(sG0);
      gv = reinterpret_cast<const uint32_t*>(gbuf + (k & 1u) * kGatherLds)[lane] & 0xffffu;
    }
    uint32_t bin = LUTM == kLdsU8Tail ? cur.bin : gv;
    uint32_t gate = kSentinel;
    // chain: routes longer than /24 need a second, dependent gather (tbl_long); issued here, before
    // the next tile's work, and waited for after it, so it does not drain the prefetches
    bool lng = false, any_lng = false;
    uint32_t sTL = 0;
    if constexpr (CHAIN) {
      gate = gv;
      lng = cur.fast && (gv & 0x8000u);
      any_lng = kG && __builtin_amdgcn_ballot_w64(lng) != 0;
      if (any_lng) {
        glds2(a.tbl_long + (lng ? ((gv & 0x7fffu) << 8) + cur.iplo : 0u), tl_lds);
        sTL = ++seq;
      }
    }
    if (k + 1 < nt) {
      wait_seq(sP1);
      sG1 = hash(k + 1, nxt);
    }
    if (k + 3 < nt) {
      wait_seq(sD3);
      sP3 = issue_pk(k + 3);
    }
    if constexpr (CHAIN) {
      if (any_lng) {
        wait_seq(sTL);
        const uint32_t t = reinterpret_cast<const uint32_t*>(tlbuf)[lane] & 0xffffu;
        if (lng) gate = t;
      }
    }
    if constexpr (MODE == 1) {
      // whole owned windows back from LDS: lane (quad, part) stores chunk `part` of packet
      // 16j + quad, chunk 0 with the MACs swapped; lanes of other packets store to the sink
      const uint8_t* tile = ring + (k % kPR) * kTileLds;
      const uint32_t part = lane & 3u, quad = lane >> 2;
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t q = j * 16u + quad;
        uint4 v = *reinterpret_cast<const uint4*>(tile + q * kRow + part * 16u);
        const uint32_t qo = doff(k)[q], ql = dlen(k)[q] & 0xffffu;
        const uint32_t w3 =
            static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(v.w), 0x00, 0xf, 0xf, false));
        const bool qfast = tb + q < a.n_pkts && (qo & 15u) == 0 && ql >= 48u && ((w3 >> 16) & 0xfu) == 5u;
        if (part == 0u)
          v = make_uint4((v.y >> 16) | (v.z << 16), (v.z >> 16) | (v.x << 16), (v.x >> 16) | (v.y << 16), v.w);
        stg16_nt(qfast ? a.pkts + qo + part * 16u : sink, v);
      }
    } else if constexpr (MODE == 2) {
      uint32_t* mo = reinterpret_cast<uint32_t*>(cur.fast ? a.mac_out + static_cast<size_t>(p) * 12u : sink);
      mo[0] = cur.r0;
      mo[1] = cur.r1;
      mo[2] = cur.r2;
    }
    if (valid && !cur.fast) {
      // byte-wise loads: their waits stay inside this branch
      bin = classify_slow<LUTM, F4, CHAIN>(a, lut, a.pkts + doff(k)[lane], dlen(k)[lane] & 0xffffu, p, gate);
      asm volatile("" : "+v"(bin), "+v"(gate)::"memory");
    }
    if constexpr (CHAIN) {
      if (cur.fast && gate >= a.lpm_groups) bin = a.nb;  // test/lpm would panic: never reaches maglev
      *(valid ? a.gate + p : reinterpret_cast<uint16_t*>(sink)) = static_cast<uint16_t>(gate);
    }
    *(valid ? a.backend + p : reinterpret_cast<uint16_t*>(sink)) = static_cast<uint16_t>(bin == a.nb ? kSentinel : bin);
    seq += kS;
    if constexpr (HIST) {
      if (valid) atomicAdd(&hist[(k & 1u) * hstride + bin], 1u);
      lds_sync();
      if (wave == k % kStreamW) {
        uint32_t* h = hist + (k & 1u) * hstride;
        stream_flush<HIST>(a, h, nbins, ((b + k * G) * kStreamW * 64u) / a.part_pkts, lane);
      }
    }
    if (k + 4 < nt) sD4 = issue_desc(k + 4);  // into tile k's descriptor slot, now free
    cur = nxt;
    sP1 = sP2;
    sP2 = sP3;
    sD3 = sD4;
    sG0 = sG1;
  }
}

}  // namespace

// classify_stream_desc_kernel's dynamic LDS as it is carved up at its top: the LUT (u8 only), per wave
// desc_wave_lds (tile ring, descriptor slots, gather words), then two block histograms.
size_t stream_desc_lds(uint32_t nb, int mode, bool wide_lut) {
  const size_t hwords = 2 * (((nb + 1) + 3) & ~3u);
  const size_t wave = mode == 1 ? desc_wave_lds<1>() : (mode == 2 ? desc_wave_lds<2>() : desc_wave_lds<0>());
  return (wide_lut ? 0u : kLutLds) + static_cast<size_t>(kStreamW) * wave + hwords * 4u;
}

namespace {

template <bool F4, bool HIST, int GB>
int launch_stream_mode(const ClassifyArgs& a, const StreamBatches& sb, const LagGroup& lg, int mode, int grid,
                       size_t lds, hipStream_t s) {
  auto fn = mode == 1 ? classify_stream_kernel<F4, HIST, 1, GB>
                      : (mode == 2 ? classify_stream_kernel<F4, HIST, 2, GB> : classify_stream_kernel<F4, HIST, 0, GB>);
  static bool attr_set[2][2][3] = {};
  if (int rc = raise_lds_limit("streaming classify: LDS attribute: %s", fn, 160 * 1024, &attr_set[F4][HIST][mode])) return rc;
  return launch_checked("streaming classify launch: %s", fn, dim3(grid), dim3(kStreamNT), lds, s, a, sb, lg);
}

template <int LUTM, bool F4, bool HIST, int MODE, bool CHAIN>
int launch_desc_v(const ClassifyArgs& a, int grid, size_t lds, hipStream_t s) {
  auto fn = classify_stream_desc_kernel<LUTM, F4, HIST, MODE, CHAIN>;
  static bool attr_set = false;
  if (int rc = raise_lds_limit("streaming classify (descriptors): LDS attribute: %s", fn, 160 * 1024, &attr_set)) return rc;
  return launch_checked("streaming classify (descriptors) launch: %s", fn, dim3(grid), dim3(kStreamNT), lds, s, a);
}

template <int LUTM, bool F4, bool HIST>
int launch_desc_mode(const ClassifyArgs& a, int mode, int grid, size_t lds, hipStream_t s) {
  if (a.tbl24) {
    if constexpr (LUTM == kLdsU8Tail) return launch_desc_v<LUTM, F4, HIST, 0, true>(a, grid, lds, s);
    return set_error(NBG_EINVAL, "streaming classify (descriptors): chain needs the u8 LUT");
  }
  if (mode == 2) return launch_desc_v<LUTM, F4, HIST, 2, false>(a, grid, lds, s);
  if (mode == 1) {
    if constexpr (LUTM == kGlobalU16) return launch_desc_v<LUTM, F4, HIST, 1, false>(a, grid, lds, s);
    return set_error(NBG_EINVAL, "streaming classify (descriptors): in place needs the u16 LUT");
  }
  return launch_desc_v<LUTM, F4, HIST, 0, false>(a, grid, lds, s);
}

template <int LUTM>
int launch_desc_lut(const ClassifyArgs& a, int mode, int grid, size_t lds, hipStream_t s) {
  const bool hist = a.part_hist != nullptr;
  if (a.m == 65537u)
    return hist ? launch_desc_mode<LUTM, true, true>(a, mode, grid, lds, s)
                : launch_desc_mode<LUTM, true, false>(a, mode, grid, lds, s);
  return hist ? launch_desc_mode<LUTM, false, true>(a, mode, grid, lds, s)
              : launch_desc_mode<LUTM, false, false>(a, mode, grid, lds, s);
}

}  // namespace

int launch_classify_stream_desc(const ClassifyArgs& a, bool wide_lut, int mode, int grid, void* stream) {
  const size_t lds = stream_desc_lds(a.nb, mode, wide_lut);
  if (lds > 160u * 1024u) return set_error(NBG_EINVAL, "streaming classify (descriptors): %zu B of LDS", lds);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return wide_lut ? launch_desc_lut<kGlobalU16>(a, mode, grid, lds, s) : launch_desc_lut<kLdsU8Tail>(a, mode, grid, lds, s);
}

int launch_classify_stream_multi(const ClassifyArgs& a, const StreamBatches& sb, int mode, int grid, void* stream) {
  const bool hist = a.part_hist != nullptr;
  const size_t lds = stream_lds(a.nb, mode, false);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LagGroup none{};
  if (a.m == 65537u)
    return hist ? launch_stream_mode<true, true, 0>(a, sb, none, mode, grid, lds, s)
                : launch_stream_mode<true, false, 0>(a, sb, none, mode, grid, lds, s);
  return hist ? launch_stream_mode<false, true, 0>(a, sb, none, mode, grid, lds, s)
              : launch_stream_mode<false, false, 0>(a, sb, none, mode, grid, lds, s);
}

// a's one batch as a StreamBatches
static StreamBatches one_batch(const ClassifyArgs& a) {
  StreamBatches sb{};
  sb.pkts[0] = a.pkts;
  sb.backend[0] = a.backend;
  sb.mac_out[0] = a.mac_out;
  sb.part_hist[0] = a.part_hist;
  sb.n_pkts[0] = a.n_pkts;
  sb.unit_base[0] = 0;
  sb.unit_base[1] = (((a.n_pkts + 63u) >> 6) + kStreamW - 1) / kStreamW;
  sb.n = 1;
  return sb;
}

int launch_classify_stream_lag(const ClassifyArgs& a, const LagGroup& lg, int mode, int grid, void* stream) {
  const uint32_t nbins = a.nb + 1;
  if (!a.part_hist || nbins > 512 || lg.n_parts > static_cast<uint32_t>(grid))
    return set_error(NBG_EINVAL, "streaming classify (lagged group): %u bins, %u partitions on %d blocks", nbins,
                     lg.n_parts, grid);
  const StreamBatches sb = one_batch(a);
  const size_t lds = stream_lds(a.nb, mode, true);
  if (lds > 160u * 1024u) return set_error(NBG_EINVAL, "streaming classify (lagged group): %zu B of LDS", lds);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool b7 = nbins <= 128;
  if (a.m == 65537u)
    return b7 ? launch_stream_mode<true, true, 7>(a, sb, lg, mode, grid, lds, s)
              : launch_stream_mode<true, true, 9>(a, sb, lg, mode, grid, lds, s);
  return b7 ? launch_stream_mode<false, true, 7>(a, sb, lg, mode, grid, lds, s)
            : launch_stream_mode<false, true, 9>(a, sb, lg, mode, grid, lds, s);
}

int launch_classify_ring(const ClassifyArgs& a, const RingArgs& r, int mode, int grid, void* stream) {
  const bool f4 = a.m == 65537u;
  auto fn = mode == 1 ? (f4 ? classify_ring_kernel<true, 1> : classify_ring_kernel<false, 1>)
                      : (f4 ? classify_ring_kernel<true, 0> : classify_ring_kernel<false, 0>);
  if (int rc = raise_lds_limit("ring classify: LDS attribute: %s", fn, 160 * 1024)) return rc;  // every launch
  return launch_checked("ring classify launch: %s", fn, dim3(grid), dim3(kRingNT), ring_lds(mode),
                        static_cast<hipStream_t>(stream), a, r);
}

int launch_ring_gate(const uint32_t* dcomp, const uint32_t* dexit, uint32_t target, uint32_t grid, void* stream) {
  return launch_checked("ring gate launch: %s", ring_gate_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                        dcomp, dexit, target, grid);
}

int launch_classify_stream(const ClassifyArgs& a, int mode, int grid, void* stream) {
  return launch_classify_stream_multi(a, one_batch(a), mode, grid, stream);
}

}  // namespace nbg

// Diagnostics (not in include/nbgpu.h; tests only): `blocks` one-wave workgroups that each hold
// `lds_bytes` of a CU's LDS for `us` microseconds (100 MHz wall clock; every wave exits by time) —
// other work occupying CUs when a persistent ring starts (tests/test_gpu_ring.py).
namespace nbg {
__global__ __launch_bounds__(64) void hold_cus_kernel(uint64_t ticks, uint32_t* sink) {
  extern __shared__ uint32_t held[];
  const uint64_t t0 = wall_clock64();
  held[threadIdx.x] = threadIdx.x;
  while (static_cast<uint64_t>(wall_clock64()) - t0 < ticks) __builtin_amdgcn_s_sleep(16);
  if (held[threadIdx.x] == 0xdeadbeefu) sink[0] = 1u;
}
}  // namespace nbg

extern "C" int nbg_debug_hold_cus(uint32_t blocks, uint32_t lds_bytes, uint32_t us, void* stream) {
  if (blocks == 0 || blocks > 4096 || lds_bytes < 256 || lds_bytes > 160u * 1024u || us > 10000000u) return NBG_EINVAL;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(nbg::hold_cus_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    return NBG_EIO;
  hipLaunchKernelGGL(nbg::hold_cus_kernel, dim3(blocks), dim3(64), lds_bytes, static_cast<hipStream_t>(stream),
                     static_cast<uint64_t>(us) * 100u, static_cast<uint32_t*>(nullptr));
  return hipGetLastError() == hipSuccess ? NBG_OK : NBG_EIO;
}
