// The grouping kernels: partition histograms, their scan over partitions, and the stable per-group
// FIFO order (group_by.rs:46-51) for few, many (<= 1024) and very many (<= 32768) bins.
//
// scan_kernel — (many backends only) per backend bin, exclusive scan of the partition
//   histograms over partitions, and the bin totals (64 bins per block, coalesced rows).
// group_kernel — per partition: the per-bin prefix over earlier partitions and the group
//   bases, then per 4096-packet chunk wave ballot multisplit ranks (stable), a local counting
//   sort in LDS, and coalesced stores of perm[] = packet indices grouped by backend.
//
// Integer/byte work only; no MFMA.  HBM-bound.
#include <atomic>
#include <cstdlib>

#include "kernel_common.h"

namespace nbg {

namespace {

// Many backends: the partition histograms come from this kernel instead of the classify kernel
// (whose per-block flush would cost about one global atomic per packet at ~1000 bins).  One
// 512-thread block per partition counts its packets' backends in LDS and stores the whole row.
// Blocks [j * hm.per, j * hm.per + h[j].n_parts) count batch j (a single batch: j = 0).
__global__ __launch_bounds__(kGBlock) void hist_kernel(HistMulti hm) {
  extern __shared__ __align__(16) uint32_t hs[];
  const uint32_t bj = blockIdx.x / hm.per;
  const HistArgs a = hm.h[bj];
  const uint32_t nbins = a.nb + 1, tid = threadIdx.x, c_lin = blockIdx.x - bj * hm.per;
  // the group kernel's XCD-aware partition order: partition c's backends, read here, are read again by
  // the group block of partition c on the same XCD, from its L2
  const uint32_t c = (a.n_parts % 8u == 0u && c_lin < a.n_parts) ? (c_lin % 8u) * (a.n_parts / 8u) + c_lin / 8u : c_lin;
  if (c >= a.n_parts) return;
  const uint32_t pbeg = c * a.part_pkts, pend = min(pbeg + a.part_pkts, a.n_pkts);
  for (uint32_t b = tid; b < nbins; b += kGBlock) hs[b] = 0;
  lds_sync();
  // one chunk per pass, every load unconditional (clamped) and in flight together
  for (uint32_t i0 = pbeg; i0 < pend; i0 += kChunk) {
    uint32_t v[kGRounds];
#pragma unroll
    for (int k = 0; k < kGRounds; ++k) v[k] = ld_u16(a.backend, min(i0 + k * kGBlock + tid, a.n_pkts - 1u) * 2u);
#pragma unroll
    for (int k = 0; k < kGRounds; ++k) {
      // min: the sentinel (0xFFFF) is bin nb; so is any other value > nb, which no classify writes
      // but a ring batch's backend[] can hold after a ring that ended before completing it
      if (i0 + k * kGBlock + tid < pend) atomicAdd(&hs[min(v[k], a.nb)], 1u);
    }
  }
  lds_sync();
  if (a.hist16) {  // half the row bytes the group kernel's direct prefix reads
    const uint32_t hw = (nbins + 1) >> 1;
    uint32_t* row = a.part_hist + static_cast<size_t>(c) * hw;
    for (uint32_t w = tid; w < hw; w += kGBlock) row[w] = hs[2 * w] | (2 * w + 1 < nbins ? hs[2 * w + 1] << 16 : 0u);
    return;
  }
  uint32_t* row = a.part_hist + static_cast<size_t>(c) * nbins;
  for (uint32_t b = tid; b < nbins; b += kGBlock) row[b] = hs[b];
}

// Many backends: exclusive scan of part_hist[.][bin] over partitions, and every bin's total.
// One block per 64 consecutive bins, one lane per bin; wave w scans partitions [32w, 32w + 32)
// in registers (each row segment is one coalesced 256-B load, all 32 in flight), and the waves'
// sums are combined through LDS.
constexpr uint32_t kScanBins = 64, kScanWaves = kMaxParts / 32;
__global__ __launch_bounds__(kScanWaves * 64) void scan_kernel(ScanMulti sm) {
  __shared__ uint32_t s_sum[kScanWaves][kScanBins];
  const ScanArgs a = sm.s[blockIdx.y];  // batch
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t b = blockIdx.x * kScanBins + lane;
  const uint32_t bc = min(b, a.nbins - 1u), q0 = wave * 32u;
  uint32_t v[32];
#pragma unroll
  for (uint32_t k = 0; k < 32; ++k) v[k] = ld_u32(a.part_hist, (min(q0 + k, a.n_parts - 1u) * a.nbins + bc) * 4u);
  uint32_t run = 0;
#pragma unroll
  for (uint32_t k = 0; k < 32; ++k) {
    const uint32_t x = q0 + k < a.n_parts ? v[k] : 0u;
    v[k] = run;  // exclusive within this wave's partitions
    run += x;
  }
  s_sum[wave][lane] = run;
  __syncthreads();
  uint32_t off = 0, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < kScanWaves; ++w) {
    const uint32_t t = s_sum[w][lane];
    off += w < wave ? t : 0u;
    total += t;
  }
  if (b < a.nbins) {
#pragma unroll
    for (uint32_t k = 0; k < 32; ++k)
      if (q0 + k < a.n_parts) a.part_prefix[static_cast<size_t>(q0 + k) * a.nbins + b] = off + v[k];
    if (wave == 0) a.totals[b] = total;
  }
}

// ---- many backends (more than kMaxGroupBins - 1, up to 32767) ------------------------------------
// The multisplit group kernel keeps a counter row per wave and bin in LDS, which does not scale to
// 32768 bins.  Past 1023 backends the per-partition histograms (hist_kernel) and their prefix over
// partitions (scan_kernel) feed two small kernels: bin_base_kernel scans the bin totals into group
// bases (and writes counts), and group_wide_kernel walks each partition in packet order, one wave
// per partition, with one LDS counter per bin: a lane's position is its bin's base + the bin's
// prefix over earlier partitions + the bin's count so far in this partition + its rank among the
// lanes of its 64-packet step with the same bin (a readlane match over the step), so perm keeps the
// per-group FIFO order of group_by.rs:46-51 for any bin count.
__global__ __launch_bounds__(kGBlock) void bin_base_kernel(GroupArgs a) {
  __shared__ uint32_t s_wave[kGBlock / 64];
  const uint32_t nbins = a.nb + 1, tid = threadIdx.x;
  const uint32_t per = (nbins + kGBlock - 1) / kGBlock;  // consecutive bins per thread
  uint32_t s = 0;
  for (uint32_t k = 0; k < per; ++k) {
    const uint32_t b = tid * per + k;
    s += b < nbins ? a.totals[b] : 0u;
  }
  uint32_t all;
  uint32_t base = block_excl_scan_n<kGBlock>(s, s_wave, all);
  for (uint32_t k = 0; k < per; ++k) {
    const uint32_t b = tid * per + k;
    if (b < nbins) {
      const uint32_t t = a.totals[b];
      a.bin_base[b] = base;
      if (a.counts) a.counts[b] = t;
      base += t;
    }
  }
}

__global__ __launch_bounds__(64) void group_wide_kernel(GroupArgs a) {
  extern __shared__ __align__(16) uint32_t cnt[];  // [nbins]: packets of each bin seen so far
  const uint32_t nbins = a.nb + 1, lane = threadIdx.x, c = blockIdx.x;
  for (uint32_t b = lane; b < nbins; b += 64) cnt[b] = 0;
  const uint32_t pbeg = c * a.part_pkts, pend = min(pbeg + a.part_pkts, a.n_pkts);
  const uint32_t* prefix = a.part_prefix + static_cast<size_t>(c) * nbins;
  for (uint32_t i0 = pbeg; i0 < pend; i0 += 64u) {
    const uint32_t i = i0 + lane;
    const bool valid = i < pend;
    const uint32_t raw = ld_u16(a.backend, min(i, a.n_pkts - 1u) * 2u);
    const uint32_t bin = !valid ? 0xffffffffu : (raw == NBG_SENTINEL ? a.nb : raw);
    // rank among earlier lanes of this step with the same bin, and the bin's lanes in the step
    uint32_t rank, count;
    wave_match_rank<15>(valid ? bin : 0u, valid, lane, rank, count);
    // every lane reads its bin's count before any lane of the step writes one (one wave: its LDS
    // operations execute in issue order; the wave barriers keep the compiler from moving them)
    const uint32_t slot = valid ? bin : 0u;
    const uint32_t before = cnt[slot];
    __builtin_amdgcn_wave_barrier();
    if (valid && a.perm) a.perm[a.bin_base[bin] + prefix[bin] + before + rank] = i;
    if (valid) cnt[bin] = before + count;  // every lane of a bin stores the same new count
    __builtin_amdgcn_wave_barrier();
  }
}

// One 512-thread block per partition (part_pkts packets, processed in 4096-packet chunks): the
// stable per-group FIFO order of group_by.rs:46-51.  Wave w owns rounds [8w, 8w + 8) of 64 packets of
// every chunk (packet = chunk base + 512 w + 64 r + lane).
//   Entry: every global load of the block is issued at once: the first chunk's backends, then the
//     prologue's (kScanDirect: this partition's share of the L2-resident partition rows; kScanKernel:
//     scan_kernel's prefix row and the bin totals).  The first chunk is ranked while the prologue's
//     loads are in flight (a wave ballot multisplit per 64-packet round, one ballot per bin bit; the
//     wave's 16-bit LDS counter row carries its earlier rounds).
//   Then four barrier-separated phases per chunk: (1) the prologue's sums and the first half of the
//     chunk's bin-major exclusive scan over the (bin, wave) counters; (2) the group bases (exclusive
//     scan of the totals over bins) and the scan's write-back; (3) per bin, the perm position of the
//     chunk's first packet of the bin, and the local counting sort into LDS; (4) coalesced perm
//     stores (consecutive sorted slots of one bin are consecutive perm entries).
// The round-4 form ranked only after the prologue and took 8 barriers per chunk; its phase timeline
// (tools/gprobe.py, profiles/r05_gprobe_v1.txt) had the row prologue (1.84 us) and the ranks (1.55 us,
// VALU-bound) one after the other on each block's critical path.  The ranks take 4 VALU operations per
// bin bit (mismatch_all), the backends and the rows are raw buffer loads (no clamps, one 32-bit offset
// per lane): 11,324 instead of 14,954 cycles per C2 block (profiles/r05_gprobe_final.txt).  Up to 128
// bins a lane's peers come from a per-wave LDS table of lane masks instead (one OR, one read, one clear
// per round; 1,069 instead of 1,565 VALU instructions in the kernel): 11,026 cycles
// (profiles/r05_gprobe_peer.txt), the ranks now wait on the backends' HBM latency.
// 4 waves per SIMD (two resident blocks per CU, <= 128 VGPRs).
constexpr int kGroupWaves = 4;
// BITS: bin bits the multisplit compares (7 for up to 128 bins, else 10); unused high bits are 0
template <int SCAN, int BITS>
// Blocks [j * gm.per, j * gm.per + g[j].n_parts) group batch j (a single batch: j = 0, c = blockIdx.x).
__global__ __launch_bounds__(kGBlock, kGroupWaves) void group_kernel(GroupMulti gm) {
  extern __shared__ __align__(16) uint32_t gs[];  // group_lds() (after the kernel) sizes this carve-up
  __shared__ uint32_t s_wave[2][kGBlock / 64];
  constexpr uint32_t kW = kGBlock / 64;  // waves
  constexpr uint32_t kMaxBins = 1u << BITS;
  const uint32_t bj = blockIdx.x / gm.per;
  const GroupArgs a = gm.g[bj];
  const uint32_t nbins = a.nb + 1;
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  // partition of batch bj, XCD-aware: the dispatcher deals blocks round-robin over the 8 XCDs, and
  // neighbouring partitions write adjacent pieces of every bin's perm run (~4 packets per bin and chunk
  // at 1001 bins), so XCD x takes partitions [x n / 8, (x + 1) n / 8) and the pieces of one line meet
  // in one L2: C3 hist + scan + group 20.5 -> 19.5 us, 8 per launch 6.8 -> 6.2 us per batch, C2 9.3 ->
  // 9.1 us (profiles/r05_group_xcd_ab.txt)
  const uint32_t c_lin = blockIdx.x - bj * gm.per;
  const uint32_t c = (a.n_parts % 8u == 0u && c_lin < a.n_parts) ? (c_lin % 8u) * (a.n_parts / 8u) + c_lin / 8u : c_lin;
  // The next call accumulates into the other histogram buffer: every block of the grid zeroes a
  // slice of it, last, after its perm stores.  Stores issued earlier would sit in vmcnt, and the
  // first wait for a backend load would also wait for them (the counter retires in issue order).
  auto zero_next = [&] {
    for (uint32_t i = blockIdx.x * kGBlock + tid; i < a.next_words; i += gridDim.x * kGBlock) a.part_hist_next[i] = 0;
  };
  if (c >= a.n_parts) {  // a smaller batch of a multi-batch launch
    zero_next();
    return;
  }
  const uint32_t nbp = (nbins + 3) & ~3u;
  uint32_t* base = gs;                 // [nbins] next perm position of this partition, per bin
  uint32_t* tot = base + nbp;          // [nbins] bin totals (prologue), then the chunk's perm bases
  // 16-bit per-wave counters (a wave counts <= 512 packets of a chunk; chunk slots < kChunk) and one
  // word per sorted slot (bin << 12 | packet within the chunk): 40 KB of LDS at 1001 bins
  static_assert(kChunk <= 4096 && kChunk == kGBlock * kGRounds, "sorted slots hold a 12-bit packet index");
  const uint32_t cst = (nbins + 8) & ~7u;  // cnt row stride: a scratch slot for lanes past the end; 16-B rows
  uint16_t* cnt = reinterpret_cast<uint16_t*>(tot + nbp);  // [kW][cst]
  uint32_t* sslot = reinterpret_cast<uint32_t*>(cnt + kW * cst);  // [kChunk]
  uint16_t* mycnt = cnt + wave * cst;
  // <= 128 bins: the lanes that share a lane's bin come from a per-wave table of 64-bit lane masks
  // [kW][nbins + 1] (slot nbins: lanes past the end), else from the ballot multisplit
  constexpr bool kPeer = BITS <= 7;
  unsigned long long* peer = reinterpret_cast<unsigned long long*>(sslot + kChunk) + wave * (nbins + 1);
  const bool perm = a.perm != nullptr;

  // ---- entry: the first chunk's backends, then the prologue's loads, all in flight together
  const uint32_t pbeg = c * a.part_pkts;
  const uint32_t pend = min(pbeg + a.part_pkts, a.n_pkts);
  const __amdgpu_buffer_rsrc_t rbe = raw_rsrc(a.backend, a.n_pkts * 2u);  // packets past the batch read 0
  uint32_t pre_bin[kGRounds];
  {
    const uint32_t wb = pbeg + wave * (64u * kGRounds);
#pragma unroll
    for (int r = 0; r < kGRounds; ++r) pre_bin[r] = __builtin_amdgcn_raw_buffer_load_b16(rbe, (wb + r * 64u + lane) * 2u, 0, 0);
  }
  // the scheduler keeps the backend loads ahead of the prologue's (vmcnt retires in issue order: the
  // ranks then wait for the backends only)
  __builtin_amdgcn_sched_barrier(0);
  // kScanDirect: thread (w, j) = (tid % hw, tid / hw) sums rows j, j + L, ... of row word w (L threads
  // per word; consecutive threads read consecutive words of one row); the first kU of its rows are
  // loaded here.  kScanKernel: this thread's consecutive bins of the prefix row and the totals.
  constexpr uint32_t kU = 18;  // 65 backends, 16-bit rows: 33 words, L = 15, 18 rows per thread
  constexpr uint32_t kCb = kMaxBins > kGBlock ? kMaxBins / kGBlock : 1u;  // consecutive bins per thread
  const uint32_t hw = a.hist16 ? (nbins + 1) >> 1 : nbins;  // row words
  const uint32_t L = hw >= kGBlock ? 1u : kGBlock / hw;
  const uint32_t rw0 = tid % hw, rj0 = tid / hw;  // this thread's first (word, row) pair
  uint32_t h[kU];
  uint32_t pk[kCb], tk[kCb];
  if constexpr (SCAN == kScanDirect) {
    // every thread loads its first (word, row) pair's first kU rows (a thread past hw * L ignores
    // them): a load inside a branch makes the compiler wait for all of them at the join, before the
    // ranks
    const __amdgpu_buffer_rsrc_t rrows = raw_rsrc(a.part_hist, a.n_parts * hw * 4u);  // rows past the last read 0
#pragma unroll
    for (uint32_t k = 0; k < kU; ++k) h[k] = __builtin_amdgcn_raw_buffer_load_b32(rrows, ((rj0 + k * L) * hw + rw0) * 4u, 0, 0);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kCb; ++k) {
      const uint32_t b = min(tid * kCb + k, nbins - 1u);
      pk[k] = ld_u32(a.part_prefix, (c * nbins + b) * 4u);
      tk[k] = ld_u32(a.totals, b * 4u);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  for (uint32_t b = tid; b < nbp; b += kGBlock) {
    base[b] = 0;
    tot[b] = 0;
  }
  // each wave clears its own peer table (its LDS operations execute in order: no barrier)
  if constexpr (kPeer)
    for (uint32_t b = lane; b <= nbins; b += 64) peer[b] = 0;

  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const uint32_t lt_lo = static_cast<uint32_t>(lt), lt_hi = static_cast<uint32_t>(lt >> 32);
  uint32_t br[kGRounds];  // rank << 16 | bin (bins < kMaxGroupBins, ranks < kChunk), or ~0 past the end
  // one chunk's ranks (its backends in pre_bin); afterwards the next chunk's backends are loaded
  auto rank_chunk = [&](uint32_t cbase) {
    // each wave zeroes its own counter row: every reader of the previous chunk's counters has passed
    // a barrier since, and one wave's LDS operations execute in order
#pragma unroll
    for (uint32_t k = 0; k < (kMaxBins + 8 + 511) / 512; ++k)
      if ((lane + k * 64) * 8 < cst) reinterpret_cast<uint4*>(mycnt)[lane + k * 64] = make_uint4(0, 0, 0, 0);
    const uint32_t wbase = cbase + wave * (64u * kGRounds);
#pragma unroll
    for (int r = 0; r < kGRounds; ++r) {
      const uint32_t i = wbase + r * 64u + lane;
      const bool valid = i < pend;
      const uint32_t bin = min(pre_bin[r], a.nb);  // the sentinel (and any value > nb, as in hist_kernel)
      const uint32_t slot = valid ? bin : nbins;   // lanes past the end use the scratch slot
      uint32_t elo, ehi;                           // the lanes with my bin (and my validity)
      if constexpr (kPeer) {
        // every lane ORs its bit into its slot's mask, reads the mask back and clears it: three LDS
        // instructions of one wave, executed in order (the compiler barriers keep them in order)
        unsigned long long* pw = peer + slot;
        __hip_atomic_fetch_or(pw, 1ull << lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __asm__ volatile("" ::: "memory");
        const unsigned long long pm = *pw;
        __asm__ volatile("" ::: "memory");
        *pw = 0;
        elo = static_cast<uint32_t>(pm);
        ehi = static_cast<uint32_t>(pm >> 32);
      } else {
        // accumulate, per bin bit, the lanes whose ballot bit differs from mine; the rest match
        const uint32_t mv = valid ? ~0u : 0u;
        const unsigned long long bv = __builtin_amdgcn_ballot_w64(valid);
        uint32_t mlo = static_cast<uint32_t>(bv) ^ mv, mhi = static_cast<uint32_t>(bv >> 32) ^ mv;
        mismatch_all<BITS>(bin, mlo, mhi);
        elo = ~mlo;
        ehi = ~mhi;
      }
      // every lane of a bin stores the same new count (no branch)
      const uint32_t prior = mycnt[slot];
      mycnt[slot] = static_cast<uint16_t>(prior + __popc(elo) + __popc(ehi));
      const uint32_t rank = prior + __popc(elo & lt_lo) + __popc(ehi & lt_hi);
      br[r] = valid ? (rank << 16) | bin : 0xffffffffu;
    }
    // the next chunk's backends (partitions of more than one chunk): loaded now, behind this
    // chunk's scans and stores
    if (cbase + kChunk < pend) {
#pragma unroll
      for (int r = 0; r < kGRounds; ++r)
        pre_bin[r] = __builtin_amdgcn_raw_buffer_load_b16(rbe, (wbase + kChunk + r * 64u + lane) * 2u, 0, 0);
    }
  };
  if (perm) rank_chunk(pbeg);

  // bin-major exclusive scan over the chunk's (bin, wave) counters: the chunk-local slot where wave
  // w's packets of bin b start (each thread owns kPer consecutive elements: whole bins' wave counters
  // when kPer >= kW); first half: the wave-level scan
  constexpr uint32_t kPer = (kMaxBins * kW + kGBlock - 1) / kGBlock;
  const uint32_t ne = nbins * kW;
  uint32_t ev[kPer], esum = 0, ex = 0;
  // kPer == 2 * kW (10 bits): a thread's elements are bins 2t and 2t + 1 of every wave's row, one
  // 32-bit LDS word per wave (the rows are 16-B aligned, cst even)
  constexpr bool kPair = kPer == 2 * kW;
  auto chunk_scan_begin = [&] {
    esum = 0;
    if constexpr (kPair) {
#pragma unroll
      for (uint32_t w = 0; w < kW; ++w) {
        const uint32_t v = 2 * tid < nbins ? reinterpret_cast<const uint32_t*>(cnt + w * cst)[tid] : 0u;
        ev[w] = v & 0xffffu;
        ev[kW + w] = 2 * tid + 1 < nbins ? v >> 16 : 0u;
      }
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) esum += ev[k];
      ex = wave_incl_scan(esum);
      if (lane == 63u) s_wave[0][wave] = ex;
      return;
    }
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t e = tid * kPer + k;
      ev[k] = e < ne ? cnt[(e % kW) * cst + e / kW] : 0u;
      esum += ev[k];
    }
    ex = wave_incl_scan(esum);
    if (lane == 63u) s_wave[0][wave] = ex;
  };
  // second half (after a barrier): the wave's offset, the write-back; returns the chunk's packets
  auto chunk_scan_end = [&]() -> uint32_t {
    uint32_t wpre = 0, ctotal = 0;
#pragma unroll
    for (uint32_t w = 0; w < kW; ++w) {
      const uint32_t t = s_wave[0][w];
      wpre += w < wave ? t : 0u;
      ctotal += t;
    }
    uint32_t x = wpre + ex - esum;
    if constexpr (kPair) {
      uint32_t lo[kW];
#pragma unroll
      for (uint32_t w = 0; w < kW; ++w) {  // bin 2t over the waves, then bin 2t + 1
        lo[w] = x;
        x += ev[w];
      }
#pragma unroll
      for (uint32_t w = 0; w < kW; ++w) {
        if (2 * tid < nbins) reinterpret_cast<uint32_t*>(cnt + w * cst)[tid] = lo[w] | (x << 16);
        x += ev[kW + w];
      }
      return ctotal;
    }
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t e = tid * kPer + k;
      if (e < ne) cnt[(e % kW) * cst + e / kW] = static_cast<uint16_t>(x);
      x += ev[k];
    }
    return ctotal;
  };

  lds_sync();  // (B1) base / tot zeroed, every wave's counts of the first chunk in LDS

  // ---- (1) prologue sums, the chunk scan's first half
  uint32_t gs_incl = 0, gs_own = 0;  // kScanKernel: this thread's bins' totals, scanned over the wave
  if constexpr (SCAN == kScanDirect) {
    // (word, row) pair (rw, rj): rows rj, rj + L, ...; the first kU of the first pair's rows are in
    // h[] (static indices only, so that h stays in registers), any further rows are loaded one by one
    // (more than kU rows per thread, or more than kGBlock row words: many bins, rare)
    auto add_row = [&](uint32_t q, uint32_t v, uint32_t (&acc)[4]) {
      const uint32_t lo = q < a.n_parts ? (a.hist16 ? v & 0xffffu : v) : 0u;
      const uint32_t hi = q < a.n_parts && a.hist16 ? v >> 16 : 0u;
      acc[0] += q < c ? lo : 0u;
      acc[1] += q < c ? hi : 0u;
      acc[2] += lo;
      acc[3] += hi;
    };
    auto publish = [&](uint32_t rw, const uint32_t (&acc)[4]) {
      const uint32_t b0 = a.hist16 ? 2 * rw : rw;
      atomicAdd(&base[b0], acc[0]);
      atomicAdd(&tot[b0], acc[2]);
      if (a.hist16 && b0 + 1 < nbins) {
        atomicAdd(&base[b0 + 1], acc[1]);
        atomicAdd(&tot[b0 + 1], acc[3]);
      }
    };
    if (tid < hw * L) {
      uint32_t acc[4] = {0u, 0u, 0u, 0u};
      if (a.hist16 && a.part_pkts * 15u < 65536u) {
        // packed: the two 16-bit bins of a row word are summed by one 32-bit add, at most 15 rows per
        // partial sum (15 partitions' counts of one bin fit 16 bits); rows past the last read 0
        uint32_t pall = 0, ppre = 0;
#pragma unroll
        for (uint32_t k = 0; k < kU; ++k) {
          pall += h[k];
          ppre += rj0 + k * L < c ? h[k] : 0u;
          if (k % 15u == 14u || k == kU - 1u) {
            acc[0] += ppre & 0xffffu;
            acc[1] += ppre >> 16;
            acc[2] += pall & 0xffffu;
            acc[3] += pall >> 16;
            pall = ppre = 0;
          }
        }
      } else {
#pragma unroll
        for (uint32_t k = 0; k < kU; ++k) add_row(rj0 + k * L, h[k], acc);
      }
      for (uint32_t q = rj0 + kU * L; q < a.n_parts; q += L) add_row(q, ld_u32(a.part_hist, (q * hw + rw0) * 4u), acc);
      publish(rw0, acc);
    }
    for (uint32_t t = tid + kGBlock; t < hw * L; t += kGBlock) {
      uint32_t acc[4] = {0u, 0u, 0u, 0u};
      const uint32_t rw = t % hw;
      for (uint32_t q = t / hw; q < a.n_parts; q += L) add_row(q, ld_u32(a.part_hist, (q * hw + rw) * 4u), acc);
      publish(rw, acc);
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kCb; ++k) gs_own += tid * kCb + k < nbins ? tk[k] : 0u;
    gs_incl = wave_incl_scan(gs_own);
    if (lane == 63u) s_wave[1][wave] = gs_incl;
  }
  if (perm) chunk_scan_begin();
  lds_sync();  // (B2)

  // ---- (2) group bases (exclusive scan of the totals over bins), the chunk scan's write-back
  if constexpr (SCAN == kScanDirect && kMaxBins <= 128) {  // one wave, <= 2 bins per lane
    if (wave == 0) {
      uint32_t t2[2], s = 0;
#pragma unroll
      for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t b = lane * 2 + k;
        t2[k] = b < nbins ? tot[b] : 0u;
        s += t2[k];
      }
      uint32_t gb = wave_incl_scan(s) - s;
#pragma unroll
      for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t b = lane * 2 + k;
        if (b < nbins) {
          if (c == 0 && a.counts) a.counts[b] = t2[k];
          base[b] += gb;  // group base + prefix over earlier partitions
        }
        gb += t2[k];
      }
    }
  } else if constexpr (SCAN == kScanDirect) {  // many bins summed here: a block-wide scan of tot[]
    uint32_t tb[kCb], s = 0;
#pragma unroll
    for (uint32_t k = 0; k < kCb; ++k) {
      const uint32_t b = tid * kCb + k;
      tb[k] = b < nbins ? tot[b] : 0u;
      s += tb[k];
    }
    uint32_t all;
    uint32_t gb = block_excl_scan_n<kGBlock>(s, s_wave[1], all);
#pragma unroll
    for (uint32_t k = 0; k < kCb; ++k) {
      const uint32_t b = tid * kCb + k;
      if (b < nbins) {
        if (c == 0 && a.counts) a.counts[b] = tb[k];
        base[b] += gb;
      }
      gb += tb[k];
    }
  } else {  // the wave-level scan of (1) completed across waves
    uint32_t gb = gs_incl - gs_own;
#pragma unroll
    for (uint32_t w = 0; w < kW; ++w) gb += w < wave ? s_wave[1][w] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < kCb; ++k) {
      const uint32_t b = tid * kCb + k;
      if (b < nbins) {
        if (c == 0 && a.counts) a.counts[b] = tk[k];
        base[b] = pk[k] + gb;
      }
      gb += tk[k];
    }
  }
  if (!perm) {
    zero_next();
    return;
  }
  uint32_t ctotal = chunk_scan_end();
  for (uint32_t cbase = pbeg;;) {
    lds_sync();  // (B3)
    // ---- (3) per bin: perm position of chunk slot j of bin b = tot[b] + j; advance past the bin.
    // Local counting sort of the chunk's packets into LDS.
    for (uint32_t b = tid; b < nbins; b += kGBlock) {
      const uint32_t st = cnt[b];                                // wave 0's start = the bin's start
      const uint32_t en = b + 1 < nbins ? cnt[b + 1] : ctotal;
      tot[b] = base[b] - st;
      base[b] += en - st;
    }
    const uint32_t wbase = cbase + wave * (64u * kGRounds);
#pragma unroll
    for (int r = 0; r < kGRounds; ++r) {
      if (br[r] != 0xffffffffu) {
        const uint32_t bin = br[r] & 0xffffu;
        const uint32_t j = mycnt[bin] + (br[r] >> 16);
        sslot[j] = (bin << 12) | (wbase - cbase + r * 64u + lane);
      }
    }
    lds_sync();  // (B4)
    // ---- (4) coalesced output, unrolled: the slot reads, then the dependent base reads, issue back
    // to back (a loop paid two LDS round trips per iteration)
    {
      uint32_t sv[kGRounds], pb[kGRounds];
#pragma unroll
      for (int k = 0; k < kGRounds; ++k) sv[k] = sslot[tid + k * kGBlock];  // < kChunk; slots >= ctotal unused
#pragma unroll
      for (int k = 0; k < kGRounds; ++k) pb[k] = tot[min(sv[k] >> 12, nbins - 1u)];
#pragma unroll
      for (int k = 0; k < kGRounds; ++k) {
        const uint32_t j = tid + k * kGBlock;
        if (j < ctotal) a.perm[pb[k] + j] = cbase + (sv[k] & 0xfffu);
      }
    }
    cbase += kChunk;
    if (cbase >= pend) break;
    // the next chunk (its backends are loaded): ranks, then the scan's two halves
    rank_chunk(cbase);
    lds_sync();
    chunk_scan_begin();
    lds_sync();
    ctotal = chunk_scan_end();
  }
  zero_next();
}

}  // namespace

// The dynamic LDS of group_kernel (above) and group_direct_kernel (below) as each carves it up at its top.
// group_kernel: base[nbp] + tot[nbp] u32, cnt[waves][cst] u16, sslot[kChunk] u32 (40 KB at 1001 bins),
// and <= 128 bins peer[waves][nbins + 1] u64 (22 KB at 66 bins);
// compact (group_direct_kernel): run[2][nbp] + tot[nbp] u32, cnt[waves][cst] u16 (28 KB at 1001 bins)
size_t group_lds(uint32_t nbins, bool compact) {
  const size_t nbp = (nbins + 3) & ~3u, cst = (nbins + 8) & ~7u;
  if (compact) return (nbp * 3 + cst * (kGBlock / 64) / 2) * 4;
  const size_t peer = nbins <= 128 ? (kGBlock / 64) * (nbins + 1) * 8 : 0;
  return (nbp * 2 + kChunk + cst * (kGBlock / 64) / 2) * 4 + peer;
}

namespace {

// group_direct_kernel: the compact form of group_kernel, for many bins beside an in-place
// persistent ring (whose blocks leave ~30 KB of a CU's LDS; group_kernel takes 40 KB at 1001 bins
// and would wait for the ring to end).  Same grid, arguments and outputs.  One 512-thread block per
// partition (part_pkts packets, processed in 4096-packet chunks): the stable per-group FIFO order
// of group_by.rs:46-51.  Wave w owns the contiguous 512-packet segment [512w, 512w + 512) of every
// chunk, 8 rounds of 64 packets.
//   Ranks: per round a ballot multisplit (one ballot per bin bit) gives every lane its rank among
//     the round's lanes of its bin; the wave's LDS counter row (16 bit per bin) carries the counts
//     of its earlier rounds.  The first chunk is ranked while the prologue's loads are in flight.
//   Prologue: this partition's prefix over earlier partitions and the bin totals, summed from the
//     L2-resident partition rows (few bins) or read from scan_kernel's output; group bases (an
//     exclusive scan of the totals over bins) give run[b], the perm position of the partition's
//     first packet of bin b.
//   Per chunk, one pass over the bins turns each bin's 8 wave counts into exclusive prefixes (and
//     advances run[] past the chunk), then every lane stores perm[run[b] + prefix[w][b] + rank] =
//     its packet directly, without the local sort (measured 1-2 us per 1M batch slower than
//     group_kernel's coalesced stores: profiles/r05_group_ab.txt).
// LDS: run[2][nbins] + tot[nbins] u32, cnt[8][nbins] u16: 28 KB at 1001 bins.
template <int SCAN, int BITS>
__global__ __launch_bounds__(kGBlock, kGroupWaves) void group_direct_kernel(GroupMulti gm) {
  extern __shared__ __align__(16) uint32_t gs[];  // group_lds(compact) (before the kernel) sizes this carve-up
  __shared__ uint32_t s_wave[kGBlock / 64];
  constexpr uint32_t kW = kGBlock / 64;  // waves
  static_assert(kChunk == kGBlock * kGRounds && kChunk / kW <= 65535, "16-bit per-wave counters");
  const uint32_t bj = blockIdx.x / gm.per;
  const GroupArgs a = gm.g[bj];
  const uint32_t nbins = a.nb + 1;
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  // partition of batch bj, XCD-aware as in group_kernel (neighbouring partitions on one XCD)
  const uint32_t c_lin = blockIdx.x - bj * gm.per;
  const uint32_t c = (a.n_parts % 8u == 0u && c_lin < a.n_parts) ? (c_lin % 8u) * (a.n_parts / 8u) + c_lin / 8u : c_lin;
  // The next call accumulates into the other histogram buffer: every block of the grid zeroes a
  // slice of it, last, after its perm stores.  Stores issued earlier would sit in vmcnt, and the
  // first wait for a backend load would also wait for them (the counter retires in issue order).
  auto zero_next = [&] {
    for (uint32_t i = blockIdx.x * kGBlock + tid; i < a.next_words; i += gridDim.x * kGBlock) a.part_hist_next[i] = 0;
  };
  if (c >= a.n_parts) {  // a smaller batch of a multi-batch launch
    zero_next();
    return;
  }
  const uint32_t nbp = (nbins + 3) & ~3u;
  const uint32_t cst = (nbins + 8) & ~7u;  // cnt row stride: a scratch slot for lanes past the end; 16-B rows
  uint32_t* run = gs;                      // [2][nbp] by chunk parity
  uint32_t* tot = run + 2 * nbp;           // [nbp] bin totals (prologue)
  uint16_t* cnt = reinterpret_cast<uint16_t*>(tot + nbp);  // [kW][cst]
  uint16_t* mycnt = cnt + wave * cst;
  constexpr uint32_t kMaxBins = 1u << BITS;

  // ---- the first chunk's backends, then the prologue's loads: all in flight together
  const uint32_t pbeg = c * a.part_pkts;
  const uint32_t pend = min(pbeg + a.part_pkts, a.n_pkts);
  uint32_t pre_bin[kGRounds];
  {
    const uint32_t wb = pbeg + wave * (64u * kGRounds);
#pragma unroll
    for (int r = 0; r < kGRounds; ++r) pre_bin[r] = ld_u16(a.backend, min(wb + r * 64u + lane, a.n_pkts - 1u) * 2u);
  }
  // kScanDirect: L threads per row word, each summing a strided subset of the partition rows (its
  // first kU rows loaded here); kScanKernel: this partition's prefix row and the totals
  constexpr uint32_t kU = 24;
  const uint32_t hw = a.hist16 ? (nbins + 1) >> 1 : nbins;  // row words
  const uint32_t L = hw >= kGBlock ? 1u : kGBlock / hw;
  uint32_t h[kU];
  constexpr uint32_t kCh = (kMaxBins + kGBlock - 1) / kGBlock;
  uint32_t pk[kCh], tk[kCh];
  auto load_rows = [&](uint32_t t, uint32_t q0) {
#pragma unroll
    for (uint32_t k = 0; k < kU; ++k) h[k] = ld_u32(a.part_hist, (min(q0 + k * L, a.n_parts - 1u) * hw + t % hw) * 4u);
  };
  if constexpr (SCAN == kScanDirect) {
    if (tid < hw * L) load_rows(tid, tid / hw);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kCh; ++k) {
      const uint32_t b = min(tid + k * kGBlock, nbins - 1u);
      pk[k] = a.part_prefix[static_cast<size_t>(c) * nbins + b];
      tk[k] = a.totals[b];
    }
  }

  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const uint32_t lt_lo = static_cast<uint32_t>(lt), lt_hi = static_cast<uint32_t>(lt >> 32);
  uint32_t br[kGRounds];  // rank << 16 | bin, or ~0 past the end
  // one chunk's ranks (its backends in pre_bin); afterwards the next chunk's backends are loaded
  auto rank_chunk = [&](uint32_t cbase) {
#pragma unroll
    for (uint32_t k = 0; k < (kMaxBins + 8 + 511) / 512; ++k)
      if ((lane + k * 64) * 8 < cst) reinterpret_cast<uint4*>(mycnt)[lane + k * 64] = make_uint4(0, 0, 0, 0);
    const uint32_t wbase = cbase + wave * (64u * kGRounds);
#pragma unroll
    for (int r = 0; r < kGRounds; ++r) {
      const uint32_t i = wbase + r * 64u + lane;
      const bool valid = i < pend;
      const uint32_t bin = min(pre_bin[r], a.nb);  // the sentinel (and any value > nb, as in hist_kernel)
      // lanes with my bin (and my validity): accumulate, per bit, the lanes whose ballot bit differs
      // from mine; the rest match
      const uint32_t mv = valid ? ~0u : 0u;
      const unsigned long long bv = __builtin_amdgcn_ballot_w64(valid);
      uint32_t mlo = static_cast<uint32_t>(bv) ^ mv, mhi = static_cast<uint32_t>(bv >> 32) ^ mv;
      mismatch_all<BITS>(bin, mlo, mhi);
      const uint32_t elo = ~mlo, ehi = ~mhi;
      // every lane of a bin stores the same new count (no branch); lanes past the end use the
      // scratch slot
      const uint32_t slot = valid ? bin : nbins;
      const uint32_t prior = mycnt[slot];
      mycnt[slot] = static_cast<uint16_t>(prior + __popc(elo) + __popc(ehi));
      const uint32_t rank = prior + __popc(elo & lt_lo) + __popc(ehi & lt_hi);
      br[r] = valid ? (rank << 16) | bin : 0xffffffffu;
    }
    if (cbase + kChunk < pend) {
#pragma unroll
      for (int r = 0; r < kGRounds; ++r)
        pre_bin[r] = ld_u16(a.backend, min(wbase + kChunk + r * 64u + lane, a.n_pkts - 1u) * 2u);
    }
  };
  if (a.perm) rank_chunk(pbeg);

  // ---- prologue: per-bin prefix over earlier partitions (run[0]) and totals
  if constexpr (SCAN == kScanDirect) {
    for (uint32_t b = tid; b < nbp; b += kGBlock) {
      run[b] = 0;
      tot[b] = 0;
    }
    lds_sync();
    // the first (thread, word) pair's rows are loaded already; more than kGBlock row words (many bins,
    // 16-bit rows off) take further pairs
    for (uint32_t t = tid; t < hw * L; t += kGBlock) {
      const uint32_t w = t % hw, j = t / hw;
      if (t != tid) load_rows(t, j);
      uint32_t pre_lo = 0, pre_hi = 0, all_lo = 0, all_hi = 0;
      for (uint32_t q0 = j;;) {
#pragma unroll
        for (uint32_t k = 0; k < kU; ++k) {
          const uint32_t q = q0 + k * L;
          const uint32_t lo = q < a.n_parts ? (a.hist16 ? h[k] & 0xffffu : h[k]) : 0u;
          const uint32_t hi = q < a.n_parts && a.hist16 ? h[k] >> 16 : 0u;
          all_lo += lo;
          all_hi += hi;
          pre_lo += q < c ? lo : 0u;
          pre_hi += q < c ? hi : 0u;
        }
        q0 += kU * L;
        if (q0 >= a.n_parts) break;
        load_rows(t, q0);
      }
      const uint32_t b0 = a.hist16 ? 2 * w : w;
      if (pre_lo) atomicAdd(&run[b0], pre_lo);
      if (all_lo) atomicAdd(&tot[b0], all_lo);
      if (a.hist16 && b0 + 1 < nbins) {
        if (pre_hi) atomicAdd(&run[b0 + 1], pre_hi);
        if (all_hi) atomicAdd(&tot[b0 + 1], all_hi);
      }
    }
    lds_sync();
  }
  // group bases: an exclusive scan of the totals over bins.  Loops have compile-time trip counts
  // (bins < 2^BITS) so that their LDS reads issue back to back.
  if constexpr (SCAN == kScanDirect && kMaxBins <= 128) {  // one wave, <= 2 bins per lane
    if (wave == 0) {
      uint32_t t2[2], s = 0;
#pragma unroll
      for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t b = lane * 2 + k;
        t2[k] = b < nbins ? tot[b] : 0u;
        s += t2[k];
      }
      uint32_t gb = wave_incl_scan(s) - s;
#pragma unroll
      for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t b = lane * 2 + k;
        if (b < nbins) {
          if (c == 0 && a.counts) a.counts[b] = t2[k];
          run[b] += gb;  // group base + prefix over earlier partitions
        }
        gb += t2[k];
      }
    }
  } else {  // the whole block; bin b = tid + k * kGBlock... scanned in thread-major order below
    constexpr uint32_t kCb = (kMaxBins + kGBlock - 1) / kGBlock;  // consecutive bins per thread
    uint32_t tb[kCb], pb[kCb], s = 0;
    if constexpr (SCAN == kScanDirect) {
#pragma unroll
      for (uint32_t k = 0; k < kCb; ++k) {
        const uint32_t b = tid * kCb + k;
        tb[k] = b < nbins ? tot[b] : 0u;
        pb[k] = b < nbins ? run[b] : 0u;
      }
    } else {  // this thread's loaded bins (tid + k * kGBlock) to consecutive ones through LDS
#pragma unroll
      for (uint32_t k = 0; k < kCh; ++k) {
        const uint32_t b = tid + k * kGBlock;
        if (b < nbins) {
          run[b] = pk[k];
          tot[b] = tk[k];
        }
      }
      lds_sync();
#pragma unroll
      for (uint32_t k = 0; k < kCb; ++k) {
        const uint32_t b = tid * kCb + k;
        tb[k] = b < nbins ? tot[b] : 0u;
        pb[k] = b < nbins ? run[b] : 0u;
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < kCb; ++k) s += tb[k];
    uint32_t all;
    uint32_t gb = block_excl_scan_n<kGBlock>(s, s_wave, all);
#pragma unroll
    for (uint32_t k = 0; k < kCb; ++k) {
      const uint32_t b = tid * kCb + k;
      if (b < nbins) {
        if (c == 0 && a.counts) a.counts[b] = tb[k];
        run[b] = pb[k] + gb;
      }
      gb += tb[k];
    }
  }
  if (!a.perm) {
    zero_next();
    return;
  }

  // ---- per chunk: wave prefixes per bin, then the stores (the first chunk is ranked already)
  uint32_t par = 0;
  for (uint32_t cbase = pbeg;;) {
    lds_sync();  // every wave's counts of the chunk (and, the first time, run[]) are in LDS
    for (uint32_t b = tid; b < nbins; b += kGBlock) {
      uint32_t s = 0;
#pragma unroll
      for (uint32_t w = 0; w < kW; ++w) {
        const uint32_t t = cnt[w * cst + b];
        cnt[w * cst + b] = static_cast<uint16_t>(s);
        s += t;
      }
      run[(par ^ 1u) * nbp + b] = run[par * nbp + b] + s;
    }
    lds_sync();
    const uint32_t* rb = run + par * nbp;
    const uint32_t wbase = cbase + wave * (64u * kGRounds);
#pragma unroll
    for (int r = 0; r < kGRounds; ++r) {
      if (br[r] != 0xffffffffu) {
        const uint32_t bin = br[r] & 0xffffu;
        a.perm[rb[bin] + mycnt[bin] + (br[r] >> 16)] = wbase + r * 64u + lane;
      }
    }
    cbase += kChunk;
    if (cbase >= pend) break;
    par ^= 1u;
    rank_chunk(cbase);  // its own counter row only: the other waves' prefixes are read by now
  }
  zero_next();
}

// hist_kernel over hm.h[0 .. n): hm.per blocks per batch
int launch_hist(const HistMulti& hm, uint32_t n, void* stream) {
  const size_t lds = static_cast<size_t>(hm.h[0].nb + 1) * 4;
  if (lds > 64 * 1024) {  // many backends: up to 32768 bins (128 KiB), one batch only
    if (n > 1) return set_error(NBG_EINVAL, "hist (multi): at most 16383 bins");
    static bool attr = false;
    if (int rc = raise_lds_limit("hist: LDS attribute: %s", hist_kernel, 160 * 1024, &attr)) return rc;
  }
  return launch_checked(n == 1 ? "hist launch: %s" : "hist launch (multi): %s", hist_kernel, dim3(hm.per * n),
                        dim3(kGBlock), lds, static_cast<hipStream_t>(stream), hm);
}

// scan_kernel over sm.s[0 .. n): blockIdx.y = batch
int launch_scan(const ScanMulti& sm, uint32_t n, void* stream) {
  return launch_checked("scan launch: %s", scan_kernel, dim3((sm.s[0].nbins + kScanBins - 1) / kScanBins, n),
                        dim3(kScanWaves * 64), 0, static_cast<hipStream_t>(stream), sm);
}

// nb + 1 > kMaxGroupBins: two launches over one batch
int launch_group_wide(const GroupArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = launch_checked("bin_base launch: %s", bin_base_kernel, dim3(1), dim3(kGBlock), 0, s, a);
  if (rc) return rc;
  const size_t lds = static_cast<size_t>(a.nb + 1) * 4;
  static bool attr = false;
  if ((rc = raise_lds_limit("group_wide: LDS attribute: %s", group_wide_kernel, 160 * 1024, &attr))) return rc;
  return launch_checked("group_wide launch: %s", group_wide_kernel, dim3(a.n_parts), dim3(64), lds, s, a);
}

}  // namespace

// What an in-place persistent ring leaves of a CU's LDS for one co-resident group block: 160 KiB less
// the ring block's LDS, rounded up to the allocation granule (one ring block per CU; the grouping's
// hist and group kernels run in stream order, so one group block is what must fit beside it).
constexpr size_t kLdsGranule = 512u;
size_t group_lds_beside_ring() {
  const size_t ring = (ring_lds(1) + kLdsGranule - 1) / kLdsGranule * kLdsGranule;
  return 160u * 1024u - ring;
}

// The grouping beside a running ring takes the compact kernel when the default one's block would not
// fit in what the ring leaves.  The compact block fits for every bin count the group kernels take
// (<= 1024 bins: group_lds(1024, true) = 28,800 B, checked by tests/test_cpu_wrapper.py through
// nbg_debug_group_lds); a block that did not would simply wait for the ring to end (stop or idle
// exit), never deadlock: the ring completes its batches without the grouping.
// g_group_compact: -1 = that rule, 0 / 1 = forced (tests and measurements: nbg_debug_set_group_compact,
// or NBG_GROUP_COMPACT read once at the first grouping).
std::atomic<int> g_group_compact{-2};
bool group_compact(uint32_t nbins, bool ring_running) {
  int f = g_group_compact.load(std::memory_order_relaxed);
  if (f == -2) {
    const char* e = std::getenv("NBG_GROUP_COMPACT");
    int v = e ? (std::atoi(e) != 0) : -1;
    g_group_compact.compare_exchange_strong(f, v);
    f = g_group_compact.load(std::memory_order_relaxed);
  }
  if (f >= 0) return f != 0;
  return ring_running && group_lds(nbins, false) > group_lds_beside_ring();
}

auto group_fn(uint32_t bits, int scan, bool compact) {
  if (compact)
    return bits <= 7 ? (scan == kScanDirect ? group_direct_kernel<kScanDirect, 7> : group_direct_kernel<kScanKernel, 7>)
                     : (scan == kScanDirect ? group_direct_kernel<kScanDirect, 10> : group_direct_kernel<kScanKernel, 10>);
  return bits <= 7 ? (scan == kScanDirect ? group_kernel<kScanDirect, 7> : group_kernel<kScanKernel, 7>)
                   : (scan == kScanDirect ? group_kernel<kScanDirect, 10> : group_kernel<kScanKernel, 10>);
}

int launch_group_plan(const GroupPlan& p, void* stream, bool compact) {
  if (p.n == 0 || p.n > kMaxMulti || (p.wide && p.n != 1)) return set_error(NBG_EINVAL, "group (multi): %u batches", p.n);
  int rc;
  if (p.hist_kernel && (rc = launch_hist(p.hm, p.n, stream))) return rc;
  if (p.scan == kScanKernel && (rc = launch_scan(p.sm, p.n, stream))) return rc;
  if (p.wide) return launch_group_wide(p.gm.g[0], stream);
  // one launch grouping gm.g[0 .. n): gm.per blocks per batch
  return launch_checked(p.n == 1 ? "group launch: %s" : "group launch (multi): %s", group_fn(p.bits, p.scan, compact),
                        dim3(p.per * p.n), dim3(kGBlock), group_lds(p.nb + 1, compact), static_cast<hipStream_t>(stream),
                        p.gm);
}

}  // namespace nbg

// Diagnostics (not in include/nbgpu.h; tests only, no GPU needed): force the compact group kernel
// (mode 1), the default one (0) or the library's rule (-1); and the LDS sizes the rule compares.
extern "C" int nbg_debug_set_group_compact(int mode) {
  if (mode < -1 || mode > 1) return NBG_EINVAL;
  nbg::g_group_compact.store(mode);
  return NBG_OK;
}
extern "C" uint64_t nbg_debug_group_lds(uint32_t nbins, int compact) { return nbg::group_lds(nbins, compact != 0); }
extern "C" uint64_t nbg_debug_lds_beside_ring(void) { return nbg::group_lds_beside_ring(); }
