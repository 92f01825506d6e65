// Host policy of the classify half of a call: which of the five kernels it takes (small, tiled
// lookup, streaming, streaming over descriptors, tile per wave), the LUT's source, the layout rules,
// the write mode and the launch geometry, in one ClassifyRoute for every launch site
// (nbgpu_api.hip).  No HIP, no allocation.
#include <algorithm>
#include <cstdlib>

#include "nbgpu_internal.h"

namespace nbg {

namespace {

bool env_on(const char* name) {
  const char* e = std::getenv(name);
  return !e || std::atoi(e) != 0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

bool wide(const RouteFacts& f) { return f.nb > 256; }  // u16 LUT entries

// Kernels that need a whole CU's LDS (the streaming kernels, the LDS-staged LUT) would wait for a
// persistent ring on the device to end: batches then take the tile-per-wave kernel, which co-runs in
// the LDS the ring leaves free.
bool ring_runs(const RouteFacts& f) { return f.device < 0 ? f.ring_forced : device_ring_running(f.device); }

// Batches of at most 2048 packets take the single-launch small kernel (one block: 3.5 us per call
// back to back at 32 packets and 6.9 us at 1024, against 9.5 and 10.6 us for classify + group; at
// 4096 packets one CU is too little: 14.1 against 11.0 us, profiles/r02_small_batches.json).
// NBG_SMALL=0 disables it (A/B measurements).
bool use_small(const RouteFacts& f, const ClassifyCall& c) {
  static const bool on = env_on("NBG_SMALL");
  return on && !c.lpm && c.n_pkts <= std::min<uint32_t>(small_max(), 2048) && f.nb + 1 <= kMaxGroupBins &&
         !(c.flags & (NBG_DEFER_GROUP | NBG_LUT_LDS | NBG_LUT_TILED)) && aligned16(c.pkts);
}

// The streaming classify kernel serves lean fixed slots with a u8 LUT of at most 65537 entries
// (config C2); NBG_STREAM=0 selects the tile-per-wave kernel instead (A/B measurements).
// Below ~2 units per block the per-block LUT staging (64 KiB from L2 for every CU) is not
// amortised: smaller batches take the tile-per-wave kernel.
bool use_stream(const RouteFacts& f, uint64_t n_pkts) {
  static const bool on = env_on("NBG_STREAM");
  return on && !wide(f) && f.m <= 65537 && n_pkts >= 262144 && !ring_runs(f);
}

// NBG_STREAM_DESC: descriptor layouts (IMIX offsets + lengths) with owned windows take the
// streaming kernel too: the u8 LUT staged in LDS (read only, records, or the lpm chain), or the u16
// LUT gathered from L2 (any mode, no chain).  The in-place mode with the u8 LUT does not fit LDS.
// Opt-in: one stream, it classifies C5 in 27.1 us against 28.7 for the tile-per-wave kernel, but it
// holds all LDS of every CU, so with three streams the tile-per-wave kernels co-running beat it
// (profiles/r02_stream_desc_ab.txt).
bool use_stream_desc(const RouteFacts& f, const ClassifyCall& c, int mode) {
  if (!(c.flags & NBG_STREAM_DESC) || c.n_pkts < 262144 || ring_runs(f)) return false;
  if (wide(f)) return !c.lpm;
  return f.m <= 65537 && mode != 1;
}

}  // namespace

bool lean_slots(bool owned, uint32_t stride, uint32_t fixed_len, const void* base) {
  return owned && stride % 16 == 0 && fixed_len >= 48 && aligned16(base);
}

// A chained call swaps nothing (lpm's and maglev's swaps cancel).
int write_mode(uint32_t flags, bool records, bool chain) {
  return chain || !(flags & NBG_SWAP_MACS) ? 0 : (records ? 2 : 1);
}

// One block per CU, or NBG_STREAM_GRID (measurement: 1..CUs).
int stream_grid(int cus) {
  static const int forced = [] {
    const char* e = std::getenv("NBG_STREAM_GRID");
    return e ? std::atoi(e) : 0;
  }();
  return forced > 0 && forced <= cus ? forced : cus;
}

ClassifyRoute pick_route(const RouteFacts& f, const ClassifyCall& c, bool capturing, const GroupPlan& gp) {
  ClassifyRoute r{};
  // The LUT is gathered from L2 by default (measured faster: the LDS-staged copy costs occupancy);
  // NBG_LUT_LDS stages it in LDS when it fits.
  r.lds_lut = (c.flags & NBG_LUT_LDS) && f.lut_bytes <= 72 * 1024 && !ring_runs(f);
  // a 64-B window per packet start is owned: fixed slots of >= 64 B, or the caller says so
  r.win_owned = (!c.off && c.stride >= 64) || (c.flags & NBG_OWNED_WINDOWS);
  r.lean = !c.off && !c.len && lean_slots(r.win_owned, c.stride, c.fixed_len, c.pkts);
  r.mode = write_mode(c.flags, c.mac_out != nullptr, c.lpm != nullptr);
  if (use_small(f, c))
    r.kernel = kKernelSmall;
  else if ((c.flags & NBG_LUT_TILED) && wide(f) && !c.lpm)
    r.kernel = kKernelTiled;
  else if (r.lean && !r.lds_lut && !c.lpm && use_stream(f, c.n_pkts))
    r.kernel = kKernelStream;
  else if (c.off && r.win_owned && !r.lds_lut && aligned16(c.pkts) && use_stream_desc(f, c, r.mode))
    r.kernel = kKernelStreamDesc;  // lengths given, or filled (below)
  else
    r.kernel = kKernelTileWave;
  // Descriptor kernels read off[] and len[] both; the small kernel reads fixed_len itself.
  r.fill_len = c.off && !c.len && r.kernel != kKernelSmall;

  // each wave walks tpw consecutive 64-packet tiles (software-pipelined); the LDS-LUT variant
  // runs a resident grid of 1024-thread blocks so that the LUT staging is amortised
  const uint32_t waves_per_block = (r.lds_lut ? kLdsBlock : kBlock) / 64;
  const uint64_t n_tiles64 = (c.n_pkts + 63) / 64;
  if (r.kernel == kKernelStream) {
    const uint64_t waves = static_cast<uint64_t>(f.cus) * stream_waves_per_block();
    r.tpw = static_cast<uint32_t>((n_tiles64 + waves - 1) / waves);
    r.grid = stream_grid(f.cus);
  } else {
    // a block's packets (64 * waves * tpw, a power of two <= kChunk) must not straddle a partition
    const uint32_t tpw_max = kChunk / (64u * waves_per_block);
    r.tpw = std::min(f.tiles_per_wave, tpw_max);
    if (r.lds_lut) {
      const uint64_t resident = static_cast<uint64_t>(f.grid_lds) * waves_per_block;
      const uint64_t want = (n_tiles64 + resident - 1) / resident;
      r.tpw = 1;
      while (r.tpw < want && r.tpw < tpw_max) r.tpw <<= 1;
    }
    const uint64_t block_tiles = static_cast<uint64_t>(r.tpw) * waves_per_block;
    r.grid = r.kernel == kKernelStreamDesc ? f.cus : static_cast<int>((n_tiles64 + block_tiles - 1) / block_tiles);
  }
  // NBG_GROUP_LAG: the batch's grouping is left pending (carried by the next call's launch) when it
  // takes the streaming kernel with in-kernel histograms and the direct scan, one block per partition
  r.lag = r.kernel == kKernelStream && (c.flags & NBG_GROUP_LAG) && !(c.flags & NBG_LUT_TILED) && !capturing &&
          (c.perm || c.counts) && !gp.wide && !gp.hist_kernel && gp.scan == kScanDirect &&
          gp.per <= static_cast<uint32_t>(f.cus) && stream_lds(f.nb, r.mode, true) <= 160u * 1024u;
  return r;
}

bool multi_fused(const RouteFacts& f, const nbg_batch* batches, uint32_t n_batches, uint32_t stride,
                 uint32_t fixed_len, bool group, bool rows_forced, const GroupPlan& gp) {
  uint64_t total = 0;
  bool lean = stride >= 64 && stride < (1u << 24);
  for (uint32_t j = 0; j < n_batches; ++j) {
    lean = lean && batches[j].n_pkts != 0 && lean_slots(true, stride, fixed_len, batches[j].d_pkts);
    total += batches[j].n_pkts;
  }
  const uint32_t nbins = f.nb + 1;
  return lean && nbins <= 256 && use_stream(f, total) &&
         (!group || ((rows_forced || hist_in_classify(nbins)) && gp.scan != kScanKernel));
}

}  // namespace nbg

// Diagnostics (not in include/nbgpu.h; tests only, no GPU needed): the route of one call on a handle
// of nb backends and table size m on a device of `cus` CUs.  layout: 0 fixed slots, 1 offsets +
// lengths, 2 offsets only.  bits: 1 mac_out, 2 chain, 4 base 16-B aligned, 8 capturing, 16 a ring
// runs on the device, 32 grouped.  out: kernel, lds_lut, win_owned, lean, fill_len, lag, mode, tpw, grid.
extern "C" int nbg_debug_classify_route(uint32_t nb, uint64_t m, uint32_t cus, uint32_t grid_lds,
                                        uint32_t tiles_per_wave, int layout, uint32_t stride, uint32_t fixed_len,
                                        uint64_t n_pkts, uint32_t flags, uint32_t bits, uint32_t* out) {
  using namespace nbg;
  if (!out || nb < 1 || m < 2 || cus < 1 || grid_lds < 1 || tiles_per_wave < 1 || layout < 0 || layout > 2 ||
      fixed_len > 65535 || n_pkts < 1 || n_pkts >= (1ull << 30))
    return NBG_EINVAL;
  const bool is_wide = nb > 256;
  RouteFacts f{};
  f.nb = nb;
  f.m = m;
  f.lut_bytes = static_cast<uint32_t>((m * (is_wide ? 2 : 1) + 15) & ~uint64_t(15));
  f.cus = static_cast<int>(cus);
  f.grid_lds = static_cast<int>(grid_lds);
  f.tiles_per_wave = tiles_per_wave;
  f.device = -1;
  f.ring_forced = bits & 16u;
  // never dereferenced: only null or not, and the base's alignment
  uint8_t* const base = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>((bits & 4u) ? 4096 : 4104));
  ClassifyCall c{};
  c.pkts = base;
  c.off = layout ? reinterpret_cast<const uint32_t*>(base) : nullptr;
  c.len = layout == 1 ? reinterpret_cast<const uint16_t*>(base) : nullptr;
  c.stride = layout ? 0 : stride;
  c.fixed_len = static_cast<uint16_t>(fixed_len);
  c.n_pkts = n_pkts;
  c.flags = flags;
  c.counts = (bits & 32u) ? reinterpret_cast<uint32_t*>(base) : nullptr;
  c.mac_out = (bits & 1u) ? base : nullptr;
  c.lpm = (bits & 2u) ? reinterpret_cast<const nbg_lpm*>(base) : nullptr;
  GroupPlan gp;
  plan_begin(gp, nb, n_pkts, kRowsClassify);
  const ClassifyRoute r = pick_route(f, c, bits & 8u, gp);
  const uint32_t v[9] = {static_cast<uint32_t>(r.kernel), r.lds_lut, r.win_owned, r.lean, r.fill_len, r.lag,
                         static_cast<uint32_t>(r.mode), r.tpw, static_cast<uint32_t>(r.grid)};
  std::copy(v, v + 9, out);
  return NBG_OK;
}

// The fused rule of nbg_maglev_classify_device_multi for n batches of n_pkts[j] packets in fixed
// slots; bits as above (4 every base aligned, 16 ring, 32 grouped).  Returns 1 fused, 0 not, < 0 bad input.
extern "C" int nbg_debug_multi_fused(uint32_t nb, uint64_t m, uint32_t cus, const uint64_t* n_pkts, uint32_t n,
                                     uint32_t stride, uint32_t fixed_len, uint32_t bits) {
  using namespace nbg;
  if (!n_pkts || nb < 1 || m < 2 || cus < 1 || n == 0 || n > kMaxMulti) return -1;
  RouteFacts f{};
  f.nb = nb;
  f.m = m;
  f.cus = static_cast<int>(cus);
  f.device = -1;
  f.ring_forced = bits & 16u;
  nbg_batch b[kMaxMulti] = {};
  uint64_t max_pkts = 0;
  for (uint32_t j = 0; j < n; ++j) {
    if (n_pkts[j] >= (1ull << 30)) return -1;
    b[j].d_pkts = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>((bits & 4u) ? 4096 : 4104));
    b[j].n_pkts = n_pkts[j];
    max_pkts = std::max(max_pkts, n_pkts[j]);
  }
  GroupPlan gp;
  plan_begin(gp, nb, max_pkts, kRowsClassify);
  return multi_fused(f, b, n, stride, fixed_len, bits & 32u, false, gp) ? 1 : 0;
}
