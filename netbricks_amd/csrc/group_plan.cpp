// Host policy of the grouping (hist -> scan -> group) that follows a classify: the partition size, where
// the partition rows come from, direct scan or scan_kernel, and the kernels' argument structs, in one
// GroupPlan for every launch site (nbgpu_api.hip).  No HIP, no allocation.
#include <algorithm>
#include <cstdlib>

#include "nbgpu_internal.h"

namespace nbg {

// Partition histograms from the classify kernel's per-block flush for few bins, from hist_kernel
// for many (NBG_HIST_KERNEL_BINS overrides the threshold, for measurements).
bool hist_in_classify(uint32_t nbins) {
  static const uint32_t limit = [] {
    const char* e = std::getenv("NBG_HIST_KERNEL_BINS");
    return e ? static_cast<uint32_t>(std::atoi(e)) : 257u;
  }();
  return nbins < limit;
}

// Default: sum the partition histograms from L2 inside the group kernel while the rows are
// small (every block reads all of them), else a separate scan kernel.  NBG_GSCAN=0/2 forces a mode
// (measurements).
int pick_group_scan(uint32_t nbins, uint32_t n_parts) {
  static const int forced = [] {
    const char* e = std::getenv("NBG_GSCAN");
    return e ? std::atoi(e) : -1;
  }();
  if (forced == kScanKernel || forced == kScanDirect) return forced;
  return static_cast<size_t>(nbins) * n_parts <= 32u * 1024u ? kScanDirect : kScanKernel;
}

void plan_begin(GroupPlan& p, uint32_t nb, uint64_t max_pkts, RowsSource src) {
  p = GroupPlan{};
  const uint32_t nbins = nb + 1;
  // At most kMaxParts partitions of whole chunks.  The two max(.., 1) give a call of only empty
  // batches (descriptor multi) one partition and so a non-empty grid; every other site comes here
  // with at least one packet, where they change nothing.
  const uint64_t chunks = std::max<uint64_t>((max_pkts + kChunk * kMaxParts - 1) / (kChunk * kMaxParts), 1);
  p.nb = nb;
  p.part_pkts = static_cast<uint32_t>(chunks * kChunk);
  p.per = static_cast<uint32_t>(std::max<uint64_t>((max_pkts + p.part_pkts - 1) / p.part_pkts, 1));
  while ((1u << p.bits) < nbins) ++p.bits;
  p.wide = nbins > kMaxGroupBins;
  p.hist_kernel = src != kRowsClassify || !hist_in_classify(nbins);
  p.scan = p.wide ? kScanKernel : pick_group_scan(nbins, p.per);
  // Rows of two 16-bit bins per word where the group kernel sums them itself and a partition's counts
  // stay below 65536: the rows the classify kernel writes, and the ring's rows from hist_kernel.  A
  // handle's hist_kernel rows stay 32-bit.
  const bool packed = p.scan == kScanDirect && p.part_pkts < 65536;
  p.hist16 = packed && (src == kRowsRing || !p.hist_kernel) ? 1u : 0u;
  p.hm.per = p.gm.per = p.per;
}

void plan_add(GroupPlan& p, const uint16_t* backend, uint32_t n_pkts, uint32_t* rows, uint32_t* prefix,
              uint32_t* totals, uint32_t* perm, uint32_t* counts) {
  const uint32_t j = p.n++;
  const uint32_t n_parts = (n_pkts + p.part_pkts - 1) / p.part_pkts;  // 0 for an empty batch
  HistArgs& ha = p.hm.h[j];
  ha.backend = backend;
  ha.n_pkts = n_pkts;
  ha.nb = p.nb;
  ha.part_pkts = p.part_pkts;
  ha.n_parts = n_parts;
  ha.part_hist = rows;
  ha.hist16 = p.hist_kernel ? p.hist16 : 0u;
  ScanArgs& sa = p.sm.s[j];
  sa.part_hist = rows;
  sa.part_prefix = prefix;
  sa.totals = totals;
  sa.n_parts = std::max(n_parts, 1u);  // an empty batch scans row 0 (in bounds, unused: no group block)
  sa.nbins = p.nb + 1;
  GroupArgs& ga = p.gm.g[j];
  ga.backend = backend;
  ga.n_pkts = n_pkts;
  ga.nb = p.nb;
  ga.bits = p.bits;
  ga.n_parts = n_parts;
  ga.part_pkts = p.part_pkts;
  ga.part_hist = rows;
  ga.part_prefix = prefix;
  ga.totals = totals;
  ga.hist16 = p.hist16;
  ga.counts = counts;
  ga.perm = perm;
}

void plan_zero_next(GroupPlan& p, uint32_t* part_hist_next, uint32_t next_words) {
  for (uint32_t j = 0; j < p.n; ++j) {
    p.gm.g[j].part_hist_next = part_hist_next;
    p.gm.g[j].next_words = next_words;
  }
}

void plan_bin_base(GroupPlan& p, uint32_t* bin_base) { p.gm.g[0].bin_base = bin_base; }

}  // namespace nbg

// Diagnostics (not in include/nbgpu.h; tests only, no GPU needed): the plan of n batches of
// n_pkts[j] packets for nb backends, rows_source 0 = a handle's call, 1 = the ring's grouping.
// out: part_pkts, per, scan, hist_kernel, hist16, wide, then n_parts[0 .. n).
extern "C" int nbg_debug_group_plan(uint32_t nb, const uint64_t* n_pkts, uint32_t n, int rows_source, uint32_t* out) {
  using namespace nbg;
  if (!n_pkts || !out || n == 0 || n > kMaxMulti || rows_source < 0 || rows_source > 1) return NBG_EINVAL;
  uint64_t max_pkts = 0;
  for (uint32_t j = 0; j < n; ++j) {
    if (n_pkts[j] >= (1ull << 30)) return NBG_EINVAL;
    max_pkts = std::max(max_pkts, n_pkts[j]);
  }
  GroupPlan p;
  plan_begin(p, nb, max_pkts, rows_source ? kRowsRing : kRowsClassify);
  for (uint32_t j = 0; j < n; ++j)
    plan_add(p, nullptr, static_cast<uint32_t>(n_pkts[j]), nullptr, nullptr, nullptr, nullptr, nullptr);
  const uint32_t head[6] = {p.part_pkts, p.per, static_cast<uint32_t>(p.scan), p.hist_kernel, p.hist16, p.wide};
  std::copy(head, head + 6, out);
  for (uint32_t j = 0; j < n; ++j) out[6 + j] = p.gm.g[j].n_parts;
  return NBG_OK;
}
