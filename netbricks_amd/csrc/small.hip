// ---- small batches: classify + stable grouping in one launch -------------------------------------
// A batch of at most kSmallMax packets (one grouping partition) and at most kMaxGroupBins bins is
// classified and grouped by one 1024-thread block: NetBricks' own bursts are 32 packets
// (receive_batch.rs:26), where two launches and their gaps were the whole cost of a call.  Wave w
// owns packets [256w, 256w + 256) in four 64-packet rounds.  Per packet: the chunks 0..2 of its
// 64-B window are loaded as three 16-B vectors when the frame allows (aligned, >= 48 B), and it
// takes the fast path (IHL 5) or the byte-wise path.  The loads are coalesced: in a round, load k
// of lane l fetches chunk (64k + l) % 3 of packet (64k + l) / 3, so three neighbouring lanes read one
// packet's 48 contiguous bytes in one instruction (one request per line, where a lane per packet
// touched every line three times, once per instruction: the host path's direct batches read their
// windows over PCIe, uncached); an LDS pass hands each lane its packet's three chunks.  Then each round ranks its lanes among the
// same bin (readlane match) into per-wave counters, one block scan over (bin, wave) in bin-major
// order gives every wave's start per bin, and perm is scattered: per-group FIFO order as the
// reference's producer (group_by.rs:46-51).
#include "kernel_common.h"

namespace nbg {

namespace {

constexpr uint32_t kSmallNT = 1024, kSmallW = kSmallNT / 64;
constexpr uint32_t kSmallMax = 4 * kSmallNT;

// W32 (the host path's 32-B staging, a.win32): window p holds frame bytes 8..39 (the host swapped the
// MACs and staged no bytes below 8), so c[0] is frame bytes 8..23 and c[1] bytes 24..39, and the frame
// starts 8 B before its window; every byte the parse reads for IHL <= 5 lies in it (the host stages a
// batch with a longer IP header in whole 48/64/80-B windows instead).
template <int LUTM, bool F4, bool W32 = false>
__device__ __forceinline__ uint32_t small_classify(const ClassifyArgs& a, uint32_t p, uint32_t off, uint32_t len,
                                                   const uint4* c) {
  if constexpr (W32) {
    uint8_t* w = a.pkts + off;
    if ((reinterpret_cast<uintptr_t>(w) & 15u) == 0 && len >= 40u && ((c[0].y >> 16) & 0xfu) == 5u) {
      // frame bytes: IHL 14, protocol 23, src 26..29, dst 30..33, ports 34..37
      const uint32_t src = (c[1].x >> 16) | (c[1].y << 16);
      const uint32_t dst = (c[1].y >> 16) | (c[1].z << 16);
      const uint32_t ports = (c[1].z >> 16) | (c[1].w << 16);
      uint32_t lo, hi;
      fnv_flow(lo, hi, src, dst, ports, c[0].w >> 24);
      return lookup<LUTM, F4>(a, nullptr, lo, hi);
    }
    uint32_t gate;  // reads frame bytes 14 .. min(len, 40) - 1 only (no swap on this path)
    return classify_slow<LUTM, F4, false>(a, nullptr, w - 8, len, p, gate);
  }
  uint8_t* pk = a.pkts + off;
  const bool vec = (reinterpret_cast<uintptr_t>(pk) & 15u) == 0 && len >= 48u;
  if (vec && ((c[0].w >> 16) & 0xfu) == 5u) {
    const uint32_t src = (c[1].z >> 16) | (c[1].w << 16);
    const uint32_t dst = (c[1].w >> 16) | (c[2].x << 16);
    const uint32_t ports = (c[2].x >> 16) | (c[2].y << 16);
    uint32_t lo, hi;
    fnv_flow(lo, hi, src, dst, ports, c[1].y >> 24);
    const uint32_t bin = lookup<LUTM, F4>(a, nullptr, lo, hi);
    if (a.swap) {
      const uint32_t w0 = (c[0].y >> 16) | (c[0].z << 16), w1 = (c[0].z >> 16) | (c[0].x << 16),
                     w2 = (c[0].x >> 16) | (c[0].y << 16);
      if (a.mac_out) {
        uint32_t* mo = reinterpret_cast<uint32_t*>(a.mac_out + static_cast<size_t>(p) * 12u);
        mo[0] = w0;
        mo[1] = w1;
        mo[2] = w2;
      } else {
        *reinterpret_cast<uint4*>(pk) = make_uint4(w0, w1, w2, c[0].w);
      }
    }
    return bin;
  }
  uint32_t gate;
  return classify_slow<LUTM, F4, false>(a, nullptr, pk, len, p, gate);
}

template <int LUTM, bool F4, int BITS, bool W32 = false>
__device__ __forceinline__ void small_body(const ClassifyArgs& a, const GroupArgs& g) {
  extern __shared__ __align__(16) uint32_t sm[];  // small_lds() (after this body) sizes this carve-up
  const uint32_t nbins = a.nb + 1, nbp = (nbins + 3) & ~3u;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t nw = blockDim.x >> 6;  // waves launched: ceil(n / 256)
  uint32_t* cnt = sm;                                            // [nw][nbp]: per-wave counts
  uint16_t* rank16 = reinterpret_cast<uint16_t*>(cnt + kSmallW * nbp);  // [kSmallMax]
  uint16_t* bin16 = rank16 + kSmallMax;                          // [kSmallMax]
  __shared__ uint32_t s_wave[kSmallW];
  const bool group = g.perm || g.counts;
  if (group)
    for (uint32_t i = tid; i < nw * nbp; i += blockDim.x) cnt[i] = 0;
  // this wave's rounds that hold packets (wave-uniform)
  const uint32_t rounds = min(4u, (a.n_pkts - min(a.n_pkts, wave * 256u) + 63u) / 64u);
  // loads of every round first (unconditional, clamped), then every round's classification (its
  // LUT gathers in flight together), then the ranking
  uint32_t off[4], len[4], bin[4];
  uint4 v[4][3];
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) {
    const uint32_t p = min(wave * 256u + r * 64u + lane, a.n_pkts - 1u);
    off[r] = a.off ? a.off[p] : p * a.stride;
    len[r] = a.len ? a.len[p] : a.fixed_len;
  }
  // owned windows (slots of >= 64 B, mbuf data rooms, the host path's staging): the 48 B at every
  // packet start are readable whatever its length, so the window loads do not wait for len[] (over
  // PCIe, for the host path's direct batches, one round trip less per batch)
  const bool owned = a.win_owned != 0;
  constexpr uint32_t kCh = W32 ? 2u : 3u;  // 16-B chunks per window
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) {
    if constexpr (W32) {
      // 32-B windows: lane pair (2i, 2i + 1) reads window i of the round's first 32, then of the last
#pragma unroll
      for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t q = 64u * k + lane, pi = q >> 1, part = q & 1u;
        const uint8_t* w = a.pkts + __shfl(off[r], static_cast<int>(pi));
        const bool vec = (reinterpret_cast<uintptr_t>(w) & 15u) == 0;
        v[r][k] = *reinterpret_cast<const uint4*>((vec ? w : a.pkts) + 16u * part);
      }
      continue;
    }
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      const uint32_t q = 64u * k + lane, pi = q / 3u, part = q - 3u * pi;
      const uint8_t* pk = a.pkts + __shfl(off[r], static_cast<int>(pi));
      bool vec = (reinterpret_cast<uintptr_t>(pk) & 15u) == 0;
      if (!owned) {
        // every lane shuffles (not under `vec &&`: a bpermute from a lane the short-circuit
        // disabled reads 0, and the packet would then take the batch base's window)
        const uint32_t l = __shfl(len[r], static_cast<int>(pi));
        vec = vec && l >= 48u;
      }
      // the batch base is 16-B aligned by the host check; its 48 B are read for packets off the path
      v[r][k] = *reinterpret_cast<const uint4*>((vec ? pk : a.pkts) + 16u * part);
    }
  }
  uint4* tp = reinterpret_cast<uint4*>(bin16 + kSmallMax) + wave * 192u;  // [192] chunks of one round
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) {
#pragma unroll
    for (uint32_t k = 0; k < kCh; ++k) tp[64u * k + lane] = v[r][k];
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();  // one wave: its LDS operations run in issue order
    uint4 c[3];
#pragma unroll
    for (uint32_t k = 0; k < kCh; ++k) c[k] = tp[kCh * lane + k];
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();  // the next round's writes after these reads
    const uint32_t p = wave * 256u + r * 64u + lane;
    bin[r] = 0xffffffffu;
    if (r < rounds && p < a.n_pkts) bin[r] = small_classify<LUTM, F4, W32>(a, p, off[r], len[r], c);
  }
  // backend[] after every round's gathers: vmcnt counts stores too and retires in order, so a store
  // issued between two rounds' LUT gathers made the second gather's wait also wait for the store (a
  // PCIe round trip for the host path's direct batches)
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) {
    const uint32_t p = wave * 256u + r * 64u + lane;
    if (r < rounds && p < a.n_pkts) a.backend[p] = static_cast<uint16_t>(bin[r] == a.nb ? kSentinel : bin[r]);
  }
  if (!group) return;
  lds_sync();  // counters zeroed
  uint32_t* wc = cnt + wave * nbp;
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t p = wave * 256u + r * 64u + lane;
    const bool valid = p < a.n_pkts;
    const uint32_t b = valid ? bin[r] : 0u;
    uint32_t rank, count;
    wave_match_rank<BITS>(b, valid, lane, rank, count);
    // every lane of a bin reads the same count and stores the same new one (one wave: its LDS
    // operations execute in issue order)
    const uint32_t before = wc[b];
    __builtin_amdgcn_wave_barrier();
    if (valid) {
      rank16[p] = static_cast<uint16_t>(before + rank);
      bin16[p] = static_cast<uint16_t>(b);
      wc[b] = before + count;
    }
    __builtin_amdgcn_wave_barrier();
  }
  lds_sync();
  // exclusive scan over the counters in (bin, wave) order; each thread owns `per` consecutive
  // entries; the waves' partial sums are combined through s_wave
  const uint32_t ne = nbins * nw, per = (ne + blockDim.x - 1) / blockDim.x;
  uint32_t sum = 0;
  for (uint32_t k = 0; k < per; ++k) {
    const uint32_t e = tid * per + k;
    sum += e < ne ? cnt[(e % nw) * nbp + e / nw] : 0u;
  }
  const uint32_t xs = wave_incl_scan(sum);
  if (lane == 63u) s_wave[wave] = xs;
  // counts: a bin's packets = the sum of its wave counters (read before they are replaced)
  if (g.counts)
    for (uint32_t b = tid; b < nbins; b += blockDim.x) {
      uint32_t t = 0;
      for (uint32_t w = 0; w < nw; ++w) t += cnt[w * nbp + b];
      g.counts[b] = t;
    }
  lds_sync();
  uint32_t x = xs - sum;
  for (uint32_t w = 0; w < wave; ++w) x += s_wave[w];
  for (uint32_t k = 0; k < per; ++k) {
    const uint32_t e = tid * per + k;
    if (e < ne) {
      const uint32_t v = cnt[(e % nw) * nbp + e / nw];
      cnt[(e % nw) * nbp + e / nw] = x;
      x += v;
    }
  }
  lds_sync();
  if (g.perm) {
    // perm is scattered in LDS (the load-transpose area, free now: 3 KB per wave >= 4 B per packet)
    // and stored in order, 16 B per lane: scattered 4-B stores were a partial line each, and over
    // PCIe (the host path's direct batches) a write of its own for the block's system fence to wait
    // for (host-batch server at 16 pipelines: 41.5 us body + 27.4 us fence per 992-packet batch)
    uint32_t* pl = reinterpret_cast<uint32_t*>(bin16 + kSmallMax);
    for (uint32_t p = tid; p < a.n_pkts; p += blockDim.x) pl[cnt[(p >> 8) * nbp + bin16[p]] + rank16[p]] = p;
    lds_sync();
    if ((reinterpret_cast<uintptr_t>(g.perm) & 15u) == 0) {
      for (uint32_t i = 4u * tid; i < a.n_pkts; i += 4u * blockDim.x) {
        if (i + 4u <= a.n_pkts) {
          *reinterpret_cast<uint4*>(g.perm + i) = *reinterpret_cast<const uint4*>(pl + i);
        } else {
          for (uint32_t j = i; j < a.n_pkts; ++j) g.perm[j] = pl[j];
        }
      }
    } else {
      for (uint32_t i = tid; i < a.n_pkts; i += blockDim.x) g.perm[i] = pl[i];
    }
  }
}

}  // namespace

// small_body's dynamic LDS as it is carved up at its top:
// counters [kSmallW][nbp], rank16 / bin16 [kSmallMax], then a 3-KB load transpose area per wave
size_t small_lds(uint32_t nb, uint32_t waves) {
  return (kSmallW * (((nb + 1) + 3) & ~3u)) * 4u + kSmallMax * 4u + waves * 192u * 16u;
}

namespace {

// done (nullable): a completion word in pinned host memory (nbg_maglev_host_submit's direct path), set
// to done_val once every output of the batch is visible to the host: each thread's stores are
// released at system scope, then, behind the block barrier, one vector store of the word.  The host
// polls it with plain loads instead of querying an event through the runtime.
template <int LUTM, bool F4, int BITS, bool W32>
__global__ __launch_bounds__(kSmallNT) void small_kernel(ClassifyArgs a, GroupArgs g, uint32_t* done, uint32_t done_val) {
  small_body<LUTM, F4, BITS, W32>(a, g);
  if (done) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(done, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- host-batch server (nbg_host_ring_*) ---------------------------------------------------------
// One launch per GPU serves every producer thread's small host batches (nbg_maglev_host_submit's
// direct path) without a kernel launch per batch: the GPU's dispatch rate, ~200k launches/s per GPU
// measured with 16 producer threads, capped the drop-in path at ~200 Mpps at the
// reference's 992-packet batches.  Each 1024-thread block: claim the next ticket (device atomic), wait
// for its descriptor in pinned host memory (thread 0 polls seq with s_sleep; exits on the host's stop,
// or after idle_ticks without any post), copy it to LDS, acknowledge it, run the small kernel's body
// on it, set the batch's completion word.  Every posted ticket is claimed by some block before any
// block can exit on a stop (tickets are claimed in order and a block exits only at an unposted one).
__global__ __launch_bounds__(kSmallNT) void host_ring_kernel(HostRingArgs r) {
  __shared__ __align__(16) uint32_t s_desc[kHostRingDescBytes / 4];
  __shared__ uint32_t s_ticket, s_go;
  const uint32_t tid = threadIdx.x;
  for (;;) {
    if (tid == 0) {
      const uint32_t t = __hip_atomic_fetch_add(r.claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t* seq = reinterpret_cast<const uint32_t*>(r.desc + static_cast<size_t>(t & (r.slots - 1u)) *
                                                                           kHostRingDescBytes);
      uint64_t t_act = wall_clock64();
      uint32_t seen = __hip_atomic_load(&r.ctl->posted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      uint32_t go = 0;
      for (uint32_t nap = 1;; nap = min(2u * nap, 8u)) {
        if (__hip_atomic_load(seq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == t + 1u) {
          go = 1;
          break;
        }
        if (__hip_atomic_load(&r.ctl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) break;
        const uint32_t p = __hip_atomic_load(&r.ctl->posted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (p != seen) {
          seen = p;
          t_act = wall_clock64();
        } else if (static_cast<uint64_t>(wall_clock64()) - t_act > r.idle_ticks) {
          __hip_atomic_store(&r.ctl->ended, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          break;
        }
        for (uint32_t i = 0; i < nap; ++i) __builtin_amdgcn_s_sleep(4);
      }
      s_ticket = t;
      s_go = go;
    }
    __syncthreads();
    if (!s_go) break;
    const uint32_t t = s_ticket;
    uint32_t* d = reinterpret_cast<uint32_t*>(r.desc + static_cast<size_t>(t & (r.slots - 1u)) * kHostRingDescBytes);
    if (tid < sizeof(HostRingDesc) / 4)
      s_desc[tid] = __hip_atomic_load(d + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    if (tid == 0) __hip_atomic_store(d + 1, t + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // ack: reusable
    const HostRingDesc& hd = *reinterpret_cast<const HostRingDesc*>(s_desc);
    const ClassifyArgs a = hd.a;
    const GroupArgs g = hd.g;
    switch (hd.variant & 15u) {
      case 0: small_body<kGlobalU8, false, 7>(a, g); break;
      case 1: small_body<kGlobalU16, false, 7>(a, g); break;
      case 2: small_body<kGlobalU8, true, 7>(a, g); break;
      case 3: small_body<kGlobalU16, true, 7>(a, g); break;
      case 4: small_body<kGlobalU8, false, 10>(a, g); break;
      case 5: small_body<kGlobalU16, false, 10>(a, g); break;
      case 6: small_body<kGlobalU8, true, 10>(a, g); break;
      case 7: small_body<kGlobalU16, true, 10>(a, g); break;
      case 8: small_body<kGlobalU8, false, 7, true>(a, g); break;
      case 9: small_body<kGlobalU16, false, 7, true>(a, g); break;
      case 10: small_body<kGlobalU8, true, 7, true>(a, g); break;
      case 11: small_body<kGlobalU16, true, 7, true>(a, g); break;
      case 12: small_body<kGlobalU8, false, 10, true>(a, g); break;
      case 13: small_body<kGlobalU16, false, 10, true>(a, g); break;
      case 14: small_body<kGlobalU8, true, 10, true>(a, g); break;
      default: small_body<kGlobalU16, true, 10, true>(a, g); break;
    }
    __threadfence_system();  // this thread's outputs are visible to the host
    __syncthreads();
    if (tid == 0) __hip_atomic_store(hd.done, hd.done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();  // s_desc and the small body's LDS are reused by the next batch
  }
}

}  // namespace

int launch_small(const ClassifyArgs& a, const GroupArgs& g, bool wide_lut, void* stream, uint32_t* done,
                 uint32_t done_val) {
  using Fn = void (*)(ClassifyArgs, GroupArgs, uint32_t*, uint32_t);
  static const Fn kFns[16] = {
      small_kernel<kGlobalU8, false, 7, false>,  small_kernel<kGlobalU16, false, 7, false>,
      small_kernel<kGlobalU8, true, 7, false>,   small_kernel<kGlobalU16, true, 7, false>,
      small_kernel<kGlobalU8, false, 10, false>, small_kernel<kGlobalU16, false, 10, false>,
      small_kernel<kGlobalU8, true, 10, false>,  small_kernel<kGlobalU16, true, 10, false>,
      small_kernel<kGlobalU8, false, 7, true>,   small_kernel<kGlobalU16, false, 7, true>,
      small_kernel<kGlobalU8, true, 7, true>,    small_kernel<kGlobalU16, true, 7, true>,
      small_kernel<kGlobalU8, false, 10, true>,  small_kernel<kGlobalU16, false, 10, true>,
      small_kernel<kGlobalU8, true, 10, true>,   small_kernel<kGlobalU16, true, 10, true>};
  const Fn fn = kFns[small_variant(wide_lut, a.m, a.nb, a.win32 != 0)];
  const uint32_t waves = (a.n_pkts + 255u) / 256u;  // 1..16: a wave per 256 packets
  const size_t lds = small_lds(a.nb, waves);
  if (lds > 64 * 1024)  // every such launch: the variants share no flag
    if (int rc = raise_lds_limit("small: LDS attribute: %s", fn, lds)) return rc;
  return launch_checked("small launch: %s", fn, dim3(1), dim3(64 * waves), lds, static_cast<hipStream_t>(stream), a, g,
                        done, done_val);
}

uint32_t small_max() { return kSmallMax; }

// host_ring_kernel's dispatch over the small kernel's instantiations (as launch_small picks them)
uint32_t small_variant(bool wide_lut, uint32_t m, uint32_t nb, bool win32) {
  return (wide_lut ? 1u : 0u) | (m == 65537u ? 2u : 0u) | (nb + 1 > 128 ? 4u : 0u) | (win32 ? 8u : 0u);
}

int launch_host_ring(const HostRingArgs& r, uint32_t blocks, void* stream) {
  const size_t lds = small_lds(kMaxGroupBins - 1, kSmallW);  // any handle's batch: up to 1023 backends
  if (int rc = raise_lds_limit("host ring: LDS attribute: %s", host_ring_kernel, lds)) return rc;  // every launch
  return launch_checked("host ring launch: %s", host_ring_kernel, dim3(blocks), dim3(kSmallNT), lds,
                        static_cast<hipStream_t>(stream), r);
}

}  // namespace nbg
