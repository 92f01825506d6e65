#!/usr/bin/env python3
"""Benchmark: device-resident Maglev (parse + MAC swap + FNV + LUT + per-backend FIFO grouping).

Workload (BASELINE.json configs[1], "C2"): 65 backends, 65537-slot LUT, 1,048,576 synthetic
64-B UDP frames (60-B frames in 64-B slots) per batch, resident in HBM, MAC swap in place.
One step = one rotation over 8 distinct batches (512 MiB > the 256 MiB Infinity Cache).  NetBricks
runs one pipeline per RX queue (scheduler/context.rs:241-255); the headline path (--headline):
  multi  (default) each step's 8 batches as 2 `nbg_maglev_classify_device_multi` calls of 4 RX
         queues' 1M batches (one streaming classify launch + one group launch per call, every batch
         with its own backend / perm / counts) round-robin on 2 streams;
  launch one `nbg_maglev_classify_device_ex` call per batch round-robin on `--streams` (3) streams
         (rounds 1-2's headline; also reported as variants.launch_in_place);
  ring   the persistent RX ring (nbg_ring_*) with every completed batch grouped on side streams.
The headline runs exactly --warmup untimed steps before its K timed steps.
Calls are made straight through ctypes with prebuilt arguments; every batch of the K steps is fully
classified and grouped between the two synchronisations.  `variants.in_place_lag` is the launch
path with NBG_GROUP_LAG (batch i grouped inside batch i+1's classify launch; slower).

Process model.  `python bench.py --gpus N` is a launcher: it never touches the GPU, spawns N
rank processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 in their environment),
waits for them and prints rank 0's JSON line.  `--gpus 1` runs one rank through the same code.
Under `torch.distributed.run` (WORLD_SIZE already set) the process is a rank itself.  Every rank
owns its own batches (weak scaling, no data-path collective in the timed region); the LUT is
built on rank 0 and broadcast once over RCCL (setup, untimed).  `--selftest` runs the same
launcher and rank logic on the CPU with gloo and no HIP call (the CPU test of the launcher).

A plain run (`--gpus 1 --steps K --warmup W`) does what the headline needs and no more: traces and
handles, W untimed steps, K timed steps, `--dump-outputs DIR` (what the last timed step computed, as
.npy files: see dump_outputs) and the line.  Everything below is measured only with `--full`, which
also writes the full record file.

Roofline: the dominant kernel (the headline path's classify launch) is timed with HIP events around
each launch in a separate single-stream pass (grouping deferred past the stop event);
its HBM traffic is measured in the same invocation by two rocprofv3 --pmc passes (FETCH_SIZE,
WRITE_SIZE) of a short child run, at N = 1.  Variants beside the headline: lagged grouping,
records / read-only, several batches per launch, the persistent ring, config C4's per-GPU shard
(131,072 packets per launch or ring batch), and configs C3 / C5 (IMIX).

Prints ONE JSON line (rank 0 / the launcher; see DESIGN.md "Measurement").
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import hashlib
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_BACKENDS = 65
TABLE = 65537
BATCH = 1 << 20
SLOT = 64
FRAME = 60
N_BATCHES = 8           # rotating batches; one step = one rotation (BATCHES_PER_STEP launches)
BATCHES_PER_STEP = N_BATCHES
C4_SHARD = BATCH // 8   # config C4: a 1M batch in 8 contiguous shards, one per GPU
IMIX_BATCHES = 2        # C3 / C5 one call per batch: at least 2 distinct 1M IMIX batches (2 x 374 MB > the MALL),
                        # one per stream (an in-place swap never runs on a buffer another stream's call holds)
# batches per launch of the multi-batch variants and their streams (distinct batch groups in
# flight); the environment overrides are for sweeps (tools/runs/gpu_multi_sweep.sh)
MULTI_K = int(os.environ.get("NBG_BENCH_MULTI_K", "4"))
RING_BATCHES = 4096   # batches per ring pass (variants.ring_*)
RING_GROUP_STREAMS = int(os.environ.get("NBG_BENCH_RING_GROUP_STREAMS", "2"))  # side streams grouping ring batches
# the ring passes' inputs: RING_ROTATE dedicated 1M batches (32 x 64 MiB = 2 GiB, 8x the 256 MiB
# Infinity Cache, so no figure rides on cache hits), checked against pristine copies after every pass
RING_ROTATE = int(os.environ.get("NBG_BENCH_RING_ROTATE", "32"))
WS_SWEEP = tuple(int(x) for x in os.environ.get("NBG_BENCH_WS_SWEEP", "8,16,32").split(","))  # working-set sweep
RING_BACKENDS = 128   # backend[] buffers a ring pass rotates over (more than the 64 slots + the grouping lag)
RING_CHECK = 16       # the last batches of every ring pass, checked against the launch path
RING_GROUP_BURST = int(os.environ.get("NBG_BENCH_RING_GROUP_BURST", "2"))  # 1M batches per nbg_ring_group_burst
C4_GROUP_BURST = int(os.environ.get("NBG_BENCH_C4_GROUP_BURST", "8"))      # C4 shards per nbg_ring_group_burst
C4_GROUP_STREAMS = int(os.environ.get("NBG_BENCH_C4_GROUP_STREAMS", "2"))
MULTI_STREAMS = int(os.environ.get("NBG_BENCH_MULTI_STREAMS", "2"))
# C3 / C5 (IMIX descriptors): batches per multi-batch launch and streams (each stream its own inputs)
IMIX_MULTI_K = int(os.environ.get("NBG_BENCH_IMIX_MULTI_K", "8"))
IMIX_MULTI_STREAMS = int(os.environ.get("NBG_BENCH_IMIX_MULTI_STREAMS", "2"))
SEED = 0x4E42474D41474C56
# --dump-outputs: per batch, backend[] / perm[] at DUMP_SAMPLE seeded packet indices, the MACs of DUMP_PKTS
DUMP_SEED, DUMP_SAMPLE, DUMP_PKTS = 20240607, 1 << 18, 1 << 15
# algorithmic bytes per packet of the classify kernel per variant:
#   in place: 64 B packet read + 12 B MAC write + 2 B backend write
#   records:  64 B packet read + 12 B dense MAC record + 2 B backend
#   read only (north_star's parse + hash + lookup): 64 B read + 2 B backend
# the whole path adds the grouping's 4 B perm write; a lagged launch (classify batch i + group
# batch i-1) moves the whole path's bytes per packet at steady state.
CLASSIFY_BYTES = {"in_place": 64 + 12 + 2, "records": 64 + 12 + 2, "read_only": 64 + 2}
PATH_BYTES = {k: v + 4 for k, v in CLASSIFY_BYTES.items()}
C3_BYTES = {"classify": 64 + 6 + 12 + 2, "path": 64 + 6 + 12 + 2 + 4}      # + u32 off + u16 len
C5_BYTES = {"classify": 64 + 6 + 2 + 2 + 4, "path": 64 + 6 + 2 + 2 + 4 + 4}  # gate + backend + 2 LPM gathers
HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
PMC_WARMUP, PMC_STEPS = 10, 40
# the child's launch sequence, one classify dispatch per call, in this order
PMC_ORDER = ("in_place", "in_place_lag", "records", "read_only", "c4_shard", "c3", "c5")
PMC_MULTI = ("read_only", "in_place")  # then these as multi-batch launches (variants.<name>_multi<K>)
PMC_DESC_MULTI = ("c3", "c5")  # and these with IMIX_MULTI_K descriptor batches per launch (after the ring)
PMC_RING_BATCHES = RING_BATCHES  # then the ring runs (one dispatch each, read only then in place), as timed
NBG_SWAP_MACS, NBG_OWNED_WINDOWS, NBG_DEFER_GROUP, NBG_GROUP_LAG = 0x1, 0x4, 0x10, 0x80


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# ---------------------------------------------------------------------------------------------
# the stdout line: a compact record the driver can read whole (its stdout tail is ~8.3 KB); the
# full record (prose, PMC blocks, sweeps) goes to a file.  The reference's own measurement is a
# one-line rate print (test/maglev/src/main.rs:83-88).
# ---------------------------------------------------------------------------------------------

LINE_LIMIT = 7000  # bytes of the stdout JSON line; bench fails loudly above it
VARIANT_FIELDS = ("us_per_batch", "frac", "pmc_ratio", "classify_us_per_batch")
FULL_RECORD = os.environ.get("NBG_BENCH_FULL", os.path.join("gpurun_out", "bench_full_latest.json"))


def _r(x, nd=4):
    return round(float(x), nd) if isinstance(x, (int, float)) and not isinstance(x, bool) else None


def _variant_row(name, v, pmc):
    """[us per batch (or shard), frac (classify / kernel), PMC hbm/algorithmic, classify us per batch]."""
    if not isinstance(v, dict):
        return None
    if "error" in v and "value" not in v and "us_per_batch" not in v:
        return "error: " + str(v["error"])[:60]
    us = v.get("us_per_batch")
    if us is None and "ms_per_batch" in v:
        us = v["ms_per_batch"] * 1e3
    if us is None:
        us = v.get("us_per_shard")
    ratio = v.get("traffic_ratio")
    pname = "in_place" if name == "launch_in_place" else name  # the same classify launch
    if ratio is None and isinstance(pmc, dict) and isinstance(pmc.get(pname), dict):
        ratio = pmc[pname].get("ratio")
    frac = v.get("frac", v.get("path_frac"))
    return [_r(us, 3), _r(frac), _r(ratio, 3), _r(v.get("classify_us_per_batch"), 2)]


def compact_line(full: dict) -> dict:
    """The driver-facing line: headline, roofline (with PMC traffic), cpu_baseline, north_star, c4,
    e2e and a {variant: [us_per_batch, frac, pmc_ratio, classify_us_per_batch]} map; no prose."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_batch",
            "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "per_gpu_mpps", "lut_digest",
            "rccl_ranks", "comm_backend", "hbm_gbps_per_gpu", "hbm_bytes_per_pkt", "aggregate_frac",
            "steady_state", "north_star", "selftest")
    line = {k: full[k] for k in keep if k in full}
    cfg = full.get("config", {})
    line["config"] = {k: cfg[k] for k in ("workload", "backends", "table_size", "batch_pkts", "slot_bytes",
                                          "mac_swap", "batches_per_launch", "streams", "parallelism") if k in cfg}
    digs = full.get("lut_digest_per_rank")
    if digs:
        line["lut_digests_agree"] = len(set(digs)) == 1
    roof = full.get("roofline")
    if isinstance(roof, dict):
        line["roofline"] = {k: roof[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic",
                                                 "traffic_ratio", "bytes_per_pkt", "pkts_per_launch",
                                                 "batches_per_launch", "avg_launch_us", "us_per_batch")
                            if k in roof}
        if "kernel" in roof:
            line["roofline"]["kernel"] = roof["kernel"].split(" (")[0][:100]
        if isinstance(roof.get("traffic"), (int, float)) and "traffic_ratio" not in roof and roof.get("achieved"):
            alg = roof.get("bytes_per_pkt", 0) * roof.get("pkts_per_launch", 0)
            if alg:
                line["roofline"]["traffic_ratio"] = round(roof["traffic"] / alg, 3)
    cpu = full.get("cpu_baseline")
    if isinstance(cpu, dict):
        line["cpu_baseline"] = {k: cpu[k] for k in ("value", "unit", "cores", "kind", "single_core_mpps",
                                                    "cpu_model") if k in cpu}
        line["cpu_baseline"]["sample"] = str(cpu.get("sample", ""))[:240]
    else:
        line["cpu_baseline"] = cpu
    c4 = full.get("c4")
    if isinstance(c4, dict):
        line["c4"] = {k: ({q: w for q, w in v.items() if q != "what"} if isinstance(v, dict) else v)
                      for k, v in c4.items() if k != "path"}
    e2e = full.get("e2e")
    if isinstance(e2e, dict):
        line["e2e"] = e2e.get("compact", {k: v for k, v in e2e.items() if not isinstance(v, (dict, list))})
    pmc = full.get("pmc")
    variants = full.get("variants")
    if isinstance(variants, dict):
        rows = {}
        for k, v in variants.items():
            if k in ("ws_sweep", "ring_output_checks", "ring_group_sweep", "imix_multi_sweep", "imix_output_checks"):
                continue
            row = _variant_row(k, v, pmc)
            if row is not None:
                rows[k] = row
        sw = variants.get("ws_sweep")
        if isinstance(sw, dict):  # "ws<rot>_<name>": the working-set sweep's rows
            for rot, row in sw.items():
                if isinstance(row, dict):
                    for k, v in row.items():
                        r = _variant_row(k, v, None)
                        if r is not None:
                            rows[f"ws{rot}_{k}"] = r
        line["variants_fields"] = list(VARIANT_FIELDS)
        line["variants"] = rows
        for ck in ("ring_output_checks", "imix_output_checks"):
            if isinstance(variants.get(ck), dict):
                line[ck] = variants[ck]
    if isinstance(pmc, dict) and "error" in pmc:
        line["pmc_error"] = str(pmc["error"])[:200]
    line["full_record"] = FULL_RECORD
    return line


def emit_line(full: dict, record: bool = True) -> None:
    """Write the full record to FULL_RECORD (record=False, a run without --full: no file) and print the
    compact line (one line, <= LINE_LIMIT bytes: a longer one would be cut by a reader that keeps only
    the tail of stdout, so fail loudly instead)."""
    if record:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(FULL_RECORD)), exist_ok=True)
            with open(FULL_RECORD, "w") as f:
                json.dump(full, f, indent=1)
        except OSError as e:
            log(f"bench: could not write the full record {FULL_RECORD}: {e}")
    line = compact_line(full)
    if not record:
        del line["full_record"]
    s = json.dumps(line, separators=(",", ":"))
    if len(s) > LINE_LIMIT:
        log(f"bench: the JSON line is {len(s)} bytes, above the {LINE_LIMIT}-byte limit")
        raise SystemExit(3)
    print(s, flush=True)


# ---------------------------------------------------------------------------------------------
# CPU baseline (rank 0, N = 1): the oracle's C port of the reference's per-core loop
# ---------------------------------------------------------------------------------------------

def cpu_inventory():
    """(CPUs in the affinity mask, cgroup CPU quota in CPUs or None, CPU model).  The GPU box pins a
    256-CPU affinity mask under a 16-CPU cgroup quota: the quota is the share that really runs."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    quota = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = round(int(q) / int(p), 2)
    except Exception:
        pass
    try:
        model = [ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")][0]
    except Exception:
        model = "unknown"
    return cores, quota, model


def spread_cpus(cpus):
    """The CPUs dealt round-robin over their L3 caches (sysfs cache/index3), the order within one L3
    kept: the drop-in path's thread placement (nb_maglev's spread_over_l3), two cores per 8-core CCD at
    16 threads instead of every core of two CCDs."""
    groups = {}
    for c in cpus:
        try:
            key = open(f"/sys/devices/system/cpu/cpu{c}/cache/index3/shared_cpu_list").read().strip()
        except OSError:
            key = "?"
        groups.setdefault(key, []).append(c)
    out, i = [], 0
    while len(out) < len(cpus):
        out += [g[i] for g in groups.values() if i < len(g)]
        i += 1
    return out


def idle_cpus(cpus, sample_s=0.1):
    """(idle, busy): the CPUs other processes kept busy over a short sample of /proc/stat (more than 20 %
    of their time: a shared host's other jobs) apart from the rest, each in the given order (the drop-in
    pipelines' placement, nb_maglev's idle_first, used for the baseline's threads too)."""
    def sample():
        out = {}
        try:
            for ln in open("/proc/stat"):
                f = ln.split()
                if f[0].startswith("cpu") and f[0] != "cpu":
                    v = [int(x) for x in f[1:9]]
                    out[int(f[0][3:])] = (v[0] + v[1] + v[2] + v[5] + v[6] + v[7], sum(v))
        except OSError:
            pass
        return out
    a = sample()
    time.sleep(sample_s)
    b = sample()
    idle, busy = [], []
    for c in cpus:
        if c in a and c in b and b[c][1] > a[c][1] and (b[c][0] - a[c][0]) * 5 > b[c][1] - a[c][1]:
            busy.append(c)
        else:
            idle.append(c)
    return idle, busy


def cpu_baseline(host_bufs, lut, target_cpu_s=8.0):
    """The reference's per-core producer loop restated in C (oracle/, kind "port"), timed on this
    host's cores: MAC swap, ipv4_extract_flow, FNV-1a, the FNV-keyed memo map (nf.rs:91,104),
    lut[hash % M], 32-packet bursts, enqueue into per-group 1024-slot rings.  One pinned thread per
    allowed core, each streaming its contiguous shard of all 8 batches (512 MiB: DRAM, not cache)
    `reps` times; single-core and no-memo-map variants beside."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orc  # test infrastructure: the oracle is the baseline/checker only

    L = orc.lib()
    affinity, quota, model = cpu_inventory()
    cores = max(1, min(affinity, int(quota))) if quota else affinity  # threads that can run at once
    lut32 = np.ascontiguousarray(lut, dtype=np.uint32)
    buf = np.concatenate(host_bufs)
    n_all = BATCH * len(host_bufs)

    def run(n, threads, reps, cache):
        return L.orc_cpu_baseline_reps(buf.ctypes.data, None, SLOT, None, FRAME, n, lut32.ctypes.data, TABLE,
                                       N_BACKENDS, 1 if cache else 0, threads, reps, None)

    def measure(n, threads, cache, cpu_s):
        t = run(n, threads, 1, cache)  # cold pass: page faults, memo fill; also sizes the sample
        reps = int(min(max(1, cpu_s / max(t * threads, 1e-6)), 10000))
        s = run(n, threads, reps, cache)
        return n * reps / s / 1e6, reps, s * threads

    # the threads on idle CPUs first (as the drop-in path's pipelines: a shared host's other jobs keep
    # some cores busy), in CPU order, then dealt over the L3 caches as the drop-in path deals its
    # pipelines: the baseline is the faster of the two placements
    idle, busy = idle_cpus(sorted(os.sched_getaffinity(0)))

    def placed(order):
        arr = (C.c_int * len(order))(*order)
        L.orc_set_cpu_order(arr, len(order))

    try:
        placed((idle + busy)[:cores])
        single, r1, c1 = measure(BATCH, 1, True, 2.0)
        packed, ra, ca = measure(n_all, cores, True, target_cpu_s)
        nocache, rn, cn = measure(n_all, cores, False, target_cpu_s / 2)
        placed((spread_cpus(idle) + spread_cpus(busy))[:cores])
        spread, rs, cs = measure(n_all, cores, True, target_cpu_s)
    finally:
        L.orc_set_cpu_order(None, 0)
    allc, ra, ca = (spread, rs, cs) if spread > packed else (packed, ra, ca)
    return {"value": round(allc, 1), "unit": "Mpps", "cores": cores, "kind": "port",
            "single_core_mpps": round(single, 2), "no_cache_mpps": round(nocache, 1),
            "packed_mpps": round(packed, 1), "spread_l3_mpps": round(spread, 1),
            "placement": "idle CPUs, spread over L3 caches" if spread > packed else "idle CPUs in order",
            "busy_cpus_skipped": len(busy),
            "affinity_cpus": affinity, "cgroup_cpu_quota": quota, "cpu_model": model,
            "sample": f"C port of the reference loop (FNV-keyed memo map nf.rs:91,104, 32-pkt bursts, per-group "
                      f"1024-slot rings) over the {len(host_bufs)} C2 batches ({n_all:,} 64-B UDP packets, 65 backends, "
                      f"M=65537): {cores} pinned threads (min of the {affinity}-CPU affinity mask and the cgroup "
                      f"quota {quota}) x {ra} passes ({ca:.1f} CPU-s); single core {r1} passes "
                      f"over one 1M batch ({c1:.1f} CPU-s); no memo map {rn} passes ({cn:.1f} CPU-s); "
                      f"host CPU: {model}"}


# ---------------------------------------------------------------------------------------------
# multi-rank helpers (shared with tests/test_dist_cpu.py)
# ---------------------------------------------------------------------------------------------

def shard_seed(rank: int, batch: int) -> int:
    """Seed of rank `rank`'s batch `batch`: every rank owns distinct packets (weak scaling)."""
    return SEED + 1000003 * rank + batch


def shared_lut(names, table, rank, world, device):
    """Rank 0 builds the Maglev LUT (Maglev::new, nf.rs:70-76) and broadcasts it once (RCCL over
    xGMI on GPUs, gloo in the CPU tests); every rank returns the same u16 table."""
    import torch
    import torch.distributed as dist

    import netbricks_amd as nb

    lut_t = torch.empty(table, dtype=torch.int32, device=device)
    if rank == 0:
        lut_t.copy_(torch.from_numpy(nb.build_lut(names, table).astype(np.int32)))
    if world > 1:
        dist.broadcast(lut_t, 0)
    return lut_t.cpu().numpy().astype(np.uint16)


def lut_digest(lut) -> str:
    return hashlib.sha256(np.ascontiguousarray(lut, dtype="<u2").tobytes()).hexdigest()[:16]


def scatter_shard(global_buf, out, rank: int, world: int) -> None:
    """Config C4's data-path collective: rank 0 holds the whole batch (world contiguous shards)
    and scatters shard r to rank r (RCCL ncclScatter over xGMI on GPUs; gloo in the CPU tests).
    Shard-major order == global packet order, so per-shard grouping composes."""
    import torch.distributed as dist

    if rank == 0:
        dist.scatter(out, list(global_buf.chunk(world)), src=0)
    else:
        dist.scatter(out, None, src=0)


def gather_results(backend, counts, gbuf, gcounts, rank: int, world: int) -> None:
    """Config C4's return leg: rank 0 collects every shard's backend[] (u16, sent as bytes: RCCL has
    no 16-bit integer type) and per-group counts (RCCL gather over xGMI on GPUs; gloo in the CPU
    tests).  Shard-major order == global packet order."""
    import torch
    import torch.distributed as dist

    b = backend.view(torch.uint8)
    c = counts.view(torch.int32)
    if rank == 0:
        dist.gather(b, list(gbuf.chunk(world)), dst=0)
        dist.gather(c, list(gcounts.chunk(world)), dst=0)
    else:
        dist.gather(b, None, dst=0)
        dist.gather(c, None, dst=0)


def completion_slope(stamps, batches: int):
    """Seconds per batch of a persistent ring in steady state: the slope of (time, batches complete)
    stamps over the middle three quarters of a run of `batches` batches (the ramp after the start and
    the drain at the stop left out).  None when the stamps do not span that window."""
    if len(stamps) < 2:
        return None
    ts = np.array([x[0] for x in stamps], dtype=np.float64)
    cs = np.array([x[1] for x in stamps], dtype=np.int64)
    i0, i1 = np.searchsorted(cs, batches // 8), np.searchsorted(cs, batches - batches // 8)
    if i1 >= len(cs) or i1 <= i0 or cs[i1] == cs[i0]:
        return None
    return float((ts[i1] - ts[i0]) / (cs[i1] - cs[i0]))


def aggregate_frac(total_pkts: float, seconds: float, bytes_per_pkt: int, world: int) -> float:
    """Whole-job HBM fraction: all ranks' algorithmic bytes per second over N x the HBM peak."""
    return round(total_pkts * bytes_per_pkt / seconds / 1e9 / (world * HBM_PEAK_GBPS), 4)


class KernelTimer:
    """HIP events created with hipEventDisableSystemFence (timing only): a default timing event's
    system-scope release writes back and invalidates L2 at every record, which lands inside the
    interval of a kernel that writes (the in-place MAC swap) and inflates its measured duration.
    Uses the HIP runtime torch already loaded (same soname, one runtime per process)."""

    FLAGS = 0x20000000  # hipEventDisableSystemFence

    def __init__(self, n: int):
        import ctypes as C

        self.C = C
        self.hip = C.CDLL("libamdhip64.so.7")
        self.ev = [(C.c_void_p(), C.c_void_p()) for _ in range(n)]
        for a, b in self.ev:
            for e in (a, b):
                rc = self.hip.hipEventCreateWithFlags(C.byref(e), C.c_uint(self.FLAGS))
                if rc != 0:
                    raise RuntimeError(f"hipEventCreateWithFlags failed ({rc})")

    def start(self, i: int, stream: int) -> None:
        self.hip.hipEventRecord(self.ev[i][0], self.C.c_void_p(stream))

    def stop(self, i: int, stream: int) -> None:
        self.hip.hipEventRecord(self.ev[i][1], self.C.c_void_p(stream))

    def ms(self):
        out = []
        for a, b in self.ev:
            self.hip.hipEventSynchronize(b)
            t = self.C.c_float()
            if self.hip.hipEventElapsedTime(self.C.byref(t), a, b) != 0:
                raise RuntimeError("hipEventElapsedTime failed")
            out.append(t.value)
        return np.array(out)

    def close(self) -> None:
        for a, b in self.ev:
            self.hip.hipEventDestroy(a)
            self.hip.hipEventDestroy(b)


# ---------------------------------------------------------------------------------------------
# PMC traffic (launcher, N = 1): two rocprofv3 --pmc passes of a short child run
# ---------------------------------------------------------------------------------------------

def _pmc_rows(d, counter, ring=False, desc=False):
    """Classify-kernel counter values (bytes) in dispatch order from one --pmc pass (ring: the
    persistent ring kernel's dispatches instead; desc: the multi-batch descriptor kernel's)."""
    path = None
    for dp, _, files in os.walk(d):
        for f in files:
            if f.endswith("counter_collection.csv"):
                path = os.path.join(dp, f)
    if path is None:
        raise RuntimeError(f"no counter_collection.csv under {d}")
    rows = []
    for row in csv.DictReader(open(path)):
        name = row.get("Kernel_Name", "")
        want = (("classify_ring_kernel" in name) if ring else ("classify_desc_multi_kernel" in name) if desc
                else ("classify_stream_kernel" in name or "classify_kernel" in name))
        if row.get("Counter_Name") == counter and want:
            rows.append((int(row.get("Dispatch_Id", len(rows))), float(row["Counter_Value"]) * 1024.0,
                         name))
    rows.sort()
    return [v for _, v, _ in rows], [n for _, _, n in rows]


def _pmc_algorithmic(name: str) -> int:
    """Algorithmic bytes of one launch of a PMC_ORDER / multi entry."""
    if name == "in_place_lag":  # lagged: classify this batch + group the previous one (steady state)
        return BATCH * PATH_BYTES["in_place"]
    if name in ("in_place", "records", "read_only"):
        return BATCH * CLASSIFY_BYTES[name]
    if name == "c4_shard":
        return C4_SHARD * CLASSIFY_BYTES["in_place"]
    if name == "c3":
        return BATCH * C3_BYTES["classify"]
    if name == "c5":
        return BATCH * C5_BYTES["classify"]
    base = name.split("_multi")[0]
    return MULTI_K * BATCH * CLASSIFY_BYTES[base]


def pmc_traffic(timeout_s: int = 180):
    """HBM bytes per classify launch for each variant, measured now (MI355X_MICROARCH.md HBM
    section: FETCH_SIZE x2 on gfx950 for 16-B-per-lane streaming reads, WRITE_SIZE as read; both in
    KB).  The child (`--pmc-child`) runs PMC_WARMUP + PMC_STEPS launches of each variant in order."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    env = dict(os.environ, TMPDIR="/tmp")
    vals, names, rvals, dvals = {}, [], {}, {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix=f"nbg_pmc_{counter}_", dir="/tmp")
        cmd = ["timeout", "-k", "5", "-s", "KILL", str(timeout_s), "rocprofv3", "--pmc", counter, "--kernel-trace",
               "-d", d, "-o", "run", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--pmc-child"]
        r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            shutil.rmtree(d, ignore_errors=True)
            return {"error": f"rocprofv3 --pmc {counter} rc={r.returncode}: {r.stderr[-300:]}"}
        try:
            vals[counter], names = _pmc_rows(d, counter)
            rvals[counter], _ = _pmc_rows(d, counter, ring=True)
            dvals[counter], _ = _pmc_rows(d, counter, desc=True)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    seg = PMC_WARMUP + PMC_STEPS
    out = {"counters": "FETCH_SIZE x2 + WRITE_SIZE (separate rocprofv3 --pmc passes, KB = 1024 B)",
           "launches_per_variant": PMC_STEPS}
    order = list(PMC_ORDER) + [f"{v}_multi{MULTI_K}" for v in PMC_MULTI]
    for k, name in enumerate(order):
        f = vals["FETCH_SIZE"][k * seg + PMC_WARMUP:(k + 1) * seg]
        w = vals["WRITE_SIZE"][k * seg + PMC_WARMUP:(k + 1) * seg]
        if len(f) != PMC_STEPS or len(w) != PMC_STEPS:
            if k >= len(PMC_ORDER):
                break  # no multi-batch launches in this run
            return {"error": f"unexpected classify dispatch count ({len(vals['FETCH_SIZE'])}, "
                             f"{len(vals['WRITE_SIZE'])}) at {name}"}
        rd, wr = 2.0 * float(np.mean(f)), float(np.mean(w))
        alg = _pmc_algorithmic(name)
        kname = names[k * seg + PMC_WARMUP] if len(names) > k * seg + PMC_WARMUP else ""
        out[name] = {"read_bytes": round(rd), "write_bytes": round(wr), "hbm_bytes": round(rd + wr),
                     "algorithmic_bytes": alg, "ratio": round((rd + wr) / alg, 3),
                     "kernel": kname.replace("void nbg::(anonymous namespace)::", "").split("(nbg::")[0]}
    rf, rw = rvals.get("FETCH_SIZE", []), rvals.get("WRITE_SIZE", [])
    if len(rf) == 2 and len(rw) == 2:
        # the ring: one dispatch per pass (read only, then in place), RING_BATCHES batches over
        # RING_ROTATE inputs each: the same batch count and working set as the timed passes
        for k, (name, v) in enumerate((("ring_read_only", "read_only"), ("ring_in_place", "in_place"))):
            rd, wr = 2.0 * rf[k], rw[k]
            alg = PMC_RING_BATCHES * BATCH * CLASSIFY_BYTES[v]
            out[name] = {"read_bytes": round(rd), "write_bytes": round(wr), "hbm_bytes": round(rd + wr),
                         "batches": PMC_RING_BATCHES, "working_set_mib": RING_ROTATE * BATCH * SLOT >> 20,
                         "hbm_bytes_per_batch": round((rd + wr) / PMC_RING_BATCHES),
                         "algorithmic_bytes": alg, "ratio": round((rd + wr) / alg, 3),
                         "kernel": f"classify_ring_kernel<true, {k}>"}
    df, dw = dvals.get("FETCH_SIZE", []), dvals.get("WRITE_SIZE", [])
    if len(df) == len(dw) == seg * len(PMC_DESC_MULTI):
        for k, cfg in enumerate(PMC_DESC_MULTI):
            rd = 2.0 * float(np.mean(df[k * seg + PMC_WARMUP:(k + 1) * seg]))
            wr = float(np.mean(dw[k * seg + PMC_WARMUP:(k + 1) * seg]))
            alg = IMIX_MULTI_K * BATCH * (C3_BYTES if cfg == "c3" else C5_BYTES)["classify"]
            out[f"{cfg}_multi{IMIX_MULTI_K}"] = {
                "read_bytes": round(rd), "write_bytes": round(wr), "hbm_bytes": round(rd + wr),
                "algorithmic_bytes": alg, "ratio": round((rd + wr) / alg, 3),
                "read_bytes_per_pkt": round(rd / (IMIX_MULTI_K * BATCH), 1),  # membench IMIX windows: 94.7 B
                "kernel": "classify_desc_multi_kernel"}
    return out


def e2e_block(timeout_s: int = 240):
    """The end-to-end rate over PCIe (north_star: host memory in and out, DPDK mbufs; native/pmd.c:192-206,
    framework/src/operators/packet_batch.rs:78-99), measured by tools/e2e_bench.py in a child process
    after the ranks ended: pipelined H2D -> classify -> D2H, the synchronous and pipelined host-mbuf
    entry points over 2-KiB mbufs, zero-copy over a registered pool, and copies alone."""
    cmd = ["timeout", "-k", "5", str(timeout_s), sys.executable, os.path.join(ROOT, "tools", "e2e_bench.py")]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        return {"error": f"e2e_bench rc={r.returncode}: {r.stderr[-300:]}"}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if not lines:
        return {"error": "e2e_bench printed no JSON line"}
    res = json.loads(lines[-1])
    # the drop-in operator path (nb_maglev --loop: test/maglev's operator chain with the pipelined GPU
    # group_by at the reference's 1024-slot queues and 992-packet batches), 1 / 4 / 16 pipelines
    cmd = ["timeout", "-k", "5", str(timeout_s), sys.executable, os.path.join(ROOT, "tools", "dropin_bench.py")]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        res["dropin"] = {"error": f"dropin_bench rc={r.returncode}: {r.stderr[-300:]}"}
    else:
        d = json.loads(lines[-1])
        res["dropin"] = d
        if isinstance(res.get("compact"), dict):
            res["compact"]["dropin"] = d["dropin"]
    return res


# ---------------------------------------------------------------------------------------------
# launcher
# ---------------------------------------------------------------------------------------------

def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(args, argv) -> int:
    """Spawn args.gpus rank processes (this process never initialises the GPU), wait for all of
    them, and print rank 0's JSON line (+ the PMC traffic at N = 1).  A failing rank ends the job."""
    n = args.gpus
    if n < 1:
        raise SystemExit("--gpus must be >= 1")
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NBG_BENCH_LAUNCHED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr))
    rcs = [None] * n
    out0 = b""
    while any(rc is None for rc in rcs):
        for r, p in enumerate(procs):
            if rcs[r] is None:
                rcs[r] = p.poll()
        if any(rc not in (None, 0) for rc in rcs):
            for r, p in enumerate(procs):
                if rcs[r] is None:
                    p.kill()
                    rcs[r] = p.wait()
            break
        time.sleep(0.05)
    out0 = procs[0].stdout.read()
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
    if bad:
        log(f"bench: rank(s) failed: {bad}")
        return max(abs(rc) for _, rc in bad) or 1
    lines = [ln for ln in out0.decode().splitlines() if ln.startswith("{")]
    if not lines:
        log("bench: rank 0 printed no JSON line")
        return 1
    line = json.loads(lines[-1])
    if n == 1 and not args.selftest and not args.no_pmc:
        t0 = time.time()
        pmc = pmc_traffic()
        log(f"bench: PMC passes {time.time() - t0:.0f}s")
        line["pmc"] = pmc
        roof = line.get("roofline", {})
        variants = line.get("variants", {})
        if isinstance(pmc, dict) and "in_place" in pmc:
            for k, v in variants.items():
                if k in pmc and isinstance(v, dict):
                    v["traffic"] = pmc[k]["hbm_bytes"]
                    v["kernel"] = pmc[k]["kernel"]
            if isinstance(variants.get("launch_in_place"), dict):
                variants["launch_in_place"]["traffic"] = pmc["in_place"]["hbm_bytes"]
        for name in ("ring_read_only", "ring_in_place"):
            ring_v = variants.get(name)
            if isinstance(pmc, dict) and name in pmc and isinstance(ring_v, dict) and "us_per_batch" in ring_v:
                # physical bytes per batch (PMC of the same batch count and working set) over the timed
                # per-batch time: must stay within what HBM can move
                ring_v["traffic_per_batch"] = pmc[name]["hbm_bytes_per_batch"]
                ring_v["traffic_ratio"] = pmc[name]["ratio"]
                ring_v["physical_tbps"] = round(pmc[name]["hbm_bytes_per_batch"] / ring_v["us_per_batch"] / 1e6, 2)
        if not isinstance(pmc, dict) or not roof:
            pass
        elif roof.get("kernel", "").startswith("classify_ring_kernel") and "ring_in_place" in pmc:
            # per launch, like `achieved`: the measured bytes per batch x the timed launch's batches
            roof["traffic"] = pmc["ring_in_place"]["hbm_bytes_per_batch"] * roof["batches_per_launch"]
            roof["traffic_ratio"] = pmc["ring_in_place"]["ratio"]
        elif roof.get("batches_per_launch", 1) > 1 and f"in_place_multi{roof['batches_per_launch']}" in pmc:
            roof["traffic"] = pmc[f"in_place_multi{roof['batches_per_launch']}"]["hbm_bytes"]
        elif "in_place" in pmc:
            roof["traffic"] = pmc["in_place"]["hbm_bytes"]
    if n == 1 and not args.selftest and not args.no_e2e:
        t0 = time.time()
        line["e2e"] = e2e_block()
        log(f"bench: end-to-end pass {time.time() - t0:.0f}s")
    emit_line(line, record=args.full)
    return 0


# ---------------------------------------------------------------------------------------------
# one rank
# ---------------------------------------------------------------------------------------------

def run_rank(args) -> None:
    import torch
    import torch.distributed as dist

    import netbricks_amd as nb

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench: WORLD_SIZE={world} but --gpus {args.gpus}")
    gpu = not args.selftest
    if gpu:
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
    else:
        dev = torch.device("cpu")
    if world > 1:
        if gpu:
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
        if dist.get_world_size() != world:
            raise SystemExit(f"bench: process group has {dist.get_world_size()} ranks, expected {world}")
    comm = None
    if world > 1:
        # the communicator's own rank count: an all-reduce of 1 per rank over it (RCCL on GPUs, gloo in
        # the selftest), so the line shows how many ranks the collective library really connected
        one = torch.ones(1, dtype=torch.int32, device=dev)
        dist.all_reduce(one)
        comm = {"rccl_ranks": int(one.item()), "comm_backend": str(dist.get_backend())}
        if int(one.item()) != world:
            raise SystemExit(f"bench: the communicator counted {int(one.item())} ranks, expected {world}")

    def sync_all():
        if gpu:
            torch.cuda.synchronize(dev)

    def gather_floats(x: float):
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        if world == 1:
            return [x]
        out = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(out, t)
        return [float(o[0]) for o in out]

    names = [f"backend-{i}" for i in range(N_BACKENDS)]
    lut = shared_lut(names, TABLE, rank, world, dev) if world > 1 else nb.build_lut(names, TABLE)
    digest = lut_digest(lut)
    # every rank's LUT digest (first 56 bits as an integer), so rank 0 can show they agree
    digests = [f"{int(v):013x}" for v in gather_floats(float(int(digest[:13], 16)))]

    t0 = time.time()
    host_bufs, dbufs = [], []
    for b in range(1 if args.selftest else N_BATCHES):
        buf, _, _ = nb.make_trace(BATCH, 0, seed=shard_seed(rank, b))
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            host_bufs.append(buf.copy())
        dbufs.append(torch.from_numpy(buf).to(dev) if gpu else torch.from_numpy(buf))
    log(f"[rank {rank}] traces ready in {time.time() - t0:.1f}s")

    S = args.streams
    if gpu:
        from netbricks_amd._lib import lib as clib

        mgs = [nb.Maglev(lut=lut, n_backends=N_BACKENDS, device=local) for _ in range(S)]
        streams = [torch.cuda.Stream(dev) for _ in range(S)]
        # two output sets per stream: with NBG_GROUP_LAG a batch's backend[] is read by the next
        # call's launch (which groups it) while that launch writes its own batch's backend[]
        outs = [[dict(backend=torch.empty(BATCH, dtype=torch.uint16, device=dev),
                      perm=torch.empty(BATCH, dtype=torch.uint32, device=dev),
                      counts=torch.empty(N_BACKENDS + 1, dtype=torch.uint32, device=dev)) for _ in range(2)]
                for _ in range(S)]
        recs = [[torch.empty(BATCH * 12, dtype=torch.uint8, device=dev) for _ in range(2)] for _ in range(S)]
        classify = clib.nbg_maglev_classify_device_ex
        finish = clib.nbg_maglev_finish_group
        hs = [m._h for m in mgs]
        sts = [s.cuda_stream for s in streams]
        pk = [d.data_ptr() for d in dbufs]
        optr = [[(o["backend"].data_ptr(), o["perm"].data_ptr(), o["counts"].data_ptr()) for o in os_] for os_ in outs]
        rptr = [[r.data_ptr() for r in rs] for rs in recs]

    def issue(j, k, par, variant, lag, stream=None, n=BATCH, pkts=None, defer=False):
        """One batch through the C-ABI on handle / stream j, output set par (prebuilt arguments: the
        timed loop pays one ctypes call per batch)."""
        flags = ((NBG_SWAP_MACS if variant != "read_only" else 0) | (NBG_GROUP_LAG if lag else 0)
                 | (NBG_DEFER_GROUP if defer else 0))
        be, pm, ct = optr[j][par]
        rc = classify(hs[j], pk[k] if pkts is None else pkts, None, None, SLOT, FRAME, n, flags, be, pm, ct,
                      rptr[j][par] if variant == "records" else None, sts[j] if stream is None else stream)
        if rc:
            raise RuntimeError(f"nbg_maglev_classify_device_ex: {rc}: {nb._lib.last_error()}")

    def finish_all(stream=None):
        for j in range(S):
            rc = finish(hs[j], sts[j] if stream is None else stream)
            if rc:
                raise RuntimeError(f"nbg_maglev_finish_group: {rc}: {nb._lib.last_error()}")

    def rotation(step, variant, lag, n=BATCH, shard=None):
        """One step: BATCHES_PER_STEP batches round-robin over the streams (global batch index g
        picks the handle g % S and, per handle, alternating output sets)."""
        for q in range(BATCHES_PER_STEP):
            g = step * BATCHES_PER_STEP + q
            j = g % S
            if shard is None:
                issue(j, g % N_BATCHES, (g // S) & 1, variant, lag)
            else:  # C4 shard: packets of shard (g mod 64) of the 8 batches
                s = g % (N_BATCHES * 8)
                issue(j, 0, (g // S) & 1, variant, lag, n=n, pkts=pk[s // 8] + (s % 8) * n * SLOT)

    def timed(variant, steps, warmup, lag, barrier=False, **kw):
        """Whole-job time of `steps` rotations; every rotating batch is warmed first (at least one
        rotation, whatever --warmup says), and lagged groups are finished inside the timed region."""
        if gpu:
            for i in range(max(1, warmup)):
                rotation(i, variant, lag, **kw)
            finish_all()
            sync_all()
            for m in mgs:
                m.check()
        if barrier and world > 1:
            dist.barrier()
        sync_all()
        if gpu:
            start_ev = torch.cuda.Event()
            start_ev.record(torch.cuda.current_stream(dev))
            for st in streams:
                st.wait_event(start_ev)
        t_start = time.perf_counter()
        if gpu:
            for i in range(steps):
                rotation(i, variant, lag, **kw)
            finish_all()
        sync_all()
        el = time.perf_counter() - t_start
        if barrier and world > 1:
            dist.barrier()
        if gpu:
            for m in mgs:
                m.check()
        return el

    def kernel_pass(variant, launches, lag, n=BATCH, shard=False):
        """The classify launch alone: single stream, HIP events around each launch on the stream it
        runs on.  lag: each launch classifies batch i and groups batch i-1 (the first launch, which
        has nothing to group, is left out of the average).  Otherwise the grouping is deferred and
        launched after the stop event."""
        st = sts[0]
        kt = KernelTimer(launches + 1)
        gt = None if lag else KernelTimer(launches + 1)
        for i in range(launches + 1):
            pkts = pk[(i // 8) % N_BATCHES] + (i % 8) * n * SLOT if shard else None
            kt.start(i, st)
            issue(0, i % N_BATCHES, i & 1, variant, lag, stream=st, n=n, pkts=pkts, defer=not lag)
            kt.stop(i, st)
            if not lag:
                gt.start(i, st)
                finish(hs[0], st)
                gt.stop(i, st)
        finish(hs[0], st)
        sync_all()
        c_ms = kt.ms()[1:]
        g_ms = gt.ms()[1:] if gt else None
        kt.close()
        if gt:
            gt.close()
        bpp = PATH_BYTES[variant] if lag else CLASSIFY_BYTES[variant]
        ach = n * bpp / (c_ms.mean() / 1e3) / 1e9
        r = {"avg_launch_us": round(c_ms.mean() * 1e3, 2), "achieved": round(ach, 1),
             "frac": round(ach / HBM_PEAK_GBPS, 4), "bytes_per_pkt": bpp, "pkts_per_launch": n}
        if g_ms is not None:
            r["group_kernel_avg_us"] = round(g_ms.mean() * 1e3, 2)
        return r

    # ---- several batches per launch (nbg_maglev_classify_device_multi): MULTI_K batches of 1M in
    #      one streaming-classify launch and one group launch, each batch with its own outputs
    m_arrs = {}
    if gpu and N_BATCHES % MULTI_K == 0 and (args.headline == "multi" or (world == 1 and not args.no_variants
                                                                          and not args.no_multi)):
        from netbricks_amd._lib import NbgBatch
        m_outs = [(torch.empty(BATCH, dtype=torch.uint16, device=dev), torch.empty(BATCH, dtype=torch.uint32, device=dev),
                   torch.empty(N_BACKENDS + 1, dtype=torch.uint32, device=dev)) for _ in range(N_BATCHES)]
        for g0 in range(N_BATCHES // MULTI_K):
            arr = (NbgBatch * MULTI_K)()
            for q in range(MULTI_K):
                be, pm, ct = m_outs[g0 * MULTI_K + q]
                arr[q] = NbgBatch(dbufs[g0 * MULTI_K + q].data_ptr(), BATCH, be.data_ptr(), pm.data_ptr(), ct.data_ptr(),
                                  None)
            m_arrs[g0] = arr

    def mcall(i, variant, stream, defer=False, j=0):
        flags = (NBG_SWAP_MACS if variant == "in_place" else 0) | (NBG_DEFER_GROUP if defer else 0)
        rc = clib.nbg_maglev_classify_device_multi(hs[j], m_arrs[i % len(m_arrs)], MULTI_K, SLOT, FRAME, flags,
                                                   stream)
        if rc:
            raise RuntimeError(f"nbg_maglev_classify_device_multi: {rc}")

    def multi_pass(variant, calls, warmup):
        """Whole-job rate with MULTI_K batches per call on MULTI_STREAMS streams (distinct batch
        groups in flight), then the multi classify kernel alone (events, grouping deferred)."""
        ms = min(MULTI_STREAMS, len(m_arrs), S)
        for i in range(max(warmup, len(m_arrs))):
            mcall(i, variant, sts[i % ms], j=i % ms)
        sync_all()
        start_ev = torch.cuda.Event()
        start_ev.record(torch.cuda.current_stream(dev))
        for st in streams[:ms]:
            st.wait_event(start_ev)
        t1 = time.perf_counter()
        for i in range(calls):
            mcall(i, variant, sts[i % ms], j=i % ms)
        sync_all()
        el = time.perf_counter() - t1
        st = sts[0]
        kt = KernelTimer(calls)
        for i in range(calls):
            kt.start(i, st)
            mcall(i, variant, st, defer=True)
            kt.stop(i, st)
            finish(hs[0], st)
        sync_all()
        c_ms = kt.ms()
        kt.close()
        for m in mgs:
            m.check()
        ach = MULTI_K * BATCH * CLASSIFY_BYTES[variant] / (c_ms.mean() / 1e3) / 1e9
        return {"value": round(MULTI_K * BATCH * calls / el / 1e6, 1), "unit": "Mpps",
                "ms_per_batch": round(el / (calls * MULTI_K) * 1e3, 5), "batches_per_launch": MULTI_K,
                "streams": ms, "classify_bytes_per_pkt": CLASSIFY_BYTES[variant],
                "pkts_per_launch": MULTI_K * BATCH, "avg_launch_us": round(c_ms.mean() * 1e3, 2),
                "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBPS, 4),
                "what": f"{MULTI_K} batches of 1M (one per RX-queue pipeline) per launch of the streaming classify "
                        "kernel and one group launch (nbg_maglev_classify_device_multi); every batch keeps its own "
                        "backend / perm / counts; frac from the multi-batch classify launch timed alone"}

    def multi_kernel(variant, calls):
        """The multi-batch classify launch alone: one stream, HIP events around each launch (grouping
        deferred and launched after the stop event)."""
        st = sts[0]
        kt = KernelTimer(calls + 1)
        for i in range(calls + 1):
            kt.start(i, st)
            mcall(i, variant, st, defer=True)
            kt.stop(i, st)
            finish(hs[0], st)
        sync_all()
        c_ms = kt.ms()[1:]
        kt.close()
        bpp = CLASSIFY_BYTES[variant]
        ach = MULTI_K * BATCH * bpp / (c_ms.mean() / 1e3) / 1e9
        return {"avg_launch_us": round(c_ms.mean() * 1e3, 2), "achieved": round(ach, 1),
                "frac": round(ach / HBM_PEAK_GBPS, 4), "bytes_per_pkt": bpp, "pkts_per_launch": MULTI_K * BATCH}

    def timed_multi(steps, warmup, barrier=False):
        """The headline with several RX queues' batches per launch: each step's 8 batches as
        BATCHES_PER_STEP / MULTI_K calls of nbg_maglev_classify_device_multi (MULTI_K batches of 1M,
        each with its own backend / perm / counts) round-robin on MULTI_STREAMS streams; bracketed
        like timed()."""
        ms = min(MULTI_STREAMS, len(m_arrs), S)
        cps = BATCHES_PER_STEP // MULTI_K
        for i in range(max(1, warmup) * cps):
            mcall(i, "in_place", sts[i % ms], j=i % ms)
        sync_all()
        for m in mgs:
            m.check()
        if barrier and world > 1:
            dist.barrier()
        sync_all()
        start_ev = torch.cuda.Event()
        start_ev.record(torch.cuda.current_stream(dev))
        for st in streams[:ms]:
            st.wait_event(start_ev)
        t_start = time.perf_counter()
        for i in range(steps * cps):
            mcall(i, "in_place", sts[i % ms], j=i % ms)
        sync_all()
        el = time.perf_counter() - t_start
        if barrier and world > 1:
            dist.barrier()
        for m in mgs:
            m.check()
        return el

    # ---- the persistent RX ring (nbg_ring_*): one resident classify kernel fed batch descriptors
    ring_data = {}

    def ring_setup():
        """RING_ROTATE dedicated 1M batches with pristine copies (the output check), RING_BACKENDS
        backend[] buffers, scratch outputs for the launch-path check."""
        if not ring_data:
            t0 = time.time()
            bufs, orig = [], []
            for b in range(RING_ROTATE):
                buf, _, _ = nb.make_trace(BATCH, 0, seed=shard_seed(rank, 100 + b))
                bufs.append(torch.from_numpy(buf).to(dev))
                orig.append(bufs[-1].clone())
            ring_data.update(
                bufs=bufs, orig=orig,
                be=[torch.empty(BATCH, dtype=torch.uint16, device=dev) for _ in range(RING_BACKENDS)],
                sbe=torch.empty(BATCH, dtype=torch.uint16, device=dev),
                sperm=torch.empty(BATCH, dtype=torch.uint32, device=dev),
                scnt=torch.empty(N_BACKENDS + 1, dtype=torch.uint32, device=dev))
            sync_all()
            log(f"[rank {rank}] ring inputs ({RING_ROTATE} x 64 MiB + copies) ready in {time.time() - t0:.1f}s")
        return ring_data

    def ring_inputs(rotate, n):
        """(buffer, shard) of every distinct input of a pass: whole batches, or (C4) each batch's
        BATCH // n contiguous shards; post i takes input i % len."""
        return [(w, q) for w in range(rotate) for q in range(BATCH // n)]

    def ring_restore(rotate):
        rd = ring_setup()
        for w in range(rotate):
            rd["bufs"][w].copy_(rd["orig"][w])
        sync_all()

    def launch_ref(pkts, n, group=False):
        """The launch path's read-only classification of n packets at pkts (backend[], and with group
        perm / counts) into the scratch outputs: the reference the ring's outputs are checked against."""
        rd = ring_setup()
        st = torch.cuda.current_stream(dev).cuda_stream
        rc = classify(hs[0], pkts, None, None, SLOT, FRAME, n, 0, rd["sbe"].data_ptr(),
                      rd["sperm"].data_ptr() if group else None, rd["scnt"].data_ptr() if group else None, None, st)
        if rc:
            raise RuntimeError(f"launch-path check classify: {rc}: {nb._lib.last_error()}")
        sync_all()

    def ring_check(swap, rotate, n, total, be_of, groups=()):
        """What a ring run of `total` posts left behind: the backend[] of its last RING_CHECK batches
        against the launch path's classification of the same inputs; every input buffer's bytes
        against its pristine copy, MACs swapped iff the run swapped it an odd number of times (in
        place) or untouched (read only); `groups`: (post, perm, counts) of groupings to check."""
        rd = ring_setup()
        ins = ring_inputs(rotate, n)
        bad = []
        for i in range(max(0, total - RING_CHECK), total):
            w, q = ins[i % len(ins)]
            launch_ref(rd["bufs"][w].data_ptr() + q * n * SLOT, n)
            if not torch.equal(rd["sbe"][:n], be_of(i)[:n]):
                bad.append(f"backend of post {i}")
        for i, perm, cnt in groups:
            w, q = ins[i % len(ins)]
            launch_ref(rd["bufs"][w].data_ptr() + q * n * SLOT, n, group=True)
            if not (torch.equal(rd["sperm"][:n], perm[:n]) and torch.equal(rd["scnt"], cnt)):
                bad.append(f"perm/counts of post {i}")
        times = np.bincount(np.arange(total) % len(ins), minlength=len(ins))
        per = BATCH // n
        for w in range(rotate):
            exp = rd["orig"][w]
            odd = [q for q in range(per) if swap and times[w * per + q] % 2]
            if odd:
                exp = exp.clone()
                v, o = exp.view(BATCH, SLOT), rd["orig"][w].view(BATCH, SLOT)
                for q in odd:
                    r0, r1 = q * n, (q + 1) * n
                    v[r0:r1, 0:6] = o[r0:r1, 6:12]
                    v[r0:r1, 6:12] = o[r0:r1, 0:6]
            if not torch.equal(rd["bufs"][w], exp):
                bad.append(f"bytes of buffer {w}")
        out = {"backend_batches": min(RING_CHECK, total), "groupings": len(groups), "buffers": rotate,
               "ok": not bad}
        if bad:
            out["mismatch"] = bad[:8]
            log(f"ring output check FAILED: {bad[:8]}")
        return out

    def ring_pass(variant, batches, n=BATCH, rotate=RING_ROTATE):
        """Per-batch time of the ring in steady state: the producer posts the rotating inputs whenever
        a slot is free (bare ctypes, prebuilt arguments) and stamps every change of the completed
        count; the time per batch is the slope of completions over the middle three quarters of the
        run (no launch, LUT staging or ramp per batch; HIP events cannot bracket a batch inside one
        resident kernel).  No grouping: backend[] (and the in-place swap) only.  The run's outputs are
        checked afterwards (ring_check)."""
        swap = variant == "in_place"
        rd = ring_setup()
        ring_restore(rotate)
        from netbricks_amd._lib import NbgRingBatch

        bes = [b.data_ptr() for b in rd["be"]]
        pks = [rd["bufs"][w].data_ptr() + q * n * SLOT for w, q in ring_inputs(rotate, n)]
        slots = nb._lib.NBG_RING_SLOTS
        # the producer's descriptors, prebuilt: post i of the run is entry i % len(arr); an RX burst
        # is a window of it (nbg_ring_post_burst posts as many as there are free slots)
        per = len(pks) * len(bes) // int(np.gcd(len(pks), len(bes)))
        arr = (NbgRingBatch * (per + slots))()
        for i in range(per + slots):
            arr[i] = NbgRingBatch(pks[i % len(pks)], n, bes[i % len(bes)])
        esz = C.sizeof(NbgRingBatch)
        base_addr = C.addressof(arr)
        k, tk, cc = C.c_uint32(), C.c_uint64(), C.c_uint64()
        ring = mgs[0].ring(swap_macs=swap, stream=streams[0])
        burst, poll, rr = clib.nbg_ring_post_burst, clib.nbg_ring_poll, ring._r

        def post_upto(first, count):
            if burst(rr, C.c_void_p(base_addr + (first % per) * esz), count, C.byref(k), C.byref(tk)):
                raise RuntimeError(f"nbg_ring_post_burst: {nb._lib.last_error()}")
            return k.value

        # an input is posted again only once its previous batch is complete (at most len(pks) batches
        # in flight): a batch must not read a buffer an earlier in-flight batch is still rewriting, nor
        # find its lines freshly written in a cache (round 3's 8-input rotation allowed both)
        cap = min(slots, len(pks))
        try:
            warm = 0
            while warm < 16:  # warm: the kernel is resident and the first inputs touched
                if poll(rr, C.byref(cc)):
                    raise RuntimeError(f"nbg_ring_poll: {nb._lib.last_error()}")
                room = min(16 - warm, cap - (warm - cc.value))
                if room > 0:
                    warm += post_upto(warm, room)
            ring.wait(15)
            base, stamps, posted, done = 16, [], 0, 0
            t0 = time.perf_counter()
            last_move, last_state = t0, None
            while done < batches:
                if (posted, done) != last_state:
                    last_move, last_state = time.perf_counter(), (posted, done)
                elif time.perf_counter() - last_move > 10.0:
                    raise RuntimeError(f"ring_pass stalled: posted {posted} done {done} cap {cap} n {n}")
                room = min(batches - posted, cap - (posted - done))
                if room > 0:
                    posted += post_upto(16 + posted, room)
                if poll(rr, C.byref(cc)):
                    raise RuntimeError(f"nbg_ring_poll: {nb._lib.last_error()}")
                c = cc.value - base
                if c != done:
                    stamps.append((time.perf_counter(), c))
                    done = c
            wall = time.perf_counter() - t0
        finally:
            ring.stop()
        total = 16 + batches
        check = ring_check(swap, rotate, n, total, lambda i: rd["be"][i % len(bes)])
        ts = np.array([x[0] for x in stamps])
        cs = np.array([x[1] for x in stamps])
        if os.environ.get("NBG_BENCH_DUMP"):  # the completion stamps behind us_per_batch (profiles/)
            fn = os.path.join(os.environ["NBG_BENCH_DUMP"], f"ring_{variant}_n{n}_rot{rotate}_b{batches}.csv")
            np.savetxt(fn, np.stack([(ts - ts[0]) * 1e6, cs], 1), fmt="%.3f,%d", header="us_since_first,completed",
                       comments="")
        slope = completion_slope(stamps, batches)
        us = slope * 1e6 if slope else wall / batches * 1e6
        bpp = CLASSIFY_BYTES[variant]
        ach = n * bpp / us / 1e3
        return {"value": round(n / us, 1), "unit": "Mpps", "us_per_batch": round(us, 2),
                "wall_us_per_batch": round(wall / batches * 1e6, 2), "batches": batches, "bytes_per_pkt": bpp,
                "pkts_per_batch": n, "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBPS, 4),
                "working_set_mib": rotate * BATCH * SLOT >> 20, "rotating_inputs": len(pks), "max_in_flight": cap,
                "output_check": check,
                "kernel": f"classify_ring_kernel<true, {1 if swap else 0}>",
                "what": "persistent RX ring (nbg_ring_*): one resident classify kernel (LUT staged once) takes "
                        "batches as the producer posts them through a pinned descriptor ring, relayed into HBM by "
                        "the kernel's last block; per-batch time from the completion slope (middle 3/4 of the "
                        "run); backend[] (+ in-place MAC swap) only, no grouping; outputs checked after the run"}

    ring_res = {}

    def ring_path(batches, n=BATCH, rotate=RING_ROTATE, gstreams=RING_GROUP_STREAMS, gburst=RING_GROUP_BURST,
                  check=False):
        """The whole in-place path on the ring: start the ring (its buffers are kept by the handle after
        the first start), post RX bursts, and enqueue each burst's grouping right away
        (nbg_ring_group_burst: a gate kernel on the side stream waits for the batches' completion in
        HBM, then hist + group launches co-run with the resident ring kernel) round-robin on `gstreams`
        side streams: no host poll between completion and grouping.  A backend[] buffer is reused only
        after the grouping that reads it has run (an event per group burst).  Waits for the last
        grouping and stops the ring.  Returns (wall seconds, ring kernel ms, output check)."""
        from netbricks_amd._lib import NbgRingBatch

        rd = ring_setup()
        if not ring_res:
            ring_res["sides"] = [torch.cuda.Stream(dev) for _ in range(4)]
            ring_res["perm"] = [[torch.empty(BATCH, dtype=torch.uint32, device=dev) for _ in range(8)]
                                for _ in range(4)]
            ring_res["cnt"] = [[torch.empty(N_BACKENDS + 1, dtype=torch.uint32, device=dev) for _ in range(8)]
                               for _ in range(4)]
        sides = ring_res["sides"][:gstreams]
        nbe = len(rd["be"])
        pks = [rd["bufs"][w].data_ptr() + q * n * SLOT for w, q in ring_inputs(rotate, n)]
        slots = nb._lib.NBG_RING_SLOTS
        per = len(pks) * nbe // int(np.gcd(len(pks), nbe))
        arr = (NbgRingBatch * (per + slots))()
        for i in range(per + slots):
            arr[i] = NbgRingBatch(pks[i % len(pks)], n, rd["be"][i % nbe].data_ptr())
        esz, base_addr = C.sizeof(NbgRingBatch), C.addressof(arr)
        k, tk, cc = C.c_uint32(), C.c_uint64(), C.c_uint64()
        cap = min(slots, len(pks))  # an input is reposted only once its previous batch is complete
        sps = [C.c_void_p(x.cuda_stream) for x in sides]
        pps = [(C.c_void_p * gburst)(*[p.data_ptr() for p in ring_res["perm"][q][:gburst]]) for q in range(gstreams)]
        cps = [(C.c_void_p * gburst)(*[c.data_ptr() for c in ring_res["cnt"][q][:gburst]]) for q in range(gstreams)]
        burst, grp, poll = clib.nbg_ring_post_burst, clib.nbg_ring_group_burst, clib.nbg_ring_poll
        evs = {}  # first post of a group burst -> (event after it on its side stream, posts in it)
        last_on = [None] * gstreams  # (first post, count) of the last burst grouped on each side stream
        if check:
            ring_restore(rotate)
        t0 = time.perf_counter()
        ring = mgs[0].ring(swap_macs=True, stream=streams[0])
        rr = ring._r
        stamps = []  # (time, batches complete on the ring) at every change seen by the producer
        try:
            posted = grouped = safe = done = 0  # safe: every grouping of posts < safe has run
            last_move, last_state = time.perf_counter(), None
            while grouped < batches:
                if poll(rr, C.byref(cc)):
                    raise RuntimeError(f"nbg_ring_poll: {nb._lib.last_error()}")
                if cc.value != done:
                    done = cc.value
                    stamps.append((time.perf_counter(), done))
                state = (posted, grouped, safe, done)
                if state != last_state:
                    last_move, last_state = time.perf_counter(), state
                elif time.perf_counter() - last_move > 10.0:  # fail loudly rather than hang the job
                    poll(rr, C.byref(cc))
                    raise RuntimeError(f"ring_path stalled: posted {posted} grouped {grouped} safe {safe} done {done} "
                                       f"ring completed {cc.value} cap {cap} n {n} gburst {gburst} "
                                       f"pending group bursts {sorted(evs)[:4]}")
                # ... and every post stays groupable: a group burst names tickets among the last 64 posted
                want = min(batches - posted, slots - (posted - grouped), safe + nbe - posted, cap - (posted - done))
                if want <= 0:  # the backend[] buffers of the next posts still wait for their grouping
                    while safe in evs and evs[safe][0].query():
                        safe += evs.pop(safe)[1]
                    continue
                if burst(rr, C.c_void_p(base_addr + (posted % per) * esz), want, C.byref(k), C.byref(tk)):
                    raise RuntimeError(f"nbg_ring_post_burst: {nb._lib.last_error()}")
                posted += k.value
                while grouped + gburst <= posted or (grouped < posted and posted == batches):
                    cnt = min(gburst, posted - grouped)
                    q = (grouped // gburst) % gstreams
                    if grp(rr, grouped, cnt, pps[q], cps[q], sps[q]):
                        raise RuntimeError(f"nbg_ring_group_burst: {nb._lib.last_error()}")
                    ev = torch.cuda.Event()
                    ev.record(sides[q])
                    evs[grouped] = (ev, cnt)
                    last_on[q] = (grouped, cnt)
                    grouped += cnt
        finally:
            ring.stop()
        for q, x in enumerate(sides):  # the last groupings; a gate that never opens fails the job loudly
            ev = torch.cuda.Event()
            ev.record(x)
            tq = time.perf_counter()
            while not ev.query():
                if time.perf_counter() - tq > 10.0:
                    raise RuntimeError(f"ring_path: side stream {q} did not drain in 10 s (posted {posted}, grouped "
                                       f"{grouped}, last burst {last_on[q]})")
                time.sleep(1e-4)
        wall = time.perf_counter() - t0
        kms = C.c_float()
        if clib.nbg_ring_kernel_ms(mgs[0]._h, C.byref(kms)):
            raise RuntimeError(f"nbg_ring_kernel_ms: {nb._lib.last_error()}")
        out_check = None
        if check:
            groups = [(f + j, ring_res["perm"][q][j], ring_res["cnt"][q][j])
                      for q, lo in enumerate(last_on) if lo is not None for f, c in [lo] for j in range(c)]
            out_check = ring_check(True, rotate, n, batches, lambda i: rd["be"][i % nbe], groups)
        # steady state, as ring_pass measures the ring alone: the slope of ring completions over the
        # middle three quarters of the run.  Posting is held back by the groupings (a backend[] buffer is
        # reposted only after the grouping that reads it ran), so the slope is the rate of ring +
        # grouping together; `wall` adds the ring's start and stop and the last groupings' drain.
        return wall, float(kms.value), out_check, completion_slope(stamps, batches)

    def ring_grouped(batches, n=BATCH, gstreams=RING_GROUP_STREAMS, gburst=RING_GROUP_BURST):
        """variants.ring_in_place_grouped / c4_shard_ring_grouped: ring_path over `batches` batches (the
        ring's buffers warmed by a first short run), whole-job wall time, the ring kernel's own time and
        the output check of the timed run."""
        ring_path(2 * BATCHES_PER_STEP, n=n, gstreams=gstreams, gburst=gburst)
        wall, kms, chk, slope = ring_path(batches, n=n, gstreams=gstreams, gburst=gburst, check=True)
        wall_us = wall / batches * 1e6
        us = slope * 1e6 if slope else wall_us
        ach_path = n * PATH_BYTES["in_place"] / us / 1e3
        ach = batches * n * CLASSIFY_BYTES["in_place"] / (kms * 1e-3) / 1e9
        return {"value": round(n / us, 1), "unit": "Mpps", "us_per_batch": round(us, 2),
                "wall_us_per_batch": round(wall_us, 2), "batches": batches,
                "pkts_per_batch": n, "path_bytes_per_pkt": PATH_BYTES["in_place"],
                "path_frac": round(ach_path / HBM_PEAK_GBPS, 4),
                "group_streams": gstreams, "group_burst": gburst, "working_set_mib": RING_ROTATE * BATCH * SLOT >> 20,
                "ring_kernel_us": round(kms * 1e3, 1), "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBPS, 4),
                "output_check": chk,
                "what": "in place + grouping on the persistent ring: RX bursts posted to the resident classify kernel, "
                        "each burst's grouping enqueued right after the post (nbg_ring_group_burst: a gate kernel "
                        "waits on the side stream for the batches' completion word in HBM, then hist + group co-run "
                        "with the ring), no host poll; us_per_batch from the slope of ring completions over the middle "
                        "3/4 of the run (posting is held back by the groupings: the rate of ring + grouping), "
                        "wall_us_per_batch the whole job incl. ring start/stop (path_frac at 82 B/pkt); frac from "
                        "the ring kernel's HIP-event time"}

    def timed_ring(steps, warmup, barrier=False):
        """The headline on the ring: `steps` rotations (steps x 8 batches) through ring_path, bracketed
        by a barrier + device synchronisation (the ring is started and stopped inside the bracket);
        warmed first by `warmup` rotations (the ring's buffers allocated, every input touched)."""
        ring_path(max(1, warmup) * BATCHES_PER_STEP)
        if barrier and world > 1:
            dist.barrier()
        sync_all()
        t_start = time.perf_counter()
        _, kms, _, _ = ring_path(steps * BATCHES_PER_STEP)
        sync_all()
        el = time.perf_counter() - t_start
        if barrier and world > 1:
            dist.barrier()
        mgs[0].check()
        return el, kms

    def multi_rot_kernel(variant, rotate, calls):
        """The multi-batch classify launch alone (HIP events, grouping deferred) over the ring's inputs
        rotated through `rotate` batches (MULTI_K per launch): the working-set sweep's launch path."""
        from netbricks_amd._lib import NbgBatch

        rd = ring_setup()
        ring_restore(rotate)
        outs_ = [(torch.empty(BATCH, dtype=torch.uint16, device=dev), torch.empty(BATCH, dtype=torch.uint32, device=dev),
                  torch.empty(N_BACKENDS + 1, dtype=torch.uint32, device=dev)) for _ in range(2 * MULTI_K)]
        arrs = []
        for g0 in range(rotate // MULTI_K):
            arr = (NbgBatch * MULTI_K)()
            for q in range(MULTI_K):
                be, pm, ct = outs_[(g0 & 1) * MULTI_K + q]
                arr[q] = NbgBatch(rd["bufs"][g0 * MULTI_K + q].data_ptr(), BATCH, be.data_ptr(), pm.data_ptr(),
                                  ct.data_ptr(), None)
            arrs.append(arr)
        flags = (NBG_SWAP_MACS if variant == "in_place" else 0) | NBG_DEFER_GROUP
        st = sts[0]
        kt = KernelTimer(calls + 1)
        for i in range(calls + 1):
            kt.start(i, st)
            if clib.nbg_maglev_classify_device_multi(hs[0], arrs[i % len(arrs)], MULTI_K, SLOT, FRAME, flags, st):
                raise RuntimeError(f"nbg_maglev_classify_device_multi: {nb._lib.last_error()}")
            kt.stop(i, st)
            finish(hs[0], st)
        sync_all()
        c_ms = kt.ms()[1:]
        kt.close()
        bpp = CLASSIFY_BYTES[variant]
        ach = MULTI_K * BATCH * bpp / (c_ms.mean() / 1e3) / 1e9
        return {"avg_launch_us": round(c_ms.mean() * 1e3, 2), "us_per_batch": round(c_ms.mean() * 1e3 / MULTI_K, 2),
                "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBPS, 4), "bytes_per_pkt": bpp,
                "working_set_mib": rotate * BATCH * SLOT >> 20, "launches": calls}

    def c4_shard_multi(calls, k=8, n=C4_SHARD, n_streams=2):
        """C4's per-GPU shard through the multi-batch launch: a rank batches k consecutive shards of its RX
        queue per nbg_maglev_classify_device_multi call (one streaming-classify launch + one group launch,
        every shard with its own backend / perm / counts), round-robin on n_streams streams over the ring
        inputs' 256 distinct shards; then the launch alone (HIP events, grouping deferred)."""
        from netbricks_amd._lib import NbgBatch

        rd = ring_setup()
        ring_restore(RING_ROTATE)
        ins = [rd["bufs"][w].data_ptr() + q * n * SLOT for w, q in ring_inputs(RING_ROTATE, n)]
        outs_ = [[(torch.empty(n, dtype=torch.uint16, device=dev), torch.empty(n, dtype=torch.uint32, device=dev),
                   torch.empty(N_BACKENDS + 1, dtype=torch.uint32, device=dev)) for _ in range(k)]
                 for _ in range(n_streams)]
        arrs = []
        for g in range(len(ins) // k):
            arr = (NbgBatch * k)()
            for q in range(k):
                be, pm, ct = outs_[g % n_streams][q]
                arr[q] = NbgBatch(ins[g * k + q], n, be.data_ptr(), pm.data_ptr(), ct.data_ptr(), None)
            arrs.append(arr)

        def call(i, st, flags):
            if clib.nbg_maglev_classify_device_multi(hs[i % n_streams], arrs[i % len(arrs)], k, SLOT, FRAME, flags, st):
                raise RuntimeError(f"nbg_maglev_classify_device_multi: {nb._lib.last_error()}")

        for i in range(2 * len(arrs)):
            call(i, sts[i % n_streams], NBG_SWAP_MACS)
        sync_all()
        start_ev = torch.cuda.Event()
        start_ev.record(torch.cuda.current_stream(dev))
        for st in streams[:n_streams]:
            st.wait_event(start_ev)
        t1 = time.perf_counter()
        for i in range(calls):
            call(i, sts[i % n_streams], NBG_SWAP_MACS)
        sync_all()
        el = time.perf_counter() - t1
        kt = KernelTimer(calls)
        for i in range(calls):
            kt.start(i, sts[0])
            call(i * n_streams, sts[0], NBG_SWAP_MACS | NBG_DEFER_GROUP)  # stream 0's handle and outputs
            kt.stop(i, sts[0])
            finish(hs[0], sts[0])
        sync_all()
        c_ms = kt.ms()
        kt.close()
        for m in mgs:
            m.check()
        us = el / (calls * k) * 1e6
        ach = k * n * CLASSIFY_BYTES["in_place"] / (c_ms.mean() / 1e3) / 1e9
        return {"value": round(n / us, 1), "unit": "Mpps", "us_per_shard": round(us, 3), "shards_per_launch": k,
                "streams": n_streams, "path_frac": round(n * PATH_BYTES["in_place"] / us / 1e3 / HBM_PEAK_GBPS, 4),
                "avg_launch_us": round(c_ms.mean() * 1e3, 2), "achieved": round(ach, 1),
                "frac": round(ach / HBM_PEAK_GBPS, 4),
                "what": "C4's per-GPU shard (131,072 packets) with a rank batching 8 consecutive shards of its RX queue "
                        "per multi-batch launch (MAC swap in place + grouping, each shard its own outputs), 2 streams; "
                        "frac from the launch timed alone"}

    def ws_sweep(batches):
        """The working-set sweep: the ring (read only, in place) and the multi-batch launch (in place,
        read only) over 8 / 16 / 32 rotating 1M batches (0.5 / 1 / 2 GiB against the 256 MiB Infinity
        Cache).  Every ring pass's outputs are checked."""
        out = {}
        for rot in WS_SWEEP:
            if rot > RING_ROTATE or rot % MULTI_K:
                continue
            row = {}
            for v in ("read_only", "in_place"):
                try:
                    row[f"ring_{v}"] = ring_pass(v, batches, rotate=rot)
                except Exception as e:  # noqa: BLE001
                    log(f"ring_{v} at {rot} failed: {e}")
                    row[f"ring_{v}"] = {"error": str(e)[:300]}
            for v in ("in_place", "read_only"):
                row[f"{v}_multi{MULTI_K}"] = multi_rot_kernel(v, rot, max(40, 2 * rot // MULTI_K))
            out[str(rot)] = row
        return out

    def c4_block(n_batches, scatter_steps):
        """SURVEY.md section 8(e)'s C4: a 1M batch in `world` contiguous shards, one per rank (see the call
        site).  Returns the line's `c4` block; raises on any check failure."""
        shard_n = BATCH // world
        gburst = C4_GROUP_BURST if shard_n <= 262144 else RING_GROUP_BURST
        gstreams = C4_GROUP_STREAMS if shard_n <= 262144 else RING_GROUP_STREAMS
        blk = {"shards": world, "shard_pkts": shard_n, "batch_pkts": BATCH,
               "path": "per rank: persistent ring (in place) + nbg_ring_group_burst on side streams"}
        if gpu:
            ring_path(2 * BATCHES_PER_STEP, n=shard_n, gstreams=gstreams, gburst=gburst)  # warm
            if world > 1:
                dist.barrier()
            sync_all()
            # ring_path's own wall time: ring start, every shard posted and grouped, ring stop (its input
            # restore for the output check runs before that clock starts)
            el, _, chk, _ = ring_path(n_batches, n=shard_n, gstreams=gstreams, gburst=gburst, check=True)
            if not chk["ok"]:
                raise RuntimeError(f"C4 device-resident output check failed on rank {rank}: {chk}")
        else:  # --selftest: no HIP; the timing fields are not a measurement
            el = 1e-3
        els = gather_floats(el)
        worst = max(els)
        total = world * shard_n * n_batches
        blk["device_resident"] = {
            "value": round(total / worst / 1e6, 1), "unit": "Mpps", "shards_per_rank": n_batches,
            "per_gpu_mpps": [round(shard_n * n_batches / e / 1e6, 1) for e in els],
            "us_per_shard": round(worst / n_batches * 1e6, 3),
            "aggregate_frac": aggregate_frac(total, worst, PATH_BYTES["in_place"], world),
            "group_burst": gburst, "group_streams": gstreams,
            "what": "every rank streams its own resident 1M/N-packet shards through its ring (MAC swap in place + "
                    "grouping), max-over-ranks time, no collective; aggregate_frac at 82 B/pkt over N x 8 TB/s"}
        if world == 1 or scatter_steps <= 0:
            return blk
        # scatter-inclusive: two global batches alternate on rank 0; two shard buffers per rank
        glob = None
        if rank == 0:
            glob = []
            for b in range(2):
                buf, _, _ = nb.make_trace(BATCH, 0, seed=shard_seed(0, 900 + b))
                glob.append(torch.from_numpy(buf).to(dev) if gpu else torch.from_numpy(buf))
        recv = [torch.empty(shard_n * SLOT, dtype=torch.uint8, device=dev) for _ in range(2)]
        be = [torch.empty(shard_n, dtype=torch.uint16, device=dev) for _ in range(2)]
        pm = [torch.empty(shard_n, dtype=torch.uint32, device=dev) for _ in range(2)]
        ct = [torch.zeros(N_BACKENDS + 1, dtype=torch.uint32, device=dev) for _ in range(2)]
        gb = torch.empty(world * shard_n * 2, dtype=torch.uint8, device=dev) if rank == 0 else None
        gc = torch.empty(world * (N_BACKENDS + 1), dtype=torch.int32, device=dev) if rank == 0 else None
        steps_run = 3 + scatter_steps
        if gpu:
            side = torch.cuda.Stream(dev)
            ring = mgs[0].ring(swap_macs=True, stream=streams[0])
            tk = [None, None]
            gev = [None, None]
        t1 = None
        try:
            for step in range(steps_run):
                if step == 3:  # 3 untimed steps, then the timed ones
                    if gpu:
                        side.synchronize()
                    dist.barrier()
                    sync_all()
                    t1 = time.perf_counter()
                x = step & 1
                if gpu:  # the buffers of step - 2: classified and gathered before they are reused
                    if tk[x] is not None:
                        ring.wait(tk[x])
                        gev[x].synchronize()
                scatter_shard(glob[x] if rank == 0 else None, recv[x], rank, world)
                if gpu:
                    torch.cuda.current_stream(dev).synchronize()  # the ring reads the shard
                    tk[x] = ring.post(recv[x], shard_n, be[x])
                    ring.group(tk[x], pm[x], ct[x], stream=side)
                    with torch.cuda.stream(side):
                        gather_results(be[x], ct[x], gb, gc, rank, world)
                    gev[x] = torch.cuda.Event()
                    gev[x].record(side)
                else:  # selftest stand-in for the ring: every packet in group 0
                    be[x].zero_()
                    ct[x].zero_()
                    ct[x][0] = shard_n
                    gather_results(be[x], ct[x], gb, gc, rank, world)
            if gpu:
                side.synchronize()
            el = time.perf_counter() - t1
        finally:
            if gpu:
                ring.stop()
        st_s = max(gather_floats(el))
        ok = True
        if rank == 0:  # the last step's gathered results against the launch path on the whole batch
            if int(gc.sum()) != BATCH:
                raise RuntimeError(f"C4 scatter pass: gathered counts sum {int(gc.sum())} != {BATCH}")
            if gpu:
                launch_ref(glob[(steps_run - 1) & 1].data_ptr(), BATCH)
                if not torch.equal(ring_data["sbe"], gb.view(torch.uint16)):
                    raise RuntimeError("C4 scatter pass: gathered backend[] differs from the launch path")
        blk["scatter_inclusive"] = {
            "value": round(BATCH * scatter_steps / st_s / 1e6, 1), "unit": "Mpps", "steps": scatter_steps,
            "ms_per_batch": round(st_s / scatter_steps * 1e3, 4),
            "root_egress_GBps": round(BATCH * SLOT * (world - 1) / world * scatter_steps / st_s / 1e9, 1),
            "checked": ok,
            "what": "rank 0 scatters one 1M 64-B batch in world contiguous shards (ncclScatter over xGMI), each "
                    "rank's ring classifies + groups its shard, ncclGather returns backend[] + counts to rank 0 "
                    "(two batches in flight); rank 0 checks the last batch against its own launch-path result"}
        return blk

    # ---- configs C3 / C5 (IMIX descriptors): handles, traces and one call per batch
    imix = {}

    def imix_setup():
        if imix:
            return imix
        routes = json.load(open(os.path.join(ROOT, "tests", "golden", "lpm_routes.json")))
        bufs, offs, lens = [], [], []
        for b in range(max(IMIX_BATCHES, S)):
            buf, off, ln = nb.make_trace(BATCH, 1, seed=1000 + b)
            bufs.append(torch.from_numpy(buf).to(dev))
            offs.append(torch.from_numpy(off.view(np.int32)).to(dev).view(torch.uint32))
            lens.append(torch.from_numpy(ln.view(np.int16)).to(dev).view(torch.uint16))
        imix.update(bufs=bufs, offs=offs, lens=lens, pristine=[b.clone() for b in bufs], swaps=[0] * len(bufs),
                    c3=[nb.Maglev([f"be{i}" for i in range(1000)], 655373, device=local) for _ in range(S)],
                    lpm=nb.Lpm(routes["reference"] + routes["mixed"], device=local),
                    gates=[torch.empty(BATCH, dtype=torch.uint16, device=dev) for _ in range(S)],
                    c3out=[dict(backend=torch.empty(BATCH, dtype=torch.uint16, device=dev),
                                perm=torch.empty(BATCH, dtype=torch.uint32, device=dev),
                                counts=torch.empty(1001, dtype=torch.uint32, device=dev)) for _ in range(S)])
        return imix

    def imix_issue(cfg, g, j, stream=None, defer=False, lut_lds=False):
        x = imix
        # stream j's own input: calls in flight on different streams never share a buffer (C3 swaps in
        # place), and calls on one stream run in order
        k = j
        st = sts[j] if stream is None else stream
        if cfg == "c3":
            x["swaps"][k] += 1
            x["c3"][j].group_by(x["bufs"][k], BATCH, offsets=x["offs"][k], lens=x["lens"][k], owned_windows=True,
                                bounds_check=False, defer_group=defer, stream=st, **x["c3out"][j])
        else:
            nb.chain_lpm_maglev(mgs[j], x["lpm"], x["bufs"][k], BATCH, offsets=x["offs"][k], lens=x["lens"][k],
                                owned_windows=True, bounds_check=False, defer_group=defer, gate=x["gates"][j], stream=st, lut_lds=lut_lds,
                                backend=outs[j][0]["backend"], perm=outs[j][0]["perm"], counts=outs[j][0]["counts"])

    def imix_variant(cfg, steps, warmup, lut_lds=False):
        """Config C3 (1000 backends / 655373, IMIX, MAC swap in place) or C5 (lpm -> maglev, IMIX):
        whole-job rate on S streams (step = BATCHES_PER_STEP batches), then the classify kernel alone."""
        imix_setup()
        cm = imix["c3"] if cfg == "c3" else mgs
        for i in range(max(1, warmup) * BATCHES_PER_STEP):
            imix_issue(cfg, i, i % S, lut_lds=lut_lds)
        sync_all()
        start_ev = torch.cuda.Event()
        start_ev.record(torch.cuda.current_stream(dev))
        for st in streams:
            st.wait_event(start_ev)
        n_calls = steps * BATCHES_PER_STEP
        t1 = time.perf_counter()
        for i in range(n_calls):
            imix_issue(cfg, i, i % S, lut_lds=lut_lds)
        sync_all()
        el = time.perf_counter() - t1
        kt = KernelTimer(n_calls)
        st = sts[0]
        for i in range(n_calls):
            kt.start(i, st)
            imix_issue(cfg, i, 0, stream=st, defer=True, lut_lds=lut_lds)
            kt.stop(i, st)
            cm[0].finish_group(st)
        sync_all()
        for m in cm:
            m.check()
        kus = float(kt.ms().mean()) * 1e3
        kt.close()
        cb = (C3_BYTES if cfg == "c3" else C5_BYTES)
        ach = BATCH * cb["classify"] / kus / 1e3
        r = {"value": round(BATCH * n_calls / el / 1e6, 1), "unit": "Mpps",
             "ms_per_batch": round(el / n_calls * 1e3, 5), "streams": S, "avg_launch_us": round(kus, 2),
             "classify_bytes_per_pkt": cb["classify"], "path_bytes_per_pkt": cb["path"], "achieved": round(ach, 1),
             "frac": round(ach / HBM_PEAK_GBPS, 4)}
        if cfg == "c3":
            r["what"] = ("C3: 1000 backends / 655373-slot u16 LUT (L2-gathered), 1M IMIX 7:4:1 frames per batch "
                         "(u32 off + u16 len descriptors, owned 64-B windows), MAC swap in place + grouping "
                         "(hist + scan + group kernels)")
        else:
            r["what"] = ("C5: test/lpm -> test/maglev fused in one classify kernel (DIR-24-8 of the reference's 105 "
                         "routes + 902 mixed, tbl24 32 MiB), 65 backends / 65537, 1M IMIX frames per batch; the two MAC "
                         "swaps cancel (read only); gate + backend + grouping")
        return r

    # ---- C3 / C5 with several RX queues' IMIX batches per launch (nbg_maglev_classify_desc_multi,
    #      nbg_chain_lpm_maglev_multi): MULTI_K distinct 1M IMIX batches per call, each stream its own
    #      MULTI_K inputs (no buffer is in two calls in flight), per-batch outputs
    def imix_multi_setup(k, ms):
        """k distinct 1M IMIX inputs per stream for ms streams (no buffer is in two calls in flight),
        per-batch outputs, one nbg_desc_batch array per (config, k, stream)."""
        x = imix_setup()
        x.setdefault("marr", {})
        x.setdefault("mout", {})
        if ("c3", k, ms - 1) in x["marr"]:
            return x
        from netbricks_amd._lib import NbgDescBatch
        for b in range(len(x["bufs"]), k * ms):
            buf, off, ln = nb.make_trace(BATCH, 1, seed=1000 + b)
            x["bufs"].append(torch.from_numpy(buf).to(dev))
            x["offs"].append(torch.from_numpy(off.view(np.int32)).to(dev).view(torch.uint32))
            x["lens"].append(torch.from_numpy(ln.view(np.int16)).to(dev).view(torch.uint16))
            x["pristine"].append(x["bufs"][-1].clone())
            x["swaps"].append(0)
        for cfg, nbins in (("c3", 1001), ("c5", N_BACKENDS + 1)):
            for j in range(ms):
                arr = (NbgDescBatch * k)()
                x["mout"][(cfg, k, j)] = []
                for q in range(k):
                    i = j * k + q
                    o = [torch.empty(BATCH, dtype=torch.uint16, device=dev), torch.empty(BATCH, dtype=torch.uint32, device=dev),
                         torch.empty(nbins, dtype=torch.uint32, device=dev), torch.empty(BATCH, dtype=torch.uint16, device=dev)]
                    x["mout"][(cfg, k, j)].append(o)
                    arr[q] = NbgDescBatch(x["bufs"][i].data_ptr(), x["offs"][i].data_ptr(), x["lens"][i].data_ptr(), BATCH,
                                          o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                          o[3].data_ptr() if cfg == "c5" else None)
                x["marr"][(cfg, k, j)] = arr
        return x

    def imix_mcall(cfg, k, j, stream, defer=False):
        x = imix
        flags = NBG_OWNED_WINDOWS | (NBG_DEFER_GROUP if defer else 0)
        if cfg == "c3":
            for q in range(k):  # every batch of the call has its MACs swapped in place once more
                x["swaps"][j * k + q] += 1
            rc = clib.nbg_maglev_classify_desc_multi(x["c3"][j]._h, x["marr"][("c3", k, j)], k, flags | NBG_SWAP_MACS,
                                                     stream)
        else:
            rc = clib.nbg_chain_lpm_maglev_multi(mgs[j]._h, x["lpm"]._h, 3, x["marr"][("c5", k, j)], k, flags, stream)
        if rc:
            from netbricks_amd._lib import last_error
            raise RuntimeError(f"{cfg} multi call: {rc} {last_error()}")

    def mac_swapped(buf, off):
        """buf with the MACs of every frame (bytes [off, off + 12)) swapped: what an odd number of
        in-place classify calls leaves (the IMIX frames are all >= 14 B)."""
        o = off.to(torch.int64).unsqueeze(1)
        ar = torch.arange(12, device=dev, dtype=torch.int64)
        dst = (o + ar).reshape(-1)
        src = (o + torch.cat([ar[6:], ar[:6]])).reshape(-1)
        out = buf.clone()
        out[dst] = buf[src]
        return out

    def imix_output_check(cfg, k, ms):
        """After an IMIX multi pass: every batch's outputs of its stream's last multi call (backend, perm,
        counts, and the chain's gate) against the single-batch HIP path (nbg_maglev_classify_device_ex /
        nbg_chain_lpm_maglev_device, read only) on the same input, and every input's bytes against its
        pristine copy (C3: MACs swapped iff the pass and earlier ones swapped it an odd number of times;
        C5: untouched)."""
        x = imix
        sync_all()
        bad = []
        for j in range(ms):
            for q, o in enumerate(x["mout"][(cfg, k, j)]):
                i = j * k + q
                if cfg == "c3":
                    r = x["c3"][j].group_by(x["bufs"][i], BATCH, offsets=x["offs"][i], lens=x["lens"][i],
                                            owned_windows=True, swap_macs=False, bounds_check=False, stream=sts[j])
                    ref = (r.backend, r.perm, r.counts)
                else:
                    r = nb.chain_lpm_maglev(mgs[j], x["lpm"], x["bufs"][i], BATCH, offsets=x["offs"][i],
                                            lens=x["lens"][i], owned_windows=True, bounds_check=False, stream=sts[j])
                    ref = (r.backend, r.perm, r.counts, r.gate)
                # the inputs are shared by the C3 and C5 passes: C3's calls swapped them in place
                exp = mac_swapped(x["pristine"][i], x["offs"][i]) if x["swaps"][i] % 2 else x["pristine"][i]
                sync_all()
                if not all(torch.equal(a[:b.numel()], b) for a, b in zip(o, ref)):
                    bad.append((i, "outputs"))
                elif not torch.equal(x["bufs"][i], exp):
                    bad.append((i, "bytes"))
        return {"ok": not bad, "batches": k * ms, "bad_batches": bad[:8]}

    def imix_multi_variant(cfg, steps, warmup, k=IMIX_MULTI_K, ms=IMIX_MULTI_STREAMS):
        """C3 / C5 with k IMIX batches of 1M per call on ms streams (whole-job rate), then the
        multi-batch classify launch alone (events, grouping deferred)."""
        ms = min(ms, S)
        x = imix_multi_setup(k, ms)
        cm = x["c3"] if cfg == "c3" else mgs
        calls = max(steps * BATCHES_PER_STEP // k, 10)
        for i in range(max(warmup, 2) * ms):
            imix_mcall(cfg, k, i % ms, sts[i % ms])
        sync_all()
        start_ev = torch.cuda.Event()
        start_ev.record(torch.cuda.current_stream(dev))
        for st in streams[:ms]:
            st.wait_event(start_ev)
        t1 = time.perf_counter()
        for i in range(calls):
            imix_mcall(cfg, k, i % ms, sts[i % ms])
        sync_all()
        el = time.perf_counter() - t1
        st = sts[0]
        kt = KernelTimer(calls)
        for i in range(calls):
            kt.start(i, st)
            imix_mcall(cfg, k, 0, st, defer=True)
            kt.stop(i, st)
            cm[0].finish_group(st)
        sync_all()
        for m in cm[:ms]:
            m.check()
        kus = float(kt.ms().mean()) * 1e3
        kt.close()
        check = imix_output_check(cfg, k, ms)
        cb = C3_BYTES if cfg == "c3" else C5_BYTES
        ach = k * BATCH * cb["classify"] / kus / 1e3
        return {"output_check": check, "value": round(k * BATCH * calls / el / 1e6, 1), "unit": "Mpps",
                "ms_per_batch": round(el / (calls * k) * 1e3, 5), "batches_per_launch": k, "streams": ms,
                "avg_launch_us": round(kus, 2), "classify_us_per_batch": round(kus / k, 2),
                "classify_bytes_per_pkt": cb["classify"], "path_bytes_per_pkt": cb["path"],
                "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBPS, 4),
                "what": (f"{cfg.upper()} with {k} RX queues' 1M IMIX batches per launch "
                         f"({'nbg_maglev_classify_desc_multi' if cfg == 'c3' else 'nbg_chain_lpm_maglev_multi'}: one "
                         "classify launch, then one hist / scan / group launch over all batches, per-batch outputs), "
                         f"{ms} streams with distinct inputs; classify_us_per_batch from the multi launch timed alone")}

    def dump_outputs(path, headline, steps):
        """--dump-outputs: what the headline's last timed step left on the device, as a caller of that
        path receives it, one set of .npy files per batch b of the step: b<b>_counts (all N_BACKENDS + 1
        group sizes), b<b>_backend and b<b>_perm (the entries at DUMP_SAMPLE fixed, seeded packet
        indices) and b<b>_macs (the first 12 bytes, rewritten in place, of DUMP_PKTS fixed, seeded
        packets), float32 (perm float64); 38 MB in all.  The inputs are seeded and the same arguments swap
        every batch the same number of times, so two builds run alike write comparable files."""
        if headline == "multi":
            sets = {b: m_outs[b] for b in range(N_BATCHES)}
        elif headline == "launch":  # 2 x S output sets: a set's last writer within the step owns it
            owner = {}
            for q in range(BATCHES_PER_STEP):
                g = (steps - 1) * BATCHES_PER_STEP + q
                owner[(g % S, (g // S) & 1)] = g % N_BATCHES
            sets = {b: tuple(outs[j][par][k] for k in ("backend", "perm", "counts")) for (j, par), b in owner.items()}
        else:
            raise SystemExit(f"bench: --dump-outputs does not cover the headline path {headline!r}")
        os.makedirs(path, exist_ok=True)
        rs = np.random.RandomState(DUMP_SEED)
        idx = torch.from_numpy(np.sort(rs.choice(BATCH, DUMP_SAMPLE, replace=False))).to(dev)
        pidx = torch.from_numpy(np.sort(rs.choice(BATCH, DUMP_PKTS, replace=False))).to(dev)
        total = 0
        for b, (be, pm, ct) in sorted(sets.items()):
            arrs = {"backend": be.view(torch.int16)[idx].cpu().numpy().view(np.uint16).astype(np.float32),
                    "perm": pm.view(torch.int32)[idx].cpu().numpy().view(np.uint32).astype(np.float64),
                    "counts": ct.view(torch.int32).cpu().numpy().view(np.uint32).astype(np.float32),
                    "macs": dbufs[b].view(BATCH, SLOT)[pidx, :12].cpu().numpy().astype(np.float32)}
            for name, a in arrs.items():
                np.save(os.path.join(path, f"b{b}_{name}.npy"), a)
                total += a.nbytes
        log(f"[rank {rank}] --dump-outputs: {4 * len(sets)} arrays, {total / 1e6:.1f} MB in {path}")

    if args.pmc_child:  # under rocprofv3 --pmc: each variant's launches in a fixed order, one stream
        st = sts[0]
        for v in PMC_ORDER:
            for i in range(PMC_WARMUP + PMC_STEPS):
                if v in ("in_place", "records", "read_only"):
                    issue(0, i % N_BATCHES, i & 1, v, False, stream=st)
                elif v == "in_place_lag":
                    issue(0, i % N_BATCHES, i & 1, "in_place", True, stream=st)
                elif v == "c4_shard":
                    issue(0, 0, i & 1, "in_place", False, stream=st, n=C4_SHARD,
                          pkts=pk[(i // 8) % N_BATCHES] + (i % 8) * C4_SHARD * SLOT)
                else:
                    if not imix:
                        sync_all()
                        imix_setup()
                    imix_issue(v, i, 0, stream=st)
            finish(hs[0], st)
            sync_all()
            mgs[0].check()
        if m_arrs:  # then the multi-batch launches (one classify dispatch per MULTI_K batches)
            for v in PMC_MULTI:
                for i in range(PMC_WARMUP + PMC_STEPS):
                    mcall(i, v, st)
                sync_all()
                mgs[0].check()
        # then the ring runs exactly as variants.ring_read_only / ring_in_place are timed (RING_BATCHES
        # batches over RING_ROTATE inputs, one dispatch each): the ring alone (the profiler may
        # serialise dispatches, so no grouping launches beside it)
        if not args.no_ring:
            for v in ("read_only", "in_place"):
                ring_pass(v, PMC_RING_BATCHES)
        # then C3 and C5 with IMIX_MULTI_K batches per launch (classify_desc_multi_kernel dispatches)
        if not args.no_imix:
            imix_multi_setup(IMIX_MULTI_K, 1)
            for cfg in PMC_DESC_MULTI:
                for i in range(PMC_WARMUP + PMC_STEPS):
                    imix_mcall(cfg, IMIX_MULTI_K, 0, st, defer=True)
                    (imix["c3"][0] if cfg == "c3" else mgs[0]).finish_group(st)
                sync_all()
        return

    if args.multi_only:  # profiling run: only the multi-batch passes
        print(json.dumps({f"{v}_multi{MULTI_K}": multi_pass(v, max(args.steps * BATCHES_PER_STEP // MULTI_K, 10), 3)
                          for v in ("read_only", "in_place")}), flush=True)
        return

    # ---- timed region: K steps, bracketed by barrier + synchronize, max over ranks.  The headline
    #      path (--headline): MULTI_K RX queues' 1M batches per launch (default), one launch per batch
    #      on S streams, or the persistent ring with per-batch grouping (measured slower for runs of a
    #      few hundred batches: the ring's per-batch time drifts down over ~1,000 batches, DESIGN.md
    #      section 4).
    warm = args.warmup  # exactly the steps the line reports (the contract's W)
    headline = args.headline if gpu else "launch"
    if headline == "multi" and not m_arrs:
        headline = "launch"
    ring_kms = None
    if headline == "multi":
        elapsed_rank = timed_multi(args.steps, warm, barrier=True)
    elif headline == "ring":
        try:
            elapsed_rank, ring_kms = timed_ring(args.steps, warm, barrier=True)
        except Exception as e:  # noqa: BLE001
            if world > 1:
                raise  # ranks must agree on the path: fail the job
            log(f"ring headline failed; the launch path is the headline: {e}")
            headline = f"launch (the ring failed: {str(e)[:200]})"
    if headline not in ("ring", "multi"):
        elapsed_rank = timed("in_place", args.steps, warm, lag=False, barrier=True)
    per_rank_s = gather_floats(elapsed_rank)
    elapsed = max(per_rank_s)
    kms_max = max(gather_floats(ring_kms if ring_kms is not None else 0.0))
    if args.dump_outputs and rank == 0:  # before any later pass runs over the same batches
        if not gpu:
            raise SystemExit("bench: --dump-outputs needs the GPU path (no outputs under --selftest)")
        dump_outputs(args.dump_outputs, headline, args.steps)
    # the same measurement at >= 50 steps (400 batches), in the same line: the K-step value is the
    # steady-state rate when the two agree
    steady = None
    if gpu and args.steady_steps > 0:
        if headline == "ring":
            st_el = max(gather_floats(timed_ring(args.steady_steps, 1, barrier=True)[0]))
        elif headline == "multi":
            st_el = max(gather_floats(timed_multi(args.steady_steps, 1, barrier=True)))
        else:
            st_el = max(gather_floats(timed("in_place", args.steady_steps, 1, lag=False, barrier=True)))
        steady = {"steps": args.steady_steps,
                  "value": round(BATCH * BATCHES_PER_STEP * args.steady_steps * world / st_el / 1e6, 1),
                  "ms_per_step": round(st_el / args.steady_steps * 1e3, 5)}

    # ---- config C4 as SURVEY.md section 8(e) defines it: ONE 1M batch split into `world` contiguous
    #      shards (131,072 packets at 8 GPUs), one per rank, each classified + grouped through the
    #      rank's persistent ring.  Device-resident: every rank streams its own resident shards (no
    #      collective in the timed region).  Scatter-inclusive (N > 1): rank 0 holds the 1M batch,
    #      ncclScatter hands each rank its shard, the rank's ring classifies + groups it, ncclGather
    #      returns backend[] + counts to rank 0, which checks them against its own launch-path
    #      classification of the batch.  Any failure fails the job.
    c4 = None
    if not args.no_c4:
        log(f"[rank {rank}] C4 block")
        c4 = c4_block(args.c4_batches, args.scatter_steps)
        log(f"[rank {rank}] C4 block done")

    # ---- roofline: the headline launch timed alone; labelled variants beside (N = 1)
    roof, mroof, variants = None, None, {}
    if gpu and args.full:
        launches = args.steps * BATCHES_PER_STEP
        roof = kernel_pass("in_place", launches, lag=False)
        mroof = multi_kernel("in_place", max(launches // MULTI_K, 10)) if headline == "multi" else None
        if world == 1 and not args.no_variants and headline in ("ring", "multi"):
            el = timed("in_place", args.steps, warm, lag=False, barrier=True)
            variants["launch_in_place"] = {
                "value": round(BATCH * BATCHES_PER_STEP * args.steps / el / 1e6, 1), "unit": "Mpps",
                "ms_per_batch": round(el / (args.steps * BATCHES_PER_STEP) * 1e3, 5), "streams": S, **roof,
                "what": "the same path (C2 in place + grouping) with one streaming-classify launch + one group "
                        "launch per 1M batch, round-robin on S streams (the round-1/2 headline); frac from the "
                        "classify launch timed alone on one stream (HIP events)"}
        if world == 1 and not args.no_variants:
            el = timed("in_place", args.steps, args.warmup, lag=True)
            variants["in_place_lag"] = {
                "value": round(BATCH * BATCHES_PER_STEP * args.steps / el / 1e6, 1), "unit": "Mpps",
                "ms_per_batch": round(el / (args.steps * BATCHES_PER_STEP) * 1e3, 5),
                **kernel_pass("in_place", launches, lag=True),
                "what": "NBG_GROUP_LAG: batch i grouped inside batch i+1's streaming classify launch (one launch per "
                        "batch); slower here: the CU is VALU-busy classifying, so the grouping cannot hide under the "
                        "launch's HBM time (DESIGN.md section 4)"}
            for v in ("records", "read_only"):
                el = timed(v, args.steps, args.warmup, lag=False)
                variants[v] = {"value": round(BATCH * BATCHES_PER_STEP * args.steps / el / 1e6, 1), "unit": "Mpps",
                               "ms_per_batch": round(el / (args.steps * BATCHES_PER_STEP) * 1e3, 5),
                               "classify_bytes_per_pkt": CLASSIFY_BYTES[v], "path_bytes_per_pkt": PATH_BYTES[v],
                               **kernel_pass(v, launches, lag=False)}
            variants["records"]["what"] = ("MAC swap written as dense 12-B egress records (packet bytes untouched) "
                                           "+ grouping, same streams")
            variants["read_only"]["what"] = ("north_star's parse + hash + lookup: no MAC rewrite, backend[] + grouping, "
                                             "same streams")
            # config C4's per-GPU workload: 131,072-packet shards of the 8 batches (64 distinct)
            el = timed("in_place", args.steps, args.warmup, lag=False, n=C4_SHARD, shard=True)
            variants["c4_shard"] = {
                "value": round(C4_SHARD * BATCHES_PER_STEP * args.steps / el / 1e6, 1), "unit": "Mpps",
                "ms_per_batch": round(el / (args.steps * BATCHES_PER_STEP) * 1e3, 5),
                **kernel_pass("in_place", launches, lag=False, n=C4_SHARD, shard=True),
                "what": "C4's per-GPU shard: one 1M C2 batch in 8 contiguous 131,072-packet shards, each "
                        "classified + grouped as one rank would (MAC swap in place), 64 distinct shards rotating "
                        "on the same streams; below the streaming kernel's 262,144-packet threshold, so the "
                        "tile-per-wave classify kernel + group kernel (pmc.c4_shard.kernel)"}
            log(f"[rank {rank}] launch-path variants done")
            if not args.no_ring:
                # the working-set sweep (0.5 / 1 / 2 GiB of rotating 1M batches): the ring read only and
                # in place, RING_BATCHES batches per pass, slope over the middle three quarters, outputs
                # checked after every pass; the multi-batch launch beside.  variants.ring_read_only /
                # ring_in_place are the sweep's RING_ROTATE row (2 GiB).
                kr = max(args.steps * BATCHES_PER_STEP, RING_BATCHES)
                try:
                    sweep = ws_sweep(kr)
                except Exception as e:  # noqa: BLE001
                    log(f"working-set sweep failed: {e}")
                    sweep = {"error": str(e)[:300]}
                variants["ws_sweep"] = sweep
                log(f"[rank {rank}] working-set sweep done")
                top = sweep.get(str(RING_ROTATE), {}) if isinstance(sweep, dict) else {}
                for name in ("ring_read_only", "ring_in_place"):
                    variants[name] = top.get(name, {"error": "not measured"})
                kb = max(args.steps * BATCHES_PER_STEP, 1024)
                ring_runs = [  # C4's per-GPU shard on the ring: 131,072-packet batches, no launch per shard
                    ("c4_shard_ring", lambda: ring_pass("in_place", RING_BATCHES, n=C4_SHARD)),
                    ("c4_shard_ring_grouped", lambda: ring_grouped(RING_BATCHES, n=C4_SHARD,
                                                                    gstreams=C4_GROUP_STREAMS,
                                                                    gburst=C4_GROUP_BURST))]
                if headline != "ring":
                    ring_runs.append(("ring_in_place_grouped", lambda: ring_grouped(kb)))
                ring_runs.append(("c4_shard_multi8", lambda: c4_shard_multi(max(args.steps * BATCHES_PER_STEP, 256))))
                for name, fn in ring_runs:
                    try:  # a ring variant that fails is reported in the line, beside the other figures
                        variants[name] = fn()
                    except Exception as e:  # noqa: BLE001
                        log(f"{name} failed: {e}")
                        variants[name] = {"error": str(e)[:300]}
                if "us_per_batch" in variants["c4_shard_ring"]:
                    variants["c4_shard_ring"]["what"] = (
                        "C4's per-GPU shard (131,072 packets: one 1M C2 batch in 8 contiguous shards) through the "
                        "persistent ring, MAC swap in place: no launch, LUT staging or ramp per shard; backend[] + "
                        "swap only")
                if os.environ.get("NBG_BENCH_RING_GROUP_SWEEP"):  # tuning: burst size x side streams
                    gs = {}
                    for n_, name_ in ((BATCH, "1M"), (C4_SHARD, "c4_shard")):
                        for gb_ in ((1, 2, 4) if n_ == BATCH else (4, 8)):
                            for st_ in (2, 3, 4):
                                try:
                                    r_ = ring_grouped(1024 if n_ == BATCH else 4096, n=n_, gstreams=st_, gburst=gb_)
                                    gs[f"{name_}_b{gb_}_s{st_}"] = {k_: r_[k_] for k_ in ("us_per_batch", "path_frac")}
                                except Exception as e:  # noqa: BLE001
                                    gs[f"{name_}_b{gb_}_s{st_}"] = {"error": str(e)[:200]}
                    variants["ring_group_sweep"] = gs
                checks = [v.get("output_check") for k, v in variants.items()
                          if isinstance(v, dict) and isinstance(v.get("output_check"), dict)]
                checks += [r.get("output_check") for row in (sweep.values() if isinstance(sweep, dict) else [])
                           if isinstance(row, dict) for r in row.values()
                           if isinstance(r, dict) and isinstance(r.get("output_check"), dict)]
                variants["ring_output_checks"] = {"passes": len(checks), "ok": all(c["ok"] for c in checks)}

            if m_arrs:
                calls = max(args.steps * BATCHES_PER_STEP // MULTI_K, 10)
                for v in ("read_only", "in_place"):
                    variants[f"{v}_multi{MULTI_K}"] = multi_pass(v, calls, max(args.warmup, 3))
            if not args.no_imix:
                t0 = time.time()
                imix_setup()
                log(f"[rank {rank}] IMIX traces ready in {time.time() - t0:.1f}s")
                variants["c3"] = imix_variant("c3", args.steps, args.warmup)
                variants["c5"] = imix_variant("c5", args.steps, args.warmup)
                variants["c5_lut_lds"] = imix_variant("c5", args.steps, args.warmup, lut_lds=True)
                variants["c5_lut_lds"]["what"] = (
                    "C5 with the u8 LUT staged in LDS (NBG_LUT_LDS: one 1024-thread block per CU, two tiles' loads "
                    "in flight per wave): removes the LUT's L2 gather from every wave's critical path")
                variants[f"c3_multi{IMIX_MULTI_K}"] = imix_multi_variant("c3", args.steps, args.warmup)
                variants[f"c5_multi{IMIX_MULTI_K}"] = imix_multi_variant("c5", args.steps, args.warmup)
                # C3 and C5 at the API's maximum of 16 batches per launch (the ramp paid once per 16M
                # packets; profiles/r05_sweep_multi_burst.txt: C3's path 1-1.5 us per batch faster, C5's slower)
                if IMIX_MULTI_K != 16:
                    variants["c3_multi16"] = imix_multi_variant("c3", args.steps, args.warmup, k=16)
                    variants["c5_multi16"] = imix_multi_variant("c5", args.steps, args.warmup, k=16)
                ichecks = [v["output_check"] for name_, v in variants.items()
                           if name_.startswith(("c3_multi", "c5_multi")) and isinstance(v, dict) and "output_check" in v]
                variants["imix_output_checks"] = {"passes": len(ichecks), "ok": all(c["ok"] for c in ichecks),
                                                  "batches": sum(c["batches"] for c in ichecks)}
                sweep_spec = os.environ.get("NBG_BENCH_IMIX_SWEEP", "")  # measurement: "KxS,..."
                if sweep_spec:
                    isw = {}
                    for spec in sweep_spec.split(","):
                        k, m = (int(v) for v in spec.split("x"))
                        for cfg in ("c3", "c5"):
                            r = imix_multi_variant(cfg, args.steps, args.warmup, k=k, ms=m)
                            isw[f"{cfg}_{spec}"] = {q: r[q] for q in ("ms_per_batch", "classify_us_per_batch", "value")}
                    variants["imix_multi_sweep"] = isw

    if rank == 0:
        cpu = None
        if gpu and world == 1 and not args.no_cpu_baseline:
            try:
                cpu = cpu_baseline(host_bufs, lut)
            except Exception as e:  # the baseline is informational; never fail the bench on it
                log(f"cpu baseline failed: {e}")
        total_pkts = BATCH * BATCHES_PER_STEP * args.steps * world
        line = {
            "metric": "Mpps + HBM GB/s device-resident Maglev (64B pkts)",
            "value": round(total_pkts / elapsed / 1e6, 1),
            "unit": "Mpps",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 5),
            "ms_per_batch": round(elapsed / (args.steps * BATCHES_PER_STEP) * 1e3, 5),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "config": {"workload": "C2: Maglev 65 backends / 65537-slot LUT, 64B synthetic UDP, "
                                   "1M-packet device-resident batch per GPU",
                       "backends": N_BACKENDS, "table_size": TABLE, "batch_pkts": BATCH, "slot_bytes": SLOT,
                       "frame_bytes": FRAME, "rotating_batches": N_BATCHES, "batches_per_step": BATCHES_PER_STEP,
                       "mac_swap": "in place",
                       "group_by": ("perm + counts: nbg_ring_group (hist + group launches) per completed batch on "
                                    f"{RING_GROUP_STREAMS} side streams" if headline == "ring"
                                    else f"perm + counts (one group launch per {MULTI_K} batches, per-batch outputs)"
                                    if headline == "multi" else "perm + counts (group launch per batch)"),
                       "path": ("persistent RX ring (nbg_ring_*): one resident classify kernel per GPU fed RX bursts"
                                if headline == "ring" else
                                f"{MULTI_K} RX queues' 1M batches per launch (nbg_maglev_classify_device_multi) on "
                                f"{min(MULTI_STREAMS, S)} streams" if headline == "multi" else
                                f"one launch per 1M batch on {S} streams" if headline == "launch" else headline),
                       "batches_per_launch": MULTI_K if headline == "multi" else 1,
                       "streams": min(MULTI_STREAMS, S) if headline == "multi" else S,
                       "parallelism": f"shard{world}"},
            "per_gpu_mpps": [round(BATCH * BATCHES_PER_STEP * args.steps / s / 1e6, 1) for s in per_rank_s],
            "lut_digest": digest,
            "lut_digest_per_rank": digests,
            "hbm_gbps_per_gpu": round(total_pkts / world * PATH_BYTES["in_place"] / elapsed / 1e9, 1),
            "hbm_bytes_per_pkt": PATH_BYTES["in_place"],
            "aggregate_frac": aggregate_frac(total_pkts, elapsed, PATH_BYTES["in_place"], world),
        }
        if steady is not None:
            steady["ratio"] = round(line["value"] / steady["value"], 4)
            line["steady_state"] = steady
        if headline == "ring" and kms_max > 0:
            nbt = args.steps * BATCHES_PER_STEP
            bpp = CLASSIFY_BYTES["in_place"]
            ach = nbt * BATCH * bpp / (kms_max * 1e-3) / 1e9
            line["roofline"] = {
                "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": round(ach / HBM_PEAK_GBPS, 4), "traffic": None,
                "kernel": "classify_ring_kernel<true, 1> (persistent RX ring: LUT staged in LDS once, LDS-DMA tile "
                          "ring across batches, relay block for the descriptors)",
                "bytes_per_pkt": bpp, "pkts_per_launch": nbt * BATCH, "batches_per_launch": nbt,
                "avg_launch_us": round(kms_max * 1e3, 2), "us_per_batch": round(kms_max * 1e3 / nbt, 3),
                "timing": "HIP events on the ring kernel's stream around its one launch in the timed region "
                          "(nbg_ring_kernel_ms, max over ranks): that launch classifies all steps x 8 batches, its "
                          "ramp and drain included",
                "note": "in place, every 64-B slot is written back whole (HBM writes whole bursts): physical traffic "
                        "~1.7x the 78 algorithmic bytes (DESIGN.md section 5); variants.launch_in_place is the "
                        "launch-per-batch path and its classify kernel's roofline"}
        elif headline == "multi" and mroof is not None:
            line["roofline"] = {
                "bound": "hbm", "achieved": mroof["achieved"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": mroof["frac"], "traffic": None,
                "kernel": f"classify_stream_kernel<F4,HIST,in place> over {MULTI_K} batches per launch (LDS LUT, "
                          "LDS-DMA tile ring, per-batch partition rows)",
                "bytes_per_pkt": mroof["bytes_per_pkt"], "pkts_per_launch": mroof["pkts_per_launch"],
                "batches_per_launch": MULTI_K, "avg_launch_us": mroof["avg_launch_us"],
                "us_per_batch": round(mroof["avg_launch_us"] / MULTI_K, 3),
                "timing": "single-stream pass, HIP events around each multi-batch classify launch (grouping "
                          "deferred); `value` is the multi-stream rate, where the grouping of one launch's batches "
                          "overlaps the next launch's classify",
                "note": "in place, every 64-B slot is written back whole (HBM writes whole bursts): physical traffic "
                        "~1.7x the 78 algorithmic bytes (DESIGN.md section 5); variants.launch_in_place is one launch "
                        "per 1M batch"}
        elif roof is not None:
            line["roofline"] = {"bound": "hbm", "achieved": roof["achieved"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                "frac": roof["frac"], "traffic": None,
                                "kernel": "classify_stream_kernel<F4,HIST,in place> (LDS LUT, LDS-DMA tile ring)",
                                "bytes_per_pkt": roof["bytes_per_pkt"], "pkts_per_launch": BATCH,
                                "avg_launch_us": roof["avg_launch_us"],
                                "group_kernel_avg_us": roof["group_kernel_avg_us"],
                                "timing": "single-stream pass, HIP events around each classify launch (grouping "
                                          "deferred); `value` is the multi-stream rate, where the grouping of one "
                                          "batch overlaps the classify of the next",
                                "note": "in place, every 64-B slot is written back whole (HBM writes whole bursts), "
                                        "so the physical traffic is ~1.7x the 78 algorithmic bytes and this variant's "
                                        "frac is capped near 0.46 by the measured read+rewrite ceiling with nt loads "
                                        "(DESIGN.md section 5); variants.read_only / read_only_multi4 are north_star's "
                                        "parse + hash + lookup"}
        if variants:
            line["variants"] = variants
            ro = variants.get(f"read_only_multi{MULTI_K}")
            if isinstance(ro, dict) and "frac" in ro:  # BASELINE.json north_star: parse + hash + lookup >= 70 %
                rr_ = variants.get("ring_read_only", {})
                line["north_star"] = {"target_frac": 0.70, "frac": float(ro["frac"]), "met": bool(ro["frac"] >= 0.70),
                                      "variant": f"read_only_multi{MULTI_K}",
                                      "single_batch_frac": variants.get("read_only", {}).get("frac"),
                                      "ring_slope_frac": rr_.get("frac"),
                                      "ring_working_set_mib": rr_.get("working_set_mib")}
        line["cpu_baseline"] = cpu
        if c4 is not None:
            line["c4"] = c4
        if comm is not None:
            line.update(comm)
        if args.selftest:
            line["selftest"] = True
            line["data"] = "synthetic (launcher selftest on CPU: no HIP call, steps are empty)"
        if os.environ.get("NBG_BENCH_LAUNCHED") == "1":
            print(json.dumps(line), flush=True)  # the launcher adds PMC / e2e and prints the compact line
        else:
            emit_line(line, record=args.full)  # a rank of torch.distributed.run: rank 0 prints the line itself
    if gpu:
        for m in mgs:
            m.close()
        for m in imix.get("c3", []):
            m.close()
        if imix:
            imix["lpm"].close()
    if world > 1:
        dist.destroy_process_group()


def parse_args(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50, help="timed steps (one step = one rotation over the 8 batches)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--steady-steps", type=int, default=50,
                    help="also time this many steps (same line, `steady_state`); 0 = skip")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-variants", action="store_true", help="skip the variant passes")
    ap.add_argument("--no-multi", action="store_true", help="skip the multi-batch variants")
    ap.add_argument("--no-imix", action="store_true", help="skip configs C3 / C5")
    ap.add_argument("--no-ring", action="store_true", help="skip the persistent-ring variants")
    ap.add_argument("--headline", choices=("multi", "launch", "ring"), default="multi",
                    help="headline path: multi = MULTI_K RX queues' 1M batches per launch on MULTI_STREAMS streams "
                         "(default); launch = one launch per 1M batch on --streams streams; ring = the persistent "
                         "ring with per-batch grouping")
    ap.add_argument("--multi-only", action="store_true",
                    help="profiling: only the multi-batch passes (rocprof kernel stats of the multi launch)")
    ap.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 --pmc traffic passes")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end (PCIe) pass")
    ap.add_argument("--inline", action="store_true",
                    help="run as a single rank in this process (no launcher; for running under a profiler)")
    ap.add_argument("--selftest", action="store_true",
                    help="launcher + rank logic on the CPU with gloo, no HIP call (tests)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--scatter-steps", type=int, default=50,
                    help="N>1: steps of C4's scatter-inclusive pass (RCCL scatter of one 1M batch from rank 0, "
                         "ring classify + group, RCCL gather); 0 = skip")
    ap.add_argument("--c4-batches", type=int, default=RING_BATCHES,
                    help="shards per rank in C4's device-resident pass (through the rank's ring)")
    ap.add_argument("--no-c4", action="store_true", help="skip the C4 block")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the steady-state pass, the roofline passes, every variant, the C4 "
                         "block, the CPU baseline, the PMC traffic passes, the end-to-end pass and the full record "
                         "file (each still switched off by its own --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the headline path's last timed step computed to "
                         "DIR/<name>.npy (rank 0; see dump_outputs)")
    args = ap.parse_args(argv)
    if not args.full:  # a plain run: set up, warm up, time the K steps, print the line
        args.steady_steps = 0
        args.no_cpu_baseline = args.no_variants = args.no_c4 = args.no_pmc = args.no_e2e = True
    return args


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    if "WORLD_SIZE" in os.environ or args.inline or args.pmc_child:
        run_rank(args)
        return 0
    return launch(args, argv)


if __name__ == "__main__":
    sys.exit(main())
