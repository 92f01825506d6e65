"""The Python wrapper refuses output buffers the library would overrun (it writes them through raw
pointers): wrong dtype, too small, non-contiguous.  Checked before any library call, so no GPU."""
import ctypes as C

import numpy as np
import pytest

from netbricks_amd import Maglev


def _bare():
    m = Maglev.__new__(Maglev)  # no device handle: validation must fire before the library call
    m._h = C.c_void_p()
    m.n_backends = 65
    m.device = 0
    return m


@pytest.mark.parametrize("bad", [
    dict(backend=np.empty(10, np.uint32)),
    dict(backend=np.empty(9, np.uint16)),
    dict(backend=np.empty(20, np.uint16)[::2]),
    dict(perm=np.empty(10, np.int64)),
    dict(perm=np.empty(5, np.uint32)),
    dict(counts=np.empty(65, np.uint32)),
    dict(backend=[0] * 10),
])
def test_host_submit_rejects_bad_outputs(bad):
    m = _bare()
    args = dict(backend=np.empty(10, np.uint16), perm=np.empty(10, np.uint32), counts=np.empty(66, np.uint32))
    args.update(bad)
    with pytest.raises(ValueError):
        m.host_submit(np.zeros(10, np.uint64), np.zeros(10, np.uint16), **args)


def test_host_submit_rejects_length_mismatch():
    with pytest.raises(ValueError):
        _bare().host_submit(np.zeros(10, np.uint64), np.zeros(9, np.uint16), np.empty(10, np.uint16))


def test_compact_group_block_fits_beside_ring():
    """The grouping beside a running in-place ring takes the compact group kernel when the default
    block would not fit in the LDS the ring leaves (maglev_kernels.hip group_compact): the compact
    block must fit there for every bin count the group kernels take (<= 1024 bins; above 1023
    backends group_wide_kernel runs), and the default block must fit for C2's 66 bins."""
    from netbricks_amd._lib import lib

    budget = lib.nbg_debug_lds_beside_ring()
    assert 24 * 1024 <= budget < 40 * 1024
    for nbins in (2, 66, 129, 257, 1001, 1024):
        assert lib.nbg_debug_group_lds(nbins, 1) <= budget, nbins
    assert lib.nbg_debug_group_lds(66, 0) <= budget
    assert lib.nbg_debug_group_lds(1001, 0) > budget  # C3 beside a ring: the compact kernel
    assert lib.nbg_debug_set_group_compact(2) != 0
    assert lib.nbg_debug_set_group_compact(-1) == 0


_DIRECT, _KERNEL = 2, 0  # GroupScan (nbgpu_internal.h)

# nb, rows' source (0 a handle's call, 1 the ring), n_pkts per batch ->
# part_pkts, per, scan, hist_kernel, hist16, wide, n_parts per batch
_GROUP_PLANS = [
    (65, 0, [1048576], (4096, 256, _DIRECT, 0, 1, 0), [256]),
    (65, 0, [1048577], (8192, 129, _DIRECT, 0, 1, 0), [129]),
    (65, 0, [15728640], (61440, 256, _DIRECT, 0, 1, 0), [256]),
    (65, 0, [16777216], (65536, 256, _DIRECT, 0, 0, 0), [256]),
    (1000, 0, [131072], (4096, 32, _DIRECT, 1, 0, 0), [32]),
    (1000, 0, [135168], (4096, 33, _KERNEL, 1, 0, 0), [33]),
    (1000, 0, [1048576], (4096, 256, _KERNEL, 1, 0, 0), [256]),
    (1500, 0, [140000], (4096, 35, _KERNEL, 1, 0, 1), [35]),
    (65, 0, [262161, 0, 1, 5000, 70000], (4096, 65, _DIRECT, 0, 1, 0), [65, 0, 1, 2, 18]),
    (65, 0, [0, 0], (4096, 1, _DIRECT, 0, 1, 0), [0, 0]),
    (65, 1, [131072], (4096, 32, _DIRECT, 1, 1, 0), [32]),
    (200, 1, [1048576], (4096, 256, _KERNEL, 1, 0, 0), [256]),
]


@pytest.mark.parametrize("nb,source,n_pkts,head,n_parts", _GROUP_PLANS)
def test_group_plan_table(nb, source, n_pkts, head, n_parts):
    """The grouping plan every launch site builds (group_plan.cpp), pinned for the edges of its rules:
    partitions of whole 4096-packet chunks, at most 256 of them; packed 16-bit rows below 65536
    packets per partition; the direct scan up to 32,768 row entries; hist_kernel from 257 bins (always
    for the ring, whose rows are packed); the wide path above 1024 bins; one partition size for
    several batches, an empty batch having no partition and a call of only empty ones a grid of one."""
    import os

    from netbricks_amd._lib import lib

    if "NBG_GSCAN" in os.environ or "NBG_HIST_KERNEL_BINS" in os.environ:
        pytest.skip("NBG_GSCAN / NBG_HIST_KERNEL_BINS override the plan's rules")
    n = len(n_pkts)
    out = (C.c_uint32 * (6 + n))()
    assert lib.nbg_debug_group_plan(nb, (C.c_uint64 * n)(*n_pkts), n, source, out) == 0
    assert tuple(out[:6]) == head
    assert list(out[6:]) == n_parts
