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
    block would not fit in the LDS the ring leaves (group.hip group_compact): the compact
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


@pytest.mark.parametrize("nbins,compact,lds", [
    (66, 0, 22368),
    (129, 0, 19616),
    (1001, 0, 40544),
    (1001, 1, 28176),
    (1024, 1, 28800),
])
def test_group_lds_pinned(nbins, compact, lds):
    """group_lds() (group.hip) is a hand-written mirror of the LDS carve-up at the top of group_kernel
    and group_direct_kernel: its bytes are pinned at C2's 66 bins (with the peer table), the first bin
    count without it, C3's 1001 bins on both kernels and the compact kernel's largest, so that a slip
    in the size function fails here and not as a kernel writing past its dynamic LDS."""
    from netbricks_amd._lib import lib

    assert lib.nbg_debug_group_lds(nbins, compact) == lds


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


_ROUTE_ENV = ("NBG_STREAM", "NBG_SMALL", "NBG_STREAM_GRID", "NBG_GSCAN", "NBG_HIST_KERNEL_BINS")
_SMALL, _TILED, _STREAM, _SDESC, _TPW = range(5)  # ClassifyKernel (nbgpu_internal.h)
_SWAP, _LDS, _OWNED, _DEFER, _LUTT, _SD, _LAG = 0x1, 0x2, 0x4, 0x10, 0x20, 0x40, 0x80  # NBG_* flags
_H65, _H1000 = (65, 65537), (1000, 655373)  # nb, M
_F, _D, _O = 0, 1, 2  # layout: fixed slots, offsets + lengths, offsets only
_M = 1048576


def _route_row(handle, layout, n, flags, expect, stride=64, fixed_len=60, mac_out=False, chain=False, aligned=True,
               capturing=False, ring=False, grouped=True, cus=256, grid_lds=256):
    bits = mac_out * 1 | chain * 2 | aligned * 4 | capturing * 8 | ring * 16 | grouped * 32
    return (handle, cus, grid_lds, layout, stride, fixed_len, n, flags, bits, expect)


# the issue's table, row by row: handle, layout, n, flags -> the route's fields it names
_ROUTES = [
    _route_row(_H65, _F, _M, _SWAP, dict(kernel=_STREAM, lean=1, win_owned=1, mode=1, tpw=8, grid=256, lag=0)),
    _route_row(_H65, _F, 262144, _SWAP, dict(kernel=_STREAM, tpw=2)),
    _route_row(_H65, _F, 262143, _SWAP, dict(kernel=_TPW, lds_lut=0, lean=1, tpw=1, grid=1024)),
    _route_row(_H65, _F, _M, _SWAP, dict(kernel=_TPW, lds_lut=0), ring=True),
    _route_row((65, 65539), _F, _M, _SWAP, dict(kernel=_TPW)),
    _route_row(_H65, _F, _M, _SWAP, dict(kernel=_STREAM, mode=2), mac_out=True),
    _route_row(_H65, _F, _M, 0, dict(kernel=_STREAM, mode=0)),
    _route_row(_H65, _F, _M, _SWAP, dict(kernel=_TPW, lean=0, win_owned=1), fixed_len=47),
    _route_row(_H65, _F, _M, _SWAP, dict(kernel=_TPW, lean=0), stride=72),
    _route_row(_H65, _F, _M, _SWAP, dict(kernel=_TPW, lean=0, win_owned=0), stride=48, fixed_len=48),
    _route_row(_H65, _F, _M, _SWAP, dict(kernel=_TPW, lean=0), aligned=False),
    _route_row(_H65, _F, _M, _SWAP | _LDS, dict(kernel=_TPW, lds_lut=1, tpw=4, grid=256), grid_lds=256),
    _route_row(_H65, _F, _M, _SWAP | _LDS, dict(kernel=_TPW, lds_lut=0), ring=True),
    _route_row(_H1000, _F, _M, _SWAP | _LDS, dict(kernel=_TPW, lds_lut=0)),  # 1,310,752 B > 72 KiB
    _route_row(_H1000, _F, _M, _SWAP, dict(kernel=_TPW, lds_lut=0)),
    _route_row(_H1000, _F, _M, _SWAP | _LUTT, dict(kernel=_TILED)),
    _route_row(_H1000, _F, _M, _LUTT, dict(kernel=_TPW), chain=True),
    _route_row(_H65, _F, 2048, _SWAP, dict(kernel=_SMALL)),
    _route_row(_H65, _F, 2049, _SWAP, dict(kernel=_TPW)),
    _route_row(_H65, _F, 100, _DEFER, dict(kernel=_TPW)),
    _route_row(_H65, _F, 100, _LDS, dict(not_small=1)),
    _route_row(_H65, _F, 100, _LUTT, dict(not_small=1)),
    _route_row(_H65, _F, 100, 0, dict(not_small=1), chain=True),
    _route_row(_H65, _F, 100, _SWAP, dict(not_small=1), aligned=False),
    _route_row((1023, 65537), _F, 100, 0, dict(kernel=_SMALL)),
    _route_row((1024, 65537), _F, 100, 0, dict(not_small=1)),  # 1025 bins
    _route_row(_H65, _D, _M, _OWNED, dict(kernel=_TPW, win_owned=1, lean=0, fill_len=0)),
    _route_row(_H65, _D, _M, _OWNED | _SD, dict(kernel=_SDESC, mode=0)),
    _route_row(_H65, _D, _M, _OWNED | _SD | _SWAP, dict(kernel=_TPW)),  # in place does not fit with the u8 LUT
    _route_row(_H65, _D, _M, _OWNED | _SD | _SWAP, dict(kernel=_SDESC, mode=2), mac_out=True),
    _route_row(_H65, _D, _M, _OWNED | _SD, dict(kernel=_SDESC, mode=0), chain=True),
    _route_row(_H1000, _D, _M, _OWNED | _SD | _SWAP, dict(kernel=_SDESC, mode=1)),
    _route_row(_H1000, _D, _M, _OWNED | _SD, dict(kernel=_TPW), chain=True),
    _route_row(_H65, _D, _M, _SD, dict(kernel=_TPW)),
    _route_row(_H65, _D, 262143, _OWNED | _SD, dict(kernel=_TPW)),
    _route_row(_H65, _O, _M, 0, dict(kernel=_TPW, fill_len=1)),
    _route_row(_H65, _O, 2048, 0, dict(kernel=_SMALL, fill_len=0)),
    # captured: classify_common refuses a route that needs the length fill ("pass d_len to capture ...")
    _route_row(_H65, _O, _M, 0, dict(kernel=_TPW, fill_len=1), capturing=True),
    _route_row(_H65, _F, _M, _SWAP | _LAG, dict(kernel=_STREAM, lag=1)),
    _route_row(_H65, _F, _M, _SWAP | _LAG, dict(kernel=_STREAM, lag=0), cus=128),  # 256 partitions > 128 blocks
    _route_row(_H65, _F, _M, _SWAP | _LAG, dict(lag=0), grouped=False),
    _route_row(_H65, _F, _M, _SWAP | _LAG | _LUTT, dict(kernel=_STREAM, lag=0)),
    _route_row((256, 65537), _F, 524288, _SWAP | _LAG, dict(kernel=_STREAM, lag=0)),  # 257 bins: hist_kernel rows
    _route_row((187, 65537), _F, 524288, _SWAP | _LAG, dict(lag=1)),  # 163,488 B of LDS
    _route_row((188, 65537), _F, 524288, _SWAP | _LAG, dict(lag=0)),  # 163,872 B > 160 KiB
    _route_row((255, 65537), _F, 524288, _SWAP | _LAG, dict(lag=1), mac_out=True),  # mode 2 rows are 48 B
    _route_row((187, 65537), _F, _M, _SWAP | _LAG, dict(lag=0)),  # 188 x 256 row entries > 32,768: scan kernel
]


@pytest.mark.parametrize("handle,cus,grid_lds,layout,stride,fixed_len,n,flags,bits,expect", _ROUTES,
                         ids=[str(i + 1) for i in range(len(_ROUTES))])
def test_classify_route_table(handle, cus, grid_lds, layout, stride, fixed_len, n, flags, bits, expect):
    """The classify route every launch site takes (classify_route.cpp), pinned at the edges of its
    rules: 2,048 packets (small kernel), 262,144 (streaming), M <= 65537, 256 / 257 bins, a
    persistent ring on the device, the fixed-slot rule, the write mode, the descriptor streaming
    modes, the length fill, and the lagged launch's partition, scan and 160 KiB LDS bounds."""
    import os

    from netbricks_amd._lib import lib

    if any(e in os.environ for e in _ROUTE_ENV):
        pytest.skip("NBG_STREAM / NBG_SMALL / NBG_STREAM_GRID / NBG_GSCAN / NBG_HIST_KERNEL_BINS override the rules")
    out = (C.c_uint32 * 9)()
    nb, m = handle
    assert lib.nbg_debug_classify_route(nb, m, cus, grid_lds, 1, layout, stride, fixed_len, n, flags, bits, out) == 0
    got = dict(zip(("kernel", "lds_lut", "win_owned", "lean", "fill_len", "lag", "mode", "tpw", "grid"), out))
    got["not_small"] = int(got["kernel"] != _SMALL)
    assert {k: got[k] for k in expect} == expect


# handle, batch sizes, fused; stride 64, fixed_len 60, aligned, no ring, grouped unless said
_FUSED = [
    (_H65, [131072, 131072], {}, 1),
    (_H65, [131072, 131071], {}, 0),
    (_H65, [262144, 0], {}, 0),  # an empty batch
    (_H65, [131072, 131072], dict(stride=72), 0),
    (_H65, [131072, 131072], dict(stride=48), 0),
    (_H65, [131072, 131072], dict(ring=True), 0),
    ((255, 65537), [524288, 524288], {}, 1),  # 256 bins x 128 partitions = 32,768: direct scan
    ((255, 65537), [1048576, 1048576], {}, 0),  # scan kernel
    ((255, 65537), [1048576, 1048576], dict(grouped=False), 1),
    ((256, 65537), [524288, 524288], {}, 0),  # 257 bins
]


@pytest.mark.parametrize("handle,sizes,extras,fused", _FUSED, ids=[str(i + 1) for i in range(len(_FUSED))])
def test_multi_fused_table(handle, sizes, extras, fused):
    """nbg_maglev_classify_device_multi's fused rule (classify_route.cpp multi_fused): lean slots in
    every batch, none empty, 262,144 packets in all, at most 256 bins, no ring, and a grouping that
    scans directly."""
    import os

    from netbricks_amd._lib import lib

    if any(e in os.environ for e in _ROUTE_ENV):
        pytest.skip("NBG_STREAM / NBG_SMALL / NBG_STREAM_GRID / NBG_GSCAN / NBG_HIST_KERNEL_BINS override the rules")
    bits = 4 | extras.get("ring", False) * 16 | extras.get("grouped", True) * 32
    n = len(sizes)
    nb, m = handle
    got = lib.nbg_debug_multi_fused(nb, m, 256, (C.c_uint64 * n)(*sizes), n, extras.get("stride", 64), 60, bits)
    assert got == fused
