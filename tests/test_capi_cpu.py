"""The C-ABI library builds for gfx950, loads without a GPU and exports every symbol include/geobo_hip.h declares.
No compute calls here (CPU-only container)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from geobo_amd.build import build
    path = build()
    assert os.path.exists(path)
    return ctypes.CDLL(path)


def declared_functions():
    src = open(os.path.join(ROOT, "include", "geobo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(geobo_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    names = declared_functions()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), "libgeobo_hip.so does not export %s" % n


def test_ctypes_table_matches_header():
    from geobo_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_functions()
    _lib.load()


def test_host_side_helpers(lib):
    lib.geobo_pad_m.restype = ctypes.c_int64
    lib.geobo_pad_m.argtypes = [ctypes.c_int64]
    lib.geobo_pad_n.restype = ctypes.c_int64
    lib.geobo_pad_n.argtypes = [ctypes.c_int64]
    lib.geobo_potrf_ws_bytes.restype = ctypes.c_size_t
    lib.geobo_potrf_ws_bytes.argtypes = [ctypes.c_int64]
    assert lib.geobo_version() == 213
    assert lib.geobo_pad_m(8242) == 8448 and lib.geobo_pad_m(256) == 256 and lib.geobo_pad_m(1) == 256
    assert lib.geobo_pad_n(480) == 512 and lib.geobo_pad_n(262144) == 262144
    # one T buffer per node [lo, mid, hi) of the L^-1 tree, (hi - mid) x (mid - lo) blocks of 128 x 128; split on even block counts
    def tree_blocks(n):
        if n <= 1:
            return 0
        mid = n // 2
        if n > 2 and mid & 1:
            mid += 1
        return (n - mid) * mid + tree_blocks(mid) + tree_blocks(n - mid)
    assert tree_blocks(8) == 16 + 2 * 4 + 4 * 1 and tree_blocks(66) == 2145
    # ... followed by the counters of the persistent tile-DAG kernel: 16 control words, nb row counters, nb x nb tile flags, 2 nb flags of
    # the partial sums parked for the chain walker (round 6)
    for m in (256, 1024, 2048, 8448, 33024):
        nb = m // 128
        assert lib.geobo_potrf_ws_bytes(m) == tree_blocks(nb) * 128 * 128 * 8 + 4 * (16 + 3 * nb + nb * nb)


def test_argument_validation_without_gpu(lib):
    """Entry points validate before touching the device: null pointers / misaligned dims give error codes."""
    from geobo_amd import _lib
    L = _lib.load()
    assert L.geobo_gemm_nt(256, 128, 16, 1.0, None, 16, None, 16, 0.0, None, 128, 0, 0, None) == -1
    assert L.geobo_ak_fused(1, None, 256, 256, 256, None, None, None, 0, 128, 1., 1., 1., 1., None, 128, None) == -1
    assert L.geobo_potrf_inv(100, None, 100, None, 100, None, None, 0, None, 0, None) == -1
    # an unknown schedule is refused FIRST: with pointers that must not be looked at (nothing here is device memory) and no device
    for dummy in (0x1000, 0x7fff0000):
        assert L.geobo_potrf_inv(256, dummy, 256, dummy, 256, dummy, dummy, 1 << 30, None, 7, None) == -1
        assert L.geobo_potrf_inv(256, dummy, 256, dummy, 256, dummy, dummy, 1 << 30, None, -1, None) == -1
    hdr = open(os.path.join(ROOT, "include", "geobo_hip.h")).read()
    assert re.search(r"GEOBO_POTRF_AUTO = 0, GEOBO_POTRF_STREAMS = 1, GEOBO_POTRF_DAG = 2\b", hdr)
    from geobo_amd import hip
    assert hip.POTRF_SCHEDULES == {"auto": 0, "streams": 1, "dag": 2}
    with pytest.raises(ValueError):
        hip.potrf_inv(None, schedule="stream")


def test_the_library_reads_no_environment(lib):
    """Every choice reaches the C library as an argument: it imports no getenv (a minimal hipcc-built shared object imports none either,
    so the runtime's own start-up code does not hide one), and no source under csrc names it."""
    import subprocess
    from geobo_amd.build import CSRC, LIB
    syms = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout.split()
    assert any(s.startswith("hipLaunchKernel") for s in syms)                   # (the listing is what it should be: the runtime's entry points are in it)
    assert not [s for s in syms if "getenv" in s]
    for f in sorted(os.listdir(CSRC)):
        assert "getenv" not in open(os.path.join(CSRC, f)).read(), f


@pytest.mark.parametrize("nbi,nbj,tm,tn", [(33, 32, 256, 128), (33, 66, 256, 128), (66, 66, 128, 128), (5, 3, 128, 128), (4, 64, 256, 128),
                                            (17, 9, 256, 128)])
def test_tile_order_visits_every_tile_once(nbi, nbj, tm, tn):
    """The arithmetic item order the GEMM launches decode on the device (no tile lists in device memory any more): every
    valid tile exactly once, for the plain, lower-only and triangular-operand forms."""
    import numpy as np
    from geobo_amd import _lib
    L = _lib.load()
    for lower, xl, yl in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        buf = (ctypes.c_int * (nbi * nbj))()
        n = L.geobo_tile_order(nbi, nbj, tm, tn, lower, xl, yl, buf, nbi * nbj)
        got = [(v >> 16, v & 0xffff) for v in list(buf)[:n]]
        want = {(bi, bj) for bi in range(nbi) for bj in range(nbj) if not lower or bj * tn < (bi + 1) * tm}
        assert n == len(want) and len(set(got)) == n and set(got) == want, (lower, xl, yl)
        if lower or not (xl or yl):
            # 32 consecutive items = at most 4 row tiles (one band): the supertile an XCD's L2 holds
            for g in range(0, n, 32):
                rows = {bi for bi, _ in got[g:g + 32]}
                assert max(rows) - min(rows) <= 7
        if xl:
            assert [bi for bi, _ in got] == sorted((bi for bi, _ in got), reverse=True)   # longest contraction first
        if yl:
            assert [bj for _, bj in got] == sorted(bj for _, bj in got)


def _map_rule(ymode, reduce, nbi, nbj, tm, tn, tri, batch, lower_items):
    """Plain transcription of the choice in launch() (gemm_f64.hip): (map, items per batch, grid x, grid y)."""
    mem = ymode in (1, 2, 4)
    lower, xy = tri & 1, tri & 6
    xcd_map = 1 if nbi >= 8 else 0
    if mem and not lower and nbi >= 4 and nbj >= 8:
        xcd_map = 2
    ntiles = 0
    if (mem and not reduce and batch <= 64 and nbi * nbj >= (16 if xy else 64) and nbi * nbj * batch <= 65536 and nbi <= 4096
            and xy != 6):
        ntiles = lower_items if lower else nbi * nbj
        if ntiles > 0:
            xcd_map = 3
    if xcd_map == 3:
        groups = (ntiles * batch + 31) // 32
        return 3, ntiles, 256 * ((groups + 7) // 8), 1
    nblocks = nbi * nbj
    if xcd_map == 1:
        nblocks = 8 * ((nbi + 7) // 8) * nbj
    if xcd_map == 2:
        nst = nbi * ((nbj + 31) // 32) if tri & 2 else ((nbi + 3) // 4) * ((nbj + 7) // 8)
        nblocks = 256 * ((nst + 7) // 8)
    return xcd_map, 0, nblocks, batch


@pytest.mark.parametrize("ymode", [0, 1, 2, 3, 4])
def test_gemm_map_matches_the_launch_rule(ymode):
    """geobo_gemm_map is the function launch() itself calls: map, item count and grid against the rule written out in Python, for
    every flag combination, both tile heights, both epilogues and batches on either side of the map-3 limit of 64."""
    from geobo_amd import _lib
    L = _lib.load()
    out = (ctypes.c_int * 4)()
    seen = set()
    for tm in (128, 256):
        for nbi in range(1, 41):
            for nbj in range(1, 41):
                # tiles with col0 < row0 + tm: row tile bi has its first ceil((bi + 1) tm / 128) column tiles
                lower_items = sum(min(nbj, -(-(bi + 1) * tm // 128)) for bi in range(nbi))
                for tri in range(8):
                    for batch in (1, 3, 64, 65):
                        for reduce in (0, 1):
                            assert L.geobo_gemm_map(ymode, reduce, nbi, nbj, tm, 128, tri, batch, out) == 0
                            want = _map_rule(ymode, reduce, nbi, nbj, tm, 128, tri, batch, lower_items)
                            assert tuple(out) == want, (ymode, reduce, nbi, nbj, tm, tri, batch)
                            seen.add(want[0])
    assert seen == ({0, 1, 2, 3} if ymode in (1, 2, 4) else {0, 1})
    for bad in ((5, 0, 4, 4, 256, 128, 0, 1), (1, 0, 0, 4, 256, 128, 0, 1), (1, 0, 4, 4, 64, 128, 0, 1), (1, 0, 4, 4, 256, 64, 0, 1),
                (1, 0, 4, 4, 256, 128, 8, 1), (1, 0, 4, 4, 256, 128, 0, 0)):
        assert L.geobo_gemm_map(*bad, out) == -1


def test_gemm_map_wrapper_picks_the_tile_height():
    """hip.gemm_map does the tile choice of launch_by_rows: 256-row tiles when m % 256 == 0 and not small_tiles, else 128."""
    from geobo_amd import hip
    assert hip.gemm_map(2304, 1024) == dict(map=3, ntiles=72, nblocks=256, grid_y=1, nbi=9, nbj=8, tm=256)
    assert hip.gemm_map(1280, 1024, small_tiles=True)["tm"] == 128 and hip.gemm_map(1152, 1024)["nbi"] == 9
    assert hip.gemm_map(2304, 384) == dict(map=1, ntiles=0, nblocks=48, grid_y=1, nbi=9, nbj=3, tm=256)
    assert hip.gemm_map(1152, 1024, batch=65, entry="gemm_batched_nt")["map"] == 2
    assert hip.gemm_map(1152, 1024, batch=64, entry="gemm_batched_nt")["ntiles"] == 72
    r = hip.gemm_map(1280, 1152, entry="posterior_reduce", m_valid=1100)
    assert (r["map"], r["nbi"], r["nbj"], r["nblocks"]) == (2, 5, 9, 256)
    assert hip.gemm_map(2304, 256, entry="ak_fused")["map"] == 1 and hip.gemm_map(256, 256, entry="ak_fused_grid")["map"] == 0


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "geobo_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "geobo_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, f


def test_compute_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from geobo_amd import _lib, kernels
    with pytest.raises(_lib.GeoboHipUnavailable):
        kernels.gpkernel([1.0, 2.0], 3.0)
