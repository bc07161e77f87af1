"""Host arithmetic of the resident loop's full LDS layout (options loop_lds_tables and loop_waves; no GPU): icp_loop_cu_layout of the library against
the rule written out here.  Rows of 128 bytes, four per planned block, and a 256-byte header; then the scene's two tables, width + height floats
rounded up to four (a width and height of 0: no tables asked for); then whole blocks of 12-byte points in what is left of the limit -- 160 KiB for
a 16-wave workgroup, 80 KiB for an 8-wave one, two of which share a compute unit -- at most the plan's blocks, at most the cap.  Tables first,
whole blocks after: the tables are granted whenever they fit beside rows and header.  Nothing for a plan whose rows and header pass 64 KiB."""

import ctypes as C

import pytest

from pose_refine_amd import _lib

TOTAL = 160 << 10
BUDGET = 64 << 10


@pytest.fixture(scope="module")
def sizing():
    lib = C.CDLL(_lib.LIB_PATH)
    nbytes = getattr(lib, "_ZN3prk21icp_loop_cu_lds_bytesEj")
    nbytes.restype, nbytes.argtypes = C.c_size_t, [C.c_uint32]
    blocks = getattr(lib, "_ZN3prk22icp_loop_cu_lds_blocksEjji")
    blocks.restype, blocks.argtypes = C.c_uint32, [C.c_uint32, C.c_uint32, C.c_int]
    fn = getattr(lib, "_ZN3prk18icp_loop_cu_layoutEjjijjjPj")
    fn.restype, fn.argtypes = C.c_uint32, [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]

    def layout(nblk, steps, cap, width, height, waves):
        fixed = C.c_uint32()
        r = fn(nblk, steps, cap, width, height, waves, C.byref(fixed))
        return r, fixed.value

    return nbytes, blocks, layout


def expected(nblk, ppb, cap, width, height, waves):
    limit = TOTAL if waves == 16 else TOTAL // 2
    rows = nblk * 4 * 128 + 256
    if rows > BUDGET:
        return 0, rows
    tables = 4 * ((width + height + 3) // 4 * 4)
    if rows + tables > limit:
        tables = 0
    r = min(nblk, (limit - rows - tables) // (ppb * 12))
    return (r if cap < 0 else min(r, cap)), rows + tables


@pytest.mark.parametrize("waves", [16, 8])
@pytest.mark.parametrize("size", [(640, 480), (1280, 720), (96, 64), (4096, 3000), (0, 0)])
@pytest.mark.parametrize("ppb", [1024, 3072])
def test_layout_follows_the_rule(sizing, waves, size, ppb):
    nbytes, blocks, layout = sizing
    limit = TOTAL if waves == 16 else TOTAL // 2
    for nblk in (1, 4, 9, 22, 31, 32, 100, 127, 128, 300):
        for cap in (-1, 0, 1, 2, 1000):
            r, fixed = layout(nblk, ppb // 1024, cap, *size, waves)
            assert (r, fixed) == expected(nblk, ppb, cap, *size, waves), (nblk, ppb, cap, size, waves)
            assert r <= nblk and fixed >= nbytes(nblk)
            if nbytes(nblk) <= BUDGET:
                assert fixed + r * ppb * 12 <= limit
            if waves == 16:                                          # without tables, the 16-wave layout is the old function
                assert layout(nblk, ppb // 1024, cap, 0, 0, 16) == (blocks(nblk, ppb // 1024, cap), nbytes(nblk))
        r, fixed = layout(nblk, ppb // 1024, -1, *size, waves)
        if nbytes(nblk) <= BUDGET and r < nblk:                      # not one block more would fit
            assert fixed + (r + 1) * ppb * 12 > limit


def test_the_benchmark_plan(sizing):
    """Nine blocks of 3072 points at 640 x 480: rows and header 4864 bytes, tables 4480."""
    nbytes, blocks, layout = sizing
    # 16 waves: 4864 + 4480 + 4 * 36 864 = 156 800, still four blocks; without tables 152 320
    assert layout(9, 3, -1, 640, 480, 16) == (4, 4864 + 4480)
    assert layout(9, 3, -1, 0, 0, 16) == (4, 4864)
    # 8 waves, 80 KiB: two blocks (78 592) or the tables and one (46 208); tables and two blocks are 83 072
    assert layout(9, 3, -1, 0, 0, 8) == (2, 4864)
    assert layout(9, 3, -1, 640, 480, 8) == (1, 4864 + 4480)


def test_the_window_plan_keeps_four_blocks(sizing):
    """22 blocks: 11 520 + 4480 + 147 456 = 163 456 of the 163 840 bytes."""
    nbytes, blocks, layout = sizing
    assert nbytes(22) == 11520
    assert layout(22, 3, -1, 640, 480, 16) == (4, 16000)
    assert 4 * ((640 + 480 + 3) // 4 * 4) <= 4864


def test_a_large_frame(sizing):
    """1280 x 720: 8000 bytes of tables.  Tables first: the whole-frame plan of 100 blocks at 640 x 480 gives a block for them."""
    nbytes, blocks, layout = sizing
    assert layout(9, 3, -1, 1280, 720, 16) == (4, 4864 + 8000)
    assert layout(9, 3, -1, 1280, 720, 8) == (1, 4864 + 8000)
    assert layout(100, 3, -1, 0, 0, 16) == (3, 51456)                 # 51 456 + 3 * 36 864 = 162 048: 4480 more do not fit
    assert layout(100, 3, -1, 640, 480, 16) == (2, 51456 + 4480)


def test_rows_over_the_budget(sizing):
    nbytes, blocks, layout = sizing
    assert nbytes(128) == 65792 > BUDGET
    for waves in (16, 8):
        assert layout(128, 3, -1, 640, 480, waves) == (0, 65792)
        assert layout(128, 3, -1, 0, 0, waves) == (0, 65792)
    assert layout(127, 3, -1, 640, 480, 16) == (2, 65280 + 4480)
    assert layout(127, 3, -1, 640, 480, 8) == (0, 65280 + 4480)      # 80 KiB: rows, header and tables, no block
    assert layout(127, 3, -1, 4096, 3000, 8) == (0, 65280)           # 28 384 bytes of tables do not fit 80 KiB beside these rows: none


def test_the_old_functions_keep_their_values(sizing):
    nbytes, blocks, layout = sizing
    assert nbytes(9) == 4864 and blocks(9, 3, -1) == 4
    assert [blocks(n, 3, -1) for n in (1, 9, 31, 32, 100, 127)] == [1, 4, 4, 3, 3, 2]
    assert [blocks(n, 1, -1) for n in (1, 9, 31, 32, 100, 127)] == [1, 9, 12, 11, 9, 8]
    for nblk in (1, 9, 31, 32, 100, 127, 128, 300):
        assert nbytes(nblk) == nblk * 512 + 256
