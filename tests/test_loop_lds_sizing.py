"""Host arithmetic of the resident loop's LDS image (option loop_lds_blocks; no GPU): icp_loop_cu_lds_bytes and icp_loop_cu_lds_blocks of the library
against the rule written out here -- rows of 128 bytes, four per planned block, a 256-byte header, then as many whole blocks of 12-byte points as
the compute unit's 160 KiB hold, at most the plan's blocks, at most the cap; nothing for a plan whose rows and header pass 64 KiB."""

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
    return nbytes, blocks


def expected(nblk, ppb, cap):
    fixed = nblk * 4 * 128 + 256
    if fixed > BUDGET:
        return 0
    r = min(nblk, (TOTAL - fixed) // (ppb * 12))
    return r if cap < 0 else min(r, cap)


@pytest.mark.parametrize("ppb", [1024, 3072])
@pytest.mark.parametrize("nblk", [1, 9, 31, 32, 100, 127, 128, 300])
def test_blocks_and_bytes(sizing, nblk, ppb):
    nbytes, blocks = sizing
    fixed = nbytes(nblk)
    assert fixed == nblk * 512 + 256
    for cap in (-1, 0, 1, 2, 1000):
        r = blocks(nblk, ppb // 1024, cap)
        assert r == expected(nblk, ppb, cap), (nblk, ppb, cap)
        assert r <= nblk
        if fixed <= BUDGET:
            assert fixed + r * ppb * 12 <= TOTAL
    r = blocks(nblk, ppb // 1024, -1)
    if fixed <= BUDGET and r < nblk:                                 # not one block more would fit
        assert fixed + (r + 1) * ppb * 12 > TOTAL


def test_the_benchmark_plan(sizing):
    """Nine blocks of 3072 points: rows and header 4864 bytes, four blocks (147 456 bytes) behind them, 152 320 in all."""
    nbytes, blocks = sizing
    assert nbytes(9) == 4864 and blocks(9, 3, -1) == 4
    assert [blocks(n, 3, -1) for n in (1, 9, 31, 32, 100, 127)] == [1, 4, 4, 3, 3, 2]
    assert [blocks(n, 1, -1) for n in (1, 9, 31, 32, 100, 127)] == [1, 9, 12, 11, 9, 8]
