"""Host-only check of the eight-phase NT GEMM's tile-to-workgroup assignment (gemm8.h g8_tiles, the function the kernel calls):
for every persistent grid 1..256 and every tile count 1..1536 each output tile is taken by exactly one workgroup, exactly once."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_tile_exactly_once():
    from commu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "commu-code_amd", "build.py")])
    lib = _lib.load()
    fn = lib.commu_gemm8_tile_cover
    fn.argtypes = [ctypes.c_int, ctypes.c_int]
    fn.restype = ctypes.c_int
    for grid in range(1, 257):
        assert fn(grid, 1536) == 0, grid
    assert fn(0, 16) == -1
