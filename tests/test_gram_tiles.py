"""CPU: the main Gram's 256 x 128 tile list with paired diagonal blocks (csrc/gram_tiles.h, shared by
the kernels and the host setup), compiled with the host sanitizers (-fsanitize=address,undefined):
tests/native/gram_tiles_check.cpp checks the coverage of the 128 x 128 blocks, the one owner of every
panel's fused Aᵀv rows and the item count for nb = 2, 4, 6, 10, 96, 128."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "gram_tiles_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gram_tile_list_coverage_under_sanitizers(tmp_path):
    exe = tmp_path / "gram_tiles_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr
    got = {}
    for ln in r.stdout.strip().splitlines():
        nb, paired, nt = (int(v) for v in ln.split())
        got[(nb, paired)] = nt
    for nb in (2, 4, 6, 10, 96, 128):
        nbi = nb // 2
        full = sum(2 * I + 2 for I in range(nbi))
        assert got[(nb, 0)] == full
        assert got[(nb, 1)] == full - nbi // 2
    assert got[(128, 0)] == 4160 and got[(128, 1)] == 4128   # m = 16384: 16.25 -> 16.125 rounds of 256
