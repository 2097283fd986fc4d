"""CPU: the data view's one definition (csrc/data_view.h) under the host sanitizers
(-fsanitize=address,undefined), as a stand-alone program: what each kind of view exchanges with the
view in place (DESIGN §2f's table), that a second exchange restores both sides, and that the buffer
walk behind free_view / reset_data / sparse_view_bytes reaches every pointer field once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "data_view_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_data_view_exchange_and_buffers_under_sanitizers(tmp_path):
    exe = tmp_path / "data_view_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert [ln.split()[0] for ln in lines] == ["exchange"] * 4 + ["buffers"], r.stdout
    assert lines[-1] == "buffers 30, counted as a sparse view's bytes 21"
