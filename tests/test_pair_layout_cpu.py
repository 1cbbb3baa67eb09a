"""CPU: the compact pair list's chunk layout of csrc/ovl_pair_layout.h.

tests/c/pair_layout_check.cpp sweeps jobs cut as the pipeline cuts them, at both index widths and in every form of a
chunk's a area, and compares each area with the expressions the layout replaced: equal to the byte, 16-byte aligned,
disjoint, and inside the space up to the next chunk's base or the end of the job's buffer.  Here the program is
built with warnings as errors and run (`make pair-layout-check` runs it under the sanitizers)."""
import os
import subprocess

from conftest import PKG, ROOT


def test_pair_layout_check(tmp_path):
    exe = tmp_path / "pair_layout_check"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        "-o", str(exe), os.path.join(ROOT, "tests", "c", "pair_layout_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    # the sweep ran: every size from 1 to 4,200 alone is more chunks than this
    assert int(lines[0].split()[1]) > 100000
