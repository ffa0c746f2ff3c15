"""ABI of the sliding-window entry points (include/kmcp_gpu.h kmcpg_window_spec): the ctypes mirror in kmcp_amd/lib.py has the C layout, as a C
compiler lays the struct out from the header."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "kmcp_gpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(kmcpg_window_spec), offsetof(kmcpg_window_spec, step), offsetof(kmcpg_window_spec, window),
         offsetof(kmcpg_window_spec, greedy), offsetof(kmcpg_window_spec, reserved));
  return 0;
}
'''


def test_window_spec_layout(tmp_path):
    from kmcp_amd import lib
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    (tmp_path / "w.c").write_text(SRC)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "w"), str(tmp_path / "w.c")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "w")], capture_output=True, text=True, check=True).stdout.split()]
    W = lib.WindowSpec
    assert got == [C.sizeof(W), W.step.offset, W.window.offset, W.greedy.offset, W.reserved.offset] == [24, 0, 8, 16, 20]
