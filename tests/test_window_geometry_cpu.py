"""kmcp-search's sliding-window geometry (cli/search_batch.hpp window_count / window_span: how many windows a record has, where each
starts and ends) against the library's kmcpg_window_count / kmcpg_window_locate, without a GPU - tests/window_geometry_check.cpp under
ASan/UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_library_cut_the_same_windows(tmp_path):
    exe = str(tmp_path / "window_geometry_check")
    lib_dir = os.path.join(ROOT, "kmcp_amd")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "window_geometry_check.cpp"), "-L" + lib_dir, "-lkmcpgpu", "-lz", "-lpthread",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout + r.stderr[-3000:]
