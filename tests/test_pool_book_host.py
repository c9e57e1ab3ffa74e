"""The bookkeeping of the device allocator (padne_amd/csrc/pool_book.hpp: size rounding with guard zones, alignment of the
pointer handed out, the requested size per block, cached blocks across a switch of PADNE_POOL_GUARD) in a stand-alone host
program, tests/native/pool_book_test.cpp, built with AddressSanitizer and UBSan and run on its own: a fake allocate / free pair
stands in for the device, no device code is involved."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_bookkeeping_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pool_book_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "pool_book_test.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pool_book ok" in run.stdout
