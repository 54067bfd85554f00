"""The f16x3 range guard's bookkeeping (davo_amd/csrc/range_book.h) is plain host C++: tests/range_book_check.cpp exercises it
in a program of its own, built with the host compiler under AddressSanitizer and UBSan.  No GPU, no HIP, nothing of Python's
loaded into the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_book_bookkeeping_under_sanitizers(tmp_path):
    """Sequence numbers skip 0; the ring of eight rotates, holds and releases; the newest writer of a pose buffer wins
    (overlap, adjacency, earlier batches, the host path); spans are kept only behind a pending ticket and pruned; the deferred
    verdict is first-wins and cleared by taking it and by reset."""
    exe = str(tmp_path / "range_book_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing to preload
                           "-I", os.path.join(ROOT, "davo_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "range_book_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "range book ok" in out.stdout, (out.stdout + out.stderr)[-3000:]
