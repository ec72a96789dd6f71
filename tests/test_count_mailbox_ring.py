"""CPU-only: the ring logic of the count mailbox (eprecon_amd/csrc/count_mailbox_ring.hpp) is host-only and free of HIP, so it
is compiled on its own with a stand-alone driver (tests/count_mailbox_ring_threads.cpp: four threads that acquire, publish,
release and abandon slots) under the host sanitizers and run as a program of its own.  Nothing is preloaded and nothing is
loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_ring_under_host_sanitizers(tmp_path, sanitizers):
    exe = tmp_path / "ring_threads"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-fsanitize={sanitizers}",
                           "-fno-sanitize-recover=all", "-pthread", "-I", os.path.join(ROOT, "eprecon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "count_mailbox_ring_threads.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ring ok" in out.stdout
