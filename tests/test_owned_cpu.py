"""CPU check of the buffer owner (csrc/iqlhip_owned.h) on its own: tools/owned_check.cpp instantiates OwnedT on a stub
allocator, fails the n-th allocation of a feature for every n, rolls back, and asserts that everything made since the
mark is freed exactly once, every stored pointer is null again, earlier allocations survive and release_all frees the
rest (its own bookkeeping: the stub counts every free of every block).  A stand-alone host program: no GPU, nothing
loaded into Python.  The file's header gives the AddressSanitizer / UBSan build of the same program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")      # the compiler the library's build brings


def test_owned_rolls_back_and_releases(tmp_path):
    exe = str(tmp_path / "owned_check")
    cmd = [CXX, "-std=c++17", "-g", "-O1", "-Wall",
           "-I", os.path.join(ROOT, "jsrl-corl_amd", "csrc"), os.path.join(ROOT, "tools", "owned_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert res.stdout.count(": ok (") == 6 and "owned_check: all checks passed" in res.stdout
