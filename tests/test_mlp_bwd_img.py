"""CPU check of the LDS-DMA tile images of the MLP step's backward (csrc/kernels/mlp_bwd_img.h): builds
tools/check_mlp_bwd_img.cpp with the host compiler and runs it.  The program proves, for K0 = 32 and 64,
that every 16-byte chunk of a dact2 tile and of an X tile is written exactly once, inside its buffer and
lane-linearly, that every reader gets the elements it got from the register-staged images, and that
every read instruction is bank-conflict-free under the LDS lane groups."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_bwd_lds_images(tmp_path):
    cxx = _host_cxx()
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "check_mlp_bwd_img")
    src = os.path.join(ROOT, "tools", "check_mlp_bwd_img.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "csrc", "kernels"), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:")
