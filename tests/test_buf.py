"""The owning buffer type (csrc/kh_buf.h) on the CPU: tests/cpp/test_buf.cpp is a program of its own over a
malloc-backed policy, built here with the address and undefined-behaviour sanitizers and run.  No GPU, no library."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def _host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = cand and shutil.which(cand)
        if p:
            return p
    return None


def test_buffer_type_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found (set CXX=...)"
    src = os.path.join(ROOT, "tests", "cpp", "test_buf.cpp")
    exe = str(tmp_path / "test_buf")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-self-move",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("test_buf: ok")


def test_buffer_header_is_host_only():
    """kh_buf.h includes nothing from HIP (the CPU program above could not build otherwise) and stays out of the
    hash of the device-code headers: the hash speaks of kernels."""
    from kuiperllama_amd import build
    text = open(os.path.join(build.CSRC, "kh_buf.h")).read()
    assert "hip/" not in text and "kh_common.h" not in text
    assert "kh_buf.h" in build.HEADERS
    import hashlib
    h = hashlib.sha1()
    for f in sorted(os.listdir(build.CSRC)):
        if f.startswith("kh_") and f.endswith(".h") and f not in ("kh_model_internal.h", "kh_dispatch.h", "kh_buf.h"):
            h.update(f.encode())
            h.update(open(os.path.join(build.CSRC, f), "rb").read())
    assert build.kernel_sources_sha1() == h.hexdigest()
