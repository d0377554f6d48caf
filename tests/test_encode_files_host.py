"""The host half of bjxa_hip_encode_files under ASan and UBSan: libbjxa.c,
the CPU core and the no-device stand-in for the HIP side compiled into one
stand-alone program with tests/c/test_encode_files.c, which is run directly
(no shared library, nothing loaded into Python).  No GPU needed."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "bjxa_amd", "csrc")


def test_encode_files_host_sanitized(tmp_path):
    exe = tmp_path / "test_encode_files"
    # libbjxa.c is built with the Makefile's forced includes; its c99 flags
    # would hide ssize_t from the test program, which includes sys/types.h
    cmd = ["gcc", "-std=c99", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-include", "stdio.h", "-include", "sys/types.h",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", str(exe),
           os.path.join(ROOT, "tests", "c", "test_encode_files.c"),
           os.path.join(CSRC, "libbjxa.c"), os.path.join(CSRC, "xa_cpu.c"),
           os.path.join(CSRC, "xa_gpu_none.c"), "-lpthread"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    r = subprocess.run([str(exe)], stdin=subprocess.DEVNULL, capture_output=True, text=True,
                       env=env, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_encode_files: ok" in r.stdout
