"""The engine's host-side bookkeeping (PlanKey, GraphKey, graph_may_replay, CacheTag, DeviceBuf) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/host_pieces.cpp is compiled as a stand-alone host program, with DeviceBuf's device
calls swapped for malloc / free, and run.  No GPU and nothing loaded into this process."""
import os
import subprocess

from stablediffusion_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


def _compiler():
    """The clang++ next to hipcc (plain C++: the program has no device code); hipcc itself where the layout differs."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    return ([clang] if os.path.exists(clang) else [hipcc, "-x", "c++"]), rocm_include


def test_host_pieces_under_sanitizers(tmp_path):
    cc, rocm_include = _compiler()
    exe = str(tmp_path / "host_pieces")
    cmd = [*cc, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-DSD_DEVICEBUF_HOST_ALLOC", "-I", rocm_include, "-I", build.CSRC,
           os.path.join(HERE, "host_pieces.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and "host pieces: ok" in r.stdout, r.stdout + r.stderr
