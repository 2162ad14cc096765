"""The host programs under tests/tools/ for the tests that use them: each includes one header of csrc/ and has its own main, is built with
the host compiler -- plainly or under the address and undefined-behaviour sanitizers -- and runs as its own process.  Nothing is loaded
into Python.  No GPU."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drl-dronenavigation_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def rocm_include():
    """The include directory of the HIP headers, or None where they are not installed."""
    hipcc = shutil.which("hipcc")
    roots = [os.environ.get("ROCM_PATH"), os.path.dirname(os.path.dirname(os.path.realpath(hipcc))) if hipcc else None, "/opt/rocm"]
    for r in roots:
        if r and os.path.exists(os.path.join(r, "include", "hip", "hip_runtime.h")):
            return os.path.join(r, "include")
    return None


def build(name, directory, sanitize=False, hip_headers=False, extra_flags=()):
    """tests/tools/<name>.cpp -> <directory>/<name>; the path, or None when hip_headers is asked for and they are not installed."""
    hip = []
    if hip_headers:
        inc = rocm_include()
        if inc is None:
            return None
        hip = ["-D__HIP_PLATFORM_AMD__", "-I" + inc]
    exe = os.path.join(str(directory), name)
    src = os.path.join(ROOT, "tests", "tools", name + ".cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + list(extra_flags) + hip + ["-I" + CSRC] + (SANITIZE if sanitize else []) + [src, "-o", exe])
    return exe


def run_lines(exe, *args, timeout=60):
    """Runs the program; its exit status must be 0.  Returns its last line of output parsed as JSON, and all its lines."""
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    return json.loads(lines[-1]), lines


def run(exe, *args, timeout=60):
    """The result of a program that prints its result line and nothing else, parsed."""
    result, lines = run_lines(exe, *args, timeout=timeout)
    assert len(lines) == 1, lines
    return result
