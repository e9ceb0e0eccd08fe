"""csrc/lupin_owned.hpp, the owner of every device allocation, over a counting host allocator under the sanitizers: no GPU.

tests/owned_main.cpp is a stand-alone program (its own main, nothing loaded into Python): it instantiates the owner template
and grow_buffer over malloc / free with a set of live pointers and a switch that fails the next allocation, and walks the
contract the device code relies on (make, failed make, moves, reset, swap, the nine-owner shape of ensure_path_buffers,
grow_buffer).  The device allocation-failure paths are covered here and by reading the code: no test provokes one on a GPU."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def sanitizer_runtime_flags(tmp):
    """The flags that link a sanitizer runtime the host compiler has (static, else shared), found with an empty program that
    must build and start; skips when neither does.  Only this empty program can turn a failure into a skip."""
    src, exe = os.path.join(tmp, "empty.cpp"), os.path.join(tmp, "empty")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    errors = []
    for runtimes in (["-static-libasan", "-static-libubsan"], []):
        try:
            build = subprocess.run(["g++"] + SANITIZE_FLAGS + runtimes + [src, "-o", exe], capture_output=True, text=True, timeout=120)
            if build.returncode == 0:
                start = subprocess.run([exe], capture_output=True, text=True, timeout=60)
                if start.returncode == 0:
                    return runtimes
                errors.append(start.stderr[-300:])
            else:
                errors.append(build.stderr[-300:])
        except (OSError, subprocess.SubprocessError) as e:
            errors.append(str(e))
    pytest.skip("the host compiler's sanitizer runtimes are not usable: an empty program with -fsanitize=address,undefined fails: " + " | ".join(errors))


def test_owner_contract_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        runtimes = sanitizer_runtime_flags(tmp)
        exe = os.path.join(tmp, "owned")
        build = subprocess.run(["g++"] + SANITIZE_FLAGS + runtimes + ["-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "owned_main.cpp"), "-o", exe],
                               capture_output=True, text=True, timeout=600)
        assert build.returncode == 0, build.stderr[-4000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
        print(run.stdout, run.stderr)
        assert run.returncode == 0, run.stderr[-4000:]
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
