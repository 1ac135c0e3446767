"""The stand-alone host programs of tests/host/: built with the sanitizers and
run directly, never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(name, tmp_path, *, float_cast=True, no_warnings=False, word=None):
    """tests/host/<name>_main.cpp as an executable under ``tmp_path``, built
    with ASan + UBSan (``float_cast``: float-cast-overflow too); skips where
    there is no compiler or no sanitizer runtime.  ``word``: what a compile
    error of the program's own mentions (default: ``name``)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / (name + "_main"))
    sanitize = ["-fsanitize=undefined,address"] + (["-fsanitize=float-cast-overflow"] if float_cast else [])
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           *sanitize, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rossby-wave-ray-tracing_amd", "csrc"),
           "-o", exe, os.path.join(ROOT, "tests", "host", name + "_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr and (word or name) not in b.stderr:
        pytest.skip("this toolchain has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    if no_warnings:
        assert "warning" not in b.stderr, b.stderr[-3000:]
    return exe


def fixture(name, **kw):
    """A module-scoped fixture that builds the program once: ``host_program = fixture("flux_rows")``."""
    @pytest.fixture(scope="module")
    def host_program(tmp_path_factory):
        return build(name, tmp_path_factory.mktemp(name), **kw)
    return host_program


def sanitizer_env():
    """The environment a program runs in."""
    # (verify_asan_link_order=0: the environment may preload a library of its own)
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
                UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def run_process(exe, lines=None, args=(), timeout=120):
    """The finished process of ``exe args`` fed ``lines`` on stdin: it ended
    with status 0 and no sanitizer had anything to say."""
    text = None if lines is None else "\n".join(lines) + "\n"
    r = subprocess.run([exe, *args], input=text, capture_output=True, text=True, env=sanitizer_env(),
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return r


def run(exe, lines, timeout=120):
    """The lines ``exe`` wrote to stdout when fed ``lines``."""
    return run_process(exe, lines, timeout=timeout).stdout.splitlines()
