"""The coalescer of concurrent single-query searches (rlr_index_set_coalescing) under ThreadSanitizer on the CPU build:
the host half of every translation unit of csrc/ (hipcc --offload-host-only -fsanitize=thread), built exactly as
test_host_sanitize_cpu.py builds it, linked against the CPU stand-in for the HIP runtime (tests/sanitize/stub_hip.cpp)
and driven by tests/sanitize/tsan_coalesce.cpp: 4 / 8 / 12 / 16 caller threads of single-query searches with mixed k
and two guard bands, engine calls that hand their query back to the coalescer, mutations between rounds.  The stub's
simulated device latency makes groups form; RLR_BATCH_MIN=2 lets them qualify on a small corpus.  Pass = no
ThreadSanitizer report, no deadlock (timeout), every call returned RLR_OK, the statistics add up."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(CLANGXX)), reason="needs hipcc + clang++")
def test_coalescer_under_thread_sanitizer(tmp_path):
    csrc = os.path.join(ROOT, "rust-local-rag_amd", "csrc")
    import __graft_entry__  # (the repository root is on sys.path: tests/conftest.py)

    units = __graft_entry__._load_build_module().SOURCES  # the library's one list of translation units
    san = ["-fsanitize=thread", "-g", "-O1"]
    procs, objs = [], []
    for u in units:
        obj = str(tmp_path / (os.path.splitext(u)[0] + ".o"))
        objs.append(obj)
        cmd = [HIPCC, *(["-x", "hip"] if u.endswith(".cpp") else []), "--offload-arch=gfx950", "--offload-host-only",
               "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-option-ignored", *san,
               "-I", os.path.join(ROOT, "include"), "-c", os.path.join(csrc, u), "-o", obj]
        procs.append((u, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for u, p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, f"{u}:\n{out[-4000:]}"
    for src, extra in (("stub_hip.cpp", ["-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include"]), ("tsan_coalesce.cpp", [])):
        obj = str(tmp_path / (os.path.splitext(src)[0] + ".o"))
        objs.append(obj)
        subprocess.run([CLANGXX, "-x", "c++", "-std=c++17", *san, *extra, "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "sanitize", src), "-o", obj], check=True)
    exe = str(tmp_path / "tsan_coalesce")
    # (host-only objects name their missing device image as an undefined symbol; the stub runtime never reads it)
    subprocess.run([CLANGXX, *san, *objs, "-o", exe, "-lpthread", "-ldl", "-Wl,--unresolved-symbols=ignore-all"], check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 second_deadlock_stack=1 exitcode=66", STUB_SYNC_US="300",
               RLR_MAX_CONTEXTS="4", RLR_WAIT="block", RLR_BATCH_MIN="2")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe, "2", "20"], capture_output=True, text=True, env=env, timeout=900)
    assert "ThreadSanitizer" not in out.stderr, out.stderr[-8000:]
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    assert "tsan_coalesce ok" in out.stdout
    assert "groups 0," not in out.stdout, out.stdout[-2000:]
