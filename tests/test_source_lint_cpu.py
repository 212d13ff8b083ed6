"""Source-level guards for three classes of defect the GPU fuzzers have found or would not find reliably:
* device memory the library allocates must come from rlr::dev_malloc, so that RLR_POISON_ALLOC=1 covers every buffer;
* device and pinned memory is owned by a DevBuf / PinBuf (csrc/device_buffer.h), so that no early return can leak it and
  no destructor's list can fall behind the members;
* a null-stream fill / device-to-device copy of device memory may return before it has run and is NOT ordered
  against the non-blocking streams searches run on (the histogram defect of round 1), so each one must be followed
  by an explicit wait before the function goes on, or be issued Async on the consumer's own stream.
And one for a class of code no test would run: an environment switch that nothing sets (the last test)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = sorted(glob.glob(os.path.join(ROOT, "rust-local-rag_amd", "csrc", "*.hip")) +
                 glob.glob(os.path.join(ROOT, "rust-local-rag_amd", "csrc", "*.cpp")) +
                 glob.glob(os.path.join(ROOT, "rust-local-rag_amd", "csrc", "*.h")))


def _lines(path):
    with open(path) as f:
        return f.read().split("\n")


def test_every_device_allocation_goes_through_dev_malloc():
    assert SOURCES
    bare = []
    for path in SOURCES:
        for i, line in enumerate(_lines(path), 1):
            code = line.split("//")[0]
            if re.search(r"(?<![A-Za-z_])hipMalloc\(", code):
                bare.append((os.path.basename(path), i))
    # the one call inside rlr::dev_malloc itself
    assert len(bare) == 1 and bare[0][0] == "index.hip", bare


# (file, enclosing function) -> why that function frees or pins memory by hand.  An entry must not be a function that
# itself allocates what it frees (a scoped temporary is a local DevBuf / PinBuf).  Empty: every buffer has an owner.
HAND_MANAGED = {}


def _enclosing_function(lines, i):
    """Name of the function whose body holds line i: the nearest line above that starts in column 0 and opens a
    parameter list (csrc/ puts every function's name there and its opening brace on the next line).  A heuristic: a
    macro or a file-scope initialiser above the hit would be taken for the function.  That cannot pass a hit while
    HAND_MANAGED is empty (any name fails); check the first entry that is ever added against the source by hand."""
    for j in range(i, -1, -1):
        m = re.match(r"[A-Za-z_].*?([A-Za-z_][A-Za-z0-9_]*)\(", lines[j])
        if m and not lines[j].startswith(("namespace", "extern", "struct", "class", "template", "constexpr", "static_assert")):
            return m.group(1)
    return ""


def test_device_and_pinned_memory_is_freed_only_by_its_owner_types():
    found, used = [], set()
    for path in SOURCES:
        name = os.path.basename(path)
        if name == "device_buffer.h":
            continue
        lines = _lines(path)
        for i, line in enumerate(lines):
            if re.search(r"(?<![A-Za-z_])(hipFree|hipHostFree|hipHostMalloc)\(", line.split("//")[0]):
                key = (name, _enclosing_function(lines, i))
                used.add(key)
                if key not in HAND_MANAGED:
                    found.append((name, i + 1, key[1]))
    assert not found, found
    assert used == set(HAND_MANAGED), f"stale allow-list entries: {sorted(set(HAND_MANAGED) - used)}"
    with open(os.path.join(ROOT, "rust-local-rag_amd", "csrc", "device_buffer.h")) as f:
        owner = f.read()
    assert "hipFree(" in owner and "hipHostFree(" in owner and "hipHostMalloc(" in owner


def test_null_stream_fills_and_device_copies_are_followed_by_a_wait():
    waits = ("hipStreamSynchronize(nullptr)", "hipDeviceSynchronize()", "hipMemcpyDeviceToHost", "hipMemcpyHostToDevice")
    loose = []
    for path in SOURCES:
        lines = _lines(path)
        for i, line in enumerate(lines):
            code = line.split("//")[0]
            fill = re.search(r"(?<![A-Za-z_])hipMemset\(", code)
            d2d = re.search(r"(?<![A-Za-z_])hipMemcpy\(", code) and "hipMemcpyDeviceToDevice" in " ".join(lines[i:i + 3])
            if not (fill or d2d):
                continue
            # a wait (or a synchronous host copy on the same null stream) within the next few statements
            window = " ".join(l.split("//")[0] for l in lines[i + 1:i + 9])
            if not any(w in window for w in waits):
                loose.append((os.path.basename(path), i + 1, code.strip()))
    assert not loose, loose


# launch-shape overrides: each parametrises one kernel rather than selecting a second implementation, and the sweep
# scripts under scratch/ depend on them
LAUNCH_SHAPE_OVERRIDES = {"RLR_SCAN_VARIANT", "RLR_SCAN_IMAGE_VARIANT", "RLR_Q8_VARIANT", "RLR_SCAN_MULTI_VARIANT"}


def test_every_environment_switch_is_documented_and_exercised():
    """An environment switch is a second code path.  One stays in the library only while something runs it: a test,
    bench.py, a tool -- or it is one of the launch-shape overrides above.  Every quoted "RLR_..." literal in csrc/ is a
    name handed to getenv, directly or through a helper (the RLR_ macros and enumerators are never quoted)."""
    switches = set()
    for path in SOURCES + sorted(glob.glob(os.path.join(ROOT, "rust-local-rag_amd", "csrc", "*.h"))):
        for line in _lines(path):
            switches.update(re.findall(r'"(RLR_[A-Z0-9_]+)"', line.split("//")[0]))
    assert switches, "no getenv names found: the pattern above no longer matches how csrc/ reads its switches"
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        documented = set(re.findall(r"RLR_[A-Z0-9_]+", f.read()))
    users = [p for p in glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True)
             if os.path.abspath(p) != os.path.abspath(__file__)]
    users += [os.path.join(ROOT, "bench.py")] + glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True)
    exercised = set()
    for p in users:
        with open(p) as f:
            exercised.update(re.findall(r"RLR_[A-Z0-9_]+", f.read()))
    undocumented = sorted(switches - documented)
    unexercised = sorted(switches - exercised - LAUNCH_SHAPE_OVERRIDES)
    assert not undocumented, f"not in INTEGRATION.md: {undocumented}"
    assert not unexercised, f"set or read by no test, bench.py or tool: {unexercised}"
