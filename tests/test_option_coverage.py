"""Every library option is set by some test, or listed here with the reason
it is not: an option added to runtime.cpp's table without a test that sets
it fails here, without a GPU."""

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# options no test sets, each with its reason
UNTESTED = {
    "debug": "prints diagnostics on stderr only",
    "ktime": "the kernel timer itself: read by the tests that prove which variant ran",
    "alloc_skew": "host allocator placement of blocks >= 256 MiB: no kernel code",
    "alloc_contig": "host allocator placement of blocks >= 256 MiB: no kernel code",
}


def _option_table():
    with open(os.path.join(ROOT, "polaroid_amd", "csrc", "runtime.cpp")) as f:
        src = f.read()
    rows = re.findall(r'\{"(\w+)",\s*"PLGPU_(\w+)",\s*&Options::(\w+)\}', src)
    assert len(rows) >= 40, "the option table of runtime.cpp was not found"
    for name, env, field in rows:
        assert env == name.upper() and field == name, (name, env, field)
    return [name for name, _, _ in rows]


def _options_set_by_tests():
    found = set()
    tests = os.path.join(ROOT, "tests")
    for fn in sorted(os.listdir(tests)):
        if not fn.endswith(".py") or fn == os.path.basename(__file__):
            continue
        with open(os.path.join(tests, fn)) as f:
            found.update(re.findall(r'(?:plgpu_option|set_option)\(\s*"(\w+)"', f.read()))
    return found


def test_every_option_is_set_by_a_test_or_listed():
    names = _option_table()
    assert len(set(names)) == len(names)
    used = _options_set_by_tests()
    missing = [n for n in names if n not in used and n not in UNTESTED]
    assert not missing, f"options no test sets (plgpu_option / set_option) and UNTESTED does not list: {missing}"
    stale = [n for n in UNTESTED if n not in names]
    assert not stale, f"UNTESTED lists names that are not options: {stale}"
