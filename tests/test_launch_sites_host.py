"""Every kernel launch of the library goes through svin::launch (svin_amd/csrc/kernels.hpp), which grants dynamic LDS and throws
on a refused launch.  This scan pins that on the CPU: outside the helper and ensureDynamicLds no source file launches a kernel
itself, sets a function attribute or reads the sticky hipGetLastError(), and the throw-on-error macro HIP_OK is defined once."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svin_amd", "csrc")

# (file, first line of a definition whose body may use the calls below)
ALLOWED = [("kernels.hpp", "void launch(void (*kernel)(P...)"),
           ("kernels.hip", "void ensureDynamicLds(const void* fn, size_t bytes)")]
FORBIDDEN = ["hipLaunchKernelGGL", "<<<", "hipFuncSetAttribute", "hipGetLastError"]


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def drop_body(text, head):
    """`text` with the brace-delimited body of the definition that starts with `head` blanked (line numbers kept)"""
    start = text.index(head)
    i = text.index("{", start)
    depth = 0
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[:i] + re.sub(r"[^\n]", " ", text[i:j + 1]) + text[j + 1:]
    raise AssertionError("unbalanced braces after %r" % head)


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")) +
                   glob.glob(os.path.join(CSRC, "*.hpp")))
    assert len(files) > 10, "no library sources under %s" % CSRC
    for path in files:
        with open(path) as f:
            text = strip_comments(f.read())
        for name, head in ALLOWED:
            if os.path.basename(path) == name:
                assert head in text, "%s no longer defines %r" % (name, head)
                text = drop_body(text, head)
        yield os.path.basename(path), text


def test_no_launch_or_error_state_outside_the_helper():
    found = []
    for name, text in sources():
        for no, line in enumerate(text.split("\n"), 1):
            found += ["%s:%d: %s" % (name, no, line.strip()) for word in FORBIDDEN if word in line]
    assert not found, "launch, attribute or sticky-error call outside svin::launch / ensureDynamicLds:\n" + "\n".join(found)


def test_one_throw_on_error_macro():
    defs = ["%s: %s" % (name, m.group(0)) for name, text in sources()
            for m in re.finditer(r"#\s*define\s+\w*HIP\w*_OK\b", text)]
    assert defs == ["kernels.hpp: #define HIP_OK"], defs
