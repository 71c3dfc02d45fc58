"""One owner for device memory, streams and events (DESIGN.md "Device resources"): the rule is
checked on the sources.  No translation unit outside rt_hip_util.h allocates or frees device
memory or creates or destroys a stream or an event, the error macro and the device guard exist
once, and the private copies the owners replaced stay gone."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go_raytracer_amd", "csrc")
OWNER = "rt_hip_util.h"
# the six call families, each with whatever suffix HIP gives its variants (hipMallocAsync,
# hipStreamCreateWithFlags, hipEventCreateWithFlags, hipFreeAsync, ...)
FAMILIES = ["hipMalloc", "hipFree", "hipStreamCreate", "hipStreamDestroy", "hipEventCreate", "hipEventDestroy"]


def _sources():
    paths = sorted(p for ext in ("*.hip", "*.h", "*.cpp") for p in glob.glob(os.path.join(CSRC, ext)))
    assert len(paths) > 20 and os.path.join(CSRC, OWNER) in paths
    return {os.path.basename(p): open(p, encoding="utf-8").read() for p in paths}


def test_resource_calls_only_in_the_owner_header():
    src = _sources()
    for fam in FAMILIES:  # by name, comments included
        assert re.search(rf"\b{fam}\w*\s*\(", src[OWNER]), f"{OWNER} does not call {fam}*"
        users = [name for name, text in src.items() if name != OWNER and fam in text]
        assert users == [], f"{fam}* named outside {OWNER}: {users}"


def test_one_error_macro_and_one_device_guard():
    src = _sources()
    for needle in ("#define HIP_OK", "struct DeviceGuard"):
        where = {name: text.count(needle) for name, text in src.items() if needle in text}
        assert where == {OWNER: 1}, (needle, where)


def test_private_copies_are_gone():
    src = _sources()
    for word in (r"\bB_OK\b", r"\bFreeOnExit\b", r"\bDevBuf\b", r"\bstruct\s+Scratch\b"):
        where = [name for name, text in src.items() if re.search(word, text)]
        assert where == [], (word, where)
