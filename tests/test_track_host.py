"""The counted front for device resources (csrc/ek_track.h) without a GPU: the two
exports answer, a context that cannot be created leaves nothing behind, and no source
of csrc/ calls the HIP runtime for memory, streams or events except ek_track.hip."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "enspara_amd", "csrc")

RAW = ["hipMalloc", "hipExtMallocWithFlags", "hipMallocAsync", "hipMallocManaged",
       "hipMallocPitch", "hipMalloc3D", "hipFree", "hipFreeAsync",
       "hipHostMalloc", "hipHostAlloc", "hipMallocHost", "hipHostFree", "hipFreeHost",
       "hipHostRegister", "hipHostUnregister",
       "hipStreamCreate", "hipStreamCreateWithFlags", "hipStreamCreateWithPriority",
       "hipStreamDestroy",
       "hipEventCreate", "hipEventCreateWithFlags", "hipEventDestroy"]


def _code(text):
    """the source without its comments (they may speak of the runtime's own calls: what
    was measured about hipFree stays said about hipFree)"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_raw_resource_calls_only_in_the_tracker():
    pat = re.compile(r"\b(%s)\b" % "|".join(RAW))
    seen = set()
    for name in sorted(os.listdir(CSRC)):
        found = set(pat.findall(_code(open(os.path.join(CSRC, name)).read())))
        if name == "ek_track.hip":
            seen = found
        else:
            assert not found, "%s names %s: use the wrappers of ek_track.h" % (
                name, sorted(found))
    # the tracker does wrap what the library uses
    assert {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipStreamCreateWithFlags",
            "hipStreamDestroy", "hipEventCreate", "hipEventDestroy"} <= seen


def test_tracker_is_built_and_declared():
    from enspara_amd import _lib, build
    assert "ek_track.hip" in build.SOURCES
    assert {"ek_live_resources", "ek_fail_alloc_at"} <= set(_lib.SYMBOLS)
    assert _lib.load().ek_abi_version() == 1


def test_live_resources_and_the_arm_answer_without_a_device():
    from enspara_amd import _lib
    L = _lib.load()
    assert L.ek_live_resources(None) == _lib.EK_EARG
    r = _lib.live_resources()
    assert r._fields == ("dev_allocs", "dev_bytes", "pinned_allocs", "pinned_bytes",
                         "streams", "events", "dev_allocs_total")
    assert all(isinstance(v, int) and v >= 0 for v in r)
    # arming and disarming: the previous arm comes back, a negative k disarms
    assert _lib.fail_alloc_at(-1) == -1
    assert _lib.fail_alloc_at(5) == -1
    assert _lib.fail_alloc_at(2) == 5
    assert _lib.fail_alloc_at(-7) == 2
    assert _lib.fail_alloc_at(-1) == -1
    assert _lib.live_resources() == r


def test_a_context_that_cannot_be_created_leaves_nothing():
    from enspara_amd import _lib
    L = _lib.load()
    if L.ek_device_count() > 0:
        # with a device: what a context takes, it gives back
        before = _lib.live_resources()
        h = ctypes.c_void_p()
        assert L.ek_ctx_create(0, 10, 4, 0, None, ctypes.byref(h)) == _lib.EK_OK
        during = _lib.live_resources()
        assert during.dev_allocs > before.dev_allocs and during.streams == before.streams + 1
        assert L.ek_ctx_destroy(h) == _lib.EK_OK
        assert _lib.live_resources()[:6] == before[:6]
        return
    assert tuple(_lib.live_resources()) == (0,) * 7
    h = ctypes.c_void_p()
    assert L.ek_ctx_create(0, 10, 4, 0, None, ctypes.byref(h)) == _lib.EK_EHIP
    assert not h.value
    assert tuple(_lib.live_resources()) == (0,) * 7
    # an armed failure changes nothing where no allocation is reached
    assert _lib.fail_alloc_at(0) == -1
    assert L.ek_ctx_create(0, 10, 4, 0, None, ctypes.byref(h)) == _lib.EK_EHIP
    assert _lib.fail_alloc_at(-1) == 0
    assert tuple(_lib.live_resources()) == (0,) * 7
