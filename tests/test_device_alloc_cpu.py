"""Every device block libdcs owns goes through one allocator (CPU-only source scan).

The guard-band harness (tests/test_gpu_guard.py) sees only the device memory that libdcs allocates through
``dcs_dev_alloc`` (weights, packed copies, plan tables, ramps) or ``DcsBuffer`` (scratch): those get red zones and a
poisoned payload under DCS_WS_GUARD.  A bare hipMalloc would hand a kernel a buffer the harness does not watch, so
``hipMalloc(`` / ``hipFree(`` (and their variants) may appear only inside those two in csrc/api.hip."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepconvsep_amd", "csrc")

# device allocation / release calls of the HIP runtime (pinned host memory, hipHostMalloc / hipHostFree, is not meant)
_CALL = re.compile(r"\bhip(?:Ext)?(?:Malloc|Free)\w*\s*\(")
# the functions that may call them, all in api.hip
_ALLOWED = ("hipError_t dcs_dev_alloc(", "void dcs_dev_free(", "int DcsBuffer::ensure(", "void DcsBuffer::release(")


_NOT_CODE = re.compile(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', re.S)


def _strip(src):
    """the source with comments and string / character literals blanked (offsets kept)"""
    return _NOT_CODE.sub(lambda m: re.sub(r"[^\n]", " ", m.group(0)), src)


def _code(path):
    with open(path) as fh:
        return _strip(fh.read())


def _body(code, signature):
    """[start, end) of the braces of the function defined by `signature`"""
    i = code.index(signature)
    start = code.index("{", i)
    depth = 0
    for j in range(start, len(code)):
        depth += {"{": 1, "}": -1}.get(code[j], 0)
        if depth == 0:
            return start, j + 1
    raise AssertionError("unbalanced braces after %r" % signature)


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) >= 20, files
    return files


def test_hipmalloc_and_hipfree_only_in_the_allocator_and_dcsbuffer():
    stray = []
    for path in _sources():
        code = _code(path)
        spans = []
        if os.path.basename(path) == "api.hip":
            for sig in _ALLOWED:
                s, e = _body(code, sig)
                assert _CALL.search(code, s, e), "%s no longer calls the HIP runtime: is the scan still right?" % sig
                spans.append((s, e))
        for m in _CALL.finditer(code):
            if not any(s <= m.start() < e for s, e in spans):
                line = code.count("\n", 0, m.start()) + 1
                stray.append("%s:%d: %s" % (os.path.relpath(path, ROOT), line, m.group(0)))
    assert not stray, "device memory outside dcs_dev_alloc / dcs_dev_free / DcsBuffer:\n" + "\n".join(stray)


def test_the_scan_sees_a_bare_allocation():
    planted = 'int f() { hipMalloc((void**)&p, 4); hipFreeAsync(p, 0); hipHostMalloc(&q, 4, 0); }  // hipMalloc(\nputs("hipFree(");'
    assert [m.group(0) for m in _CALL.finditer(_strip(planted))] == ["hipMalloc(", "hipFreeAsync("]


def test_owned_device_blocks_go_through_the_allocator():
    """the model, generic-graph and plan code allocate and free through the pair"""
    for name in ("net.hip", "generic.hip", "api.hip"):
        code = _code(os.path.join(CSRC, name))
        assert "dcs_dev_alloc(" in code and "dcs_dev_free(" in code, name
