"""CPU: the two test hooks of include/hop_testhooks.h (the LDS fill and its witness scan)
are exported and bound under their own table, appear in no product header, and validate
their arguments on the host before any launch."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hop_test_lds_fill", "hop_test_lds_scan"]


@pytest.fixture(scope="module")
def lib():
    from time_opt_ilqr_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _functions(header):
    src = open(os.path.join(REPO, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|const char\*)\s+(hop_\w+)\s*\(", src,
                                 flags=re.M)))


def test_testhook_symbols_exported_and_separate(lib):
    from time_opt_ilqr_amd import _lib, build
    assert _functions("hop_testhooks.h") == NAMES
    assert sorted(_lib.TESTHOOK_SIGNATURES) == NAMES
    out = os.popen(f"nm -D {_lib.LIB_PATH}").read()
    for name in NAMES:
        assert hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), name
        for table in (_lib.SIGNATURES, _lib.WIDE_SIGNATURES, _lib.WIDE_JCURVE_SIGNATURES,
                      _lib.CHAIN_SIGNATURES, _lib.ONEPASS_SIGNATURES):
            assert name not in table
    headers = sorted(h for h in os.listdir(os.path.join(REPO, "include")) if h.endswith(".h"))
    assert "hop_testhooks.h" in headers and "hop.h" in headers
    for h in headers:  # the names (and the header's own) appear in no other header
        if h != "hop_testhooks.h":
            text = open(os.path.join(REPO, "include", h)).read()
            assert "hop_test_" not in text and "hop_testhooks" not in text, h
    assert len(_functions("hop.h")) == 40 and lib.hop_abi_version() == 1
    assert "lds_probe.hip" in build.SOURCES
    text = open(os.path.join(REPO, "include", "hop_testhooks.h")).read()
    assert "TEST SUPPORT ONLY" in text and "not part of the product interface" in text
    assert f"#define HOP_TEST_LDS_BYTES {_lib.TEST_LDS_BYTES} " in text


def _scan(lib, *, lds=48128, threads=128, groups=3, null=False):
    d = C.c_void_p(16)  # never dereferenced: every call here ends on the host
    return lib.hop_test_lds_scan(0, lds, threads, groups, None if null else d, None)


def test_testhook_validation_without_gpu(lib):
    for g in (0, -1, 17):
        assert lib.hop_test_lds_fill(0, g, None) == -1
        assert b"groups_per_cu must be in [1, 16]" in lib.hop_last_error()
    for lds in (0, -8, 4, 12, 48124, 163848):
        assert _scan(lib, lds=lds) == -1 and b"lds_bytes" in lib.hop_last_error(), lds
    for th in (0, 63, 1025):
        assert _scan(lib, threads=th) == -1 and b"threads" in lib.hop_last_error(), th
    for g in (0, -3, 1 << 31):
        assert _scan(lib, groups=g) == -1 and b"groups" in lib.hop_last_error(), g
    assert _scan(lib, null=True) == -1 and b"null" in lib.hop_last_error()
    # the order of the checks: a bad size is reported before the null pointer
    assert _scan(lib, lds=4, null=True) == -1 and b"lds_bytes" in lib.hop_last_error()
