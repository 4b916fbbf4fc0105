"""CPU: the wide brute-force J curve of include/hop_wide_jcurve.h is exported and bound
in a table of its own, stays out of hop.h and hop_wide.h, and validates its arguments
on the host before any launch."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hop_bruteforce_jcurve_wide_f64"


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


def test_wide_jcurve_header_symbol_exported_and_separate(lib):
    from time_opt_ilqr_amd import _lib
    names = _functions("hop_wide_jcurve.h")
    assert names == [NAME]
    assert sorted(_lib.WIDE_JCURVE_SIGNATURES) == names
    out = os.popen(f"nm -D {_lib.LIB_PATH}").read()
    assert hasattr(lib, NAME)
    assert re.search(rf"\bT {NAME}\b", out)
    assert NAME not in _functions("hop.h") and NAME not in _functions("hop_wide.h")
    assert NAME not in _lib.SIGNATURES and NAME not in _lib.WIDE_SIGNATURES
    # the entry takes hop_bruteforce_jcurve_f64's argument list
    assert _lib.WIDE_JCURVE_SIGNATURES[NAME] == _lib.SIGNATURES["hop_bruteforce_jcurve_f64"]
    assert lib.hop_abi_version() == 1


def test_wide_jcurve_header_is_in_the_build_digest():
    from time_opt_ilqr_amd import build
    import inspect
    assert "hop_wide_jcurve.h" in inspect.getsource(build._digest)
    assert "riccati_wide.hip" in build.SOURCES  # the entry's source file


def _jc(lib, *, n=20, m=4, n_alloc=10, t_max=10, wrap=0, batch=4, null=False, strides=(0,) * 5):
    d = C.c_void_p(16)  # never dereferenced: every call here ends on the host
    p = None if null else d
    s = strides
    return lib.hop_bruteforce_jcurve_wide_f64(p, p, p, p, p, s[0], p, s[1], p, s[2], p, s[3], p,
                                              s[4], None, None, None, 1e-6, 0.0, wrap, batch,
                                              n_alloc, n, m, t_max, p, p, None)


def test_wide_jcurve_validation_without_gpu(lib):
    err = lib.hop_last_error
    assert _jc(lib, batch=-1) == -1 and b"batch < 0" in err()
    assert _jc(lib, n=32) == -2 and b"n must be in [1, 31]" in err()
    assert _jc(lib, n=0) == -2 and b"n must be in [1, 31]" in err()
    assert _jc(lib, m=17) == -2 and b"m must be in [1, 16]" in err()
    assert _jc(lib, m=0) == -2
    assert _jc(lib, t_max=0) == -1 and b"t_max < 1" in err()
    assert _jc(lib, t_max=11) == -1 and b"t_max > n_alloc" in err()  # the reference's IndexError
    assert _jc(lib, wrap=1 << 20) == -1 and b"wrap_mask" in err()
    assert _jc(lib, n=31, wrap=1 << 31) == -1 and b"wrap_mask" in err()
    for i in range(5):
        s = [0] * 5
        s[i] = -1
        assert _jc(lib, strides=tuple(s)) == -1 and b"negative stride" in err(), i
    assert _jc(lib, null=True) == -1 and b"null pointer" in err()
    # batch * t_max waves beyond one grid (the dispatch limit is 2^32 work-items)
    assert _jc(lib, batch=1 << 40) == -2 and b"too large" in err()
    assert _jc(lib, batch=(1 << 26) // 10 + 1) == -2 and b"too large" in err()
    assert _jc(lib, batch=1 << 62, t_max=1, n_alloc=1) == -2  # no overflow in the product
    # an empty batch (an empty shard) launches nothing, with or without pointers
    assert _jc(lib, batch=0, null=True) == 0
    assert _jc(lib, batch=0) == 0
    # ... but its shape arguments are still checked
    assert _jc(lib, batch=0, n=32) == -2


def test_narrow_jcurve_limit_unchanged(lib):
    """hop_bruteforce_jcurve_f64 still rejects what only the wide entry takes"""
    nul = None
    rc = lib.hop_bruteforce_jcurve_f64(*([nul] * 4), nul, 0, nul, 0, nul, 0, nul, 0, nul, 0, nul,
                                       nul, nul, 1e-6, 0.0, 0, 3, 10, 17, 4, 10, nul, nul, nul)
    assert rc == -2 and b"n must be in [1, 16]" in lib.hop_last_error()
