"""CPU: the wide entries of include/hop_wide.h are exported and bound, stay out of
hop.h, and validate their arguments on the host before any launch."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_wide_header_symbols_exported_and_separate(lib):
    from time_opt_ilqr_amd import _lib
    names = _functions("hop_wide.h")
    assert names == ["hop_augment_wide_f64", "hop_lft_sweep_wide_f64", "hop_riccati_wide_f64"]
    assert sorted(_lib.WIDE_SIGNATURES) == names
    out = os.popen(f"nm -D {_lib.LIB_PATH}").read()
    narrow = _functions("hop.h")
    for n in names:
        assert hasattr(lib, n)
        assert re.search(rf"\bT {n}\b", out), n
        assert n not in narrow and n not in _lib.SIGNATURES
    assert _lib.MAX_DIM == 16 and _lib.WIDE_MAX_DIM == 32
    assert lib.hop_abi_version() == 1


def _sweep(lib, *, s=20, m=4, n_alloc=10, n_use=10, r_inv=1, t_min=0, t_max=0, null=False):
    d = C.c_void_p(16)  # never dereferenced: every call here ends on the host
    p = None if null else d
    return lib.hop_lft_sweep_wide_f64(p, p, p, p, 0, 0, r_inv, p, p, 0, 4, n_alloc, n_use, s, m, 8,
                                      t_min, t_max, p, p, p, p, None, None, None)


def test_wide_sweep_validation_without_gpu(lib):
    assert _sweep(lib, s=33) == -2 and b"s must be in [1, 32]" in lib.hop_last_error()
    assert _sweep(lib, s=0) == -2
    assert _sweep(lib, m=17) == -2 and b"m must be" in lib.hop_last_error()
    assert _sweep(lib, r_inv=0) == -1 and b"R^-1" in lib.hop_last_error()
    assert _sweep(lib, n_use=11) == -1 and b"n_use > n_alloc" in lib.hop_last_error()
    assert _sweep(lib, n_use=0, null=True) == 0  # the reference's empty J: nothing launched
    assert _sweep(lib, null=True) == -1 and b"null" in lib.hop_last_error()
    assert _sweep(lib, t_min=0, t_max=5) == -1 and b"t_min" in lib.hop_last_error()
    assert _sweep(lib, t_min=3, t_max=11) == -1
    assert _sweep(lib, t_min=6, t_max=5) == -1


def _augment(lib, *, n=20, m=4, n_alloc=10, n_build=10, wrap=0, null=False):
    d = C.c_void_p(16)
    p = None if null else d
    return lib.hop_augment_wide_f64(p, p, p, p, p, p, 0, p, 0, p, 0, p, 0, p, 0, None, None, None,
                                    wrap, 1e-9, 1e-12, 4, n_alloc, n_build, n, m, p, p, p, p, p,
                                    None)


def test_wide_augment_validation_without_gpu(lib):
    assert _augment(lib, n=32) == -2 and b"n must be in [1, 31]" in lib.hop_last_error()  # s = 33
    assert _augment(lib, n=0) == -2
    assert _augment(lib, m=17) == -2
    assert _augment(lib, n_build=11) == -1 and b"n_use > n_alloc" in lib.hop_last_error()
    assert _augment(lib, n_build=0) == 0
    assert _augment(lib, null=True) == -1 and b"null" in lib.hop_last_error()
    assert _augment(lib, n=20, wrap=1 << 20) == -1 and b"wrap_mask" in lib.hop_last_error()
    assert _augment(lib, n=31, wrap=1 << 31) == -1


def _riccati(lib, *, n=20, m=4, mode=0, wrap=0, reg=12, batch=4, null=False):
    d = C.c_void_p(16)
    p = None if null else d
    return lib.hop_riccati_wide_f64(p, p, p, p, p, 0, p, 0, p, 0, p, 0, p, 0, None, None, None, p, p,
                                    0.0, wrap, mode, reg, batch, 10, n, m, p, p, None, None, None,
                                    p, None)


def test_wide_riccati_validation_without_gpu(lib):
    assert _riccati(lib, n=32) == -2 and b"n must be in [1, 31]" in lib.hop_last_error()
    assert _riccati(lib, m=17) == -2
    assert _riccati(lib, mode=2) == -1 and b"mode" in lib.hop_last_error()
    assert _riccati(lib, reg=0) == -1
    assert _riccati(lib, wrap=1 << 20) == -1 and b"wrap_mask" in lib.hop_last_error()
    assert _riccati(lib, null=True) == -1 and b"null" in lib.hop_last_error()
    assert _riccati(lib, batch=0, null=True) == 0


def test_narrow_limits_unchanged(lib):
    """the narrow entries still reject what only the wide ones take"""
    nul = None
    rc = lib.hop_lft_sweep_f64(nul, nul, nul, nul, 0, 0, 1, nul, nul, 0, 4, 10, 10, 17, 4, 8,
                               0, 0, nul, nul, nul, nul, nul, nul, nul)
    assert rc == -2 and b"s must be in [1, 16]" in lib.hop_last_error()
