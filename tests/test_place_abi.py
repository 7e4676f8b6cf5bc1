"""Place recognition without a GPU: the nine entry points are declared in include/nos.h with the agreed prototypes, listed
in C_ABI_SYMBOLS and exported by libnos_hip.so; NULL arguments and parameters outside their limits are rejected before any
device is touched (and nothing is written); and — read from the gfx950 code object hipcc cross-compiled into
csrc/nos_place.o — place_descriptor_kernel and place_search_kernel are there, neither spills nor uses scratch memory, and
the descriptor kernel's bins fit 64 KB of LDS."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

NOS_ERR_INVALID_ARGUMENT = 1
SENTINEL = 12345

PROTOTYPES = {
    "nos_scan_descriptor": r"int nos_scan_descriptor\(nos_scan\* scan, const nos_place_params\* params, double\* desc_out, "
                           r"size_t\* n_used\);",
    "nos_place_db_create": r"int nos_place_db_create\(nos_ctx\* ctx, const nos_place_params\* params, size_t reserve, "
                           r"nos_place_db\*\* out_db\);",
    "nos_place_db_destroy": r"int nos_place_db_destroy\(nos_place_db\* db\);",
    "nos_place_db_size": r"size_t nos_place_db_size\(const nos_place_db\* db\);",
    "nos_place_db_add": r"int nos_place_db_add\(nos_place_db\* db, const double\* desc, size_t\* index\);",
    "nos_place_db_add_scan": r"int nos_place_db_add_scan\(nos_place_db\* db, nos_scan\* scan, size_t\* index, size_t\* n_used\);",
    "nos_place_db_get": r"int nos_place_db_get\(nos_place_db\* db, size_t index, double\* desc_out\);",
    "nos_place_db_search": r"int nos_place_db_search\(nos_place_db\* db, const double\* queries, int32_t n_queries, size_t first, "
                           r"size_t count, double\* distance_out, int32_t\* shift_out\);",
    "nos_place_db_search_scan": r"int nos_place_db_search_scan\(nos_place_db\* db, nos_scan\* scan, size_t first, size_t count, "
                                r"double\* distance_out, int32_t\* shift_out, size_t\* n_used\);",
}


def _lib():
    from nonlinear_optimizer_for_slam_amd import _lib
    return _lib, _lib.hip_lib()


def _params(n_rings=20, n_sectors=60, max_range=80.0, z_floor=-2.0):
    from nonlinear_optimizer_for_slam_amd import _lib
    return _lib.NosPlaceParams(n_rings, n_sectors, max_range, z_floor)


def test_the_entry_points_are_declared_listed_and_exported_with_their_prototypes():
    _lib_mod, lib = _lib()
    text = open(os.path.join(ROOT, "include", "nos.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    flat = re.sub(r"\s+", " ", text)
    dense = re.sub(r"\s+", "", text)  # the prototypes are compared without white space
    for name, proto in PROTOTYPES.items():
        assert name in declared, name
        assert name in _lib_mod.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name
        assert re.search(proto.replace(" ", ""), dense), name
    assert re.search(r"typedef struct nos_place_params \{ int32_t n_rings; int32_t n_sectors; double max_range; double z_floor; \} "
                     r"nos_place_params;", flat)
    assert re.search(r"typedef struct nos_place_db nos_place_db;", flat)
    assert ctypes.sizeof(_lib_mod.NosPlaceParams) == 24
    assert lib.nos_place_db_size.restype is ctypes.c_size_t


def test_null_arguments_are_rejected_without_a_device_and_write_nothing():
    _, lib = _lib()
    p = _params()
    desc = (ctypes.c_double * 1200)(*([7.0] * 1200))
    used = ctypes.c_size_t(SENTINEL)
    out = ctypes.c_void_p(SENTINEL)
    index = ctypes.c_size_t(SENTINEL)
    dist = (ctypes.c_double * 4)(*([7.0] * 4))
    shift = (ctypes.c_int32 * 4)(*([7] * 4))
    calls = [
        lambda: lib.nos_scan_descriptor(None, ctypes.byref(p), desc, ctypes.byref(used)),
        lambda: lib.nos_place_db_create(None, ctypes.byref(p), 0, ctypes.byref(out)),
        lambda: lib.nos_place_db_add(None, desc, ctypes.byref(index)),
        lambda: lib.nos_place_db_add_scan(None, None, ctypes.byref(index), ctypes.byref(used)),
        lambda: lib.nos_place_db_get(None, 0, desc),
        lambda: lib.nos_place_db_search(None, desc, 1, 0, 4, dist, shift),
        lambda: lib.nos_place_db_search_scan(None, None, 0, 4, dist, shift, ctypes.byref(used)),
    ]
    for k, call in enumerate(calls):
        assert call() == NOS_ERR_INVALID_ARGUMENT, k
        assert b"NULL" in lib.nos_last_error(), (k, lib.nos_last_error())
    assert used.value == SENTINEL and out.value == SENTINEL and index.value == SENTINEL
    assert list(desc) == [7.0] * 1200 and list(dist) == [7.0] * 4 and list(shift) == [7] * 4
    # a NULL parameter block, a NULL output
    assert lib.nos_scan_descriptor(None, None, desc, ctypes.byref(used)) == NOS_ERR_INVALID_ARGUMENT
    assert lib.nos_place_db_create(None, None, 0, ctypes.byref(out)) == NOS_ERR_INVALID_ARGUMENT
    assert lib.nos_place_db_create(None, ctypes.byref(p), 0, None) == NOS_ERR_INVALID_ARGUMENT
    assert out.value == SENTINEL
    # the two that take NULL
    assert lib.nos_place_db_destroy(None) == 0
    assert lib.nos_place_db_size(None) == 0


BAD_PARAMS = [
    (dict(n_rings=0), b"n_rings"), (dict(n_rings=65), b"n_rings"), (dict(n_rings=-1), b"n_rings"),
    (dict(n_sectors=0), b"n_sectors"), (dict(n_sectors=129), b"n_sectors"),
    (dict(max_range=0.0), b"max_range"), (dict(max_range=-1.0), b"max_range"), (dict(max_range=float("inf")), b"max_range"),
    (dict(max_range=float("nan")), b"max_range"),
    (dict(z_floor=float("nan")), b"z_floor"), (dict(z_floor=float("inf")), b"z_floor"), (dict(z_floor=float("-inf")), b"z_floor"),
]
# one inside each limit: the parameters pass, and the call goes on to reject the NULL object
GOOD_PARAMS = [dict(n_rings=1), dict(n_rings=64), dict(n_sectors=1), dict(n_sectors=128), dict(max_range=1e-300),
               dict(max_range=1e300), dict(z_floor=-1e300), dict(z_floor=1e300)]


@pytest.mark.parametrize("kw,word", BAD_PARAMS)
def test_bad_parameters_are_rejected_without_a_device(kw, word):
    _, lib = _lib()
    p = _params(**kw)
    out = ctypes.c_void_p(SENTINEL)
    desc = (ctypes.c_double * 4)(*([7.0] * 4))
    used = ctypes.c_size_t(SENTINEL)
    assert lib.nos_place_db_create(None, ctypes.byref(p), 0, ctypes.byref(out)) == NOS_ERR_INVALID_ARGUMENT
    assert word in lib.nos_last_error() and b"NULL" not in lib.nos_last_error(), lib.nos_last_error()
    assert lib.nos_scan_descriptor(None, ctypes.byref(p), desc, ctypes.byref(used)) == NOS_ERR_INVALID_ARGUMENT
    assert word in lib.nos_last_error() and b"NULL" not in lib.nos_last_error(), lib.nos_last_error()
    assert out.value == SENTINEL and used.value == SENTINEL and list(desc) == [7.0] * 4


@pytest.mark.parametrize("kw", GOOD_PARAMS)
def test_parameters_at_their_limits_pass_the_parameter_check(kw):
    _, lib = _lib()
    p = _params(**kw)
    out = ctypes.c_void_p(SENTINEL)
    assert lib.nos_place_db_create(None, ctypes.byref(p), 0, ctypes.byref(out)) == NOS_ERR_INVALID_ARGUMENT
    assert b"ctx is NULL" in lib.nos_last_error(), lib.nos_last_error()
    assert out.value == SENTINEL


def test_the_place_kernels_are_in_their_object_and_have_no_spills_and_no_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_place.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = kernel_resources.kernel_resources(obj)
    desc = [k for k in kernels if "nos::place_descriptor_kernel<" in k["name"]]
    search = [k for k in kernels if "nos::place_search_kernel<" in k["name"]]
    finish = [k for k in kernels if "nos::place_finish_kernel(" in k["name"]]
    # the descriptor kernel at 16 KB of bins (the default 20 x 60 among them) and at the 64 x 128 limit; the search with one
    # and with two shifts per lane
    assert len(desc) == 2 and len(search) == 2 and len(finish) == 1, [k["name"][:80] for k in kernels]
    for k in desc + search + finish:
        assert k["spill"] == 0 and k["scratch"] == 0, k
    assert sorted(k["lds"] for k in desc) == [2048 * 8, 64 * 128 * 8]
    assert all(k["lds"] <= 64 * 1024 for k in desc)
    # the search keeps the candidate in dynamic LDS (n_rings * n_sectors doubles, 64 KB at the limit): nothing static
    assert all(k["lds"] == 0 for k in search)
    # one wave per workgroup at <= 128 registers: the 64 KB candidate, not the registers, bounds the waves per CU
    assert all(k["vgpr"] <= 128 for k in desc + search), [(k["name"][:40], k["vgpr"]) for k in desc + search]
