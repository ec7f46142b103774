"""The C-ABI library loads on a machine without a GPU, exports every symbol include/csvgpu.h declares,
and refuses to create a context when there is no device (no silent CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "csvgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef CSV_TEST_HOOKS.*?#endif", "", text, flags=re.S)          # the test build's hook is not part of the product ABI
    return sorted(set(re.findall(r"\b(csvgpu_[a-z0-9_]+)\s*\(", text)))


def _test_hooks():
    """What the CSV_TEST_HOOKS block of the header declares."""
    text = open(os.path.join(ROOT, "include", "csvgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    block = re.search(r"#ifdef CSV_TEST_HOOKS(.*?)#endif", text, flags=re.S).group(1)
    return sorted(set(re.findall(r"\b(csvgpu_[a-z0-9_]+)\s*\(", block)))


def test_header_symbols_exported():
    from contextsv_amd import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/csvgpu.h but not exported"
    assert sorted(_lib.ABI) == names, "ctypes table and header disagree"
    assert lib.csvgpu_abi_version() == _lib.ABI_VERSION == 4
    assert not hasattr(lib, "csvgpu_test_fail_next_alloc"), "the allocation-failure hook must not be in the product library"
    hooks = _test_hooks()
    assert sorted(hooks) == sorted(["csvgpu_test_fail_next_alloc", *_lib.TEST_HOOKS]) and len(_lib.TEST_HOOKS) == 4
    for n in hooks:
        assert not hasattr(lib, n), f"{n}: a test hook must not be in the product library"
        assert n not in _lib.ABI
    assert "csvgpu_set_tuning" in names and _lib.ABI["csvgpu_set_tuning"][1][1]._type_ is _lib.csv_tuning


def test_struct_layouts_match_header():
    from contextsv_amd import _lib
    assert C.sizeof(_lib.csv_reads) == 64 and C.sizeof(_lib.csv_hmm) == 8 * (36 + 6 + 6 + 6 + 1 + 5 + 5 + 1)
    assert _lib.SIG_DTYPE.itemsize == 16 and C.sizeof(_lib.csv_chr_result) == 8 * 4 + 4 + 4 + 8 + 8 * 8
    text = open(os.path.join(ROOT, "include", "csvgpu.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct csv_tuning \{(.*?)\} csv_tuning;", text, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"int32_t\s+(\w+);", body) == [f for f, _ in _lib.csv_tuning._fields_] and C.sizeof(_lib.csv_tuning) == 4 * 5


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import contextsv_amd as cs
    with pytest.raises(cs.CsvError) as ei:
        cs.Context(0)
    assert ei.value.status == cs._lib.CSV_ENODEV
    from contextsv_amd import host
    with pytest.raises(RuntimeError):       # the host mirror's DBSCAN has no context -> loud failure, no CPU path
        host.merge_svs(host.make_calls([1, 2], [100, 101], [0, 0]), 0.1, 2, False)


# environment switches that once steered SVCaller::runResident; the run's shape is RunParams::schedule now
RETIRED_HOST_SWITCHES = ("CSV_NO_EARLY_CN", "CSV_EARLY_CN_WAIT_ALL", "CSV_EARLY_SMALL_BATCHES", "CSV_NO_SPLIT_BESIDE_PASS", "CSV_SPLIT_NO_SELF",
                         "CSV_TEST_PREPARE_DELAY_MS", "CSV_NO_EARLY_SPLIT", "CSV_NO_LATE_JOIN", "CSV_EARLY_ONE_BATCH", "CSV_SPLIT_ONE_CALL",
                         "CSV_JOBS_AHEAD")


# switches of the device library that csv_tuning (csvgpu_set_tuning) replaced or that were retired: it reads no environment variable
RETIRED_DEVICE_SWITCHES = ("CSV_SCAN_FORM", "CSV_SORT_ONESWEEP", "CSV_DBSCAN_SMALL_BRUTE", "CSV_SPLIT_TAIL", "CSV_SPLIT_SMALL", "CSV_DEPTH_WPL",
                           "CSV_SPIN_US", "CSV_BG_PRIORITY")


def test_device_library_reads_no_environment():
    csrc = os.path.join(ROOT, "contextsv_amd", "csrc")
    files = [os.path.join(d, f) for d in (csrc, os.path.join(csrc, "api"), os.path.join(csrc, "kernels")) for f in sorted(os.listdir(d))
             if f.endswith((".hip", ".hpp"))]
    assert len(files) >= 25 and os.path.join(csrc, "api", "job.hip") in files and os.path.join(csrc, "kernels", "scan.hip") in files
    for f in files:
        txt = open(f, errors="ignore").read()
        assert "getenv" not in txt and not [s for s in RETIRED_DEVICE_SWITCHES if s in txt], f


def test_product_package_does_not_touch_the_oracle():
    pkg = os.path.join(ROOT, "contextsv_amd")
    host_src = os.path.join(pkg, "csrc", "host")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hpp", ".hip")) or f == "Makefile":
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "libcsvoracle" not in txt and "oracle_lib" not in txt and "csv_oracle" not in txt, os.path.join(dp, f)
                if os.path.abspath(dp).startswith(host_src):
                    assert not [s for s in RETIRED_HOST_SWITCHES if s in txt], os.path.join(dp, f)


def test_testhooks_build_exports_the_same_abi_plus_the_hook():
    """libcsvgpu_testhooks.so (the product library's own objects, with csrc/api/testhooks.hip linked in the place of nohooks.hip; loaded only by
    tests/test_gpu_job_errors.py and tests/test_gpu_sort_primitives.py) = the product ABI + the hooks: the allocation failure and the four
    on the device primitives."""
    from contextsv_amd import _lib
    lib = C.CDLL(os.path.join(ROOT, "contextsv_amd", "lib", "libcsvgpu_testhooks.so"))
    for n in _declared():
        assert hasattr(lib, n), n
    assert hasattr(lib, "csvgpu_test_fail_next_alloc")
    for n in ("csvgpu_test_radix_sort", "csvgpu_test_radix_sort_devn", "csvgpu_test_exclusive_sum", "csvgpu_test_prefix_max"):
        assert n in _test_hooks() and n in _lib.TEST_HOOKS and hasattr(lib, n), n
    lib.csvgpu_abi_version.restype = C.c_int
    assert lib.csvgpu_abi_version() == _lib.ABI_VERSION
