"""The copy-number observation entry points through every layer that names them (CPU only): the header declares them, libcsvgpu.so
exports them, the ctypes table lists them under ABI version 4, the host mirror exports its new hooks beside the unchanged old ones, and
the Python keywords exist and default to off."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csvgpu_cn_observations_resident_many", "csvgpu_cn_decode_resident_many")


def test_header_library_and_ctypes_table_agree():
    from contextsv_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csvgpu.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*csv_ctx \*ctx, const csv_cn_regions \*regions" % name, text), name
        assert hasattr(lib, name) and name in _lib.ABI and _lib.ABI[name][1][1]._type_ is _lib.csv_cn_regions
    assert re.search(r"#define CSVGPU_ABI_VERSION 4\b", text) and lib.csvgpu_abi_version() == _lib.ABI_VERSION == 4
    body = re.search(r"typedef struct csv_cn_regions \{(.*?)\} csv_cn_regions;", text, flags=re.S).group(1)
    fields = re.findall(r"[\*\s](\w+)\s*[,;]", body)
    assert fields == [f for f, _ in _lib.csv_cn_regions._fields_] and C.sizeof(_lib.csv_cn_regions) == 8 * 11
    assert len(_lib.ABI[NEW[0]][1]) == 9 and len(_lib.ABI[NEW[1]][1]) == 12


def test_host_library_exports_the_new_hooks_and_keeps_the_old_ones():
    from contextsv_amd import host
    lib = host.load()
    for name in ("csvhost_query_snp_regions", "csvhost_cn_prediction_device", "csvhost_query_snp_region", "csvhost_cn_prediction", "csvhost_run",
                 "csvhost_genome_run"):
        assert hasattr(lib, name), name
    assert len(lib.csvhost_query_snp_region.argtypes) == 18 and len(lib.csvhost_cn_prediction.argtypes) == 16      # the old signatures stay
    assert len(lib.csvhost_query_snp_regions.argtypes) == 21 and len(lib.csvhost_cn_prediction_device.argtypes) == 17


def test_python_keywords_exist_and_default_to_off():
    from contextsv_amd import Context, host
    assert inspect.signature(host.query_snp_regions).parameters["on_device"].default is False
    assert inspect.signature(host.cn_prediction).parameters["observations_on_device"].default is False
    assert inspect.signature(host.Genome.run).parameters["cn_observations_on_device"].default is False
    for name in ("cn_observations", "cn_decode"):
        assert callable(getattr(Context, name))
    assert inspect.signature(Context.cn_decode).parameters["want_observations"].default is False


def test_the_host_mirror_reads_no_environment_switch_for_the_option():
    src = "".join(open(os.path.join(ROOT, "contextsv_amd", "csrc", "host", f)).read() for f in ("cnv_caller.cpp", "cnv_caller.h"))
    assert "getenv" not in src and "device_observations = false" in src
    assert "cn_observations_on_device = false" in open(os.path.join(ROOT, "contextsv_amd", "csrc", "host", "sv_caller.h")).read()
