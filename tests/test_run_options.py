"""The run options of the host mirror's C ABI (contextsv_amd/csrc/host/abi/csvhost_abi.h: csvhost_run_options) through every layer (CPU only).
`make -C contextsv_amd/csrc options-check` builds tools/fuzz/run_options_check.cpp — a program of its own, g++ under AddressSanitizer + UBSan —
which holds csvhost_run_options_init and the decoder (run_params_from) against RunParams field by field. The rest runs against the built
host library: the ctypes twins have the header's fields, and Genome.run, run and run_bam, called with their own keyword defaults, hand the
library exactly the struct its init makes — the Python defaults are RunParams' defaults — while each keyword alone moves only its own
field or fields. Nothing sanitized is loaded into Python."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")
HEADER = os.path.join(CSRC, "host", "abi", "csvhost_abi.h")

C_TYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "double": C.c_double}
NP_TYPES = {"uint32_t": "<u4", "int32_t": "<i4", "uint64_t": "<u8", "int64_t": "<i8", "double": "<f8"}


def _header_struct(name):
    """[(C type, field)] of `struct <name>` in the header, in declaration order."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct %s \{(.*?)\};" % name, text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(ctype, n.strip()) for n in names.split(",")]
    return fields


def test_decoder_agrees_with_run_params_under_sanitizers():
    from contextsv_amd import host
    r = subprocess.run(["make", "-s", "-C", CSRC, "options-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "run_options_check")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"run_options_check: (\d+) fields, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) == len(host.run_options._fields_) - 1 == 24          # every field behind `size`


def test_ctypes_twins_have_the_headers_fields():
    from contextsv_amd import host
    for name, twin in (("csvhost_run_options", host.run_options), ("csvhost_chr_stats", host.chr_stats), ("csvhost_stage_times", host.stage_times),
                       ("csvhost_bam_stats", host.bam_stats)):
        declared = _header_struct(name)
        assert [(f, C_TYPES[t]) for t, f in declared] == list(twin._fields_), name
    declared = _header_struct("csvhost_call")
    assert [(f, NP_TYPES[t]) for t, f in declared] == [(f, host.CALL_DTYPE[f].str) for f in host.CALL_DTYPE.names]
    assert host.CALL_DTYPE.itemsize == 48 and [host.CALL_DTYPE.fields[f][1] for f in host.CALL_DTYPE.names] == [0, 4, 8, 12, 16, 24, 32, 36, 40, 44]
    assert _header_struct("csvhost_run_options")[0] == ("uint32_t", "size")
    text = open(HEADER).read()
    assert "#include <stdint.h>" in text and len(re.findall(r"#include", text)) == 1          # POD declarations only, nothing of the mirror


def _values(opt):
    return {f: getattr(opt, f) for f, _ in type(opt)._fields_}


@pytest.fixture(scope="module")
def init_values():
    from contextsv_amd import host
    o = host.run_options()
    host.load().csvhost_run_options_init(C.byref(o))
    return _values(o)


def test_init_writes_the_size_and_run_params_defaults(init_values):
    from contextsv_amd import host
    assert init_values["size"] == C.sizeof(host.run_options) == 112
    # (sv_caller.h's initialisers, read here as text: the library's init takes them from a default-constructed RunParams)
    src = open(os.path.join(CSRC, "host", "sv_caller.h")).read()
    for field, value in init_values.items():
        if field in ("size", "early_batches"):
            continue
        m = re.search(r"\b%s = ([\w.]+)[,;]" % field, src)
        assert m, field
        word = m.group(1)
        assert (int(word == "true") if word in ("true", "false") else float(word)) == value, field
    assert "early_batches = EarlyBatches::Timed;" in src and "enum class EarlyBatches { Timed, None, AllAtOnce, EveryThree };" in src
    assert init_values["early_batches"] == 0


class _Stop(Exception):
    pass


def _entry_points():
    """name -> (the function, a call of it that reaches the options helper without a device, the keywords it hands to the helper)."""
    from contextsv_amd import host

    class Ctx:
        h, device = None, 3

    common = ["eps", "min_pts_pct", "sample_size", "min_cnv"]
    device_forms = ["split_groups_on_device", "split_fits_on_device", "split_tables_on_device", "cn_observations_on_device"]
    genome = host.Genome()
    return {
        "Genome.run": (host.Genome.run, lambda **kw: genome.run(Ctx(), None, **kw),
                       common + ["split_svs", "cigar_cn", "merges", "host_threads", "host_split_order", "overlap_split", "early_batches", "split_beside_pass",
                                 "split_order_self", "prepare_delay_ms"] + device_forms),
        "run": (host.run, lambda **kw: host.run(Ctx(), [], None, **kw), common + ["save_cnv"]),
        "run_bam": (host.run_bam, lambda **kw: host.run_bam(Ctx(), "none.bam", None, **kw),
                    common + ["split_svs", "cigar_cn", "save_cnv", "inflate_on_device", "unpack_on_device", "shard_on_device"] + device_forms),
    }


def _options_of(monkeypatch, call, **keywords):
    """The struct the entry point builds for the library when called with `keywords` (the call ends where the struct is made)."""
    from contextsv_amd import host
    real = host._run_options
    made = []

    def spy(**kw):
        made.append(real(**kw))
        raise _Stop

    with monkeypatch.context() as m:
        m.setattr(host, "_run_options", spy)
        with pytest.raises(_Stop):
            call(**keywords)
    assert len(made) == 1
    return _values(made[0])


# keyword -> (a value that is not its default, the fields that then differ from the library's init)
FLIPS = {
    "eps": (0.25, {"dbscan_epsilon": 0.25}), "min_pts_pct": (0.3, {"dbscan_min_pts_pct": 0.3}), "sample_size": (7, {"sample_size": 7}),
    "min_cnv": (999, {"min_cnv_length": 999}), "host_threads": (5, {"host_threads": 5}),
    "split_svs": (False, {"split_svs": 0}), "cigar_cn": (False, {"cigar_cn": 0}),
    "merges": (False, {"merge_split_svs": 0, "merge_final_svs": 0}),
    "host_split_order": (True, {"split_order_on_device": 0}), "overlap_split": (False, {"overlap_split_prepare": 0}),
    "early_batches": ("every3", {"early_batches": 3}), "split_beside_pass": (False, {"split_beside_pass": 0}),
    "split_order_self": (False, {"split_order_self": 0}), "prepare_delay_ms": (40_000, {"prepare_delay_ms": 40_000}),      # (past the 15 bits it once had)
    "split_groups_on_device": (True, {"split_groups_on_device": 1}), "split_fits_on_device": (True, {"split_fits_on_device": 1}),
    "split_tables_on_device": (True, {"split_tables_on_device": 1}), "cn_observations_on_device": (True, {"cn_observations_on_device": 1}),
    "save_cnv": (True, {"save_cnv": 1}), "inflate_on_device": (True, {"inflate_on_device": 1}),
    "unpack_on_device": (True, {"unpack_on_device": 1}), "shard_on_device": (True, {"shard_on_device": 1, "unpack_on_device": 1}),
}


@pytest.mark.parametrize("name", ["Genome.run", "run", "run_bam"])
def test_python_defaults_are_the_librarys_and_each_keyword_moves_its_own_field(name, init_values, monkeypatch):
    fn, call, keywords = _entry_points()[name]
    params = inspect.signature(fn).parameters
    # what the context decides, not a keyword: run_bam's inflate_device
    expected = dict(init_values, inflate_device=3) if name == "run_bam" else init_values
    assert _options_of(monkeypatch, call) == expected
    assert _options_of(monkeypatch, call, **{k: params[k].default for k in keywords}) == expected
    # every keyword of the entry point that FLIPS knows is one the entry point hands on, and the other way round
    assert sorted(keywords) == sorted(k for k in params if k in FLIPS)
    for k in keywords:
        value, moved = FLIPS[k]
        assert value != params[k].default, k
        assert _options_of(monkeypatch, call, **{k: value}) == dict(expected, **moved), k


def test_early_batches_names_and_refused_values(monkeypatch):
    from contextsv_amd import host
    _, call, _ = _entry_points()["Genome.run"]
    for word, code in (("timed", 0), ("none", 1), ("all", 2), ("every3", 3)):
        assert _options_of(monkeypatch, call, early_batches=word)["early_batches"] == code
    with pytest.raises(ValueError):
        call(early_batches="sometimes")
    for bad in (-1, 1 << 31):
        with pytest.raises(ValueError):
            call(prepare_delay_ms=bad)
    assert _options_of(monkeypatch, call, prepare_delay_ms=(1 << 31) - 1)["prepare_delay_ms"] == (1 << 31) - 1
    with pytest.raises(TypeError):
        host._run_options(passes=7)


def test_the_library_refuses_a_struct_of_another_size():
    from contextsv_amd import _lib, host
    lib = host.load()
    o = host._run_options()
    o.size -= 4
    k = C.c_uint64(0)
    g = host.Genome()
    hmm = _lib.csv_hmm()
    assert lib.csvhost_genome_run(g.h, None, 0, None, C.byref(hmm), C.byref(o), None, None, 0, C.byref(k), None, None) == -1
    assert b"csvhost_run_options: size 108" in lib.csvhost_last_error()
    # the message belongs to the thread that failed: another thread's failure does not replace it, and is read there
    import threading
    seen = []

    def fail_elsewhere():
        o.size += 8
        rc = lib.csvhost_genome_run(g.h, None, 0, None, C.byref(hmm), C.byref(o), None, None, 0, C.byref(k), None, None)
        seen.append((rc, lib.csvhost_last_error()))

    t = threading.Thread(target=fail_elsewhere)
    t.start()
    t.join()
    assert seen[0][0] == -1 and b"size 116" in seen[0][1]
    assert b"size 108" in lib.csvhost_last_error()
    g.free()


def test_no_bitmask_is_left():
    """`passes` as an ABI argument, its bit numbers and the file the ABI was split from are named nowhere."""
    stale = re.compile(r"\bint passes\s*[,)/]|\bpasses = int\(|`passes`|\bpasses\s*(&|>>)\s*\d|bits? \d+(-\d+)? of `?csvhost|hostabi\.cpp")
    files = [os.path.join(ROOT, f) for f in ("INTEGRATION.md", "DESIGN.md", "README.md", "bench.py")]
    for top in ("contextsv_amd", "tools", "tests"):
        for dp, dn, fs in os.walk(os.path.join(ROOT, top)):
            dn[:] = [d for d in dn if d not in ("_obj", "__pycache__", "lib", "golden", "kernels")]          # (the radix sort counts passes of its own)
            files += [os.path.join(dp, f) for f in fs if f.endswith((".py", ".cpp", ".h", ".hpp", ".hip", ".md")) or f == "Makefile"]
    assert len(files) > 100 and not os.path.exists(os.path.join(CSRC, "host", "hostabi.cpp"))
    for f in files:
        if os.path.abspath(f) != os.path.abspath(__file__):
            assert not stale.search(open(f, errors="ignore").read()), f
