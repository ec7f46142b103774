"""The per-region rules of a resident SNP table (contextsv_amd/csrc/snp_table_core.hpp) on the CPU. `make -C contextsv_amd/csrc
snp-table-check` builds tools/fuzz/snp_table_core_check.cpp — a program of its own, under AddressSanitizer + UBSan, linked with the host
mirror's SNPTable::queryFlat, the default SNPSource::queryFlat and SNPFileTable::query — which applies the header's rules the way
kernels/snptable.hip applies them (a table resolved once, a region as a range, the first hit per region) to the families of
tests/snp_table_inputs.py and to a few thousand random tables with a few dozen regions each, every array in a heap block of exactly its
size: positions, baf and pfb agree with the host bit for bit, NaN payloads included."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def test_core_agrees_with_the_host_sources():
    r = subprocess.run(["make", "-s", "-C", CSRC, "snp-table-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "snp_table_core_check"), "3000", "40"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"snp_table_core_check: (\d+) tables, (\d+) regions, (\d+) records, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    tables, regions, records = (int(x) for x in m.groups())
    print(r.stdout.strip())
    assert tables >= 3000 and regions >= 40 * tables and records > regions
