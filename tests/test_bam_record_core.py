"""The per-record decisions of the device's BAM record unpacking (contextsv_amd/csrc/bam_record_core.hpp) on the CPU.
`make -C contextsv_amd/csrc unpack-check` builds tools/fuzz/bam_record_core_check.cpp — a program of its own, g++ under AddressSanitizer +
UBSan — which walks the streams of tests/bam_unpack_inputs.py and byte-mutated copies of them with the core, in heap blocks of exactly the
streams' sizes, and reads the same bytes with the host reader (BamReader, unchanged): the two must agree on accept or refuse, on the
message, and on every field of every record. The GPU tests (tests/test_gpu_bam_unpack.py) run the same streams through the kernels.
CPU only; nothing sanitized is loaded into Python."""
import os
import re
import struct
import subprocess

import bam_unpack_inputs as inp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def corpus():
    streams = [inp.alignment_stream(), inp.cg_stream()[0], inp.long_cigar_stream(40, 70_000)[0], inp.plain_stream(60), inp.filter_stream(), b""]
    streams += [s for _, s, _, _ in inp.refusal_streams()]
    return streams


def test_core_agrees_with_the_host_reader_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-s", "-C", CSRC, "unpack-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    streams = corpus()
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as f:
        f.write(b"BRC1" + struct.pack("<I", len(streams)))
        for s in streams:
            f.write(struct.pack("<I", len(s)) + s)
    n_mut = 150
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "bam_record_core_check"), path, str(tmp_path), str(n_mut)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"bam_record_core_check: (\d+) buffers, (\d+) accepted, (\d+) refused, (\d+) records, (\d+) hops, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    n_buffers, n_accepted, n_refused, n_records = (int(m.group(i)) for i in range(1, 5))
    assert n_buffers == len(streams) * (n_mut + 1)
    assert n_accepted > n_buffers // 10 and n_refused > n_buffers // 10 and n_records > 1000          # both ways out ran, on more than the intact streams
