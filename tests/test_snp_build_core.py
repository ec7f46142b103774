"""The rules of the SNP table builder (contextsv_amd/csrc/snp_build_core.hpp) on the CPU. `make -C contextsv_amd/csrc snp-build-check`
builds tools/fuzz/snp_build_core_check.cpp — a program of its own, under AddressSanitizer + UBSan, linked with the host reader, no
sanitizer runtime preloaded anywhere — which runs the run rule and the key packing at their edges and a literal restatement of the
builder's append + finish (three batches out of order, each in a heap block of exactly its size; deferred lines and declined batches
through the host's line function) over the texts of tests/snp_build_inputs.py and byte-mutated copies of them: every contig's columns are
the table SNPFile::load builds from the same bytes in a file."""
import os
import re
import struct
import subprocess

import snp_build_inputs as sb
import vcf_parse_inputs as inp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def _blob(b):
    return struct.pack("<I", len(b)) + b


def _corpus():
    text, _, _ = sb.generated()
    lines = text.split(b"\n")[:-1]
    texts = [text[:40_000], text[40_000:].replace(b"\n", b"\r\n")]
    mixed = list(lines[:600])
    for k, (_, l) in enumerate(inp.DELIBERATE_SNP * 6):                       # deferred lines among the kept ones, of two contigs
        mixed.insert(11 * (k + 1), l.encode().replace(b"chr1", (b"chr1", b"chr7")[k & 1], 1))
    texts.append(sb.body(mixed))
    for _, names in sb.NAME_FAMILIES:
        texts.append(sb.name_text(names, per=3) + sb.name_text(names[::-1], per=2, start=500))
    texts.append(sb.body([sb.good(10 + k, ("chr1", "chr2")[k & 1]) for k in range(300)]))                         # every record its own run
    texts.append(sb.body([sb.good(5), sb.good(9), sb.good(8), sb.deferred(7), sb.good(3, "chr2")], last=False))   # a descent, no last line end
    texts.append(sb.body([sb.good(5)] * 40 + [b"#a comment behind data"] + [sb.good(6, "chr2")] * 40 + [sb.deferred(7)] * 3 + [sb.good(8)] * 40))
    texts.append(sb.body([sb.deferred(5 + k, ("chr1", "chr7")[k & 1]) for k in range(60)]))                       # nothing but deferred lines
    texts.append(b"")
    return b"SNPB" + _blob(inp.HEADER.encode()) + struct.pack("<I", len(texts)) + b"".join(_blob(t) for t in texts), len(texts)


def test_builder_rules_agree_with_the_host_loader(tmp_path):
    r = subprocess.run(["make", "-s", "-C", CSRC, "snp-build-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    blob, n_texts = _corpus()
    path = tmp_path / "corpus.bin"
    path.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "snp_build_core_check"), str(path), "40", "7", str(tmp_path / "scratch.vcf")], capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"snp_build_core_check: (\d+) texts, (\d+) records, (\d+) runs, (\d+) host records, (\d+) declined batches, (\d+) contigs, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    texts, records, runs, host_records, declined, contigs = (int(x) for x in m.groups())
    print(r.stdout.strip())
    assert texts == n_texts and records > 50_000 and runs > 5_000 and contigs > 1_000
    assert 500 < host_records < records / 2 and declined >= 20
