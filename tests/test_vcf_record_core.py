"""The per-line decisions of the device VCF parser (contextsv_amd/csrc/vcf_record_core.hpp) on the CPU. `make -C contextsv_amd/csrc
vcf-check` builds tools/fuzz/vcf_record_core_check.cpp — a program of its own, under AddressSanitizer + UBSan, linked with the host reader —
which runs every line of the texts of tests/vcf_parse_inputs.py and of byte-mutated copies of them (tabs, digits, ':', ',', ';', '.', 'e',
'-', NUL; every text in a heap block of exactly its size) through the core and through the host reader's two functions: KEEP, SKIP and STOP
agree field for field, and a line is deferred only where the rule allows it."""
import os
import re
import struct
import subprocess

import numpy as np

import vcf_parse_inputs as inp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def _blob(b):
    return struct.pack("<I", len(b)) + b


def _corpus():
    text, snps, rng = inp.generated_snp_text()
    texts = []
    deliberate = ("\n".join([l for _, l in inp.DELIBERATE_SNP] + inp.NOT_DEFERRED_SNP + [inp.DEFERRED_BY_ORDER]) + "\n").encode()
    for t in (text[:30_000], deliberate * 40, text[30_000:50_000].replace(b"\n", b"\r\n"), b"\n\n" + text[50_000:50_700].rstrip(b"\n")):
        texts.append(struct.pack("<I", 0) + _blob(t))
    for c in ("chr1", "chr2"):
        gt, _ = inp.generated_gnomad_text(rng, snps, c)
        pos = np.sort(np.array([q for q, l in snps if l.startswith(c + "\t")], np.uint32))
        for needle in (b"AF_nfe=", b"AF="):
            texts.append(struct.pack("<I", 1) + _blob(gt[:12_000]) + _blob(c.encode()) + _blob(needle) + struct.pack("<I", len(pos)) + pos.tobytes())
    gd = ("\n".join(l for _, l in inp.DELIBERATE_AF) + "\n").encode() * 30
    pos = np.array(inp.DELIBERATE_AF_POS, np.uint32)
    texts.append(struct.pack("<I", 1) + _blob(gd) + _blob(b"chr1") + _blob(b"AF_nfe=") + struct.pack("<I", len(pos)) + pos.tobytes())
    texts.append(struct.pack("<I", 1) + _blob(gd) + _blob(b"chr1") + _blob(b"AF_nfe=") + struct.pack("<I", 0))          # no position at all
    return b"VCFC" + struct.pack("<I", len(texts)) + b"".join(texts), len(texts)


def test_core_agrees_with_the_host_reader(tmp_path):
    r = subprocess.run(["make", "-s", "-C", CSRC, "vcf-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    blob, n_texts = _corpus()
    path = tmp_path / "corpus.bin"
    path.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "vcf_record_core_check"), str(path), "120", "7"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"vcf_record_core_check: (\d+) texts, (\d+) kept, (\d+) skipped, (\d+) deferred, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    texts, kept, skipped, deferred = (int(x) for x in m.groups())
    lines = kept + skipped + deferred
    print(r.stdout.strip())
    assert texts == n_texts and lines > 100_000
    assert min(kept, skipped, deferred) > lines / 10, (kept, skipped, deferred)
