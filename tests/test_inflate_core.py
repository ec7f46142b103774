"""The sequential core of the device inflate (contextsv_amd/csrc/inflate_core.hpp) on the CPU. `make -C contextsv_amd/csrc inflate-check`
builds tools/fuzz/inflate_core_check.cpp — a program of its own, g++ under AddressSanitizer + UBSan — which decodes the corpus of
tests/inflate_inputs.py with the core and a plain copy loop, in heap blocks of exactly the announced sizes: every zlib-made and hand-built
stream must decode (none declined), equal zlib's bytes and CRC-32, and be declined with the output size one less or one more; every
damaged or truncated stream is declined or decodes to the original bytes; no sanitizer report. The GPU tests
(tests/test_gpu_bgzf_inflate.py) run the same inputs through the kernel. CPU only; nothing sanitized is loaded into Python."""
import os
import re
import subprocess

import inflate_inputs as inp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def test_core_decodes_the_corpus_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-s", "-C", CSRC, "inflate-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    corpus = str(tmp_path / "corpus.bin")
    n_intact, n_damaged = inp.write_corpus(corpus)
    assert n_intact > 1900 and n_damaged >= 300
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "inflate_core_check"), corpus], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"inflate_core_check: (\d+) intact, (\d+) damaged \((\d+) declined\), (\d+) tokens, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    assert (int(m.group(1)), int(m.group(2))) == (n_intact, n_damaged)
    assert int(m.group(3)) > 0                                 # the decline path ran


def test_helper_streams_cover_what_they_claim():
    """the hand-built corners are what their names say (zlib decodes every one of them: checked where they are built)"""
    edges = {c.name: c for c in inp.edge_cases()}
    assert len(edges["len 258 dist 32768 at the end"].data) == 32768 + 258
    assert edges["EOF member"].comp == b"\x03\x00" and len(edges["out_len 65536"].data) == 65536
    # Fibonacci frequencies: a Huffman tree that is one long chain, which zlib cuts at its 15-bit limit
    from collections import Counter
    fib = Counter(inp.fibonacci_data())
    assert len(fib) >= 20 and max(fib.values()) > 10_000 and min(fib.values()) == 1
    assert len(inp.overlap_cases()) == 70 * 4 and len(inp.crc_cases()) == 307 and len(inp.zlib_cases()) == 54 * 25
