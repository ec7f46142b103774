"""The rules of the device's FASTA loader (contextsv_amd/csrc/fasta_core.hpp) on the CPU. `make -C contextsv_amd/csrc fasta-check` builds
tools/fuzz/fasta_core_check.cpp — a program of its own, under AddressSanitizer + UBSan, linked with the host loader — which runs the texts of
tests/fasta_inputs.py and byte-mutated copies of them (line ends, '>', blanks, '\\r', NUL put in; a byte dropped or doubled; every text and
every piece in a heap block of exactly its size) through the core and through ReferenceGenome::setFilepath / ::query: names, lengths and
sequences agree, cuts agree, and the core fed in two pieces cut at every offset and in three pieces equals the core fed whole. Three pieces:
every pair of offsets for a text of up to 320 bytes (the 300-byte feature text among them) and for a mutated copy of up to 48 bytes, 200
random pairs beyond that. Every piecewise build runs twice: through the sequential walk, and through the device's route — each line slot of
a piece decided on its own as kernels/fasta.hip decides it, the header slots as events into fastacore::apply_piece, which is the function
csvgpu_genome_builder_append runs on the device's events."""
import os
import re
import struct
import subprocess

import numpy as np

import fasta_inputs as fi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def _corpus():
    rng = np.random.default_rng(5)
    texts = fi.small_texts() + fi.header_texts() + [fi.feature_text(), fi.wrapped_text(rng, contigs=(("c1", 700), ("c2 d", 0), ("c3", 333)), width=60)]
    tiles = fi.tile_texts(rng)
    texts += [tiles["lengths0-70"], tiles["edge-1"][:4200]]
    return b"FAST" + struct.pack("<I", len(texts)) + b"".join(struct.pack("<I", len(t)) + t for t in texts), len(texts)


def test_core_agrees_with_the_host_loader(tmp_path):
    r = subprocess.run(["make", "-s", "-C", CSRC, "fasta-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    blob, n_texts = _corpus()
    path = tmp_path / "corpus.bin"
    path.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "fasta_core_check"), str(path), "12", "7", str(tmp_path / "scratch.fa")], capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"fasta_core_check: (\d+) texts, (\d+) records, (\d+) cuts, (\d+) builds, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    texts, records, cuts, builds = (int(x) for x in m.groups())
    print(r.stdout.strip())
    # (every text and its 12 copies; most texts hold a record; 29 cuts per name; a build per offset and more)
    assert texts >= n_texts * 12 and records > texts // 2 and cuts > 20 * records // 2 and builds > 100 * texts
