"""The Python statement of the FASTA loader's rules (tests/fasta_inputs.py) — what the GPU tests of the device genome compare with — held
against the host mirror's ReferenceGenome and against the oracle restatement (oracle.fasta_describe / fasta_query), on every family of
texts the GPU tests use. CPU only."""
import numpy as np
import pytest

import fasta_inputs as fi
from contextsv_amd import host


@pytest.fixture(scope="module")
def texts():
    return fi.all_texts(np.random.default_rng(5))


def _ranges(rng, length):
    edge = [(0, 0), (0, 5), (1, 0), (1, 1), (1, length), (1, length + 1), (2, 1), (length, length), (length, length + 1), (length + 1, length + 1),
            (1, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (3, 2), (5, 5)]
    rand = [tuple(int(x) for x in rng.integers(0, length + 3, 2)) for _ in range(6)]
    return edge + rand


def test_rules_agree_with_the_host_loader_and_the_oracle(texts, oracle, tmp_path):
    rng = np.random.default_rng(9)
    n_records = n_cuts = 0
    for key, text in texts.items():
        path = str(tmp_path / "t.fa")
        with open(path, "wb") as f:
            f.write(text)
        recs = fi.records(text)
        g = host.ReferenceGenome(path)
        hdr, names = oracle.fasta_describe(path)
        assert g.getChromosomes() == names == fi.chromosomes(recs), key
        assert g.getContigHeader() == hdr == fi.contig_header(recs), key
        table = fi.lookup(recs)
        n_records += len(recs)
        for name, (_, seq) in table.items():
            chr_ = name.decode("latin-1")
            assert g.getChromosomeLength(chr_) == len(seq), (key, name)
            whole = g.query(chr_, 1, len(seq)) if seq else b""
            assert whole == seq, (key, name)
            heavy = len(text) > 100_000                # (the oracle reads the file again for every query)
            for a, b in _ranges(rng, len(seq))[: 3 if heavy else None]:
                got = g.query(chr_, a, b)
                assert got == fi.cut(seq, a, b) and len(got) == fi.cut_len(len(seq), a, b), (key, name, a, b)
                if "\r" not in chr_:                   # (the same bytes either way; the oracle's path is checked where its C string holds them)
                    assert got == oracle.fasta_query(path, chr_, a, b), (key, name, a, b)
                n_cuts += 1
        g.close()
    assert n_records > 150 and n_cuts > 1500


def test_the_families_hold_what_they_promise(texts):
    recs = fi.records(texts["features"])
    names = [n for n, _ in recs]
    assert names.count(b"chrA") == 2 and b"name\rwith" in names and b"last" in names
    assert fi.lookup(recs)[b"chrA"][0] == max(i for i, n in enumerate(names) if n == b"chrA")        # the last of a name
    assert recs[0][1].startswith(b"ACGTNN\r")          # residues in front of the first header and under `> lead desc` fall to the first named one
    assert fi.records(b">x\nAA\n>\nCC\n") == [(b"x", b"AA")]                                          # no named header follows: dropped
    assert fi.records(b">x\nAA\n>\nCC\n>y\nGG\n") == [(b"x", b"AA"), (b"y", b"CCGG")]
    assert fi.records(b"AC\n>\nGT\n>z\nA\n") == [(b"z", b"ACGTA")]
    assert len(fi.records(texts["many_short"])[0][1]) == 302_000
    assert fi.cut(b"ACGTRYKMacgtrykm", 1, 16, mask=True) == b"ACGTNNNNacgtNNNN"
    assert fi.cut(b"ACGT", 0, 3) == b"" and fi.cut(b"ACGT", 2, 4) == b"CGT" and fi.cut(b"ACGT", 2, 5) == b""
