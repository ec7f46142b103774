"""host.ReferenceGenome with the sequences on the device (load_on_device=True: ReferenceGenome::setFilepath with FastaDeviceOptions,
csvgpu_genome_builder_* / csvgpu_genome_fetch underneath) against the host backing: every accessor, query and compare, output.vcf through
save_vcf (byte for byte, also against the oracle) and through run_bam, and the counters that show the device did the work."""
import numpy as np
import pytest

import contextsv_amd as cs
import fasta_inputs as fi
from contextsv_amd import host, make_hmm
from contextsv_amd.host import CALL_DTYPE
from test_vcf_writer import DATE, random_calls, write_fasta, write_gaps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gctx():
    """the genome's own context: its fetches never share a stream with a run"""
    c = cs.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("fa") / "genome.fa")
    return path, write_fasta(path, np.random.default_rng(11))


def _ranges(rng, L):
    edge = [(0, 0), (0, 5), (1, 0), (1, 1), (1, L), (1, L + 1), (2, 1), (L, L), (L, L + 1), (L + 1, L + 1), (1, 0xFFFFFFFF), (5, 5), (3, 40)]
    return edge + [tuple(int(x) for x in rng.integers(0, L + 3, 2)) for _ in range(25)]


@pytest.mark.parametrize("window_bytes", [64, 4096, 0])
def test_accessors_query_and_compare(gctx, fasta, window_bytes):
    path, contigs = fasta
    off = host.ReferenceGenome(path)
    on = host.ReferenceGenome(path, load_on_device=True, ctx=gctx, window_bytes=window_bytes)
    st = on.device_stats
    text = open(path, "rb").read()
    recs = fi.records(text)
    assert st["on_device"] == 1 and st["fallback"] == 0 and st["bytes_uploaded"] == len(text) and st["fetch_calls"] == 0
    assert st["records"] == len(recs) == 5 and st["bases"] == sum(len(s) for _, s in recs) and st["lines"] == text.count(b"\n")
    assert off.device_stats["on_device"] == 0 and off.device_stats["bytes_uploaded"] == 0
    assert on.getChromosomes() == off.getChromosomes() and on.getContigHeader() == off.getContigHeader() and on.path == off.path
    rng = np.random.default_rng(4)
    n_q = 0
    for name, s in contigs.items():
        L = len(s)
        assert on.getChromosomeLength(name) == off.getChromosomeLength(name) == L
        for a, b in _ranges(rng, L):
            want = off.query(name, a, b)
            assert on.query(name, a, b) == want, (name, a, b)
            n_q += 1
            for seq, thr in ((want, 1.0), (want[::-1], 0.9), (want + b"A", 0.5), (b"N" * len(want), 0.1)):
                assert on.compare(name, a, b, seq, thr) == off.compare(name, a, b, seq, thr), (name, a, b, thr)
    assert on.getChromosomeLength("nope") == off.getChromosomeLength("nope") == 0
    for g in (on, off):
        with pytest.raises(KeyError):
            g.query("nope", 1, 2)
        with pytest.raises(KeyError):
            g.compare("nope", 1, 2, b"AC", 0.5)
    st = on.device_stats
    assert st["fetch_calls"] >= n_q and st["items_fetched"] == st["fetch_calls"] and st["fallback"] == 0
    on.close()
    off.close()


@pytest.mark.parametrize("with_gaps", [False, True])
def test_save_vcf_is_the_host_backings_and_the_oracles(gctx, fasta, oracle, tmp_path, with_gaps):
    path, contigs = fasta
    rng = np.random.default_rng(3 + with_gaps)
    off = host.ReferenceGenome(path)
    on = host.ReferenceGenome(path, load_on_device=True, ctx=gctx, window_bytes=4096)
    items = []
    for name in ["chr2", "chrA", "chrB", "chr10"]:
        L = len(contigs[name])
        calls, alts = random_calls(rng, 400, L)
        depth = rng.integers(0, 90, (L + 1) if name != "chrB" else L // 2).astype(np.uint32)
        items.append((name, calls, alts, depth))
    items.append(("chrEmpty", np.zeros(0, CALL_DTYPE), [], None))
    gap = None
    if with_gaps:
        gap = str(tmp_path / "gaps.bed")
        write_gaps(gap, contigs, rng)
    want_path = str(tmp_path / "oracle.vcf")
    rc, want_counts = oracle.save_vcf(want_path, path, items, gap_path=gap, file_date=DATE)
    assert rc == 0
    want = open(want_path, "rb").read()
    for map_order in (False, True):
        outs = {}
        for key, g in (("off", off), ("on", on)):
            d = tmp_path / f"{key}{int(map_order)}"
            d.mkdir()
            before = g.device_stats
            assert host.save_vcf(str(d), g, items, gap_path=gap, file_date=DATE, map_order=map_order) == want_counts
            outs[key] = (d / "output.vcf").read_bytes()
            after = g.device_stats
            if key == "on":                               # one fetch per contig that has a REF to look up, its items the DEL and INS calls
                assert after["fetch_calls"] - before["fetch_calls"] == 4 and after["items_fetched"] - before["items_fetched"] > 300 and after["fallback"] == 0
            else:
                assert after["fetch_calls"] == 0 and after["on_device"] == 0
        assert outs["on"] == outs["off"]
        if not map_order:
            assert outs["on"] == want
        else:
            assert sorted(outs["on"].split(b"\n")) == sorted(want.split(b"\n"))
    with pytest.raises(RuntimeError):                     # a call on a contig the genome does not hold: the same failure either way
        host.save_vcf(str(tmp_path / "on0"), on, [("chrNope", *random_calls(np.random.default_rng(1), 50, 100), None)], file_date=DATE)
    with pytest.raises(RuntimeError):
        host.save_vcf(str(tmp_path / "off0"), off, [("chrNope", *random_calls(np.random.default_rng(1), 50, 100), None)], file_date=DATE)
    on.close()
    off.close()


def test_run_bam_writes_the_same_vcf(ctx, gctx, tmp_path):
    from hmm_params import WGS_HMM
    from test_gpu_shard_build_run import _run_inputs
    path, off = _run_inputs(tmp_path)
    on = host.ReferenceGenome(off.path, load_on_device=True, ctx=gctx)
    assert on.device_stats["on_device"] == 1 and on.device_stats["fallback"] == 0 and on.device_stats["records"] == len(off.getChromosomes())
    hmm = make_hmm(**WGS_HMM)
    outs = {}
    for key, g in (("off", off), ("on", on)):
        d = tmp_path / key
        d.mkdir()
        calls, tid, st = host.run_bam(ctx, path, hmm, threads=8, split_svs=True, cigar_cn=True, genome=g, vcf_dir=str(d), file_date="20250926")
        outs[key] = (calls, tid, (d / "output.vcf").read_text().split("\n"))
    assert len(outs["off"][0]) > 20 and np.array_equal(outs["on"][1], outs["off"][1])
    for f in outs["off"][0].dtype.names:
        assert np.array_equal(outs["on"][0][f], outs["off"][0][f]), f
    assert outs["on"][2] == outs["off"][2] and len([l for l in outs["on"][2] if l and not l.startswith("#")]) > 20      # line for line
    st = on.device_stats
    assert st["fetch_calls"] >= 1 and st["items_fetched"] >= 1 and st["fallback"] == 0 and off.device_stats["fetch_calls"] == 0
    on.close()
    off.close()
