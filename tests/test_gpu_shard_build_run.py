"""Resident shards built on the device, through the reader and the run (BamReadOptions::device_shard, RunParams::shard_on_device): the
reader's shard holds the records the host route reads, nothing but the small per-record arrays comes down, corrupt files fail with the host
route's message and leak nothing, and runBam makes the same calls — the 50-base ALT strings, cut on the device from the shard's own
sequences, included. The kernels' own cases are in tests/test_gpu_shard_build.py and tests/test_gpu_alt_bases.py."""
import os

import numpy as np
import pytest

import bam_py
import bam_unpack_inputs as inp
from contextsv_amd import Reads, host, make_hmm
from test_gpu_alt_bases import py_alt

pytestmark = pytest.mark.gpu
M, I, S = 0, 1, 4


def _file_with_sequences(tmp_path, seed=11):
    """the three contigs of tests/test_gpu_bgzf_inflate.py with the 70 001-operation record, random sequences -> (path, names, host route's shards)"""
    import test_gpu_bgzf_inflate as tbi
    _, reads, tid, qnames, contig_len = tbi._three_contigs()
    reads, tid, qnames = tbi._with_long_cigar(reads, tid, qnames)
    rng = np.random.default_rng(seed)
    l_seq = rng.integers(0, 30, reads.n_reads).astype(np.int32)
    seq_off = np.concatenate([[0], np.cumsum((l_seq + 1) // 2)]).astype(np.uint64)
    seq = rng.integers(0, 256, int(seq_off[-1]), dtype=np.uint8)
    names = ["contig%d" % t for t in range(3)]
    path = str(tmp_path / "reads.bam")
    host.write_bam(path, names, [contig_len] * 3, tid, reads, qnames, seq_off, seq, l_seq, level=1, threads=8)
    bam = host.BamFile(path)
    want = {}
    for t in range(3):
        s = bam.read_contig(names[t], want_seq=True, want_qnames=True, threads=8)
        want[t] = dict(s, reads=tbi._copy_reads(s["reads"]), seq_off=s["seq_off"].copy(), seq=s["seq"].copy())
    bam.close()
    return path, names, want


@pytest.mark.parametrize("inflate_on_device", [False, True])
def test_reader_builds_the_shard_on_the_device(ctx, tmp_path, inflate_on_device):
    path, names, want = _file_with_sequences(tmp_path)
    assert max(np.diff(want[0]["reads"].cigar_off)) > 65535
    bam = host.BamFile(path)
    for window in (1, 5, 0):
        for t in (1, 0, 2):
            got = bam.read_contig(names[t], want_seq=True, want_qnames=True, threads=8, window_blocks=window, inflate_on_device=inflate_on_device,
                                  shard_on_device=True, ctx=ctx)
            sh, w = got["shard"], want[t]
            try:
                st = bam.unpack_stats()
                assert st["shard_resident"] == 1 and st["batches_host"] == 0 and st["batches_appended_host"] == 0 and st["cigar_words_downloaded"] == 0, (window, t, st)
                assert st["records"] == w["reads"].n_reads and st["batches_device"] >= (2 if window == 1 else 1), (window, t, st)
                assert st["batches_kept_on_device"] == (st["batches_device"] if inflate_on_device else 0), (window, t, st)
                # the host holds the small arrays only
                assert len(got["reads"].cigar) == 0 and "seq" not in got and (got["tid"], got["name"], got["target_len"]) == (w["tid"], w["name"], w["target_len"])
                for f in ("pos", "flag", "mapq"):
                    assert np.array_equal(getattr(got["reads"], f), getattr(w["reads"], f)), f
                assert got["qnames"] == w["qnames"]
                # the shard holds the host route's records
                back = sh.fetch_reads()
                for f in ("pos", "flag", "mapq", "cigar_off", "cigar"):
                    assert np.array_equal(getattr(back, f), getattr(w["reads"], f)), f
                nm = sh.fetch_names()
                assert [x.decode() for x in nm["names"]] == w["qnames"] and np.array_equal(nm["name_hash"], host.string_hashes(w["qnames"]))
                assert sh.sizes() == dict(n_reads=w["reads"].n_reads, n_cigar=w["reads"].n_cigar, n_seq=len(w["seq"]), n_name=sum(len(q) for q in w["qnames"]))
                if window == 5:                                       # its sequences, record by record
                    nb = np.diff(w["seq_off"]).astype(np.int64)
                    bases = ctx.alt_bases(sh, np.arange(len(nb)), np.zeros(len(nb)), 2 * nb)
                    raw = w["seq"].tobytes()
                    for r in range(0, len(nb), 7):
                        assert bases[r] == py_alt(raw[int(w["seq_off"][r]):int(w["seq_off"][r + 1])], 0, 2 * int(nb[r])), r
            finally:
                sh.free()
    # back on the host route with the same handle; and a contig read without sequences and names
    import test_gpu_bgzf_inflate as tbi
    tbi._same_shard(bam.read_contig(names[1], want_seq=True, want_qnames=True), want[1])
    got = bam.read_contig(names[2], shard_on_device=True, ctx=ctx)
    try:
        assert got["shard"].sizes() == dict(n_reads=want[2]["reads"].n_reads, n_cigar=want[2]["reads"].n_cigar, n_seq=0, n_name=0)
    finally:
        got["shard"].free()
    bam.close()


def test_corrupt_files_fail_like_the_host_route(ctx, tmp_path):
    def message(p, **kw):
        bam = host.BamFile(p)
        with pytest.raises(RuntimeError) as ei:
            bam.read_contig("c0", want_seq=True, want_qnames=True, threads=4, **kw)
        st = bam.unpack_stats()
        return str(ei.value), st, bam

    good = b"".join(inp.refusal_records())
    entries = inp.index_entries(good)
    bam_py.write_bam(str(tmp_path / "good.bam"), ["c0"], [1 << 28], entries)
    for k, (name, stream, reason, at) in enumerate(inp.refusal_streams()):
        p = str(tmp_path / ("bad%d.bam" % k))
        bam_py.write_bam(p, ["c0"], [1 << 28], [(stream, 0, 0, 1, 0)], with_index=False)
        open(p + ".bai", "wb").write(open(str(tmp_path / "good.bam.bai"), "rb").read())
        on_host, _, b0 = message(p)
        b0.close()
        assert on_host == inp.MESSAGES[reason]
        for inflate in (False, True):
            msg, st, bam = message(p, shard_on_device=True, inflate_on_device=inflate, ctx=ctx)
            assert msg == on_host and st["shard_resident"] == 0 and st["batches_device"] == 0 and st["batches_host"] == 1, (name, st)
            # the builder went with the failed read: the handle reads again, with the same refusal
            with pytest.raises(RuntimeError) as ei:
                bam.read_contig("c0", shard_on_device=True, ctx=ctx)
            assert str(ei.value) == on_host
            bam.close()
    # the intact file of the same records: a second read_contig on one handle works, and the shard is the twelve records
    bam = host.BamFile(str(tmp_path / "good.bam"))
    exp = inp.expected(good)
    for _ in range(2):
        got = bam.read_contig("c0", want_seq=True, want_qnames=True, shard_on_device=True, ctx=ctx)
        try:
            st = bam.unpack_stats()
            assert st["shard_resident"] == 1 and st["records"] == 12 and st["anchors"] == 12 and st["batches_appended_host"] == 0, st
            back = got["shard"].fetch_reads()
            for f in ("pos", "flag", "mapq", "cigar_off", "cigar"):
                assert np.array_equal(getattr(back, f), exp[f]), f
        finally:
            got["shard"].free()
    bam.close()


def test_declined_batch_goes_up_from_the_host_parser(ctx, tmp_path):
    """a valid file whose index points INSIDE a record: the device declines the batch (anchor missed), the host parser reads it, and its
    arrays are appended to the builder (csvgpu_shard_builder_append_host): the same shard"""
    recs = inp.refusal_records()
    good = b"".join(recs)
    exp = inp.expected(good)
    entries = inp.index_entries(good)
    p = str(tmp_path / "good.bam")
    bam_py.write_bam(p, ["c0"], [1 << 28], entries)
    # an index made for a stream whose records 3.. start 7 bytes later than they do here: its chunk begins lie inside this file's records
    shifted = [(e[0] + (b"\0" * 7 if k == 2 else b""),) + e[1:] for k, e in enumerate(entries)]
    bam_py.write_bam(str(tmp_path / "shifted.bam"), ["c0"], [1 << 28], shifted)
    os.replace(str(tmp_path / "shifted.bam.bai"), p + ".bai")
    bam = host.BamFile(p)
    got = bam.read_contig("c0", want_seq=True, want_qnames=True, shard_on_device=True, ctx=ctx)
    try:
        st = bam.unpack_stats()
        assert st["shard_resident"] == 1 and st["batches_host"] >= 1 and st["batches_appended_host"] >= 1 and st["cigar_words_downloaded"] == 0, st
        back = got["shard"].fetch_reads()
        for f in ("pos", "flag", "mapq", "cigar_off", "cigar"):
            assert np.array_equal(getattr(back, f), exp[f]), f
        nm = got["shard"].fetch_names()
        assert nm["names"] == exp["names"] and np.array_equal(nm["name_hash"], exp["name_hash"])
        assert got["qnames"] == [x.decode() for x in exp["names"]] and np.array_equal(got["reads"].pos, exp["pos"])
        nb = np.diff(exp["seq_off"]).astype(np.int64)
        raw = exp["seq"].tobytes()
        bases = ctx.alt_bases(got["shard"], np.arange(12), np.zeros(12), 2 * nb)
        assert bases == [py_alt(raw[int(exp["seq_off"][r]):int(exp["seq_off"][r + 1])], 0, 2 * int(nb[r])) for r in range(12)]
    finally:
        got["shard"].free()
    bam.close()


def _run_inputs(tmp_path):
    """three contigs with, on each, stacks of reads that carry a 50-base insertion or a 50-base soft clip, and sequences for those reads"""
    import test_gpu_bgzf_inflate as tbi
    from test_gpu_e2e import _write_genome
    contigs, reads, tid, qnames, contig_len = tbi._three_contigs()
    rng = np.random.default_rng(17)
    recs = []
    for i in range(reads.n_reads):
        a, b = int(reads.cigar_off[i]), int(reads.cigar_off[i + 1])
        recs.append((int(tid[i]), int(reads.pos[i]), int(reads.flag[i]), int(reads.mapq[i]), reads.cigar[a:b], qnames[i], np.zeros(0, np.uint8), 0))
    n_special = 0
    for t in range(3):
        for stack, (pos, cigar) in enumerate([(1_400_000, [(M, 400), (I, 50), (M, 400)]), (1_500_000, [(S, 50), (M, 600)]), (1_600_001, [(S, 7), (M, 333), (I, 50), (M, 200)])]):
            for k in range(9):
                qlen = sum(l for op, l in cigar if op in (M, I, S))
                seq = rng.integers(0, 256, (qlen + 1) // 2, dtype=np.uint8)
                words = np.array([(l << 4) | op for op, l in cigar], np.uint32)
                recs.append((t, pos, 0x10 * (k % 2), 60, words, "alt%d_%d_%d" % (t, stack, k), seq, qlen))
                n_special += 1
    recs.sort(key=lambda r: (r[0], r[1]))
    coff = np.concatenate([[0], np.cumsum([len(r[4]) for r in recs])]).astype(np.uint64)
    rd = Reads([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs], coff, np.concatenate([r[4] for r in recs]))
    l_seq = np.array([r[7] for r in recs], np.int32)
    seq_off = np.concatenate([[0], np.cumsum((l_seq + 1) // 2)]).astype(np.uint64)
    path = str(tmp_path / "reads.bam")
    host.write_bam(path, ["contig%d" % t for t in range(3)], [contig_len] * 3, np.array([r[0] for r in recs], np.int32), rd, [r[5] for r in recs], seq_off,
                   np.concatenate([r[6] for r in recs]), l_seq, level=1, threads=8)
    fasta = str(tmp_path / "genome.fa")
    _write_genome(fasta, 3, np.random.default_rng(1))
    return path, host.ReferenceGenome(fasta)


def test_run_from_bam_with_the_shard_on_the_device_gives_the_same_calls(ctx, tmp_path):
    from hmm_params import WGS_HMM
    path, genome = _run_inputs(tmp_path)
    hmm = make_hmm(**WGS_HMM)
    stats = lambda s: {k: s[k] for k in ("n_contigs", "n_reads", "n_cigar", "bam_bytes")}
    n_cut = 0
    for split in (True, False):
        d = tmp_path / ("off%d" % split)
        d.mkdir()
        want, want_tid, st = host.run_bam(ctx, path, hmm, threads=8, split_svs=split, cigar_cn=True, genome=genome, vcf_dir=str(d), file_date="20250926")
        assert len(want) > 20 and st["n_contigs"] == 3 and st["contigs_resident"] == 0
        vcf = sorted((d / "output.vcf").read_text().split("\n"))
        alts = [ln.split("\t")[4] for ln in vcf if ln and not ln.startswith("#")]
        # calls whose ALT string was cut from a read's bases: the reference base in front of fifty characters of the code table
        cut = [a for a in alts if len(a) == 51 and set(a[1:]) <= set("=ACGTN") and a[1:] != "N" * 50]
        assert len(cut) >= 3, sorted({len(a) for a in alts})
        n_cut += len(cut)
        for k, kw in enumerate((dict(shard_on_device=True), dict(shard_on_device=True, inflate_on_device=True))):
            d2 = tmp_path / ("on%d_%d" % (split, k))
            d2.mkdir()
            got, got_tid, st_on = host.run_bam(ctx, path, hmm, threads=8, split_svs=split, cigar_cn=True, genome=genome, vcf_dir=str(d2), file_date="20250926", **kw)
            assert len(got) == len(want) and np.array_equal(got_tid, want_tid), kw
            for f in want.dtype.names:                                     # call for call, field for field
                assert np.array_equal(got[f], want[f]), (f, kw)
            assert sorted((d2 / "output.vcf").read_text().split("\n")) == vcf, kw      # the ALT strings among them
            assert stats(st_on) == stats(st) and st_on["contigs_resident"] == 3, st_on
            assert st_on["unpack_batches_device"] >= 3 and st_on["unpack_batches_host"] == 0 and st_on["unpack_batches_appended_host"] == 0, st_on
            assert st_on["unpack_batches_kept_on_device"] == (st_on["unpack_batches_device"] if "inflate_on_device" in kw else 0), st_on
    assert n_cut >= 6
