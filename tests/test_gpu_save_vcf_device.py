"""host.save_vcf(format_on_device=True) and host.run_bam(vcf_on_device=True): the host mirror's opt-in route through csvgpu_vcf_format
(VCFOptions::format_on_device, host/vcf_writer.cpp) against the option off — output.vcf byte for byte, the counts, the warnings on stderr —
and the route counters that show which side wrote the records."""
import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import host, make_hmm
import synth_small as ss
import vcf_format_inputs as vi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gctx():
    """the genome's own context"""
    c = cs.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def setup(ctx, gctx, tmp_path_factory):
    rng = np.random.default_rng(41)
    seqs = {b"chr2": vi.random_seq(rng, 9000), b"chrA": vi.random_seq(rng, 7000), b"chr10": vi.random_seq(rng, 150_000)}
    path = str(tmp_path_factory.mktemp("fa") / "genome.fa")
    vi.write_fasta(path, seqs)
    off, on = host.ReferenceGenome(path), host.ReferenceGenome(path, load_on_device=True, ctx=gctx)
    assert on.device_stats["on_device"] == 1 and on.device_stats["fallback"] == 0
    shards, contigs = {}, []
    for k, (name, s) in enumerate(seqs.items()):
        reads, depth_len = ss.random_shard(20 + k, n_reads=1500, mean_ops=30, chr_len=max(len(s) - 500 * k, 8000))
        sh = ctx.upload(reads, depth_len)
        res = sh.pipeline()
        shards[name] = (sh, sh.fetch(res, want_depth=True)["depth"])
        calls, alts = vi.random_calls(rng, 400, len(s))
        calls["sv_type"][:3], calls["start"][:3], alts[:3] = 3, [0, 1, 2], [b"<INS>", b"ACG", b"T"]
        calls["sv_type"][3:5], calls["start"][3:5], calls["end"][3:5], alts[3:5] = 1, [depth_len, depth_len + 3], depth_len + 9, [b"<DUP>"] * 2
        calls["sv_type"][6:8], calls["start"][6:8], calls["end"][6:8], alts[6:8] = [0, 3], [len(s) - 3, len(s) + 2], len(s) + 5, [b"<DEL>", b"ACGT"]      # empty REF
        if name == b"chr10":
            calls["sv_type"][5], calls["start"][5], calls["end"][5], alts[5] = 0, 1000, 140_000, b"<DEL>"
        gaps = [(int(a), int(a) + int(rng.integers(1, 200))) for a in rng.integers(0, len(s), 6)]
        contigs.append(vi.contig(name, s, calls, alts, shards[name][1], gaps))
    yield dict(path=path, off=off, on=on, shards=shards, contigs=contigs)
    for sh, _ in shards.values():
        sh.free()
    on.close()
    off.close()


def items(setup, from_shards=True, contigs=None):
    return [(c["name"].decode(), c["calls"], c["alts"], setup["shards"][c["name"]][0] if from_shards else c["depth"]) for c in contigs or setup["contigs"]]


def save(setup, ctx, tmp_path, tag, capfd, genome="on", **kw):
    d = tmp_path / tag
    d.mkdir()
    capfd.readouterr()
    counts = host.save_vcf(str(d), setup[genome], kw.pop("items", None) or items(setup), file_date=vi.DATE, ctx=ctx, **kw)
    return counts, (d / "output.vcf").read_bytes(), capfd.readouterr().err


@pytest.mark.parametrize("with_gaps", [False, True])
@pytest.mark.parametrize("map_order", [False, True])
def test_device_route_writes_the_same_file(setup, ctx, tmp_path, capfd, with_gaps, map_order):
    gap = None
    if with_gaps:
        gap = str(tmp_path / "gaps.bed")
        vi.write_gaps(gap, setup["contigs"])
    host.vcf_route_stats(reset=True)
    c_off, f_off, e_off = save(setup, ctx, tmp_path, "off", capfd, gap_path=gap, map_order=map_order)
    assert host.vcf_route_stats() == dict(device=0, host=0, declined=0)
    c_on, f_on, e_on = save(setup, ctx, tmp_path, "on", capfd, gap_path=gap, map_order=map_order, format_on_device=True)
    assert host.vcf_route_stats(reset=True) == dict(device=1, host=0, declined=0)
    assert f_on == f_off and c_on == c_off and c_on[0] > 900 and (c_on[2] > 0) == with_gaps
    assert e_on == e_off and "Insertion at the first position" in e_on and "out of range of the depth map" in e_on and "Reference allele is empty" in e_on
    c_host, f_host, _ = save(setup, ctx, tmp_path, "hst", capfd, genome="off", gap_path=gap, map_order=map_order, items=items(setup, from_shards=False))
    assert f_host == f_on and c_host == c_on


def test_host_route_where_the_inputs_are_not_on_the_device(setup, ctx, tmp_path, capfd):
    _, want, _ = save(setup, ctx, tmp_path, "off", capfd)
    host.vcf_route_stats(reset=True)
    _, got, _ = save(setup, ctx, tmp_path, "hostgenome", capfd, genome="off", format_on_device=True)            # a host-backed genome
    assert got == want and host.vcf_route_stats(reset=True) == dict(device=0, host=1, declined=0)
    _, got, _ = save(setup, ctx, tmp_path, "hostdepth", capfd, format_on_device=True, items=items(setup, from_shards=False))      # host depth arrays
    assert got == want and host.vcf_route_stats(reset=True) == dict(device=0, host=1, declined=0)


def test_declined_batch_is_written_by_the_host(setup, ctx, tmp_path, capfd):
    contigs = [dict(c, calls=c["calls"].copy()) for c in setup["contigs"]]
    contigs[1]["calls"]["sv_type"][50], contigs[1]["calls"]["hmm_likelihood"][50] = 1, -1e19
    contigs[1]["alts"] = list(contigs[1]["alts"])
    contigs[1]["alts"][50] = b"<DUP>"
    _, want, e_off = save(setup, ctx, tmp_path, "off", capfd, items=items(setup, contigs=contigs))
    host.vcf_route_stats(reset=True)
    _, got, e_on = save(setup, ctx, tmp_path, "on", capfd, items=items(setup, contigs=contigs), format_on_device=True)
    assert got == want and e_on == e_off and b"HMM=-10000000000000000000.000000;" in got
    assert host.vcf_route_stats(reset=True) == dict(device=0, host=1, declined=1)
    # the host's exceptions are the host's: a call on a contig the genome has not
    with pytest.raises(RuntimeError):
        host.save_vcf(str(tmp_path / "on"), setup["on"], [("chrNope", *vi.random_calls(np.random.default_rng(1), 50, 100), setup["shards"][b"chr2"][0])], file_date=vi.DATE,
                      ctx=ctx, format_on_device=True)
    assert host.vcf_route_stats(reset=True)["host"] == 1


def test_run_bam_writes_the_same_vcf(ctx, gctx, tmp_path):
    from hmm_params import WGS_HMM
    from test_gpu_shard_build_run import _run_inputs
    path, off = _run_inputs(tmp_path)
    on = host.ReferenceGenome(off.path, load_on_device=True, ctx=gctx)
    hmm = make_hmm(**WGS_HMM)
    outs = {}
    host.vcf_route_stats(reset=True)
    for key, flag in (("off", False), ("on", True)):
        d = tmp_path / key
        d.mkdir()
        calls, tid, _ = host.run_bam(ctx, path, hmm, threads=8, split_svs=True, cigar_cn=True, genome=on, vcf_dir=str(d), file_date=vi.DATE, vcf_on_device=flag)
        outs[key] = (calls, (d / "output.vcf").read_text().split("\n"))
        assert host.vcf_route_stats() == dict(device=int(flag), host=0, declined=0)
    assert outs["on"][1] == outs["off"][1] and len([l for l in outs["on"][1] if l and not l.startswith("#")]) > 20      # line for line
    assert np.array_equal(outs["on"][0], outs["off"][0])
    on.close()
    off.close()
