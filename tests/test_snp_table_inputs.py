"""The numpy statements of tests/snp_table_inputs.py (what a resident SNP table answers) on the CPU: the per-record kind against the
loop statement of SNPTable::queryFlat that the copy-number tests already use (tests/cn_observation_inputs.py flat_snps), the first-hit
kind against a literal replay of the default SNPSource::queryFlat (two hash maps) and against the host mirror's SNPFile on real VCF
files (csvhost_snp_query). The families are the ones tests/test_gpu_snp_table.py sends to the device."""
import numpy as np
import pytest

import cn_observation_inputs as cni
import snp_table_inputs as sti
from contextsv_amd import host


def _same(got, pos, baf, pfb, what):
    assert got[0].tobytes() == np.asarray(pos, np.uint32).tobytes(), what
    assert got[1].tobytes() == np.asarray(baf, np.float64).tobytes(), what
    assert got[2].tobytes() == np.asarray(pfb, np.float64).tobytes(), what


def test_families_are_what_they_claim():
    rec, hit = sti.record_tables(), sti.hit_tables()
    assert {"empty", "one", "one_position", "runs", "extremes"} <= set(rec) and all("n%d" % n in rec and "n%d" % n in hit for n in sti.SIZES)
    for t in list(rec.values()) + list(hit.values()):
        assert (np.diff(t["pos"].astype(np.int64)) >= 0).all()
    assert (np.diff(rec["one_position"]["pos"]) == 0).all() and rec["extremes"]["pos"][0] == 0 and rec["extremes"]["pos"][-1] == 2 ** 31 - 2
    r = rec["runs"]
    runs = [np.nonzero(r["pos"] == p)[0] for p in np.unique(r["pos"])]
    shapes = {(len(i), tuple(int(x) for x in r["has_pfb"][i])) for i in runs}
    assert {(2, (1, 0)), (2, (0, 1)), (2, (0, 0)), (3, (1, 0, 0)), (3, (0, 1, 0)), (3, (0, 0, 1)), (3, (0, 0, 0))} <= shapes
    e = hit["edges"]
    assert np.isnan(e["af"]).any() and not np.isin(250, e["pos"]) and np.isin(250, e["af_pos"])
    s, en = sti.regions_for(e)
    assert (s > en).any() and (s == en).any() and (s == 0).any() and (en == sti.POS_MAX).any()
    lo_hits = sum(1 for a, b in zip(s, en) if a <= b and len(sti.query("hits", e, a, b)[0]) and (sti.query("hits", e, a, b)[2] != 0).any())
    assert 0 < lo_hits < len(s)


@pytest.mark.parametrize("name", sorted(sti.record_tables()))
def test_record_statement_is_the_loop_statement(name):
    t = sti.record_tables()[name]
    n = len(t["pos"])
    loop_t = {"pos": t["pos"], "baf": t["baf"], "pfb": np.zeros(n) if t["pfb"] is None else t["pfb"],
              "has_pfb": np.zeros(n, np.uint8) if t["has_pfb"] is None else t["has_pfb"]}
    resolved = sti.resolve_records(t)
    s, e = sti.regions_for(t, seed=1)
    for a, b in zip(s, e):
        got = sti.query("records", t, int(a), int(b), resolved)
        if a > b:
            assert len(got[0]) == 0
            continue
        _same(got, *cni.flat_snps(loop_t, int(a), int(b)), (name, a, b))


def _default_query_flat(t, start, end):
    """SNPSource::queryFlat over SNPFileTable::query, literally: the positions in table order, a map of baf (later writes win) and a map
    of pfb with the one population record the file form accepts."""
    pos = [int(p) for p in t["pos"] if start <= p <= end] if start <= end else []
    baf, pfb = {}, {}
    for p, v in zip(t["pos"], t["baf"]):
        if start <= p <= end:
            baf[int(p)] = v
    if pos:
        lo, hi = min(pos), max(pos)
        for p, v in zip(t["af_pos"], t["af"]):
            if p >= lo:
                if p <= hi:
                    pfb[int(p)] = v
                break
    return pos, [baf[p] for p in pos], [pfb.get(p, 0.0) for p in pos]


@pytest.mark.parametrize("name", sorted(sti.hit_tables()))
def test_hit_statement_is_the_default_query_flat(name):
    t = sti.hit_tables()[name]
    s, e = sti.regions_for(t, seed=2)
    for a, b in zip(s, e):
        _same(sti.query("hits", t, int(a), int(b)), *_default_query_flat(t, int(a), int(b)), (name, a, b))


def test_hit_statement_against_the_host_snp_file(tmp_path):
    """The host mirror's own tables and queries (SNPFile over a sample VCF and a population VCF): csvhost_snp_query's records and its one
    accepted population record, passed through the default queryFlat, are what the statement gives on the file's whole tables."""
    import test_snp_io as io
    rng = np.random.default_rng(23)
    snps = io.snp_lines(rng, "chr1", 600, 100_000)
    io.write_vcf(str(tmp_path / "sample.vcf"), io.HEADER, snps, False)
    (tmp_path / "g").mkdir()
    pfb = str(tmp_path / "g" / "g.chr1.vcf")
    io.write_vcf(pfb, io.GNOMAD_HEADER, io.gnomad_lines(rng, "chr1", np.array([p for p, _ in snps]), 100_000), False)
    f = host.SNPFile(str(tmp_path / "sample.vcf"))
    pos, baf, af_pos, af = f.table("chr1", pfb, "nfe")
    assert len(pos) > 200 and len(af_pos) > 20 and (np.diff(pos.astype(np.int64)) >= 0).all() and (np.diff(pos.astype(np.int64)) == 0).any()
    t = {"pos": pos, "baf": baf, "af_pos": af_pos, "af": af}
    s, e = sti.regions_for(t, seed=3, n_random=150)
    n_hit = 0
    for a, b in zip(s, e):
        if a > b:
            continue
        qpos, qbaf, hit = f.query("chr1", int(a), int(b), pfb, "nfe")
        m = {}
        for p, v in zip(qpos, qbaf):
            m[int(p)] = v
        want_pfb = [hit[1] if hit is not None and int(p) == hit[0] else 0.0 for p in qpos]
        n_hit += hit is not None
        _same(sti.query("hits", t, int(a), int(b)), qpos, [m[int(p)] for p in qpos], want_pfb, (a, b))
    assert n_hit > 20
    f.close()
