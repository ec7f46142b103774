"""The plain-Python restatement of the device VCF parser's line rules (tests/vcf_parse_inputs.py) against the unchanged host parser
(host.SNPFile, option off) and the oracle, on the generated files of tests/test_snp_io.py and on the deliberate additions: the kept
records together with the host-parsed deferred lines are exactly the host's tables, and the deferred set is exactly the listed lines.
CPU only."""
import numpy as np
import pytest

import vcf_parse_inputs as inp
from contextsv_amd import host


def _write(path, header, text: bytes):
    with open(path, "wb") as f:
        f.write(header.encode() + text)
    return str(path)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcfparse")
    text, snps, rng = inp.generated_snp_text()
    (d / "gnomad_txt").mkdir()
    g = {}
    for c in ("chr1", "chr2"):
        gt, _ = inp.generated_gnomad_text(rng, snps, c)
        g[c] = (gt, _write(d / "gnomad_txt" / ("g.%s.vcf" % c), inp.GNOMAD_HEADER, gt))
    return d, text, _write(d / "sample.vcf", inp.HEADER, text), g


def _by_chrom(text, exp):
    """the kept records of a restated SNP parse as {chrom: (offsets, pos, baf)}"""
    out = {}
    for o, n, p, v in zip(exp["line_off"], exp["chrom_len"], exp["pos"], exp["value"]):
        out.setdefault(text[int(o):int(o) + int(n)].decode(), []).append((int(o), int(p), float(v)))
    return out


def _host_snp_line(tmp, line: bytes):
    """the host parser's verdict on one data line: [] or [(chrom, pos, baf)]"""
    snp = host.SNPFile(_write(tmp / "one.vcf", inp.HEADER, line + b"\n"))
    chrom = line.split(b"\t")[0].decode()
    pos, baf, _, _ = snp.table(chrom)
    return [(chrom, int(p), float(b)) for p, b in zip(pos, baf)]


def test_generated_snp_file(corpus, oracle):
    d, text, path, g = corpus
    exp = inp.expected_snp(text)
    assert exp["declined_at"] is None and exp["stop_off"] == inp.NO_STOP and exp["n_lines"] == text.count(b"\n")
    assert len(exp["defer_off"]) == 0, "the generated corpus holds nothing outside the conversion rules"
    snp = host.SNPFile(path)
    got = _by_chrom(text, exp)
    assert sorted(got) == ["chr1", "chr2"] and snp.records_kept == len(exp["pos"]) > 700
    for c, recs in got.items():
        pos, baf, _, _ = snp.table(c)
        assert _same(pos, np.array([r[1] for r in recs], np.uint32)) and _same(baf, np.array([r[2] for r in recs]))
    # the header's types decide: without Integer DP / AD nothing is kept
    assert len(inp.expected_snp(text, dp_int=False)["pos"]) == 0 and len(inp.expected_snp(text, ad_int=False)["pos"]) == 0
    # and the oracle's regions out of the restated table (positions ascending in the generated file: a region is a slice)
    rng = np.random.default_rng(5)
    for c, span in (("chr1", 400_000), ("chr2", 300_000)):
        p = np.array([r[1] for r in got[c]], np.uint32)
        b = np.array([r[2] for r in got[c]])
        for _ in range(25):
            lo = int(rng.integers(1, span))
            hi = lo + int(rng.choice([0, 50, 2000, 20_000, 150_000]))
            epos, ebaf, _ = oracle.read_snp_af(path, None, c, c, lo, hi, "AF")
            sel = (p >= lo) & (p <= hi)
            last = {int(q): float(v) for q, v in zip(p[sel], b[sel])}          # the BAF map keeps the last duplicate
            assert _same(np.asarray(epos, np.uint32), p[sel]) and _same(np.asarray(ebaf, np.float64), np.array([last[int(q)] for q in p[sel]]))


@pytest.mark.parametrize("eth", ["nfe", "", "int"])
def test_generated_population_files(corpus, oracle, eth):
    d, text, path, g = corpus
    key = "AF_" + eth if eth else "AF"
    n_nan = 0
    for c in ("chr1", "chr2"):
        snp = host.SNPFile(path)
        pos, _, af_pos, af = snp.table(c, g[c][1], eth)
        exp = inp.expected_af(g[c][0], c, key + "=", np.sort(pos))
        assert len(exp["defer_off"]) == 0 and exp["declined_at"] is None
        if eth == "int":                                      # declared Integer: the host reads no line at all; the device is never asked
            assert len(af_pos) == 0
            continue
        assert _same(af_pos, exp["pos"]) and _same(af, exp["value"]) and len(af) > 50
        n_nan += int(np.isnan(af).sum())
        # the oracle's one frequency per region: the first restated record inside [min SNP, max SNP]
        for lo, hi in ((1, 400_000), (50_000, 120_000), (200_000, 200_500)):
            epos, _, epfb = oracle.read_snp_af(path, g[c][1], c, c, lo, hi, key)
            inside = [(int(q), float(v)) for q, v in zip(exp["pos"], exp["value"]) if len(epos) and min(epos) <= q <= max(epos)]
            assert (epfb is None) == (not inside)
            if inside:
                assert epfb[0] == inside[0][0] and (epfb[1] == inside[0][1] or (np.isnan(epfb[1]) and np.isnan(inside[0][1])))
    assert eth == "int" or n_nan > 0
    # the last position's line ends the file for the device as for the host: a STOP line exists in each generated file
    pos, _, _, _ = host.SNPFile(path).table("chr1")
    assert inp.expected_af(g["chr1"][0], "chr1", "AF=", np.sort(pos))["stop_off"] != inp.NO_STOP


def test_deliberate_snp_lines(corpus, tmp_path):
    d, text, path, g = corpus
    head = text[:text.index(b"\n", 4000) + 1]
    extra = [l for _, l in inp.DELIBERATE_SNP] + inp.NOT_DEFERRED_SNP + [inp.DEFERRED_BY_ORDER]
    full = head + ("\n".join(extra) + "\n").encode() + text[len(head):len(head) + 3000]
    full = full[:full.rindex(b"\n") + 1]
    exp = inp.expected_snp(full)
    want = sorted(full.index(l.encode()) for l in [l for _, l in inp.DELIBERATE_SNP] + [inp.DEFERRED_BY_ORDER])
    assert exp["defer_off"].tolist() == want, "exactly the listed lines are deferred"
    for name, l in inp.DELIBERATE_SNP:
        assert inp.snp_rule(l.encode()) == ("defer",), name
    merged = [(o, c, p, v) for c, recs in _by_chrom(full, exp).items() for o, p, v in recs]
    n_host_kept = 0
    for o in exp["defer_off"]:
        line = full[int(o):full.index(b"\n", int(o))]
        for c, p, v in _host_snp_line(tmp_path, line):
            merged.append((int(o), c, p, v))
            n_host_kept += 1
    assert n_host_kept >= 8                                   # libc reads a number out of most of them: deferring is what keeps them right
    merged.sort(key=lambda r: r[0])
    snp = host.SNPFile(_write(tmp_path / "full.vcf", inp.HEADER, full))
    assert snp.records_kept == len(merged)
    for c in {r[1] for r in merged}:
        pos, baf, _, _ = snp.table(c)
        assert _same(pos, np.array([r[2] for r in merged if r[1] == c], np.uint32)) and _same(baf, np.array([r[3] for r in merged if r[1] == c]))


def test_deliberate_population_lines(tmp_path):
    positions = [900, 1000] + inp.DELIBERATE_AF_POS + [1500]
    sample = ("\n".join(inp.GOOD % (p, "50", "40", "10,30") for p in positions) + "\n").encode()
    spath = _write(tmp_path / "s.vcf", inp.HEADER, sample)
    (tmp_path / "chr").mkdir()
    lines = [inp.GN % ("900", "AF_nfe=0.25"), inp.GN % ("1000", "AF=0.5;AF_nfe=.")] + [l for _, l in inp.DELIBERATE_AF] + [inp.GN % ("1500", "AF_nfe=0.75")]
    gtext = ("\n".join(lines) + "\n").encode()
    exp = inp.expected_af(gtext, "chr1", "AF_nfe=", positions)
    assert exp["defer_off"].tolist() == [gtext.index(l.encode()) for _, l in inp.DELIBERATE_AF]
    assert exp["pos"].tolist() == [900, 1000, 1500] and exp["stop_off"] == inp.NO_STOP          # the device cannot see the deferred STOP line
    # merged in file order with the host's verdict on each deferred line, the first STOP ending it
    merged = []
    recs = sorted([(int(o), "kept", int(p), float(v)) for o, p, v in zip(exp["line_off"], exp["pos"], exp["value"])] +
                  [(int(o), "defer", 0, 0.0) for o in exp["defer_off"]])
    for o, kind, p, v in recs:
        if kind == "kept":
            merged.append((p, v))
            continue
        line = gtext[o:gtext.index(b"\n", o)]
        one = host.SNPFile(spath)
        # a line behind the last position is a STOP for the host: a sentinel record behind it shows whether the host went on
        probe = _write(tmp_path / "chr" / "one.vcf", inp.GNOMAD_HEADER, line + b"\n" + (inp.GN % ("1500", "AF_nfe=0.125")).encode() + b"\n")
        _, _, ap, av = one.table("chr1", probe, "nfe")
        if 1500 not in ap.tolist():
            break                                             # STOP
        merged += [(int(a), float(b)) for a, b in zip(ap[:-1], av[:-1])]
    _, _, af_pos, af = host.SNPFile(spath).table("chr1", _write(tmp_path / "chr" / "g.vcf", inp.GNOMAD_HEADER, gtext), "nfe")
    assert _same(af_pos, np.array([m[0] for m in merged], np.uint32)) and _same(af, np.array([m[1] for m in merged]))
    assert 1500 not in af_pos.tolist() and 1007 in af_pos.tolist()      # "1007x" is 1007 to libc; the 10-digit POS ended the file


def test_value_rule_against_python_float():
    """inside the rule, one double operation gives what Python's correctly rounded float() gives"""
    toks = inp.value_tokens()
    assert len(toks) >= 2000 and len(set(toks)) > 1900
    for t in toks:
        assert inp.tok_real(t.encode()) == float(t), t
    for t in ("1e23", "1234567890123456", "0x10", "1e", ".", "-", "", "1.5.2", "nan", "1e-23", "0." + "0" * 70 + "1"):
        assert inp.tok_real(t.encode()) is None, t
