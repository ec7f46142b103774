"""The Python model of the SNP table builder (tests/snp_build_inputs.py) on its own, on the CPU: for every input family the rules alone
give the runs and the per-contig columns that tests/test_gpu_snp_build.py expects of the device, and the generated text leaves most of
its kept records to the device, so that no device test can pass on the host path alone."""
import numpy as np

import snp_build_inputs as sb
import vcf_parse_inputs as inp


def test_runs_of_the_name_families():
    for label, names in sb.NAME_FAMILIES:
        text = sb.name_text(names, per=3)
        e = sb.expected_append(text)
        assert e["n_kept"] == 3 * len(names) and e["n_deferred"] == 0, label
        assert e["run_names"] == [n.encode() for n in names], label
        assert e["run_first"].tolist() == [3 * i for i in range(len(names))], label
        assert e["run_chrom_len"].tolist() == [len(n) for n in names], label
        for off, n in zip(e["run_line_off"].tolist(), names):
            assert text[off:off + len(n) + 1] == n.encode() + b"\t", label


def test_tile_edge_texts_put_the_name_across_the_edge():
    for label, names in sb.NAME_FAMILIES[4:6]:
        texts = sb.tile_edge_texts(names)
        assert len(texts) == len(names[0]) - 1
        for cut, text in enumerate(texts, 1):
            e = sb.expected_append(text)
            assert e["run_line_off"][0] == sb.T - cut and e["run_names"] == [n.encode() for n in names], (label, cut)
            assert e["n_kept"] == 2 * len(names)


def test_skipped_and_deferred_lines_break_no_run():
    text = sb.body([sb.good(5), sb.deferred(6), sb.skipped(7), sb.deferred(8, "chr2"), sb.good(9), sb.good(10, "chr2"), sb.deferred(11)])
    e = sb.expected_append(text)
    assert e["run_names"] == [b"chr1", b"chr2"] and e["run_first"].tolist() == [0, 2]
    assert e["n_deferred"] == 3 and e["n_kept"] == 3


def test_model_columns():
    m = sb.Model()
    a = sb.body([sb.good(5), sb.good(3, "chr2"), sb.deferred(9, "chr3"), sb.good(7)])
    b = sb.body([sb.good(1), sb.deferred(2, "chr2", ref="N"), sb.good(8, "chr2")])
    eb = m.append(b, text_base=len(a))                            # the later batch first: the key orders
    ea = m.append(a)
    assert (eb["first_run"], ea["first_run"]) == (0, 2) and m.run_contig == [0, 1, 0, 1, 0]
    m.host_records(a, ea["defer_off"])
    assert m.host_records(b, eb["defer_off"], len(a))[0].tolist() == []          # REF N: the stand-in host parser keeps nothing
    cols = m.columns()
    assert sorted(cols) == [0, 1, 2] and m.ids == {b"chr1": 0, b"chr2": 1, b"chr3": 2}
    assert cols[0][0].tolist() == [5, 7, 1] and not cols[0][2]
    assert cols[1][0].tolist() == [3, 8] and cols[1][2]
    assert cols[2][0].tolist() == [9] and cols[2][1].tolist() == [sb.DEFER_BAF]
    m2 = sb.Model()
    assert [x.tolist() for x in m2.host_batch(a)] == [[0, 1, 2, 0], [0, len(sb.good(5)) + 1, 2 * len(sb.good(5)) + 2, a.rfind(b"chr1")], [5, 3, 9, 7],
                                                      [0.75, 0.75, sb.DEFER_BAF, 0.75]]


def test_the_generated_text_leaves_most_records_to_the_device():
    """fewer than half of the kept records can come from deferred lines: even if the host parser kept every deferred line"""
    text, _, _ = sb.generated()
    e = sb.expected_append(text)
    assert e["n_kept"] > 700
    assert e["n_deferred"] < e["n_kept"]
    # ... and with the deliberate deferred lines of tests/vcf_parse_inputs.py mixed in
    mixed = text + sb.body([l.encode() for _, l in inp.DELIBERATE_SNP])
    e = sb.expected_append(mixed)
    assert e["n_deferred"] == len(inp.DELIBERATE_SNP) < e["n_kept"]
    assert e["run_names"] == [b"chr1", b"chr2"]


def test_big_text():
    text = sb.big_text()
    e = sb.expected_append(text)
    assert e["n_kept"] >= 70_000 and e["n_deferred"] == 0 and e["n_runs"] > 100
    assert e["n_kept"] > 65_536                                   # more than the capped grid of the builder's kernels (256 x 256 lanes)
    m = sb.Model()
    m.append(text)
    assert len(m.columns()) == 5 and all(c[2] for c in m.columns().values())
