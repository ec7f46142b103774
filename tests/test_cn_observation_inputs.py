"""The region families of tests/cn_observation_inputs.py against the oracle (CPU only): what the device form of the copy-number
observations relies on is checked on the reference's real container — oracle.query_snp_region iterates a std::unordered_map<std::string,
double> — and every family is shown to reach what it is there for.

On every region: equal keys are adjacent windows; the observations are exactly, as a multiset, what the distinct keys give by the slice
rule (node [ws, we] takes the SNP records with ws <= pos <= we, each record counting, or one dummy observation); the node's log2 ratio is
the run's LAST window's; and there are at most ss + 3 S of them."""
from collections import Counter

import numpy as np
import pytest

import cn_observation_inputs as cni


@pytest.fixture(scope="module")
def cn_inputs(oracle):
    reads = cni.build_reads()
    depth, dsum, dnz = oracle.depth(reads, cni.CHR_LEN + 1)
    tables = cni.build_snps()
    regions = cni.families(tables)
    mean_cov = dsum / dnz
    rows = []
    for r in regions:
        snps = tables[r["table"]]
        p, b, f = cni.flat_snps(snps, r["start"], r["end"])
        ss = max(len(p), r["ss"])
        l2, ws, we = oracle.window_log2(depth, r["start"], r["end"], ss, mean_cov)
        obs = oracle.query_snp_region(depth, r["start"], r["end"], mean_cov, r["ss"], snps)
        rows.append((r, ss, p, b, f, l2, ws, we, obs))
    return depth, tables, rows


def test_at_least_200_distinct_regions(cn_inputs):
    _, _, rows = cn_inputs
    assert len({(r["table"], r["start"], r["end"], r["ss"]) for r, *_ in rows}) >= 200
    assert all(r["start"] <= r["end"] < 2 ** 31 - 1 and r["ss"] > 0 for r, *_ in rows)


def test_equal_keys_are_adjacent_and_the_slice_rule_gives_the_containers_observations(cn_inputs):
    _, _, rows = cn_inputs
    for r, ss, p, b, f, l2, ws, we, obs in rows:
        assert (np.diff(ws.astype(np.int64)) >= 0).all() and (np.diff(we.astype(np.int64)) >= 0).all(), r
        assert np.array_equal(we[:-1], ws[1:]), r
        head = np.ones(ss, bool)
        head[1:] = (ws[1:] != ws[:-1]) | (we[1:] != we[:-1])
        first = np.nonzero(head)[0]
        keys = list(zip(ws[first].tolist(), we[first].tolist()))
        assert len(set(keys)) == len(keys), r                            # a key never comes back after another one: runs only
        last = np.append(first[1:], ss) - 1
        want = Counter()
        for (a, e), lw in zip(keys, last):
            lo, hi = int(np.searchsorted(p, a, "left")), int(np.searchsorted(p, e, "right"))
            if hi > lo:
                for k in range(lo, hi):
                    want[(int(p[k]), float(b[k]), float(f[k]), float(l2[lw]), True)] += 1
            else:
                want[((a + e) // 2, -1.0, 0.5, float(l2[lw]), False)] += 1
        got = Counter(zip(obs["pos"].tolist(), obs["baf"].tolist(), obs["pfb"].tolist(), obs["log2_cov"].tolist(), obs["is_snp"].tolist()))
        assert got == want, r
        assert len(obs["pos"]) <= ss + 3 * len(p), r


def _nodes(ws, we):
    return len(set(zip(ws.tolist(), we.tolist())))


def test_rehash_family_has_node_counts_on_both_sides_of_every_rehash(cn_inputs):
    _, _, rows = cn_inputs
    for t in range(2):
        got = sorted(_nodes(ws, we) for r, ss, p, b, f, l2, ws, we, obs in rows if r["family"] == "rehash" and r["table"] == t)
        assert got == sorted(cni.REHASH_SS)


def test_short_family_collapses_keys_and_puts_a_snp_in_three_nodes(cn_inputs):
    _, _, rows = cn_inputs
    short = [x for x in rows if x[0]["family"] == "short"]
    assert all(_nodes(x[6], x[7]) < x[1] for x in short)
    assert any(_nodes(x[6], x[7]) > cni.SMALL_MAX for x in short) or any(x[1] > cni.SMALL_MAX for x in short)     # collapse in the workgroup form too
    three = 0
    for r, ss, p, b, f, l2, ws, we, obs in short:
        c = Counter(obs["pos"][obs["is_snp"]].tolist())
        mult = Counter(p.tolist())
        three += any(c[q] == 3 * mult[q] for q in c)
    assert three >= 4


def test_snps_family_is_snp_driven_or_has_no_snp(cn_inputs):
    _, _, rows = cn_inputs
    fam = [x for x in rows if x[0]["family"] == "snps"]
    assert sum(x[1] > x[0]["ss"] for x in fam) >= 8 and any(x[1] > cni.SMALL_MAX for x in fam)
    assert sum(len(x[2]) == 0 and not x[8]["is_snp"].any() for x in fam) >= 8


def test_edges_family_has_snps_on_window_starts_and_ends(cn_inputs):
    _, _, rows = cn_inputs
    twice = 0
    for r, ss, p, b, f, l2, ws, we, obs in rows:
        if r["family"] != "edges":
            continue
        on_edge = [q for q in set(p.tolist()) if q in set(ws[1:].tolist())]                    # ws[i] == we[i - 1]: the start of one window, the end of another
        c, mult = Counter(obs["pos"][obs["is_snp"]].tolist()), Counter(p.tolist())
        twice += any(c[q] == 2 * mult[q] for q in on_edge)
        assert r["start"] != int(p[0]) or ws[0] == p[0]
    assert twice >= 12


def test_dups_family_counts_every_record(cn_inputs):
    _, tables, rows = cn_inputs
    n = 0
    for r, ss, p, b, f, l2, ws, we, obs in rows:
        if r["family"] != "dups":
            continue
        mult = Counter(p.tolist())
        assert max(mult.values()) >= 2
        c = Counter(obs["pos"][obs["is_snp"]].tolist())
        assert all(c[q] % mult[q] == 0 and c[q] >= mult[q] for q in mult)
        n += 1
    assert n >= 40


def test_hole_family_reaches_the_floor_and_the_end_of_the_map(cn_inputs):
    depth, _, rows = cn_inputs
    assert not depth[300_000:306_000].any()
    fam = [x for x in rows if x[0]["family"] == "hole"]
    assert sum((x[5] < -20).any() for x in fam) >= 6                 # log2(1e-9 / n / mean) is about -35
    assert sum(x[0]["end"] >= len(depth) and (x[5] == 0).any() for x in fam) >= 6      # no position inside the map: log2 ratio 0


def test_large_family_has_key_texts_of_every_length(cn_inputs):
    _, _, rows = cn_inputs
    lens = set()
    for r, ss, p, b, f, l2, ws, we, obs in rows:
        if r["family"] == "large":
            lens |= {len(f"{a}-{e}") for a, e in zip(ws.tolist(), we.tolist())}
    assert lens == set(range(3, 22))
    assert max(x[7].max() for x in rows) == 2 ** 31 - 1


def test_device_tables_are_in_the_calls_domain(cn_inputs):
    _, tables, rows = cn_inputs
    t = cni.device_tables(tables, [x[0] for x in rows])
    n_win = np.maximum(t["sample_size"], np.diff(t["snp_off"]).astype(np.int64))
    assert n_win.max() == cni.MAX_WINDOWS and (n_win <= cni.SMALL_MAX).any() and (n_win > cni.SMALL_MAX).any()
    for i in range(len(n_win)):
        assert (np.diff(t["snp_pos"][int(t["snp_off"][i]): int(t["snp_off"][i + 1])].astype(np.int64)) >= 0).all()
