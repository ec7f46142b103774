"""csvgpu_cn_observations_resident_many / csvgpu_cn_decode_resident_many (kernels/cnobs.hip): the copy-number pass's observation vectors
built on the device, on every region family of tests/cn_observation_inputs.py in ONE call over two shards — against the oracle's real
std::unordered_map region by region (order included), against the host mirror's assembly byte for byte, and the fused call against
csvgpu_viterbi on the seam's arrays bit for bit."""
import numpy as np
import pytest

import cn_observation_inputs as cni
from contextsv_amd import CsvError, _lib, host, make_hmm
from hmm_params import WGS_HMM

pytestmark = pytest.mark.gpu
FIELDS = ("pos", "baf", "pfb", "log2_cov", "is_snp")


@pytest.fixture(scope="module")
def cn_setup(ctx):
    reads = cni.build_reads()
    shards = [ctx.upload(reads, cni.CHR_LEN + 1) for _ in range(2)]
    res = [sh.pipeline(eps=0.1, min_pts_pct=0.1) for sh in shards]
    depth = shards[0].fetch(res[0], want_depth=True)["depth"]
    mean_cov = [res[0].mean_cov, 1.7 * res[1].mean_cov]            # the second shard's windows against another mean: other log2 ratios
    tables = cni.build_snps()
    t = cni.device_tables(tables, cni.families(tables))
    args = (shards, mean_cov, t["reg_off"], t["region_start"], t["region_end"], t["sample_size"], t["snp_off"], t["snp_pos"], t["snp_baf"], t["snp_pfb"])
    obs = ctx.cn_observations(*args)
    yield shards, mean_cov, depth, tables, t, args, obs
    for sh in shards:
        sh.free()


def _region(obs, i):
    a, b = int(obs["obs_off"][i]), int(obs["obs_off"][i + 1])
    return {f: obs[f][a:b] for f in FIELDS}


def _subset(t, shards, mean_cov, keep):
    """The call's arguments for the regions `keep` (indices into t's region list, ascending)."""
    keep = np.asarray(keep)
    shard_of = np.searchsorted(t["reg_off"], keep, "right") - 1
    reg_off = np.concatenate([[0], np.cumsum([(shard_of == s).sum() for s in range(len(shards))])]).astype(np.uint64)
    lens = np.diff(t["snp_off"]).astype(np.int64)[keep]
    idx = np.concatenate([np.arange(int(t["snp_off"][i]), int(t["snp_off"][i + 1])) for i in keep] + [np.zeros(0, np.int64)]).astype(np.int64)
    snp_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return (shards, mean_cov, reg_off, t["region_start"][keep], t["region_end"][keep], t["sample_size"][keep], snp_off, t["snp_pos"][idx],
            t["snp_baf"][idx], t["snp_pfb"][idx])


def test_offsets_and_bound(cn_setup):
    shards, mean_cov, depth, tables, t, args, obs = cn_setup
    n_win = np.maximum(t["sample_size"], np.diff(t["snp_off"]).astype(np.int64))
    per = np.diff(obs["obs_off"].astype(np.int64))
    assert obs["obs_off"][0] == 0 and int(obs["obs_off"][-1]) == len(obs["pos"]) and (per >= 1).all()
    assert (per <= n_win + 3 * np.diff(t["snp_off"]).astype(np.int64)).all()
    assert len(t["regions"]) >= 200


def test_every_region_matches_the_oracle(cn_setup, oracle):
    shards, mean_cov, depth, tables, t, args, obs = cn_setup
    for i, r in enumerate(t["regions"]):
        exp = oracle.query_snp_region(depth, r["start"], r["end"], mean_cov[r["table"]], r["ss"], tables[r["table"]])
        got = _region(obs, i)
        assert np.array_equal(got["pos"], exp["pos"]) and np.array_equal(got["is_snp"].astype(bool), exp["is_snp"]), r      # identical order
        assert np.array_equal(got["baf"], exp["baf"]) and np.array_equal(got["pfb"], exp["pfb"]), r
        np.testing.assert_allclose(got["log2_cov"], exp["log2_cov"], rtol=0, atol=1e-6, err_msg=str(r))


def test_byte_identical_to_the_host_assembly(ctx, cn_setup):
    """host.query_snp_regions(on_device=False) is the replaced route: the same window kernel feeds both, so log2_cov is identical too."""
    shards, mean_cov, depth, tables, t, args, obs = cn_setup
    groups = {}
    for i, r in enumerate(t["regions"]):
        groups.setdefault((r["table"], r["ss"]), []).append(i)
    for (tab, ss), idx in groups.items():
        h = host.query_snp_regions(ctx, shards[tab], t["region_start"][idx], t["region_end"][idx], mean_cov[tab], ss, tables[tab], on_device=False)
        for k, i in enumerate(idx):
            got = _region(obs, i)
            for f in FIELDS:
                a, b = int(h["obs_off"][k]), int(h["obs_off"][k + 1])
                want = h[f][a:b]
                assert got[f].astype(want.dtype).tobytes() == want.tobytes(), (t["regions"][i], f)


def test_both_kernel_forms_are_reached_and_agree_with_the_whole_call(ctx, cn_setup):
    shards, mean_cov, depth, tables, t, args, obs = cn_setup
    n_win = np.maximum(t["sample_size"], np.diff(t["snp_off"]).astype(np.int64))
    small, big = np.nonzero(n_win <= cni.SMALL_MAX)[0], np.nonzero(n_win > cni.SMALL_MAX)[0]
    assert len(small) >= 100 and len(big) >= 20 and n_win.max() == cni.MAX_WINDOWS and (n_win == cni.SMALL_MAX).any() and (n_win == cni.SMALL_MAX + 1).any()
    for keep in (small, big):                                       # a call with one form only
        part = ctx.cn_observations(*_subset(t, shards, mean_cov, keep))
        for k, i in enumerate(keep):
            a, b = _region(part, k), _region(obs, i)
            assert all(a[f].tobytes() == b[f].tobytes() for f in FIELDS), t["regions"][i]


def test_decode_equals_viterbi_on_the_seams_arrays(ctx, cn_setup):
    shards, mean_cov, depth, tables, t, args, obs = cn_setup
    hmm = make_hmm(**WGS_HMM)
    states, ll = ctx.viterbi(hmm, obs["log2_cov"], obs["baf"], obs["pfb"], obs["obs_off"])
    dec = ctx.cn_decode(hmm, *args)
    assert np.array_equal(dec["obs_off"], obs["obs_off"]) and np.array_equal(dec["pos"], obs["pos"])
    assert np.array_equal(dec["states"], states) and dec["loglik"].tobytes() == ll.tobytes()
    assert set(dec) == {"obs_off", "pos", "states", "loglik"}
    full = ctx.cn_decode(hmm, *args, want_observations=True)
    assert all(full[f].tobytes() == obs[f].tobytes() for f in FIELDS)
    assert np.array_equal(full["states"], states) and full["loglik"].tobytes() == ll.tobytes()


def test_capacity_reports_the_exact_count(ctx, cn_setup):
    shards, mean_cov, depth, tables, t, args, obs = cn_setup
    total = len(obs["pos"])
    with pytest.raises(CsvError) as e:
        ctx.cn_observations(*args, capacity=total - 1)
    assert e.value.status == _lib.CSV_ECAPACITY and e.value.needed == total
    with pytest.raises(CsvError) as e:
        ctx.cn_observations(*args, capacity=0)
    assert e.value.status == _lib.CSV_ECAPACITY and e.value.needed == total
    again = ctx.cn_observations(*args, capacity=total)
    assert np.array_equal(again["obs_off"], obs["obs_off"]) and all(again[f].tobytes() == obs[f].tobytes() for f in FIELDS)


def test_domain_violations_are_rejected_and_the_context_stays_usable(ctx, cn_setup):
    shards, mean_cov, depth, tables, t, args, obs = cn_setup
    one = [shards[:1], mean_cov[:1], [0, 1]]
    none = (np.zeros(0, np.uint32), np.zeros(0), np.zeros(0))
    bad = {
        "sample_size <= 0": (*one, [1000], [2000], [0], [0, 0], *none),
        "start > end": (*one, [2000], [1000], [20], [0, 0], *none),
        "2^31": (*one, [2 ** 31 - 100], [2 ** 31 - 1], [20], [0, 0], *none),
        "5087 windows": (*one, [1000], [90_000], [cni.MAX_WINDOWS + 1], [0, 0], *none),
        "decrease": (*one, [1000], [2000], [20], [0, 3], np.asarray([1100, 1300, 1200], np.uint32), np.full(3, 0.5), np.full(3, 0.5)),
        "reg_off": (shards, mean_cov, [0, 2, 1], [1000], [2000], [20], [0, 0], *none),
    }
    hmm = make_hmm(**WGS_HMM)
    for what, a in bad.items():
        for call in (lambda: ctx.cn_observations(*a), lambda: ctx.cn_decode(hmm, *a)):
            with pytest.raises(CsvError) as e:
                call()
            assert e.value.status == _lib.CSV_EINVAL, what
            assert what.split()[0] in str(e.value) or what in str(e.value), (what, str(e.value))
    ok = ctx.cn_observations(*_subset(t, shards, mean_cov, [0, 1, len(t["regions"]) - 1]))
    for k, i in enumerate([0, 1, len(t["regions"]) - 1]):
        assert all(_region(ok, k)[f].tobytes() == _region(obs, i)[f].tobytes() for f in FIELDS)
    empty = ctx.cn_observations(shards, mean_cov, [0, 0, 0], [], [], [], [0], *none)
    assert len(empty["pos"]) == 0 and list(empty["obs_off"]) == [0]
