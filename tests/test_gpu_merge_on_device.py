"""SVCaller::merge_on_device: the CIGAR merge's representatives chosen on the device behind the DBSCAN (csvgpu_chr_job_cluster_select),
the merge threads only materialising SVCalls from the records. Every comparison is option on against option off on the same shards: the
call set, the ALT strings and the per-contig statistics must be identical, whichever route a contig takes; host.merge_route_stats() says
which it took. Also a directed case of the slot replay's streamed closing segment."""
import numpy as np
import pytest

import contextsv_amd as cs
import merge_select_inputs as mi
import synth_small as ss
from contextsv_amd import _lib, host, make_hmm
from hmm_params import WGS_HMM

pytestmark = pytest.mark.gpu
CAP = _lib.SORT_SLOT_LDS_CAP

SHARDS = {
    "ont_like": dict(seed=311, n_reads=400, mean_ops=60, big_frac=0.08),
    "hifi_like": dict(seed=312, n_reads=700, mean_ops=12, big_frac=0.03, all_ops=False),
    "no_signatures": dict(seed=313, n_reads=50, mean_ops=3, big_frac=0.0, all_ops=False),
}
STAT_FIELDS = ("n_signatures", "n_del", "n_ins", "depth_sum", "depth_nonzero", "min_pts", "mean_cov", "n_calls")


def _shard_reads(kind):
    reads, depth_len = ss.random_shard(**SHARDS[kind])
    if kind == "no_signatures":
        reads.cigar[:] = (reads.cigar & 0xF) | (np.minimum(reads.cigar >> 4, 30) << 4)       # no op reaches the 50 of a signature
    else:                                                                                       # some insertions of exactly 50: their ALT is cut from the read
        ins = np.nonzero(((reads.cigar & 0xF) == 1) & ((reads.cigar >> 4) >= 50))[0][::3]
        reads.cigar[ins] = (50 << 4) | 1
    return reads, depth_len


def _sequences(reads, seed):
    """random 4-bit packed sequences as long as every read's query (M, I, S, =, X lengths)"""
    rng = np.random.default_rng(seed)
    op, ln = reads.cigar & 0xF, (reads.cigar >> 4).astype(np.int64)
    q = np.where(np.isin(op, (0, 1, 4, 7, 8)), ln, 0)
    csum = np.concatenate([[0], np.cumsum(q)])
    qlen = csum[reads.cigar_off[1:].astype(np.int64)] - csum[reads.cigar_off[:-1].astype(np.int64)]
    seq_off = np.concatenate([[0], np.cumsum((qlen + 1) // 2)]).astype(np.uint64)
    return seq_off, rng.integers(0, 256, int(seq_off[-1])).astype(np.uint8)


def _same_stats(a, b):
    for f in STAT_FIELDS:
        assert getattr(a, f) == getattr(b, f), f


@pytest.mark.parametrize("kind", sorted(SHARDS))
def test_process_resident_chromosome_on_equals_off(ctx, kind):
    """calls, tags, statistics and ALT strings — with host sequences and with the sequences the shard itself holds (the resident SeqStore)"""
    host.set_context(ctx)
    reads, depth_len = _shard_reads(kind)
    seq_off, seq = _sequences(reads, 5)
    sh = ctx.upload(reads, depth_len)
    b = ctx.shard_builder(_lib.SB_SEQ)
    b.append_host(reads, seq_off, seq)
    shs = b.finish(depth_len)
    try:
        host.merge_route_stats(reset=True)
        off_calls, off_tags, off_st = host.process_resident_chromosome(ctx, sh, 0.1, 0.1)
        assert host.merge_route_stats() == dict(device=0, host_declined=0, host_overflow=0, buckets_declined=0)       # off: nothing of it
        on_calls, on_tags, on_st = host.process_resident_chromosome(ctx, sh, 0.1, 0.1, merge_on_device=True)
        assert on_calls.tobytes() == off_calls.tobytes() and np.array_equal(on_tags, off_tags)
        _same_stats(on_st, off_st)
        assert (len(off_calls) > 5) == (kind != "no_signatures")
        assert host.merge_route_stats(reset=True) == dict(device=1, host_declined=0, host_overflow=0, buckets_declined=0)
        off_alts = host.process_resident_chromosome_alts(ctx, sh, 0.1, 0.1, seq_off, seq)
        assert host.process_resident_chromosome_alts(ctx, sh, 0.1, 0.1, seq_off, seq, merge_on_device=True) == off_alts
        res_alts = host.process_resident_chromosome_alts(ctx, shs, 0.1, 0.1, resident_seq=True)
        assert res_alts == off_alts
        assert host.process_resident_chromosome_alts(ctx, shs, 0.1, 0.1, resident_seq=True, merge_on_device=True) == off_alts
        # a bound of one partition: the larger buckets are declined, the contig takes the host route, the calls stay
        host.merge_route_stats(reset=True)
        d_calls, d_tags, d_st = host.process_resident_chromosome(ctx, sh, 0.1, 0.1, merge_on_device=True, merge_max_partitions=1)
        assert d_calls.tobytes() == off_calls.tobytes() and np.array_equal(d_tags, off_tags)
        _same_stats(d_st, off_st)
        r = host.merge_route_stats(reset=True)
        assert r["device"] + r["host_declined"] == 1 and r["host_overflow"] == 0 and (r["buckets_declined"] > 0) == (r["host_declined"] == 1)
    finally:
        sh.free(); shs.free()


def test_pipelined_and_lanes_on_equal_off(ctx):
    """five passes over each of two shards, software-pipelined on one context and side by side on two contexts behind a gate"""
    host.set_context(ctx)
    data = [_shard_reads("ont_like"), _shard_reads("hifi_like")]
    ctx2 = cs.Context(0)
    gate = cs.Gate()
    shards = []
    try:
        shards = [ctx.upload(*data[0]), ctx2.upload(*data[1])]
        single = [host.process_resident_chromosome(c, sh, 0.1, 0.1) for c, sh in zip((ctx, ctx2), shards)]
        host.merge_route_stats(reset=True)
        for c, sh, (calls, tags, st) in zip((ctx, ctx2), shards, single):
            off = host.process_resident_pipelined(c, sh, 5, 0.1, 0.1)
            on = host.process_resident_pipelined(c, sh, 5, 0.1, 0.1, merge_on_device=True)
            for got in (off, on):
                assert got[0].tobytes() == calls.tobytes() and np.array_equal(got[1], tags) and got[4] == 5 * len(calls)
                _same_stats(got[2], st)
        assert host.merge_route_stats(reset=True) == dict(device=10, host_declined=0, host_overflow=0, buckets_declined=0)
        ctx.set_gate(gate); ctx2.set_gate(gate)
        for on in (False, True):
            got, st, ms, total = host.process_resident_lanes([ctx, ctx2], shards, [5, 5], 0.1, 0.1, merge_on_device=on)
            assert got.tobytes() == single[0][0].tobytes() and total == 5 * (len(single[0][0]) + len(single[1][0]))
            assert st.n_signatures == single[0][2].n_signatures
        assert host.merge_route_stats(reset=True)["device"] == 10
    finally:
        ctx.set_gate(None)
        for sh in shards:
            sh.free()
        ctx2.close()
        gate.close()


def test_genome_run_on_equals_off(ctx):
    """three small contigs, Genome.run with merge_on_device() on against off, with one lane and with three; then with a bound of one
    partition: identical again, and the accessor reports the declines and the host route taken"""
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    g = host.Genome()
    for t, L in enumerate([500_000, 300_000, 400_000]):
        syn = host.SynthShard(0xD1CE00 + 13 * t, L, 20.0, t % 2, 2, sv_per_bp=1.0 / 20000.0)
        r = syn.reads
        reads = cs.Reads(r.pos.copy(), r.flag.copy(), r.mapq.copy(), r.cigar_off.copy(), r.cigar.copy())
        qid = syn.qname_id.astype(np.uint32) + np.uint32(t << 24)
        rng = np.random.default_rng(200 + t)
        n_snp = L // 1000
        pos = np.sort(rng.choice(np.arange(1000, L - 1000), n_snp, replace=False)).astype(np.uint32)
        snps = {"pos": pos, "baf": np.where(rng.random(n_snp) < 0.66, 0.45 + 0.1 * rng.random(n_snp), 1.0), "pfb": np.zeros(n_snp), "has_pfb": np.zeros(n_snp, np.uint8)}
        g.add(ctx, "contig%d" % t, t, reads, syn.depth_len, qid, snps, name_style=0)
        syn.free()
    lanes = [cs.Context(0) for _ in range(3)]
    gate = cs.Gate()
    try:
        for c in lanes:
            c.set_gate(gate)
        ref, ref_tid, ref_st, ref_per = g.run(ctx, hmm)
        assert len(ref) > 10

        def check(**kw):
            got, tid, st, per = g.run(ctx, hmm, **kw)
            assert np.array_equal(tid, ref_tid) and got.tobytes() == ref.tobytes()
            for a, b in zip(per, ref_per):
                _same_stats(a, b)
            assert st.n_signatures == ref_st.n_signatures and st.n_cigar_calls == ref_st.n_cigar_calls and st.n_final_calls == ref_st.n_final_calls

        host.merge_route_stats(reset=True)
        check(lanes=lanes)                                               # off with lanes
        assert host.merge_route_stats()["device"] == 0
        g.merge_on_device()
        check(); check(lanes=lanes)
        assert host.merge_route_stats(reset=True) == dict(device=6, host_declined=0, host_overflow=0, buckets_declined=0)
        g.merge_on_device(max_partitions=1)
        check(); check(lanes=lanes)
        r = host.merge_route_stats(reset=True)
        # (a contig whose every bucket happens to be decided by one partition stays on the device route)
        assert r["device"] + r["host_declined"] == 6 and r["host_declined"] >= 2 and r["buckets_declined"] >= r["host_declined"] and r["host_overflow"] == 0
        g.merge_on_device(False)
        check(lanes=lanes)
        assert host.merge_route_stats()["device"] == 0
    finally:
        for c in lanes:
            c.set_gate(None)
            c.close()
        gate.close()
        g.free()


def test_sort_slot_streamed_range_cut_straight_to_a_closing_segment(ctx):
    """A segment above CAP whose FIRST partition leaves 16 members or fewer on the slot's side: the closing rank is then read from global
    memory, never from LDS — at lo == 0 (the pivot is the 12th largest key: slots 0 .. 5) and at lo != 0 (the 12th smallest: the last slots).
    Distinct keys; the median of three is planted at the middle position between the largest key at position 1 and the smallest at n - 1."""
    n = 2 * CAP + 5

    def planted(pivot_val):
        k = np.random.default_rng(3).permutation(n).astype(np.uint32)
        for pos, val in ((1, n - 1), (n - 1, 0), (n // 2, pivot_val)):
            j = int(np.nonzero(k == val)[0][0])
            k[j], k[pos] = k[pos], k[j]
        return k

    for keys, slots in ((planted(n - 12), list(range(6))), (planted(11), list(range(n - 6, n)))):
        for p in slots:
            assert host.sort_select_rounds(keys, p) == 1                  # one partition, then the closing segment
        off = np.arange(len(slots) + 1, dtype=np.uint64) * n
        for max_partitions in (0, 1):                                     # also within a bound of one
            idx, declined = ctx.sort_slot(np.tile(keys, len(slots)), off, np.asarray(slots, np.uint64), max_partitions)
            assert not declined.any()
            assert idx.tolist() == [host.sort_select_check(keys, p)[0] for p in slots]
