"""Resident shards built on the device from BAM batches (csvgpu_shard_builder_*, api/shard_build.hip): whatever the batches, the cuts, the
anchors, the reserve and the route a batch takes (the device's unpacking, or the host parser's arrays), the finished shard is the one
csvgpu_shard_upload makes of the same records — its reads, names, hashes and sizes byte for byte (csvgpu_shard_fetch_*), and everything the
chromosome pipeline computes on it: signatures, labels, counts, the depth map at every position, the alignment intervals. The expected
records come from tests/bam_unpack_inputs.py (the host reader's rules in Python); the packed sequences are read back through
csvgpu_alt_bases_resident against the rule of tests/test_gpu_alt_bases.py."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bam_py
import bam_unpack_inputs as inp
from contextsv_amd import CsvError, Reads, _lib, host
from test_gpu_alt_bases import py_alt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = _lib.SB_SEQ | _lib.SB_NAMES | _lib.SB_NAME_HASH
DEPTH_LEN = 3000
M, I, D, S = 0, 1, 2, 4


# ---- streams of this file (records through inp.record: flags and qualities the scan keeps, operations long enough to be signatures) ---------
def signal_stream(n=48, seed=21):
    rng = np.random.default_rng(seed)
    recs = []
    for k in range(n):
        cigar = [((20 + k % 7) << 4) | M, ((50 + 10 * (k % 3)) << 4) | (I, D, S)[k % 3], ((30 + k % 5) << 4) | M, ((55 + k % 4) << 4) | D, (25 << 4) | M]
        recs.append(inp.record(rng, pos=40 + 11 * (k // 2), qname=b"sig%d" % k, cigar=cigar[: 3 + 2 * (k % 2)], l_seq=k % 7, mapq=60 if k % 9 else 5,
                               flag=(0, 16, 0x800, 0)[k % 4]))
    return b"".join(recs)


def three_records(positions):
    rng = np.random.default_rng(3)
    cig = [(100 << 4) | M, (60 << 4) | D, (100 << 4) | M]
    return [inp.record(rng, pos=p, qname=b"t%d" % k, cigar=cig, l_seq=4, mapq=60, flag=0) for k, p in enumerate(positions)]


# ---- the two routes and their comparison -------------------------------------------------------------------------------------------------------
def pipeline_outputs(ctx, sh):
    """csvgpu_chr_pipeline_fetch + the depth map at every position (and beyond) + the alignment intervals"""
    cap = 1 << 14
    sig, lab = np.zeros(cap, _lib.SIG_DTYPE), np.zeros(cap, np.int32)
    res = _lib.csv_chr_result()
    ctx._check(ctx.lib.csvgpu_chr_pipeline_fetch(ctx.h, sh.h, 50, 20, 0.1, 0.1, C.byref(res), sig.ctypes.data, lab.ctypes.data, cap))
    n = sh.n_reads
    iv = [np.zeros(max(n, 1), np.int32) for _ in range(3)]
    ctx._check(ctx.lib.csvgpu_aln_intervals_resident(ctx.h, sh.h, *[a.ctypes.data for a in iv]))
    return dict(counts=(res.n_sig, res.n_del, res.n_ins, res.depth_sum, res.depth_nonzero, res.min_pts, res.mean_cov),
                sig=sig[: res.n_sig].tobytes(), lab=lab[: res.n_sig].tobytes(), depth=sh.depth_lookup(np.arange(sh.depth_len + 5)).tobytes(),
                ref_end=iv[0][:n].tobytes(), q_start=iv[1][:n].tobytes(), q_end=iv[2][:n].tobytes())


_REFERENCE = {}


def reference(ctx, key, exp, depth_len=DEPTH_LEN):
    """the upload route's outputs for the expected records, computed once per key"""
    if key not in _REFERENCE:
        up = ctx.upload(Reads(exp["pos"], exp["flag"], exp["mapq"], exp["cigar_off"], exp["cigar"]), depth_len)
        try:
            back = up.fetch_reads()
            assert up.sizes() == dict(n_reads=exp["n_kept"], n_cigar=len(exp["cigar"]), n_seq=0, n_name=0)
            _REFERENCE[key] = dict(pipeline_outputs(ctx, up), reads={f: getattr(back, f).tobytes() for f in ("pos", "flag", "mapq", "cigar_off", "cigar")})
        finally:
            up.free()
    return _REFERENCE[key]


def same_as_upload(ctx, sh, key, exp, want=ALL, depth_len=DEPTH_LEN):
    ref = reference(ctx, key, exp, depth_len)
    assert sh.sizes() == dict(n_reads=exp["n_kept"], n_cigar=len(exp["cigar"]), n_seq=len(exp["seq"]) if want & _lib.SB_SEQ else 0,
                              n_name=len(exp["name"]) if want & _lib.SB_NAMES else 0)
    back = sh.fetch_reads()
    for f in ("pos", "flag", "mapq", "cigar_off", "cigar"):
        assert getattr(back, f).tobytes() == ref["reads"][f] == exp[f].tobytes(), f
    if want & (_lib.SB_NAMES | _lib.SB_NAME_HASH):
        nm = sh.fetch_names(want_names=bool(want & _lib.SB_NAMES), want_hashes=bool(want & _lib.SB_NAME_HASH))
        if want & _lib.SB_NAMES:
            assert np.array_equal(nm["name_off"], exp["name_off"]) and nm["name"].tobytes() == exp["name"].tobytes() and nm["names"] == exp["names"]
        if want & _lib.SB_NAME_HASH:
            assert np.array_equal(nm["name_hash"], exp["name_hash"])
    if want & _lib.SB_SEQ and exp["n_kept"]:                                   # every record's whole sequence, pad nibble included
        nb = np.diff(exp["seq_off"]).astype(np.int64)
        got = ctx.alt_bases(sh, np.arange(exp["n_kept"]), np.zeros(exp["n_kept"]), 2 * nb)
        raw = exp["seq"].tobytes()
        for r in range(exp["n_kept"]):
            a = int(exp["seq_off"][r] - exp["seq_off"][0])
            assert got[r] == py_alt(raw[a:a + int(nb[r])], 0, 2 * int(nb[r])), r
    out = pipeline_outputs(ctx, sh)
    for k, v in out.items():
        assert v == ref[k], k
    assert pipeline_outputs(ctx, sh) == out                                    # and again on the same shard


def append_in_batches(b, stream, cuts, every=None, tid=-1, end=0):
    """the stream in batches cut at `cuts` (any byte offsets); the caller carries [consumed, len) into the next batch -> counts per batch"""
    carry, prev, out = b"", 0, []
    for cut in list(cuts) + [len(stream)]:
        chunk, prev = carry + stream[prev:cut], cut
        offs = inp.walk(chunk)[0]
        anchors = ([0] if every is None or not offs else offs[::every]) if chunk else []
        rc, c = b.append_bam(chunk, anchors, tid, end)
        assert rc == 0, c
        out.append(c)
        carry = chunk[c["consumed"]:]
        if c["stopped"]:
            return out
    assert carry == b""
    return out


def cuts_for(stream, n_batches, into):
    offs = inp.walk(stream)[0]
    return [offs[len(offs) * j // n_batches] + into for j in range(1, n_batches)]


# ---- 1. batches --------------------------------------------------------------------------------------------------------------------------------
STREAMS = {"plain": lambda: inp.plain_stream(60), "cg": lambda: inp.cg_stream()[0], "signal": signal_stream}


@pytest.mark.parametrize("name", sorted(STREAMS))
@pytest.mark.parametrize("n_batches", [1, 2, 3, 7])
def test_batches(ctx, name, n_batches):
    stream = STREAMS[name]()
    exp = inp.expected(stream)
    assert exp["n_kept"] >= 28
    if name == "signal":
        assert reference(ctx, name, exp)["counts"][0] > 20 and reference(ctx, name, exp)["counts"][1] > 5          # signatures, deletions among them
    for into in ((0,) if n_batches == 1 else (0, 1, 5, 33)):
        for every in (None, 7):
            b = ctx.shard_builder(ALL)
            counts = append_in_batches(b, stream, cuts_for(stream, n_batches, into), every)
            assert len(counts) == n_batches and sum(c["n_kept"] for c in counts) == exp["n_kept"]
            assert b.sizes() == dict(n_reads=exp["n_kept"], n_cigar=len(exp["cigar"]), n_seq=len(exp["seq"]), n_name=len(exp["name"]))
            sh = b.finish(DEPTH_LEN)
            try:
                same_as_upload(ctx, sh, name, exp)
            finally:
                sh.free()


def test_contig_filter_across_batches(ctx):
    """tid and end as the reader's readContig passes them: a leading batch that keeps nothing, a kept run that ends inside a batch (stopped:
    the caller appends no more), a run that ends with the stream"""
    stream = inp.filter_stream()
    offs = inp.walk(stream)[0]
    seen = set()
    for tid, end in ((1, 1000), (1, 35), (1, 10), (2, 1000), (0, 1 << 31), (3, 1000), (-1, 0), (0, 900)):
        exp = inp.expected(stream, tid, end)
        for cut in (offs[2], offs[3], offs[5] + 9, offs[9]):
            b = ctx.shard_builder(ALL)
            counts = append_in_batches(b, stream, [cut], every=2, tid=tid, end=end)
            assert sum(c["n_kept"] for c in counts) == exp["n_kept"] and counts[-1]["stopped"] == exp["stopped"]
            seen.add((counts[0]["n_kept"] == 0 and len(counts) == 2 and counts[1]["n_kept"] > 0, counts[0]["stopped"]))
            sh = b.finish(DEPTH_LEN)
            try:
                same_as_upload(ctx, sh, ("filter", tid, end), exp)
            finally:
                sh.free()
    assert (True, False) in seen and (False, True) in seen          # a first batch that kept nothing before one that did; a run that ended in the first batch


# ---- 2. growth ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reserve", [None, (1, 1, 1, 1)])
def test_growth_across_a_long_record(ctx, reserve):
    stream, at = inp.long_cigar_stream(n_small=300, n_ops=70_000)
    exp = inp.expected(stream)
    offs = exp["rec_off"]
    assert int(np.diff(exp["cigar_off"])[at]) == 70_000 and 100 < at < 200
    b = ctx.shard_builder(ALL, reserve)
    assert b.sizes() == dict(n_reads=0, n_cigar=0, n_seq=0, n_name=0)
    done = 0
    for a, z in ((0, 100), (100, 200), (200, 301)):
        rc, c = b.append_bam(stream[offs[a]:offs[z] if z < 301 else len(stream)], [0, offs[a + 50] - offs[a]])
        assert rc == 0 and c["n_kept"] == z - a
        done = z
        assert b.sizes() == dict(n_reads=done, n_cigar=int(exp["cigar_off"][done]), n_seq=int(exp["seq_off"][done]), n_name=int(exp["name_off"][done]))
    sh = b.finish(DEPTH_LEN)
    try:
        same_as_upload(ctx, sh, "long", exp)
    finally:
        sh.free()


# ---- 3. tail alignment -------------------------------------------------------------------------------------------------------------------------
def test_every_tail_alignment_at_a_batch_boundary(ctx):
    stream = inp.alignment_stream()
    exp = inp.expected(stream)
    offs = exp["rec_off"]
    residues = lambda k: (int(exp["cigar_off"][k]) % 4, int(exp["seq_off"][k]) % 4, int(exp["name_off"][k]) % 4)
    need, cuts = {(a, r) for a in range(3) for r in range(4)}, []
    for k in range(1, len(offs)):
        new = {(a, r) for a, r in enumerate(residues(k))} & need
        if new:
            cuts.append(k)
            need -= new
    assert not need and len(cuts) <= 12, (need, cuts)
    for k in cuts:
        b = ctx.shard_builder(ALL)
        append_in_batches(b, stream, [offs[k]], every=5)
        assert b.sizes()["n_reads"] == exp["n_kept"]
        sh = b.finish(DEPTH_LEN)
        try:
            same_as_upload(ctx, sh, "alignment", exp)
        finally:
            sh.free()
    # the same boundaries with the second batch through the host parser's arrays
    for k in cuts[:4]:
        first, second = inp.expected(stream[:offs[k]]), inp.expected(stream[offs[k]:])
        b = ctx.shard_builder(ALL)
        assert b.append_bam(stream[:offs[k]], [0])[0] == 0
        b.append_host(Reads(second["pos"], second["flag"], second["mapq"], second["cigar_off"], second["cigar"]), second["seq_off"], second["seq"],
                      second["name_off"], second["name"], second["name_hash"])
        assert b.sizes()["n_reads"] == first["n_kept"] + second["n_kept"]
        sh = b.finish(DEPTH_LEN)
        try:
            same_as_upload(ctx, sh, "alignment", exp)
        finally:
            sh.free()


# ---- 4. sortedness -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("positions", [(100, 300, 200), (100, 200, 300)], ids=["unsorted", "sorted"])
def test_sortedness_is_known_across_batches(ctx, positions):
    recs = three_records(positions)
    stream = b"".join(recs)
    exp = inp.expected(stream)
    assert list(exp["pos"]) == list(positions)
    for cuts in ([], [len(recs[0]) + len(recs[1])], [len(recs[0])], [len(recs[0]), len(recs[0]) + len(recs[1])]):
        b = ctx.shard_builder(0)
        append_in_batches(b, stream, cuts)
        sh = b.finish(DEPTH_LEN)
        try:
            same_as_upload(ctx, sh, ("three", positions), exp, want=0)
        finally:
            sh.free()
    # the third record through the host parser's arrays: the same word
    third = inp.expected(recs[2])
    b = ctx.shard_builder(0)
    assert b.append_bam(recs[0] + recs[1], [0])[0] == 0
    b.append_host(Reads(third["pos"], third["flag"], third["mapq"], third["cigar_off"], third["cigar"]))
    sh = b.finish(DEPTH_LEN)
    try:
        same_as_upload(ctx, sh, ("three", positions), exp, want=0)
    finally:
        sh.free()


# ---- 5. declined, then the host parser's arrays ------------------------------------------------------------------------------------------------
def test_declined_batch_then_host_arrays(ctx):
    recs = inp.refusal_records()
    good = b"".join(recs)
    exp = inp.expected(good)
    A, B, Cc = b"".join(recs[:4]), b"".join(recs[4:8]), b"".join(recs[8:])
    eB = inp.expected(B)
    host_args = (Reads(eB["pos"], eB["flag"], eB["mapq"], eB["cigar_off"], eB["cigar"]), eB["seq_off"], eB["seq"], eB["name_off"], eB["name"], eB["name_hash"])
    bad_batches = [(s[len(A):len(A) + len(B)], [0], reason, at - len(A)) for _, s, reason, at in inp.refusal_streams()]
    bad_batches.append((B, [0, len(recs[4]) + 7], inp.ANCHOR, len(recs[4]) + 7))                      # valid bytes, an anchor inside a record
    for bad, anchors, reason, at in bad_batches:
        b = ctx.shard_builder(ALL)
        assert b.append_bam(A, [0])[0] == 0
        before = b.sizes()
        rc, c = b.append_bam(bad, anchors)
        assert rc == 1 and (c["reason"], c["offset"]) == (reason, at) and c["n_kept"] == 0, c
        assert b.sizes() == before                                                                     # nothing appended
        for k in (1, 3, 5):                                                                            # a wanted array that is null
            args = list(host_args)
            args[k] = args[k + 1 if k < 5 else k] = None
            with pytest.raises(CsvError) as ei:
                b.append_host(*args)
            assert ei.value.status == _lib.CSV_EINVAL and b.sizes() == before
        b.append_host(*host_args)
        assert b.sizes()["n_reads"] == 8
        assert b.append_bam(Cc, [0])[0] == 0
        sh = b.finish(DEPTH_LEN)
        try:
            same_as_upload(ctx, sh, "refusal records", exp)
        finally:
            sh.free()
    b = ctx.shard_builder(ALL)                                                                         # and the three valid batches
    for part in (A, B, Cc):
        assert b.append_bam(part, [0])[0] == 0
    sh = b.finish(DEPTH_LEN)
    try:
        same_as_upload(ctx, sh, "refusal records", exp)
    finally:
        sh.free()


# ---- 6. empty ----------------------------------------------------------------------------------------------------------------------------------
def test_empty_builder(ctx):
    exp = inp.expected(b"")
    assert exp["n_kept"] == 0
    for empties in (0, 3):
        b = ctx.shard_builder(ALL)
        for _ in range(empties):
            rc, c = b.append_bam(b"", [])
            assert rc == 0 and c["n_kept"] == 0
        b.append_host(Reads(*(exp[f] for f in ("pos", "flag", "mapq", "cigar_off", "cigar"))), exp["seq_off"], exp["seq"], exp["name_off"], exp["name"], exp["name_hash"])
        sh = b.finish(DEPTH_LEN)
        try:
            same_as_upload(ctx, sh, "empty", exp)
            assert ctx.alt_bases(sh, [], [], []) == []
        finally:
            sh.free()
    b = ctx.shard_builder(0)                          # a builder that is dropped, not finished
    assert b.append_bam(inp.plain_stream(5), [0])[0] == 0
    b.destroy()
    with pytest.raises(ValueError):
        b.sizes()


# ---- 7. failed growth --------------------------------------------------------------------------------------------------------------------------
_INJECT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import contextsv_amd as cs
from contextsv_amd import _lib
import bam_unpack_inputs as inp
import test_gpu_shard_build as t
stream = inp.plain_stream(60)
exp = inp.expected(stream)
cut = exp["rec_off"][30]
with cs.Context(0) as ctx:
    b = ctx.shard_builder(t.ALL)
    assert b.append_bam(stream[:cut], [0])[0] == 0
    before = b.sizes()
    second = np.frombuffer(stream[cut:], np.uint8)
    dev = ctx.lib.csvgpu_dev_alloc(ctx.h, len(second))          # (a guarded allocation itself: made before the hook is armed)
    assert dev
    ctx._check(ctx.lib.csvgpu_upload(ctx.h, dev, second.ctypes.data, len(second)))
    for n_fail in (1, 1, 1):
        ctx.lib.csvgpu_test_fail_next_alloc(n_fail)
        try:
            b.append_bam_ptr(dev, len(second), [0])
            raise SystemExit("the injected allocation failure did not surface")
        except cs.CsvError as e:
            assert e.status == _lib.CSV_ENOMEM and "shard builder growth" in str(e), str(e)
        assert b.sizes() == before
    ctx.lib.csvgpu_test_fail_next_alloc(0)
    rc, c = b.append_bam_ptr(dev, len(second), [0])             # the same append again
    assert rc == 0 and c["n_kept"] == 30
    ctx.lib.csvgpu_dev_free(ctx.h, dev)
    sh = b.finish(t.DEPTH_LEN)
    t.same_as_upload(ctx, sh, "plain", exp)
    sh.free()
print("ok")
"""


def test_failed_growth_in_the_testhooks_build():
    """csvgpu_test_fail_next_alloc(1) in front of an append that must grow (libcsvgpu_testhooks.so, in a child process): CSV_ENOMEM, the sizes
    unchanged — three times, so that arrays grown by an earlier attempt are met again —, then the same append succeeds and the shard is the
    upload route's"""
    env = dict(os.environ, CSVGPU_LIB=os.path.join(ROOT, "contextsv_amd", "lib", "libcsvgpu_testhooks.so"))
    r = subprocess.run([sys.executable, "-c", _INJECT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- 8. hashes ---------------------------------------------------------------------------------------------------------------------------------
def test_name_hashes_in_place(ctx):
    rng = np.random.default_rng(12)
    lens = (0, 1, 7, 8, 9, 254)
    names = [bytes(rng.integers(33, 127, n, dtype=np.uint8)) for n in lens]
    cig = [(80 << 4) | M]
    recs = [inp.record(rng, pos=10 + 5 * k, qname=nm, cigar=cig, l_seq=0, mapq=60, flag=0) for k, nm in enumerate(names)]
    recs += [inp.record(rng, pos=100 + 5 * k, qname=names[k], cigar=cig, l_seq=0, mapq=60, flag=0x800) for k in (1, 3, 5)]   # supplementary records of three of them
    stream = b"".join(recs)
    exp = inp.expected(stream)
    want = host.string_hashes([nm.decode() for nm in names + [names[1], names[3], names[5]]])
    b = ctx.shard_builder(_lib.SB_NAME_HASH)
    append_in_batches(b, stream, [len(recs[0]) + len(recs[1]) + 3])
    sh = b.finish(DEPTH_LEN)
    up = ctx.upload(Reads(exp["pos"], exp["flag"], exp["mapq"], exp["cigar_off"], exp["cigar"]), DEPTH_LEN)
    try:
        same_as_upload(ctx, sh, "hashes", exp, want=_lib.SB_NAME_HASH)
        assert np.array_equal(sh.fetch_names(want_names=False)["name_hash"], want)
        with pytest.raises(CsvError):
            sh.fetch_names(want_hashes=False)                     # no names kept
        with pytest.raises(CsvError):
            up.fetch_names(want_names=False)                      # no hashes yet
        up.set_qname_hash(want)
        assert np.array_equal(up.fetch_names(want_names=False)["name_hash"], want)
        supp = np.unique(want[6:])
        for s in (sh, up):
            s.pipeline()
        got, ref = ctx.split_order([sh], 20, supp), ctx.split_order([up], 20, supp)
        assert len(ref[0]) == 3 and np.array_equal(got[0], ref[0])
    finally:
        sh.free()
        up.free()
