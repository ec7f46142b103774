"""BAM records unpacked on the device (csvgpu_bam_unpack / _dev, kernels/bamunpack.hip): array for array what tests/bam_unpack_inputs.py
computes in Python from the host reader's rules (tests/test_bam_unpack_inputs.py pins those against the host reader itself on the CPU, and
tests/test_bam_record_core.py has run the per-record decisions against it under the sanitizers). Every output array lies between guard
bytes and carries slack behind its last element: everything outside the kept records' ranges must still hold the guard byte afterwards."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bam_unpack_inputs as inp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 64                      # guard elements on either side of every array
DTYPES = dict(pos=np.int32, flag=np.uint16, mapq=np.uint8, cigar_off=np.uint64, cigar=np.uint32, seq_off=np.uint64, seq=np.uint8,
              name_off=np.uint64, name=np.uint8, name_hash=np.uint64)


class Out:
    """guarded output arrays with room for (n_rec, n_cigar, n_seq, n_name) + slack; `shift` moves the byte arrays off their alignment"""

    def __init__(self, n_rec, n_cigar, n_seq, n_name, slack=3, want=("seq", "name", "name_hash"), shift=0):
        sizes = dict(pos=n_rec, flag=n_rec, mapq=n_rec, cigar_off=n_rec + 1, cigar=n_cigar)
        if "seq" in want:
            sizes.update(seq_off=n_rec + 1, seq=n_seq)
        if "name" in want:
            sizes.update(name_off=n_rec + 1, name=n_name)
        if "name_hash" in want:
            sizes.update(name_hash=n_rec)
        self.full, self.view = {}, {}
        for k, n in sizes.items():
            isz = np.dtype(DTYPES[k]).itemsize
            sh = shift if isz == 1 else 0
            self.full[k] = np.full((n + slack + 2 * G) * isz + 8, inp.GUARD, np.uint8)
            self.view[k] = self.full[k][G * isz + sh:(G + n + slack) * isz + sh].view(DTYPES[k])

    def intact_outside(self, counts):
        """every byte outside the ranges the call owns still holds the guard"""
        n = counts["n_kept"]
        owned = dict(pos=n, flag=n, mapq=n, name_hash=n, cigar_off=n + 1, seq_off=n + 1, name_off=n + 1, cigar=counts["n_cigar"], seq=counts["n_seq"],
                     name=counts["n_name"])
        for k, full in self.full.items():
            lo = self.view[k].ctypes.data - full.ctypes.data
            m = np.ones(len(full), bool)
            m[lo:lo + owned[k] * np.dtype(DTYPES[k]).itemsize] = False
            if not (full[m] == inp.GUARD).all():
                return k
        return None


def _run(ctx, stream, anchors=(0,), tid=-1, end=0, bases=(0, 0, 0), exp=None, **kw):
    """one call into guarded arrays sized by the expectation -> (rc, counts, Out)"""
    exp = inp.expected(stream, tid, end, bases) if exp is None else exp
    out = Out(exp["n_kept"], len(exp["cigar"]), len(exp["seq"]), len(exp["name"]), **kw)
    rc, c = ctx.bam_unpack_into(np.frombuffer(stream, np.uint8), anchors, out.view, tid, end, bases)
    return rc, c, out


def _assert_equal(c, out, exp, want=("seq", "name", "name_hash")):
    for k in ("n_records", "kept_first", "n_kept", "stopped", "consumed"):
        assert c[k] == exp[k], (k, c[k], exp[k])
    assert c["status"] == 0 and c["n_cigar"] == len(exp["cigar"])
    keys = ["pos", "flag", "mapq", "cigar_off", "cigar"] + (["seq_off", "seq"] if "seq" in want else []) + (["name_off", "name"] if "name" in want else []) + \
           (["name_hash"] if "name_hash" in want else [])
    for k in keys:
        got = out.view[k][:len(exp[k])]
        assert np.array_equal(got, exp[k]), (k, np.flatnonzero(got != exp[k])[:5])
    assert out.intact_outside(c) is None, "written outside the kept records' ranges: " + str(out.intact_outside(c))


def _check(ctx, stream, anchors=(0,), tid=-1, end=0, bases=(0, 0, 0), **kw):
    exp = inp.expected(stream, tid, end, bases)
    rc, c, out = _run(ctx, stream, anchors, tid, end, bases, exp=exp, **kw)
    assert rc == 0, (rc, c)
    _assert_equal(c, out, exp, kw.get("want", ("seq", "name", "name_hash")))
    return exp


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_alignment_and_empties(ctx, shift):
    """(a) l_name 1..8 and 255, n_cigar 0, l_seq 0 and odd, the empty name, a NUL inside l_name, name lengths of every residue mod 8 up to
    254; the stream itself and the byte outputs at every alignment (shift)"""
    stream = inp.alignment_stream()
    exp = inp.expected(stream)
    lens = {len(x) for x in exp["names"]}
    assert {n % 8 for n in lens} == set(range(8)) and 254 in lens and 0 in lens and exp["n_kept"] > 40
    assert {(o + 36 + struct.unpack_from("<B", stream, o + 12)[0]) % 4 for o in exp["rec_off"]} == {0, 1, 2, 3}      # the CIGAR sources
    # the stream at address % 4 == shift: a view into a larger aligned buffer
    buf = np.full(len(stream) + 16, 0x5A, np.uint8)
    base = (-buf.ctypes.data) % 4
    view = buf[base + shift: base + shift + len(stream)]
    view[:] = np.frombuffer(stream, np.uint8)
    assert view.ctypes.data % 4 == shift
    out = Out(exp["n_kept"], len(exp["cigar"]), len(exp["seq"]), len(exp["name"]), shift=shift)
    rc, c = ctx.bam_unpack_into(view, [0], out.view)
    assert rc == 0, c
    _assert_equal(c, out, exp)
    anchors = exp["rec_off"][::3]
    rc, c = ctx.bam_unpack_into(view, anchors, out.view)
    assert rc == 0
    _assert_equal(c, out, exp)


def test_outputs_not_wanted(ctx):
    """seq, names and hashes are optional, each on its own"""
    stream = inp.alignment_stream()
    for want in ((), ("seq",), ("name",), ("name_hash",), ("seq", "name_hash")):
        exp = _check(ctx, stream, want=want)
        rc, c, _ = _run(ctx, stream, want=want)
        assert c["n_seq"] == (len(exp["seq"]) if "seq" in want else 0) and c["n_name"] == (len(exp["name"]) if "name" in want else 0)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------------
def test_cg_rule(ctx):
    """(b) the CG tag taken and not taken, behind an aux field of every type, behind malformed and unknown ones"""
    stream, names, taken = inp.cg_stream()
    exp = _check(ctx, stream, anchors=[0])
    n_words = np.diff(exp["cigar_off"]).astype(int)
    n_field = [struct.unpack_from("<H", stream, o + 4 + 12)[0] for o in exp["rec_off"]]
    is_taken = [int(w) != f for w, f in zip(n_words, n_field)]
    assert [i for i, t in enumerate(is_taken) if t] == [i for i in taken if names[i] != "count equal to n_cigar"], [names[i] for i, t in enumerate(is_taken) if t]
    _check(ctx, stream, anchors=exp["rec_off"])


def test_long_cigar_among_many_short(ctx):
    """(b) one 70 000-operation record among 5 000 one-operation records: the gather split across waves, the search over many offsets"""
    stream, at = inp.long_cigar_stream()
    exp = _check(ctx, stream, anchors=[0])
    assert int(np.diff(exp["cigar_off"])[at]) == 70_000 and exp["n_kept"] == 5001
    _check(ctx, stream, anchors=exp["rec_off"][::7], want=())


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------
def test_anchors(ctx):
    """(c) one anchor, one per record, every 7th: the same arrays; an anchor inside a record: declined, anchor missed; not ascending: CSV_EINVAL"""
    from contextsv_amd import CsvError, _lib
    stream = inp.plain_stream(300)
    exp = inp.expected(stream)
    offs = exp["rec_off"]
    for anchors in ([0], offs, offs[::7], [0, offs[-1]], [0, offs[1], offs[299]]):
        _check(ctx, stream, anchors=anchors)
    for bad, where in (([0, offs[5] + 1], offs[5] + 1), ([0, offs[5], offs[9] + 40, offs[200]], offs[9] + 40), (offs[:50] + [offs[50] - 1], offs[50] - 1),
                       ([0, len(stream) - 1], len(stream) - 1)):
        rc, c, out = _run(ctx, stream, anchors=bad, exp=exp)
        assert rc == 1 and (c["reason"], c["offset"]) == (_lib.BAM_ANCHOR, where) and c["consumed"] == 0 and c["n_kept"] == 0, (bad[-2:], c)
        assert out.intact_outside(dict(n_kept=exp["n_kept"], n_cigar=len(exp["cigar"]), n_seq=len(exp["seq"]), n_name=len(exp["name"]))) is None
    for bad in ([0, offs[3], offs[3]], [0, offs[4], offs[2]], [0, len(stream)], []):
        out = Out(exp["n_kept"], len(exp["cigar"]), len(exp["seq"]), len(exp["name"]))
        with pytest.raises(CsvError) as ei:
            ctx.bam_unpack_into(np.frombuffer(stream, np.uint8), bad, out.view)
        assert ei.value.status == _lib.CSV_EINVAL and "bam_unpack" in str(ei.value)
        assert out.intact_outside(dict(n_kept=0, n_cigar=0, n_seq=0, n_name=0)) is None


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------
def test_tail_and_carry(ctx):
    """(d) the stream cut at every offset of the last record's first 40 bytes: consumed is that record's start; two calls with bases equal
    one call"""
    stream = inp.plain_stream(40)
    whole = inp.expected(stream)
    last = whole["rec_off"][-1]
    for cut in range(41):
        part = stream[:last + cut]
        exp = _check(ctx, part, anchors=[0, whole["rec_off"][20]])
        assert exp["consumed"] == last and exp["n_records"] == 39
    # two calls: [0, cut) then the carry + the rest, appended behind the first call's arrays
    cut = whole["rec_off"][17] + 23
    e1 = inp.expected(stream[:cut])
    out = Out(whole["n_kept"], len(whole["cigar"]), len(whole["seq"]), len(whole["name"]))
    rc, c1 = ctx.bam_unpack_into(np.frombuffer(stream[:cut], np.uint8), [0], out.view)
    assert rc == 0 and c1["consumed"] == whole["rec_off"][17] == e1["consumed"] and c1["n_kept"] == 17
    n1 = c1["n_kept"]
    second = {k: v[{"cigar": c1["n_cigar"], "seq": c1["n_seq"], "name": c1["n_name"]}.get(k, n1):] for k, v in out.view.items()}
    rc, c2 = ctx.bam_unpack_into(np.frombuffer(stream[c1["consumed"]:], np.uint8), [0], second, bases=(c1["n_cigar"], c1["n_seq"], c1["n_name"]))
    assert rc == 0 and c2["n_kept"] == 40 - 17 and c2["consumed"] == len(stream) - c1["consumed"]
    both = dict(whole, n_records=c1["n_records"] + c2["n_records"])
    total = dict(c2, n_records=40, n_kept=40, n_cigar=c1["n_cigar"] + c2["n_cigar"], n_seq=c1["n_seq"] + c2["n_seq"], n_name=c1["n_name"] + c2["n_name"],
                 consumed=len(stream))
    _assert_equal(total, out, both)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------------
def test_contig_filter(ctx):
    """(e) an earlier contig's tail in front, unplaced records, pos >= end, a later contig behind, tid = -1"""
    stream = inp.filter_stream()
    offs = inp.expected(stream)["rec_off"]
    for tid, end, first, kept, stopped in ((1, 1000, 3, 5, True), (1, 35, 3, 3, True), (1, 10, 3, 0, True), (2, 1000, 8, 2, True), (0, 1 << 31, 0, 3, True),
                                           (3, 1000, 10, 0, True), (-1, 0, 0, 12, False), (0, 900, 0, 0, True)):
        for anchors in ([0], offs[::2]):
            exp = _check(ctx, stream, anchors=anchors, tid=tid, end=end)
            assert (exp["kept_first"], exp["n_kept"], exp["stopped"]) == (first, kept, stopped), (tid, end)
    # the run of a contig that is the stream's last is not stopped; an unsorted file stops at the first record of another contig
    exp = _check(ctx, stream[:offs[10]], tid=2, end=1000)
    assert (exp["kept_first"], exp["n_kept"], exp["stopped"]) == (8, 2, False)
    swapped = stream[offs[3]:offs[5]] + stream[:offs[3]] + stream[offs[5]:]           # contig 1, 1, then 0, 0, 0, then 1, 1, 1, 2, ...
    exp = _check(ctx, swapped, tid=1, end=1000)
    assert (exp["kept_first"], exp["n_kept"], exp["stopped"]) == (0, 2, True)


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """(f) each of the host's four checks fails at a known record: declined with that reason and offset, nothing written; a refused field
    of a record outside the kept run refuses nothing (the host does not look at it either)"""
    for name, stream, reason, at in inp.refusal_streams():
        with pytest.raises(inp.Declined) as ei:
            inp.expected(stream)
        assert (ei.value.reason, ei.value.offset) == (reason, at), name
        for anchors in ([0], [0, at]):
            out = Out(12, 64, 64, 64)
            rc, c = ctx.bam_unpack_into(np.frombuffer(stream, np.uint8), anchors, out.view)
            assert rc == 1 and (c["reason"], c["offset"]) == (reason, at) and c["consumed"] == 0 and c["n_records"] == 0, (name, c)
            assert out.intact_outside(dict(n_kept=0, n_cigar=0, n_seq=0, n_name=0)) is None, name
    name, stream, reason, at = [r for r in inp.refusal_streams() if r[0] == "l_seq -1"][0]
    patched = stream[:at + 4] + struct.pack("<i", 5) + stream[at + 8:]                   # that record on contig 5: outside the run of contig 0
    exp = _check(ctx, patched, tid=0, end=1 << 30)
    assert exp["n_kept"] == 7 and exp["stopped"]


def test_capacity(ctx):
    """(f) CSV_ECAPACITY returns the exact counts and writes nothing; the sizing call of Context.bam_unpack rests on it"""
    from contextsv_amd import _lib
    stream = inp.plain_stream(50)
    exp = inp.expected(stream)
    sizes = [exp["n_kept"], len(exp["cigar"]), len(exp["seq"]), len(exp["name"])]
    for short in range(4):
        s = list(sizes)
        s[short] -= 4                                            # (slack 3: one below what is needed)
        out = Out(*s)
        rc, c = ctx.bam_unpack_into(np.frombuffer(stream, np.uint8), [0], out.view)
        assert rc == _lib.CSV_ECAPACITY, short
        assert [c["n_kept"], c["n_cigar"], c["n_seq"], c["n_name"]] == sizes and c["consumed"] == exp["consumed"] and c["n_records"] == 50
        assert out.intact_outside(dict(n_kept=0, n_cigar=0, n_seq=0, n_name=0)) is None
    got = ctx.bam_unpack(stream, [0], want_seq=True, want_names=True, want_hashes=True)
    for k in ("pos", "flag", "mapq", "cigar_off", "cigar", "seq_off", "seq", "name_off", "name", "name_hash"):
        assert np.array_equal(got[k], exp[k]), k
    empty = ctx.bam_unpack(b"", [])
    assert empty["n_records"] == 0 and empty["status"] == 0


def test_hashes_equal_the_host_mirror(ctx):
    """the device's name hashes against std::hash<std::string> itself (host.string_hashes), every length 0..254"""
    from contextsv_amd import host
    rng = np.random.default_rng(9)
    names = [bytes(rng.integers(33, 127, n, dtype=np.uint8)) for n in range(255)]
    stream = b"".join(inp.record(rng, pos=k, qname=nm, n_cigar=1, l_seq=0) for k, nm in enumerate(names))
    got = ctx.bam_unpack(stream, [0], want_hashes=True)
    assert np.array_equal(got["name_hash"], host.string_hashes([nm.decode() for nm in names])[:255])


# ---- (g) ---------------------------------------------------------------------------------------------------------------------------------------
def test_device_tensors_to_the_pipeline():
    """(g) inflate_dev -> unpack_dev -> csvgpu_shard_wrap_dev -> chr_pipeline on torch tensors, against csvgpu_shard_upload of the host
    reader's arrays. In a process of its own, torch first (tests/bam_unpack_dev_check.py)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bam_unpack_dev_check.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "unpack_dev ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- (h): through the reader and the run -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate_on_device", [False, True])
def test_reader_with_device_unpack_equals_host_route(tmp_path, inflate_on_device):
    """(h) read_contig with unpack_on_device: array for array what the host route reads, with sequences and names, at window_blocks 1, 5
    and default (batch boundaries inside records: a record of 280 KiB lies in the file), with a CG-tag CIGAR; with and without the inflate
    on the device, on the same context"""
    import test_gpu_bgzf_inflate as tbi
    from contextsv_amd import host
    _, reads, tid, qnames, contig_len = tbi._three_contigs()
    reads, tid, qnames = tbi._with_long_cigar(reads, tid, qnames)
    rng = np.random.default_rng(11)
    l_seq = rng.integers(0, 30, reads.n_reads).astype(np.int32)
    seq_off = np.concatenate([[0], np.cumsum((l_seq + 1) // 2)]).astype(np.uint64)
    seq = rng.integers(0, 256, int(seq_off[-1]), dtype=np.uint8)
    seq[seq_off[1:][l_seq % 2 == 1] - 1] &= 0xF0
    names = ["contig%d" % t for t in range(3)]
    path = str(tmp_path / "reads.bam")
    host.write_bam(path, names, [contig_len] * 3, tid, reads, qnames, seq_off, seq, l_seq, level=1, threads=8)
    bam = host.BamFile(path)
    want = {}
    for t in range(3):
        s = bam.read_contig(names[t], want_seq=True, want_qnames=True, threads=8)
        want[t] = dict(s, reads=tbi._copy_reads(s["reads"]), seq_off=s["seq_off"].copy(), seq=s["seq"].copy())
    assert max(np.diff(want[0]["reads"].cigar_off)) > 65535
    for window in (1, 5, 0):
        for t in (1, 0, 2):
            got = bam.read_contig(names[t], want_seq=True, want_qnames=True, threads=8, window_blocks=window, inflate_on_device=inflate_on_device,
                                  unpack_on_device=True)
            tbi._same_shard(got, want[t])
            # and it was the device that read them: every batch unpacked there, none left to the host parser, cut at anchors from the index
            st = bam.unpack_stats()
            assert st["batches_host"] == 0 and st["batches_device"] >= (2 if window == 1 else 1), (window, t, st)   # (a contig is a few blocks long)
            assert st["records"] == want[t]["reads"].n_reads, (window, t, st)
            assert st["anchors"] > st["batches_device"] + (10 if window == 0 else 0), (window, t, st)
            # with the inflate on the same context the decoded bytes never came to the host; without it they were never on the device before
            assert st["batches_downloaded"] == 0 and st["batches_kept_on_device"] == (st["batches_device"] if inflate_on_device else 0), (window, t, st)
    got = bam.read_contig(names[1], threads=8, unpack_on_device=True)                    # neither sequences nor names
    for f in ("pos", "flag", "mapq", "cigar_off", "cigar"):
        assert np.array_equal(getattr(got["reads"], f), getattr(want[1]["reads"], f)), f
    tbi._same_shard(bam.read_contig(names[1], want_seq=True, want_qnames=True), want[1])   # and back on the host with the same handle
    bam.close()


def test_reader_with_device_unpack_fails_like_the_host_route(tmp_path):
    """(h) refused records and a flipped byte: the same message on both routes (the device declines, the host parser words the refusal),
    and the counters say that this is what happened"""
    import bam_py
    from contextsv_amd import host

    def message(p, **kw):
        bam = host.BamFile(p)
        with pytest.raises(RuntimeError) as ei:
            bam.read_contig("c0", want_seq=True, want_qnames=True, threads=4, **kw)
        st = bam.unpack_stats()
        bam.close()
        return str(ei.value), st

    good = b"".join(inp.refusal_records())
    entries = inp.index_entries(good)
    for k, (name, stream, reason, at) in enumerate(inp.refusal_streams()):
        p = str(tmp_path / ("bad%d.bam" % k))
        # the index of the intact records (one 16 Kbp window each): its chunk begins and linear offsets are the true record starts
        bam_py.write_bam(p, ["c0"], [1 << 28], [(stream, 0, 0, 1, 0)], with_index=False)
        bam_py.write_bam(str(tmp_path / "good.bam"), ["c0"], [1 << 28], entries)
        os.replace(str(tmp_path / "good.bam.bai"), p + ".bai")
        on_host, st = message(p)
        assert on_host == inp.MESSAGES[reason] and st["batches_device"] == st["batches_host"] == 0, name
        for window in (0, 1):
            for inflate in (False, True):
                msg, st = message(p, unpack_on_device=True, inflate_on_device=inflate, window_blocks=window)
                assert msg == on_host, name
                # the device saw the batch and declined it; the host parser worded the refusal (the bytes came down for it)
                assert st["batches_device"] == 0 and st["batches_host"] == 1 and st["batches_downloaded"] == (1 if inflate else 0), (name, st)
    # the intact file of the same records is the device's: the anchors of its index are hit
    os.replace(p + ".bai", str(tmp_path / "good.bam.bai"))
    bam = host.BamFile(str(tmp_path / "good.bam"))
    got = bam.read_contig("c0", unpack_on_device=True)
    st = bam.unpack_stats()
    assert got["reads"].n_reads == 12 and st["batches_device"] == 1 and st["batches_host"] == 0 and st["anchors"] == 12 and st["records"] == 12, st
    bam.close()
    # a flipped byte inside a block behind the header's (64-byte blocks: records straddle them): the inflate fails, on either route with the
    # same message
    src = str(tmp_path / "multi.bam")
    bam_py.write_bam(src, ["c0"], [1 << 28], entries, block_payload=64)
    raw = bytearray(open(src, "rb").read())
    raw[len(raw) * 3 // 4] ^= 0x5A
    p = str(tmp_path / "flip.bam")
    open(p, "wb").write(bytes(raw))
    os.replace(src + ".bai", p + ".bai")
    on_host, _ = message(p)
    assert "BGZF" in on_host or "BAM" in on_host
    for inflate in (False, True):
        assert message(p, unpack_on_device=True, inflate_on_device=inflate)[0] == on_host


def test_run_from_bam_with_device_unpack_gives_the_same_calls(ctx, tmp_path):
    """(h) runBam with the option off and on, and on beside the device inflate: identical calls and per-contig statistics"""
    import test_gpu_bgzf_inflate as tbi
    from contextsv_amd import host, make_hmm
    from hmm_params import WGS_HMM
    contigs, reads, tid, qnames, contig_len = tbi._three_contigs()
    path = str(tmp_path / "reads.bam")
    host.write_bam(path, ["contig%d" % t for t in range(3)], [contig_len] * 3, tid, reads, qnames, level=1, threads=8)
    hmm = make_hmm(**WGS_HMM)
    want, want_tid, st = host.run_bam(ctx, path, hmm, threads=8)
    assert len(want) > 20 and st["n_contigs"] == 3
    stats = lambda s: {k: s[k] for k in ("n_contigs", "n_reads", "n_cigar", "bam_bytes")}
    for kw in (dict(unpack_on_device=True), dict(unpack_on_device=True, inflate_on_device=True)):
        got, got_tid, st_on = host.run_bam(ctx, path, hmm, threads=8, **kw)
        assert got.tobytes() == want.tobytes() and np.array_equal(got_tid, want_tid) and stats(st_on) == stats(st), kw
        # every contig's batches were the device's, cut at anchors from the index; with the inflate beside it the bytes stayed on the device
        assert st_on["unpack_batches_device"] >= 3 and st_on["unpack_batches_host"] == 0 and st_on["unpack_anchors"] > 10 * st_on["unpack_batches_device"], st_on
        assert st_on["unpack_batches_kept_on_device"] == (st_on["unpack_batches_device"] if "inflate_on_device" in kw else 0), st_on
    assert st["unpack_batches_device"] == st["unpack_batches_host"] == 0
