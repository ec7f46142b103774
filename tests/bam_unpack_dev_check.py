"""Body of tests/test_gpu_bam_unpack.py::test_device_tensors_to_the_pipeline (run as a script, torch first: torch finds no device once the
product library's copy of the HIP runtime is up in the process). A BAM's BGZF members are inflated by csvgpu_bgzf_inflate_dev, the decoded
bytes unpacked by csvgpu_bam_unpack_dev where they lie, the arrays wrapped by csvgpu_shard_wrap_dev and run through the chromosome
pipeline: signatures, labels and depth must equal those of csvgpu_shard_upload on the host reader's arrays."""
import os
import struct
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch.cuda.set_device(0)
import contextsv_amd as cs  # noqa: E402
from contextsv_amd import _lib, host  # noqa: E402
import bam_py  # noqa: E402
import bam_unpack_inputs as inp  # noqa: E402
import synth_small as ss  # noqa: E402
import tempfile  # noqa: E402

reads, depth_len = ss.random_shard(321, n_reads=600, mean_ops=30, big_frac=0.1, chr_len=80_000)
order = np.argsort(reads.pos, kind="stable")
recs = []
for k, i in enumerate(order):
    a, b = int(reads.cigar_off[i]), int(reads.cigar_off[i + 1])
    recs.append(bam_py.encode_record(0, int(reads.pos[i]), int(reads.mapq[i]), int(reads.flag[i]), b"q%d" % k, [int(w) for w in reads.cigar[a:b]],
                                     force_cg=(k % 50 == 7)))
stream = b"".join(recs)
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "in.bam")
bam_py.write_bam(path, ["c0"], [depth_len], inp.index_entries(stream), block_payload=0x8000)
want = host.BamFile(path).read_contig("c0")["reads"]

# the member table of the file (header block(s) included: the records start behind the BAM header in the decoded bytes)
raw = open(path, "rb").read()
blocks, o, out_off = [], 0, 0
while o < len(raw):
    bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
    crc, isize = struct.unpack_from("<II", raw, o + bsize - 8)
    blocks.append((o + 18, out_off, bsize - 26, isize, crc, 0))
    o += bsize
    out_off += isize
blocks = np.array(blocks, _lib.BGZF_BLOCK_DTYPE)
head = 12 + 4 + 3 + 4                                                   # magic, l_text, n_ref, one reference "c0"
assert out_off == head + len(stream)

d_comp = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
d_bytes = torch.zeros(out_off, dtype=torch.uint8, device="cuda")
d_status = torch.full((len(blocks),), 0xFF, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
with cs.Context(0) as ctx:
    assert ctx.bgzf_inflate_dev(d_comp, blocks, d_bytes, d_status) == 0
    d_records = d_bytes[head:]                                          # (an odd offset: the stream is not dword-aligned)
    n, m = want.n_reads, want.n_cigar
    out = dict(pos=torch.zeros(n, dtype=torch.int32, device="cuda"), flag=torch.zeros(n, dtype=torch.int16, device="cuda"),
               mapq=torch.zeros(n, dtype=torch.uint8, device="cuda"), cigar_off=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
               cigar=torch.zeros(m, dtype=torch.int32, device="cuda"), name_hash=torch.zeros(n, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    offs = inp.walk(stream)[0]
    rc, c = ctx.bam_unpack_dev(d_records, offs[::16], out, tid=0, end=depth_len)
    assert rc == 0 and (c["n_kept"], c["n_cigar"], c["consumed"], c["stopped"]) == (n, m, len(stream), False), c
    assert np.array_equal(out["pos"].cpu().numpy(), want.pos) and np.array_equal(out["cigar"].cpu().numpy().view(np.uint32), want.cigar)
    assert np.array_equal(out["cigar_off"].cpu().numpy().view(np.uint64), want.cigar_off)
    assert np.array_equal(out["name_hash"].cpu().numpy().view(np.uint64), host.string_hashes(["q%d" % k for k in range(n)]))
    sh = ctx.wrap_device(out["pos"], out["flag"], out["mapq"], out["cigar_off"], out["cigar"], depth_len)
    res = sh.pipeline(eps=0.1, min_pts_pct=0.1)
    got = sh.fetch(res, want_depth=True)
    sh.free()
    up = ctx.upload(want, depth_len)
    res2 = up.pipeline(eps=0.1, min_pts_pct=0.1)
    ref = up.fetch(res2, want_depth=True)
    up.free()
    # the stream and the byte outputs at every address % 4 (the host-pointer form stages both at aligned addresses): (a)'s records
    a_stream = inp.alignment_stream()
    exp = inp.expected(a_stream)
    nk, G = exp["n_kept"], 64
    for shift in range(4):
        d_in = torch.full((len(a_stream) + 8,), 0x5A, dtype=torch.uint8, device="cuda")
        d_in[shift:shift + len(a_stream)] = torch.from_numpy(np.frombuffer(a_stream, np.uint8).copy()).cuda()
        guarded = lambda n: torch.full((n + 2 * G,), inp.GUARD, dtype=torch.uint8, device="cuda")
        g_seq, g_name = guarded(len(exp["seq"])), guarded(len(exp["name"]))
        o2 = dict(pos=torch.zeros(nk, dtype=torch.int32, device="cuda"), flag=torch.zeros(nk, dtype=torch.int16, device="cuda"),
                  mapq=torch.zeros(nk, dtype=torch.uint8, device="cuda"), cigar_off=torch.zeros(nk + 1, dtype=torch.int64, device="cuda"),
                  cigar=torch.zeros(len(exp["cigar"]), dtype=torch.int32, device="cuda"),
                  seq_off=torch.zeros(nk + 1, dtype=torch.int64, device="cuda"), seq=g_seq[G + shift:G + shift + len(exp["seq"])],
                  name_off=torch.zeros(nk + 1, dtype=torch.int64, device="cuda"), name=g_name[G + (shift + 1) % 4:G + (shift + 1) % 4 + len(exp["name"])],
                  name_hash=torch.zeros(nk, dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()
        assert (d_in.data_ptr() + shift) % 4 == shift and o2["seq"].data_ptr() % 4 == shift
        rc, c = ctx.bam_unpack_dev(d_in[shift:shift + len(a_stream)], exp["rec_off"][::5], o2)
        assert rc == 0 and c["n_kept"] == nk and c["consumed"] == len(a_stream), c
        for k, bits in (("pos", np.int32), ("flag", np.uint16), ("mapq", np.uint8), ("cigar_off", np.uint64), ("cigar", np.uint32), ("seq_off", np.uint64),
                        ("seq", np.uint8), ("name_off", np.uint64), ("name", np.uint8), ("name_hash", np.uint64)):
            assert np.array_equal(o2[k].cpu().numpy().view(bits), exp[k]), (shift, k)
        for g, lo, n in ((g_seq, G + shift, len(exp["seq"])), (g_name, G + (shift + 1) % 4, len(exp["name"]))):
            h = g.cpu().numpy()
            assert (h[:lo] == inp.GUARD).all() and (h[lo + n:] == inp.GUARD).all(), shift
assert (res.n_sig, res.n_del, res.depth_sum, res.min_pts) == (res2.n_sig, res2.n_del, res2.depth_sum, res2.min_pts) and res.n_sig > 0
for k in ("sig_del", "sig_ins", "label_del", "label_ins", "depth"):
    assert np.array_equal(got[k], ref[k]), k
print("unpack_dev ok: %d records, %d signatures" % (n, res.n_sig))
