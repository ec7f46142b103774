"""Body of tests/test_gpu_vcf_parse.py::test_device_tensors_and_the_inflate_seam (run as a script, torch first: torch finds no device once
the product library's copy of the HIP runtime is up in the process). csvgpu_vcf_snp_parse_dev / csvgpu_vcf_af_parse_dev on torch tensors
with the text pointer shifted by 1 to 15 bytes, between guard bytes; and the seam: whole-line text in BGZF members inflated by
csvgpu_bgzf_inflate_dev and parsed where it lies, equal to the host-pointer call."""
import os
import struct
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch.cuda.set_device(0)
import contextsv_amd as cs  # noqa: E402
from contextsv_amd import _lib  # noqa: E402
import bam_py  # noqa: E402
import vcf_parse_inputs as inp  # noqa: E402

G = 64


def guarded(n, itemsize):
    return torch.full(((n + 2 * G) * itemsize,), inp.GUARD, dtype=torch.uint8, device="cuda")


def outputs(n, d, af):
    full = dict(line_off=guarded(n, 4), pos=guarded(n, 4), value=guarded(n, 8), defer_off=guarded(d, 4))
    if not af:
        full["chrom_len"] = guarded(n, 4)
    size = dict(line_off=4, pos=4, value=8, defer_off=4, chrom_len=4)
    count = dict(line_off=n, pos=n, value=n, defer_off=d, chrom_len=n)
    view = {k: t[G * size[k]:(G + count[k]) * size[k]].view(torch.float64 if k == "value" else torch.int32) for k, t in full.items()}
    return full, view, size, count


def check(full, view, size, count, exp, c, rc):
    assert rc == 0 and c["n_kept"] == len(exp["pos"]) and c["n_deferred"] == len(exp["defer_off"]) and c["n_lines"] == exp["n_lines"] and c["stop_off"] == exp["stop_off"], c
    for k, t in view.items():
        got = t.cpu().numpy()
        got = got if k == "value" else got.view(np.uint32)
        assert np.array_equal(got, exp[k], equal_nan=(k == "value")), k
        f = full[k].cpu().numpy()
        assert (f[:G * size[k]] == inp.GUARD).all() and (f[(G + count[k]) * size[k]:] == inp.GUARD).all(), "written outside " + k


text, snps, rng = inp.generated_snp_text()
text = text[:text.index(b"\n", 20_000) + 1] + ("\n".join(l for _, l in inp.DELIBERATE_SNP) + "\n").encode()
gtext, _ = inp.generated_gnomad_text(rng, snps, "chr1")
gtext = gtext[:gtext.index(b"\n", 20_000) + 1]
spos = np.sort(np.array([q for q, l in snps if l.startswith("chr1\t")], np.uint32))
spos = spos[spos <= int(gtext.rstrip(b"\n").rsplit(b"\n", 1)[1].split(b"\t")[1]) - 5]       # a STOP line inside the cut text
exp_s, exp_a = inp.expected_snp(text), inp.expected_af(gtext, "chr1", "AF_nfe=", spos)
assert len(exp_s["pos"]) > 100 and len(exp_s["defer_off"]) == len(inp.DELIBERATE_SNP) and len(exp_a["pos"]) > 20 and exp_a["stop_off"] != inp.NO_STOP

with cs.Context(0) as ctx:
    d_spos = torch.from_numpy(spos.view(np.int32).copy()).cuda()
    for shift in range(1, 16):
        for t, exp, af in ((text, exp_s, False), (gtext, exp_a, True)):
            d_in = torch.full((len(t) + 48,), 0x0A, dtype=torch.uint8, device="cuda")      # line ends all around the text: none of them may count
            base = (-d_in.data_ptr()) % 16
            d_in[base + shift:base + shift + len(t)] = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
            d_text = d_in[base + shift:base + shift + len(t)]
            assert d_text.data_ptr() % 16 == shift
            full, view, size, count = outputs(len(exp["pos"]), len(exp["defer_off"]), af)
            torch.cuda.synchronize()
            rc, c = ctx.vcf_af_parse_dev(d_text, "chr1", "AF_nfe=", d_spos, view) if af else ctx.vcf_snp_parse_dev(d_text, view)
            check(full, view, size, count, exp, c, rc)
    # the seam: members of whole lines -> csvgpu_bgzf_inflate_dev -> csvgpu_vcf_snp_parse_dev, against the host-pointer call
    raw, blocks, o, out_off = b"", [], 0, 0
    cuts = [0] + [text.rindex(b"\n", 0, k) + 1 for k in range(3000, len(text), 3000)] + [len(text)]
    for a, b in zip(cuts, cuts[1:]):
        raw += bam_py.bgzf_block(text[a:b])
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, o + bsize - 8)
        blocks.append((o + 18, out_off, bsize - 26, isize, crc, 0))
        o += bsize
        out_off += isize
    blocks = np.array(blocks, _lib.BGZF_BLOCK_DTYPE)
    assert out_off == len(text) and len(blocks) > 5
    d_comp = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
    d_bytes = torch.zeros(out_off, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(blocks),), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.bgzf_inflate_dev(d_comp, blocks, d_bytes, d_status) == 0
    full, view, size, count = outputs(len(exp_s["pos"]), len(exp_s["defer_off"]), False)
    torch.cuda.synchronize()
    rc, c = ctx.vcf_snp_parse_dev(d_bytes, view)
    check(full, view, size, count, exp_s, c, rc)
    h = ctx.vcf_snp_parse(text)
    assert not h["declined"]
    for k in ("line_off", "chrom_len", "pos", "defer_off"):
        assert np.array_equal(h[k], view[k].cpu().numpy().view(np.uint32)), k
    assert np.array_equal(h["value"], view["value"].cpu().numpy(), equal_nan=True)
print("vcf_parse_dev ok: 15 shifts x 2 forms, seam of %d members" % len(blocks))
