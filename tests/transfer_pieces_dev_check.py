"""Body of tests/test_gpu_transfer_pieces.py::test_vcf_host_form_against_device_form_beyond_two_pieces (run as a script, torch first: torch
finds no device once the product library's copy of the HIP runtime is up in the process). One VCF text of more than two pieces of the
page-locked block (the lines of tests/test_snp_io.py's generator, repeated at positions further along) through csvgpu_vcf_snp_parse and
through csvgpu_vcf_snp_parse_dev on torch tensors: the same counts and arrays, and every generated line counted."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch.cuda.set_device(0)
import contextsv_amd as cs  # noqa: E402
import vcf_parse_inputs as inp  # noqa: E402

P = 4 << 20                      # kPiece of contextsv_amd/csrc/api/glue.hpp
SPAN, REPEATS = 400_000, 120

base = [l.split("\t", 2) for _, l in inp.snp_lines(np.random.default_rng(23), "chr1", 1400, SPAN)]
lines = ["%s\t%d\t%s" % (chrom, int(pos) + r * SPAN, rest) for r in range(REPEATS) for chrom, pos, rest in base]
text = ("\n".join(lines) + "\n").encode()
assert len(text) > 2 * P and len(lines) == len(base) * REPEATS >= 1400 * REPEATS

with cs.Context(0) as ctx:
    h = ctx.vcf_snp_parse(text)
    assert not h["declined"] and h["n_lines"] == len(lines) and h["stop_off"] == inp.NO_STOP, {k: h[k] for k in ("declined", "n_lines", "stop_off")}
    n, d = h["n_kept"], h["n_deferred"]
    assert n > len(lines) // 2 and len(h["pos"]) == n and len(h["defer_off"]) == d
    view = {k: torch.zeros(d if k == "defer_off" else n, dtype=torch.float64 if k == "value" else torch.int32, device="cuda")
            for k in ("line_off", "chrom_len", "pos", "value", "defer_off")}
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    rc, c = ctx.vcf_snp_parse_dev(d_text, view)
    assert rc == 0 and all(c[k] == h[k] for k in ("n_lines", "n_kept", "n_deferred", "stop_off")), (rc, c)
    for k in ("line_off", "chrom_len", "pos", "defer_off"):
        assert np.array_equal(h[k], view[k].cpu().numpy().view(np.uint32)), k
    assert np.array_equal(h["value"], view["value"].cpu().numpy(), equal_nan=True)
    assert int(h["line_off"][-1]) > 2 * P                                   # kept lines in the third piece of the text
print("transfer_pieces_dev ok: %d lines, %d bytes, %d kept, %d deferred" % (len(lines), len(text), n, d))
