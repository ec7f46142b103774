"""Body of tests/test_gpu_bgzf_inflate.py::test_every_block_kind_on_device_tensors (run as a script, torch first: torch finds no device
once the product library's copy of the HIP runtime is up in the process)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch.cuda.set_device(0)
import contextsv_amd as cs  # noqa: E402
import inflate_inputs as inp  # noqa: E402

cases = inp.zlib_cases()
comp, blocks, out = inp.layout(cases)
d_comp = torch.from_numpy(comp.copy()).cuda()
d_out = torch.from_numpy(out.copy()).cuda()
d_status = torch.full((len(blocks),), 0xFF, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
with cs.Context(0) as ctx:
    n_declined = ctx.bgzf_inflate_dev(d_comp, blocks, d_out, d_status)
    got, status = d_out.cpu().numpy(), d_status.cpu().numpy()
assert n_declined == 0 and not status.any(), (n_declined, [cases[i].name for i in status.nonzero()[0]][:10])
wrong = [c.name for c, b in zip(cases, blocks) if got[int(b["out_off"]): int(b["out_off"]) + int(b["out_len"])].tobytes() != c.data]
assert not wrong, wrong[:10]
assert inp.guards_intact(got, blocks), "bytes outside the members' output ranges were written"
assert (d_comp.cpu().numpy() == comp).all()
print("inflate_dev ok: %d members" % len(cases))
