"""Body of tests/test_gpu_vcf_format.py::test_allocation_failure_leaves_the_context_usable (run as a script with CSVGPU_LIB = the test
build): csvgpu_test_fail_next_alloc in front of csvgpu_vcf_format's guarded reservation gives CSV_ENOMEM, in the sizing call and in the
call that writes; the context stays usable and the next call gives the model's text. Not covered: a failure of the arena's own growth
(arena_reserve frees its block before it asks for the larger one and carries no hook): the hook here returns before anything is touched."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import contextsv_amd as cs
from contextsv_amd import _lib
from contextsv_amd.context import ptr
import synth_small as ss
import vcf_format_inputs as vi
import vcf_format_model as vm


def main():
    ctx = cs.Context(0)
    if not hasattr(ctx.lib, "csvgpu_test_fail_next_alloc"):
        sys.exit("csvgpu_test_fail_next_alloc is not in %s: CSVGPU_LIB must name the test build" % _lib.LIB_PATH)
    rng = np.random.default_rng(3)
    seq = vi.random_seq(rng, 5000)
    b = ctx.genome_builder(0)
    b.append(b">chrT test\n" + seq + b"\n")
    genome = b.finish()
    reads, depth_len = ss.random_shard(8, n_reads=400, mean_ops=20, chr_len=8000)
    sh = ctx.upload(reads, depth_len)
    res = sh.pipeline()
    depth = sh.fetch(res, want_depth=True)["depth"]
    calls, alts = vi.random_calls(rng, 200, len(seq))
    contigs = [vi.contig(b"chrT", seq, calls, alts, depth, [(100, 400)])]
    want, want_status, want_counts = vm.model(contigs)
    tab = [(b"chrT", len(calls), sh, ([100], [400]))]
    out = np.zeros(len(want), np.uint8)
    for cap, p in ((0, None), (len(out), ptr(out))):
        ctx.lib.csvgpu_test_fail_next_alloc(1)
        rc, _, _ = ctx.vcf_format_raw(genome, tab, calls, alts, vm.METHOD, cap, p)
        ctx.lib.csvgpu_test_fail_next_alloc(0)
        assert rc == _lib.CSV_ENOMEM, rc
        assert not out.any()
        text, status, counts = ctx.vcf_format(genome, tab, calls, alts)
        assert text == want and np.array_equal(status, want_status) and counts == want_counts
    sh.free()
    genome.free()
    ctx.close()
    print("vcf_format_alloc_check: ok")


if __name__ == "__main__":
    main()
