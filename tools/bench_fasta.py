#!/usr/bin/env python
"""The reference genome on the device against the host loader (profiles/device_fasta/).

  python tools/bench_fasta.py --mb 3072 --reps 7 --out profiles/device_fasta/fasta.json

Two generated FASTA files of --mb MiB each, 4 contigs: one wrapped at 60 columns, one unwrapped (a line per contig). Per file, the median of
--reps warm runs with p10 / p90, the settings taking turns inside every repetition:
  host          host.ReferenceGenome(path): the host loader on one thread, the file in the page cache (ReferenceGenome() end to end, off)
  file_on       host.ReferenceGenome(path, load_on_device=True, ctx=ctx): the same end to end with the option on — the mapped file up in
                windows through the page-locked block, names and lengths back
  dev           csvgpu_genome_builder_append_dev with the text resident, in windows of --window-mb: wall time of create + appends + finish, and
                the context's CSV_K_MISC timer (the launches, not the read-backs) as GB/s of text and as a fraction of 8 TB/s over the text
                read three times (line ends, line starts, compaction) plus the bases written
  host_ptr      csvgpu_genome_builder_append from a host array (the upload through the page-locked block included)
  fetch         csvgpu_genome_fetch of --items cuts of a VCF-like length mix (most 1 base, some tens to thousands) against a loop of
                ReferenceGenome.query over the same cuts
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.cuda.set_device(0)
import contextsv_amd as cs  # noqa: E402
from contextsv_amd import host  # noqa: E402

HBM_PEAK = 8e12


def make_text(rng, total, wrapped):
    parts = []
    per = total // 4
    for c in range(4):
        seq = np.frombuffer(b"ACGTACGTACGTACGN", np.uint8)[rng.integers(0, 16, per, dtype=np.uint8)]
        parts.append(np.frombuffer(b">chr%d generated contig\n" % (c + 1), np.uint8))
        if wrapped:
            rows = per // 60
            body = np.full((rows, 61), 0x0A, np.uint8)
            body[:, :60] = seq[: rows * 60].reshape(rows, 60)
            parts.append(body.reshape(-1))
        else:
            parts += [seq, np.frombuffer(b"\n", np.uint8)]
    return np.concatenate(parts)


def stats(xs):
    xs = np.sort(np.asarray(xs, np.float64))
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=3072)
    ap.add_argument("--window-mb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--items", type=int, default=30_000)
    ap.add_argument("--kinds", default="wrapped,unwrapped", help="which of the two files (a profiler run takes one at a time)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    result = dict(mb=a.mb, window_mb=a.window_mb, reps=a.reps, items=a.items, device=torch.cuda.get_device_name(0), files={})
    tmp = tempfile.mkdtemp(prefix="bench_fasta_")
    with cs.Context(0) as ctx:
        for kind in a.kinds.split(","):
            text = make_text(rng, a.mb << 20, kind == "wrapped")
            n = len(text)
            path = os.path.join(tmp, kind + ".fa")
            text.tofile(path)
            d_text = torch.from_numpy(text).cuda()
            torch.cuda.synchronize()
            win = a.window_mb << 20
            t = {k: [] for k in ("host", "file_on", "dev", "dev_kernels", "host_ptr")}
            genome = hg = None
            for rep in range(a.reps + 1):                # (the first repetition warms the arenas and the page cache and is dropped)
                t0 = time.perf_counter()
                g = host.ReferenceGenome(path)
                t["host"].append(time.perf_counter() - t0)
                if hg is not None:
                    hg.close()
                hg = g
                t0 = time.perf_counter()
                g_on = host.ReferenceGenome(path, load_on_device=True, ctx=ctx, window_bytes=win)
                t["file_on"].append(time.perf_counter() - t0)
                st = g_on.device_stats
                assert st["on_device"] == 1 and st["fallback"] == 0 and st["bytes_uploaded"] == n, st
                g_on.close()
                ctx.timing_enable(1)
                ctx.timing_reset()
                t0 = time.perf_counter()
                b = ctx.genome_builder(n)
                for o in range(0, n, win):
                    b.append_ptr(d_text.data_ptr() + o, min(win, n - o))
                gd = b.finish()
                t["dev"].append(time.perf_counter() - t0)
                t["dev_kernels"].append(ctx.timing()["misc"][0] / 1e3)
                ctx.timing_enable(0)
                if genome is not None:
                    genome.free()
                genome = gd
                t0 = time.perf_counter()
                b = ctx.genome_builder(n)
                for o in range(0, n, win):
                    b.append(text[o: o + win])
                b.finish().free()
                t["host_ptr"].append(time.perf_counter() - t0)
            desc = genome.describe()
            bases = desc["total_bases"]
            assert [x.decode() for x in desc["names"]] == ["chr1", "chr2", "chr3", "chr4"] and all(int(L) == hg.getChromosomeLength(nm.decode()) for nm, L in zip(desc["names"], desc["lengths"]))
            # cuts of a VCF-like mix
            L = int(desc["lengths"][0])
            rec = rng.integers(0, 4, a.items).astype(np.uint32)
            length = rng.choice([1, 1, 1, 1, 1, 1, 2, 12, 60, 300, 2500], a.items)
            ps = rng.integers(1, L - 3000, a.items).astype(np.uint32)
            pe = (ps + length - 1).astype(np.uint32)
            names = [nm.decode() for nm in desc["names"]]
            tf = {"fetch_dev": [], "fetch_host_loop": []}
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                got = genome.fetch(rec, ps, pe, mask=True)
                tf["fetch_dev"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                exp = [hg.query(names[r], int(s), int(e)) for r, s, e in zip(rec, ps, pe)]
                tf["fetch_host_loop"].append(time.perf_counter() - t0)
            assert got == exp                            # (the generated bases hold no ambiguity code: the mask changes nothing)
            entry = dict(text_bytes=n, bases=bases, lines=desc["n_lines"])
            for k, xs in list(t.items()) + list(tf.items()):
                entry[k] = stats(xs[1:])
            for k in ("host", "file_on", "dev", "dev_kernels", "host_ptr"):
                entry[k]["text_gb_per_s"] = n / entry[k]["median"] / 1e9
            entry["dev_kernels"]["hbm_fraction"] = (3 * n + bases) / entry["dev_kernels"]["median"] / HBM_PEAK
            result["files"][kind] = entry
            print(kind, json.dumps(entry), flush=True)
            genome.free()
            hg.close()
            os.remove(path)
            del d_text
    os.rmdir(tmp)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
