"""The per-record rule of the device VCF formatter (contextsv_amd/csrc/vcf_format_core.hpp) on the CPU. `make -C contextsv_amd/csrc
vcf-format-check` builds tools/fuzz/vcf_format_core_check.cpp — a program of its own, under AddressSanitizer + UBSan, linked with the host
writer and the host-backed genome — which holds the core's "%f" against snprintf on directed and 10^7 generated doubles, its digit counts
against printf at every power of ten, and whole lines, assembled into heap blocks of exactly the computed length, against writeVCF's text
and counts on generated and directed call sets. A batch the rule refuses is not compared; where the host throws for it, it must."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def test_core_agrees_with_the_host_writer():
    r = subprocess.run(["make", "-s", "-C", CSRC, "vcf-format-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "vcf_format_core_check"), "10000000", "300", "7"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.stderr.strip() == "", r.stderr[-3000:]
    m = re.search(r"vcf_format_core_check: (\d+) doubles \((\d+) refused\), (\d+) batches, (\d+) calls, (\d+) lines, (\d+) declined \((\d+) thrown by the host\), 0 failures\n$",
                  r.stdout)
    assert m, r.stdout[-2000:]
    doubles, refused, batches, calls, lines, declined, threw = (int(x) for x in m.groups())
    print(r.stdout.strip())
    assert doubles - refused >= 10_000_000 and 0 < refused < 100        # only the directed values at and above 2^63
    assert batches > 1000 and lines > 20_000 and calls > lines
    assert declined > 20 and threw >= 7
