"""Texts for the device VCF parser (csvgpu_vcf_snp_parse / csvgpu_vcf_af_parse) and a plain-Python restatement of the two line rules of
contextsv_amd/csrc/vcf_record_core.hpp, the DEFER rule included. tests/test_vcf_parse_inputs.py holds the restatement against the host
parser and the oracle on the CPU; tests/test_gpu_vcf_parse.py holds the device against the restatement. The generators and headers are
those of tests/test_snp_io.py."""
import re
import struct

import numpy as np

from test_snp_io import GNOMAD_HEADER, HEADER, gnomad_lines, snp_lines, write_vcf  # noqa: F401  (re-exported)

INT32_MIN = -(1 << 31)
NO_STOP = (1 << 64) - 1
GUARD = 0xA5

_INT = re.compile(rb"[+-]?[0-9]{1,9}")
_REAL = re.compile(rb"([+-]?)([0-9]*)(?:\.([0-9]*))?(?:[eE]([+-]?[0-9]+))?")


def tok_int(t: bytes):
    """the integer rule: the whole token is [+-]?[0-9]{1,9}; None = outside it"""
    return int(t) if _INT.fullmatch(t) else None


def tok_real(t: bytes):
    """the real-number rule: at most 64 bytes, [+-]?D*(.D*)?([eE][+-]?D+)? with a digit in front of the exponent, at most 15 digits without
    the leading zeros, exponent less fraction length within +-22; the value is ONE double operation on exact operands. None = outside it."""
    if not t or len(t) > 64:
        return None
    m = _REAL.fullmatch(t)
    if not m:
        return None
    sign, ip, fp, ex = m.group(1), m.group(2), m.group(3) or b"", m.group(4)
    digits = ip + fp
    if not digits:
        return None
    sig = digits.lstrip(b"0")
    if len(sig) > 15:
        return None
    e = (int(ex) if ex else 0) - len(fp)
    if e < -22 or e > 22:
        return None
    w = float(int(sig or b"0"))
    d = w * float(10 ** e) if e >= 0 else w / float(10 ** -e)
    return -d if sign == b"-" else d


def _allele(a: bytes):
    return (len(a) == 1 and a != b"*") or a in (b"<X>", b"<*>")


def is_snp(ref: bytes, alt: bytes):
    if not _allele(ref):
        return False
    return alt == b"." or all(_allele(a) for a in alt.split(b","))


def _format_int(t: bytes):
    """one value of an integer FORMAT field -> int (INT32_MIN: missing) or None (outside the integer rule)"""
    if t in (b"", b"."):
        return INT32_MIN
    return tok_int(t)


def _sample_field(sample: bytes, idx: int):
    f = sample.split(b":")
    return f[idx] if idx < len(f) else b""


def _f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def snp_rule(line: bytes, dp_int=True, ad_int=True):
    """-> ("skip",) | ("defer",) | ("keep", chrom_len, pos, baf)"""
    f = line.split(b"\t")
    if len(f) < 9:
        return ("skip",)
    if not is_snp(f[3], f[4]):
        return ("skip",)
    if f[5] == b".":
        return ("skip",)
    q = tok_real(f[5])
    if q is None:
        return ("defer",)
    if not _f32(q) > 30:
        return ("skip",)
    keys = f[8].split(b":")
    if not dp_int or b"DP" not in keys:
        return ("skip",)
    if len(f) > 10:                                           # a second sample column
        return ("defer",)
    sample = f[9] if len(f) > 9 else b""
    dp = _format_int(_sample_field(sample, keys.index(b"DP")).split(b",")[0])
    if dp is None:
        return ("defer",)
    if dp <= 10:
        return ("skip",)
    if f[6] not in (b".", b"PASS") and b"PASS" not in f[6].split(b";"):
        return ("skip",)
    if not ad_int or b"AD" not in keys:
        return ("skip",)
    ad = _sample_field(sample, keys.index(b"AD")).split(b",")
    if len(ad) < 2:
        return ("skip",)
    a0, a1 = _format_int(ad[0]), _format_int(ad[1])
    if a0 is None or a1 is None:
        return ("defer",)
    pos = tok_int(f[1])
    if pos is None:
        return ("defer",)
    with np.errstate(all="ignore"):
        baf = float(np.float64(a1) / np.float64(_i32(a0 + a1)))
    return ("keep", len(f[0]), pos & 0xFFFFFFFF, baf)


def af_rule(line: bytes, contig: bytes, needle: bytes, sorted_pos, last_pos: int):
    """-> ("skip",) | ("defer",) | ("stop",) | ("keep", pos, af); sorted_pos: a set of the positions"""
    f = line.split(b"\t")
    if len(f) < 8 or f[0] != contig:
        return ("skip",)
    pos = tok_int(f[1])
    if pos is None:
        return ("defer",)
    pos &= 0xFFFFFFFF
    if pos > last_pos:
        return ("stop",)
    if pos not in sorted_pos or not is_snp(f[3], f[4]):
        return ("skip",)
    info = f[7]
    k = info.find(needle)
    while k > 0 and info[k - 1:k] != b";":
        k = info.find(needle, k + 1)
    if k < 0:
        return ("skip",)
    val = re.split(rb"[;,]", info[k + len(needle):], maxsplit=1)[0]
    if not val:
        return ("skip",)
    if val == b".":
        return ("keep", pos, float("nan"))
    d = tok_real(val)
    if d is None:
        return ("defer",)
    v = _f32(d)
    if v <= 0.01 or v >= 0.99:
        return ("skip",)
    return ("keep", pos, v)


def lines_of(text: bytes):
    """(offset, line) of every non-empty line, a trailing '\\r' stripped; the last line may lack its '\\n'"""
    a = 0
    while a < len(text):
        e = text.find(b"\n", a)
        if e < 0:
            e = len(text)
        line = text[a:e]
        if line.endswith(b"\r"):
            line = line[:-1]
        if line:
            yield a, line
        a = e + 1


def _expected(text: bytes, rule, af: bool):
    codes = [(off, (("skip",) if line[:1] == b"#" else rule(line)), line[:1] == b"#") for off, line in lines_of(text)]
    stops = [off for off, c, _ in codes if c[0] == "stop"]
    stop_off = min(stops) if stops else NO_STOP
    live = [(off, c, h) for off, c, h in codes if off < stop_off]
    hashes = [off for off, _, h in live if h]
    kept = [(off, c) for off, c, _ in live if c[0] == "keep"]
    out = dict(n_lines=len(live), stop_off=stop_off, declined_at=min(hashes) if hashes else None,
               line_off=np.array([o for o, _ in kept], np.uint32), defer_off=np.array([o for o, c, _ in live if c[0] == "defer"], np.uint32))
    if af:
        out.update(pos=np.array([c[1] for _, c in kept], np.uint32), value=np.array([c[2] for _, c in kept], np.float64))
    else:
        out.update(chrom_len=np.array([c[1] for _, c in kept], np.uint32), pos=np.array([c[2] for _, c in kept], np.uint32),
                   value=np.array([c[3] for _, c in kept], np.float64))
    return out


def expected_snp(text: bytes, dp_int=True, ad_int=True):
    """what csvgpu_vcf_snp_parse reports for `text`: arrays in file order, n_lines, declined_at (the lowest '#' line, or None)"""
    return _expected(text, lambda l: snp_rule(l, dp_int, ad_int), False)


def expected_af(text: bytes, contig, needle, sorted_pos):
    contig, needle = (x.encode() if isinstance(x, str) else x for x in (contig, needle))
    s = set(int(x) for x in sorted_pos)
    last = int(sorted_pos[-1]) if len(sorted_pos) else 0
    return _expected(text, lambda l: af_rule(l, contig, needle, s, last), True)


# ---- texts ---------------------------------------------------------------------------------------------------------------------------
def body(lines) -> bytes:
    return ("\n".join(l for _, l in lines) + "\n").encode()


def generated_snp_text(seed=17):
    """the data lines of tests/test_snp_io.py's sample file, and the records as (pos, line)"""
    rng = np.random.default_rng(seed)
    snps = snp_lines(rng, "chr1", 900, 400_000) + snp_lines(rng, "chr2", 500, 300_000)
    return body(snps), snps, rng


def generated_gnomad_text(rng, snps, chrom):
    p = np.array([q for q, l in snps if l.startswith(chrom + "\t")])
    lines = gnomad_lines(rng, chrom, p, 400_000)
    return body(lines), lines


GOOD = "chr1\t%d\t.\tA\tG\t%s\tPASS\tDP=40\tGT:DP:AD\t0/1:%s:%s"
# (name, line): each one is deferred, and for the reason its name says
DELIBERATE_SNP = [
    ("hex QUAL", GOOD % (1001, "0x1p5", "40", "10,30")),
    ("QUAL with trailing junk", GOOD % (1002, "31abc", "40", "10,30")),
    ("QUAL with a leading blank", GOOD % (1003, " 50", "40", "10,30")),
    ("16-digit QUAL", GOOD % (1004, "31.00000000000001", "40", "10,30")),
    ("QUAL 1e-30", GOOD % (1005, "1e-30", "40", "10,30")),
    ("QUAL inf", GOOD % (1006, "inf", "40", "10,30")),
    ("two samples", GOOD % (1007, "50", "40", "10,30") + "\t0/1:5:1,1"),
    ("10-digit POS", GOOD % (4000000000, "50", "40", "10,30")),
    ("DP +12x", GOOD % (1009, "50", "+12x", "10,30")),
]
# lines that look odd and are NOT deferred: the integer and real rules cover them
NOT_DEFERRED_SNP = [
    GOOD % (1100, "+5e1", "+40", "+10,30"),
    GOOD % (1101, "50.", "40", "10,30,junk"),
    GOOD % (1102, ".5e2", "40,zz", "10,30"),
    GOOD % (1103, "0031", "040", "010,030"),
    GOOD % (1104, "-50", "40", "10,30"),                     # negative QUAL: skipped
    "chr1\t1105\t.\tA\tAT\tinf\tPASS\t.\tGT:DP:AD\t0/1:40:10,30",   # not a SNP: QUAL is never looked at
]
# deferred although the host would skip it on FILTER: DP is read in front of FILTER, as on the host, and is outside the integer rule
DEFERRED_BY_ORDER = "chr1\t1106\t.\tA\tG\t50\tq10\t.\tGT:DP:AD\t0/1:4x:10,30"

GN = "chr1\t%s\trs1\tA\tG\t.\tPASS\t%s"
DELIBERATE_AF = [
    ("hex AF", GN % ("1001", "AF_nfe=0x1p-2")),
    ("AF with trailing junk", GN % ("1002", "AC=1;AF_nfe=0.5x")),
    ("AF with a leading blank", GN % ("1003", "AF_nfe= 0.5")),
    ("16-digit AF", GN % ("1004", "AF_nfe=0.1234567890123456")),
    ("AF 1e-30", GN % ("1005", "AF_nfe=1e-30")),
    ("AF nan", GN % ("1006", "AF_nfe=nan")),
    ("POS with junk", GN % ("1007x", "AF_nfe=0.5")),
    ("10-digit POS", GN % ("4000000000", "AF_nfe=0.5")),
]
DELIBERATE_AF_POS = [1001, 1002, 1003, 1004, 1005, 1006, 1007]


def value_tokens(n=2200, seed=3):
    """QUAL / AF tokens inside the conversion rule: random ones of every shape of the grammar (whose w / 10^k is mostly inexact), values
    next to 30, 0.01 and 0.99, the rule's edges"""
    rng = np.random.default_rng(seed)
    toks = ["1e-22", "999999999999999", "0.999999999999999", "9.99999999999999e22", "1e22", "123456789012345e-22", "30", "30.0000001", "30.000001",
            "30.000002", "29.999999", "30.0000019", "30.00000191", "0.01", "0.0100000001", "0.010000001", "0.00999999", "0.99", "0.98999999",
            "0.989999999", "0.9900000001", "0.99000001", "0", "-0", "0.0", "000.5", ".5", "5.", "+0.25", "1E-1", "3.1e+1", "0.5e0", "00031.5",
            "0.30000000000000", "16777217", "16777217e-8", "33554433e-9", "0.1", "0.2", "0.3", "0.7", "1e-1", "0.0999999999999999"]
    while len(toks) < n:
        nd = int(rng.integers(1, 16))
        digits = "".join(rng.choice(list("0123456789"), nd))
        cut = int(rng.integers(0, nd + 1))
        t = digits[:cut] + ("." + digits[cut:] if rng.random() < 0.8 or cut == 0 else digits[cut:])
        if rng.random() < 0.3:
            frac = len(t.split(".")[1]) if "." in t else 0
            e = int(rng.integers(-22 + frac, 23 + frac)) if frac <= 22 else frac - 22
            t += "%s%s%d" % (rng.choice(["e", "E"]), rng.choice(["", "+"]) if e >= 0 else "", e)
        if tok_real(t.encode()) is not None:
            toks.append(t)
    return toks
