"""Inputs of the VCF formatter's tests (tests/test_vcf_format_model.py on the CPU, tests/test_gpu_vcf_format.py and
tests/test_gpu_save_vcf_device.py on the device): contigs in the form tests/vcf_format_model.py takes, the files the host writer and the
oracle read, and the directed call sets of the rule's edges."""
import numpy as np

from contextsv_amd.host import CALL_DTYPE

DATE = "20250926"
IUPAC = "RYKMSWBDHV"
# likelihoods at the edges of std::to_string(double): both ties, the carry, -0.0, a denormal, below and above the sixth decimal's half
LIKELIHOODS = [1 / 128, 3 / 128, 0.9999995, 0.99999949, 1.9999995, -0.0, 0.0, 5e-324, -5e-324, 4.76837158203125e-07, 5e-7, 1.5e-6, 2.5e-6, -2533.541937, 123456789.123456789,
               9007199254740993.0, 9223372036854774784.0, -9223372036854774784.0, float("inf"), float("-inf")]
NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001]
# decimal-digit boundaries of uint32 and int32
U32_EDGES = sorted({0, 1, 9, 2**31 - 1, 2**31, 2**32 - 1} | {10**k + d for k in range(1, 10) for d in (-1, 0)})
I32_EDGES = sorted({0, -1, 1, 2**31 - 1, -2**31, -2**31 + 1} | {s * (10**k + d) for k in range(1, 10) for d in (-1, 0) for s in (1, -1)})


def random_seq(rng, n) -> bytes:
    """Upper and lower case, N, and IUPAC codes of either case."""
    pool = np.frombuffer(("ACGT" * 12 + "acgtNn" + IUPAC + IUPAC.lower()).encode(), np.uint8)
    return pool[rng.integers(0, len(pool), n)].tobytes()


def blank_calls(n) -> np.ndarray:
    c = np.zeros(n, CALL_DTYPE)
    c["id"] = np.arange(n)
    return c


def default_alt(t: int, rng=None) -> bytes:
    if t == 3:
        return b"<INS>" if rng is None or rng.random() < 0.4 else random_seq(rng, int(rng.integers(1, 60))).upper()
    return {0: b"<DEL>", 1: b"<DUP>", 2: b"<INV>", 4: b"<BND>"}.get(t, b".")


def random_calls(rng, n, length):
    """The kind tests/test_vcf_writer.py draws, with LOH among the types."""
    c = blank_calls(n)
    c["sv_type"] = rng.choice([-1, 0, 0, 0, 1, 2, 3, 3, 3, 4, 5, 6], n)
    c["start"] = rng.integers(0, length + 5, n)
    c["end"] = c["start"] + np.where(rng.random(n) < 0.3, 0, rng.integers(0, 120, n))
    c["cluster_size"] = rng.integers(0, 50, n)
    c["hmm_likelihood"] = np.where(rng.random(n) < 0.3, 0.0, -rng.random(n) * 10.0 ** rng.integers(0, 6, n))
    c["aln_flags"] = rng.integers(0, 1 << 10, n)
    c["genotype"] = rng.integers(0, 4, n)
    c["cn_state"] = rng.integers(0, 7, n)
    c["aln_offset"] = rng.integers(-300, 300, n)
    return c, [default_alt(int(t), rng) for t in c["sv_type"]]


def contig(name, seq, calls, alts, depth, gaps=None) -> dict:
    return dict(name=name if isinstance(name, bytes) else name.encode(), seq=seq, calls=calls, alts=list(alts), depth=depth, gaps=list(gaps or []))


def write_fasta(path, seqs: dict, width: int = 60):
    """seqs: name (bytes) -> bases; a duplicated name is written by giving the pair list instead of a dict."""
    pairs = seqs.items() if isinstance(seqs, dict) else seqs
    with open(path, "wb") as f:
        for name, s in pairs:
            f.write(b">" + name + b" description\n")
            for i in range(0, len(s), width):
                f.write(s[i: i + width] + b"\n")


def write_gaps(path, contigs):
    with open(path, "w") as f:
        f.write("# comment\n\nchrZ\t1\t100\n")
        for c in contigs:
            for a, b in c["gaps"]:
                f.write("%s\t%d\t%d\tgap\n" % (c["name"].decode(), a, b))


def items_of(contigs, depth_of=None):
    """What host.save_vcf and oracle.save_vcf take: [(name, calls, alts, depth)]."""
    return [(c["name"].decode(), c["calls"], c["alts"], c["depth"] if depth_of is None else depth_of(c)) for c in contigs]


def directed_positions(seq_len: int, depth_len: int):
    """Every type at the starts and ends of the rule's edges (a batch of its own each: a refusal must hide nothing else) -> [(calls, alts)]."""
    L = seq_len
    starts = [0, 1, 2, 3, L - 1, L, L + 1, depth_len - 1, depth_len, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 2, 2**32 - 1]
    out = []
    for t in (0, 1, 2, 3, 4, 6):
        rows = [(s, (s + d) & 0xFFFFFFFF) for s in starts for d in (-3, -1, 0, 1, 40, 2**31 - 2, 2**31 - 1)]
        for s, e in rows:
            c = blank_calls(1)
            c["sv_type"], c["start"], c["end"], c["genotype"], c["cn_state"], c["aln_flags"] = t, s, e, (s + e) % 4, (s + e) % 7, (s * 7 + e) % 1024
            out.append((c, [b"acgtn" if t == 3 and e % 2 else default_alt(t)]))
    return out


def enum_product(length: int):
    """Every type x genotype x cn_state on valid positions, and every evidence mask."""
    rows = [(t, g, cn) for t in range(-1, 7) for g in range(4) for cn in range(7)]
    c = blank_calls(len(rows) + 1024)
    for i, (t, g, cn) in enumerate(rows):
        c[i]["sv_type"], c[i]["genotype"], c[i]["cn_state"] = t, g, cn
    k = len(rows)
    c["sv_type"][k:] = np.arange(1024) % 5                 # DEL DUP INV INS BND
    c["aln_flags"][k:] = np.arange(1024)
    c["start"] = 2 + (np.arange(len(c)) * 7) % (length - 60)
    c["end"] = c["start"] + np.arange(len(c)) % 50
    return c, [default_alt(int(t)) for t in c["sv_type"]]


def digit_edges(length: int):
    """CLUSTER and ALNOFFSET at every decimal-digit boundary of int32, END / SVLEN of a DUP at those of uint32, the likelihoods' edges."""
    n = max(len(I32_EDGES), len(U32_EDGES), len(LIKELIHOODS) + len(NANS))
    c = blank_calls(n)
    c["sv_type"], c["start"], c["genotype"], c["cn_state"] = 1, 1, 1, 4      # (start 1: SVLEN is END as an int)
    c["end"] = [U32_EDGES[i % len(U32_EDGES)] for i in range(n)]
    c["cluster_size"] = [I32_EDGES[i % len(I32_EDGES)] for i in range(n)]
    c["aln_offset"] = [I32_EDGES[-1 - i % len(I32_EDGES)] for i in range(n)]
    like = np.array(LIKELIHOODS, np.float64).view(np.uint64).tolist() + NANS
    c["hmm_likelihood"] = np.array([like[i % len(like)] for i in range(n)], np.uint64).view(np.float64)
    return c, [b"<DUP>"] * n
