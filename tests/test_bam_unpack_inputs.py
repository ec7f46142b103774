"""The expectations of tests/bam_unpack_inputs.py (pure Python) pinned against the host reader on the CPU: every stream is written as a BAM
by tests/bam_py.py and read by BamReader (read_contig with sequences and names), which must give the arrays the Python rules give; the
refused streams fail with the message of the reason the rules name; the Python _Hash_bytes equals host.string_hashes. The GPU tests
(tests/test_gpu_bam_unpack.py) hold the kernels against the same expectations."""
import numpy as np
import pytest

import bam_py
import bam_unpack_inputs as inp
from contextsv_amd import host

NAMES = ["c0", "c1", "c2"]


def _write(tmp_path, stream, ref_lens, name="in.bam", payload=0xff00):
    path = str(tmp_path / name)
    bam_py.write_bam(path, NAMES, ref_lens, inp.index_entries(stream), block_payload=payload)
    return path


def _same(shard, exp):
    r = shard["reads"]
    for k in ("pos", "flag", "mapq", "cigar_off", "cigar"):
        assert np.array_equal(getattr(r, k), exp[k]), k
    assert np.array_equal(shard["seq_off"], exp["seq_off"]) and np.array_equal(shard["seq"], exp["seq"])
    assert shard["qnames"] == [x.decode() for x in exp["names"]]
    assert np.array_equal(host.string_hashes(shard["qnames"])[:len(exp["names"])], exp["name_hash"])


@pytest.mark.parametrize("which", ["alignment", "cg", "long", "plain"])
def test_streams_of_one_contig(tmp_path, which):
    stream = {"alignment": inp.alignment_stream, "cg": lambda: inp.cg_stream()[0], "long": lambda: inp.long_cigar_stream(300)[0],
              "plain": inp.plain_stream}[which]()
    lens = [1 << 28] * 3
    bam = host.BamFile(_write(tmp_path, stream, lens, payload=0xff00 if which != "plain" else 777))
    exp = inp.expected(stream, 0, lens[0])
    assert exp["n_kept"] >= 30
    _same(bam.read_contig("c0", want_seq=True, want_qnames=True), exp)
    bam.close()


def test_cg_cases_are_what_their_names_say():
    stream, names, taken = inp.cg_stream()
    exp = inp.expected(stream)
    words = np.diff(exp["cigar_off"]).astype(int)
    fields = [int.from_bytes(stream[o + 16:o + 18], "little") for o in exp["rec_off"]]
    assert len(names) == exp["n_kept"] == len(fields) and len(set(names)) == len(names)
    for i, name in enumerate(names):
        if i in taken:
            assert fields[i] == 2 and words[i] >= 2, name                    # the placeholder's two words replaced by the tag's
            assert (words[i] != 2) or name == "count equal to n_cigar", name
        else:
            assert words[i] == fields[i], name
    assert len(taken) == 4 + len(inp.AUX_FIELDS) + 1 and len(inp.AUX_FIELDS) == 18


def test_filter_stream(tmp_path):
    stream = inp.filter_stream()
    lens = [1 << 28, 35, 1 << 28]
    bam = host.BamFile(_write(tmp_path, stream, lens))
    for t, n in ((0, 3), (1, 3), (2, 2)):
        exp = inp.expected(stream, t, lens[t])
        assert exp["n_kept"] == n and exp["stopped"]
        _same(bam.read_contig(NAMES[t], want_seq=True, want_qnames=True), exp)
    bam.close()
    assert inp.expected(stream)["n_kept"] == 12 and not inp.expected(stream)["stopped"]


def test_refused_streams_fail_with_the_reason_message(tmp_path):
    for k, (name, stream, reason, at) in enumerate(inp.refusal_streams()):
        with pytest.raises(inp.Declined) as ei:
            inp.expected(stream)
        assert (ei.value.reason, ei.value.offset) == (reason, at), name
        path = str(tmp_path / ("bad%d.bam" % k))
        bam_py.write_bam(path, NAMES, [1 << 28] * 3, [(stream, 0, 0, 1, 0)], with_index=False)
        with pytest.raises(RuntimeError) as ei:
            host.BamFile(path, load_index=False).read_all(want_seq=True)
        assert str(ei.value) == inp.MESSAGES[reason], name
    assert {r[2] for r in inp.refusal_streams()} == {inp.SHORT, inp.LONG, inp.NEG_LSEQ, inp.FIELDS}


def test_python_hash_is_std_hash():
    rng = np.random.default_rng(3)
    names = ["".join(chr(c) for c in rng.integers(33, 127, n)) for n in range(255)]
    assert np.array_equal(host.string_hashes(names), np.array([inp.hash_bytes(x.encode()) for x in names], np.uint64))
