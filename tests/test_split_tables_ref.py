"""The split-read tables from record references (csvgpu_split_tables_resident / csvgpu_split_resident_fits), the parts that need no GPU: the
ABI, a numpy restatement of what the device builds from the references (`reference_tables`, which tests/test_gpu_split_tables.py compares the
kernel against), and the references themselves — host.split_refs, what SplitPass::prepare() hands to SplitParams::device_tables — against
their definition: the primaries that have a supplementary record, in the iteration order of a real std::unordered_map, each with its name's
supplementary records in file order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import host
from test_gpu_split import _make_split_shard
from test_split_fits_ref import TABLE_FIELDS, _struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MAPQ = 20
F_REVERSE, F_SUPP, F_SKIP = 0x10, 0x800, 0x100 | 0x4 | 0x400 | 0x200


# ---- C1: the ABI -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    from contextsv_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csvgpu.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, n_args in (("csvgpu_split_tables_resident", 6), ("csvgpu_split_resident_fits", 10)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.ABI
        assert len(_lib.ABI[name][1]) == n_args
    assert re.search(r"#define\s+CSVGPU_ABI_VERSION\s+4\b", text) and re.search(r"CSV_K_COUNT\s*=\s*11\b", text)
    assert _lib.ABI_VERSION == 4 and _lib.K_COUNT == 11 and _lib.KERNEL_NAMES[_lib.K_MISC] == "misc"


def test_refs_struct_matches_the_header():
    from contextsv_amd import _lib
    fields = _struct_fields("csv_split_refs")
    assert [n for n, _, _, _ in fields] == ["n_members", "n_supp", "member_rec", "supp_off", "supp_rec", "supp_where"] == [n for n, _ in _lib.csv_split_refs._fields_]
    for (n, ty, pointer, _), (_, ct) in zip(fields, _lib.csv_split_refs._fields_):
        assert (ct is C.c_void_p) == pointer and (pointer or (ty == "uint64_t" and ct is C.c_uint64)), n
    assert [ty for _, ty, pointer, _ in fields if pointer] == ["uint32_t", "uint64_t", "uint32_t", "uint8_t"]
    assert C.sizeof(_lib.csv_split_refs) == 48
    r = cs.SplitRefs([3, 1], [0, 1, 1], [7], [2])
    f = r.c_struct()
    assert (f.n_members, f.n_supp) == (2, 1) and f.supp_where == r.supp_where.ctypes.data


# ---- C2: the restatement ---------------------------------------------------------------------------------------------------------------
def reference_tables(segments, refs, seg_off):
    """What the device builds: segments[c] = dict(pos, flag, ref_end, q_start, q_end) of shard c's records, refs = SplitRefs, segment c =
    members [seg_off[c], seg_off[c + 1]). -> dict of the eleven csv_split_tables arrays (an entry on another tid: its flags, coordinates 0)."""
    t = {k: [] for k in TABLE_FIELDS}

    def row(S, r):
        return int(S["pos"][r]) + 1, int(S["ref_end"][r]), int(S["q_start"][r]), int(S["q_end"][r]), 1 if int(S["flag"][r]) & F_REVERSE else 0

    for c, S in enumerate(segments):
        for m in range(int(seg_off[c]), int(seg_off[c + 1])):
            s, e, qs, qe, rev = row(S, int(refs.member_rec[m]))
            t["start"].append(s); t["end"].append(e); t["q_start"].append(qs); t["q_end"].append(qe); t["reverse"].append(rev)
            for z in range(int(refs.supp_off[m]), int(refs.supp_off[m + 1])):
                where = int(refs.supp_where[z])
                s, e, qs, qe, f = row(S, int(refs.supp_rec[z])) if where == 0 else (0, 0, 0, 0, where)
                t["supp_start"].append(s); t["supp_end"].append(e); t["supp_q_start"].append(qs); t["supp_q_end"].append(qe); t["supp_flags"].append(f)
    t["supp_off"] = np.asarray(refs.supp_off, np.uint64)
    dt = {"reverse": np.uint8, "supp_flags": np.uint8, "supp_off": np.uint64}
    return {k: np.asarray(v, dtype=dt.get(k, np.int32)) for k, v in t.items()}


def masked(t):
    """A table dict with the four coordinates of every entry on another tid as 0 (the host writes pos + 1 into supp_start there; nothing reads it)."""
    t = {k: np.array(v) for k, v in t.items()}
    other = (t["supp_flags"] & 2) != 0
    for k in ("supp_start", "supp_end", "supp_q_start", "supp_q_end"):
        t[k][other] = 0
    return t


def assert_same_tables(got, want, what=""):
    for k in TABLE_FIELDS:
        a, b = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k)), np.asarray(want[k] if isinstance(want, dict) else getattr(want, k))
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, k, a[:8], b[:8])


def test_restatement_on_a_hand_example():
    seg0 = dict(pos=[99, 199, 299, 399], flag=[0, 0x810, 0x10, 0x800], ref_end=[150, 260, 350, 480], q_start=[0, 7, 3, 60], q_end=[50, 67, 53, 140])
    seg1 = dict(pos=[9, 19], flag=[0x800, 0], ref_end=[15, 40], q_start=[1, 2], q_end=[6, 22])
    # segment 0: member = record 2 (reverse) with entries record 1, record 3 (file order), then member = record 0 with one entry elsewhere, reverse;
    # segment 1: member = record 1 with entries record 0 and one elsewhere, forward
    refs = cs.SplitRefs([2, 0, 1], [0, 2, 3, 5], [1, 3, 5, 0, 9], [0, 0, 3, 0, 2])
    t = reference_tables([seg0, seg1], refs, [0, 2, 3])
    assert t["start"].tolist() == [300, 100, 20] and t["end"].tolist() == [350, 150, 40]
    assert t["q_start"].tolist() == [3, 0, 2] and t["q_end"].tolist() == [53, 50, 22] and t["reverse"].tolist() == [1, 0, 0]
    assert t["supp_off"].tolist() == [0, 2, 3, 5]
    assert t["supp_start"].tolist() == [200, 400, 0, 10, 0] and t["supp_end"].tolist() == [260, 480, 0, 15, 0]
    assert t["supp_q_start"].tolist() == [7, 60, 0, 1, 0] and t["supp_q_end"].tolist() == [67, 140, 0, 6, 0]
    assert t["supp_flags"].tolist() == [1, 0, 3, 0, 2]
    assert t["reverse"].dtype == np.uint8 and t["supp_flags"].dtype == np.uint8 and t["supp_off"].dtype == np.uint64 and t["start"].dtype == np.int32


# ---- C3: the references ----------------------------------------------------------------------------------------------------------------
def contig_slices(tid, n_contigs):
    """Records are sorted by (tid, pos): contig c = records [lo[c], lo[c + 1])."""
    return np.searchsorted(tid, np.arange(n_contigs + 1)).astype(np.int64)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_split_refs_are_the_survivors_in_map_order_with_their_records_in_file_order(seed):
    reads, tid, qn, n_contigs = _make_split_shard(seed)
    refs, seg_off, supp_tid = host.split_refs(tid, reads.pos, reads.flag, reads.mapq, qn, n_contigs, MIN_MAPQ)
    lo = contig_slices(tid, n_contigs)
    flag = reads.flag.astype(np.int64)
    passing = ((flag & F_SKIP) == 0) & (reads.mapq >= MIN_MAPQ)
    is_supp = passing & ((flag & F_SUPP) != 0)
    is_prim = passing & ~is_supp
    supp_of = {}                                               # name -> its supplementary records, file order
    for i in np.nonzero(is_supp)[0]:
        supp_of.setdefault(int(qn[i]), []).append(int(i))
    assert len(seg_off) == n_contigs + 1 and int(seg_off[0]) == 0 and int(seg_off[-1]) == refs.n_members
    assert int(refs.supp_off[0]) == 0 and int(refs.supp_off[-1]) == refs.n_supp and len(supp_tid) == refs.n_supp
    n_other = n_multi = 0
    for c in range(n_contigs):
        prim = np.nonzero(is_prim[lo[c]:lo[c + 1]])[0]         # record indices within the contig
        has = np.array([int(qn[lo[c] + i]) in supp_of for i in prim], bool)
        got = refs.member_rec[int(seg_off[c]):int(seg_off[c + 1])]
        assert sorted(got.tolist()) == prim[has].tolist(), c    # the member set
        order_real, order_emu, _ = host.umap_order_check(["r%d" % qn[lo[c] + i] for i in prim], (~has).astype(np.uint8))
        assert np.array_equal(order_real, order_emu) and np.array_equal(got, prim[order_real].astype(np.uint32)), c
        for m in range(int(seg_off[c]), int(seg_off[c + 1])):
            want = supp_of[int(qn[lo[c] + int(refs.member_rec[m])])]
            z0, z1 = int(refs.supp_off[m]), int(refs.supp_off[m + 1])
            assert z1 - z0 == len(want) >= 1
            n_multi += len(want) >= 2
            for z, i in zip(range(z0, z1), want):
                t = int(tid[i])
                assert int(supp_tid[z]) == t and int(refs.supp_rec[z]) == i - lo[t]
                assert int(refs.supp_where[z]) == (0 if t == c else 2 | (1 if flag[i] & F_REVERSE else 0))
                n_other += t != c
    assert n_other >= 1 and n_multi >= 1 and refs.n_members > 100


def test_split_refs_of_nothing():
    z = np.zeros(0, np.int32)
    refs, seg_off, supp_tid = host.split_refs(z, z, z, z, z, 3)
    assert refs.n_members == 0 and refs.n_supp == 0 and seg_off.tolist() == [0, 0, 0, 0] and refs.supp_off.tolist() == [0]
