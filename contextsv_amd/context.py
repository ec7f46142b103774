"""Thin object wrapper over the csvgpu C-ABI: one `Context` per GPU (host-pointer entry points)
and `Shard` for inputs that stay resident in HBM. All compute happens behind the C-ABI."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import SIG_DTYPE, CsvError, csv_chr_result, csv_hmm, csv_reads, csv_split_refs, csv_split_tables, ptr


def _as_u8(x) -> np.ndarray:
    """bytes-like or array-like -> contiguous uint8 array (no copy where there need be none)"""
    return np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x, np.uint8)


def _handles(objs):
    """the C handles of shards, tables, ... as a void* array for the C-ABI (None: a null handle; at least one element long)"""
    return (C.c_void_p * max(len(objs), 1))(*[None if o is None else o.h for o in objs])


def _is_dev(t, element_size: int) -> bool:
    """a contiguous torch tensor on a device, of that element size"""
    return t.is_cuda and t.is_contiguous() and t.element_size() == element_size


@dataclass
class SplitTables:
    """The members of a batch of contigs (primary alignments that have a supplementary record, map iteration order per segment) and
    their supplementary records (include/csvgpu.h csv_split_tables)."""
    start: np.ndarray         # int32 [n_members]  pos + 1
    end: np.ndarray           # int32 [n_members]  bam_endpos
    q_start: np.ndarray
    q_end: np.ndarray
    reverse: np.ndarray       # uint8 [n_members]  1 = FLAG 0x10
    supp_off: np.ndarray      # uint64 [n_members + 1]
    supp_start: np.ndarray    # int32 [n_supp]
    supp_end: np.ndarray
    supp_q_start: np.ndarray
    supp_q_end: np.ndarray
    supp_flags: np.ndarray    # uint8 [n_supp]  bit 0 reverse strand, bit 1 on another tid than the primary

    def __post_init__(self):
        for f in ("start", "end", "q_start", "q_end", "supp_start", "supp_end", "supp_q_start", "supp_q_end"):
            setattr(self, f, np.ascontiguousarray(getattr(self, f), dtype=np.int32))
        self.reverse = np.ascontiguousarray(self.reverse, dtype=np.uint8)
        self.supp_flags = np.ascontiguousarray(self.supp_flags, dtype=np.uint8)
        self.supp_off = np.ascontiguousarray(self.supp_off, dtype=np.uint64)
        n, k = len(self.start), len(self.supp_start)
        if not (len(self.end) == n and len(self.q_start) == n and len(self.q_end) == n and len(self.reverse) == n and len(self.supp_off) == n + 1):
            raise ValueError("SplitTables: member array lengths disagree")
        if not (len(self.supp_end) == k and len(self.supp_q_start) == k and len(self.supp_q_end) == k and len(self.supp_flags) == k):
            raise ValueError("SplitTables: supplementary array lengths disagree")

    @property
    def n_members(self) -> int:
        return len(self.start)

    @property
    def n_supp(self) -> int:
        return len(self.supp_start)

    def c_struct(self) -> csv_split_tables:
        t = csv_split_tables()
        t.n_members, t.n_supp = self.n_members, self.n_supp
        for f in ("start", "end", "q_start", "q_end", "reverse", "supp_off", "supp_start", "supp_end", "supp_q_start", "supp_q_end", "supp_flags"):
            setattr(t, f, ptr(getattr(self, f)))
        return t


@dataclass
class Reads:
    """Struct-of-arrays view of one shard's alignment records (include/csvgpu.h csv_reads)."""
    pos: np.ndarray        # int32   [n]
    flag: np.ndarray       # uint16  [n]
    mapq: np.ndarray       # uint8   [n]
    cigar_off: np.ndarray  # uint64  [n+1]
    cigar: np.ndarray      # uint32  [m] packed len<<4|op
    tid: np.ndarray | None = None

    def __post_init__(self):
        self.pos = np.ascontiguousarray(self.pos, dtype=np.int32)
        self.flag = np.ascontiguousarray(self.flag, dtype=np.uint16)
        self.mapq = np.ascontiguousarray(self.mapq, dtype=np.uint8)
        self.cigar_off = np.ascontiguousarray(self.cigar_off, dtype=np.uint64)
        self.cigar = np.ascontiguousarray(self.cigar, dtype=np.uint32)
        n = len(self.pos)
        if not (len(self.flag) == n and len(self.mapq) == n and len(self.cigar_off) == n + 1):
            raise ValueError("Reads: array lengths disagree")
        if int(self.cigar_off[-1]) != len(self.cigar):
            raise ValueError("Reads: cigar_off[-1] != len(cigar)")

    @property
    def n_reads(self) -> int:
        return len(self.pos)

    @property
    def n_cigar(self) -> int:
        return len(self.cigar)

    def c_struct(self) -> csv_reads:
        r = csv_reads()
        r.n_reads, r.n_cigar = self.n_reads, self.n_cigar
        r.pos, r.flag, r.mapq = ptr(self.pos), ptr(self.flag), ptr(self.mapq)
        r.tid = ptr(self.tid) if self.tid is not None else None
        r.cigar_off, r.cigar = ptr(self.cigar_off), ptr(self.cigar)
        return r

    @staticmethod
    def from_cigar_lists(pos, flag, mapq, cigars) -> "Reads":
        """cigars: list of lists of (op, length) with BAM op codes (M0 I1 D2 N3 S4 H5 P6 =7 X8)."""
        off = np.zeros(len(cigars) + 1, dtype=np.uint64)
        words = []
        for i, c in enumerate(cigars):
            for op, ln in c:
                words.append((int(ln) << 4) | int(op))
            off[i + 1] = len(words)
        return Reads(np.asarray(pos), np.asarray(flag), np.asarray(mapq), off, np.asarray(words, dtype=np.uint32))


class Gate:
    """csv_gate: several Contexts on one GPU queue their scan + depth pairs back to back on the gate's one stream (csvgpu_gate_*)."""

    def __init__(self, device: int | None = None):
        """device given: the gate's stream is created now (csvgpu_gate_open) — do that BEFORE creating the lanes' Contexts, see csvgpu.h"""
        self.lib = _lib.load()
        self.h = self.lib.csvgpu_gate_create()
        if not self.h:
            raise CsvError(_lib.CSV_ENOMEM, "csvgpu_gate_create failed")
        if device is not None:
            rc = self.lib.csvgpu_gate_open(self.h, device)
            if rc:
                raise CsvError(rc, "csvgpu_gate_open failed")

    def close(self):
        if getattr(self, "h", None):
            self.lib.csvgpu_gate_destroy(self.h)
            self.h = None


class Context:
    """One csv_ctx (= one GPU). `stream` may be an existing hipStream_t handle (e.g. torch's)."""

    def __init__(self, device: int = 0, stream: int | None = None, background: bool = False):
        self.lib = _lib.load()
        self.device = device
        self.h = self.lib.csvgpu_create_background(device) if background else self.lib.csvgpu_create(device, stream)
        if not self.h:
            msg = self.lib.csvgpu_last_error(None)
            raise CsvError(_lib.CSV_ENODEV, (msg or b"csvgpu_create failed").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.csvgpu_destroy(self.h)
            self.h = None

    def set_gate(self, gate: "Gate | None"):
        self._check(self.lib.csvgpu_set_gate(self.h, gate.h if gate is not None else None))

    def set_tuning(self, scan_form: int | None = None, split_tail: int | None = None, sort_three_launch: bool = False,
                   dbscan_all_pairs: bool = False, split_chain_only: bool = False):
        """csvgpu_set_tuning: which of several kernels with the same result this context launches from now on (csv_tuning in csvgpu.h).
        scan_form 0..3 / split_tail 0..3 force a value, None leaves the choice to the library; no argument at all = the defaults."""
        t = _lib.csv_tuning(-1 if scan_form is None else scan_form, -1 if split_tail is None else split_tail, int(sort_three_launch),
                            int(dbscan_all_pairs), int(split_chain_only))
        self._check(self.lib.csvgpu_set_tuning(self.h, C.byref(t)))

    def set_cigar_packing(self, on: bool = True):
        """csvgpu_set_cigar_packing: whether long-read shards uploaded from now on keep their CIGAR ops in 16 bits (the default) or in 32."""
        self._check(self.lib.csvgpu_set_cigar_packing(self.h, int(on)))

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _error(self, status: int) -> CsvError:
        return CsvError(status, (self.lib.csvgpu_last_error(self.h) or b"").decode())

    def _check(self, rc: int):
        if rc != 0:
            raise self._error(rc)

    # -------------------------------------------------------------------------------- host-pointer seams
    def cigar_scan(self, reads: Reads, depth_len: int, min_oplen: int = 50, min_mapq: int = 20, capacity: int | None = None):
        """-> structured array of signatures in the reference's chr_sv_calls order."""
        cap = reads.n_cigar if capacity is None else capacity
        out = np.zeros(max(cap, 1), dtype=SIG_DTYPE)
        n = C.c_uint64(cap)
        rs = reads.c_struct()
        self._check(self.lib.csvgpu_cigar_scan(self.h, C.byref(rs), depth_len, min_oplen, min_mapq, ptr(out), C.byref(n)))
        return out[: n.value].copy()

    def aln_intervals(self, reads: Reads):
        n = reads.n_reads
        ref_end, qs, qe = (np.zeros(max(n, 1), np.int32) for _ in range(3))
        rs = reads.c_struct()
        self._check(self.lib.csvgpu_aln_intervals(self.h, C.byref(rs), ptr(ref_end), ptr(qs), ptr(qe)))
        return ref_end[:n], qs[:n], qe[:n]

    def depth(self, reads: Reads, depth_len: int, want_array: bool = True):
        d = np.zeros(max(depth_len, 1), np.uint32) if want_array else None
        s, nz = C.c_uint64(0), C.c_uint32(0)
        rs = reads.c_struct()
        self._check(self.lib.csvgpu_depth(self.h, C.byref(rs), depth_len, ptr(d), C.byref(s), C.byref(nz)))
        return (d[:depth_len] if d is not None else None), s.value, nz.value

    def dbscan_iv(self, start, end, eps: float, min_pts: int):
        start = np.ascontiguousarray(start, np.uint32)
        end = np.ascontiguousarray(end, np.uint32)
        n = len(start)
        labels = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.csvgpu_dbscan_iv(self.h, ptr(start), ptr(end), n, eps, min_pts, ptr(labels)))
        return labels[:n]

    def dbscan_iv_batch(self, start, end, seg_off, eps: float, min_pts: int):
        start = np.ascontiguousarray(start, np.uint32)
        end = np.ascontiguousarray(end, np.uint32)
        seg_off = np.ascontiguousarray(seg_off, np.uint64)
        labels = np.zeros(max(len(start), 1), np.int32)
        self._check(self.lib.csvgpu_dbscan_iv_batch(self.h, ptr(start), ptr(end), ptr(seg_off), len(seg_off) - 1, eps, min_pts, ptr(labels)))
        return labels[: len(start)]

    def dbscan_1d(self, pts, seg_off, eps: float, min_pts: int):
        pts = np.ascontiguousarray(pts, np.int32)
        seg_off = np.ascontiguousarray(seg_off, np.uint64)
        labels = np.zeros(max(len(pts), 1), np.int32)
        self._check(self.lib.csvgpu_dbscan_1d(self.h, ptr(pts), ptr(seg_off), len(seg_off) - 1, eps, min_pts, ptr(labels)))
        return labels[: len(pts)]

    def sort_slot(self, keys, seg_off, nth, max_partitions: int = 0):
        """csvgpu_sort_slot: for every segment keys[seg_off[s]:seg_off[s + 1]] the index (inside the segment) of the element that libstdc++'s
        std::sort by key descending leaves at slot nth[s] -> (idx uint32, declined bool). A segment whose chain of partitions exceeds
        max_partitions (0: the library's own depth limit) is declined, idx = SORT_SLOT_NONE; so is idx of an empty segment (not declined)."""
        keys = np.ascontiguousarray(keys, np.uint32)
        seg_off = np.ascontiguousarray(seg_off, np.uint64)
        nth = np.ascontiguousarray(nth, np.uint64)
        n_seg = len(seg_off) - 1
        assert n_seg >= 0 and len(nth) == n_seg
        idx = np.zeros(max(n_seg, 1), np.uint32)
        declined = np.zeros(max(n_seg, 1), np.uint8)
        self._check(self.lib.csvgpu_sort_slot(self.h, ptr(keys), ptr(seg_off), n_seg, ptr(nth), max_partitions, ptr(idx), ptr(declined)))
        return idx[:n_seg], declined[:n_seg].astype(bool)

    def merge_select(self, sig, labels, n_del: int, max_partitions: int = 0, capacity=None):
        """csvgpu_merge_select: mergeSVs' representatives of one contig from host arrays — sig[SIG_DTYPE] with the n_del DEL signatures
        first, labels as dbscan_iv gives them per type -> (records[MERGE_REP_DTYPE], counts dict). capacity None: always enough."""
        sig = np.ascontiguousarray(sig, SIG_DTYPE)
        labels = np.ascontiguousarray(labels, np.int32)
        assert len(labels) == len(sig) and 0 <= n_del <= len(sig)
        return _merge_records(self, capacity, len(sig), lambda rep, cap, cnt: self.lib.csvgpu_merge_select(
            self.h, ptr(sig), ptr(labels), n_del, len(sig) - n_del, max_partitions, ptr(rep), cap, C.byref(cnt)))

    def window_log2(self, depth, region_start, region_end, sample_size, mean_cov: float):
        depth = np.ascontiguousarray(depth, np.uint32)
        rs = np.ascontiguousarray(region_start, np.uint32)
        re = np.ascontiguousarray(region_end, np.uint32)
        ss = np.ascontiguousarray(sample_size, np.int32)
        off = np.zeros(len(rs) + 1, np.uint64)
        off[1:] = np.cumsum(ss.astype(np.int64))
        nw = int(off[-1])
        l2 = np.zeros(max(nw, 1), np.float64)
        ws, we = np.zeros(max(nw, 1), np.uint32), np.zeros(max(nw, 1), np.uint32)
        self._check(self.lib.csvgpu_window_log2(self.h, ptr(depth), len(depth), ptr(rs), ptr(re), ptr(ss), ptr(off), len(rs),
                                                mean_cov, ptr(l2), ptr(ws), ptr(we)))
        return l2[:nw], ws[:nw], we[:nw], off

    def viterbi(self, hmm: csv_hmm, o1, o2, pfb, seq_off):
        o1 = np.ascontiguousarray(o1, np.float64)
        o2 = np.ascontiguousarray(o2, np.float64)
        pfb = np.ascontiguousarray(pfb, np.float64)
        seq_off = np.ascontiguousarray(seq_off, np.uint64)
        n_seq = len(seq_off) - 1
        states = np.zeros(max(len(o1), 1), np.int32)
        ll = np.zeros(max(n_seq, 1), np.float64)
        self._check(self.lib.csvgpu_viterbi(self.h, C.byref(hmm), ptr(o1), ptr(o2), ptr(pfb), ptr(seq_off), n_seq, ptr(states), ptr(ll)))
        return states[: len(o1)], ll[:n_seq]

    def split_order(self, shards, min_mapq: int, supp_hash, capacity: int | None = None):
        """csvgpu_split_order: per contig (shard with query-name hashes attached) the records of the surviving primaries in the
        iteration order of the reference's qname map -> list of uint32 arrays."""
        supp_hash = np.ascontiguousarray(supp_hash, np.uint64)
        n = len(shards)
        hs = _handles(shards)
        cap = capacity if capacity is not None else max(1024, 2 * len(supp_hash))
        out = np.zeros(max(cap, 1), np.uint32)
        off = np.zeros(n + 1, np.uint64)
        rc = self.lib.csvgpu_split_order(self.h, n, hs, min_mapq, ptr(supp_hash), len(supp_hash), ptr(out), cap, ptr(off))
        if rc == _lib.CSV_ECAPACITY and capacity is None:
            return self.split_order(shards, min_mapq, supp_hash, capacity=int(off[n]))
        self._check(rc)
        return [out[int(off[k]): int(off[k + 1])].copy() for k in range(n)]

    def split_order_two_calls(self, shards, min_mapq: int, supp_hash, capacity: int = 4):
        """csvgpu_split_order_begin (everything that needs no supplementary record, queued) + csvgpu_split_order_finish; a too small
        `capacity` exercises the retry of _finish after CSV_ECAPACITY."""
        supp_hash = np.ascontiguousarray(supp_hash, np.uint64)
        n = len(shards)
        hs = _handles(shards)
        self._check(self.lib.csvgpu_split_order_begin(self.h, n, hs, min_mapq))
        out = np.zeros(max(capacity, 1), np.uint32)
        off = np.zeros(n + 1, np.uint64)
        rc = self.lib.csvgpu_split_order_finish(self.h, ptr(supp_hash), len(supp_hash), ptr(out), capacity, ptr(off))
        if rc == _lib.CSV_ECAPACITY:
            capacity = int(off[n])
            out = np.zeros(max(capacity, 1), np.uint32)
            rc = self.lib.csvgpu_split_order_finish(self.h, ptr(supp_hash), len(supp_hash), ptr(out), capacity, ptr(off))
        self._check(rc)
        return [out[int(off[k]): int(off[k + 1])].copy() for k in range(n)]

    def split_order_self(self, shards, min_mapq: int, capacity: int = 4):
        """csvgpu_split_order_begin_self (the supplementary hashes are those of the same shards' supplementary records; the whole order is
        queued) + csvgpu_split_order_finish without hashes."""
        n = len(shards)
        hs = _handles(shards)
        self._check(self.lib.csvgpu_split_order_begin_self(self.h, n, hs, min_mapq))
        out = np.zeros(max(capacity, 1), np.uint32)
        off = np.zeros(n + 1, np.uint64)
        rc = self.lib.csvgpu_split_order_finish(self.h, None, 0, ptr(out), capacity, ptr(off))
        if rc == _lib.CSV_ECAPACITY:
            capacity = int(off[n])
            out = np.zeros(max(capacity, 1), np.uint32)
            rc = self.lib.csvgpu_split_order_finish(self.h, None, 0, ptr(out), capacity, ptr(off))
        self._check(rc)
        return [out[int(off[k]): int(off[k + 1])].copy() for k in range(n)]

    def split_groups(self, start, end, seg_off, capacity: int | None = None):
        """csvgpu_split_groups: the overlap groups (more than one member) of every segment, members of a segment given in the iteration
        order of its qname map as closed intervals -> (seg_group_off, group_off, members), members = indices within the segment in
        findOverlaps' traversal order. capacity None: sized from the input and retried once on CSV_ECAPACITY; given: CsvError when too small."""
        start = np.ascontiguousarray(start, np.int32)
        end = np.ascontiguousarray(end, np.int32)
        seg_off = np.ascontiguousarray(seg_off, np.uint64)
        n_seg = len(seg_off) - 1
        if n_seg < 0 or len(start) != len(end) or (n_seg >= 0 and len(seg_off) and int(seg_off[-1]) != len(start)):
            raise ValueError("split_groups: seg_off must have n_seg + 1 entries and end at the number of members")
        cap = capacity if capacity is not None else max(1024, 2 * len(start))
        sgo = np.zeros(n_seg + 1, np.uint64)
        go = np.zeros(len(start) + 1, np.uint64)
        mem = np.zeros(max(cap, 1), np.uint32)
        n = C.c_uint64(cap)
        rc = self.lib.csvgpu_split_groups(self.h, ptr(start), ptr(end), ptr(seg_off), n_seg, ptr(sgo), ptr(go), ptr(mem), C.byref(n))
        if rc == _lib.CSV_ECAPACITY and capacity is None:
            return self.split_groups(start, end, seg_off, capacity=int(n.value))
        self._check(rc)
        return sgo, go[: int(sgo[n_seg]) + 1].copy(), mem[: int(n.value)].copy()

    @staticmethod
    def _split_refs_args(shards, refs, seg_off, what):
        seg_off = np.ascontiguousarray(seg_off, np.uint64)
        n_seg = len(seg_off) - 1
        if n_seg < 0 or len(shards) != n_seg:
            raise ValueError(what + ": seg_off must have one entry more than there are shards")
        hs = _handles(shards)
        return seg_off, n_seg, hs

    def split_tables_resident(self, shards, refs, seg_off) -> "SplitTables":
        """csvgpu_split_tables_resident: the SplitTables of record references (SplitRefs) into resident shards — segment c = members
        [seg_off[c], seg_off[c + 1]) of shards[c], on which the pipeline has run — built on the device and copied back."""
        seg_off, n_seg, hs = self._split_refs_args(shards, refs, seg_off, "split_tables_resident")
        nm, ns = refs.n_members, refs.n_supp
        i32 = lambda n: np.zeros(n, np.int32)
        out = SplitTables(i32(nm), i32(nm), i32(nm), i32(nm), np.zeros(nm, np.uint8), np.zeros(nm + 1, np.uint64), i32(ns), i32(ns), i32(ns), i32(ns),
                          np.zeros(ns, np.uint8))
        t, f = out.c_struct(), refs.c_struct()
        self._check(self.lib.csvgpu_split_tables_resident(self.h, n_seg, hs, C.byref(f), ptr(seg_off), C.byref(t)))
        if (t.n_members, t.n_supp) != (nm, ns):
            raise RuntimeError("split_tables_resident: the library returned other counts than the references hold")
        return out

    def split_resident_fits(self, shards, refs, seg_off, eps: float = 100.0, min_pts: int = 5):
        """csvgpu_split_resident_fits: the tables of split_tables_resident built where the groups -> fits chain reads them, and that chain: what
        split_fits(split_tables_resident(...), seg_off) returns, with nothing but the references going up and the records coming back.
        -> (seg_group_off, fits)."""
        seg_off, n_seg, hs = self._split_refs_args(shards, refs, seg_off, "split_resident_fits")
        sgo = np.zeros(n_seg + 1, np.uint64)
        out = np.zeros(max(refs.n_members, 1), _lib.SPLIT_FIT_DTYPE)
        n = C.c_uint64(0)
        f = refs.c_struct()
        self._check(self.lib.csvgpu_split_resident_fits(self.h, n_seg, hs, C.byref(f), ptr(seg_off), eps, min_pts, ptr(sgo), ptr(out), C.byref(n)))
        return sgo, out[: int(n.value)].copy()

    def split_fits(self, tables, seg_off, groups=None, eps: float = 100.0, min_pts: int = 5):
        """csvgpu_split_fits / csvgpu_split_groups_fits: the evidence the reference derives from every overlap group — strand vote, the six
        point sets, their DBSCAN1D fits, the largest clusters and their medians — as one SPLIT_FIT_DTYPE record per group.
        tables: SplitTables (members and their supplementary records, segment by segment); groups: (seg_group_off, group_off, members) as
        split_groups or host.split_groups_host returns them, or None for the fused call, which computes the groups on the device and
        leaves them there. -> (seg_group_off, fits)."""
        seg_off = np.ascontiguousarray(seg_off, np.uint64)
        n_seg = len(seg_off) - 1
        if n_seg < 0:
            raise ValueError("split_fits: seg_off must have n_seg + 1 entries")
        t = tables.c_struct()
        if groups is None:
            sgo = np.zeros(n_seg + 1, np.uint64)
            out = np.zeros(max(tables.n_members, 1), _lib.SPLIT_FIT_DTYPE)
            n = C.c_uint64(0)
            self._check(self.lib.csvgpu_split_groups_fits(self.h, C.byref(t), ptr(seg_off), n_seg, eps, min_pts, ptr(sgo), ptr(out), C.byref(n)))
            return sgo, out[: int(n.value)].copy()
        sgo, go, mem = (np.ascontiguousarray(groups[0], np.uint64), np.ascontiguousarray(groups[1], np.uint64), np.ascontiguousarray(groups[2], np.uint32))
        if len(sgo) != n_seg + 1 or len(go) < int(sgo[n_seg]) + 1 or len(mem) < int(go[int(sgo[n_seg])]):
            raise ValueError("split_fits: the group tables do not fit the segments")
        out = np.zeros(max(int(sgo[n_seg]), 1), _lib.SPLIT_FIT_DTYPE)
        self._check(self.lib.csvgpu_split_fits(self.h, C.byref(t), ptr(seg_off), n_seg, ptr(sgo), ptr(go), ptr(mem), eps, min_pts, ptr(out)))
        return sgo, out[: int(sgo[n_seg])]

    @staticmethod
    def _cn_regions(shards, mean_cov, reg_off, region_start, region_end, sample_size, snp_off, snp_pos, snp_baf, snp_pfb, what):
        """csv_cn_regions over these arrays -> (struct, keep-alive tuple, R)."""
        reg_off = np.ascontiguousarray(reg_off, np.uint64)
        if len(reg_off) != len(shards) + 1 or len(mean_cov) != len(shards):
            raise ValueError(what + ": reg_off needs one entry more than there are shards, mean_cov one per shard")
        rs, re = np.ascontiguousarray(region_start, np.uint32), np.ascontiguousarray(region_end, np.uint32)
        ss = np.ascontiguousarray(sample_size, np.int32)
        so = np.ascontiguousarray(snp_off, np.uint64)
        sp = np.ascontiguousarray(snp_pos, np.uint32)
        sb, sf = np.ascontiguousarray(snp_baf, np.float64), np.ascontiguousarray(snp_pfb, np.float64)
        R = len(rs)
        if not (len(re) == R and len(ss) == R and len(so) == R + 1 and len(sb) == len(sp) and len(sf) == len(sp)):
            raise ValueError(what + ": array lengths disagree")
        if (len(reg_off) and int(reg_off[-1]) != R) or int(so[-1]) != len(sp):
            raise ValueError(what + ": reg_off must end at the number of regions, snp_off at the number of SNP records")
        hs = _handles(shards)
        mc = np.ascontiguousarray(mean_cov, np.float64)
        t = _lib.csv_cn_regions(len(shards), C.cast(hs, C.c_void_p), ptr(mc), ptr(reg_off), ptr(rs), ptr(re), ptr(ss), ptr(so), ptr(sp), ptr(sb), ptr(sf))
        return t, (hs, mc, reg_off, rs, re, ss, so, sp, sb, sf), R

    def cn_observations(self, shards, mean_cov, reg_off, region_start, region_end, sample_size, snp_off, snp_pos, snp_baf, snp_pfb,
                        capacity: int | None = None) -> dict:
        """csvgpu_cn_observations_resident_many: the copy-number pass's observation vectors of regions [reg_off[c], reg_off[c + 1]) on
        shards[c] (resident depth maps), built on the device: region r has max(sample_size[r], its SNP records) windows, its SNP records are
        snp_*[snp_off[r]:snp_off[r + 1]] with non-decreasing positions. -> dict(obs_off, pos, baf, pfb, log2_cov, is_snp), region r at
        [obs_off[r], obs_off[r + 1]). capacity None: sized by the bound (windows + 3 records); given: CsvError(CSV_ECAPACITY) when too small,
        with the exact count in the exception's `needed`."""
        t, keep, R = self._cn_regions(shards, mean_cov, reg_off, region_start, region_end, sample_size, snp_off, snp_pos, snp_baf, snp_pfb, "cn_observations")
        cap = capacity if capacity is not None else int(np.maximum(keep[5], np.diff(keep[6]).astype(np.int64)).sum()) + 3 * len(keep[7])
        return self._cn_call(R, cap, False, False, True, lambda off, pos, st, ll, baf, pfb, l2, snp, n: self.lib.csvgpu_cn_observations_resident_many(
            self.h, C.byref(t), ptr(off), ptr(pos), ptr(baf), ptr(pfb), ptr(l2), ptr(snp), C.byref(n)))

    def cn_decode(self, hmm: csv_hmm, shards, mean_cov, reg_off, region_start, region_end, sample_size, snp_off, snp_pos, snp_baf, snp_pfb,
                  want_observations: bool = False) -> dict:
        """csvgpu_cn_decode_resident_many: cn_observations and viterbi on them in one call, the observations staying on the device.
        -> dict(obs_off, pos, states, loglik), and baf / pfb / log2_cov / is_snp with want_observations."""
        t, keep, R = self._cn_regions(shards, mean_cov, reg_off, region_start, region_end, sample_size, snp_off, snp_pos, snp_baf, snp_pfb, "cn_decode")
        cap = int(np.maximum(keep[5], np.diff(keep[6]).astype(np.int64)).sum()) + 3 * len(keep[7])
        return self._cn_call(R, cap, False, True, want_observations, lambda off, pos, st, ll, baf, pfb, l2, snp, n: self.lib.csvgpu_cn_decode_resident_many(
            self.h, C.byref(t), C.byref(hmm), ptr(off), ptr(pos), ptr(st), ptr(ll), ptr(baf), ptr(pfb), ptr(l2), ptr(snp), C.byref(n)))

    # -------------------------------------------------------------------------------- resident SNP tables
    def _snp_table(self, what, arrays, counts):
        """arrays: (name, value or None, dtype) in the creator's order; all numpy / array-likes (the host form) or all device tensors."""
        given = [a for _, a, _ in arrays if a is not None]
        dev = bool(given) and all(hasattr(a, "is_cuda") for a in given)
        if dev:
            for name, a, dt in arrays:
                if a is not None and not _is_dev(a, np.dtype(dt).itemsize):
                    raise ValueError(f"{what}: {name} must be a contiguous device tensor of {np.dtype(dt).itemsize}-byte elements")
            ptrs = [None if a is None or a.numel() == 0 else a.data_ptr() for _, a, _ in arrays]
            lens = [None if a is None else a.numel() for _, a, _ in arrays]
            keep = None
        else:
            keep = [None if a is None else np.ascontiguousarray(a, dt) for _, a, dt in arrays]
            ptrs = [ptr(a) for a in keep]
            lens = [None if a is None else len(a) for a in keep]
        for (name, _, _), ln, want in zip(arrays, lens, counts):
            if ln is not None and ln != lens[want]:
                raise ValueError(f"{what}: {name} has {ln} entries, {arrays[want][0]} has {lens[want]}")
        return dev, ptrs, lens, keep

    def snp_table(self, pos, baf, pfb=None, has_pfb=None) -> "SnpTable":
        """csvgpu_snp_table_create (numpy arrays) / _create_dev (device tensors): one contig's SNP records resident on the device, the
        per-record kind — every member of a run of equal positions answers with the run's last baf and with the pfb of the run's last
        record that has one (has_pfb), else 0.0. pos ascending (uint32), baf / pfb float64, has_pfb uint8."""
        arrays = (("pos", pos, np.uint32), ("baf", baf, np.float64), ("pfb", pfb, np.float64), ("has_pfb", has_pfb, np.uint8))
        dev, p, lens, keep = self._snp_table("snp_table", arrays, (0, 0, 0, 0))
        fn = self.lib.csvgpu_snp_table_create_dev if dev else self.lib.csvgpu_snp_table_create
        h = fn(self.h, p[0], p[1], p[2], p[3], lens[0])
        if not h:
            raise self._error(_lib.CSV_EINVAL)
        return SnpTable(self, h)

    def snp_table_hits(self, pos, baf, af_pos, af) -> "SnpTable":
        """csvgpu_snp_table_create_hits / _hits_dev: the first-hit kind — a region's pfb comes from the first population record (af_pos
        ascending, af) inside the span of the region's own records, for the records at that position; 0.0 for every other record."""
        arrays = (("pos", pos, np.uint32), ("baf", baf, np.float64), ("af_pos", af_pos, np.uint32), ("af", af, np.float64))
        dev, p, lens, keep = self._snp_table("snp_table_hits", arrays, (0, 0, 2, 2))
        fn = self.lib.csvgpu_snp_table_create_hits_dev if dev else self.lib.csvgpu_snp_table_create_hits
        h = fn(self.h, p[0], p[1], p[2], p[3], lens[0], lens[2])
        if not h:
            raise self._error(_lib.CSV_EINVAL)
        return SnpTable(self, h)

    def snp_table_query_raw(self, table: "SnpTable", region_start, region_end, snp_off, pos, baf, pfb, capacity: int):
        """csvgpu_snp_table_query into the caller's arrays -> (status, n)."""
        rs, re = np.ascontiguousarray(region_start, np.uint32), np.ascontiguousarray(region_end, np.uint32)
        if len(rs) != len(re):
            raise ValueError("snp_table_query: region_start and region_end differ in length")
        n = C.c_uint64(capacity)
        rc = self.lib.csvgpu_snp_table_query(self.h, table.h, ptr(rs), ptr(re), len(rs), ptr(snp_off), ptr(pos), ptr(baf), ptr(pfb), C.byref(n))
        return rc, int(n.value)

    def snp_table_query(self, table: "SnpTable", region_start, region_end) -> dict:
        """What SNPSource::queryFlat appends for each region, back to back -> dict(snp_off, pos, baf, pfb): a first call sizes the arrays."""
        R = len(region_start)
        off = np.zeros(R + 1, np.uint64)
        rc, n = self.snp_table_query_raw(table, region_start, region_end, off, None, None, None, 0)
        if rc == _lib.CSV_ECAPACITY:
            pos, baf, pfb = np.zeros(n, np.uint32), np.zeros(n, np.float64), np.zeros(n, np.float64)
            rc, n = self.snp_table_query_raw(table, region_start, region_end, off, pos, baf, pfb, n)
        else:
            pos, baf, pfb = np.zeros(0, np.uint32), np.zeros(0, np.float64), np.zeros(0, np.float64)
        self._check(rc)
        return dict(snp_off=off, pos=pos, baf=baf, pfb=pfb)

    @staticmethod
    def _cn_table_regions(shards, tables, mean_cov, reg_off, region_start, region_end, sample_size, what):
        """csv_cn_table_regions over these arrays -> (struct, keep-alive tuple, R)."""
        reg_off = np.ascontiguousarray(reg_off, np.uint64)
        if len(reg_off) != len(shards) + 1 or len(mean_cov) != len(shards) or len(tables) != len(shards):
            raise ValueError(what + ": reg_off needs one entry more than there are shards, mean_cov and tables one per shard")
        rs, re = np.ascontiguousarray(region_start, np.uint32), np.ascontiguousarray(region_end, np.uint32)
        ss = np.ascontiguousarray(sample_size, np.int32)
        R = len(rs)
        if not (len(re) == R and len(ss) == R):
            raise ValueError(what + ": array lengths disagree")
        if len(reg_off) and int(reg_off[-1]) != R:
            raise ValueError(what + ": reg_off must end at the number of regions")
        hs = _handles(shards)
        ts = _handles(tables)
        mc = np.ascontiguousarray(mean_cov, np.float64)
        t = _lib.csv_cn_table_regions(len(shards), C.cast(hs, C.c_void_p), C.cast(ts, C.c_void_p), ptr(mc), ptr(reg_off), ptr(rs), ptr(re), ptr(ss))
        return t, (hs, ts, mc, reg_off, rs, re, ss), R

    def _cn_call(self, R, cap, retry, decode, want_observations, call):
        """The result handling of the four copy-number calls: the arrays for `cap` observations, the call, and the answer cut to its count.
        None when the library declines; CSV_ECAPACITY: with `retry`, once more with the count the library answers, else CsvError with that
        count in `needed`."""
        while True:
            m = max(cap, 1)
            off = np.zeros(R + 1, np.uint64)
            pos = np.zeros(m, np.uint32)
            states, ll = (np.zeros(m, np.int32), np.zeros(max(R, 1), np.float64)) if decode else (None, None)
            baf, pfb, l2 = ((np.zeros(m, np.float64) if want_observations else None) for _ in range(3))
            snp = np.zeros(m, np.uint8) if want_observations else None
            n = C.c_uint64(cap)
            rc = call(off, pos, states, ll, baf, pfb, l2, snp, n)
            if rc == 1:
                return None
            if rc == _lib.CSV_ECAPACITY:
                if retry and int(n.value) > cap:
                    cap = int(n.value)
                    continue
                e = self._error(rc)
                e.needed = int(n.value)
                raise e
            self._check(rc)
            k = int(n.value)
            out = dict(obs_off=off, pos=pos[:k].copy())
            if decode:
                out.update(states=states[:k].copy(), loglik=ll[:R].copy())
            if want_observations:
                out.update(baf=baf[:k].copy(), pfb=pfb[:k].copy(), log2_cov=l2[:k].copy(), is_snp=snp[:k].copy())
            return out

    def cn_observations_tables(self, shards, tables, mean_cov, reg_off, region_start, region_end, sample_size, capacity: int | None = None):
        """csvgpu_cn_observations_tables_many: cn_observations with the SNP records looked up on the device in tables[c] (a SnpTable of this
        device per shard, None: no SNPs); sample_size[r] is the floor of region r's window count. -> the same dict, byte for byte; None when
        the library declines (a region whose records call for more than 5087 windows: `last_error()` says why). capacity given and below
        the bound (windows + 3 records): CsvError(CSV_ECAPACITY) with that bound in `needed`."""
        t, keep, R = self._cn_table_regions(shards, tables, mean_cov, reg_off, region_start, region_end, sample_size, "cn_observations_tables")
        return self._cn_call(R, capacity or 0, capacity is None, False, True, lambda off, pos, st, ll, baf, pfb, l2, snp, n: self.lib.csvgpu_cn_observations_tables_many(
            self.h, C.byref(t), ptr(off), ptr(pos), ptr(baf), ptr(pfb), ptr(l2), ptr(snp), C.byref(n)))

    def cn_decode_tables(self, hmm: csv_hmm, shards, tables, mean_cov, reg_off, region_start, region_end, sample_size, want_observations: bool = False,
                         capacity: int | None = None):
        """csvgpu_cn_decode_tables_many: cn_decode on resident SNP tables -> the same dict, bit for bit; None when the library declines."""
        t, keep, R = self._cn_table_regions(shards, tables, mean_cov, reg_off, region_start, region_end, sample_size, "cn_decode_tables")
        return self._cn_call(R, capacity or 0, capacity is None, True, want_observations, lambda off, pos, st, ll, baf, pfb, l2, snp, n: self.lib.csvgpu_cn_decode_tables_many(
            self.h, C.byref(t), C.byref(hmm), ptr(off), ptr(pos), ptr(st), ptr(ll), ptr(baf), ptr(pfb), ptr(l2), ptr(snp), C.byref(n)))

    def last_error(self) -> str:
        return (self.lib.csvgpu_last_error(self.h) or b"").decode(errors="replace")

    # -------------------------------------------------------------------------------- BGZF members
    def bgzf_inflate(self, comp, blocks, out):
        """csvgpu_bgzf_inflate: the members `blocks` (_lib.BGZF_BLOCK_DTYPE records) of the compressed bytes `comp` (uint8) inflated on the
        device into `out` (uint8, written in place, only inside the decoded members' ranges). -> (number of declined members, status bytes:
        0 decoded and CRC-checked, 1 declined — decode that member on the host)."""
        comp, blocks = np.ascontiguousarray(comp, np.uint8), np.ascontiguousarray(blocks, _lib.BGZF_BLOCK_DTYPE)
        if out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError("bgzf_inflate: out must be a writeable contiguous uint8 array")
        status = np.full(max(len(blocks), 1), 0xFF, np.uint8)
        rc = self.lib.csvgpu_bgzf_inflate(self.h, ptr(comp), len(comp), ptr(blocks), len(blocks), ptr(out), len(out), ptr(status))
        if rc < 0:
            self._check(rc)
        return rc, status[: len(blocks)]

    def bgzf_inflate_dev(self, d_comp, blocks, d_out, d_status) -> int:
        """csvgpu_bgzf_inflate_dev: the same with comp / out / status as uint8 torch tensors on this context's device; the decoded bytes stay
        there. -> number of declined members."""
        blocks = np.ascontiguousarray(blocks, _lib.BGZF_BLOCK_DTYPE)
        for t in (d_comp, d_out, d_status):
            if not _is_dev(t, 1):
                raise ValueError("bgzf_inflate_dev: contiguous uint8 device tensors expected")
        if d_status.numel() < len(blocks):
            raise ValueError("bgzf_inflate_dev: status shorter than the member table")
        rc = self.lib.csvgpu_bgzf_inflate_dev(self.h, d_comp.data_ptr(), d_comp.numel(), ptr(blocks), len(blocks), d_out.data_ptr(), d_out.numel(),
                                              d_status.data_ptr())
        if rc < 0:
            self._check(rc)
        return rc

    # -------------------------------------------------------------------------------- BAM records
    _BAM_DTYPES = dict(pos=np.int32, flag=np.uint16, mapq=np.uint8, cigar_off=np.uint64, cigar=np.uint32, seq_off=np.uint64, seq=np.uint8,
                       name_off=np.uint64, name=np.uint8, name_hash=np.uint64)
    _BAM_SIZES = dict(pos=4, flag=2, mapq=1, cigar_off=8, cigar=4, seq_off=8, seq=1, name_off=8, name=1, name_hash=8)

    @staticmethod
    def _bam_out(arrays, address, numel, what):
        """csv_bam_out over the caller's arrays (numpy or torch, by the two accessors): the capacities are what the arrays hold."""
        o = _lib.csv_bam_out()
        for k in ("pos", "flag", "mapq", "cigar_off", "cigar"):
            if arrays.get(k) is None:
                raise ValueError(f"{what}: array '{k}' is required")
        for k in Context._BAM_SIZES:
            a = arrays.get(k)
            setattr(o, k, address(a, k) if a is not None else None)
        per_record = [numel(arrays[k]) for k in ("pos", "flag", "mapq", "name_hash") if arrays.get(k) is not None]
        per_record += [numel(arrays[k]) - 1 for k in ("cigar_off", "seq_off", "name_off") if arrays.get(k) is not None]
        if min(per_record) < 0:
            raise ValueError(f"{what}: an offset array needs at least one entry")
        o.cap_records = min(per_record)
        o.cap_cigar = numel(arrays["cigar"])
        o.cap_seq = numel(arrays["seq"]) if arrays.get("seq") is not None else 0
        o.cap_name = numel(arrays["name"]) if arrays.get("name") is not None else 0
        return o

    @staticmethod
    def _bam_counts(c) -> dict:
        d = {k: int(getattr(c, k)) for k in ("n_records", "kept_first", "n_kept", "n_cigar", "n_seq", "n_name", "consumed", "status")}
        d["stopped"] = bool(c.stopped)
        d["reason"], d["offset"] = d["status"] & 0xFF, d["status"] >> 8
        return d

    def _bam_call(self, fn, data_ptr, length, anchors, tid, end, bases, o):
        anchors = np.ascontiguousarray(anchors, np.uint32)
        c = _lib.csv_bam_counts()
        rc = fn(self.h, data_ptr, length, ptr(anchors), len(anchors), int(tid), int(end), int(bases[0]), int(bases[1]), int(bases[2]), C.byref(o), C.byref(c))
        if rc < 0 and rc != _lib.CSV_ECAPACITY:
            self._check(rc)
        return rc, self._bam_counts(c)

    def bam_unpack_into(self, data, anchors, out: dict, tid: int = -1, end: int = 0, bases=(0, 0, 0)):
        """csvgpu_bam_unpack: the decoded BAM record stream `data` (uint8) unpacked on the device into the caller's numpy arrays `out`
        (pos int32, flag uint16, mapq uint8, cigar_off uint64 [records + 1], cigar uint32; optional seq_off + seq, name_off + name,
        name_hash); the capacities are the arrays' lengths. anchors: ascending offsets of record starts, anchors[0] the first record's.
        -> (rc, counts): rc 0 written, 1 declined (counts['reason'] at counts['offset']), CSV_ECAPACITY with the exact counts."""
        data = _as_u8(data)

        def address(a, k):
            if a.dtype != self._BAM_DTYPES[k] or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
                raise ValueError(f"bam_unpack: '{k}' must be a writeable contiguous {np.dtype(self._BAM_DTYPES[k]).name} array")
            return a.ctypes.data
        o = self._bam_out(out, address, len, "bam_unpack")
        return self._bam_call(self.lib.csvgpu_bam_unpack, ptr(data), len(data), anchors, tid, end, bases, o)

    def bam_unpack(self, data, anchors, tid: int = -1, end: int = 0, bases=(0, 0, 0), want_seq=False, want_names=False, want_hashes=False):
        """The same into arrays of exactly the kept records' sizes (a sizing call first: CSV_ECAPACITY carries the exact counts).
        -> dict of the counts and, unless the stream was declined (status != 0), the arrays."""
        def alloc(n_rec, n_cigar, n_seq, n_name):
            a = dict(pos=np.zeros(max(n_rec, 1), np.int32), flag=np.zeros(max(n_rec, 1), np.uint16), mapq=np.zeros(max(n_rec, 1), np.uint8),
                     cigar_off=np.zeros(n_rec + 1, np.uint64), cigar=np.zeros(max(n_cigar, 1), np.uint32))
            if want_seq:
                a.update(seq_off=np.zeros(n_rec + 1, np.uint64), seq=np.zeros(max(n_seq, 1), np.uint8))
            if want_names:
                a.update(name_off=np.zeros(n_rec + 1, np.uint64), name=np.zeros(max(n_name, 1), np.uint8))
            if want_hashes:
                a.update(name_hash=np.zeros(max(n_rec, 1), np.uint64))
            return a
        arrays = alloc(0, 0, 0, 0)
        rc, c = self.bam_unpack_into(data, anchors, arrays, tid, end, bases)
        if rc == _lib.CSV_ECAPACITY:
            arrays = alloc(c["n_kept"], c["n_cigar"], c["n_seq"], c["n_name"])
            rc, c = self.bam_unpack_into(data, anchors, arrays, tid, end, bases)
            if rc < 0:
                self._check(rc)
        if rc == 0:
            n = c["n_kept"]
            for k, a in arrays.items():
                total = {"cigar": c["n_cigar"], "seq": c["n_seq"], "name": c["n_name"]}.get(k, n + 1 if k.endswith("_off") else n)
                c[k] = a[:total]
        return c

    def bam_unpack_dev(self, d_bytes, anchors, out: dict, tid: int = -1, end: int = 0, bases=(0, 0, 0)):
        """csvgpu_bam_unpack_dev: the same with the stream and the outputs as torch tensors on this context's device (element sizes of the
        numpy form: int32 / int16 / uint8 / int64 / int32 bit patterns) — behind bgzf_inflate_dev the bytes never leave the device, and
        pos / flag / mapq / cigar_off / cigar are what wrap_device takes. -> (rc, counts) as bam_unpack_into."""
        def address(t, k):
            if not _is_dev(t, self._BAM_SIZES[k]):
                raise ValueError(f"bam_unpack_dev: '{k}' must be a contiguous device tensor of {self._BAM_SIZES[k]}-byte elements")
            return t.data_ptr()
        if not _is_dev(d_bytes, 1):
            raise ValueError("bam_unpack_dev: contiguous uint8 device tensor expected")
        o = self._bam_out(out, address, lambda t: int(t.numel()), "bam_unpack_dev")
        return self._bam_call(self.lib.csvgpu_bam_unpack_dev, d_bytes.data_ptr(), int(d_bytes.numel()), anchors, tid, end, bases, o)

    # -------------------------------------------------------------------------------- VCF lines
    _VCF_DTYPES = dict(line_off=np.uint32, chrom_len=np.uint32, pos=np.uint32, value=np.float64, defer_off=np.uint32)

    @staticmethod
    def _vcf_out(arrays, address, numel, af, what):
        """csv_vcf_out over the caller's arrays (numpy or torch, by the two accessors): the capacities are what the arrays hold."""
        o = _lib.csv_vcf_out()
        per_record = ["line_off", "pos", "value"] + ([] if af else ["chrom_len"])
        for k in per_record + ["defer_off"]:
            if arrays.get(k) is None:
                raise ValueError(f"{what}: array '{k}' is required")
            setattr(o, k, address(arrays[k], k))
        o.cap = min(numel(arrays[k]) for k in per_record)
        o.cap_defer = numel(arrays["defer_off"])
        return o

    @staticmethod
    def _vcf_counts(c) -> dict:
        d = {k: int(getattr(c, k)) for k in ("n_lines", "n_kept", "n_deferred", "stop_off", "status")}
        d["reason"], d["offset"] = d["status"] & 0xFF, d["status"] >> 8
        return d

    def _vcf_call(self, dev, text_ptr, length, o, af_args):
        c = _lib.csv_vcf_counts()
        if af_args[0] == "snp":
            fn = self.lib.csvgpu_vcf_snp_parse_dev if dev else self.lib.csvgpu_vcf_snp_parse
            rc = fn(self.h, text_ptr, length, int(bool(af_args[1])), int(bool(af_args[2])), C.byref(o), C.byref(c))
        else:
            _, contig, needle, pos_ptr, n = af_args
            contig, needle = (x.encode() if isinstance(x, str) else bytes(x) for x in (contig, needle))
            fn = self.lib.csvgpu_vcf_af_parse_dev if dev else self.lib.csvgpu_vcf_af_parse
            rc = fn(self.h, text_ptr, length, contig, len(contig), needle, len(needle), pos_ptr, n, C.byref(o), C.byref(c))
        if rc < 0 and rc != _lib.CSV_ECAPACITY:
            self._check(rc)
        return rc, self._vcf_counts(c)

    def _vcf_host(self, text, out, af, form):
        text = _as_u8(text)

        def address(a, k):
            if a.dtype != self._VCF_DTYPES[k] or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
                raise ValueError(f"vcf_parse: '{k}' must be a writeable contiguous {np.dtype(self._VCF_DTYPES[k]).name} array")
            return a.ctypes.data
        o = self._vcf_out(out, address, len, af, "vcf_parse")
        return self._vcf_call(False, ptr(text), len(text), o, form)

    def _vcf_sized(self, into, af):
        """a sizing call (CSV_ECAPACITY carries the exact counts), then the call into arrays of exactly those sizes"""
        def alloc(n, d):
            a = dict(line_off=np.zeros(max(n, 1), np.uint32)[:n], pos=np.zeros(max(n, 1), np.uint32)[:n], value=np.zeros(max(n, 1), np.float64)[:n],
                     defer_off=np.zeros(max(d, 1), np.uint32)[:d])
            if not af:
                a["chrom_len"] = np.zeros(max(n, 1), np.uint32)[:n]
            return a
        arrays = alloc(0, 0)
        rc, c = into(arrays)
        if rc == _lib.CSV_ECAPACITY:
            arrays = alloc(c["n_kept"], c["n_deferred"])
            rc, c = into(arrays)
            if rc < 0:
                self._check(rc)
        c["declined"] = rc == 1
        if rc == 0:
            c.update(arrays)
        return c

    def vcf_snp_parse_into(self, text, out: dict, dp_int: bool = True, ad_int: bool = True):
        """csvgpu_vcf_snp_parse: the lines of `text` (uint8: whole VCF data lines, no header) decided on the device by the rules of
        SNPFile::load into the caller's numpy arrays `out` (line_off, chrom_len, pos uint32; value float64: the BAF; defer_off uint32: the
        lines the caller parses itself); the capacities are the arrays' lengths. -> (rc, counts): rc 0 written, 1 declined
        (counts['reason'] at counts['offset']), CSV_ECAPACITY with the exact counts."""
        return self._vcf_host(text, out, False, ("snp", dp_int, ad_int))

    def vcf_snp_parse(self, text, dp_int: bool = True, ad_int: bool = True) -> dict:
        """The same into arrays of exactly the kept and deferred counts -> dict of the counts, 'declined', and (unless declined) the arrays."""
        return self._vcf_sized(lambda a: self.vcf_snp_parse_into(text, a, dp_int, ad_int), False)

    def vcf_af_parse_into(self, text, contig, needle, sorted_pos, out: dict):
        """csvgpu_vcf_af_parse: the population file's lines by the rules of SNPFile::table — the records of `contig` at one of the
        ascending `sorted_pos` whose INFO holds `needle` ("AF=" / "AF_<ethnicity>="); value: the frequency; counts['stop_off']: the first
        line behind the last position (VCF_NO_STOP if none). -> (rc, counts) as vcf_snp_parse_into."""
        sorted_pos = np.ascontiguousarray(sorted_pos, np.uint32)
        return self._vcf_host(text, out, True, ("af", contig, needle, ptr(sorted_pos), len(sorted_pos)))

    def vcf_af_parse(self, text, contig, needle, sorted_pos) -> dict:
        return self._vcf_sized(lambda a: self.vcf_af_parse_into(text, contig, needle, sorted_pos, a), True)

    def _vcf_dev(self, d_text, out, af, form):
        def address(t, k):
            if not _is_dev(t, np.dtype(self._VCF_DTYPES[k]).itemsize):
                raise ValueError(f"vcf_parse_dev: '{k}' must be a contiguous device tensor of {np.dtype(self._VCF_DTYPES[k]).itemsize}-byte elements")
            return t.data_ptr()
        if not _is_dev(d_text, 1):
            raise ValueError("vcf_parse_dev: contiguous uint8 device tensor expected")
        o = self._vcf_out(out, address, lambda t: int(t.numel()), af, "vcf_parse_dev")
        return self._vcf_call(True, d_text.data_ptr(), int(d_text.numel()), o, form)

    def vcf_snp_parse_dev(self, d_text, out: dict, dp_int: bool = True, ad_int: bool = True):
        """csvgpu_vcf_snp_parse_dev: the same with the text (at any alignment: what bgzf_inflate_dev left) and the outputs as torch tensors
        on this context's device (4-byte elements; value 8-byte). -> (rc, counts) as vcf_snp_parse_into."""
        return self._vcf_dev(d_text, out, False, ("snp", dp_int, ad_int))

    def vcf_af_parse_dev(self, d_text, contig, needle, d_sorted_pos, out: dict):
        """csvgpu_vcf_af_parse_dev: d_sorted_pos a device tensor of 4-byte elements, ascending (not checked)."""
        if not _is_dev(d_sorted_pos, 4):
            raise ValueError("vcf_af_parse_dev: sorted_pos must be a contiguous device tensor of 4-byte elements")
        return self._vcf_dev(d_text, out, True, ("af", contig, needle, d_sorted_pos.data_ptr(), int(d_sorted_pos.numel())))

    # -------------------------------------------------------------------------------- timing
    def synchronize(self):
        self._check(self.lib.csvgpu_synchronize(self.h))

    def timing_enable(self, on=True):
        """0 / False: off; 1 / True: HIP-event timers around every kernel group; 2: only around the CIGAR scan and the depth pass."""
        self._check(self.lib.csvgpu_timing_enable(self.h, int(on)))

    def timing_reset(self):
        self._check(self.lib.csvgpu_timing_reset(self.h))

    def timing(self) -> dict:
        out = {}
        for k, name in enumerate(_lib.KERNEL_NAMES):
            ms, n = C.c_double(0), C.c_uint64(0)
            self._check(self.lib.csvgpu_timing_get(self.h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    # -------------------------------------------------------------------------------- resident shards
    def upload(self, reads: Reads, depth_len: int) -> "Shard":
        rs = reads.c_struct()
        h = self.lib.csvgpu_shard_upload(self.h, C.byref(rs), depth_len)
        if not h:
            raise self._error(_lib.CSV_ENOMEM)
        return Shard(self, h, reads.n_reads, depth_len)

    def wrap_device_ptrs(self, n_reads: int, n_cigar: int, pos: int, flag: int, mapq: int, cigar_off: int, cigar: int, depth_len: int, keep=None) -> "Shard":
        """Arrays that already live in HBM, given as device addresses (csv_reads layouts), wrapped without a copy
        (csvgpu_shard_wrap_dev). They must outlive the shard; `keep` is held by it for that purpose."""
        r = csv_reads()
        r.n_reads, r.n_cigar = n_reads, n_cigar
        r.pos, r.flag, r.mapq, r.tid, r.cigar_off, r.cigar = pos, flag, mapq, None, cigar_off, cigar       # (void * fields)
        h = self.lib.csvgpu_shard_wrap_dev(self.h, C.byref(r), depth_len)
        if not h:
            raise self._error(_lib.CSV_EINVAL)
        sh = Shard(self, h, n_reads, depth_len)
        sh._keep = keep
        return sh

    def wrap_device(self, pos, flag, mapq, cigar_off, cigar, depth_len: int) -> "Shard":
        """The same for torch tensors on this context's device (int32 / int16 / uint8 / int64 / int32 bit patterns of csv_reads)."""
        n, m = int(pos.numel()), int(cigar.numel())
        if not (flag.numel() == n and mapq.numel() == n and cigar_off.numel() == n + 1):
            raise ValueError("wrap_device: array lengths disagree")
        for t, size in ((pos, 4), (flag, 2), (mapq, 1), (cigar_off, 8), (cigar, 4)):
            if not _is_dev(t, size):
                raise ValueError("wrap_device: tensors must be contiguous device tensors of the csv_reads element sizes")
        return self.wrap_device_ptrs(n, m, pos.data_ptr(), flag.data_ptr(), mapq.data_ptr(), cigar_off.data_ptr(), cigar.data_ptr(), depth_len,
                                     keep=(pos, flag, mapq, cigar_off, cigar))


    # -------------------------------------------------------------------------------- shards built on the device
    def shard_builder(self, want: int = 0, reserve=None) -> "ShardBuilder":
        """csvgpu_shard_builder_create: a resident shard that grows on the device, batch by batch. want: _lib.SB_SEQ | SB_NAMES |
        SB_NAME_HASH; reserve: (n_reads, n_cigar, n_seq, n_name) allocated now, or None."""
        return ShardBuilder(self, want, reserve)

    def genome_builder(self, reserve_bytes: int = 0) -> "GenomeBuilder":
        """csvgpu_genome_builder_create: a reference genome that is built on the device from FASTA text. reserve_bytes: room allocated now
        (the file's size: the array never grows then)."""
        return GenomeBuilder(self, reserve_bytes)

    def snp_builder(self, reserve: int = 0) -> "SnpBuilder":
        """csvgpu_snp_builder_create: per-contig SNP columns that are built on the device from VCF text batches. reserve: records
        allocated now."""
        return SnpBuilder(self, reserve)

    # -------------------------------------------------------------------------------- VCF records formatted on the device
    def vcf_format_raw(self, genome: "Genome", contigs, calls, alts, method: bytes, cap: int, text_ptr, dev: bool = False):
        """One csvgpu_vcf_format (dev: _dev) call. contigs: [(name, n_calls, shard or None, gaps or None[, record])] — gaps = (gap_start,
        gap_end) BED rows in file order, record = the genome record's index (-1: none; left out: the last record of that name, -1 when there
        is none); calls: all contigs' calls in order (_lib.VCF_CALL_DTYPE); alts: one bytes per call; text_ptr: `cap` writeable bytes (an
        address; the device's with dev). -> (rc, line_status uint8[n], counts dict)."""
        calls = np.ascontiguousarray(calls, _lib.VCF_CALL_DTYPE)
        alts = [a.encode("latin-1") if isinstance(a, str) else bytes(a) for a in alts]
        if len(alts) != len(calls) or sum(int(c[1]) for c in contigs) != len(calls):
            raise ValueError("vcf_format: array lengths disagree")
        n_contigs = len(contigs)
        call_off, alt_off = np.zeros(n_contigs + 1, np.uint64), np.zeros(len(calls) + 1, np.uint64)
        call_off[1:] = np.cumsum([int(c[1]) for c in contigs], dtype=np.uint64)
        alt_off[1:] = np.cumsum([len(a) for a in alts], dtype=np.uint64)
        alt_bytes = np.frombuffer(b"".join(alts) + b"\0", np.uint8)
        tab = (_lib.csv_vcf_contig * max(n_contigs, 1))()
        keep = []                                          # what the table points into
        for t, c in enumerate(contigs):
            name = c[0].encode("latin-1") if isinstance(c[0], str) else bytes(c[0])
            name_arr = np.frombuffer(name + b"\0", np.uint8)
            shard, gaps = c[2], c[3] if len(c) > 3 else None
            if len(c) > 4:
                record = int(c[4])
            else:
                try:
                    record = genome.record_of(name)
                except KeyError:
                    record = -1
            gs, ge = (np.ascontiguousarray(g, np.uint32) for g in gaps) if gaps is not None else (np.zeros(0, np.uint32),) * 2
            if len(gs) != len(ge):
                raise ValueError("vcf_format: gap arrays disagree")
            keep += [name_arr, gs, ge]
            tab[t] = _lib.csv_vcf_contig(ptr(name_arr), len(name), record, shard.h if shard is not None else None, ptr(gs) if len(gs) else None,
                                         ptr(ge) if len(ge) else None, len(gs))
        status = np.zeros(max(len(calls), 1), np.uint8)
        cnt = _lib.csv_vcf_format_counts()
        method = np.frombuffer(bytes(method) + b"\0", np.uint8)
        fn = self.lib.csvgpu_vcf_format_dev if dev else self.lib.csvgpu_vcf_format
        rc = fn(self.h, genome.h, tab, n_contigs, ptr(call_off), ptr(calls) if len(calls) else None, ptr(alt_off), ptr(alt_bytes), ptr(method), len(method) - 1,
                int(cap), text_ptr, ptr(status), C.byref(cnt))
        counts = {k: int(getattr(cnt, k)) for k in ("text_bytes", "n_lines", "total", "unclassified", "gap_filtered", "declined_why")}
        return rc, status[: len(calls)], counts

    def vcf_format(self, genome: "Genome", contigs, calls, alts, method: bytes = b"ContextSV v1.0.0"):
        """csvgpu_vcf_format: the record lines of the VCF writer for `calls`, assembled on the device from the resident genome and the
        shards' depth maps -> (text: bytes, line_status: uint8[n], counts: dict). Arguments as vcf_format_raw. Two calls: the first sizes the
        second. A declined batch returns text=None with counts["declined_why"] set; CSV_E* raises."""
        rc, status, counts = self.vcf_format_raw(genome, contigs, calls, alts, method, 0, None)
        if rc == _lib.CSV_ECAPACITY:
            out = np.zeros(counts["text_bytes"], np.uint8)
            rc, status, counts = self.vcf_format_raw(genome, contigs, calls, alts, method, len(out), ptr(out))
            if rc == _lib.CSV_OK:
                return out.tobytes(), status, counts
        if rc == 1:
            return None, status, counts
        self._check(rc)
        return b"", status, counts

    def alt_bases(self, shard: "Shard", read, qpos, lengths):
        """csvgpu_alt_bases_resident: for item i the `lengths[i]` bases from query offset qpos[i] of record read[i], cut from the packed
        sequences a built shard holds (ambiguity codes as N; all N where the bases leave the stored sequence) -> list of str."""
        read, qpos = np.ascontiguousarray(read, np.uint32), np.ascontiguousarray(qpos, np.uint32)
        off = np.zeros(len(read) + 1, np.uint64)
        off[1:] = np.cumsum(np.asarray(lengths, np.uint64), dtype=np.uint64)
        if len(qpos) != len(read) or len(off) != len(read) + 1:
            raise ValueError("alt_bases: array lengths disagree")
        out = np.zeros(max(int(off[-1]), 1), np.uint8)
        self._check(self.lib.csvgpu_alt_bases_resident(self.h, shard.h, ptr(read), ptr(qpos), ptr(off), len(read), ptr(out)))
        text = out.tobytes().decode("latin-1")
        return [text[int(off[i]): int(off[i + 1])] for i in range(len(read))]


class SnpTable:
    """One contig's SNP records resident on the device (csv_snp_table): immutable, readable from every Context of its device."""

    def __init__(self, ctx: Context, handle):
        self.ctx, self.h = ctx, handle
        self.n = int(ctx.lib.csvgpu_snp_table_size(handle))

    def free(self):
        if self.h:
            self.ctx.lib.csvgpu_snp_table_free(self.ctx.h, self.h)
            self.h = None


class SnpBuilder:
    """csv_snp_builder: the kept SNP records of VCF text batches in device arrays that grow, cut into CHROM runs on the device; finish()
    orders them by (contig id, order key) and gives SnpColumns."""

    _RUN_KEYS = ("run_first", "run_line_off", "run_chrom_len")

    def __init__(self, ctx: Context, reserve: int = 0):
        self.ctx = ctx
        self.h = ctx.lib.csvgpu_snp_builder_create(ctx.h, int(reserve))
        if not self.h:
            raise ctx._error(_lib.CSV_ENOMEM)

    def _live(self):
        if not self.h:
            raise ValueError("SnpBuilder: already finished or destroyed")

    def _append(self, dev, text_ptr, length, text_base, out, dp_int, ad_int):
        self._live()
        o = _lib.csv_snp_runs()
        for k in self._RUN_KEYS + ("defer_off",):
            a = out.get(k)
            if a is None or a.dtype != np.uint32 or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
                raise ValueError(f"snp_builder.append: '{k}' must be a writeable contiguous uint32 array")
            setattr(o, k, a.ctypes.data)
        o.cap_runs = min(len(out[k]) for k in self._RUN_KEYS)
        o.cap_defer = len(out["defer_off"])
        c = _lib.csv_snp_append_counts()
        fn = self.ctx.lib.csvgpu_snp_builder_append_dev if dev else self.ctx.lib.csvgpu_snp_builder_append
        rc = fn(self.ctx.h, self.h, text_ptr, int(length), int(text_base), int(bool(dp_int)), int(bool(ad_int)), C.byref(o), C.byref(c))
        d = {k: int(getattr(c, k)) for k in ("n_lines", "n_kept", "n_deferred", "n_runs", "first_run", "status")}
        d["reason"], d["offset"] = d["status"] & 0xFF, d["status"] >> 8
        return rc, d

    def append_into(self, text, out: dict, text_base: int = 0, dp_int: bool = True, ad_int: bool = True):
        """csvgpu_snp_builder_append: whole VCF data lines (bytes or a uint8 array) whose first byte is byte `text_base` of the file. out:
        uint32 numpy arrays run_first / run_line_off / run_chrom_len (the call's CHROM runs) and defer_off; the capacities are their
        lengths. -> (rc, counts): rc 0 appended, 1 declined, or a negative CSV_E* (CSV_ECAPACITY with the exact counts, CSV_ENOMEM with
        the builder unchanged)."""
        data = _as_u8(text)
        return self._append(False, ptr(data) if len(data) else None, len(data), text_base, out, dp_int, ad_int)

    def append_dev_into(self, d_text, out: dict, text_base: int = 0, dp_int: bool = True, ad_int: bool = True):
        """csvgpu_snp_builder_append_dev: the same for a uint8 torch tensor on the context's device, at any alignment."""
        if not _is_dev(d_text, 1):
            raise ValueError("append_dev: contiguous uint8 device tensor expected")
        return self.append_ptr_into(d_text.data_ptr(), int(d_text.numel()), out, text_base, dp_int, ad_int)

    def append_ptr_into(self, dev_ptr: int, length: int, out: dict, text_base: int = 0, dp_int: bool = True, ad_int: bool = True):
        """The same for `length` bytes at a device address."""
        return self._append(True, dev_ptr if length else None, length, text_base, out, dp_int, ad_int)

    def _sized(self, into):
        def alloc(r, d):
            a = {k: np.zeros(max(r, 1), np.uint32)[:r] for k in self._RUN_KEYS}
            a["defer_off"] = np.zeros(max(d, 1), np.uint32)[:d]
            return a
        arrays = alloc(0, 0)
        rc, c = into(arrays)
        if rc == _lib.CSV_ECAPACITY:
            arrays = alloc(c["n_runs"], c["n_deferred"])
            rc, c = into(arrays)
        if rc < 0:
            self.ctx._check(rc)
        c["declined"] = rc == 1
        if rc == 0:
            c.update(arrays)
        return c

    def append(self, text, text_base: int = 0, dp_int: bool = True, ad_int: bool = True) -> dict:
        """The same into arrays of exactly the run and deferred counts (a sizing call first) -> dict of the counts, 'declined', and
        (unless declined) the arrays."""
        return self._sized(lambda a: self.append_into(text, a, text_base, dp_int, ad_int))

    def append_dev(self, d_text, text_base: int = 0, dp_int: bool = True, ad_int: bool = True) -> dict:
        return self._sized(lambda a: self.append_dev_into(d_text, a, text_base, dp_int, ad_int))

    def append_host_raw(self, contig_id, order_key, pos, baf) -> int:
        """csvgpu_snp_builder_append_host -> status."""
        self._live()
        cid, key = np.ascontiguousarray(contig_id, np.uint32), np.ascontiguousarray(order_key, np.uint64)
        pos, baf = np.ascontiguousarray(pos, np.uint32), np.ascontiguousarray(baf, np.float64)
        if not len(cid) == len(key) == len(pos) == len(baf):
            raise ValueError("append_host: array lengths disagree")
        return self.ctx.lib.csvgpu_snp_builder_append_host(self.ctx.h, self.h, len(cid), ptr(cid), ptr(key), ptr(pos), ptr(baf))

    def append_host(self, contig_id, order_key, pos, baf):
        """Records the host parser kept (deferred lines, declined batches), each with its contig id (< 2^16) and its line's file offset."""
        self.ctx._check(self.append_host_raw(contig_id, order_key, pos, baf))

    def finish(self, run_contig) -> "SnpColumns":
        """csvgpu_snp_builder_finish: run_contig[r] = the contig id of global run r. The builder is consumed, also on failure."""
        self._live()
        rc_ = np.ascontiguousarray(run_contig, np.uint32)
        h, self.h = self.ctx.lib.csvgpu_snp_builder_finish(self.ctx.h, self.h, ptr(rc_) if len(rc_) else None, len(rc_)), None
        if not h:
            raise self.ctx._error(_lib.CSV_EINVAL)
        return SnpColumns(self.ctx, h)

    def destroy(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.csvgpu_snp_builder_destroy(self.ctx.h, self.h)
        self.h = None

    __del__ = destroy


class SnpColumns:
    """csv_snp_columns: per-contig pos / baf columns resident on the device, in file order inside each contig."""

    def __init__(self, ctx: Context, handle):
        self.ctx, self.h = ctx, handle

    def free(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.csvgpu_snp_columns_free(self.ctx.h, self.h)
        self.h = None

    __del__ = free

    def describe(self) -> dict:
        """-> dict(contig_id uint32, count uint64, ascending bool) of the contigs that hold a record, by ascending id."""
        n = C.c_uint64(0)
        self.ctx.lib.csvgpu_snp_columns_describe(self.h, 0, None, None, None, C.byref(n))
        k = int(n.value)
        cid, cnt, asc = np.zeros(max(k, 1), np.uint32)[:k], np.zeros(max(k, 1), np.uint64)[:k], np.zeros(max(k, 1), np.uint8)[:k]
        self.ctx._check(self.ctx.lib.csvgpu_snp_columns_describe(self.h, k, ptr(cid), ptr(cnt), ptr(asc), C.byref(n)))
        return dict(contig_id=cid, count=cnt, ascending=asc.astype(bool))

    def fetch(self, contig_id: int, want_pos: bool = True, want_baf: bool = True):
        """csvgpu_snp_columns_fetch -> (pos uint32 or None, baf float64 or None) of one contig."""
        d = self.describe()
        at = np.nonzero(d["contig_id"] == contig_id)[0]
        k = int(d["count"][at[0]]) if len(at) else 0
        pos = np.zeros(max(k, 1), np.uint32)[:k] if want_pos else None
        baf = np.zeros(max(k, 1), np.float64)[:k] if want_baf else None
        self.ctx._check(self.ctx.lib.csvgpu_snp_columns_fetch(self.ctx.h, self.h, int(contig_id), ptr(pos), ptr(baf)))
        return pos, baf

    def _af_call(self, dev, contig_id, text_ptr, length, contig, needle, o):
        c = _lib.csv_vcf_counts()
        contig, needle = (x.encode() if isinstance(x, str) else bytes(x) for x in (contig, needle))
        fn = self.ctx.lib.csvgpu_snp_columns_af_parse_dev if dev else self.ctx.lib.csvgpu_snp_columns_af_parse
        rc = fn(self.ctx.h, self.h, int(contig_id), text_ptr, int(length), contig, len(contig), needle, len(needle), C.byref(o), C.byref(c))
        if rc < 0 and rc != _lib.CSV_ECAPACITY:
            self.ctx._check(rc)
        return rc, Context._vcf_counts(c)

    def af_parse_into(self, contig_id: int, text, contig, needle, out: dict):
        """csvgpu_snp_columns_af_parse: Context.vcf_af_parse_into with sorted_pos = the contig's resident positions. -> (rc, counts)."""
        text = _as_u8(text)

        def address(a, k):
            if a.dtype != Context._VCF_DTYPES[k] or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
                raise ValueError(f"af_parse: '{k}' must be a writeable contiguous {np.dtype(Context._VCF_DTYPES[k]).name} array")
            return a.ctypes.data
        o = Context._vcf_out(out, address, len, True, "af_parse")
        return self._af_call(False, contig_id, ptr(text), len(text), contig, needle, o)

    def af_parse(self, contig_id: int, text, contig, needle) -> dict:
        """The same into arrays of exactly the kept and deferred counts, as Context.vcf_af_parse."""
        return self.ctx._vcf_sized(lambda a: self.af_parse_into(contig_id, text, contig, needle, a), True)

    def af_parse_dev(self, contig_id: int, d_text, contig, needle, out: dict):
        """csvgpu_snp_columns_af_parse_dev: the text and the outputs as torch tensors on the context's device. -> (rc, counts)."""
        def address(t, k):
            if not _is_dev(t, np.dtype(Context._VCF_DTYPES[k]).itemsize):
                raise ValueError(f"af_parse_dev: '{k}' must be a contiguous device tensor of {np.dtype(Context._VCF_DTYPES[k]).itemsize}-byte elements")
            return t.data_ptr()
        if not _is_dev(d_text, 1):
            raise ValueError("af_parse_dev: contiguous uint8 device tensor expected")
        o = Context._vcf_out(out, address, lambda t: int(t.numel()), True, "af_parse_dev")
        return self._af_call(True, contig_id, d_text.data_ptr(), int(d_text.numel()), contig, needle, o)

    def table(self, contig_id: int, af_pos, af) -> "SnpTable":
        """csvgpu_snp_columns_table: the first-hit table of one ascending contig, its records copied on the device; af_pos / af numpy."""
        af_pos, af = np.ascontiguousarray(af_pos, np.uint32), np.ascontiguousarray(af, np.float64)
        if len(af_pos) != len(af):
            raise ValueError("table: af_pos and af differ in length")
        h = self.ctx.lib.csvgpu_snp_columns_table(self.ctx.h, self.h, int(contig_id), ptr(af_pos), ptr(af), len(af))
        if not h:
            raise self.ctx._error(_lib.CSV_EINVAL)
        return SnpTable(self.ctx, h)


class GenomeBuilder:
    """csv_genome_builder: FASTA text appended in pieces (cut anywhere) into one base array the library owns; finish() gives a Genome."""

    def __init__(self, ctx: Context, reserve_bytes: int = 0):
        self.ctx = ctx
        self.h = ctx.lib.csvgpu_genome_builder_create(ctx.h, int(reserve_bytes))
        if not self.h:
            raise ctx._error(_lib.CSV_ENOMEM)

    def _live(self):
        if not self.h:
            raise ValueError("GenomeBuilder: already finished or destroyed")

    def append(self, text):
        """csvgpu_genome_builder_append: the next bytes of the text (bytes or a uint8 numpy array), through the page-locked block."""
        self._live()
        data = _as_u8(text)
        self.ctx._check(self.ctx.lib.csvgpu_genome_builder_append(self.ctx.h, self.h, ptr(data) if len(data) else None, len(data)))

    def append_dev(self, d_text):
        """csvgpu_genome_builder_append_dev: the same for a uint8 torch tensor on the context's device, at any alignment."""
        self._live()
        if not _is_dev(d_text, 1):
            raise ValueError("append_dev: contiguous uint8 device tensor expected")
        self.append_ptr(d_text.data_ptr(), int(d_text.numel()))

    def append_ptr(self, dev_ptr: int, length: int):
        """The same for `length` bytes at a device address."""
        self._live()
        self.ctx._check(self.ctx.lib.csvgpu_genome_builder_append_dev(self.ctx.h, self.h, dev_ptr if length else None, int(length)))

    def finish(self) -> "Genome":
        """csvgpu_genome_builder_finish: the builder's array becomes a Genome (the builder is consumed, also on failure)."""
        self._live()
        h, self.h = self.ctx.lib.csvgpu_genome_builder_finish(self.ctx.h, self.h), None
        if not h:
            raise self.ctx._error(_lib.CSV_EINVAL)
        return Genome(self.ctx, h)

    def destroy(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.csvgpu_genome_builder_destroy(self.ctx.h, self.h)
        self.h = None

    __del__ = destroy


class Genome:
    """csv_genome: a reference genome resident on the device. Records are the FASTA's named headers in file order."""

    def __init__(self, ctx: Context, handle):
        self.ctx, self.h = ctx, handle
        self._desc = None

    def free(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.csvgpu_genome_free(self.ctx.h, self.h)
        self.h = None

    __del__ = free

    def describe_raw(self, cap_records: int, cap_name_bytes: int):
        """One csvgpu_genome_describe call with the given capacities -> (rc, counts dict, name_off, names, lengths)."""
        name_off, names, lengths = np.zeros(cap_records + 1, np.uint64), np.zeros(max(cap_name_bytes, 1), np.uint8), np.zeros(max(cap_records, 1), np.uint32)
        c = _lib.csv_genome_counts()
        rc = self.ctx.lib.csvgpu_genome_describe(self.ctx.h, self.h, cap_records, cap_name_bytes, ptr(name_off), ptr(names), ptr(lengths), C.byref(c))
        counts = {k: int(getattr(c, k)) for k in ("n_records", "n_name_bytes", "total_bases", "n_text_bytes", "n_lines")}
        return rc, counts, name_off, names, lengths

    def describe(self) -> dict:
        """The records: names (bytes, file order, duplicates kept), lengths, and the counts (two calls: the first sizes the second)."""
        if self._desc is None:
            rc, counts, *_ = self.describe_raw(0, 0)
            if rc not in (_lib.CSV_OK, _lib.CSV_ECAPACITY):
                self.ctx._check(rc)
            rc, counts, name_off, names, lengths = self.describe_raw(counts["n_records"], counts["n_name_bytes"])
            self.ctx._check(rc)
            raw, n = names.tobytes(), counts["n_records"]
            self._desc = dict(counts, names=[raw[int(name_off[i]): int(name_off[i + 1])] for i in range(n)], lengths=lengths[:n].copy())
        return self._desc

    def record_of(self, name) -> int:
        """The LAST record of that name (the host loader's map keeps the last one stored). KeyError when there is none."""
        name = name.encode("latin-1") if isinstance(name, str) else bytes(name)
        names = self.describe()["names"]
        for i in range(len(names) - 1, -1, -1):
            if names[i] == name:
                return i
        raise KeyError(name)

    @staticmethod
    def cut_len(length: int, pos_start: int, pos_end: int) -> int:
        ps, pe = (pos_start - 1) & 0xFFFFFFFF, (pos_end - 1) & 0xFFFFFFFF
        return 0 if pe >= length or ps > pe else pe - ps + 1

    def fetch_raw(self, record, pos_start, pos_end, out_off, mask: bool, out) -> int:
        """One csvgpu_genome_fetch call on the caller's arrays; out: a writeable uint8 array. -> rc."""
        record, pos_start, pos_end = (np.ascontiguousarray(a, np.uint32) for a in (record, pos_start, pos_end))
        out_off = np.ascontiguousarray(out_off, np.uint64)
        if not (len(pos_start) == len(record) == len(pos_end) and len(out_off) == len(record) + 1):
            raise ValueError("fetch: array lengths disagree")
        return self.ctx.lib.csvgpu_genome_fetch(self.ctx.h, self.h, ptr(record), ptr(pos_start), ptr(pos_end), ptr(out_off), len(record), int(bool(mask)), ptr(out))

    def fetch(self, record, pos_start, pos_end, mask: bool = False):
        """The cuts [pos_start[i], pos_end[i]] (1-based inclusive, ReferenceGenome::query's rule) of records record[i] -> list of bytes."""
        lengths = self.describe()["lengths"]
        record = np.ascontiguousarray(record, np.uint32)
        if len(record) and int(record.max()) >= len(lengths):
            raise CsvError(_lib.CSV_EINVAL, "genome_fetch: record index beyond the genome")
        off = np.zeros(len(record) + 1, np.uint64)
        off[1:] = np.cumsum([self.cut_len(int(lengths[r]), int(s), int(e)) for r, s, e in zip(record, pos_start, pos_end)], dtype=np.uint64)
        out = np.zeros(max(int(off[-1]), 1), np.uint8)
        self.ctx._check(self.fetch_raw(record, pos_start, pos_end, off, mask, out))
        raw = out.tobytes()
        return [raw[int(off[i]): int(off[i + 1])] for i in range(len(record))]


class ShardBuilder:
    """csv_shard_builder: BAM batches appended on the device into arrays the library owns; finish() turns them into a Shard."""

    def __init__(self, ctx: Context, want: int = 0, reserve=None):
        self.ctx, self.want = ctx, int(want)
        r = _lib.csv_shard_sizes(*[int(x) for x in reserve]) if reserve is not None else None
        self.h = ctx.lib.csvgpu_shard_builder_create(ctx.h, self.want, C.byref(r) if r is not None else None)
        if not self.h:
            raise ctx._error(_lib.CSV_ENOMEM)

    def _live(self):
        if not self.h:
            raise ValueError("ShardBuilder: already finished or destroyed")

    def append_bam(self, stream_or_dev, anchors, tid: int = -1, end: int = 0):
        """csvgpu_shard_builder_append_bam: a decoded BAM record stream — host bytes / a uint8 numpy array (copied to a device buffer for the
        call) or a uint8 torch tensor on the context's device, e.g. what bgzf_inflate_dev left there — unpacked behind the builder's tail.
        -> (rc, counts) as Context.bam_unpack_into: rc 0 appended, 1 declined (nothing appended; counts['reason'] at counts['offset']);
        CsvError otherwise (CSV_ENOMEM: a failed growth, the builder keeps its contents)."""
        ctx = self.ctx
        if hasattr(stream_or_dev, "data_ptr"):
            t = stream_or_dev
            if not _is_dev(t, 1):
                raise ValueError("append_bam: contiguous uint8 device tensor expected")
            return self.append_bam_ptr(t.data_ptr(), int(t.numel()), anchors, tid, end)
        data = stream_or_dev
        data = _as_u8(data)
        dev = ctx.lib.csvgpu_dev_alloc(ctx.h, max(len(data), 1))
        if not dev:
            raise ctx._error(_lib.CSV_ENOMEM)
        try:
            ctx._check(ctx.lib.csvgpu_upload(ctx.h, dev, ptr(data), len(data)))
            return self.append_bam_ptr(dev, len(data), anchors, tid, end)
        finally:
            ctx.lib.csvgpu_dev_free(ctx.h, dev)

    def append_bam_ptr(self, dev_ptr: int, length: int, anchors, tid: int = -1, end: int = 0):
        """The same for `length` bytes at a device address (csvgpu_dev_alloc, or a tensor's data_ptr())."""
        self._live()
        anchors = np.ascontiguousarray(anchors, np.uint32)
        c = _lib.csv_bam_counts()
        rc = self.ctx.lib.csvgpu_shard_builder_append_bam(self.ctx.h, self.h, dev_ptr, int(length), ptr(anchors), len(anchors), int(tid), int(end), C.byref(c))
        if rc < 0:
            self.ctx._check(rc)
        return rc, Context._bam_counts(c)

    def append_host(self, reads: Reads, seq_off=None, seq=None, name_off=None, name=None, name_hash=None):
        """csvgpu_shard_builder_append_host: a batch the host parser read, as host arrays (offsets relative to the batch)."""
        self._live()
        u64 = lambda a: np.ascontiguousarray(a, np.uint64) if a is not None else None
        u8 = lambda a: np.ascontiguousarray(a, np.uint8) if a is not None else None
        so, sq, no, nm, nh = u64(seq_off), u8(seq), u64(name_off), u8(name), u64(name_hash)
        rs = reads.c_struct()
        self.ctx._check(self.ctx.lib.csvgpu_shard_builder_append_host(self.ctx.h, self.h, C.byref(rs), ptr(so), ptr(sq), ptr(no), ptr(nm), ptr(nh)))

    def sizes(self) -> dict:
        self._live()
        s = _lib.csv_shard_sizes()
        self.ctx._check(self.ctx.lib.csvgpu_shard_builder_sizes(self.ctx.h, self.h, C.byref(s)))
        return dict(n_reads=s.n_reads, n_cigar=s.n_cigar, n_seq=s.n_seq, n_name=s.n_name)

    def finish(self, depth_len: int) -> "Shard":
        """csvgpu_shard_builder_finish: the builder's arrays become a Shard (the builder is consumed, also on failure)."""
        self._live()
        n = self.sizes()["n_reads"]
        h, self.h = self.ctx.lib.csvgpu_shard_builder_finish(self.ctx.h, self.h, depth_len), None
        if not h:
            raise self.ctx._error(_lib.CSV_ENOMEM)
        return Shard(self.ctx, h, n, depth_len)

    def destroy(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.csvgpu_shard_builder_destroy(self.ctx.h, self.h)
        self.h = None

    __del__ = destroy


@dataclass
class SplitRefs:
    """Record references into resident shards from which the device builds SplitTables (include/csvgpu.h csv_split_refs): segment by segment,
    every member and every supplementary entry as a record index in the segment's shard, or — an entry on another tid — as its flags byte."""
    member_rec: np.ndarray    # uint32 [n_members]  record index in its segment's shard
    supp_off: np.ndarray      # uint64 [n_members + 1]
    supp_rec: np.ndarray      # uint32 [n_supp]  record index in the same shard (not read where supp_where != 0)
    supp_where: np.ndarray    # uint8 [n_supp]  0 = same shard, 2 | reverse = on another tid

    def __post_init__(self):
        self.member_rec = np.ascontiguousarray(self.member_rec, dtype=np.uint32)
        self.supp_off = np.ascontiguousarray(self.supp_off, dtype=np.uint64)
        self.supp_rec = np.ascontiguousarray(self.supp_rec, dtype=np.uint32)
        self.supp_where = np.ascontiguousarray(self.supp_where, dtype=np.uint8)
        if len(self.supp_off) != len(self.member_rec) + 1 or len(self.supp_where) != len(self.supp_rec):
            raise ValueError("SplitRefs: array lengths disagree")

    @property
    def n_members(self) -> int:
        return len(self.member_rec)

    @property
    def n_supp(self) -> int:
        return len(self.supp_rec)

    def c_struct(self) -> csv_split_refs:
        f = csv_split_refs()
        f.n_members, f.n_supp = self.n_members, self.n_supp
        for k in ("member_rec", "supp_off", "supp_rec", "supp_where"):
            setattr(f, k, ptr(getattr(self, k)))
        return f


@dataclass
class ChrResult:
    n_sig: int
    n_del: int
    n_ins: int
    depth_sum: int
    depth_nonzero: int
    min_pts: int
    mean_cov: float
    raw: csv_chr_result


def _merge_records(ctx, capacity, n_sig: int, call):
    """One csvgpu_*merge_select call into a fresh record array; CsvError(CSV_ECAPACITY) carries the counts as .counts."""
    cap = n_sig // 2 + 2 if capacity is None else capacity
    rep = np.zeros(max(cap, 1), _lib.MERGE_REP_DTYPE)
    cnt = _lib.csv_merge_counts()
    rc = call(rep, cap, cnt)
    counts = dict(n_rep=(int(cnt.n_rep[0]), int(cnt.n_rep[1])), n_declined=(int(cnt.n_declined[0]), int(cnt.n_declined[1])))
    if rc == _lib.CSV_ECAPACITY:
        e = ctx._error(rc)
        e.counts = counts
        raise e
    ctx._check(rc)
    return rep[: counts["n_rep"][0] + counts["n_rep"][1]].copy(), counts


class Shard:
    """Reads resident in HBM + the per-chromosome device pipeline (csvgpu_chr_pipeline_dev)."""

    def __init__(self, ctx: Context, handle, n_reads: int, depth_len: int):
        self.ctx, self.h, self.n_reads, self.depth_len = ctx, handle, n_reads, depth_len

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.csvgpu_shard_free(self.ctx.h, self.h)
        self.h = None

    def set_qname_hash(self, qhash):
        qhash = np.ascontiguousarray(qhash, np.uint64)
        assert len(qhash) == self.n_reads
        self.ctx._check(self.ctx.lib.csvgpu_shard_set_qname_hash(self.ctx.h, self.h, ptr(qhash)))

    def sizes(self) -> dict:
        """csvgpu_shard_sizes: records, CIGAR words, and the sequence / name bytes the shard holds (0 where it holds none)."""
        s = _lib.csv_shard_sizes()
        self.ctx._check(self.ctx.lib.csvgpu_shard_sizes(self.ctx.h, self.h, C.byref(s)))
        return dict(n_reads=s.n_reads, n_cigar=s.n_cigar, n_seq=s.n_seq, n_name=s.n_name)

    def cigar_bytes(self) -> int:
        """csvgpu_shard_cigar_bytes: device bytes of the shard's CIGAR array, padding and escape tables included."""
        return int(self.ctx.lib.csvgpu_shard_cigar_bytes(self.h))

    def fetch_reads(self, want_cigar: bool = True) -> Reads:
        """csvgpu_shard_fetch_reads: the shard's reads copied to the host (want_cigar False: pos / flag / mapq only, the CIGAR arrays empty)."""
        z = self.sizes()
        n, m = z["n_reads"], z["n_cigar"] if want_cigar else 0
        pos, flag, mapq = np.zeros(n, np.int32), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
        off, cig = np.zeros(n + 1, np.uint64), np.zeros(m, np.uint32)
        self.ctx._check(self.ctx.lib.csvgpu_shard_fetch_reads(self.ctx.h, self.h, ptr(pos), ptr(flag), ptr(mapq), ptr(off) if want_cigar else None,
                                                              ptr(cig) if want_cigar else None))
        return Reads(pos, flag, mapq, off, cig)

    def fetch_names(self, want_names: bool = True, want_hashes: bool = True) -> dict:
        """csvgpu_shard_fetch_names -> dict(name_off, name, names) and / or dict(name_hash) of a shard built with them."""
        z = self.sizes()
        n = z["n_reads"]
        off, name = (np.zeros(n + 1, np.uint64), np.zeros(z["n_name"], np.uint8)) if want_names else (None, None)
        nh = np.zeros(n, np.uint64) if want_hashes else None
        self.ctx._check(self.ctx.lib.csvgpu_shard_fetch_names(self.ctx.h, self.h, ptr(off), ptr(name), ptr(nh)))
        out = {}
        if want_names:
            raw = name.tobytes()
            out.update(name_off=off, name=name, names=[raw[int(off[i]): int(off[i + 1])] for i in range(n)])
        if want_hashes:
            out["name_hash"] = nh
        return out

    def drop_sequences(self):
        self.ctx._check(self.ctx.lib.csvgpu_shard_drop_sequences(self.ctx.h, self.h))

    def pipeline(self, eps: float = 0.1, min_pts_pct: float = 0.1, min_oplen: int = 50, min_mapq: int = 20) -> ChrResult:
        res = csv_chr_result()
        self.ctx._check(self.ctx.lib.csvgpu_chr_pipeline_dev(self.ctx.h, self.h, min_oplen, min_mapq, eps, min_pts_pct, C.byref(res)))
        return ChrResult(res.n_sig, res.n_del, res.n_ins, res.depth_sum, res.depth_nonzero, res.min_pts, res.mean_cov, res)

    def merge_select(self, res: ChrResult, max_partitions: int = 0, capacity=None):
        """csvgpu_chr_merge_select on the results of this shard's last pipeline: the representatives mergeSVs keeps, chosen on the device
        -> (records[MERGE_REP_DTYPE], counts dict); signatures and labels stay where they are."""
        return _merge_records(self.ctx, capacity, res.n_sig, lambda rep, cap, cnt: self.ctx.lib.csvgpu_chr_merge_select(
            self.ctx.h, self.h, C.byref(res.raw), max_partitions, ptr(rep), cap, C.byref(cnt)))

    def fetch(self, res: ChrResult, want_depth: bool = False):
        """Copy the pipeline's device results to host numpy arrays (test / host-merge plumbing)."""
        def d2h(p, nbytes, dtype):
            if not p or nbytes == 0:
                return np.zeros(0, dtype)
            out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype)
            self.ctx._check(self.ctx.lib.csvgpu_download(self.ctx.h, out.ctypes.data, p, nbytes))
            return out

        r = res.raw
        out = {
            "sig_del": d2h(r.sig_del, res.n_del * 16, SIG_DTYPE),
            "sig_ins": d2h(r.sig_ins, res.n_ins * 16, SIG_DTYPE),
            "label_del": d2h(r.label_del, res.n_del * 4, np.int32),
            "label_ins": d2h(r.label_ins, res.n_ins * 4, np.int32),
            "ref_end": d2h(r.ref_end, self.n_reads * 4, np.int32),
            "q_start": d2h(r.q_start, self.n_reads * 4, np.int32),
            "q_end": d2h(r.q_end, self.n_reads * 4, np.int32),
        }
        if want_depth:
            out["depth"] = d2h(r.depth, self.depth_len * 4, np.uint32)
        return out

    def depth_lookup(self, pos) -> np.ndarray:
        """depth[pos[i]] on the resident depth map; -1 where pos[i] is outside it (csvgpu_depth_lookup_resident)."""
        pos = np.ascontiguousarray(pos, np.uint32)
        out = np.zeros(max(len(pos), 1), np.int32)
        self.ctx._check(self.ctx.lib.csvgpu_depth_lookup_resident(self.ctx.h, self.h, ptr(pos), len(pos), ptr(out)))
        return out[: len(pos)]
