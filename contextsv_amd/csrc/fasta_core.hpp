// fasta_core.hpp — the rules of ReferenceGenome::setFilepath and ::query (host/fasta_query.cpp; the reference's fasta_query.cpp:28-102) and
// of the VCF writer's ambiguity masking (vcf_writer.cpp:18-29), stated once for the device (kernels/fasta.hip, api/fasta.hip) and for the
// CPU check (tools/fuzz/fasta_core_check.cpp). Compiles with g++ alone.
//   Lines      split on '\n' only; a final unterminated line counts; '\r' stays in the data and in a name; an empty line adds nothing.
//   Headers    a non-empty line whose first byte is '>'. Its name: from the byte behind '>' to the first blank or the line's end; may be
//              empty.
//   Residues   every other line's bytes, kept in file order. The loader clears its pending sequence only when it stores a named contig,
//              and it stores one when the NEXT header line (of any name) or the file's end arrives. So the kept bytes are one array, a
//              record per named header in file order, and record k is the run of kept bytes between the store in front of it and its own:
//              [end of record k - 1, kept bytes in front of the first header line behind header k). Residues in front of the first
//              header or under an empty-named header thereby fall to the first named header behind them; kept bytes behind the last store
//              belong to nobody and are dropped.
//   A cut      [pos_start, pos_end] 1-based inclusive, both decremented with uint32 wrap; empty when pos_end >= length or
//              pos_start > pos_end.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#include <string.h>
#endif
#include <string>
#include <vector>

#ifdef __HIPCC__
#define FA_HD __host__ __device__
#else
#define FA_HD
#endif

namespace fastacore {

enum : uint8_t { LINE_RESIDUES = 0, LINE_HEADER = 1 };

// the kind of a line from its first bytes (n: the bytes of the line that are at hand, at least one for a non-empty line)
FA_HD inline uint8_t line_kind(const uint8_t *p, uint64_t n) { return n > 0 && p[0] == '>' ? LINE_HEADER : LINE_RESIDUES; }

// the bytes of [p, p + n) in front of the first blank: a piece of a header's name (p behind the '>'). blank: one was found.
FA_HD inline uint32_t name_span(const uint8_t *p, uint32_t n, bool &blank)
{
    uint32_t k = 0;
    while (k < n && p[k] != ' ') k++;
    blank = k < n;
    return k;
}

// bytes of the cut [pos_start, pos_end] of a contig of `length` bytes; `first`: the offset of its first byte in the contig
FA_HD inline uint32_t cut_len(uint32_t length, uint32_t pos_start, uint32_t pos_end, uint32_t &first)
{
    pos_start--;                                          // (uint32 wrap for 0: part of the contract)
    pos_end--;
    first = pos_start;
    if (pos_end >= length || pos_start > pos_end) return 0;
    return pos_end - pos_start + 1;
}

// the VCF writer's masking: IUPAC ambiguity codes in either case become N
FA_HD inline uint8_t mask_base(uint8_t c)
{
    switch (c | 0x20) {
    case 'r': case 'y': case 'k': case 'm': case 's': case 'w': case 'b': case 'd': case 'h': case 'v':
        return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') ? (uint8_t)'N' : c;
    default: return c;
    }
}

constexpr uint64_t kMaxContig = 1ull << 32;              // a contig of this many bytes or more is refused (the loader's uint32 length)

// ---- the records, from the header lines alone (host side). Fed with every header line in file order, in pieces where the text is: what
// crosses a cut of the text is `mid_line`, `kind`, the partial name and whether it is complete, and `open_rec`.
struct Record {
    std::string name;
    uint64_t start = 0, end = 0;                          // [start, end) of the kept bytes
};

struct Assembler {
    std::vector<Record> rec;
    int64_t open_rec = -1;                                // the record of the latest complete header line, if that was named: not stored yet
    uint64_t last_end = 0;                                // where the last stored record ends: the next one starts here
    bool mid_line = false;                                // the text so far ends inside a line (a non-empty one)
    uint8_t kind = LINE_RESIDUES;                         // ... of this kind
    bool name_done = false;                               // ... a header whose name has met its blank
    std::string name;                                     // ... and this much of its name

    // a header line begins with `kept` residue bytes in front of it
    void header_begin(uint64_t kept)
    {
        if (open_rec >= 0) { rec[(size_t)open_rec].end = kept; last_end = kept; open_rec = -1; }
        name.clear();
        name_done = false;
    }
    // the next bytes of the open header line behind its '>', up to their first blank
    void header_name(const uint8_t *p, uint32_t n, bool blank)
    {
        if (name_done) return;
        name.append((const char *)p, n);
        name_done = blank;
    }
    void header_end()
    {
        if (!name.empty()) { Record r; r.name = name; r.start = last_end; rec.push_back(r); open_rec = (int64_t)rec.size() - 1; }
        name.clear();
        name_done = false;
    }
    // the text has ended with `kept` residue bytes in all. Returns the bytes that belong to a record (what lies behind is dropped).
    uint64_t finish(uint64_t kept)
    {
        if (mid_line && kind == LINE_HEADER) header_end();
        mid_line = false;
        if (open_rec >= 0) { rec[(size_t)open_rec].end = kept; last_end = kept; open_rec = -1; }
        return last_end;
    }
    // index of the first record of kMaxContig bytes or more, or -1
    int64_t too_long() const
    {
        for (size_t i = 0; i < rec.size(); i++) if (rec[i].end - rec[i].start >= kMaxContig) return (int64_t)i;
        return -1;
    }
};

// What the device reports of one piece of the text (kernels/fasta.hip: a decision per line slot, sums, a scatter): the piece's header
// lines in file order — when the previous piece left a header line open, the first event is that line's continuation — and its last slot.
struct PieceEvents {
    uint32_t n_hdr = 0;
    const uint32_t *kept = nullptr;                       // [n_hdr] residue bytes of this piece in front of the line
    const uint32_t *name_off = nullptr, *name_len = nullptr;   // [n_hdr] the line's name bytes in names[]: up to the first blank or the slot's end
    const uint8_t *blank = nullptr;                       // [n_hdr] a blank ended them
    const uint8_t *names = nullptr;
    uint32_t tail_len = 0;                                // bytes of the piece's last line slot (0: the piece ends with a line end)
    uint8_t tail_kind = LINE_RESIDUES;
};

// The piece's events into the records, and what crosses the cut behind it. kept_before: the residue bytes in front of the piece.
inline void apply_piece(Assembler &a, uint64_t kept_before, const PieceEvents &e)
{
    const bool cont_hdr = a.mid_line && a.kind == LINE_HEADER;                 // the first event goes on with the open header line
    const bool tail_open = e.tail_len > 0;                                      // the piece ends inside a line
    for (uint32_t i = 0; i < e.n_hdr; i++) {
        if (!(i == 0 && cont_hdr)) a.header_begin(kept_before + e.kept[i]);
        a.header_name(e.names + e.name_off[i], e.name_len[i], e.blank[i] != 0);
        if (!(i + 1 == e.n_hdr && tail_open && e.tail_kind == LINE_HEADER)) a.header_end();
    }
    a.mid_line = tail_open;
    if (tail_open) a.kind = e.tail_kind;
}

#ifndef __HIPCC__
// The whole rule in one sequential pass over a piece of the text (the CPU check's side; the device decides the same per line, in
// parallel). `kept` counts the residue bytes so far; residues(p, n) takes the next ones.
template <class Sink>
inline void feed(Assembler &a, uint64_t &kept, const uint8_t *text, uint64_t len, Sink &&residues)
{
    uint64_t at = 0;
    while (at < len) {
        const uint8_t *nl = (const uint8_t *)memchr(text + at, '\n', (size_t)(len - at));
        const uint64_t eol = nl ? (uint64_t)(nl - text) : len, n = eol - at;
        uint8_t kind = a.kind;
        uint64_t from = at;
        if (!a.mid_line && n > 0) {                       // a line starts here
            kind = line_kind(text + at, n);
            if (kind == LINE_HEADER) { a.header_begin(kept); from = at + 1; }
        }
        if (a.mid_line || n > 0) {
            if (kind == LINE_HEADER) {
                uint64_t k = from;                        // (name_span with 64-bit lengths: a piece here may be the whole file)
                while (k < eol && text[k] != ' ') k++;
                if (!a.name_done) { a.name.append((const char *)text + from, (size_t)(k - from)); a.name_done = k < eol; }
            } else if (n > 0) {
                residues(text + at, n);
                kept += n;
            }
            if (nl) { if (kind == LINE_HEADER) a.header_end(); a.mid_line = false; }
            else { a.mid_line = true; a.kind = kind; }
        }
        at = nl ? eol + 1 : len;
    }
}
#endif

}  // namespace fastacore
