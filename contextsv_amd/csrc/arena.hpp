// arena.hpp — the bump allocator every device workspace is carved from, and its planning twin. No HIP calls: the CPU-only layout
// check (tools/fuzz/arena_layouts_check.cpp) includes it as it stands.
// The rule of this code base: a reservation is sized by running its carve. A layout is ONE function `bool carve(Arena &)` that takes its
// slices in order and fills a workspace struct; it runs first on arena_plan() — `used` afterwards is the need — and then on the real arena.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace csv {

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Arena {                     // grow-only bump allocator over one device buffer; reset per entry point
    char  *base = nullptr;
    size_t cap = 0, used = 0;
};

#ifdef CSV_ARENA_LOG               // set by the layout check alone: every slice handed out, for its overlap and bounds test
void arena_log(const Arena &a, void *p, size_t bytes);
#endif

// 256-B aligned slice, nullptr if exhausted
static inline void *arena_alloc(Arena &a, size_t bytes)
{
    const size_t off = align_up(a.used, 256);
    if (off + bytes > a.cap) return nullptr;
    a.used = off + bytes;
#ifdef CSV_ARENA_LOG
    arena_log(a, a.base + off, bytes);
#endif
    return a.base + off;
}

// arena_alloc into a typed pointer. Carve functions join these with `&&`: the slices are taken strictly in the order written.
template <class T> static inline bool take(Arena &a, T *&p, size_t bytes) { p = (T *)arena_alloc(a, bytes); return p != nullptr; }

// An arena with no memory behind it: slices are only counted and compared, never dereferenced.
static inline Arena arena_plan() { Arena a; a.base = (char *)(uintptr_t)256; a.cap = ~(size_t)0 >> 1; return a; }
// `tmp` (256-B aligned, sized by the plan of the same carve) as an arena: the kernels' launchers carve their temporaries from it
static inline Arena arena_view(void *tmp) { Arena a; a.base = (char *)tmp; a.cap = ~(size_t)0 >> 1; return a; }
template <class Carve> static inline size_t arena_plan_bytes(Carve &&carve) { Arena p = arena_plan(); (void)carve(p); return p.used; }

}  // namespace csv
