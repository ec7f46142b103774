"""Case lists, inputs, references and checkers for the device primitives under every kernel chain: the radix sort, the exclusive sum
(kernels/sort.hip) and the prefix maximum (kernels/depth.hip). No GPU here: tests/sort_primitives_check.py (a child process of
tests/test_gpu_sort_primitives.py, which cannot see pytest fixtures) runs these cases through the test build's hooks, and
tests/test_sort_primitives_inputs.py asserts that the lists still sit on the kernels' switch points and that the checkers reject
wrong answers.

References are plain numpy: a stable argsort of the keys under the mask of the digits the sort really walks, a uint64 cumulative sum
taken mod 2^32, np.maximum.accumulate."""
import numpy as np

# What the lists below were laid out for; tests/test_sort_primitives_inputs.py reads the same names out of the kernel sources.
WAVE = 64
RS_BITS = 8
RS_ROUNDS = 32
RS_WAVES = 4
OS_MAX_PASSES = 8
ES_TILE = 2048
ES_THREADS = 256
ES1_CHUNK = 16384
ES1_MAX = 65536
PM_TILE = 2048
PM_THREADS = 256
GUARD = 4096                      # CSVGPU_TEST_GUARD

U64 = np.uint64
FULL = 0xFFFFFFFFFFFFFFFF
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1

# ------------------------------------------------------------------------------------------------------------------ radix sort
# rs_rounds_for goes 2 -> 4 -> 8 -> 16 -> 32 rounds per wave tile once 128 tiles of the next size are full: n = 127 * rounds * 64 + 1
SORT_SWITCH_POINTS = [(32512, 32513), (65024, 65025), (130048, 130049), (260096, 260097)]
SORT_SMALL = [0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513]
# 300 001: a ragged last workgroup; 524 288 / 524 289: the (digit, tile) table of the three-launch passes crosses ES1_MAX entries
SORT_LARGE = [n for pair in SORT_SWITCH_POINTS for n in pair] + [300001, 524288, 524289]
SORT_KEY_BITS = [1, 8, 9, 16, 32, 33, 41, 64]
SORT_PATTERNS = ["all_equal", "two_values", "ascending", "descending", "uniform", "all_ff", "one_tile_digit", "bits_above"]
SORT_LARGE_KEY_BITS = [16, 41]
# all_equal: every tile in one status column, the longest look-back; uniform at 16 bits: long runs of ties over many tiles (stability),
# at 41 bits nearly distinct keys; one_tile_digit: 255 columns whose only counts are zeros but for one tile
SORT_LARGE_PATTERNS = ["all_equal", "uniform", "one_tile_digit"]
SORT_VALS = ["iota", "random"]
SORT_MODES = [1, 0]               # onesweep, three launches per pass
SORT_STATE_PAIR = (300001, 129)   # sorted back to back on one context

# the queued sort: count on the device, grid and workspace from the bound. 33 bits = 5 passes (the result ends in the other buffer
# pair), 41 bits = 6 passes (it ends where the input went in)
DEVN_N = [0, 1, 2, 129, 32513, 260097]
DEVN_BOUND_MAX = 600000
DEVN_KEY_BITS = [33, 41]
DEVN_PATTERNS = ["all_equal", "uniform"]
DEVN_REFUSED_BOUNDS = [1 << 30, (1 << 30) + 1, 1 << 32]


def devn_cases():
    out = []
    for n in DEVN_N:
        for nb in (n, n + 1, DEVN_BOUND_MAX):
            out.append((n, nb))
    out.append((DEVN_BOUND_MAX, DEVN_BOUND_MAX))
    return out


def sort_passes(key_bits):
    return (key_bits + RS_BITS - 1) // RS_BITS


def digit_mask(key_bits):
    """The bits the sort orders by: whole 8-bit digits, [0, 8 * ceil(key_bits / 8))."""
    bits = RS_BITS * sort_passes(key_bits)
    return U64(FULL if bits >= 64 else (1 << bits) - 1)


def key_mask(key_bits):
    return U64(FULL if key_bits >= 64 else (1 << key_bits) - 1)


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def make_keys(pattern, n, key_bits):
    """n uint64 keys. all_ff, one_tile_digit and bits_above set bits at and above key_bits on purpose; the others stay below 2^key_bits
    (ascending / descending wrap there when n is larger)."""
    rng = _rng(SORT_PATTERNS.index(pattern), n, key_bits)
    km, dm = key_mask(key_bits), digit_mask(key_bits)
    i = np.arange(n, dtype=U64)
    if pattern == "all_equal":
        return np.zeros(n, U64)
    if pattern == "two_values":
        two = np.array([0x0123456789ABCDEF, 0xFEDCBA9876543210], U64) & km
        return two[rng.integers(0, 2, n)]
    if pattern in ("ascending", "descending"):
        step = U64(max(1, int(km) // max(n, 1)))
        k = (i * step) & km
        return k if pattern == "ascending" else k[::-1].copy()
    if pattern == "uniform":
        return rng.integers(0, 1 << 64, n, dtype=U64) & km
    if pattern == "all_ff":
        return np.full(n, FULL, U64)
    if pattern == "one_tile_digit":
        # digit 0x37 of every pass only in 64 consecutive keys (one round of one wave tile: tiles are multiples of 128 keys), digit 0 elsewhere
        k = np.zeros(n, U64)
        a = (n // 2) // 64 * 64
        k[a:a + 64] = U64(0x3737373737373737) & dm
        return k
    if pattern == "bits_above":
        # four values below 2^key_bits (long runs of ties), random bits everywhere from key_bits up: those inside the last digit order
        # the keys, those above it must not, and all of them must come back attached to their keys
        low = rng.integers(0, 4, n, dtype=U64) & km
        high = rng.integers(0, 1 << 64, n, dtype=U64) & ~km
        return low | high
    raise ValueError(pattern)


def make_vals(kind, n):
    if kind == "iota":
        return np.arange(n, dtype=np.uint32)
    v = _rng(77, n).integers(0, 1 << 32, n, dtype=np.uint32)
    v[::7] = 0xFFFFFFFF
    return v


def sort_reference(keys, key_bits):
    """The stable permutation: result[j] = input[perm[j]]."""
    return np.argsort(keys & digit_mask(key_bits), kind="stable")


def small_sort_cases():
    return [(n, kb, p) for n in SORT_SMALL for kb in SORT_KEY_BITS for p in SORT_PATTERNS]


def large_sort_cases():
    return [(n, kb, p) for n in SORT_LARGE for kb in SORT_LARGE_KEY_BITS for p in SORT_LARGE_PATTERNS]


def _first_diff(want, got):
    if len(want) != len(got):
        return "length %d, expected %d" % (len(got), len(want))
    bad = np.flatnonzero(want != got)
    if len(bad) == 0:
        return None
    j = int(bad[0])
    return "first difference at index %d of %d (%d differ): expected %s, got %s" % (j, len(want), len(bad), hex(int(want[j])), hex(int(got[j])))


def check_sort(keys, vals, perm, keys_out, vals_out):
    """None, or what differs: the values must be the stable permutation's (with iota values, the permutation itself) and every key must
    arrive whole, bits above the sorted digits included."""
    d = _first_diff(vals[perm], vals_out)
    if d:
        return "vals_out: " + d
    d = _first_diff(keys[perm], keys_out)
    if d:
        return "keys_out: " + d
    return None


# ------------------------------------------------------------------------------------------------------------------ exclusive sum
ES_SIZES = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 16383, 16384, 16385, 65535, 65536, 65537, 67585, 524288, 524289, 526337]
# Indices at which an entry's predecessor is summed by another part of the code. One workgroup (n <= ES1_MAX): a thread's run of 16, a
# wave's 1024, a 16 Ki chunk (the carry word), the second and the last chunk. Three launches: a thread's 8, a wave's 512, a 2048-entry
# tile (the block table), the first tile that only the three-launch form sees, the spine's second loop of 256 tiles and its second tile.
ES_BOUNDARIES = [8, 16, 512, 1024, ES_TILE, ES1_CHUNK, 2 * ES1_CHUNK, 3 * ES1_CHUNK, ES1_MAX, ES1_MAX + ES_TILE, ES_THREADS * ES_TILE,
                 ES_THREADS * ES_TILE + ES_TILE]
ES_VALUES = ["ones", "below_2_16", "wrapping"]


def es_spikes(n):
    """Indices of the single 0xFFFFFFFF among zeros: c - 1 and c for every boundary c inside [1, n)."""
    return sorted({i for c in ES_BOUNDARIES for i in (c - 1, c) if c < n})


def make_es(kind, n, spike=None):
    if kind == "ones":
        return np.ones(n, np.uint32)
    if kind == "below_2_16":
        return _rng(5, n).integers(0, 1 << 16, n, dtype=np.uint32)
    if kind == "wrapping":                                   # every entry at least 2^30: sixteen of them pass 2^32 four times
        return _rng(6, n).integers(1 << 30, 1 << 32, n, dtype=np.uint32)
    if kind == "spike":
        d = np.zeros(n, np.uint32)
        d[spike] = 0xFFFFFFFF
        return d
    raise ValueError(kind)


def es_cases():
    out = [(n, kind, None) for n in ES_SIZES for kind in ES_VALUES]
    out += [(n, "spike", i) for n in ES_SIZES for i in es_spikes(n)]
    return out


def es_reference(data):
    c = np.cumsum(data.astype(np.uint64), dtype=np.uint64)
    out = np.zeros(len(data), np.uint64)
    out[1:] = c[:-1]
    return (out & U64(0xFFFFFFFF)).astype(np.uint32)


def check_exclusive_sum(data, got):
    return _first_diff(es_reference(data), got)


# ------------------------------------------------------------------------------------------------------------------ prefix maximum
PM_SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 524288, 524289, 526337]
PM_VALUES = ["int_min", "decreasing", "increasing", "negative", "spike_2047", "spike_2048", "spike_last"]


def make_pm(kind, n):
    if kind == "int_min":
        return np.full(n, INT32_MIN, np.int32)
    if kind == "decreasing":                                 # the maximum is element 0: the carry must survive every block and spine loop
        return (INT32_MAX - np.arange(n, dtype=np.int64)).astype(np.int32)
    if kind == "increasing":
        return (np.arange(n, dtype=np.int64) - n // 2).astype(np.int32)
    if kind == "negative":
        return _rng(8, n).integers(INT32_MIN, 0, n, dtype=np.int64).astype(np.int32)
    if kind.startswith("spike_"):
        d = _rng(9, n).integers(-1000, 1000, n, dtype=np.int64).astype(np.int32)
        i = n - 1 if kind == "spike_last" else int(kind[6:])
        if i < n:
            d[i] = INT32_MAX
        return d
    raise ValueError(kind)


def pm_cases():
    return [(n, kind) for n in PM_SIZES for kind in PM_VALUES]


def check_prefix_max(data, got):
    return _first_diff(np.maximum.accumulate(data), got)
