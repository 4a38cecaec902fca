"""Cases, references and checks for the shared device-wide scan and radix sort (csrc/radix.hip) behind the debug entries of
include/gof_hip.h: gof_debug_scan_u32, gof_debug_radix_sort, gof_debug_sort_keys63.  tests/test_primitives_host.py runs the groups of
GROUPS over the emulated library, tests/test_primitives_gpu.py over libgof_hip.so on the device; both hand in the library and a
"memory" (up / down / ptr / sync / stream), everything else is here.

References are numpy and every comparison is exact: np.cumsum in uint64 reduced mod 2^32; np.argsort(kind="stable") of the keys
masked to the WHOLE digits the sort takes, bits [0, 8 * ceil(end_bit / 8)); np.argsort(kind="stable") of the 63-bit keys.

Sizes are named by the constant they come from, read out of radix.hip itself (constants()), so a retuned constant moves its cases;
the host queries of the library are held against the same numbers (group "plan").  Every call runs on a workspace filled with 0xA5,
and every buffer it is handed -- the four key / value buffers, the scan's output, the workspace with its zero_words_behind words, the
count and the error word -- lies between canary words that must survive."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32
POISON, CANARY, GUARD = 0xA5A5A5A5, 0x5EED1E55, 16
GOF_E_INVALID = -1
SCAN, SORT, SORT63 = 0, 1, 2
SCRATCH_ZEROED, FIRST_HIST_DONE = 1, 2


def constants():
    src = open(os.path.join(ROOT, "gaussian-opacity-fields_amd", "csrc", "radix.hip")).read()

    def num(pattern):
        return int(re.search(pattern, src).group(1))
    return {"RS_CHUNK": num(r"#define\s+GOF_RS_CHUNK\s+(\d+)"), "OS_MAX_UNITS": num(r"#define\s+GOF_OS_MAX_UNITS\s+(\d+)"),
            "SCAN_ITEMS_SMALL": num(r"#define\s+GOF_SCAN_SMALL_ITEMS\s+(\d+)"), "SCAN_ITEMS_BIG": num(r"SCAN_ITEMS_BIG\s*=\s*(\d+)"),
            "SCAN_DIRECT_MAX": num(r"SCAN_DIRECT_MAX\s*=\s*(\d+)")}


K = constants()
STEP = 64                                        # items of one wave step of the sort
QUARTER = K["RS_CHUNK"]                          # items of a wave of a sort block
BLOCK = 4 * QUARTER                              # items of a sort block
OS_EDGE = K["OS_MAX_UNITS"] * BLOCK              # the largest sort that runs as single-kernel passes
SCAN_SMALL, SCAN_BIG = 256 * K["SCAN_ITEMS_SMALL"], 256 * K["SCAN_ITEMS_BIG"]       # words of a scan workgroup
SCAN_TILE_EDGE = K["SCAN_DIRECT_MAX"] * SCAN_SMALL       # the largest scan in small tiles
SCAN_DIRECT_EDGE = K["SCAN_DIRECT_MAX"] * SCAN_BIG       # the largest scan in two launches


def around(x):
    return [x - 1, x, x + 1]


SMALL_SIZES = sorted(set([0, 1] + around(STEP) + around(256) + around(QUARTER) + around(SCAN_SMALL) + around(BLOCK) + around(SCAN_BIG) + [3 * BLOCK + 1]))
END_BITS = (1, 7, 8, 9, 16, 17, 24, 31, 32)
SCAN_INPUTS = ("ones", "small", "wrap", "tile_first", "tile_last")
KEY_PATTERNS = ("random", "equal", "descending", "two_per_digit", "block_digit", "high_bits")


def passes_of(end_bit):
    return (end_bit + 7) // 8


def mask_of(end_bit):
    return (1 << (8 * passes_of(end_bit))) - 1


def rng_of(*what):
    return np.random.default_rng(list("/".join(str(w) for w in what).encode()))


# ---- scan ------------------------------------------------------------------------------------------------------------------------------
def scan_tile(n):
    return SCAN_SMALL if n <= SCAN_TILE_EDGE else SCAN_BIG


def scan_input(kind, n):
    r = rng_of("scan", kind, n)
    if kind == "ones":
        return np.ones(n, U32)                                   # out[i] names its own index
    if kind == "small":
        return r.integers(0, 8, n, dtype=np.uint64).astype(U32)
    if kind == "wrap":
        return r.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)      # the sum wraps 2^32 about n / 2 times
    x = np.zeros(n, U32)
    if n:
        t = scan_tile(n)
        j = ((n - 1) // t + 1) // 2                              # a tile in the middle (the only one of a short input)
        x[j * t if kind == "tile_first" else min(j * t + t - 1, n - 1)] = 0x80000001
    return x


def gather_index(kind, n):
    r = rng_of("gather", kind, n)
    if kind == "permutation":
        return r.permutation(n).astype(U32)
    return r.integers(0, max(n, 1), n, dtype=np.uint64).astype(U32) if n else np.zeros(0, U32)      # with repeats: legal


def scan_ref(x, idx, inclusive):
    g = x[idx] if idx is not None else x
    inc = (np.cumsum(g.astype(np.uint64), dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(U32)
    total = int(inc[-1]) if len(g) else 0
    return (inc if inclusive else np.concatenate([np.zeros(1, U32), inc[:-1]])[:len(g)]), total


# ---- sort ------------------------------------------------------------------------------------------------------------------------------
def sort_keys(pattern, n, end_bit):
    r = rng_of("keys", pattern, n, end_bit)
    p, mask = passes_of(end_bit), mask_of(end_bit)
    rnd = r.integers(0, 1 << 32, n, dtype=np.uint64)
    i = np.arange(n, dtype=np.uint64)
    if pattern == "random":
        k = rnd & np.uint64(mask)
    elif pattern == "equal":                                     # one digit value: the longest look-back chain
        k = np.full(n, 0x5A5A5A5A & mask, np.uint64)
    elif pattern == "descending":
        k = (np.uint64(max(n, 1) - 1) - i) & np.uint64(mask)
    elif pattern == "two_per_digit":
        k = np.zeros(n, np.uint64)
        for d in range(p):
            pair = r.integers(0, 256, 2, dtype=np.uint64)
            k |= pair[r.integers(0, 2, n)] << np.uint64(8 * d)
    elif pattern == "block_digit":                               # the first digit constant per block: every block's run is whole
        k = ((rnd & np.uint64(mask)) & ~np.uint64(0xFF)) | ((i // np.uint64(BLOCK)) * np.uint64(37) & np.uint64(0xFF))
    elif pattern == "high_bits":                                 # bits at and above 8 * passes: ignored, and moved with their key
        k = (rnd & np.uint64(mask & 0x0F0F0F0F)) | ((rnd >> np.uint64(3)) & np.uint64(~mask & 0xFFFFFFFF))
        if n and p < 4:
            k[0] |= np.uint64(1 << (8 * p))
            k[-1] |= np.uint64(1 << 31)
    else:
        raise KeyError(pattern)
    return k.astype(U32)


def sort_vals(kind, n):
    if kind == "index":                                          # the stability check
        return np.arange(n, dtype=U32)
    v = rng_of("vals", n).integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)       # moved, never interpreted
    v[::3] = 0xFFFFFFFF
    v[1::7] = 0
    return v


def sort_order(keys, end_bit):
    return np.argsort(keys & U32(mask_of(end_bit)), kind="stable")


def first_histogram(keys, m):
    """the first pass's [digit][block] counts in the layout radix_classic_hist documents: stride = the blocks that hold items"""
    nblk = max(1, -(-m // BLOCK))
    flat = (keys[:m] & U32(0xFF)).astype(np.int64) * nblk + np.arange(m, dtype=np.int64) // BLOCK
    return np.bincount(flat, minlength=256 * nblk).astype(U32)


def keys63(pattern, n):
    r = rng_of("keys63", pattern, n)
    lo = r.integers(0, 1 << 32, n, dtype=np.uint64)
    hi = r.integers(0, 1 << 31, n, dtype=np.uint64)
    few = lambda: r.integers(0, 5, n, dtype=np.uint64) * np.uint64(0x01010101)        # noqa: E731
    if pattern == "low":                                         # collide in the low word only
        lo = few()
    elif pattern == "high":                                      # collide in the high word only
        hi = few()
    elif pattern == "both":
        lo, hi = few(), few()
    elif pattern == "bit62":
        hi = few()
        hi[::2] |= np.uint64(1 << 30)
        lo = few()
    return (hi << np.uint64(32)) | lo


# ---- the library and its buffers -------------------------------------------------------------------------------------------------------
def bind(lib):
    p, z, i64, i = C.c_void_p, C.c_size_t, C.c_int64, C.c_int
    lib.gof_last_error.restype = C.c_char_p
    lib.gof_debug_prim_ws_bytes.restype = z
    lib.gof_debug_prim_ws_bytes.argtypes = [i, i64, z]
    lib.gof_debug_prim_constants.argtypes = [i64, i, p, p, p, p]
    lib.gof_debug_scan_plan.argtypes = [i64, p, p]
    lib.gof_debug_scan_u32.argtypes = [p, p, p, i64, i, p, z, p, p]
    lib.gof_debug_radix_sort.argtypes = [p, p, p, p, i64, i, p, z, i, p, z, p, p, p]
    lib.gof_debug_sort_keys63.argtypes = [p, i64, p, z, p, p]
    for f in ("gof_debug_prim_constants", "gof_debug_scan_plan", "gof_debug_scan_u32", "gof_debug_radix_sort", "gof_debug_sort_keys63"):
        getattr(lib, f).restype = i
    return lib


class HostMem:
    """the memory of the emulated library: numpy arrays"""
    stream = None

    def up(self, a):
        return np.array(a, dtype=U32, copy=True)

    def down(self, h):
        return h.copy()

    def ptr(self, h, word):
        return h.ctypes.data + 4 * word

    def sync(self):
        pass


class Buf:
    """`payload` (u32 words) between two runs of GUARD canary words, in the memory of the library"""
    def __init__(self, mem, payload, name):
        payload = np.ascontiguousarray(payload, U32)
        guard = np.full(GUARD, CANARY, U32)
        self.mem, self.n, self.name = mem, len(payload), name
        self.h = mem.up(np.concatenate([guard, payload, guard]))
        self.ptr = mem.ptr(self.h, GUARD)

    def read(self):
        a = self.mem.down(self.h)
        assert (a[:GUARD] == CANARY).all(), "canary in front of %s overwritten" % self.name
        assert (a[GUARD + self.n:] == CANARY).all(), "canary behind %s overwritten" % self.name
        return a[GUARD:GUARD + self.n]


def poison(n):
    return np.full(n, POISON, U32)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s items, expected %s" % (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: got %s, expected %s" % (what, len(bad), len(got), bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())


def sort_facts(lib, n, end_bit):
    blk, ps, zw, ch = C.c_uint32(), C.c_int32(), C.c_size_t(), C.c_int32()
    assert lib.gof_debug_prim_constants(n, end_bit, C.addressof(blk), C.addressof(ps), C.addressof(zw), C.addressof(ch)) == 0
    return blk.value, ps.value, zw.value, ch.value


def scan_plan(lib, n):
    t, l = C.c_uint32(), C.c_int32()
    assert lib.gof_debug_scan_plan(n, C.addressof(t), C.addressof(l)) == 0
    return t.value, l.value


def run_scan(lib, mem, x, idx, inclusive, in_place, what):
    n = len(idx) if idx is not None else len(x)
    assert not (in_place and idx is not None)
    want, total = scan_ref(x, idx, inclusive)
    xin = Buf(mem, x, "in")
    ix = Buf(mem, idx, "idx") if idx is not None else None
    out = xin if in_place else Buf(mem, poison(n), "out")
    words = lib.gof_debug_prim_ws_bytes(SCAN, n, 0) // 4
    ws = Buf(mem, poison(words), "the workspace")
    tot = Buf(mem, poison(1), "total")
    rc = lib.gof_debug_scan_u32(xin.ptr, ix.ptr if ix else None, out.ptr, n, int(inclusive), ws.ptr, 4 * words, tot.ptr, mem.stream)
    mem.sync()
    assert rc == 0, (what, rc, lib.gof_last_error())
    same(out.read(), want, what)
    same(tot.read(), [total], what + ": grand total")
    ws.read()
    if not in_place:
        same(xin.read(), x, what + ": input left alone")
    if ix:
        same(ix.read(), idx, what + ": index left alone")


def run_sort(lib, mem, keys, vals, end_bit, what, count=None, zero_behind=0, scratch_zeroed=False, hist=None):
    """-> the number of passes.  count: the item count on the device, len(keys) is then the capacity"""
    n = len(keys)
    _, passes, zero_words, classic = sort_facts(lib, n, end_bit)
    assert passes == passes_of(end_bit)
    tmp_words = lib.gof_debug_prim_ws_bytes(SORT, n, 0) // 4
    words = lib.gof_debug_prim_ws_bytes(SORT, n, zero_behind) // 4
    assert words == tmp_words + zero_behind
    w, flags = poison(words), 0
    if scratch_zeroed:
        assert zero_words > 0 and not classic, "scratch_zeroed is the contract of the single-kernel passes"
        w[:zero_words] = 0
        flags |= SCRATCH_ZEROED
    if hist is not None:
        assert classic and len(hist) <= tmp_words, "first_hist_done is the contract of the histogram / scan / scatter launches"
        w[:len(hist)] = hist
        flags |= FIRST_HIST_DONE
    ws = Buf(mem, w, "the workspace and its zero_words_behind")
    ka, va, kb, vb = Buf(mem, keys, "keys_a"), Buf(mem, vals, "vals_a"), Buf(mem, poison(n), "keys_b"), Buf(mem, poison(n), "vals_b")
    nd = Buf(mem, [count], "n_dev") if count is not None else None
    err = Buf(mem, poison(1), "err_flag_out")
    in_b = C.c_int32(-1)
    rc = lib.gof_debug_radix_sort(ka.ptr, va.ptr, kb.ptr, vb.ptr, n, end_bit, nd.ptr if nd else None, zero_behind, flags, ws.ptr, 4 * words,
                                  C.addressof(in_b), err.ptr, mem.stream)
    mem.sync()
    assert rc == 0, (what, rc, lib.gof_last_error())
    assert in_b.value == (passes % 2 if n > 0 else 0), "%s: result_in_b_out %d after %d passes" % (what, in_b.value, passes)
    got = [b.read() for b in (ka, va, kb, vb)]
    m = n if count is None else min(count, n)
    order = sort_order(keys[:m], end_bit)
    same(got[2 * in_b.value][:m], keys[:m][order], what + ": keys")
    same(got[2 * in_b.value + 1][:m], vals[:m][order], what + ": values")
    same(ws.read()[tmp_words:], np.zeros(zero_behind, U32), what + ": zero_words_behind")
    same(err.read(), [0], what + ": error word")
    if nd:
        same(nd.read(), [count], what + ": count left alone")
    return passes


def run_sort63(lib, mem, keys, what):
    n = len(keys)
    nbytes = lib.gof_debug_prim_ws_bytes(SORT63, n, 0)
    assert nbytes % 4 == 0
    ws = Buf(mem, poison(nbytes // 4), "the workspace")
    kb = Buf(mem, np.ascontiguousarray(keys, np.uint64).view(U32), "keys")
    out = Buf(mem, poison(n), "order_out")
    rc = lib.gof_debug_sort_keys63(kb.ptr, n, ws.ptr, nbytes, out.ptr, mem.stream)
    mem.sync()
    assert rc == 0, (what, rc, lib.gof_last_error())
    same(out.read(), np.argsort(keys, kind="stable").astype(U32), what)
    same(kb.read().view(np.uint64), keys, what + ": keys left alone")
    ws.read()


# ---- groups: name -> f(lib, mem) -> number of calls checked; HOST_GROUPS also run over the emulated library ----------------------------
def g_plan(lib, mem):
    """the host queries against the constants of the source: block size, passes, the regime edges of sort and scan"""
    for e in range(1, 33):
        assert sort_facts(lib, 1, e)[:2] == (BLOCK, passes_of(e))
    for e in (8, 32):
        for n, os_regime in ((0, None), (1, True), (OS_EDGE, True), (OS_EDGE + 1, False)):
            _, ps, zw, ch = sort_facts(lib, n, e)
            units = -(-n // BLOCK)
            if os_regime is None:
                assert (zw, ch) == (0, 0)
            elif os_regime:
                assert ch == 0 and zw > ps * 256 * units and 4 * zw <= lib.gof_debug_prim_ws_bytes(SORT, n, 0)     # a descriptor per (pass, block, digit) and the header
            else:
                assert ch == 1 and zw == 0
    # zero_words_behind is folded into the one memset exactly where the cleared words end at the scratch's end: four passes
    assert 4 * sort_facts(lib, BLOCK + 1, 32)[2] == lib.gof_debug_prim_ws_bytes(SORT, BLOCK + 1, 0)
    assert 4 * sort_facts(lib, BLOCK + 1, 24)[2] < lib.gof_debug_prim_ws_bytes(SORT, BLOCK + 1, 0)
    assert lib.gof_debug_prim_ws_bytes(SORT, 100, 7) == lib.gof_debug_prim_ws_bytes(SORT, 100, 0) + 28
    for n, want in ((0, (SCAN_SMALL, 0)), (1, (SCAN_SMALL, 2)), (SCAN_TILE_EDGE, (SCAN_SMALL, 2)), (SCAN_TILE_EDGE + 1, (SCAN_BIG, 2)),
                    (SCAN_DIRECT_EDGE, (SCAN_BIG, 2)), (SCAN_DIRECT_EDGE + 1, (SCAN_BIG, 3))):
        assert scan_plan(lib, n) == want, (n, scan_plan(lib, n), want)
        assert lib.gof_debug_prim_ws_bytes(SCAN, n, 0) >= 4 * (-(-n // want[0]) + 2)          # every block sum, the grand total
    return 1


def _scan_out_of_place(sizes):
    def f(lib, mem):
        c = 0
        for n in sizes:
            for kind in SCAN_INPUTS:
                for inc in (False, True):
                    run_scan(lib, mem, scan_input(kind, n), None, inc, False, "scan n=%d %s inclusive=%d" % (n, kind, inc))
                    c += 1
        return c
    return f


def _scan_in_place_and_gather(sizes):
    def f(lib, mem):
        c = 0
        for n in sizes:
            for inc in (False, True):
                for kind in ("ones", "wrap"):
                    run_scan(lib, mem, scan_input(kind, n), None, inc, True, "scan in place n=%d %s inclusive=%d" % (n, kind, inc))
                for g in ("permutation", "repeats"):
                    run_scan(lib, mem, scan_input("wrap", n), gather_index(g, n), inc, False, "scan gather n=%d %s inclusive=%d" % (n, g, inc))
                c += 4
        return c
    return f


def _scan_big(sizes):
    """a few calls per size: each form once, between them every input kind, both variants, in place and gathered"""
    def f(lib, mem):
        c = 0
        for n in sizes:
            run_scan(lib, mem, scan_input("ones", n), None, False, True, "scan in place n=%d ones exclusive" % n)
            run_scan(lib, mem, scan_input("wrap", n), None, True, False, "scan n=%d wrap inclusive" % n)
            run_scan(lib, mem, scan_input("tile_last", n), gather_index("repeats", n), True, False, "scan gather n=%d repeats inclusive" % n)
            c += 3
        return c
    return f


def _scan_big_rest(sizes):
    def f(lib, mem):
        c = 0
        for n in sizes:
            run_scan(lib, mem, scan_input("small", n), gather_index("permutation", n), False, False, "scan gather n=%d permutation exclusive" % n)
            run_scan(lib, mem, scan_input("tile_first", n), None, False, False, "scan n=%d tile_first exclusive" % n)
            run_scan(lib, mem, scan_input("tile_last", n), None, True, True, "scan in place n=%d tile_last inclusive" % n)
            c += 3
        return c
    return f


def _sort_sizes(sizes, end_bits=(8, 32)):
    def f(lib, mem):
        c = 0
        for n in sizes:
            for e in end_bits:
                run_sort(lib, mem, sort_keys("random", n, e), sort_vals("index", n), e, "sort n=%d end_bit=%d random" % (n, e))
                c += 1
        return c
    return f


def _sort_end_bits(sizes, variants=(("high_bits", "index"), ("random", "patterns")), end_bits=END_BITS):
    def f(lib, mem):
        seen = set()
        for n in sizes:
            for e in end_bits:
                for pattern, vals in variants:
                    seen.add(run_sort(lib, mem, sort_keys(pattern, n, e), sort_vals(vals, n), e, "sort n=%d end_bit=%d %s, values: %s" % (n, e, pattern, vals)))
        assert seen == {1, 2, 3, 4}                  # both parities of the result buffer
        return len(variants) * len(sizes) * len(end_bits)
    return f


def _sort_patterns(sizes, end_bits=(8, 16, 32)):
    def f(lib, mem):
        c = 0
        for n in sizes:
            for e in end_bits:
                for pattern in KEY_PATTERNS[1:]:
                    run_sort(lib, mem, sort_keys(pattern, n, e), sort_vals("index", n), e, "sort n=%d end_bit=%d %s" % (n, e, pattern))
                    c += 1
        return c
    return f


def _sort_n_dev(capacities, counts_of, end_bits=(16, 24)):
    def f(lib, mem):
        c = 0
        for cap in capacities:
            for e in end_bits:
                keys, vals = sort_keys("two_per_digit", cap, e), sort_vals("index", cap)
                for count in counts_of(cap):
                    run_sort(lib, mem, keys, vals, e, "sort capacity=%d count=%d end_bit=%d" % (cap, count, e), count=count)
                    c += 1
        return c
    return f


def _small_counts(cap):
    return sorted(set(k for k in [0, 1, cap - 1, cap] + around(STEP) + around(QUARTER) + around(BLOCK) + [2 * BLOCK] if 0 <= k <= cap))


def _sort_zero_words(sizes):
    """zero_words_behind: folded into the one memset (four passes), a memset of its own (fewer), the launches regime and n == 0 by size"""
    def f(lib, mem):
        c = 0
        for n in sizes:
            for e in (32, 16):
                for count in (None, 1):
                    run_sort(lib, mem, sort_keys("random", n, e), sort_vals("index", n), e, "sort n=%d end_bit=%d count=%s, 37 words behind" % (n, e, count),
                             count=count, zero_behind=37)
                    c += 1
        return c
    return f


def _sort_scratch_zeroed(sizes):
    def f(lib, mem):
        c = 0
        for n in sizes:
            for e in (8, 16, 24, 32):
                run_sort(lib, mem, sort_keys("two_per_digit", n, e), sort_vals("index", n), e, "sort n=%d end_bit=%d scratch_zeroed" % (n, e), scratch_zeroed=True)
                c += 1
        return c
    return f


def g_sort_first_hist(lib, mem):
    """first_hist_done: the first pass's histogram comes from numpy, the result is that of the plain call (the reference)"""
    n, c = OS_EDGE + 1, 0
    for e, count in ((8, None), (24, None), (16, OS_EDGE - BLOCK + 1), (16, 5)):
        keys = sort_keys("random", n, e)
        m = n if count is None else count
        run_sort(lib, mem, keys, sort_vals("index", n), e, "sort n=%d end_bit=%d count=%s first_hist_done" % (n, e, count), count=count,
                 hist=first_histogram(keys, m))
        c += 1
    return c


def _sort63(sizes):
    def f(lib, mem):
        c = 0
        for n in sizes:
            for pattern in ("low", "high", "both", "bit62"):
                run_sort63(lib, mem, keys63(pattern, n), "sort_keys63 n=%d %s" % (n, pattern))
                c += 1
        return c
    return f


def g_arguments(lib, mem):
    """GOF_E_INVALID with a message, and nothing written, for a NULL buffer with n > 0, end_bit outside 1..32, a workspace too small"""
    n = 100
    bufs = [Buf(mem, poison(n), "buffer %d" % k) for k in range(5)]
    ws = Buf(mem, poison(lib.gof_debug_prim_ws_bytes(SORT63, n, 0) // 4), "the workspace")
    a, b, c, d, e = (x.ptr for x in bufs)
    res = C.c_int32(-7)
    r = C.addressof(res)
    big = 4 * ws.n
    need = lambda kind: lib.gof_debug_prim_ws_bytes(kind, n, 0)        # noqa: E731
    calls = {
        "scan in NULL": lambda: lib.gof_debug_scan_u32(None, None, b, n, 0, ws.ptr, big, e, mem.stream),
        "scan out NULL": lambda: lib.gof_debug_scan_u32(a, None, None, n, 0, ws.ptr, big, e, mem.stream),
        "scan ws NULL": lambda: lib.gof_debug_scan_u32(a, None, b, n, 0, None, big, e, mem.stream),
        "scan ws small": lambda: lib.gof_debug_scan_u32(a, None, b, n, 0, ws.ptr, need(SCAN) - 1, e, mem.stream),
        "scan n < 0": lambda: lib.gof_debug_scan_u32(a, None, b, -1, 0, ws.ptr, big, e, mem.stream),
        "sort keys_a NULL": lambda: lib.gof_debug_radix_sort(None, b, c, d, n, 8, None, 0, 0, ws.ptr, big, r, e, mem.stream),
        "sort vals_b NULL": lambda: lib.gof_debug_radix_sort(a, b, c, None, n, 8, None, 0, 0, ws.ptr, big, r, e, mem.stream),
        "sort end_bit 0": lambda: lib.gof_debug_radix_sort(a, b, c, d, n, 0, None, 0, 0, ws.ptr, big, r, e, mem.stream),
        "sort end_bit 33": lambda: lib.gof_debug_radix_sort(a, b, c, d, n, 33, None, 0, 0, ws.ptr, big, r, e, mem.stream),
        "sort flags 4": lambda: lib.gof_debug_radix_sort(a, b, c, d, n, 8, None, 0, 4, ws.ptr, big, r, e, mem.stream),
        "sort ws small": lambda: lib.gof_debug_radix_sort(a, b, c, d, n, 8, None, 0, 0, ws.ptr, need(SORT) - 1, r, e, mem.stream),
        "sort ws small for the words behind": lambda: lib.gof_debug_radix_sort(a, b, c, d, n, 8, None, 9, 0, ws.ptr, need(SORT) + 32, r, e, mem.stream),
        "sort result NULL": lambda: lib.gof_debug_radix_sort(a, b, c, d, n, 8, None, 0, 0, ws.ptr, big, None, e, mem.stream),
        "sort63 keys NULL": lambda: lib.gof_debug_sort_keys63(None, n // 2, ws.ptr, big, b, mem.stream),
        "sort63 ws small": lambda: lib.gof_debug_sort_keys63(a, n // 2, ws.ptr, lib.gof_debug_prim_ws_bytes(SORT63, n // 2, 0) - 1, b, mem.stream),
        "constants end_bit 0": lambda: lib.gof_debug_prim_constants(n, 0, None, None, None, None),
        "plan n < 0": lambda: lib.gof_debug_scan_plan(-1, None, None),
    }
    for name, f in calls.items():
        rc = f()
        assert rc == GOF_E_INVALID and lib.gof_last_error(), (name, rc)
    mem.sync()
    for x in bufs + [ws]:
        same(x.read(), poison(x.n), "a refused call wrote " + x.name)
    assert res.value == -7
    assert lib.gof_debug_prim_ws_bytes(3, n, 0) == 0 and lib.gof_debug_prim_ws_bytes(SCAN, -1, 0) == 0
    return len(calls)


HOST_GROUPS = {
    "plan": g_plan,
    "arguments": g_arguments,
    "scan_out_of_place": _scan_out_of_place(SMALL_SIZES),
    "scan_in_place_and_gather": _scan_in_place_and_gather(SMALL_SIZES),
    "sort_sizes": _sort_sizes(SMALL_SIZES),
    "sort_end_bits": _sort_end_bits([BLOCK + 1]),
    "sort_patterns": _sort_patterns([BLOCK + 1, 3 * BLOCK + 1]),
    "sort_n_dev": _sort_n_dev([3 * BLOCK + 1], _small_counts),
    "sort_zero_words_behind": _sort_zero_words([0, 1, 3 * BLOCK + 1]),
    "sort_scratch_zeroed": _sort_scratch_zeroed([1, BLOCK + 1, 3 * BLOCK + 1]),
    "sort_keys63": _sort63([0, 1, BLOCK + 1]),
}
# the regimes that exist from 2 M / 8 M words on.  On the device all of them; the emulator takes the three that cost it 2-3 s each
# (HOST_EDGE_GROUPS: the sort's histogram / scan / scatter launches at their smallest, one pass, and each form of the scan once),
# the others 7-28 s each.
GPU_GROUPS = dict(HOST_GROUPS, **{
    "sort_launches_regime": _sort_sizes([OS_EDGE + 1], end_bits=(8,)),
    "scan_tile_edge": _scan_big(around(SCAN_TILE_EDGE)),
    "scan_tile_edge_rest": _scan_big_rest(around(SCAN_TILE_EDGE)),
    "scan_direct_edge": _scan_big([SCAN_DIRECT_EDGE, SCAN_DIRECT_EDGE + 1]),
    "scan_direct_edge_rest": _scan_big_rest([SCAN_DIRECT_EDGE, SCAN_DIRECT_EDGE + 1]),
    "sort_regime_edge": _sort_sizes(around(OS_EDGE)),
    "sort_regime_edge_end_bits": _sort_end_bits([OS_EDGE + 1], variants=(("high_bits", "index"),)),
    "sort_regime_edge_values": _sort_end_bits([OS_EDGE, OS_EDGE + 1], variants=(("random", "patterns"),), end_bits=(8, 16, 24, 32)),
    "sort_regime_edge_patterns": _sort_patterns([OS_EDGE, OS_EDGE + 1], end_bits=(16,)),
    "sort_regime_edge_n_dev": _sort_n_dev([OS_EDGE, OS_EDGE + 1], lambda cap: [0, 1, 5, BLOCK, BLOCK + 1, cap - 1, cap], end_bits=(16,)),
    "sort_regime_edge_zero_words_behind": _sort_zero_words([OS_EDGE + 1]),
    "sort_regime_edge_scratch_zeroed": _sort_scratch_zeroed([OS_EDGE]),
    "sort_first_hist_done": g_sort_first_hist,
    "sort_keys63_regime_edge": _sort63([OS_EDGE + 1]),
})
HOST_EDGE_GROUPS = ("sort_launches_regime", "scan_tile_edge", "scan_direct_edge")
