// png_encode.hip -- the PNG encoder on HIP (C ABI in include/gof_png_hip.h).
//
// render.py:31-36 renders a view in a few milliseconds and then saves two images through torchvision.utils.save_image: a blocking copy
// to the host and Pillow's encoder (zlib level 6) on one CPU thread.  Here the whole data-parallel part runs on the device, float planes
// in, finished zlib stream out; the host frames the chunks and writes the file.  Three kernels and the shared scan (radix.hip):
//
//   quantise_filter  one workgroup per image row.  The row and the row above it are quantised from the float planes into LDS in chunks
//                    of 1024 pixels (so rows are independent of each other and of any width), the five PNG filters are formed per
//                    byte, their sums of |signed byte| reduced with integer LDS atomics (any order gives the same sum), the smallest
//                    sum (lowest number on a tie) chosen, and a second sweep over the chunks writes the scanline.
//   deflate_blocks   one workgroup per GOF_PNG_BLOCK_BYTES of the scanline stream; thread t owns 64 consecutive bytes.  The block is
//                    staged in LDS (padded: the lanes' 64-byte strides fall on different banks).  Runs are found with two wave-level
//                    scans (the last run start in front of a thread's bytes, the first one behind them); a run of R repeated bytes
//                    behind its first byte becomes matches of 258 and a rest of >= 3, or literals -- greedy, as zlib's Z_RLE.  The
//                    threads walk their bytes three times: histogram (integer LDS atomics), bit lengths (exclusive scan over the
//                    threads), packing (each thread ORs its tokens into the LDS image of the block at its bit offset).  Between the
//                    first two walks the workgroup builds the optimal length-limited code by package-merge: the symbols are ranked by
//                    (frequency, symbol), and per level every leaf and every package finds its place in the merged list by binary
//                    search, so a level is one parallel step.  Thread 0 writes the block header while the others measure their tokens.
//                    A block whose dynamic form would be longer than 5 + n bytes is written stored.  Per block: its bytes in a slot
//                    of the workspace, its size, and the two Adler-32 sums of its input.
//   compact          after an exclusive scan of the sizes: every block's bytes go to their place in the stream; workgroup 0 also
//                    combines the Adler-32 sums in block order and writes the zlib header, the trailer and the length.
// Every sum is an integer sum and every tie is broken by an index: the bytes do not depend on the schedule.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/gof_hip.h"
#include "../../include/gof_png_hip.h"
#include "gof_common.h"
#include "radix.h"
#include "png_common.h"

namespace gof {
namespace png {
using namespace pngc;

constexpr int THREADS = 256;
constexpr int BLOCK = GOF_PNG_BLOCK_BYTES;
constexpr int SEG = BLOCK / THREADS;            // bytes of a block one thread owns
constexpr int SLOT = BLOCK + 16;                // bytes of a block's slot in the workspace (a stored block: BLOCK + 5), a multiple of 16
constexpr int OUT_WORDS = SLOT / 4;
constexpr int NLIT_WRITTEN = 286;               // literal / length symbols a block may use (the decoder reads 288 lengths: the fixed code's)
constexpr int CH = 1024;                        // pixels of a row quantise_filter stages at a time
static_assert(BLOCK % THREADS == 0 && SEG == 64 && SLOT % 16 == 0, "deflate_blocks: one thread owns 64 bytes");
static_assert(BLOCK <= ADLER_STEP, "deflate_blocks: a block is one Adler-32 step");

// (uint8)clamp(x * 255 + 0.5, 0, 255) with the product and the sum rounded separately; NaN fails the first comparison: 0
__device__ __forceinline__ uint32_t quantise(float x)
{
#pragma clang fp contract(off)
    float v = x * 255.0f;
    v = v + 0.5f;
    return v >= 0.0f ? (v > 255.0f ? 255u : (uint32_t)v) : 0u;
}

__device__ __forceinline__ uint32_t abs_signed(uint32_t b) { return b < 128u ? b : 256u - b; }

// raw: [H][1 + 3 W]
__global__ void __launch_bounds__(THREADS)
quantise_filter(const float* __restrict__ planes, int64_t pstride, int C, int W, uint8_t* __restrict__ raw)
{
    __shared__ uint8_t s_cur[3 * (CH + 1)], s_up[3 * (CH + 1)];         // pixel p of the chunk at 3 (p + 1): the pixel to the left of the chunk first
    __shared__ uint32_t s_sum[5];
    __shared__ uint32_t s_best;
    const int tid = threadIdx.x;
    const int y = blockIdx.x;
    const size_t rowbytes = 3 * (size_t)W + 1;
    uint8_t* out = raw + (size_t)y * rowbytes;
    if (tid < 5) s_sum[tid] = 0u;
    uint32_t sum[5] = { 0u, 0u, 0u, 0u, 0u };
    uint32_t best = 0;
    for (int pass = 0; pass < 2; pass++) {
        for (int x0 = 0; x0 < W; x0 += CH) {
            const int npix = min(CH, W - x0);
            __syncthreads();
            for (int p = tid; p < npix + 1; p += THREADS) {
                const int x = x0 + p - 1;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    uint32_t cur = 0u, up = 0u;
                    if (x >= 0) {
                        const float* pl = planes + (C == 1 ? 0 : c) * pstride + (int64_t)y * W + x;
                        cur = quantise(pl[0]);
                        if (y > 0) up = quantise(pl[-W]);
                    }
                    s_cur[3 * p + c] = (uint8_t)cur;
                    s_up[3 * p + c] = (uint8_t)up;
                }
            }
            __syncthreads();
            for (int j = tid; j < 3 * npix; j += THREADS) {
                const int cur = s_cur[3 + j], a = s_cur[j], b = s_up[3 + j], c = s_up[j];
                const uint32_t f[5] = { (uint32_t)cur, (uint32_t)(cur - a) & 255u, (uint32_t)(cur - b) & 255u, (uint32_t)(cur - ((a + b) >> 1)) & 255u,
                                        (uint32_t)(cur - paeth(a, b, c)) & 255u };
                if (pass == 0) {
#pragma unroll
                    for (int k = 0; k < 5; k++) sum[k] += abs_signed(f[k]);
                } else {
                    out[1 + 3 * (size_t)x0 + j] = (uint8_t)(best == 0 ? f[0] : best == 1 ? f[1] : best == 2 ? f[2] : best == 3 ? f[3] : f[4]);
                }
            }
        }
        if (pass == 0) {
#pragma unroll
            for (int k = 0; k < 5; k++) atomicAdd(&s_sum[k], sum[k]);
            __syncthreads();
            if (tid == 0) {
                uint32_t bk = 0;
                for (uint32_t k = 1; k < 5; k++) if (s_sum[k] < s_sum[bk]) bk = k;
                s_best = bk;
                out[0] = (uint8_t)bk;
            }
            __syncthreads();
            best = s_best;
        }
    }
}

// ---- scans over the 256 threads of a workgroup: shuffles inside a wave, the four wave totals through LDS ------------------------------
struct OpAdd { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct OpMax { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct OpMin { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };

// EXCLUSIVE scan of v over the threads in front of this one (REVERSE: behind it); *total = over all threads.  Called by all threads.
template <bool REVERSE, class Op>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, Op op, uint32_t ident, uint32_t* total, uint32_t* s_wave /*[4]*/)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = REVERSE ? __shfl_down(inc, d, 64) : __shfl_up(inc, d, 64);
        if (REVERSE ? lane + d < 64u : lane >= d) inc = op(o, inc);
    }
    if (lane == (REVERSE ? 0u : 63u)) s_wave[wave] = inc;
    uint32_t ex = REVERSE ? __shfl_down(inc, 1, 64) : __shfl_up(inc, 1, 64);
    if (lane == (REVERSE ? 63u : 0u)) ex = ident;
    __syncthreads();
    uint32_t pre = ident, tot = ident;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
        const uint32_t s = s_wave[w];
        if (REVERSE ? w > wave : w < wave) pre = op(pre, s);
        tot = op(tot, s);
    }
    __syncthreads();
    *total = tot;
    return op(pre, ex);
}

// ---- optimal length-limited prefix code (package-merge), by the whole workgroup ---------------------------------------------------
struct TreeScratch {
    uint32_t w[NLIT_WRITTEN];                           // the used symbols' frequencies, ascending by (frequency, symbol)
    uint16_t sym[NLIT_WRITTEN];
    uint32_t list[2][2 * NLIT_WRITTEN + 4];             // the merged list of a level and of the level below it
    uint16_t pos[MAXBITS][NLIT_WRITTEN];                // where leaf i stands in the merged list of a level
    uint32_t n;
    uint32_t count[MAXBITS + 1];                // symbols per code length
};

// freq[nsym] -> len[nsym] (0 for an unused symbol), code[nsym] (canonical, bit-reversed: ready to be written from the low bit).
// The code minimises sum freq * len among all prefix codes with len <= L (2^L >= the number of used symbols); one used symbol gets
// one bit.  Ties are broken by the symbol number.
__device__ void build_code(const uint32_t* freq, int nsym, int L, uint8_t* len, uint16_t* code, TreeScratch& S)
{
    const int tid = threadIdx.x;
    if (tid == 0) S.n = 0u;
    if (tid <= MAXBITS) S.count[tid] = 0u;
    __syncthreads();
    for (int a = tid; a < nsym; a += THREADS) {
        const uint32_t f = freq[a];
        len[a] = 0;
        if (f) {
            int rank = 0;
            for (int b = 0; b < nsym; b++) {
                const uint32_t fb = freq[b];
                rank += (fb && (fb < f || (fb == f && b < a))) ? 1 : 0;
            }
            S.w[rank] = f;
            S.sym[rank] = (uint16_t)a;
            atomicAdd(&S.n, 1u);
        }
    }
    __syncthreads();
    const int n = (int)S.n;
    if (n == 1) {
        if (tid == 0) { len[S.sym[0]] = 1; S.count[1] = 1u; }
    } else if (n > 1) {
        int plen[MAXBITS + 1];                  // length of the merged list of level d (1 = the top)
        int prev_len = 0, cur = 0;
        for (int d = L; d >= 1; d--) {
            const uint32_t* prev = S.list[cur ^ 1];
            uint32_t* lst = S.list[cur];
            const int np = prev_len >> 1;       // packages: pairs of the level below
            for (int i = tid; i < n; i += THREADS) {
                const uint32_t wi = S.w[i];
                int lo = 0, hi = np;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (prev[2 * mid] + prev[2 * mid + 1] < wi) lo = mid + 1; else hi = mid; }
                lst[i + lo] = wi;               // a leaf stands in front of a package of its weight
                S.pos[d - 1][i] = (uint16_t)(i + lo);
            }
            for (int j = tid; j < np; j += THREADS) {
                const uint32_t pw = prev[2 * j] + prev[2 * j + 1];
                int lo = 0, hi = n;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (S.w[mid] <= pw) lo = mid + 1; else hi = mid; }
                lst[j + lo] = pw;
            }
            __syncthreads();
            prev_len = n + np;
            plen[d] = prev_len;
            cur ^= 1;
        }
        // the first 2n - 2 items of the top list; a chosen package chooses two items of the level below.  c[d] = leaves chosen at level d
        // (a prefix of the sorted leaves): leaf i has one bit per level that chose it.
        int c[MAXBITS + 1];
        int k = 2 * n - 2;
        for (int d = 1; d <= L; d++) {
            if (k > plen[d]) k = plen[d];
            int lo = 0, hi = n;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int)S.pos[d - 1][mid] < k) lo = mid + 1; else hi = mid; }
            c[d] = lo;
            k = 2 * (k - lo);
        }
        for (int i = tid; i < n; i += THREADS) {
            int l = 0;
            for (int d = 1; d <= L; d++) l += (i < c[d]) ? 1 : 0;
            len[S.sym[i]] = (uint8_t)l;
            atomicAdd(&S.count[l], 1u);
        }
    }
    __syncthreads();
    // canonical codes: by length, then by symbol
    uint32_t first[MAXBITS + 2];
    first_codes<MAXBITS>(S.count, first);
    for (int a = tid; a < nsym; a += THREADS) {
        const int l = len[a];
        uint32_t v = 0u;
        if (l) {
            uint32_t before = 0u;
            for (int b = 0; b < a; b++) before += (len[b] == l) ? 1u : 0u;
            v = reversed_code(first, l, before);
        }
        code[a] = (uint16_t)v;
    }
    __syncthreads();
}

// ---- bits, from the low end of a word -----------------------------------------------------------------------------------------------
struct BitWriter {
    uint32_t* words;
    uint64_t acc;
    uint32_t word;
    int nb;
    __device__ BitWriter(uint32_t* w, uint32_t bitpos) : words(w), acc(0ull), word(bitpos >> 5), nb((int)(bitpos & 31u)) {}
    __device__ void put(uint32_t v, int l)      // l <= 16
    {
        acc |= (uint64_t)v << nb;
        nb += l;
        if (nb >= 32) { atomicOr(&words[word], (uint32_t)acc); word++; acc >>= 32; nb -= 32; }
    }
    __device__ void flush() { if (nb > 0 && (uint32_t)acc) atomicOr(&words[word], (uint32_t)acc); }
};

// a match of length m (3..258) -> its symbol, the number of extra bits and their value
__device__ __forceinline__ void length_symbol(int m, int& sym, int& eb, uint32_t& ev)
{
    if (m == 258) { sym = 285; eb = 0; ev = 0u; return; }
    const int v = m - 3;
    if (v < 8) { sym = 257 + v; eb = 0; ev = 0u; return; }
    eb = 29 - __clz(v);                         // floor(log2 v) - 2
    sym = 261 + 4 * eb + ((v >> eb) & 3);
    ev = (uint32_t)v & ((1u << eb) - 1u);
}

// byte i of the block in its LDS image: 4 bytes of padding per thread's 64
__device__ __forceinline__ int at(int i) { return i + ((i >> 6) << 2); }

// The tokens that START in [a, b) of a block of n bytes.  run_before: the last run start in front of a (where a continues a run),
// run_after: the first run start at or behind b (n where there is none).  lit(byte), match(length).
template <class Lit, class Match>
__device__ __forceinline__ void walk_tokens(const uint8_t* s_in, int a, int b, int run_before, int run_after, Lit&& lit, Match&& match)
{
    int p = a, s = run_before;
    while (p < b) {
        const uint32_t v = s_in[at(p)];
        const bool start = p == 0 || s_in[at(p - 1)] != v;
        if (start) s = p;
        int e = p + 1;
        while (e < b && s_in[at(e)] == v) e++;
        const int stop = e;                     // the end of the run inside [a, b)
        if (e == b) e = run_after;
        int q = p;
        if (start) { lit(v); q++; }
        const int R = e - s - 1;                // the bytes of the run that repeat their predecessor
        while (q < stop) {
            const int k = q - s - 1;
            const int c = k / 258, r = k - c * 258;
            const int m = min(258, R - 258 * c);
            if (m >= 3) { if (r == 0) match(m); q += m - r; }
            else { lit(v); q++; }
        }
        p = stop;
    }
}

struct DeflateLds {
    uint8_t in[BLOCK + 4 * THREADS];
    uint32_t out[OUT_WORDS];
    uint32_t hist[NLIT_WRITTEN + 2];
    uint8_t len[NLIT_WRITTEN + 2];
    uint16_t code[NLIT_WRITTEN + 2];
    uint32_t cl_hist[NCL + 1];
    uint8_t cl_len[NCL + 1];
    uint16_t cl_code[NCL + 1];
    TreeScratch tree;
    uint32_t wave[4];
    uint32_t adler[2];
    uint32_t hlit, hdr_bits;
};

// raw: the scanline stream of `total` bytes; slots: [blocks][SLOT]; sizes: [blocks]; sums: [blocks] {sum of bytes, sum of (n - i) byte_i} mod ADLER
__global__ void __launch_bounds__(THREADS)
deflate_blocks(const uint8_t* __restrict__ raw, uint32_t total, uint8_t* __restrict__ slots, uint32_t* __restrict__ sizes, uint2* __restrict__ sums)
{
    __shared__ __attribute__((aligned(16))) DeflateLds L;
    const int tid = threadIdx.x;
    const uint32_t blk = blockIdx.x;
    const bool last_block = blk == gridDim.x - 1;
    const uint32_t base = blk * (uint32_t)BLOCK;
    const int n = (int)min((uint32_t)BLOCK, total - base);
    const uint8_t* src = raw + base;
    for (int i = tid; i < n; i += THREADS) L.in[at(i)] = src[i];
    for (int i = tid; i < OUT_WORDS; i += THREADS) L.out[i] = 0u;
    for (int i = tid; i < NLIT_WRITTEN + 2; i += THREADS) L.hist[i] = 0u;
    if (tid < NCL + 1) L.cl_hist[tid] = 0u;
    if (tid < 2) L.adler[tid] = 0u;
    __syncthreads();
    const int a = min(n, tid * SEG), b = min(n, a + SEG);
    // the run starts of this thread's bytes, and Adler-32's two sums
    uint32_t last = 0u, first = (uint32_t)n, s1 = 0u, s2 = 0u;            // last: position + 1, 0 = none
    for (int i = a; i < b; i++) {
        if (i == 0 || L.in[at(i - 1)] != L.in[at(i)]) { last = (uint32_t)i + 1u; if (first == (uint32_t)n) first = (uint32_t)i; }
    }
    adler_partial((uint32_t)n, (uint32_t)a, (uint32_t)b, 1u, [&](uint32_t i) { return (uint32_t)L.in[at((int)i)]; }, s1, s2);
    atomicAdd(&L.adler[0], s1 % ADLER);
    atomicAdd(&L.adler[1], s2 % ADLER);
    uint32_t unused;
    const int run_before = (int)block_scan<false>(last, OpMax(), 0u, &unused, L.wave) - 1;      // (byte 0 starts a run: never -1 where it is used)
    const int run_after = (int)block_scan<true>(first, OpMin(), (uint32_t)n, &unused, L.wave);
    // 1. histogram
    walk_tokens(L.in, a, b, run_before, run_after,
                [&](uint32_t v) { atomicAdd(&L.hist[v], 1u); },
                [&](int m) { int sym, eb; uint32_t ev; length_symbol(m, sym, eb, ev); atomicAdd(&L.hist[sym], 1u); atomicAdd(&L.hist[NLIT_WRITTEN], 1u); });
    if (tid == 0) L.hist[256] = 1u;
    __syncthreads();
    const bool any_match = L.hist[NLIT_WRITTEN] != 0u;
    build_code(L.hist, NLIT_WRITTEN, MAXBITS, L.len, L.code, L.tree);
    // the code lengths' own code: HLIT lengths and one distance length (1 bit for distance 1 where a match exists), no repeat symbols
    if (tid == 0) {
        int h = NLIT_WRITTEN;
        while (h > 257 && L.len[h - 1] == 0) h--;
        L.hlit = (uint32_t)h;
    }
    __syncthreads();
    const int hlit = (int)L.hlit;
    for (int i = tid; i < hlit; i += THREADS) atomicAdd(&L.cl_hist[L.len[i]], 1u);
    if (tid == 0) atomicAdd(&L.cl_hist[any_match ? 1 : 0], 1u);
    __syncthreads();
    build_code(L.cl_hist, NCL, CL_MAXBITS, L.cl_len, L.cl_code, L.tree);
    // 2. thread 0 writes the header; every thread measures its tokens
    if (tid == 0) {
        int hclen = NCL;
        while (hclen > 4 && L.cl_len[cl_order(hclen - 1)] == 0) hclen--;
        BitWriter w(L.out, 0u);
        w.put(last_block ? 1u : 0u, 1);
        w.put(2u, 2);
        w.put((uint32_t)(hlit - 257), 5);
        w.put(0u, 5);
        w.put((uint32_t)(hclen - 4), 4);
        uint32_t bits = 17u + 3u * (uint32_t)hclen;
        for (int i = 0; i < hclen; i++) w.put(L.cl_len[cl_order(i)], 3);
        for (int i = 0; i <= hlit; i++) {
            const int l = i < hlit ? L.len[i] : (any_match ? 1 : 0);
            w.put(L.cl_code[l], L.cl_len[l]);
            bits += L.cl_len[l];
        }
        w.flush();
        L.hdr_bits = bits;
    }
    uint32_t mine = 0u;
    walk_tokens(L.in, a, b, run_before, run_after,
                [&](uint32_t v) { mine += L.len[v]; },
                [&](int m) { int sym, eb; uint32_t ev; length_symbol(m, sym, eb, ev); mine += (uint32_t)L.len[sym] + (uint32_t)eb + 1u; });
    uint32_t token_bits;
    const uint32_t before = block_scan<false>(mine, OpAdd(), 0u, &token_bits, L.wave);          // (its barriers publish the header)
    const uint32_t end_bits = L.hdr_bits + token_bits + L.len[256];
    // a block that is not the last ends with an empty stored block: 3 bits, padding, 00 00 FF FF
    const uint32_t marker_at = (end_bits + 3u + 7u) >> 3;
    const uint32_t dyn_bytes = last_block ? (end_bits + 7u) >> 3 : marker_at + 4u;
    const uint32_t stored_bytes = 5u + (uint32_t)n;
    uint8_t* slot = slots + (size_t)blk * SLOT;
    if (dyn_bytes > stored_bytes) {
        if (tid == 0) {
            slot[0] = last_block ? 1 : 0;
            slot[1] = (uint8_t)(n & 255); slot[2] = (uint8_t)(n >> 8);
            slot[3] = (uint8_t)(~n & 255); slot[4] = (uint8_t)((~n >> 8) & 255);
        }
        for (int i = tid; i < n; i += THREADS) slot[5 + i] = L.in[at(i)];
    } else {
        // 3. packing
        BitWriter w(L.out, L.hdr_bits + before);
        walk_tokens(L.in, a, b, run_before, run_after,
                    [&](uint32_t v) { w.put(L.code[v], L.len[v]); },
                    [&](int m) { int sym, eb; uint32_t ev; length_symbol(m, sym, eb, ev); w.put(L.code[sym], L.len[sym]); w.put(ev, eb + 1); });      // (the extra bits, then the distance code: one 0 bit)
        w.flush();
        if (tid == 0) {
            BitWriter e(L.out, L.hdr_bits + token_bits);
            e.put(L.code[256], L.len[256]);
            e.flush();
            if (!last_block) { atomicOr(&L.out[(marker_at + 2u) >> 2], 0xFFu << (8u * ((marker_at + 2u) & 3u))); atomicOr(&L.out[(marker_at + 3u) >> 2], 0xFFu << (8u * ((marker_at + 3u) & 3u))); }
        }
        __syncthreads();
        uint32_t* slot32 = reinterpret_cast<uint32_t*>(slot);
        for (uint32_t i = tid; i < (dyn_bytes + 3u) >> 2; i += THREADS) slot32[i] = L.out[i];
    }
    if (tid == 0) {
        sizes[blk] = dyn_bytes > stored_bytes ? stored_bytes : dyn_bytes;
        sums[blk] = make_uint2(L.adler[0] % ADLER, L.adler[1] % ADLER);
    }
}

// offs: the exclusive scan of sizes; *total_dev: their sum
__global__ void __launch_bounds__(THREADS)
compact(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes, const uint32_t* __restrict__ offs, const uint32_t* __restrict__ total_dev,
        const uint2* __restrict__ sums, uint32_t total_in, uint8_t* __restrict__ out, uint64_t* __restrict__ out_size)
{
    const uint32_t blk = blockIdx.x;
    const uint8_t* slot = slots + (size_t)blk * SLOT;
    uint8_t* dst = out + 2 + (size_t)offs[blk];
    const uint32_t n = sizes[blk];
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) dst[i] = slot[i];
    if (blk == 0 && threadIdx.x == 0) {
        uint32_t s1 = 1u, s2 = 0u;
        for (uint32_t k = 0; k < gridDim.x; k++) {                          // in block order
            const uint2 p = sums[k];
            adler_append(s1, s2, min((uint32_t)BLOCK, total_in - k * (uint32_t)BLOCK), p.x, p.y);
        }
        const size_t body = *total_dev;
        out[0] = 0x78; out[1] = 0x9C;
        uint8_t* t = out + 2 + body;
        t[0] = (uint8_t)(s2 >> 8); t[1] = (uint8_t)(s2 & 255u); t[2] = (uint8_t)(s1 >> 8); t[3] = (uint8_t)(s1 & 255u);
        *out_size = (uint64_t)body + 6u;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static bool bad_size(int64_t w, int64_t h)
{
    return w < 1 || h < 1 || w > GOF_PNG_MAX_DIM || h > GOF_PNG_MAX_DIM || h * (3 * w + 1) > GOF_PNG_MAX_STREAM;
}

struct Layout { size_t raw, slots, sizes, offs, sums, tmp, total; uint32_t stream, blocks; };

static Layout layout_of(int32_t w, int32_t h)
{
    Layout l{};
    l.stream = (uint32_t)((int64_t)h * (3 * (int64_t)w + 1));
    l.blocks = (l.stream + BLOCK - 1) / BLOCK;
    size_t off = 0;
    l.raw = off;   off += align_up((size_t)l.stream);
    l.slots = off; off += align_up((size_t)l.blocks * SLOT);
    l.sizes = off; off += align_up((size_t)l.blocks * 4);
    l.offs = off;  off += align_up((size_t)l.blocks * 4);
    l.sums = off;  off += align_up((size_t)l.blocks * 8);
    l.tmp = off;   off += align_up(scan_tmp_words(l.blocks) * 4);
    l.total = off;
    return l;
}

} // namespace png
} // namespace gof

using namespace gof;
using namespace gof::png;

extern "C" {

int gof_png_abi_version(void) { return GOF_PNG_ABI_VERSION; }

int32_t gof_png_block_bytes(void) { return GOF_PNG_BLOCK_BYTES; }

size_t gof_png_ws_bytes(int32_t width, int32_t height) { return bad_size(width, height) ? 0 : layout_of(width, height).total; }

size_t gof_png_max_bytes(int32_t width, int32_t height)
{
    if (bad_size(width, height)) return 0;
    const Layout l = layout_of(width, height);
    return (size_t)l.stream + 5 * (size_t)l.blocks + 6;
}

int gof_png_encode(const GofPngEncode* a, const float* planes, void* out, size_t out_capacity, uint64_t* out_size_dev, void* ws, size_t ws_bytes,
                   void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!a) { set_error("png_encode: the arguments are NULL"); return GOF_E_INVALID; }
    if (bad_size(a->width, a->height)) {
        set_error("png_encode: %d x %d pixels: both sizes must lie in 1..%d and the scanlines may take 2^31 - 1 bytes", a->width, a->height, GOF_PNG_MAX_DIM);
        return GOF_E_INVALID;
    }
    if (a->channels != 1 && a->channels != 3) { set_error("png_encode: %d channels (1 or 3)", a->channels); return GOF_E_INVALID; }
    if (a->channels == 3 && a->plane_stride < (int64_t)a->width * a->height) {
        set_error("png_encode: a plane stride of %lld floats is smaller than a plane of %d x %d", (long long)a->plane_stride, a->width, a->height);
        return GOF_E_INVALID;
    }
    if (!planes || !out || !out_size_dev || !ws) { set_error("png_encode: a pointer is NULL"); return GOF_E_INVALID; }
    if (reinterpret_cast<uintptr_t>(ws) & 15u) { set_error("png_encode: the workspace must be 16-byte aligned"); return GOF_E_INVALID; }
    if (reinterpret_cast<uintptr_t>(out_size_dev) & 7u) { set_error("png_encode: the size word must be 8-byte aligned"); return GOF_E_INVALID; }
    const size_t bound = gof_png_max_bytes(a->width, a->height);
    if (out_capacity < bound) { set_error("png_encode: the output has %zu bytes, gof_png_max_bytes gives %zu", out_capacity, bound); return GOF_E_INVALID; }
    const Layout l = layout_of(a->width, a->height);
    if (ws_bytes < l.total) { set_error("png_encode: the workspace has %zu bytes, gof_png_ws_bytes gives %zu", ws_bytes, l.total); return GOF_E_WORKSPACE; }
    uint8_t* w = static_cast<uint8_t*>(ws);
    uint8_t* raw = w + l.raw;
    uint8_t* slots = w + l.slots;
    uint32_t* sizes = reinterpret_cast<uint32_t*>(w + l.sizes);
    uint32_t* offs = reinterpret_cast<uint32_t*>(w + l.offs);
    uint2* sums = reinterpret_cast<uint2*>(w + l.sums);
    uint32_t* tmp = reinterpret_cast<uint32_t*>(w + l.tmp);
    {
        GOF_PROFILE("png_quantise_filter", stream);
        hipLaunchKernelGGL(quantise_filter, dim3((unsigned)a->height), dim3(THREADS), 0, stream, planes, a->plane_stride, (int)a->channels, (int)a->width, raw);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    {
        GOF_PROFILE("png_deflate_blocks", stream);
        hipLaunchKernelGGL(deflate_blocks, dim3(l.blocks), dim3(THREADS), 0, stream, raw, l.stream, slots, sizes, sums);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    const uint32_t* total_dev = nullptr;
    GOF_HIP_CHECK(device_scan_u32(sizes, nullptr, offs, (size_t)l.blocks, false, tmp, &total_dev, stream));
    {
        GOF_PROFILE("png_compact", stream);
        hipLaunchKernelGGL(compact, dim3(l.blocks), dim3(THREADS), 0, stream, slots, sizes, offs, total_dev, sums, l.stream, static_cast<uint8_t*>(out), out_size_dev);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    return GOF_OK;
}

} // extern "C"
