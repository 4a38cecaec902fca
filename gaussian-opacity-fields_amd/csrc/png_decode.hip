// png_decode.hip -- the PNG decoder on HIP (C ABI in include/gof_png_read_hip.h).
//
// metrics.py:25-36 (readImages) opens two PNG files per test view with Pillow -- inflate and unfilter on one CPU thread --, divides by
// 255 and uploads the float tensor from pageable memory, for ALL views of a method before the first metric is computed.  Here the
// zlib streams of a whole batch of files are decoded on the device; the host reads the files and walks the chunks (png_reader.py).
// Three launches over the batch:
//
//   inflate   one workgroup per stream, in rounds.  A round stages the next WIN bytes of the stream in LDS (reads beyond the stream
//             give zeros and are counted, never performed); thread 0 then either parses a block header (the code lengths of a dynamic
//             block included) or resolves up to BATCH symbols of the current block into tokens (output position, literal or length /
//             distance) with every check made where the token is formed: input exhausted, distance in front of the output, output past
//             the scanline buffer.  All threads then do the round's parallel part: copy a stored block, build the canonical decode
//             tables (a first-level table and, for longer codes, the sorted symbol list walked bit by bit), or write the tokens' bytes.
//             Writing is per OUTPUT BYTE: the byte's token is found by binary search; a match byte is followed to its source -- in
//             front of the round's output it is read from memory (written in an earlier round, behind a barrier), inside it the source
//             lies in a strictly earlier token (an overlapping match is reduced modulo its distance first), so the walk ends after at
//             most BATCH hops and no thread reads what this round writes: no order among the writes is needed.  A round consumes at
//             least one bit or ends the stream, so the rounds are bounded by 8 x length.  Behind the last block the Adler-32 of the
//             scanline bytes is formed from per-thread partial sums (integer sums: any order) and compared with the trailer.
//   unfilter  one wave per image.  Paeth and Average are serial along a row and need the row above: lane k owns row 64 band + k and is
//             one pixel behind lane k - 1, so `up` is lane k - 1's pixel of the previous step (one lane shift per step), `up-left` the
//             one before it and `left` the lane's own.  A pixel is at most four bytes: one uint32.  Lane 0 reads the row above from the
//             output bytes lane 63 wrote in the previous band, behind the workgroup barrier at the band's start.
//   convert   bytes -> planes, coalesced, (float)b / 255.0f with the correctly rounded division.
// A stream that fails sets its image's status word; unfilter and convert skip that image.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "../../include/gof_hip.h"
#include "../../include/gof_png_read_hip.h"
#include "gof_common.h"
#include "png_common.h"

namespace gof {
namespace pngr {
using namespace pngc;

constexpr int THREADS = 256;
constexpr int WIN = 4096;                       // bytes of the stream staged per round
constexpr int WIN_WORDS = WIN / 4;
constexpr int WIN_PAD = 4;                      // zero words behind the window: a token that starts inside the limit ends inside them
constexpr uint32_t WIN_LIMIT_BITS = (WIN - 16) * 8;     // no token starts behind this bit of the window
constexpr int BATCH = 512;                      // tokens per round: at most 48 bits each, 3072 bytes < WIN - 16
constexpr int LBITS = 10, DBITS = 9;            // first-level table sizes: literal / length, distance (the code lengths': CL_MAXBITS, every code)
constexpr int NLIT_READ = 288, NDIST = 32;      // code lengths read: the fixed code gives 288 and 32 (a block may use 286 and 30 of them)
constexpr uint32_t LITERAL = 0x80000000u;
static_assert(BATCH * 6 + 600 < WIN - 16, "a round's tokens and a dynamic header fit the window");

enum Phase { PH_HEADER = 0, PH_HUFFMAN = 1, PH_DONE = 2, PH_ERROR = 3 };
enum Job { JOB_NONE = 0, JOB_COPY = 1, JOB_BUILD = 2, JOB_WRITE = 3 };

// the device copy of a descriptor: pointers resolved by the host
struct DevImage {
    uint32_t w, h, c, rowbytes;                 // rowbytes = w * c
    const uint8_t* stream;
    uint64_t stream_len;
    uint8_t* scan;                              // h * (rowbytes + 1) scanline bytes in the workspace
    uint8_t* bytes;                             // [h][w][c]: the caller's or the workspace's
    float* planes;                              // [c][h][w] or NULL
    uint64_t pad;
};
static_assert(sizeof(DevImage) == 64, "DevImage");

// ---- bits, from the low end of the staged window ----------------------------------------------------------------------------------
struct Bits {
    const uint32_t* w;
    uint64_t acc;
    int nb, rw;
    __device__ Bits(const uint32_t* words, uint32_t skip_bits) : w(words), acc(0ull), nb(0), rw(0) { refill(); skip((int)skip_bits); }
    __device__ __forceinline__ void refill()
    {
        if (nb <= 32) {
            const uint32_t v = rw < WIN_WORDS + WIN_PAD ? w[rw] : 0u;
            rw++;
            acc |= (uint64_t)v << nb;
            nb += 32;
        }
    }
    __device__ __forceinline__ uint32_t peek(int k) const { return (uint32_t)acc & ((1u << k) - 1u); }      // k <= 16, after refill()
    __device__ __forceinline__ void skip(int k) { acc >>= k; nb -= k; }
    __device__ __forceinline__ uint32_t get(int k) { refill(); const uint32_t v = peek(k); skip(k); return v; }
    __device__ __forceinline__ uint32_t used() const { return (uint32_t)rw * 32u - (uint32_t)nb; }            // bits of the window consumed
};

struct Code {
    uint32_t count[MAXBITS + 1];                // symbols per code length
    uint16_t sorted[NLIT_READ];                      // the symbols by (length, symbol)
};

// one symbol: the first-level table, or (an entry of length 0: a longer code, or no code) the canonical walk, one bit per length
__device__ __forceinline__ int decode(Bits& b, const uint16_t* table, int tbits, const Code& code)
{
    b.refill();
    const uint32_t e = table[b.peek(tbits)];
    const int l = (int)(e & 15u);
    if (l) { b.skip(l); return (int)(e >> 4); }
    uint32_t bits = (uint32_t)b.acc;
    int c = 0, first = 0, index = 0;
    for (int len = 1; len <= MAXBITS; len++) {
        c |= (int)(bits & 1u);
        bits >>= 1;
        const int cnt = (int)code.count[len];
        if (c - cnt < first) { b.skip(len); return (int)code.sorted[index + (c - first)]; }
        index += cnt;
        first += cnt;
        first <<= 1;
        c <<= 1;
    }
    return -1;
}

// lens[n] -> table[1 << tbits], code.  By all threads.  false: over-subscribed, or incomplete and not (no code at all, where
// `may_be_empty`, or a single code of one bit) -- zlib's rule.
__device__ bool build_tables(const uint8_t* lens, int n, uint16_t* table, int tbits, Code& code, bool may_be_empty)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < (1 << tbits); i += THREADS) table[i] = 0;
    if (tid <= MAXBITS) code.count[tid] = 0u;
    __syncthreads();
    for (int s = tid; s < n; s += THREADS) if (lens[s]) atomicAdd(&code.count[lens[s]], 1u);
    __syncthreads();
    uint32_t offs[MAXBITS + 2], next[MAXBITS + 2];
    int left = 1;
    uint32_t total = 0u;
    bool over = false;
    first_codes<MAXBITS>(code.count, next);
    offs[1] = 0u;
    for (int l = 1; l <= MAXBITS; l++) {
        const uint32_t cnt = code.count[l];
        left = 2 * left - (int)cnt;
        if (left < 0) { over = true; left = 0; }
        total += cnt;
        offs[l + 1] = offs[l] + cnt;
    }
    const bool ok = !over && (left == 0 || (total == 0u && may_be_empty) || (total == 1u && code.count[1] == 1u));
    if (ok) {
        for (int s = tid; s < n; s += THREADS) {
            const int l = lens[s];
            if (!l) continue;
            uint32_t rank = 0u;
            for (int q = 0; q < s; q++) rank += lens[q] == l ? 1u : 0u;
            code.sorted[offs[l] + rank] = (uint16_t)s;
            if (l <= tbits) {
                const uint32_t r = reversed_code(next, l, rank);
                for (uint32_t i = r; i < (1u << tbits); i += 1u << l) table[i] = (uint16_t)((s << 4) | l);
            }
        }
    }
    __syncthreads();
    return ok;
}

struct InflateLds {
    uint32_t win[WIN_WORDS + WIN_PAD];
    uint32_t tok_dst[BATCH];
    uint32_t tok_info[BATCH];                   // LITERAL | byte, or length | distance << 9
    uint16_t lit_table[1 << LBITS];
    uint16_t dist_table[1 << DBITS];
    uint16_t cl_table[1 << CL_MAXBITS];
    uint8_t lens[NLIT_READ + NDIST + 4];             // the literal / length code lengths, the distance code lengths behind them
    Code lit, dist;
    uint32_t adler[2];
    // the state thread 0 carries from round to round, and the round's parallel job
    uint64_t bitpos;
    uint32_t out_pos;
    int32_t phase, status, final_block, job;
    uint32_t job_src, job_len, ntok, nl, nd;
};

__device__ __forceinline__ void fail(InflateLds& L, int32_t status) { L.phase = PH_ERROR; L.status = status; L.job = JOB_NONE; }

// thread 0, PH_HEADER: the three header bits and what the block type needs in front of its data
__device__ void parse_header(InflateLds& L, Bits& b, uint64_t base, uint32_t valid_bits, uint64_t n, uint32_t cap)
{
    L.final_block = (int32_t)b.get(1);
    const uint32_t type = b.get(2);
    if (b.used() > valid_bits) return fail(L, GOF_PNG_READ_E_TRUNCATED);
    if (type == 3u) return fail(L, GOF_PNG_READ_E_BLOCK_TYPE);
    if (type == 0u) {
        b.skip((int)((8u - (b.used() & 7u)) & 7u));
        const uint32_t len = b.get(16), nlen = b.get(16);
        if (b.used() > valid_bits) return fail(L, GOF_PNG_READ_E_TRUNCATED);
        if ((len ^ nlen) != 0xFFFFu) return fail(L, GOF_PNG_READ_E_STORED);
        const uint64_t src = base + (b.used() >> 3);
        if (src + len > n) return fail(L, GOF_PNG_READ_E_TRUNCATED);
        if (len > cap - L.out_pos) return fail(L, GOF_PNG_READ_E_LONG);
        L.job = JOB_COPY;
        L.job_src = (uint32_t)src;              // (a stream has fewer than 2^31 bytes)
        L.job_len = len;
        L.bitpos = (src + len) * 8u;
        L.phase = L.final_block ? PH_DONE : PH_HEADER;
        return;
    }
    if (type == 1u) {
        for (int i = 0; i < NLIT_READ; i++) L.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < NDIST; i++) L.lens[NLIT_READ + i] = 5;
        L.nl = NLIT_READ; L.nd = NDIST;
    } else {
        const uint32_t hlit = b.get(5) + 257u, hdist = b.get(5) + 1u, hclen = b.get(4) + 4u;
        if (hlit > 286u || hdist > 30u) return fail(L, GOF_PNG_READ_E_CODE_LENGTHS);
        uint8_t cl[NCL];
        uint32_t count[CL_MAXBITS + 1], next[CL_MAXBITS + 2];
        for (int i = 0; i < NCL; i++) cl[i] = 0;
        for (int i = 0; i <= CL_MAXBITS; i++) count[i] = 0u;
        for (uint32_t i = 0; i < hclen; i++) { const uint32_t l = b.get(3); cl[cl_order((int)i)] = (uint8_t)l; }
        for (int i = 0; i < NCL; i++) count[cl[i]]++;
        first_codes<CL_MAXBITS>(count, next);
        int left = 1;
        for (int l = 1; l <= CL_MAXBITS; l++) {
            left = 2 * left - (int)count[l];
            if (left < 0) return fail(L, GOF_PNG_READ_E_CODE_LENGTHS);
        }
        if (left != 0) return fail(L, GOF_PNG_READ_E_CODE_LENGTHS);         // (the code-length code must be complete)
        for (int s = 0; s < NCL; s++) {                                     // (in symbol order: next[l] becomes the next symbol's first code)
            const int l = cl[s];
            if (!l) continue;
            const uint32_t r = reversed_code(next, l, 0u);
            next[l]++;
            for (uint32_t i = r; i < (1u << CL_MAXBITS); i += 1u << l) L.cl_table[i] = (uint16_t)((s << 4) | l);
        }
        const uint32_t total = hlit + hdist;    // one run of lengths: a repeat may cross from the literal / length set into the distances
        uint32_t i = 0;
        while (i < total) {
            b.refill();
            const uint32_t e = L.cl_table[b.peek(CL_MAXBITS)];
            b.skip((int)(e & 15u));
            const uint32_t sym = e >> 4;
            if (b.used() > valid_bits) return fail(L, GOF_PNG_READ_E_TRUNCATED);
            if (sym < 16u) { L.lens[i++] = (uint8_t)sym; continue; }
            uint32_t rep, v = 0u;
            if (sym == 16u) {
                if (i == 0u) return fail(L, GOF_PNG_READ_E_CODE_LENGTHS);
                v = L.lens[i - 1];
                rep = 3u + b.get(2);
            } else if (sym == 17u) rep = 3u + b.get(3);
            else rep = 11u + b.get(7);
            if (i + rep > total) return fail(L, GOF_PNG_READ_E_CODE_LENGTHS);
            for (uint32_t k = 0; k < rep; k++) L.lens[i++] = (uint8_t)v;
        }
        if (b.used() > valid_bits) return fail(L, GOF_PNG_READ_E_TRUNCATED);
        if (L.lens[256] == 0) return fail(L, GOF_PNG_READ_E_CODE_LENGTHS);
        // the distance lengths to their own place
        if (hlit < (uint32_t)NLIT_READ) {
            for (int k = (int)hdist - 1; k >= 0; k--) L.lens[NLIT_READ + k] = L.lens[hlit + k];
            for (uint32_t k = hlit; k < (uint32_t)NLIT_READ; k++) L.lens[k] = 0;
        }
        L.nl = hlit; L.nd = hdist;
    }
    L.job = JOB_BUILD;
    L.bitpos = base * 8u + b.used();
    L.phase = PH_HUFFMAN;
}

// thread 0, PH_HUFFMAN: up to BATCH tokens
__device__ void resolve_tokens(InflateLds& L, Bits& b, uint64_t base, uint32_t valid_bits, uint32_t cap)
{
    uint32_t pos = L.out_pos, ntok = 0u;
    int32_t phase = PH_HUFFMAN;
    while (ntok < (uint32_t)BATCH && b.used() <= WIN_LIMIT_BITS) {
        const int sym = decode(b, L.lit_table, LBITS, L.lit);
        if (sym < 0) return fail(L, b.used() > valid_bits ? GOF_PNG_READ_E_TRUNCATED : GOF_PNG_READ_E_SYMBOL);
        if (b.used() > valid_bits) return fail(L, GOF_PNG_READ_E_TRUNCATED);
        if (sym < 256) {
            if (pos >= cap) return fail(L, GOF_PNG_READ_E_LONG);
            L.tok_dst[ntok] = pos;
            L.tok_info[ntok] = LITERAL | (uint32_t)sym;
            ntok++;
            pos++;
            continue;
        }
        if (sym == 256) { phase = L.final_block ? PH_DONE : PH_HEADER; break; }
        const int ls = sym - 257;
        if (ls >= 29) return fail(L, GOF_PNG_READ_E_SYMBOL);
        uint32_t len;
        if (ls < 8) len = 3u + (uint32_t)ls;
        else if (ls == 28) len = 258u;
        else { const int eb = (ls >> 2) - 1; len = 3u + ((4u + ((uint32_t)ls & 3u)) << eb) + b.get(eb); }
        const int ds = decode(b, L.dist_table, DBITS, L.dist);
        if (ds < 0 || ds >= 30) return fail(L, b.used() > valid_bits ? GOF_PNG_READ_E_TRUNCATED : GOF_PNG_READ_E_SYMBOL);
        uint32_t dist;
        if (ds < 4) dist = 1u + (uint32_t)ds;
        else { const int eb = (ds >> 1) - 1; dist = 1u + ((2u + ((uint32_t)ds & 1u)) << eb) + b.get(eb); }
        if (b.used() > valid_bits) return fail(L, GOF_PNG_READ_E_TRUNCATED);
        if (dist > pos) return fail(L, GOF_PNG_READ_E_DISTANCE);
        if (len > cap - pos) return fail(L, GOF_PNG_READ_E_LONG);
        L.tok_dst[ntok] = pos;
        L.tok_info[ntok] = len | (dist << 9);
        ntok++;
        pos += len;
    }
    L.job = JOB_WRITE;
    L.ntok = ntok;
    L.job_len = pos - L.out_pos;
    L.bitpos = base * 8u + b.used();
    L.phase = phase;
}

__global__ void __launch_bounds__(THREADS)
inflate(const DevImage* __restrict__ images, int32_t* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) InflateLds L;
    const int tid = threadIdx.x;
    const DevImage im = images[blockIdx.x];
    const uint8_t* in = im.stream;
    const uint64_t n = im.stream_len;
    uint8_t* out = im.scan;
    const uint32_t cap = im.h * (im.rowbytes + 1u);
    if (tid == 0) {
        L.bitpos = 16u; L.out_pos = 0u; L.phase = PH_HEADER; L.status = GOF_PNG_READ_OK; L.final_block = 0; L.job = JOB_NONE;
        if (n < 2u) fail(L, GOF_PNG_READ_E_TRUNCATED);
        else {
            const uint32_t cmf = in[0], flg = in[1];
            if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 32u) || ((cmf << 8) | flg) % 31u != 0u) fail(L, GOF_PNG_READ_E_ZLIB_HEADER);
        }
    }
    // a round consumes at least one bit of the stream or ends it
    const uint64_t max_rounds = 8u * n + 8u;
    for (uint64_t round = 0; round < max_rounds; round++) {
        __syncthreads();
        if (L.phase >= PH_DONE) break;
        const uint64_t bitpos = L.bitpos;
        const uint64_t base = bitpos >> 3;      // <= n: every consumed bit was checked against the stream's end
        const uint64_t rest = n - base;
        const uint32_t valid = rest < (uint64_t)WIN ? (uint32_t)rest : (uint32_t)WIN;
        for (int i = tid; i < WIN_WORDS + WIN_PAD; i += THREADS) {
            uint32_t v = 0u;
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t at = 4u * (uint32_t)i + k;
                if (at < valid) v |= (uint32_t)in[base + at] << (8u * k);
            }
            L.win[i] = v;
        }
        __syncthreads();
        if (tid == 0) {
            L.job = JOB_NONE;
            Bits b(L.win, (uint32_t)(bitpos & 7u));
            if (L.phase == PH_HEADER) parse_header(L, b, base, valid * 8u, n, cap);
            else resolve_tokens(L, b, base, valid * 8u, cap);
        }
        __syncthreads();
        const int job = L.job;
        if (job == JOB_COPY) {
            const uint8_t* src = in + L.job_src;
            uint8_t* dst = out + L.out_pos;
            const uint32_t len = L.job_len;
            for (uint32_t i = tid; i < len; i += THREADS) dst[i] = src[i];
            __syncthreads();
            if (tid == 0) L.out_pos += len;
        } else if (job == JOB_BUILD) {
            const bool a = build_tables(L.lens, (int)L.nl, L.lit_table, LBITS, L.lit, false);
            const bool d = build_tables(L.lens + NLIT_READ, (int)L.nd, L.dist_table, DBITS, L.dist, true);
            if (tid == 0 && !(a && d)) fail(L, GOF_PNG_READ_E_CODE_LENGTHS);
        } else if (job == JOB_WRITE) {
            const uint32_t start = L.out_pos, total = L.job_len, ntok = L.ntok;
            for (uint32_t j = tid; j < total; j += THREADS) {
                uint32_t p = start + j, hi = ntok, v = 0u;
                for (uint32_t hop = 0; hop <= ntok; hop++) {
                    uint32_t lo = 0u;           // the last token in [0, hi) that starts at or in front of p
                    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (L.tok_dst[mid] <= p) lo = mid; else hi = mid; }
                    const uint32_t info = L.tok_info[lo];
                    if (info & LITERAL) { v = info & 255u; break; }
                    const uint32_t at = L.tok_dst[lo], dist = info >> 9;
                    const uint32_t src = at - dist + (p - at) % dist;      // (an overlapping match repeats its first `dist` bytes)
                    if (src < start) { v = out[src]; break; }
                    p = src;
                    hi = lo;                    // src < at: an earlier token
                }
                out[start + j] = (uint8_t)v;
            }
            __syncthreads();
            if (tid == 0) L.out_pos += total;
        }
    }
    __syncthreads();
    if (L.phase == PH_DONE) {
        // the trailer behind the last block's padding; Adler-32 of the output in steps of ADLER_STEP
        const uint64_t trailer = (L.bitpos + 7u) >> 3;
        const bool complete = L.out_pos == cap && trailer + 4u <= n;
        uint32_t s1 = 1u, s2 = 0u;              // (thread 0's)
        if (complete) {
            for (uint32_t b0 = 0; b0 < cap; b0 += (uint32_t)ADLER_STEP) {
                const uint32_t nb = cap - b0 < (uint32_t)ADLER_STEP ? cap - b0 : (uint32_t)ADLER_STEP;
                if (tid == 0) { L.adler[0] = 0u; L.adler[1] = 0u; }
                __syncthreads();
                uint32_t a = 0u, w = 0u;
                adler_partial(nb, (uint32_t)tid, nb, (uint32_t)THREADS, [&](uint32_t i) { return (uint32_t)out[b0 + i]; }, a, w);
                atomicAdd(&L.adler[0], a % ADLER);
                atomicAdd(&L.adler[1], w % ADLER);
                __syncthreads();
                if (tid == 0) adler_append(s1, s2, nb, L.adler[0], L.adler[1]);
            }
        }
        if (tid == 0) {
            if (L.out_pos != cap) L.status = GOF_PNG_READ_E_SHORT;
            else if (!complete) L.status = GOF_PNG_READ_E_TRUNCATED;
            else {
                const uint32_t want = ((uint32_t)in[trailer] << 24) | ((uint32_t)in[trailer + 1] << 16) | ((uint32_t)in[trailer + 2] << 8) | (uint32_t)in[trailer + 3];
                if (want != ((s2 << 16) | s1)) L.status = GOF_PNG_READ_E_ADLER;
            }
        }
    } else if (tid == 0 && L.phase != PH_ERROR) {
        L.status = GOF_PNG_READ_E_TRUNCATED;    // (the round bound: not reached by a stream whose rounds each consume a bit)
    }
    if (tid == 0) status[blockIdx.x] = L.status;
}

// ---- unfilter -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* p, uint32_t c)
{
    uint32_t v = p[0];
    if (c > 1u) v |= (uint32_t)p[1] << 8;
    if (c > 2u) v |= (uint32_t)p[2] << 16;
    if (c > 3u) v |= (uint32_t)p[3] << 24;
    return v;
}

// raw + predictor(filter, left, up, up-left), per byte
__device__ __forceinline__ uint32_t reconstruct(uint32_t ft, uint32_t raw, uint32_t left, uint32_t up, uint32_t upleft)
{
    uint32_t r = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int a = (int)((left >> (8 * k)) & 255u), b = (int)((up >> (8 * k)) & 255u), c = (int)((upleft >> (8 * k)) & 255u);
        const int pth = paeth(a, b, c);         // (formed for every filter: selects, no branch per byte)
        const int pred = ft == 0u ? 0 : ft == 1u ? a : ft == 2u ? b : ft == 3u ? (a + b) >> 1 : pth;
        r |= ((((raw >> (8 * k)) & 255u) + (uint32_t)pred) & 255u) << (8 * k);
    }
    return r;
}

__global__ void __launch_bounds__(64)
unfilter(const DevImage* __restrict__ images, int32_t* __restrict__ status)
{
    const DevImage im = images[blockIdx.x];
    if (status[blockIdx.x] != GOF_PNG_READ_OK) return;
    const int lane = threadIdx.x;
    const int W = (int)im.w, H = (int)im.h;
    const uint32_t C = im.c;
    const size_t rb = im.rowbytes;
    const uint32_t keep = C == 4u ? 0xFFFFFFFFu : (1u << (8u * C)) - 1u;
    for (int band = 0; band < H; band += 64) {
        const int row = band + lane;
        const bool active = row < H;
        const uint8_t* in = im.scan + (size_t)(active ? row : band) * (rb + 1);
        const uint32_t ft = active ? in[0] : 0u;
        // (the barrier also stands between lane 63's stores of the previous band's last row and lane 0's loads of it)
        if (__syncthreads_or(ft > 4u ? 1 : 0)) {
            if (lane == 0) status[blockIdx.x] = GOF_PNG_READ_E_FILTER;
            return;
        }
        const int rows = H - band < 64 ? H - band : 64;
        const uint8_t* above = band ? im.bytes + (size_t)(band - 1) * rb : nullptr;
        uint8_t* out = im.bytes + (size_t)(active ? row : band) * rb;
        uint32_t left = 0u, up = 0u, res = 0u;
        // the step's loads are issued one step ahead
        uint32_t raw_next = (active && lane == 0) ? load_pixel(in + 1, C) : 0u;
        uint32_t above_next = (lane == 0 && above) ? load_pixel(above, C) : 0u;
        const int steps = W + rows - 1;
        for (int s = 0; s < steps; s++) {
            const int x = s - lane;
            const bool on = active && x >= 0 && x < W;
            const uint32_t raw = raw_next, above_now = above_next;
            const int xn = x + 1;
            const bool on_next = active && xn >= 0 && xn < W;
            raw_next = on_next ? load_pixel(in + 1 + (size_t)xn * C, C) : 0u;
            above_next = (lane == 0 && above && on_next) ? load_pixel(above + (size_t)xn * C, C) : 0u;
            uint32_t up_now = __shfl_up(res, 1, 64);       // lane k - 1's pixel of the previous step: the pixel above
            if (lane == 0) up_now = above_now;
            const uint32_t upleft = up;                     // ... and of the step before it (zero in front of the row)
            up = up_now;
            if (on) {
                res = reconstruct(ft, raw, left, up_now, upleft) & keep;
                left = res;
                uint8_t* o = out + (size_t)x * C;
                o[0] = (uint8_t)res;
                if (C > 1u) o[1] = (uint8_t)(res >> 8);
                if (C > 2u) o[2] = (uint8_t)(res >> 16);
                if (C > 3u) o[3] = (uint8_t)(res >> 24);
            } else {
                res = 0u;
                left = 0u;
            }
        }
    }
}

// ---- convert --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS)
to_planes(const DevImage* __restrict__ images, const int32_t* __restrict__ status, uint32_t blocks_per_image)
{
    const uint32_t img = blockIdx.x / blocks_per_image, part = blockIdx.x % blocks_per_image;
    const DevImage im = images[img];
    if (status[img] != GOF_PNG_READ_OK || !im.planes) return;
    const uint64_t hw = (uint64_t)im.w * im.h, total = hw * im.c;
    for (uint64_t e = (uint64_t)part * THREADS + threadIdx.x; e < total; e += (uint64_t)blocks_per_image * THREADS) {
        const uint64_t c = e / hw, p = e - c * hw;
        im.planes[e] = (float)im.bytes[p * im.c + c] / 255.0f;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static bool bad_image(const GofPngImage& g)
{
    if (g.width < 1 || g.height < 1 || g.width > GOF_PNG_READ_MAX_DIM || g.height > GOF_PNG_READ_MAX_DIM) return true;
    if (g.channels < 1 || g.channels > 4) return true;
    return (int64_t)g.height * ((int64_t)g.width * g.channels + 1) > GOF_PNG_READ_MAX_BYTES;
}

static size_t scan_bytes(const GofPngImage& g) { return (size_t)g.height * ((size_t)g.width * g.channels + 1); }
static size_t pixel_bytes(const GofPngImage& g) { return (size_t)g.height * g.width * g.channels; }

// the workspace: descriptors, then per image the scanline bytes and (bytes_in_ws) the interleaved bytes; 0: refused
static size_t layout_of(int32_t n, const GofPngImage* images, bool bytes_in_ws, std::vector<size_t>* scan_at, std::vector<size_t>* bytes_at)
{
    if (n < 0 || n > GOF_PNG_READ_MAX_IMAGES || (n > 0 && !images)) return 0;
    size_t off = align_up((size_t)(n > 0 ? n : 1) * sizeof(DevImage));
    for (int32_t i = 0; i < n; i++) {
        if (bad_image(images[i])) return 0;
        if (scan_at) (*scan_at)[i] = off;
        off += align_up(scan_bytes(images[i]));
        if (bytes_in_ws) {
            if (bytes_at) (*bytes_at)[i] = off;
            off += align_up(pixel_bytes(images[i]));
        }
    }
    return off;
}

} // namespace pngr
} // namespace gof

using namespace gof;
using namespace gof::pngr;

extern "C" {

int gof_png_read_abi_version(void) { return GOF_PNG_READ_ABI_VERSION; }

size_t gof_png_decode_ws_bytes(int32_t n, const GofPngImage* images, int32_t bytes_in_workspace)
{
    return layout_of(n, images, bytes_in_workspace != 0, nullptr, nullptr);
}

int gof_png_decode_batch(int32_t n, const GofPngImage* images, const void* streams, size_t streams_bytes, void* out_bytes, size_t out_bytes_capacity,
                         float* out_planes, size_t out_planes_capacity, int32_t* status, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n < 0 || n > GOF_PNG_READ_MAX_IMAGES) { set_error("png_decode: %d images (0..%d)", n, GOF_PNG_READ_MAX_IMAGES); return GOF_E_INVALID; }
    if (n == 0) return GOF_OK;
    if (!images || !streams || !status || !ws) { set_error("png_decode: a pointer is NULL"); return GOF_E_INVALID; }
    if (!out_bytes && !out_planes) { set_error("png_decode: out_bytes and out_planes are both NULL"); return GOF_E_INVALID; }
    if (reinterpret_cast<uintptr_t>(ws) & 15u) { set_error("png_decode: the workspace must be 16-byte aligned"); return GOF_E_INVALID; }
    if ((reinterpret_cast<uintptr_t>(out_planes) & 3u) || (reinterpret_cast<uintptr_t>(status) & 3u)) {
        set_error("png_decode: the planes and the status words must be 4-byte aligned");
        return GOF_E_INVALID;
    }
    for (int32_t i = 0; i < n; i++) {
        const GofPngImage& g = images[i];
        if (bad_image(g)) {
            set_error("png_decode: image %d: %d x %d pixels of %d channels: sizes in 1..%d, 1..4 channels, at most 2^31 - 1 scanline bytes", i, g.width, g.height,
                      g.channels, GOF_PNG_READ_MAX_DIM);
            return GOF_E_INVALID;
        }
        if (g.reserved != 0) { set_error("png_decode: image %d: reserved must be 0", i); return GOF_E_INVALID; }
        if (g.stream_bytes > (uint64_t)GOF_PNG_READ_MAX_BYTES || g.stream_offset > streams_bytes || g.stream_bytes > streams_bytes - g.stream_offset) {
            set_error("png_decode: image %d: the stream [%llu, +%llu) lies outside the %zu bytes of streams", i, (unsigned long long)g.stream_offset,
                      (unsigned long long)g.stream_bytes, streams_bytes);
            return GOF_E_INVALID;
        }
        const size_t px = pixel_bytes(g);
        if (out_bytes && (g.bytes_offset > out_bytes_capacity || px > out_bytes_capacity - g.bytes_offset)) {
            set_error("png_decode: image %d: %zu bytes at %llu lie outside the out_bytes capacity of %zu", i, px, (unsigned long long)g.bytes_offset, out_bytes_capacity);
            return GOF_E_INVALID;
        }
        if (out_planes && (g.planes_offset > out_planes_capacity || px > out_planes_capacity - g.planes_offset)) {
            set_error("png_decode: image %d: %zu floats at %llu lie outside the out_planes capacity of %zu", i, px, (unsigned long long)g.planes_offset, out_planes_capacity);
            return GOF_E_INVALID;
        }
    }
    const bool bytes_in_ws = out_bytes == nullptr;
    std::vector<size_t> scan_at((size_t)n), bytes_at((size_t)n);
    const size_t need = layout_of(n, images, bytes_in_ws, &scan_at, &bytes_at);
    if (ws_bytes < need) { set_error("png_decode: the workspace has %zu bytes, gof_png_decode_ws_bytes gives %zu", ws_bytes, need); return GOF_E_WORKSPACE; }
    uint8_t* w = static_cast<uint8_t*>(ws);
    std::vector<DevImage> host((size_t)n);
    uint64_t most = 0;
    for (int32_t i = 0; i < n; i++) {
        const GofPngImage& g = images[i];
        DevImage& d = host[(size_t)i];
        d.w = (uint32_t)g.width; d.h = (uint32_t)g.height; d.c = (uint32_t)g.channels; d.rowbytes = d.w * d.c;
        d.stream = static_cast<const uint8_t*>(streams) + g.stream_offset;
        d.stream_len = g.stream_bytes;
        d.scan = w + scan_at[(size_t)i];
        d.bytes = bytes_in_ws ? w + bytes_at[(size_t)i] : static_cast<uint8_t*>(out_bytes) + g.bytes_offset;
        d.planes = out_planes ? out_planes + g.planes_offset : nullptr;
        d.pad = 0;
        if (pixel_bytes(g) > most) most = pixel_bytes(g);
    }
    DevImage* dev = reinterpret_cast<DevImage*>(w);
    GOF_HIP_CHECK(hipMemcpyAsync(dev, host.data(), (size_t)n * sizeof(DevImage), hipMemcpyHostToDevice, stream));
    {
        GOF_PROFILE("png_inflate", stream);
        hipLaunchKernelGGL(inflate, dim3((unsigned)n), dim3(THREADS), 0, stream, dev, status);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    {
        GOF_PROFILE("png_unfilter", stream);
        hipLaunchKernelGGL(unfilter, dim3((unsigned)n), dim3(64), 0, stream, dev, status);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    if (out_planes) {
        GOF_PROFILE("png_to_planes", stream);
        uint64_t per = (most + (uint64_t)THREADS * 16u - 1u) / ((uint64_t)THREADS * 16u);
        per = per < 1u ? 1u : per > 256u ? 256u : per;
        hipLaunchKernelGGL(to_planes, dim3((unsigned)((uint64_t)n * per)), dim3(THREADS), 0, stream, dev, status, (uint32_t)per);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    return GOF_OK;
}

} // extern "C"
