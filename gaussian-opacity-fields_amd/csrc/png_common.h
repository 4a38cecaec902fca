// png_common.h -- what the PNG encoder (png_encode.hip) and the PNG decoder (png_decode.hip) share of their two specifications, PNG
// and zlib / deflate (RFC 1950, 1951): each fact is written here once and used in both directions.  Inline device code and constants
// only: no kernels, no LDS, no state.  (The bit writer / bit reader and the length <-> symbol maps are inverse operations, not copies:
// they stay with their units.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gof {
namespace pngc {

constexpr int NCL = 19;                         // code-length symbols
constexpr int MAXBITS = 15;                     // the longest literal / length or distance code
constexpr int CL_MAXBITS = 7;                   // the longest code of the code-length code
constexpr uint32_t ADLER = 65521u;
// Adler-32 is formed in steps of at most this many bytes, 64 per thread of a workgroup of 256: a thread's sum of (n - i) * byte_i
// stays below 64 * 16384 * 255 < 2^32
constexpr int ADLER_STEP = 16384;

// ---- Adler-32 from integer partial sums (any order gives the same sums) ------------------------------------------------------------------
// One thread's part of a step of n <= ADLER_STEP bytes: over i = first, first + stride, ... < end,  a += byte(i),  w += (n - i) byte(i).
template <class Byte>
__device__ __forceinline__ void adler_partial(uint32_t n, uint32_t first, uint32_t end, uint32_t stride, Byte&& byte, uint32_t& a, uint32_t& w)
{
    for (uint32_t i = first; i < end; i += stride) {
        const uint32_t v = byte(i);
        a += v;
        w += (n - i) * v;
    }
}

// (s1, s2) of the bytes so far, continued by a step of n bytes whose partial sums are (a, w), each below 2^31: s2 gains n times the s1
// in front of the step.  A stream starts with (1, 0).
__device__ __forceinline__ void adler_append(uint32_t& s1, uint32_t& s2, uint32_t n, uint32_t a, uint32_t w)
{
    s2 = (uint32_t)(((uint64_t)s2 + (uint64_t)n * s1 + w) % ADLER);
    s1 = (s1 + a) % ADLER;
}

// ---- the PNG filters' Paeth predictor: a = left, b = up, c = up-left; ties go to a, then b -------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// ---- deflate's prefix codes --------------------------------------------------------------------------------------------------------------
// the order in which a dynamic block's header lists the lengths of the code-length code
__device__ __forceinline__ int cl_order(int i)
{
    constexpr uint8_t order[NCL] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
    return order[i];
}

// Canonical codes: the symbols by (length, symbol) take consecutive codes, a longer code continuing the shorter ones' with a 0 bit.
// count[1..MAXB] = symbols per length -> first[1..MAXB + 1] = the code of the first symbol of each length.
template <int MAXB, class Count>
__device__ __forceinline__ void first_codes(const Count* count, uint32_t* first)
{
    first[1] = 0u;
    for (int l = 1; l <= MAXB; l++) first[l + 1] = (first[l] + (uint32_t)count[l]) << 1;
}

// the code of the symbol that is number `rank` among those of length l (l >= 1), bit-reversed: a code goes into the stream from its high
// bit, everything else from the low one
__device__ __forceinline__ uint32_t reversed_code(const uint32_t* first, int l, uint32_t rank) { return __brev(first[l] + rank) >> (32 - l); }

} // namespace pngc
} // namespace gof
