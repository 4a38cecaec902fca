// radix.h -- the interface of radix.hip: device-wide scan and stable radix sort of u32, and the sort of 63-bit keys built on them.
// radix.hip includes this file itself, so every declaration is checked against its definition.
#pragma once
#include "gof_common.h"

namespace gof {

// ---- scan: out = scan(in[idx]) if idx else scan(in); tmp: scan_tmp_words(n) u32, the grand total is left in *total_dev_out ------------
size_t scan_tmp_words(size_t n);
hipError_t device_scan_u32(const uint32_t* in, const uint32_t* idx, uint32_t* out, size_t n, bool inclusive, uint32_t* tmp,
                           const uint32_t** total_dev_out, hipStream_t stream);

// ---- stable sort of (key, value) pairs by WHOLE 8-bit digits; tmp: rs_tmp_words(n) u32; the result aliases a* or b* -------------------
// The order is by key bits [0, 8 * radix_passes(end_bit)), not [0, end_bit): a pass takes (key >> shift) & 0xFF, so where end_bit is no
// multiple of 8 the bits from end_bit up to the next multiple take part.  A caller's keys are clear there (every caller derives end_bit
// from the largest key) or it wants them sorted.  The result lies in a* after an even number of passes (and for n == 0), else in b*.
size_t rs_tmp_words(size_t n);
hipError_t radix_sort_pairs_u32(uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, size_t n, int end_bit,
                                uint32_t* tmp, uint32_t** keys_res, uint32_t** vals_res, hipStream_t stream, const uint32_t* n_dev = nullptr);
hipError_t radix_sort_pairs_u32_z(uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, size_t n, int end_bit,
                                  uint32_t* tmp, uint32_t** keys_res, uint32_t** vals_res, hipStream_t stream, const uint32_t* n_dev,
                                  size_t zero_words_behind, bool first_hist_done, bool scratch_zeroed = false);
uint32_t rs_units(size_t n);
uint32_t rs_block_items();
int radix_passes(int end_bit);
size_t radix_zero_words(size_t n, int end_bit);
uint32_t* radix_classic_hist(uint32_t* tmp, size_t n, int end_bit);
const uint32_t* radix_sort_error_flag(const uint32_t* tmp, size_t n, int end_bit);

// ---- ascending order of n 63-bit keys (bit 63 clear): a stable sort by the low 32 bits, then by the high 31 ---------------------------
struct Sort63Ws;      // its six buffers and scratch: gof_geom.h, with the function that carves them (the geometry units' header)
// lo[0][i] = low word of keys[i], idx[0][i] = i -- for keys that exist already; a kernel that makes the keys writes the two itself
hipError_t sort63_keys_lo(const unsigned long long* keys, size_t n, const Sort63Ws& w, hipStream_t stream);
// w.lo[0] / w.idx[0] filled as above -> *order = the key indices in ascending key order, equal keys in index order (one of w.idx)
hipError_t sort_keys63(const unsigned long long* keys, size_t n, const Sort63Ws& w, uint32_t** order, hipStream_t stream);

} // namespace gof
