// qual_kernels.hpp — k_mask_low_bq: the masked copy of the packed sequence that the kernels which hold the loaded reads against a site
// table read while c3r_set_hap_min_bq is above 0 (include/c3r.h states the rule; tests/qualref.py restates it).  Included by c3r_lib.hip only.
//
// Layout: the quality of base j of read i is byte 2 * seq_off_i + j of `qual` — one byte where the sequence has a nibble — so the kernel
// runs flat over the packed sequence, whatever the read boundaries are: quality byte 2k belongs to the high nibble of sequence byte k,
// byte 2k + 1 to its low nibble.  The padding byte behind a read of odd length is 0xff and never masked.
//
// Rule: a base is masked iff q < Q && q != 0xff.  Q <= 93, so q < Q alone says it.  A masked nibble becomes 15 (N): OR-ing 0xF into a
// nibble gives 15 whatever was there, so the mask is one SWAR byte compare per 8 qualities folded to 4 bytes of nibble masks.
//
// Per lane and chunk: a 16-byte load of qualities, an 8-byte load of sequence, an 8-byte store of seq | mask.  No LDS, no scratch.  The
// count of masked bases is summed inside the wavefront and added once per wavefront (one 64-bit atomic).  Atomics on one address go
// through one at a time (12 ns each, measured: with one chunk per lane and one counter they were 97 % of the kernel), so the grid is capped
// and strides over the chunks — a wavefront adds once, after all its chunks — and the wavefronts spread their sums over MASKBQ_SLOTS
// counters in cache lines of their own, which the host adds up.  Chunk indices are 64-bit: ten million reads of a kilobase are 5 GB of
// sequence.  It moves 2 bytes per base (1 of quality, 1/2 read, 1/2 written): HBM-bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c3r {

constexpr int MASKBQ_THREADS = 128;       // two wavefronts: a streaming kernel without LDS or barriers gains nothing from a larger group
constexpr int MASKBQ_MAX_BLOCKS = 8192;   // 16,384 wavefronts: 64 a compute unit on 256 of them
constexpr int MASKBQ_SLOTS = 64;          // counters the wavefronts add to, by wavefront number
constexpr int MASKBQ_SLOT_WORDS = 16;     // 64-bit words from one counter to the next: 128 bytes

// bit 7 of every byte of x that is below q (0 <= q <= 127), by bytes: no carry crosses a byte because every minuend byte is >= 128 > q
__device__ __forceinline__ uint64_t bytes_below(uint64_t x, uint64_t q_bytes) {
    const uint64_t H = 0x8080808080808080ull;
    const uint64_t ge = ((((x & ~H) | H) - q_bytes) | x) & H;       // low seven bits >= q, or the byte is 128 and above
    return ~ge & H;
}
// the flags of 8 quality bytes (bit 7 each) -> 4 sequence bytes with 0xF in every flagged nibble: byte 2k is the high nibble of byte k
__device__ __forceinline__ uint32_t nibble_mask(uint64_t lt) {
    const uint64_t m = (lt >> 7) * 0xffull;                          // 0xff in every flagged byte
    uint64_t u = (m & 0x00f000f000f000f0ull) | ((m >> 8) & 0x000f000f000f000full);      // one sequence byte in the low half of every 16 bits
    u = (u | (u >> 8)) & 0x0000ffff0000ffffull;
    u = (u | (u >> 16)) & 0x00000000ffffffffull;
    return (uint32_t)u;
}

// qual: 16 n_chunks bytes readable (the bytes behind 2 n_seq_bytes are 0xff); seq: 8 n_chunks bytes readable (slack behind n_seq_bytes);
// out: n_seq_bytes + slack, of which only the first n_seq_bytes are written here.  n_chunks = ceil(n_seq_bytes / 8).  n_masked:
// MASKBQ_SLOTS counters, MASKBQ_SLOT_WORDS words apart, zeroed by the caller; their sum is the count.
__global__ __launch_bounds__(MASKBQ_THREADS) void k_mask_low_bq(const uint8_t *__restrict__ qual, const uint8_t *__restrict__ seq, uint8_t *__restrict__ out,
                                                                 long long n_seq_bytes, long long n_chunks, int min_bq, unsigned long long *n_masked) {
    const long long stride = (long long)gridDim.x * MASKBQ_THREADS;
    const uint64_t qb = (uint64_t)min_bq * 0x0101010101010101ull;
    unsigned long long cnt = 0;
    for (long long c = (long long)blockIdx.x * MASKBQ_THREADS + (long long)threadIdx.x; c < n_chunks; c += stride) {
        const ulonglong2 q = *(const ulonglong2 *)(qual + 16 * c);
        const uint64_t s = *(const uint64_t *)(seq + 8 * c);
        const uint64_t lo = bytes_below(q.x, qb), hi = bytes_below(q.y, qb);
        cnt += (unsigned long long)(__popcll(lo) + __popcll(hi));
        const uint64_t v = s | (uint64_t)nibble_mask(lo) | ((uint64_t)nibble_mask(hi) << 32);
        if (8 * c + 8 <= n_seq_bytes) {
            *(uint64_t *)(out + 8 * c) = v;
        } else {                                                     // the last chunk: only the bytes of the sequence
            for (long long b = 8 * c; b < n_seq_bytes; ++b) out[b] = (uint8_t)(v >> (8 * (int)(b - 8 * c)));
        }
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    const unsigned wave = blockIdx.x * (MASKBQ_THREADS / 64) + (threadIdx.x >> 6);
    if (((int)threadIdx.x & 63) == 0 && cnt) atomicAdd(n_masked + (size_t)(wave % MASKBQ_SLOTS) * MASKBQ_SLOT_WORDS, cnt);
}

}  // namespace c3r
