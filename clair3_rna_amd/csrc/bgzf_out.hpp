// bgzf_out.hpp — the BGZF block compressor of libc3r_io.so, defined once in vcfio.cpp and used by both of the library's writers: the
// bgzipped VCF (vcfio.cpp) and the haplotagged BAM (bamio.cpp: c3r_bam_write_haplotagged).  Not part of the C ABI.
#ifndef C3R_BGZF_OUT_HPP
#define C3R_BGZF_OUT_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

namespace c3r_io {

extern const uint8_t BGZF_EOF[28];         // the empty block that ends every BGZF file
const size_t BLK = 0xff00;                 // uncompressed bytes per block: the stream is cut at multiples of it, wherever they fall

// data -> BGZF (blocks of BLK bytes, deflated on `threads` threads) in `out`; coffs[i] = offset of block i in `out`.  The bytes do not
// depend on `threads`.
bool bgzf_compress(const uint8_t *data, size_t n, int threads, std::vector<uint8_t> &out, std::vector<uint64_t> &coffs);

// the deflate threads a caller's `threads` stands for: itself, or (<= 0) the CPUs this process may run on, 32 at the most
int deflate_threads(int threads);

}  // namespace c3r_io
#endif
