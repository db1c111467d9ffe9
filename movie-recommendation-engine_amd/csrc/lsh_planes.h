// lsh_planes.h -- the one copy of the sign-plane encoding of a code word: hamming_mfma.hip builds plane tables and query
// fragments with it, lsh_filter.hip writes the planes of the rows it has just encoded (ps_lsh_encode_planes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// 32 code bits -> 32 fp4 nibbles: bit b -> +1 (0x2) / -1 (0xA) = 0xA ^ (b << 3); four bits are spread to the nibble positions
// 0, 4, 8, 12 by OR-ing shifted copies (a multiply would carry between the overlapping copies)
__device__ __forceinline__ uint4 expand_word(uint32_t bits) {
    auto four = [](uint32_t n) { return (n | (n << 3) | (n << 6) | (n << 9)) & 0x1111u; };
    auto eight = [&](uint32_t byte) { return 0xaaaaaaaau ^ ((four(byte & 15u) | (four(byte >> 4) << 16)) << 3); };
    return make_uint4(eight(bits & 255u), eight((bits >> 8) & 255u), eight((bits >> 16) & 255u), eight(bits >> 24));
}
