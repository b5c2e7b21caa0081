// rd_parse.h - arithmetic of protocol.Parser.parse's front half (protocol.py:282-318), shared by the host (rd_host.cpp:
// rd_parse_packet; rd_collect_block: the streaming handles' rd_parsed records) and the kernels (rd_parse_kernels.hip: k_parse_select
// and k_freq_err of the batch path, rd_wave_parse of the streaming blocks).  Plain host + device functions, no HIP
// runtime needed: rd_host.cpp is pure host code whichever compiler builds it.
//   bit swap        every byte bit-reversed (protocol.py:79-83, :290)
//   CRC gate        CRC-16-CCITT (poly 0x1021, init 0; crc.py:19-26) over the swapped bytes [2:] must be 0 (:297)
//   frequency error -int(mean(discriminated[index : index + preamble_length]) * sample_rate / 2 pi) (:304-311)
// The parser's own dedupe on the swapped bytes (:293-295) is not restated anywhere: the packets it is given have been
// through the per-call dedupe (dsp.py:203-205) and the swap is a bijection on byte strings, so it never drops one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RD_PHD __host__ __device__ inline __attribute__((always_inline))
#else
#define RD_PHD static inline
#endif

// "no message": a void record, or a packet that failed the CRC (a frequency error is the negation of an int32: never this)
#define RD_FE_NONE INT32_MIN

RD_PHD uint32_t rd_swap_bits8(uint32_t b) {  // protocol.py:79-83
    b = ((b & 0xF0) >> 4) | ((b & 0x0F) << 4);
    b = ((b & 0xCC) >> 2) | ((b & 0x33) << 2);
    b = ((b & 0xAA) >> 1) | ((b & 0x55) << 1);
    return b;
}

// one byte into the CRC (crc.py:24-25, bitwise form)
RD_PHD uint32_t rd_crc16_step(uint32_t crc, uint32_t byte) {
    crc ^= (byte & 0xFF) << 8;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 8; j++) crc = (crc & 0x8000) ? ((crc << 1) ^ 0x1021) & 0xFFFF : (crc << 1) & 0xFFFF;
    return crc;
}

// protocol.py:304-311 from the window's sum: int() truncates toward zero
RD_PHD int32_t rd_freq_err_hz(double sum, long count, double fs) {
    const double mean = sum / (double)count;
    return -(int32_t)((mean * fs) / (2.0 * 3.141592653589793));
}
