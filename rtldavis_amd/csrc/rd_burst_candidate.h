// rd_burst_candidate.h - the test of one candidate tau of the burst decoders (include/rtldavis_hip.h, BURST DECODE, steps
// 5, 5a, 5b and 6'): pure integer code over the candidate's N symbol sums s[SL k].  Plain host + device functions in the
// convention of rd_parse.h: k_chan_burst_decode and k_chan_burst_expect call them on LDS, tests/host_harness.cpp compiles
// the same text for the CPU and tests/test_burst_repair_cpu.py holds it to the Python model.
#pragma once
#include <stdint.h>

#include "../../include/rtldavis_hip.h"
#include "rd_parse.h"

#if defined(__HIPCC__)
#define RD_UNROLL _Pragma("unroll")
#else
#define RD_UNROLL
#endif

// E[k], 16 <= k < N: the CRC of the packet whose only set symbol is k.  Symbol k is bit 7 - (k & 7) of on-air byte k >> 3,
// bit k & 7 of the bit-swapped byte; the CRC has init 0 and is linear, so the syndrome of a packet is the XOR of the E of
// its wrong symbols.
RD_PHD uint32_t rd_bd_syndrome(int k, int n_sym) {
    uint32_t crc = 0u;
    for (int b = 2; b < n_sym >> 3; b++) crc = rd_crc16_step(crc, b == (k >> 3) ? 1u << (k & 7) : 0u);
    return crc;
}

struct rd_bd_cand {
    uint32_t flips;             // count | k1 << 8 | k2 << 16 (k1 < k2), 0 for a candidate that passes as it is
    uint64_t margin;            // min |s| over the symbols that were not flipped
    uint32_t id;                // bits 0 .. 2: symbols 16, 17, 18 after the correction
};

// The candidate whose symbol k is s[SL k] > 0: false unless its first 16 symbols equal sync (the first in bit 15) and its
// N symbols, packed MSB first, pass the CRC gate of rd_parse.h - as they are or, with REPAIR, after flipping one symbol
// (max_flips >= 1) or two (max_flips >= 2) of the RD_BD_REPAIR_L payload symbols smallest in (|s|, k): the singles in
// list order, then the pairs in (a, b) order, the first whose E (E[k] = rd_bd_syndrome(k, N)) equals the syndrome.
template <bool REPAIR>
RD_PHD bool rd_bd_candidate(const int64_t *s, int SL, int N, uint32_t sync, int max_flips, const uint16_t *E, rd_bd_cand &out) {
    uint64_t margin = ~0ull;
    uint32_t word = 0u, crc = 0u, id = 0u;
    for (int k = 0; k < N; k++) {
        const int64_t v = s[SL * k];
        const uint32_t bit = v > 0 ? 1u : 0u;
        if (k < 16 && bit != ((sync >> (15 - k)) & 1u)) return false;
        const uint64_t mag = (uint64_t)(v > 0 ? v : -v);
        margin = mag < margin ? mag : margin;
        word = ((word << 1) | bit) & 0xFFu;
        if ((k & 7) == 7 && k >= 16) crc = rd_crc16_step(crc, rd_swap_bits8(word));
        if (k == 23) id = rd_swap_bits8(word) & 7u;       // symbols 16, 17, 18 are its bits 0, 1, 2
    }
    uint32_t fl = 0u;
    if (crc != 0u) {                                      // steps 5a, 5b: the syndrome S = crc
        if constexpr (!REPAIR) return false;
        uint64_t lm[RD_BD_REPAIR_L];                      // the list, ascending in (|s|, k)
        int lk[RD_BD_REPAIR_L];
        RD_UNROLL
        for (int a = 0; a < RD_BD_REPAIR_L; a++) {
            lm[a] = ~0ull;
            lk[a] = INT32_MAX;
        }
        for (int k = 16; k < N; k++) {
            const int64_t v = s[SL * k];
            uint64_t cm = (uint64_t)(v > 0 ? v : -v);
            int ck = k;
            RD_UNROLL
            for (int a = 0; a < RD_BD_REPAIR_L; a++)
                if (cm < lm[a] || (cm == lm[a] && ck < lk[a])) {   // the entry moves in, the one it displaces goes on
                    const uint64_t tm = lm[a];
                    const int tk = lk[a];
                    lm[a] = cm;
                    lk[a] = ck;
                    cm = tm;
                    ck = tk;
                }
        }
        uint32_t e[RD_BD_REPAIR_L];
        RD_UNROLL
        for (int a = 0; a < RD_BD_REPAIR_L; a++) e[a] = E[lk[a]];   // (N >= 40: 24 payload symbols, the list is full)
        RD_UNROLL
        for (int a = 0; a < RD_BD_REPAIR_L; a++)
            if (fl == 0u && e[a] == crc) fl = 1u | ((uint32_t)lk[a] << 8);
        if (max_flips >= 2) {
            RD_UNROLL
            for (int a = 0; a < RD_BD_REPAIR_L; a++)
                RD_UNROLL
                for (int b = a + 1; b < RD_BD_REPAIR_L; b++)
                    if (fl == 0u && (e[a] ^ e[b]) == crc) {
                        const uint32_t ka = (uint32_t)lk[a], kb = (uint32_t)lk[b];
                        fl = 2u | ((ka < kb ? ka : kb) << 8) | ((ka < kb ? kb : ka) << 16);
                    }
        }
        if (fl == 0u) return false;
        const int k1 = (int)((fl >> 8) & 0xFFu), k2 = (fl & 0xFFu) == 2u ? (int)(fl >> 16) : -1;
        margin = ~0ull;                                   // step 6': over the symbols that were not flipped
        for (int k = 0; k < N; k++) {
            if (k == k1 || k == k2) continue;
            const int64_t v = s[SL * k];
            const uint64_t mag = (uint64_t)(v > 0 ? v : -v);
            margin = mag < margin ? mag : margin;
        }
        if (k1 >= 16 && k1 <= 18) id ^= 1u << (k1 - 16);  // the id of the corrected symbols
        if (k2 >= 16 && k2 <= 18) id ^= 1u << (k2 - 16);
    }
    out.flips = fl;
    out.margin = margin;
    out.id = id;
    return true;
}
