// parse_asan.cpp - rd_parse_packet (rtldavis_amd/csrc/rd_host.cpp, the arithmetic of rd_parse.h) under
// -fsanitize=address,undefined (tests/test_stream_parse.py): every length 0 .. RD_MAX_PKT_BYTES with exactly sized
// buffers, so that one byte read or written too many is a report; argument errors; valid packets made here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/rtldavis_hip.h"

static unsigned swap8(unsigned b) {
    unsigned r = 0;
    for (int i = 0; i < 8; i++) r |= ((b >> i) & 1u) << (7 - i);
    return r;
}

static unsigned crc16(const std::vector<uint8_t> &d) {  // bit by bit, poly 0x1021, init 0
    unsigned crc = 0;
    for (uint8_t byte : d)
        for (int bit = 7; bit >= 0; bit--) {
            const unsigned top = (crc >> 15) & 1u;
            crc = (crc << 1) & 0xFFFFu;
            if (top ^ ((byte >> bit) & 1u)) crc ^= 0x1021u;
        }
    return crc;
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    srand(seed);
    long valid = 0, invalid = 0;
    for (int round = 0; round < 4000; round++) {
        const int nb = rand() % (RD_MAX_PKT_BYTES + 1);
        std::vector<uint8_t> msgsw;  // swapped message bytes [2:]
        for (int k = 2; k < nb; k++) msgsw.push_back((uint8_t)rand());
        const bool make_valid = nb >= 5 && (round & 1);
        if (make_valid) {
            std::vector<uint8_t> body(msgsw.begin(), msgsw.end() - 2);
            const unsigned c = crc16(body);
            msgsw[msgsw.size() - 2] = (uint8_t)(c >> 8);
            msgsw[msgsw.size() - 1] = (uint8_t)c;
        }
        std::vector<uint8_t> data((size_t)nb);
        for (int k = 0; k < nb; k++) data[(size_t)k] = k < 2 ? (uint8_t)rand() : (uint8_t)swap8(msgsw[(size_t)k - 2]);
        std::vector<uint8_t> msg(nb > 2 ? (size_t)nb - 2 : 0, 0xEE);
        int id = -7;
        const int rc = rd_parse_packet(data.data(), nb, msg.data(), &id);
        const bool want = nb > 2 && crc16(msgsw) == 0;
        if (rc != (want ? 1 : 0)) { printf("round %d: nbytes %d rc %d want %d\n", round, nb, rc, (int)want); return 1; }
        if (want) {
            if (memcmp(msg.data(), msgsw.data(), msgsw.size()) != 0 || id != (msgsw[0] & 7)) { printf("round %d: bytes / id\n", round); return 1; }
            valid++;
        } else {
            if (id != -7) { printf("round %d: id touched\n", round); return 1; }
            invalid++;
        }
        if (make_valid && !want) { printf("round %d: made packet not valid\n", round); return 1; }
    }
    uint8_t d[10] = {0};
    uint8_t m[8];
    int id = 0;
    if (rd_parse_packet(d, -1, m, &id) != RD_ERR_ARG || rd_parse_packet(d, RD_MAX_PKT_BYTES + 1, m, &id) != RD_ERR_ARG ||
        rd_parse_packet(nullptr, 10, m, &id) != RD_ERR_ARG || rd_parse_packet(d, 10, nullptr, &id) != RD_ERR_ARG ||
        rd_parse_packet(d, 10, m, nullptr) != RD_ERR_ARG || rd_parse_packet(nullptr, 0, nullptr, nullptr) != 0) {
        printf("argument checks\n");
        return 1;
    }
    printf("parse ok: %ld valid, %ld invalid\n", valid, invalid);
    return valid > 500 && invalid > 500 ? 0 : 1;
}
