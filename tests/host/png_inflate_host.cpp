// Runs spaa_amd/csrc/png_inflate_core.hpp -- the inflate the device runs one wave per image -- on the host with one "lane", so that
// malformed streams meet AddressSanitizer and UBSan before they meet a GPU.  tests/test_png_decode_cpu.py builds this with
// -fsanitize=address,undefined and feeds it the streams of the GPU tests.
//
//   png_inflate_host <container>
// container: "PIS1", uint32 count, then per stream: uint32 payload bytes, uint32 expected output bytes, uint32 expected status,
// uint32 reference bytes (0, or the expected output bytes), the payload, the reference output.  All little-endian.
// Every buffer is allocated to its exact size, so one byte read or written outside it is reported.
// One line per stream: "<index> status=<got> want=<want> out=<bytes> ok|MISMATCH"; the exit status is the number of mismatches.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../spaa_amd/csrc/png_inflate_core.hpp"

namespace {

struct HostPolicy {
    const uint8_t* src;
    uint8_t* dst;
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() {}
    uint8_t in(uint32_t pos) const { return src[pos]; }
    uint8_t& hist(uint32_t p) { return dst[p]; }
    void stored(uint32_t out, uint32_t pos, uint32_t n) { memcpy(dst + out, src + pos, n); }
    void produced(uint32_t) {}
};

bool read_u32(FILE* f, uint32_t& v) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    v = b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24;
    return true;
}

uint8_t* read_exact(FILE* f, uint32_t n) {      // malloc(0) may be NULL: one spare allocation of a byte is not what is wanted either
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);
    if (n && fread(p, 1, n, f) != n) {
        fprintf(stderr, "short container\n");
        exit(100);
    }
    if (!n) {
        free(p);
        p = nullptr;
    }
    return p;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <container>\n", argv[0]);
        return 100;
    }
    FILE* f = fopen(argv[1], "rb");
    char magic[4];
    uint32_t count = 0;
    if (!f || fread(magic, 1, 4, f) != 4 || memcmp(magic, "PIS1", 4) != 0 || !read_u32(f, count)) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 100;
    }
    pngi::Tables* tables = (pngi::Tables*)malloc(sizeof(pngi::Tables));
    int bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t in_len, expect, want, ref_len;
        if (!read_u32(f, in_len) || !read_u32(f, expect) || !read_u32(f, want) || !read_u32(f, ref_len)) return 100;
        uint8_t* payload = read_exact(f, in_len);
        uint8_t* ref = read_exact(f, ref_len);
        uint8_t* out = expect ? (uint8_t*)malloc(expect) : nullptr;
        HostPolicy p = {payload, out};
        uint32_t out_len = 0;
        const int got = pngi::inflate(p, *tables, in_len, expect, out_len);
        bool ok = (uint32_t)got == want;
        if (ok && got == SPAA_PNG_OK) ok = ref_len == expect && out_len == expect && (expect == 0 || memcmp(out, ref, expect) == 0);
        printf("%u status=%d want=%u out=%u %s\n", i, got, want, out_len, ok ? "ok" : "MISMATCH");
        bad += !ok;
        free(payload);
        free(ref);
        free(out);
    }
    free(tables);
    fclose(f);
    return bad > 99 ? 99 : bad;
}
