// Stand-alone check of csrc/ngp_workspace.h, built with -fsanitize=address,undefined by tests/test_workspace_host.py.
// Includes nothing of the project but the carver.  Exit status 0 and "carver ok" on success.
#include "ngp_workspace.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct piece { unsigned char* p; size_t bytes, align; };

struct layout {
    uint32_t* a; uint8_t* b; double* c; uint16_t* d; float* e; uint64_t* f; uint8_t* g;
    size_t total;
};

// counts chosen so that every alignment has padding to skip: 5 u32 | 3 u8 | 7 f64 at 8 | 129 u16 at 256 | nothing at 4 | 2 u64 at 64 | 1 u8; total rounded to 256
static layout make(size_t scale, void* base, piece* out) {
    ngp_carver c(base);
    layout w;
    w.a = c.take<uint32_t>(5 * scale, 1);
    w.b = c.take<uint8_t>(3, 1);
    w.c = c.take<double>(7 * scale, 8);
    w.d = c.take<uint16_t>(129 * scale);
    w.e = c.take<float>(0, 4);
    w.f = c.take<uint64_t>(2, 64);
    w.g = c.take<uint8_t>(1, 1);
    w.total = c.total(256);
    if (out) {
        out[0] = {(unsigned char*)w.a, 20 * scale, 1}; out[1] = {(unsigned char*)w.b, 3, 1}; out[2] = {(unsigned char*)w.c, 56 * scale, 8};
        out[3] = {(unsigned char*)w.d, 258 * scale, 256}; out[4] = {(unsigned char*)w.e, 0, 4}; out[5] = {(unsigned char*)w.f, 16, 64};
        out[6] = {(unsigned char*)w.g, 1, 1};
    }
    return w;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "carver_check.cpp:%d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    CHECK(ngp_align256(0) == 0 && ngp_align256(1) == 256 && ngp_align256(256) == 256 && ngp_align256(257) == 512);
    const size_t scales[3] = {1, 3, 64};
    for (size_t scale : scales) {
        const layout sized = make(scale, nullptr, nullptr);
        CHECK(!sized.a && !sized.b && !sized.c && !sized.d && !sized.e && !sized.f && !sized.g);      // a null base hands out null pieces
        CHECK(sized.total % 256 == 0 && sized.total > 0);
        unsigned char* block = (unsigned char*)malloc(sized.total);                                    // exactly `total` bytes: ASan guards both ends
        CHECK(block);
        piece p[7];
        const layout real = make(scale, block, p);
        CHECK(real.total == sized.total);                                                              // same total with and without a base
        CHECK(p[0].p == block);
        for (int i = 0; i < 7; i++) {
            const size_t off = (size_t)(p[i].p - block);
            CHECK(off % p[i].align == 0);                                                              // every piece at its alignment
            const size_t end = off + p[i].bytes;
            CHECK(end <= (i < 6 ? (size_t)(p[i + 1].p - block) : real.total));                         // and clear of the next one
            CHECK(ngp_ws_holds(block, real.total, p[i].p, p[i].bytes));
            CHECK(!ngp_ws_holds(block, end ? end - 1 : 0, p[i].p, p[i].bytes) || end == 0);
        }
        CHECK((size_t)((unsigned char*)real.c - block) == ((20 * scale + 3 + 7) & ~(size_t)7));       // an explicit alignment of 8: the next multiple of 8, not of 256
        CHECK((size_t)((unsigned char*)real.d - block) % 256 == 0 && (size_t)((unsigned char*)real.f - block) % 256 != 0);
        for (int i = 0; i < 7; i++) memset(p[i].p, 0x10 + i, p[i].bytes);                              // every byte of every piece
        for (size_t k = 0; k < 5 * scale; k++) real.a[k] += 1u;                                       // and typed accesses: UBSan checks their alignment
        for (size_t k = 0; k < 7 * scale; k++) real.c[k] = (double)k;
        for (size_t k = 0; k < 129 * scale; k++) real.d[k] = (uint16_t)k;
        real.f[0] = 1; real.f[1] = 2;
        for (int i = 1; i < 7; i += 5)                                                                  // the untyped pieces kept their fill: nothing overlapped
            for (size_t k = 0; k < p[i].bytes; k++) CHECK(p[i].p[k] == 0x10 + i);
        CHECK(real.a[0] == 0x10101011u && real.c[6] == 6.0 && real.d[128] == 128 && real.f[1] == 2);
        free(block);
    }
    puts("carver ok");
    return 0;
}
