// csrc/lam_host_pack.h -- the very header the product build includes -- as a stand-alone program for
// g++ -fsanitize=address,undefined (tests/test_pack_format_cpu.py builds and runs it; it is never loaded into another process).
// Every buffer is allocated at exactly its stated size, so a read or write past it is a heap overflow the sanitizer reports.
// encode -> decode over row-tiles; checks the decoded bits, the exception count, the overflow condition and that the chosen
// window is a maximal one; prints "ok pack" at the end.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lam_host_pack.h"

using namespace lam;

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    uint64_t z = g_state;
    z ^= z >> 33; z *= 0xff51afd7ed558ccdull; z ^= z >> 33;
    return z;
}
static double uniform() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

// exceptions of a tile for the window below `base`, by definition
static uint32_t outside(const std::vector<uint64_t> &in, uint32_t base)
{
    uint32_t c = 0;
    for (uint64_t b : in) {
        const uint32_t x = (uint32_t)(b >> 52) & 0x7ffu;
        const bool in_win = x >= 1 && x <= 2046 && x <= base && x + 6 >= base;
        c += in_win ? 0 : 1;
    }
    return c;
}

// encode -> decode one tile; want_count < 0: whatever the best window leaves out
static int check(const char *what, const std::vector<uint64_t> &in, long want_count)
{
    const uint32_t cols = (uint32_t)in.size();
    std::vector<unsigned char> data(kPackTileBytes);
    std::vector<uint64_t> exc(kPackCap), out(kPackTile);
    uint32_t header = 0;
    const uint32_t count = pack_tile(in.data(), cols, data.data(), exc.data(), &header);
    const uint32_t base = pack_header_base(header);
    // the window is a maximal one: no base leaves fewer elements outside
    uint32_t least = cols;
    for (uint32_t b = 1; b <= 2046; b++) least = std::min(least, outside(in, b));
    if (base < 1 || base > 2046 || outside(in, base) != least) { std::printf("%s: window below %u is not maximal\n", what, base); return 1; }
    if (count != least) { std::printf("%s: %u exceptions, the window leaves %u outside\n", what, count, least); return 1; }
    if (want_count >= 0 && count != (uint32_t)want_count) { std::printf("%s: %u exceptions, expected %ld\n", what, count, want_count); return 1; }
    if (pack_header_count(header) != count) { std::printf("%s: header count\n", what); return 1; }
    if (count > kPackCap) return 0;                       // not packable: the caller checks the flag, nothing to decode
    unpack_tile(data.data(), exc.data(), header, out.data());
    for (uint32_t j = 0; j < kPackTile; j++) {
        const uint64_t want = j < cols ? in[j] : 0ull;    // the padding decodes to +0.0
        if (out[j] != want) { std::printf("%s: column %u: %016llx != %016llx\n", what, j, (unsigned long long)out[j], (unsigned long long)want); return 1; }
    }
    return 0;
}

int main()
{
    int bad = 0;
    // the layout is a bijection onto the tile's bytes: every byte of every group is written exactly once
    {
        std::vector<int> seen(kPackTileBytes, 0);
        for (uint32_t j = 0; j < kPackTile; j++) {
            uint32_t w, l, e;
            pack_pos(j, &w, &l, &e);
            if (w >= kPackGroups || l >= 64 || e >= 8) return 1;
            if (j != (e >> 1) * 1024 + w * 128 + 2 * l + (e & 1)) return 1;
            for (uint32_t k = 0; k < 4; k++) seen[w * kPackGroupBytes + pack_off_lo(l, e) + k]++;
            for (uint32_t k = 0; k < 2; k++) seen[w * kPackGroupBytes + pack_off_mid(l, e) + k]++;
            seen[w * kPackGroupBytes + pack_off_hi(l, e)]++;
        }
        for (int s : seen) if (s != 1) { std::printf("layout: a byte is written %d times\n", s); return 1; }
    }
    // random bit patterns: almost everything is an exception -> far more than kPackCap, not packable
    {
        std::vector<uint64_t> in(kPackTile);
        for (auto &b : in) b = rnd();
        bad |= check("random bits", in, -1);
        // random mantissas and signs over 7 binades anywhere in the range, top and bottom binade included
        for (uint32_t top : {7u, 8u, 1023u, 2046u}) {
            for (auto &b : in) b = (rnd() & 0x800fffffffffffffull) | (uint64_t)(top - rnd() % 7) << 52;
            bad |= check("seven binades", in, 0);
        }
    }
    // the generator model's law: off-diagonal (2 u - 1) / n, one diagonal entry of the order of 1
    for (uint32_t n : {4096u, 65536u}) {
        std::vector<uint64_t> in(kPackTile);
        for (auto &b : in) b = bits_of((2.0 * uniform() - 1.0) / (double)n);
        in[1234] = bits_of(1.0 + uniform());
        bad |= check("generator law", in, -1);
        std::vector<unsigned char> data(kPackTileBytes);
        std::vector<uint64_t> exc(kPackCap);
        uint32_t header;
        const uint32_t count = pack_tile(in.data(), kPackTile, data.data(), exc.data(), &header);
        if (count < 1 || count > 100) { std::printf("generator law: %u exceptions\n", count); bad = 1; }
    }
    // all-equal exponents
    {
        std::vector<uint64_t> in(kPackTile);
        for (auto &b : in) b = (rnd() & 0x800fffffffffffffull) | 1000ull << 52;
        bad |= check("equal exponents", in, 0);
        for (auto &b : in) b = (rnd() & 0x800fffffffffffffull) | 1ull << 52;       // the lowest normal binade
        bad |= check("lowest binade", in, 0);
    }
    // every special value, next to ordinary ones
    {
        std::vector<uint64_t> in(kPackTile);
        for (auto &b : in) b = bits_of(uniform() + 1.0);
        const uint64_t special[] = {0x0ull, 0x8000000000000000ull, 0x1ull, 0x800fffffffffffffull, 0x7ff0000000000000ull, 0xfff0000000000000ull,
                                    0x7ff8000000000000ull, 0x7ff4000000abcdefull, 0xfff123456789abcdull, 0x7fefffffffffffffull, 0x0010000000000000ull};
        uint32_t k = 0;
        for (uint64_t sp : special) in[37 + 129 * k++] = sp;
        bad |= check("special values", in, (long)(sizeof special / sizeof special[0]));
        // a tile of nothing but zeros: every element an exception
        for (auto &b : in) b = 0;
        bad |= check("zeros", in, kPackTile);
    }
    // exactly kPackCap and kPackCap + 1 exceptions
    for (uint32_t extra : {0u, 1u}) {
        std::vector<uint64_t> in(kPackTile);
        for (auto &b : in) b = bits_of(uniform() + 1.0);
        for (uint32_t k = 0; k < kPackCap + extra; k++) in[(k * 15u) % kPackTile] = k % 3 == 0 ? 0ull : bits_of(1e30 * (1.0 + k));
        bad |= check(extra ? "cap + 1" : "cap", in, (long)(kPackCap + extra));
        std::vector<unsigned char> data(kPackTileBytes);
        std::vector<uint64_t> exc(kPackCap);
        uint32_t header;
        const bool overflow = pack_tile(in.data(), kPackTile, data.data(), exc.data(), &header) > kPackCap;
        if (overflow != (extra == 1)) { std::printf("overflow flag\n"); bad = 1; }
    }
    // ragged tiles: the input holds `cols` elements and not one more
    for (uint32_t cols : {2u, 384u, 1024u, 1026u, 1548u, 4094u}) {
        std::vector<uint64_t> in(cols);
        for (auto &b : in) b = bits_of((2.0 * uniform() - 1.0) / 1547.0);
        in[cols - 1] = 0;                                  // the zero padding of an odd row
        bad |= check("ragged", in, -1);
    }
    // the layout of an image
    {
        const PackLayout L = pack_layout(3, 2);
        if (L.data != 0 || L.exc < 6u * kPackTileBytes || L.hdr < L.exc + 6u * kPackCap * 8 || L.total < L.hdr + 6 * 4 || L.exc % 256 || L.hdr % 256) bad = 1;
    }
    if (bad) return 1;
    std::printf("ok pack\n");
    return 0;
}
