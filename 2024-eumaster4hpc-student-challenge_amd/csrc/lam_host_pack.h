// lam_host_pack.h -- the packed fp64 matrix format of the general product (option "packed"): 7 bytes an element, lossless.
// No HIP include and no HIP call: this header is part of the product build (csrc/lam_hip.hip includes it through lam_kernels.h;
// pack_rows_kernel and gemv_packed_kernel use the element functions below) AND is compiled by plain g++ with
// -fsanitize=address,undefined into tests/host_pack/ (`-m "not gpu"`), where pack_tile / unpack_tile are the reference coder.
//
// Unit: one matrix row x one 4096-column tile, split into the 8 wave groups of the product kernel (512 elements each, 8 per
// lane).  Tile column j = s * 1024 + w * 128 + 2 l + i (s = 0..3, i = 0..1) is element e = 2 s + i of lane l of wave group w:
// the product kernel's own traversal order, so a lane gets its 8 elements of a row and tile from four coalesced loads.
// A wave group is kPackGroupBytes = 3584 contiguous bytes:
//     [   0, 2048)  low words   (mantissa bits 0..31):  lane l, elements 0..3 at 16 l, elements 4..7 at 1024 + 16 l
//     [2048, 3072)  middle halves: lane l at 2048 + 16 l, element e at + 2 e
//     [3072, 3584)  high bytes: lane l at 3072 + 8 l, element e at + e
// High byte and middle half are the 24-bit word t = field << 21 | (mantissa bits 32..51) << 1 | sign, laid out so that the upper
// word of the double is ((t >> 1) + ((base - 6) << 20)) | t << 31: three integer operations.
// Per (row, tile) one header word, base | count << 16, and a list of up to kPackCap exact 8-byte values.  base is the biased
// exponent at the top of the window of kPackWindow = 7 consecutive binades that holds the most elements of the tile (not the
// maximum).  field = 6 - code: exponent code 0..6 is a normal number with biased exponent base - code; field 7 is an exception
// -- anything outside the window: larger and smaller elements, +-0, denormals, +-Inf, NaNs with their payload -- whose low word
// is its index into the list; the value is the list's raw bits.  Index kPackZeroIdx is reserved: it decodes to +0.0 (the padding
// behind a ragged last tile).
// More than kPackCap exceptions in one (row, tile): the matrix content is not packable and the plain kernel runs.
#pragma once

#include <stdint.h>

#include <cstddef>
#include <cstring>

#if defined(__HIPCC__)
#define LAM_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define LAM_HOST_DEVICE inline
#endif

namespace lam {

constexpr uint32_t kPackTile = 4096;           // columns of a tile (the product kernel's p tile)
constexpr uint32_t kPackGroups = 8;            // wave groups of a tile
constexpr uint32_t kPackGroupBytes = 3584;     // 512 elements of 7 bytes
constexpr uint32_t kPackTileBytes = kPackGroups * kPackGroupBytes;
constexpr uint32_t kPackWindow = 7;            // binades an exponent code addresses
constexpr uint32_t kPackCap = 256;             // exceptions a (row, tile) may hold: 2 rows x (kPackCap + 1) x 8 B of LDS next to the
                                               // 32-KiB p tile keep four 512-thread workgroups on a CU (4 x 36.2 KiB of 160 KiB)
constexpr uint32_t kPackZeroIdx = kPackCap;    // the reserved index: +0.0
constexpr uint32_t kPackFirst = 64;            // values of a list the product kernel loads without knowing the list's length
constexpr uint32_t kPackExpBins = 2048;

// where tile column j lives: wave group, lane, element of the lane
LAM_HOST_DEVICE void pack_pos(uint32_t j, uint32_t *w, uint32_t *l, uint32_t *e)
{
    *w = (j >> 7) & 7u;
    *l = (j & 127u) >> 1;
    *e = 2u * (j >> 10) + (j & 1u);
}
// The batched product's traversal of the image (multi_gemv_packed_kernel, fp64, K = 1, 2, 4 columns): its batch tile holds
// kPackTile / K columns, kPackManySteps / K steps of 512 (4 waves x 64 lanes x 2 columns).  Wave w of step s of batch tile tt
// covers the 128 global columns behind (tt * (8 / K) + s) * 512 + w * 128: lane l's two are elements 2 * pair, 2 * pair + 1 of lane
// l of wave group `group` of (row, tile) unit `unit` -- wave w reads groups w and w + 4 in turn, one pair every second step.
constexpr uint32_t kPackManySteps = 8;         // steps of the batched product in a unit
constexpr uint32_t kPackManyMaxK = 4;
LAM_HOST_DEVICE void pack_many_pos(uint32_t K, uint32_t tt, uint32_t s, uint32_t w, uint32_t *unit, uint32_t *group, uint32_t *pair)
{
    const uint32_t q = tt * (kPackManySteps / K) + s;
    *unit = q / kPackManySteps;
    *group = w + 4u * (q & 1u);
    *pair = (q % kPackManySteps) >> 1;
}
// byte offsets inside a wave group
LAM_HOST_DEVICE uint32_t pack_off_lo(uint32_t l, uint32_t e) { return (e >> 2) * 1024u + l * 16u + (e & 3u) * 4u; }
LAM_HOST_DEVICE uint32_t pack_off_mid(uint32_t l, uint32_t e) { return 2048u + l * 16u + e * 2u; }
LAM_HOST_DEVICE uint32_t pack_off_hi(uint32_t l, uint32_t e) { return 3072u + l * 8u + e; }

LAM_HOST_DEVICE uint32_t pack_exp_of(uint64_t bits) { return (uint32_t)(bits >> 52) & 0x7ffu; }
// a normal number (what the histogram counts: biased exponent 1..2046)
LAM_HOST_DEVICE bool pack_is_normal(uint64_t bits) { const uint32_t x = pack_exp_of(bits); return x >= 1u && x <= 2046u; }
// does the window whose top binade is `base` hold this element?
LAM_HOST_DEVICE bool pack_in_window(uint64_t bits, uint32_t base)
{
    const uint32_t x = pack_exp_of(bits);
    return x >= 1u && x <= 2046u && x <= base && base - x < kPackWindow;
}
// elements of a tile inside the window below `base` (hist: kPackExpBins counts by biased exponent; bins 0 and 2047 are not used)
LAM_HOST_DEVICE uint32_t pack_window_count(const uint32_t *hist, uint32_t base)
{
    uint32_t c = 0;
    for (uint32_t k = 0; k < kPackWindow; k++)
        if (base >= 1u + k && base - k <= 2046u) c += hist[base - k];
    return c;
}
// the order windows are compared in: more elements first, then the higher window
LAM_HOST_DEVICE uint32_t pack_window_key(uint32_t count, uint32_t base) { return count << 11 | base; }

// the three fields of an element inside the window ...
LAM_HOST_DEVICE void pack_encode(uint64_t bits, uint32_t base, uint32_t *lo, uint32_t *mid, uint32_t *hi)
{
    const uint32_t field = 6u - (base - pack_exp_of(bits));
    const uint32_t t = field << 21 | ((uint32_t)(bits >> 32) & 0xfffffu) << 1 | (uint32_t)(bits >> 63);
    *lo = (uint32_t)bits;
    *mid = t & 0xffffu;
    *hi = t >> 16;
}
// ... and of exception number `index` of its (row, tile)
LAM_HOST_DEVICE void pack_encode_exception(uint32_t index, uint32_t *lo, uint32_t *mid, uint32_t *hi)
{
    *lo = index;
    *mid = 0u;
    *hi = 7u << 5;
}
// t = high byte << 16 | middle half
LAM_HOST_DEVICE bool pack_is_exception(uint32_t t) { return t >= 7u << 21; }
// what the window contributes to the upper word of every element of a (row, tile); may wrap for base < 6, the sum below does not
LAM_HOST_DEVICE uint32_t pack_exp_shift(uint32_t base) { return (base - 6u) << 20; }
// the bits of an element that is not an exception
LAM_HOST_DEVICE uint64_t pack_decode(uint32_t lo, uint32_t t, uint32_t exp_shift)
{
    const uint32_t hw = ((t >> 1) + exp_shift) | t << 31;
    return (uint64_t)hw << 32 | lo;
}

LAM_HOST_DEVICE uint32_t pack_header(uint32_t base, uint32_t count) { return base | (count > 0xffffu ? 0xffffu : count) << 16; }
LAM_HOST_DEVICE uint32_t pack_header_base(uint32_t h) { return h & 0x7ffu; }
LAM_HOST_DEVICE uint32_t pack_header_count(uint32_t h) { return h >> 16; }

// bytes of the packed image of nrows x ntiles tiles: elements, exception lists, headers (each part 256-byte aligned)
struct PackLayout { size_t data, exc, hdr, total; };
inline PackLayout pack_layout(uint64_t nrows, uint64_t ntiles)
{
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    PackLayout L;
    L.data = 0;
    L.exc = up((size_t)nrows * ntiles * kPackTileBytes);
    L.hdr = L.exc + up((size_t)nrows * ntiles * kPackCap * 8);
    L.total = L.hdr + up((size_t)nrows * ntiles * 4);
    return L;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the reference coder (host): one (row, tile) ------------------------------------------------------------------------------
// in: `cols` <= kPackTile elements as raw bits; the columns behind them are padding (reserved index).  data: kPackTileBytes.
// exc: kPackCap values.  Returns the number of exceptions; more than kPackCap: the tile is not packable (data then holds the
// reserved index in place of the exceptions that found no room).
inline uint32_t pack_tile(const uint64_t *in, uint32_t cols, unsigned char *data, uint64_t *exc, uint32_t *header)
{
    uint32_t hist[kPackExpBins];
    memset(hist, 0, sizeof hist);
    for (uint32_t j = 0; j < cols; j++)
        if (pack_is_normal(in[j])) hist[pack_exp_of(in[j])]++;
    uint32_t best = 0;
    for (uint32_t base = 1; base <= 2046u; base++) {
        const uint32_t key = pack_window_key(pack_window_count(hist, base), base);
        if (key > best) best = key;
    }
    const uint32_t base = best & 0x7ffu;
    uint32_t count = 0;
    for (uint32_t j = 0; j < kPackTile; j++) {
        uint32_t w, l, e, lo, mid, hi;
        pack_pos(j, &w, &l, &e);
        if (j >= cols) pack_encode_exception(kPackZeroIdx, &lo, &mid, &hi);
        else if (pack_in_window(in[j], base)) pack_encode(in[j], base, &lo, &mid, &hi);
        else {
            if (count < kPackCap) exc[count] = in[j];
            pack_encode_exception(count < kPackCap ? count : kPackZeroIdx, &lo, &mid, &hi);
            count++;
        }
        unsigned char *g = data + (size_t)w * kPackGroupBytes;
        const uint16_t m16 = (uint16_t)mid;
        memcpy(g + pack_off_lo(l, e), &lo, 4);
        memcpy(g + pack_off_mid(l, e), &m16, 2);
        g[pack_off_hi(l, e)] = (unsigned char)hi;
    }
    *header = pack_header(base, count);
    return count;
}

// out: kPackTile elements as raw bits (the padding comes back as +0.0)
inline void unpack_tile(const unsigned char *data, const uint64_t *exc, uint32_t header, uint64_t *out)
{
    const uint32_t base = pack_header_base(header);
    for (uint32_t j = 0; j < kPackTile; j++) {
        uint32_t w, l, e, lo;
        uint16_t m16;
        pack_pos(j, &w, &l, &e);
        const unsigned char *g = data + (size_t)w * kPackGroupBytes;
        memcpy(&lo, g + pack_off_lo(l, e), 4);
        memcpy(&m16, g + pack_off_mid(l, e), 2);
        const uint32_t t = (uint32_t)g[pack_off_hi(l, e)] << 16 | m16;
        if (pack_is_exception(t)) out[j] = lo < kPackCap ? exc[lo] : 0ull;
        else out[j] = pack_decode(lo, t, pack_exp_shift(base));
    }
}
#endif

}  // namespace lam
