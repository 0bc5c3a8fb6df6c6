// The batched product's traversal of the packed image (csrc/lam_host_pack.h, pack_many_pos) on the host, under
// -fsanitize=address,undefined (tests/test_pack_many_cpu.py builds and runs this program).
// For K = 1, 2, 4 columns, a list of row lengths and EVERY starting tile of the rotation, the schedule of multi_gemv_packed_kernel
// is walked -- batch tiles of 4096 / K columns in rotated order, ceil(cols / 512) steps each, 4 waves x 64 lanes x 2 columns a step --
// and held against multi_gemv_kernel's own index arithmetic, restated here:
//   * every column below ncols is produced exactly once, and nothing at or behind the end of the last step is produced at all;
//   * every lane's sequence of (unit, wave group, lane, element) is pack_pos of the plain kernel's sequence of global columns;
//   * the element read through the mapping from pack_tile's image decodes to the row's own bits (unpack_tile's element decode);
//   * the columns of the steps that run behind a ragged end decode to +0.0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lam_host_pack.h"

using namespace lam;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// one row of ncols elements: seven binades of ordinary values, a few dozen exceptions of every kind per 4096 columns
static std::vector<uint64_t> make_row(uint32_t ncols)
{
    static const uint64_t special[] = {0x0ull, 0x8000000000000000ull, 0x1ull, 0x800fffffffffffffull, 0x7ff0000000000000ull,
                                       0xfff0000000000000ull, 0x7ff4000000abcdefull, 0x7fe0000000000001ull, 0x0010000000000000ull};
    std::vector<uint64_t> row(ncols);
    for (uint32_t j = 0; j < ncols; j++) {
        const uint64_t exp = 1000 + rnd() % kPackWindow;
        row[j] = (rnd() & 0x800fffffffffffffull) | exp << 52;
        if (rnd() % 100 == 0) row[j] = special[rnd() % (sizeof special / sizeof special[0])];
    }
    row[ncols - 1] = 0x8000000000000000ull;          // an exception in the last column: the last step of a ragged tile
    return row;
}

// the element (group, lane, e) of a unit's image, as unpack_tile decodes it
static uint64_t read_element(const unsigned char *data, const uint64_t *exc, uint32_t header, uint32_t group, uint32_t lane, uint32_t e)
{
    const unsigned char *g = data + (size_t)group * kPackGroupBytes;
    uint32_t lo;
    uint16_t m16;
    memcpy(&lo, g + pack_off_lo(lane, e), 4);
    memcpy(&m16, g + pack_off_mid(lane, e), 2);
    const uint32_t t = (uint32_t)g[pack_off_hi(lane, e)] << 16 | m16;
    if (pack_is_exception(t)) return lo < kPackCap ? exc[lo] : 0ull;
    return pack_decode(lo, t, pack_exp_shift(pack_header_base(header)));
}

#define CHECK(cond, ...)                                                                                                               \
    do {                                                                                                                               \
        if (!(cond)) {                                                                                                                 \
            printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);                                                                \
            printf(__VA_ARGS__);                                                                                                       \
            printf("\n");                                                                                                              \
            return 1;                                                                                                                  \
        }                                                                                                                              \
    } while (0)

static int walk(uint32_t K, uint32_t ncols)
{
    const uint32_t tile = kPackTile / K;                                  // multi_tile<double, double, K, 4>()
    const uint32_t ntiles = (ncols + tile - 1) / tile;
    const uint32_t nunits = (ncols + kPackTile - 1) / kPackTile;
    const uint32_t super = 512, waves = 4;

    const std::vector<uint64_t> row = make_row(ncols);
    std::vector<unsigned char> data((size_t)nunits * kPackTileBytes);
    std::vector<uint64_t> exc((size_t)nunits * kPackCap), back(kPackTile);
    std::vector<uint32_t> header(nunits);
    for (uint32_t u = 0; u < nunits; u++) {
        const uint32_t c0 = u * kPackTile, cols = ncols - c0 < kPackTile ? ncols - c0 : kPackTile;
        const uint32_t count = pack_tile(row.data() + c0, cols, data.data() + (size_t)u * kPackTileBytes, exc.data() + (size_t)u * kPackCap, &header[u]);
        CHECK(count <= kPackCap, "K %u ncols %u unit %u: %u exceptions", K, ncols, u, count);
        unpack_tile(data.data() + (size_t)u * kPackTileBytes, exc.data() + (size_t)u * kPackCap, header[u], back.data());
        for (uint32_t j = 0; j < kPackTile; j++) CHECK(back[j] == (j < cols ? row[c0 + j] : 0ull), "unit %u column %u", u, j);
    }

    std::vector<uint32_t> seen(ncols);
    for (uint32_t tt0 = 0; tt0 < ntiles; tt0++) {
        std::fill(seen.begin(), seen.end(), 0u);
        uint64_t behind = 0;
        uint32_t tt = tt0;
        for (uint32_t t = 0; t < ntiles; t++) {
            // multi_gemv_kernel: c0, cols, nsteps of batch tile tt; col = s * SUPER + wave * 128 + lane * 2; elements col, col + 1
            const uint64_t c0 = (uint64_t)tt * tile;
            const uint32_t cols = ncols - c0 < tile ? (uint32_t)(ncols - c0) : tile;
            const uint32_t nsteps = (cols + super - 1) / super;
            for (uint32_t s = 0; s < nsteps; s++)
                for (uint32_t w = 0; w < waves; w++) {
                    uint32_t unit, group, pair;
                    pack_many_pos(K, tt, s, w, &unit, &group, &pair);
                    CHECK(unit < nunits && group < kPackGroups && pair < 4, "K %u ncols %u tile %u step %u wave %u: unit %u group %u pair %u", K,
                          ncols, tt, s, w, unit, group, pair);
                    CHECK(group == w || group == w + 4, "wave %u reads group %u", w, group);
                    for (uint32_t l = 0; l < 64; l++)
                        for (uint32_t i = 0; i < 2; i++) {
                            const uint64_t plain = c0 + (uint64_t)s * super + w * 128 + 2 * l + i;      // the plain kernel's global column
                            uint32_t pw, pl, pe;
                            pack_pos((uint32_t)(plain % kPackTile), &pw, &pl, &pe);
                            CHECK(plain / kPackTile == unit && pw == group && pl == l && pe == 2 * pair + i,
                                  "K %u ncols %u start %u tile %u step %u wave %u lane %u i %u: column %llu is (%llu, %u, %u, %u), the mapping "
                                  "gives (%u, %u, %u, %u)", K, ncols, tt0, tt, s, w, l, i, (unsigned long long)plain,
                                  (unsigned long long)(plain / kPackTile), pw, pl, pe, unit, group, l, 2 * pair + i);
                            const uint64_t got = read_element(data.data() + (size_t)unit * kPackTileBytes, exc.data() + (size_t)unit * kPackCap,
                                                              header[unit], group, l, 2 * pair + i);
                            if (plain < ncols) {
                                seen[plain]++;
                                CHECK(got == row[plain], "K %u ncols %u column %llu: %016llx != %016llx", K, ncols, (unsigned long long)plain,
                                      (unsigned long long)got, (unsigned long long)row[plain]);
                            } else {
                                behind++;
                                CHECK(plain < c0 + (uint64_t)nsteps * super, "column %llu behind the last step", (unsigned long long)plain);
                                CHECK(got == 0ull, "K %u ncols %u column %llu behind the end decodes to %016llx, not +0.0", K, ncols,
                                      (unsigned long long)plain, (unsigned long long)got);
                            }
                        }
                }
            tt = tt + 1 == ntiles ? 0 : tt + 1;
        }
        for (uint32_t j = 0; j < ncols; j++) CHECK(seen[j] == 1, "K %u ncols %u start %u: column %u produced %u times", K, ncols, tt0, j, seen[j]);
        CHECK(behind == (uint64_t)(ncols + super - 1) / super * super - ncols, "K %u ncols %u start %u: %llu columns behind the end", K, ncols, tt0,
              (unsigned long long)behind);
    }
    return 0;
}

int main()
{
    const uint32_t sizes[] = {2, 384, 1548, 4096, 4098, 9002, 12288};
    uint64_t walks = 0;
    for (uint32_t K : {1u, 2u, 4u})
        for (uint32_t ncols : sizes) {
            if (walk(K, ncols)) return 1;
            walks += (ncols + kPackTile / K - 1) / (kPackTile / K);
        }
    printf("%llu walks\nok pack many\n", (unsigned long long)walks);
    return 0;
}
