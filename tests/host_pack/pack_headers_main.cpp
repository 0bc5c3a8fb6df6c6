// csrc/lam_host_pack.h -- the very header the product build includes -- as a stand-alone program for
// g++ -fsanitize=address,undefined (tests/test_packed_model_cpu.py builds and runs it; it is never loaded into another process).
// usage: pack_headers IN OUT
// IN:  two uint64 (rows, n), then rows x n fp64 values as raw bits, row by row.
// OUT: per (row, 4096-column tile), row-major, two uint32: the header pack_tile gives the tile, and a flag -- 1: unpack_tile gives
//      back the tile's bits (the padding as +0.0), 0: it does not, 2: more than kPackCap exceptions, nothing to decode.
// A row is held as the device holds it: n rounded up to the 16-byte vector, the pad column zero, and the last tile is handed to
// pack_tile with exactly the columns it has.  Every buffer is allocated at exactly its stated size, so a read or write past it is
// a heap overflow the sanitizer reports.  Prints "ok headers" at the end.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lam_host_pack.h"

using namespace lam;

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *in = std::fopen(argv[1], "rb");
    FILE *out = std::fopen(argv[2], "wb");
    uint64_t dims[2] = {0, 0};
    if (!in || !out || std::fread(dims, 8, 2, in) != 2 || dims[1] == 0) { std::fprintf(stderr, "cannot open the files or read the sizes\n"); return 2; }
    const uint64_t rows = dims[0], n = dims[1];
    const uint64_t ncols = (n + 1) / 2 * 2;
    const uint64_t ntiles = (ncols + kPackTile - 1) / kPackTile;
    std::vector<uint64_t> row(ncols), exc(kPackCap), back(kPackTile);
    std::vector<unsigned char> data(kPackTileBytes);
    for (uint64_t i = 0; i < rows; i++) {
        if (std::fread(row.data(), 8, n, in) != n) { std::fprintf(stderr, "row %llu is short\n", (unsigned long long)i); return 2; }
        for (uint64_t j = n; j < ncols; j++) row[j] = 0ull;
        for (uint64_t t = 0; t < ntiles; t++) {
            const uint64_t c0 = t * kPackTile;
            const uint32_t cols = (uint32_t)(ncols - c0 < kPackTile ? ncols - c0 : kPackTile);
            // the tile's own copy, exactly `cols` long: pack_tile may not look behind it
            const std::vector<uint64_t> tile(row.begin() + (long)c0, row.begin() + (long)(c0 + cols));
            uint32_t rec[2] = {0, 1};
            const uint32_t count = pack_tile(tile.data(), cols, data.data(), exc.data(), &rec[0]);
            if (count > kPackCap) rec[1] = 2;
            else {
                unpack_tile(data.data(), exc.data(), rec[0], back.data());
                for (uint32_t j = 0; j < kPackTile; j++)
                    if (back[j] != (j < cols ? tile[j] : 0ull)) rec[1] = 0;
            }
            if (std::fwrite(rec, 4, 2, out) != 2) { std::fprintf(stderr, "write failed\n"); return 2; }
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("ok headers\n");
    return 0;
}
