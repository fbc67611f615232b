// Host-only check of the pyramid addressing helpers of csrc/ecorr_device.h (tests/test_layout_host.py
// compiles and runs it; no HIP API is touched).  For every case -- a level format and size, a first
// query row R0 and a row count nq -- and every query row R0 + g, g < nq, and pixel (y, x):
//   slab first float + row term + cell term == pix_off(R, y, x, ...) == the format's nested array index
// and the slab's byte span covers exactly the 64-row groups (interleaved) or rows (tiled, compact)
// touched; the cell-existence predicate agrees with by < nby && bx < nbx; the tile-line base agrees
// with tiled_off() at the tile's first cell.  Prints the number of comparisons; exit status 1 and
// the first mismatch on failure.
#include <cstdio>
#include <cstdlib>

#include "ecorr_device.h"

using namespace ecorr;

static long long n_cmp = 0;

#define CHECK(cond, ...)                  \
    do {                                  \
        ++n_cmp;                          \
        if (!(cond)) {                    \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");            \
            std::exit(1);                 \
        }                                 \
    } while (0)

// lv: the level (its number picks the block shape when interleaved); ntx as the kernels get it
static void run_case(const char* name, int lv, int h, int w, int ntx, int64_t sz) {
    const int64_t R0s[] = {0, 37, 64, 100};
    const int nqs[] = {1, 27, 64, 200};
    const bool ilv = ntx < 0;
    const int sy = ilv ? ilv_sy(lv) : 0, sx = ilv ? ilv_sx(lv) : 0;
    const int nbx = -ntx, nby = ilv ? (h + (1 << sy) - 1) >> sy : 0;
    for (int64_t R0 : R0s)
        for (int nq : nqs) {
            const int64_t first = slab_first(ilv, R0, sz), bytes = slab_bytes(ilv, R0, nq, sz), g0 = slab_g0(R0);
            CHECK(bytes % 4 == 0 && bytes > 0, "%s R0 %lld nq %d: span %lld", name, (long long)R0, nq, (long long)bytes);
            // exactly the touched groups / rows
            const int64_t last = R0 + nq - 1;
            const int64_t want_first = ilv ? (R0 / kGroup) * kGroup * sz : R0 * sz;
            const int64_t want_floats = ilv ? (last / kGroup - R0 / kGroup + 1) * kGroup * sz : nq * sz;
            CHECK(first == want_first && bytes == 4 * want_floats, "%s R0 %lld nq %d: slab [%lld, +%lld B)", name,
                  (long long)R0, nq, (long long)first, (long long)bytes);
            for (int g = 0; g < nq; ++g) {
                const int64_t R = R0 + g;
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        const int64_t rel = ilv ? ilv_row_off(R, g0, lv, sz) + ilv_cell_off(y, x, lv, nbx)
                                                : g * sz + level_off(y, x, ntx, w);
                        const int64_t full = pix_off(R, y, x, lv, ntx, w, sz);
                        // the format written out as nested array indices, independently of the helpers
                        int64_t want;
                        if (ilv) {   // [group][block][row][bh][bw]
                            const int bh = 1 << sy, bw = 1 << sx;
                            want = (((R / kGroup) * ((int64_t)nby * nbx) + (y / bh) * nbx + x / bw) * kGroup + R % kGroup) *
                                       (bh * bw) + (y % bh) * bw + x % bw;
                        } else if (ntx > 0) {   // [row][tile row][tile col][4][8]
                            want = R * sz + ((y / 4) * ntx + x / 8) * 32 + (y % 4) * 8 + x % 8;
                        } else {
                            want = R * sz + y * w + x;
                        }
                        CHECK(full == want, "%s: row %lld pixel (%d, %d): pix_off %lld, the format says %lld", name,
                              (long long)R, y, x, (long long)full, (long long)want);
                        CHECK(first + rel == full, "%s R0 %lld nq %d: row %lld pixel (%d, %d): slab %lld + %lld != %lld",
                              name, (long long)R0, nq, (long long)R, y, x, (long long)first, (long long)rel,
                              (long long)full);
                        CHECK(rel >= 0 && rel * 4 + 4 <= bytes, "%s: row %lld pixel (%d, %d) outside the span", name,
                              (long long)R, y, x);
                    }
            }
            // the last row's last stored cell is the span's last float; the next float lies outside
            int64_t last_cell;
            if (ilv)   // the last block's last cell (a padding cell when the level's sides are odd)
                last_cell = ilv_row_off(last, g0, lv, sz) +
                            ilv_cell_off((nby << sy) - 1, (nbx << sx) - 1, lv, nbx);
            else
                last_cell = (nq - 1) * sz + sz - 1;
            const int64_t group_end = ilv ? ((last / kGroup - g0) + 1) * kGroup * sz - 1 : last_cell;
            CHECK(last_cell * 4 + 4 <= bytes && group_end * 4 + 4 == bytes,
                  "%s R0 %lld nq %d: last cell %lld, span %lld B", name, (long long)R0, nq, (long long)last_cell,
                  (long long)bytes);
            if (ilv && (last & (kGroup - 1)) == kGroup - 1)   // a full last group ends on its last row's last cell
                CHECK(last_cell == group_end, "%s R0 %lld nq %d: the last group's end", name, (long long)R0, nq);
        }
    // the cell-existence predicate, also past the level
    if (ilv)
        for (int y = 0; y < h + 9; ++y)
            for (int x = 0; x < w + 9; ++x)
                CHECK(ilv_cell_in(y, x, lv, nby, nbx) == ((y >> sy) < nby && (x >> sx) < nbx), "%s: cell_in (%d, %d)",
                      name, y, x);
    // the tile-line base
    if (ntx > 0)
        for (int tr = 0; tr < pad_h(h) / kTileH; ++tr)
            for (int tc = 0; tc < ntx; ++tc)
                CHECK(tile_base(tr, tc, ntx) == tiled_off(tr * kTileH, tc * kTileW, ntx), "%s: tile (%d, %d)", name, tr,
                      tc);
}

int main() {
    for (int lv = 1; lv <= 3; ++lv) {   // interleaved, 7 x 11
        CHECK(level_ilv(lv), "level %d is interleaved", lv);
        const int h = 7, w = 11, bh = 1 << ilv_sy(lv), bw = 1 << ilv_sx(lv);
        const int nby = (h + bh - 1) / bh, nbx = (w + bw - 1) / bw;
        CHECK(ilv_bsz(lv) == bh * bw, "block floats of level %d", lv);
        char name[32];
        std::snprintf(name, sizeof name, "ilv%d 7x11", lv);
        run_case(name, lv, h, w, -nbx, (int64_t)nby * nbx * bh * bw);
    }
    CHECK(!level_ilv(0) && !level_ilv(4), "levels 0 and 4 are not interleaved");
    run_case("tiled 7x11", 0, 7, 11, pad_w(11) / kTileW, (int64_t)pad_h(7) * pad_w(11));   // ntx = 2
    CHECK(level_compact(4, 3, 5) && !level_compact(0, 3, 5), "3 x 5 is compact at level 4 only");
    run_case("compact 3x5", 4, 3, 5, 0, 3 * 5);
    std::printf("%lld comparisons ok\n", n_cmp);
    return 0;
}
