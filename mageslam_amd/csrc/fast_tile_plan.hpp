// Load plan of the FAST image tile (load_tile in orb.hip): which frame bytes each thread loads,
// how wide, and where every loaded byte lands in the LW x LH tile.  Shared by the kernels and by
// the host debug entry point mage_debug_fast_tile_plan, which runs the same arithmetic on the CPU.
//
// The tile window is LW = 136 columns x LH = 38 rows starting at frame pixel (gx0, gy0); gx0 is
// 8 (mod 120), so with 8-byte aligned rows every 16-byte chunk of a window row starts 8-byte
// aligned in the frame.  A window row is 9 chunks: chunk c < 8 is window columns [16 c, 16 c + 16),
// chunk 8 is columns [128, 136).  Pixels outside the frame are reflect-101 images of pixels inside
// it; the plan covers every tile that needs at most one reflection per axis (border_ok).
#pragma once

#include <hip/hip_runtime.h>

namespace mage {
namespace tileplan {

constexpr int kLW = 136, kLH = 38;  // orb.hip asserts these against LW / LH
constexpr int kChunks = 9;

// reflect-101 for a coordinate at most one bounce outside [0, n)
__host__ __device__ constexpr int mirror1(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }
static_assert(mirror1(-1, 1280) == 1 && mirror1(-8, 1280) == 8 && mirror1(0, 1280) == 0, "left mirror");
static_assert(mirror1(1279, 1280) == 1279 && mirror1(1280, 1280) == 1278 && mirror1(1327, 1280) == 1231, "right mirror");
static_assert(mirror1(297, 297) == 295 && mirror1(303, 297) == 289 && mirror1(65, 65) == 63 && mirror1(127, 65) == 1,
              "right mirror, odd widths");
static_assert(mirror1(-4, 5) == 4 && mirror1(37, 20) == 1, "rows");

// every window coordinate [g0, g0 + len) is inside the frame after at most one reflection
__host__ __device__ constexpr bool single_bounce(int g0, int len, int n)
{
    return -g0 <= n - 1 && g0 + len - 1 <= 2 * n - 2;
}
// The wide border path stages this tile (the interior path is the case without reflection).  The
// right-edge chunk loads the row's last 16 bytes, so a row holds at least 16.
__host__ __device__ constexpr bool border_ok(int w, int h, int gx0, int gy0)
{
    return w >= 16 && single_bounce(gx0, kLW, w) && single_bounce(gy0, kLH, h);
}
static_assert(border_ok(1280, 720, -8, -4) && border_ok(1280, 720, 1192, 686) && border_ok(128, 30, -8, -4), "frames");
static_assert(!border_ok(40, 40, -8, -4) && !border_ok(16, 16, -8, -4) && !border_ok(124, 100, 112, -4), "second bounce");

enum ChunkKind {
    CHUNK_FULL = 0,   // wholly inside the frame: 16 bytes at x (chunk 8: the upper half of them)
    CHUNK_MIRROR,     // wholly right of the frame: `len` bytes at x, byte-reversed
    CHUNK_LEFT,       // chunk 0 of the left tile column (frame columns -8..7): the row's first 16 bytes;
                      // columns 8..15 are frame bytes 0..7 and columns 0..7 are frame bytes 8..1
    CHUNK_STRADDLE,   // the frame's right edge lies inside the chunk: n columns are frame bytes, the
                      // rest their mirror images; all of them are among the row's last 16 bytes (x = w - 16)
};

struct ChunkPlan {
    int kind;
    int x;    // frame column of the first byte loaded
    int len;  // chunk length: 16, or 8 for chunk 8
    int n;    // CHUNK_STRADDLE: chunk columns inside the frame, 1 .. len - 1
};

// Plan of chunk c for a tile window starting at frame column gx0 (any row: rows only move the
// load's row).  Requires border_ok.
__host__ __device__ constexpr ChunkPlan chunk_plan(int w, int gx0, int c)
{
    const int a = 16 * c, len = c < 8 ? 16 : 8;
    const int X = gx0 + a;  // frame column of the chunk's first byte
    if (X < 0) return {CHUNK_LEFT, 0, len, 0};  // gx0 = -8, c = 0
    if (X + len <= w) return {CHUNK_FULL, c < 8 ? X : X - 8, len, 0};
    if (X >= w) return {CHUNK_MIRROR, 2 * w - 2 - (X + len - 1), len, 0};
    return {CHUNK_STRADDLE, w - 16, len, w - X};
}

// Bytes one load moves: 16, except a mirrored chunk 8 (8: sixteen could pass the row's end).
__host__ __device__ constexpr int load_bytes(const ChunkPlan& cp) { return cp.kind == CHUNK_MIRROR ? cp.len : 16; }
// CHUNK_FULL / CHUNK_MIRROR / CHUNK_LEFT: the loaded byte that lands at chunk column pos
__host__ __device__ constexpr int chunk_byte(const ChunkPlan& cp, int pos)
{
    return cp.kind == CHUNK_FULL ? (cp.len == 16 ? pos : pos + 8)
           : cp.kind == CHUNK_MIRROR ? cp.len - 1 - pos
                                     : (pos < 8 ? 8 - pos : pos - 8);
}
// CHUNK_STRADDLE: byte k of the 16 loaded (frame column w - 16 + k) lands at chunk column
// straddle_direct (as itself) and at chunk column straddle_mirror (as the image of a column right
// of the frame); a value outside [0, len) means it does not land that way.
__host__ __device__ constexpr int straddle_direct(int n, int k) { return k - 16 + n; }
__host__ __device__ constexpr int straddle_mirror(int n, int k) { return k == 15 ? -1 : 14 + n - k; }
// w = 1280, last tile column (gx0 = 1192): chunk 4 = columns 1256..1271, chunk 5 = 1272..1287, n = 8
static_assert(chunk_plan(1280, 1192, 4).kind == CHUNK_FULL && chunk_plan(1280, 1192, 4).x == 1256, "1280: chunk 4");
static_assert(chunk_plan(1280, 1192, 5).kind == CHUNK_STRADDLE && chunk_plan(1280, 1192, 5).n == 8 &&
                  chunk_plan(1280, 1192, 5).x == 1264, "1280: chunk 5");
static_assert(chunk_plan(1280, 1192, 6).kind == CHUNK_MIRROR && chunk_plan(1280, 1192, 6).x == mirror1(1192 + 111, 1280),
              "1280: chunk 6 is columns 1288..1303, images of 1270..1255");
static_assert(chunk_plan(297, 232, 4).kind == CHUNK_STRADDLE && chunk_plan(297, 232, 4).n == 1 &&
                  chunk_plan(297, 232, 4).x == 281, "297: column 296 is chunk 4's first");
// n = 1: frame column 296 (k = 15) is chunk column 0; column 295 (k = 14) is chunk column 1 = image of 297
static_assert(straddle_direct(1, 15) == 0 && straddle_mirror(1, 14) == 1 && straddle_mirror(1, 0) == 15, "straddle");
static_assert(chunk_plan(1280, -8, 0).kind == CHUNK_LEFT && chunk_plan(1280, 112, 8).kind == CHUNK_FULL &&
                  chunk_plan(1280, 112, 8).x == 232, "left chunk; chunk 8 loads columns 120..135");

}  // namespace tileplan
}  // namespace mage
