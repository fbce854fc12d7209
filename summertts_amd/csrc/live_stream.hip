// live_stream.hip -- the two kernels of an open stream (engine.hip stream_admit, live_stream.hpp): the latents of an admission leave the
// frame arena, which the next run lays out again, for the stream's persistent pool (adopt_z); and, in a planned stream, so do the tables a
// newcomer carries until it retires -- its conditioning vector, its gain plan's phoneme table and slot words (adopt_tables).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace sts {

// One workgroup per (tile of AZ_COLS columns, tile of rows, segment).  A row of a tile is `units` accesses: where source and destination
// columns are co-aligned (equal offsets mod 4 floats, both leading dimensions and both bases whole quads) the scalar columns up to the
// first 16-byte boundary, then float4 quads, then the scalar rest; otherwise every column by itself.  The lanes run over (row, unit) of
// the tile flattened, and a tile takes more rows the fewer columns it has -- a 1-frame segment is 256 rows of one column per workgroup,
// a 700-frame one 16 rows of 64 quads -- so that both fill their waves.  Every access is bounded by the segment: nothing outside
// [dst_off, dst_off + len) of a row is written, nothing outside [src_off, src_off + len) read.
constexpr int AZ_THREADS = 256, AZ_COLS = 256, AZ_ROWS = 16;
__global__ __launch_bounds__(AZ_THREADS) void adopt_z_kernel(const float* __restrict__ src, long long ld_src, float* __restrict__ dst,
                                                             long long ld_dst, int C, const long long* __restrict__ tab, int B) {
    const int b = blockIdx.z;
    const int len = ((const int*)(tab + 2 * (size_t)B))[b];
    const int c0 = blockIdx.x * AZ_COLS;
    if (c0 >= len) return;
    const int n = min(len - c0, AZ_COLS);
    const int rows = n >= 64 ? AZ_ROWS : (n >= 16 ? 4 * AZ_ROWS : 16 * AZ_ROWS);
    const int r0 = blockIdx.y * rows;
    if (r0 >= C) return;
    const int nr = min(rows, C - r0);
    const long long s0 = tab[b] + c0, d0 = tab[B + b] + c0;
    const bool vec = ((ld_src | ld_dst) & 3) == 0 && ((s0 ^ d0) & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int head = vec ? min(n, (int)((4 - (s0 & 3)) & 3)) : n;
    const int quads = (n - head) >> 2;          // (not co-aligned: head == n, none)
    const int tail = n - head - 4 * quads;
    const int units = head + quads + tail;
    for (int i = threadIdx.x; i < nr * units; i += AZ_THREADS) {
        const int r = i / units, u = i - r * units;
        const float* s = src + (long long)(r0 + r) * ld_src + s0;
        float* d = dst + (long long)(r0 + r) * ld_dst + d0;
        if (u >= head && u < head + quads) {
            const int c = head + 4 * (u - head);
            *(float4*)(d + c) = *(const float4*)(s + c);
        } else {
            const int c = u < head ? u : u + 3 * quads;         // (the tail starts at column head + 4 quads = unit head + quads)
            d[c] = s[c];
        }
    }
}

void adopt_z(const float* src, long long ld_src, float* dst, long long ld_dst, int C, const long long* tab, int B, int max_len, hipStream_t st) {
    if (B <= 0 || C <= 0 || max_len <= 0) return;
    hipLaunchKernelGGL(adopt_z_kernel, dim3((unsigned)((max_len + AZ_COLS - 1) / AZ_COLS), (unsigned)((C + AZ_ROWS - 1) / AZ_ROWS), (unsigned)B),
                       dim3(AZ_THREADS), 0, st, src, ld_src, dst, ld_dst, C, tab, B);
}

// The tables of an admission into a planned stream (live_stream.hpp), one launch for everything a newcomer carries besides z.  One
// workgroup per (tile of AT_THREADS units, newcomer); the units of newcomer b are flattened --
//   [0, gin)              channel c of its conditioning vector: g[c][b] -> gpool[c][slot]
//   [gin, gin + n)        its inclusive cumulative frame counts: cum[toff + i] -> pool row 0, column poff + i
//   [gin + n, gin + 2n)   its fixed-point gains: q[toff + i] -> pool row 1, column poff + i
//   [gin + 2n, + 3)       its slot words {off, n, h}[slot]: {poff, n, h}, or the shared neutral row {cap, 1, 0} when it carries no plan
// -- so a 1-phoneme utterance (gin + 5 units) and a 700-phoneme one (gin + 1403) both fill their waves but for the last one.  Consecutive
// lanes of a phoneme section read and write consecutive words; source and destination offsets are arbitrary, so the words move one per
// lane (whole 64-lane rows of 256 bytes either way) and not in quads.  The vector's column is strided on both sides by its nature: gin
// words in all.  Every store is a plain vector store of a loaded value; nothing outside column `slot` of gpool and the words, and columns
// [poff, poff + n) of the pool, is written.  A row of the table with slot < 0 (an utterance without frames) moves nothing.
constexpr int AT_THREADS = 256;
__global__ __launch_bounds__(AT_THREADS) void adopt_tables_kernel(AdoptTablesArgs a) {
    const int b = blockIdx.y;
    const int* const row = a.tab + 5 * (size_t)b;
    const int slot = row[0], toff = row[1], n = row[2], poff = row[3], h = row[4];
    if (slot < 0) return;
    const int gin = a.gpool ? a.gin : 0;
    const int units = gin + 2 * n + 3;
    const int u = blockIdx.x * AT_THREADS + threadIdx.x;
    if (u >= units) return;
    if (u < gin) {
        a.gpool[(size_t)u * a.max_live + slot] = a.g[(size_t)u * a.B + b];
    } else if (u < gin + n) {
        const int i = u - gin;
        a.pool[(size_t)poff + i] = a.cum[(size_t)toff + i];
    } else if (u < gin + 2 * n) {
        const int i = u - gin - n;
        a.pool[(size_t)a.ld_pool + poff + i] = a.q[(size_t)toff + i];
    } else {
        const int w = u - gin - 2 * n;      // 0: off, 1: n, 2: h
        const int v = n > 0 ? (w == 0 ? poff : w == 1 ? n : h) : (w == 0 ? a.neutral : w == 1 ? 1 : 0);
        a.swords[(size_t)w * a.max_live + slot] = v;
    }
}

void adopt_tables(const AdoptTablesArgs& a, int max_n, hipStream_t st) {
    if (a.B <= 0) return;
    const int units = (a.gpool ? a.gin : 0) + 2 * max_n + 3;
    hipLaunchKernelGGL(adopt_tables_kernel, dim3((unsigned)((units + AT_THREADS - 1) / AT_THREADS), (unsigned)a.B), dim3(AT_THREADS), 0, st, a);
}

}  // namespace sts
