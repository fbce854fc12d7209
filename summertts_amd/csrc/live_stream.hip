// live_stream.hip -- the one kernel of an open stream (engine.hip stream_admit, live_stream.hpp): the latents of an admission leave the
// frame arena, which the next run lays out again, for the stream's persistent pool.
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

}  // namespace sts
