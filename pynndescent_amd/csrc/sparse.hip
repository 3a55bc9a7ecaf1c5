// sparse.hip -- sparse input: the rows of a CSR matrix that is on the device, written dense where the device-array path expects
// its float32 rows (NNDescent(scipy.sparse matrix), sparse queries, sparse update rows).  One kernel, no handle: the rows are made
// before any builder or searcher sees them, and from there on the index is a device-resident index.
//
// The work is cut by FLAT position, not by row: rows of a contiguous (n, d) buffer are 16-byte aligned only when d % 4 == 0, the
// flat buffer always is (up to its first few floats).  The flat position row * d + col increases along the CSR arrays of a
// canonical matrix (columns ascending within a row, no duplicates), so a tile of the flat buffer owns ONE contiguous run of
// stored entries.  A block takes a contiguous chunk of tiles, so the end of one tile's run is the start of the next one's; the
// end is found by a 64-ary search in the boundary row (one probe per lane, one round trip per 6 bits of the row's length).  The
// run is scattered into a zeroed LDS image of the tile -- an entry finds its row by a binary search in the tile's slice of
// indptr, staged in LDS -- and the image is streamed out in 16-byte stores.  Every element of dst is written exactly once; dst is
// never read, nothing is atomic, and there is no memset pass under the scatter.  A tile that owns no stored entry -- most tiles
// when d is in the tens of thousands -- stores zeros without touching the LDS.
#include <stdint.h>
#include <stdio.h>

#include "common.h"

#define CSR_TILE 4096     // floats per tile: 16 KiB of LDS, 4 x 16 bytes per thread and tile
#define CSR_THREADS 256
#define CSR_ROWS_CAP 1032  // the staged slice of indptr: a tile touches at most CSR_TILE / d + 2 rows, 1026 for d >= 4
#define CSR_AHEAD 4        // entries per thread loaded ahead of the image's zeroing: a run of up to 1024 entries (density 0.25)

// The first position in [s, e) of `indices` whose column is at least `col` (e: there is none), by every lane of the wave with the
// same arguments: lane l probes the last element of the l-th of 64 equal segments, the ballot names the segment that holds the
// answer, and the search goes on inside it.  One round for up to 64 entries, two for up to 4096.
template <typename IX>
__device__ __forceinline__ int64_t csr_wave_lower_bound(const IX *__restrict__ indices, int64_t s, int64_t e, int64_t col) {
    const int lane = nnd_lane();
    while (s < e) {
        const int64_t step = (e - s + 63) >> 6;
        const int64_t p = s + (int64_t)(lane + 1) * step - 1;
        const bool below = p < e && (int64_t)indices[p] < col;
        s += (int64_t)__popcll(__ballot(below)) * step;  // the probes are ascending: the lanes below `col` are the leading ones
        if (step == 1) break;                            // (every element was probed)
        e = s + step - 1 < e ? s + step - 1 : e;         // the segment's last element is at least `col`, or lies behind e
    }
    return s < e ? s : e;
}

// the first stored entry at or behind the flat position `pos` (<= n * d)
template <typename IP, typename IX>
__device__ __forceinline__ int64_t csr_first_at(const IP *__restrict__ indptr, const IX *__restrict__ indices, int64_t pos, int64_t n, int d) {
    const int64_t row = pos / d;
    if (row >= n) return (int64_t)indptr[n];
    return csr_wave_lower_bound(indices, (int64_t)indptr[row], (int64_t)indptr[row + 1], pos - row * d);
}

// `shift` = floats between the last 16-byte boundary at or before dst and dst (0 .. 3): tiles are cut at p = flat + shift, so
// that p % 4 == 0 is a 16-byte aligned address and a tile's LDS image and its piece of dst share their 16-byte chunks.
// Block b takes the tiles [b * per_block, (b + 1) * per_block).
template <typename IP, typename IX>
__global__ __launch_bounds__(CSR_THREADS) void k_csr_rows(const IP *__restrict__ indptr, const IX *__restrict__ indices,
                                                          const float *__restrict__ values, int64_t n, int d, float *__restrict__ dst,
                                                          int shift, int64_t tiles, int64_t per_block) {
    __shared__ float4 image4[CSR_TILE / 4];
    __shared__ int32_t rowptr[CSR_ROWS_CAP];
    float *image = (float *)image4;
    const int tid = (int)threadIdx.x;
    const int64_t total = n * (int64_t)d;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int64_t t_first = (int64_t)blockIdx.x * per_block;
    const int64_t t_end = t_first + per_block < tiles ? t_first + per_block : tiles;
    if (t_first >= t_end) return;
    // a tile's flat positions are [tile_lo(t), tile_lo(t + 1)), cut off at the buffer's end
    auto tile_lo = [&](int64_t t) {
        const int64_t at = t * CSR_TILE > shift ? t * CSR_TILE - shift : 0;
        return at < total ? at : total;
    };
    // the chunk's first stored entry; afterwards each tile's run [e_lo, e_hi) starts where the last one ended, and its end is
    // searched one tile ahead, under the loads of the tile at hand
    int64_t e_lo = csr_first_at(indptr, indices, tile_lo(t_first), n, d);
    int64_t e_hi = csr_first_at(indptr, indices, tile_lo(t_first + 1), n, d);
    for (int64_t t = t_first; t < t_end; t++) {
        const int64_t p0 = t * CSR_TILE;
        const int64_t lo = tile_lo(t), hi = tile_lo(t + 1);
        const int64_t run = e_hi - e_lo;
        const bool stored = run > 0;  // (the same for every thread of the block)
        int64_t col_ahead[CSR_AHEAD];
        float val_ahead[CSR_AHEAD];
        if (stored) {
#pragma unroll
            for (int j = 0; j < CSR_AHEAD; j++) {
                const int64_t i = tid + j * CSR_THREADS;
                col_ahead[j] = i < run ? (int64_t)indices[e_lo + i] : -1;
                val_ahead[j] = i < run ? values[e_lo + i] : 0.0f;
            }
        }
        const int64_t e_next = t + 1 < t_end ? csr_first_at(indptr, indices, tile_lo(t + 2), n, d) : e_hi;
        if (stored) {
            const int64_t row_lo = lo / d, n_rows = (hi - 1) / d - row_lo + 1;
            const bool staged = n_rows + 1 <= CSR_ROWS_CAP;
            for (int i = tid; i < CSR_TILE / 4; i += CSR_THREADS) image4[i] = zero4;
            if (staged) {  // rowptr[r] = where row row_lo + r starts within the run, clipped to it: rowptr[0] = 0, rowptr[n_rows] = run
                const int64_t cap = run < (1 << 30) ? run : (1 << 30);
                for (int i = tid; i <= (int)n_rows; i += CSR_THREADS) {
                    const int64_t at = (int64_t)indptr[row_lo + i] - e_lo;
                    rowptr[i] = (int32_t)(at < 0 ? 0 : (at > cap ? cap : at));
                }
            }
            __syncthreads();
            auto place = [&](int64_t i, int64_t col, float value) {
                int64_t r = 0, h = n_rows - 1;  // the entry's row: the last one of the tile that starts at or before it
                if (staged) {
                    while (r < h) {
                        const int64_t mid = (r + h + 1) >> 1;
                        if ((int64_t)rowptr[mid] <= i) r = mid;
                        else h = mid - 1;
                    }
                } else {
                    while (r < h) {
                        const int64_t mid = (r + h + 1) >> 1;
                        if ((int64_t)indptr[row_lo + mid] <= e_lo + i) r = mid;
                        else h = mid - 1;
                    }
                }
                const int64_t f = (row_lo + r) * d + col;
                // (a canonical matrix passes always; one that is not writes nothing outside the tile's image)
                if (col >= 0 && col < d && f >= lo && f < hi) image[f + shift - p0] = value;
            };
#pragma unroll
            for (int j = 0; j < CSR_AHEAD; j++)
                if (tid + j * CSR_THREADS < run) place(tid + j * CSR_THREADS, col_ahead[j], val_ahead[j]);
            for (int64_t i = tid + CSR_AHEAD * CSR_THREADS; i < run; i += CSR_THREADS) place(i, (int64_t)indices[e_lo + i], values[e_lo + i]);
            __syncthreads();
        }
        for (int i = tid; i < CSR_TILE / 4; i += CSR_THREADS) {
            const int64_t p = p0 + 4 * (int64_t)i;  // dst + (p - shift) is 16-byte aligned
            const float4 v = stored ? image4[i] : zero4;
            if (p >= shift && p + 4 <= total + shift) {
                *(float4 *)(dst + (p - shift)) = v;
            } else {  // the buffer's first and last chunk, where it does not start or end on a 16-byte boundary
                const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (p + q >= shift && p + q < total + shift) dst[p + q - shift] = e4[q];
            }
        }
        if (stored) __syncthreads();  // the image is zeroed again for the block's next tile
        e_lo = e_hi;
        e_hi = e_next;
    }
}

template <typename IP, typename IX>
static int csr_launch(hipStream_t st, const void *indptr, const void *indices, const float *values, int64_t n, int d, float *dst) {
    const int shift = (int)(((uintptr_t)dst >> 2) & 3);
    const int64_t tiles = (n * (int64_t)d + shift + CSR_TILE - 1) / CSR_TILE;
    const int64_t per_block = (tiles + 8191) / 8192;  // at most 8192 chunks of consecutive tiles
    const int64_t blocks = (tiles + per_block - 1) / per_block;
    hipLaunchKernelGGL((k_csr_rows<IP, IX>), dim3((unsigned)blocks), dim3(CSR_THREADS), 0, st, (const IP *)indptr, (const IX *)indices, values, n, d,
                       dst, shift, tiles, per_block);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

static thread_local char g_sperr[256] = {0};
void nnd_set_global_error(const char *msg);  // handle.hip: what nnd_last_global_error returns

static int sp_fail(const char *msg) {
    snprintf(g_sperr, sizeof(g_sperr), "%s", msg);
    nnd_set_global_error(g_sperr);
    return 1;
}

extern "C" int32_t nnd_device_csr_rows(int32_t device, void *hip_stream, const void *indptr_dev, int32_t indptr_width, const void *indices_dev,
                                       int32_t indices_width, const float *values_dev, int64_t n, int32_t dim, float *dst_dev) {
    if (n < 0 || dim < 0 || (indptr_width != 4 && indptr_width != 8) || (indices_width != 4 && indices_width != 8))
        return sp_fail("nnd_device_csr_rows: bad shape or index width");
    if (n == 0 || dim == 0) return 0;
    if (!indptr_dev || !dst_dev) return sp_fail("nnd_device_csr_rows: null pointer");
    if ((uintptr_t)dst_dev & 3) return sp_fail("nnd_device_csr_rows: dst is not aligned to a float");
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return sp_fail("nnd_device_csr_rows: no such device"); }
    hipStream_t st = (hipStream_t)hip_stream;
    int rc;
    if (indptr_width == 4) rc = indices_width == 4 ? csr_launch<int32_t, int32_t>(st, indptr_dev, indices_dev, values_dev, n, dim, dst_dev)
                                                   : csr_launch<int32_t, int64_t>(st, indptr_dev, indices_dev, values_dev, n, dim, dst_dev);
    else rc = indices_width == 4 ? csr_launch<int64_t, int32_t>(st, indptr_dev, indices_dev, values_dev, n, dim, dst_dev)
                                 : csr_launch<int64_t, int64_t>(st, indptr_dev, indices_dev, values_dev, n, dim, dst_dev);
    if (rc) {
        (void)hipGetLastError();
        return sp_fail("nnd_device_csr_rows: kernel launch failed");
    }
    return 0;
}
