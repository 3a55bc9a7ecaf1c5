// searcher.hip -- the searcher's lifetime: create (from host arrays or from device memory), fill, destroy; and
// quantization="uint8": the code rows and the two tables of the proxy walk.  The walk itself is query.hip.
#include "searcher.h"

// devarray.hip: rows of NND_DTYPE_* `dtype` gathered by `order` (nullptr: identity) into float32 rows of dp floats, zero padded
int nnd_launch_gather_rows(hipStream_t st, const void *src, int dtype, const int32_t *order, int64_t n, int d, int dp, float *dst);

thread_local char g_serr[512] = {0};

// the searcher's copy of the rows for the codes 2..5: the build's row transform (metric.h), one wave per row, in place --
// dot: L2-normalised; correlation: minus the row mean (float64), then normalised; hellinger: sqrt, then normalised
__global__ void k_searcher_prep_rows(float *__restrict__ x, int64_t n, int d, int dp, int metric) {
    const int lane = nnd_lane();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float *row = x + r * dp;
    const double mu = metric == 4 ? nnd_row_mean_f64<64>(row, d, lane) : 0.0;
    float s = 0.0f;
    for (int j = lane; j < d; j += 64) {
        const float v = nnd_unit_transform(metric, row[j], mu);
        row[j] = v;
        s += v * v;
    }
    s = nnd_wave_sum_f32(s);
    const float inv = s > 0.0f ? 1.0f / sqrtf(s) : 0.0f;
    for (int j = lane; j < d; j += 64) row[j] *= inv;
}

// the boolean family: the searcher's rows become indicator rows in place (x != 0 -> 1, else 0; the padding stays 0), so that
// k_row_norm2 gives nnz(x) and every product of the walk is a count
__global__ void k_searcher_indicator_rows(float *__restrict__ x, int64_t n, int dp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * dp) x[i] = x[i] != 0.0f ? 1.0f : 0.0f;
}
static void searcher_indicator_rows(nnd_searcher_s *s, hipStream_t st) {
    const int64_t total = s->n * s->dp;
    hipLaunchKernelGGL(k_searcher_indicator_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, s->x, s->n, s->dp);
}

// squared norms of the padded rows (alternative_cosine recomputes them per call, distances.py:617-620)
__global__ void k_row_norm2(const float *__restrict__ x, int64_t n, int dp, float *__restrict__ out) {
    const int lane = nnd_lane();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float s = 0.0f;
    for (int j = lane; j < dp; j += 64) {
        const float v = x[r * dp + j];
        s += v * v;
    }
    s = nnd_wave_sum_f32(s);
    if (lane == 0) out[r] = s;
}

// uint8 codes of the searcher's rows (pynndescent_.py:2207-2209: np.searchsorted(values, raw).astype(np.uint8)): one wave
// per row, one element per lane.  The search is a branchless searchsorted-left over the 256-entry table `tab` (the codebook,
// +inf past its n_values entries): a value above the last entry gets n_values, and 256 wraps to code 0 through the uint8
// cast, bit for bit as the reference.  Code rows have stride dcs, padding bytes 0.  cn2 (cosine / dot; may be null): the
// row's sum of lut[c]^2 with the walk's table.  x == nullptr: the codes are already in place, only cn2 is computed.
__global__ __launch_bounds__(256) void k_quantize_u8(const float *__restrict__ x, int64_t xstride, int64_t n, int d, int dcs,
                                                     const float *__restrict__ lut, const float *__restrict__ tab,
                                                     uint8_t *__restrict__ codes, float *__restrict__ cn2) {
    __shared__ float st[256], lt[256];
    st[threadIdx.x] = tab[threadIdx.x];
    lt[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int lane = nnd_lane();
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {  // wave-uniform
        float s = 0.0f;
        for (int j = lane; j < dcs; j += 64) {
            uint32_t c = 0;
            if (x) {
                if (j < d) {
                    const float v = x[r * xstride + j];
                    int lo = 0;
#pragma unroll
                    for (int h = 128; h > 0; h >>= 1) lo += st[lo + h - 1] < v ? h : 0;
                    lo += st[lo] < v ? 1 : 0;  // 0 .. 256
                    c = (uint32_t)lo & 0xFFu;
                }
                codes[r * dcs + j] = (uint8_t)c;
            } else {
                c = codes[r * dcs + j];
            }
            if (j < d) s += lt[c] * lt[c];
        }
        if (cn2) {
            s = nnd_wave_sum_f32(s);
            if (lane == 0) cn2[r] = s;
        }
    }
}

static int upload_padded(nnd_searcher_s *s, float **dst, const float *src, int64_t rows, int d, int dp) {
    S_ALLOC(dst, (size_t)(rows ? rows : 1) * dp);
    if (rows == 0) return 0;
    if (d == dp) {
        S_HIP(hipMemcpy(*dst, src, sizeof(float) * (size_t)rows * d, hipMemcpyHostToDevice));
    } else {
        S_HIP(hipMemset(*dst, 0, sizeof(float) * (size_t)rows * dp));
        S_HIP(hipMemcpy2D(*dst, sizeof(float) * dp, src, sizeof(float) * d, sizeof(float) * d, (size_t)rows, hipMemcpyHostToDevice));
    }
    return 0;
}

extern "C" const char *nnd_searcher_last_error(nnd_searcher_t s) { return s ? s->err : g_serr; }

extern "C" int32_t nnd_searcher_destroy(nnd_searcher_t s) {
    if (!s) return 0;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    s->mem.release_all();
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return 0;
}

// the searcher's copy of the rows, made ready on `st`: the metric's row transform, then the squared norms
static void searcher_prep(nnd_searcher_s *s, hipStream_t st) {
    if (s->metric == NND_METRIC_ALT_DOT || s->metric == NND_METRIC_CORRELATION || s->metric == NND_METRIC_ALT_HELLINGER)
        hipLaunchKernelGGL(k_searcher_prep_rows, dim3((unsigned)((s->n + 3) / 4)), dim3(256), 0, st, s->x, s->n, s->d, s->dp, s->metric);
    if (nnd_metric_bool(s->metric)) searcher_indicator_rows(s, st);
    hipLaunchKernelGGL(k_row_norm2, dim3((unsigned)((s->n + 3) / 4)), dim3(256), 0, st, s->x, s->n, s->dp, s->xn2);
}
// the four tree tables, from the host (blocking copies)
static int searcher_upload_tree(nnd_searcher_s *s, const float *hyperplanes, const float *offsets, const int32_t *children, const int32_t *tree_indices) {
    if (s->n_nodes <= 0) return 0;
    if (upload_padded(s, &s->hyper, hyperplanes, s->n_nodes, s->d, s->dp)) return 1;
    S_ALLOC(&s->offsets, (size_t)s->n_nodes);
    S_HIP(hipMemcpy(s->offsets, offsets, sizeof(float) * (size_t)s->n_nodes, hipMemcpyHostToDevice));
    S_ALLOC(&s->children, 2 * (size_t)s->n_nodes);
    S_HIP(hipMemcpy(s->children, children, sizeof(int32_t) * 2 * (size_t)s->n_nodes, hipMemcpyHostToDevice));
    S_ALLOC(&s->tree_idx, (size_t)s->n);
    S_HIP(hipMemcpy(s->tree_idx, tree_indices, sizeof(int32_t) * (size_t)s->n, hipMemcpyHostToDevice));
    return 0;
}

static int searcher_fill(nnd_searcher_s *s, const float *data, const int32_t *indptr, const int32_t *indices, const float *hyperplanes,
                         const float *offsets, const int32_t *children, const int32_t *tree_indices) {
    S_HIP(hipSetDevice(s->device));
    S_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    if (upload_padded(s, &s->x, data, s->n, s->d, s->dp)) return 1;
    S_ALLOC(&s->xn2, (size_t)s->n);
    searcher_prep(s, s->stream);
    S_ALLOC(&s->indptr, (size_t)(s->n + 1));
    S_HIP(hipMemcpy(s->indptr, indptr, sizeof(int32_t) * (size_t)(s->n + 1), hipMemcpyHostToDevice));
    S_ALLOC(&s->indices, (size_t)s->nnz);
    S_HIP(hipMemcpy(s->indices, indices, sizeof(int32_t) * (size_t)s->nnz, hipMemcpyHostToDevice));
    if (searcher_upload_tree(s, hyperplanes, offsets, children, tree_indices)) return 1;
    S_HIP(hipStreamSynchronize(s->stream));
    return 0;
}

// the same state from device memory, on the caller's stream: rows gathered by `order` straight into the padded layout
// (devarray.hip), the CSR copied device to device; the tree tables come from the host as above
static int searcher_fill_device(nnd_searcher_s *s, const void *rows, int dtype, const int32_t *order, const int32_t *indptr, const int32_t *indices,
                                const float *hyperplanes, const float *offsets, const int32_t *children, const int32_t *tree_indices, hipStream_t st) {
    S_HIP(hipSetDevice(s->device));
    S_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    S_ALLOC(&s->x, (size_t)s->n * s->dp);
    S_ALLOC(&s->xn2, (size_t)s->n);
    S_ALLOC(&s->indptr, (size_t)(s->n + 1));
    S_ALLOC(&s->indices, (size_t)s->nnz);
    if (nnd_launch_gather_rows(st, rows, dtype, order, s->n, s->d, s->dp, s->x)) {
        (void)hipGetLastError();
        s->set_error("the rows' gather could not be launched (dtype %d)", dtype);
        return 1;
    }
    searcher_prep(s, st);
    S_HIP(hipGetLastError());
    S_HIP(hipMemcpyAsync(s->indptr, indptr, sizeof(int32_t) * (size_t)(s->n + 1), hipMemcpyDeviceToDevice, st));
    if (s->nnz > 0) S_HIP(hipMemcpyAsync(s->indices, indices, sizeof(int32_t) * (size_t)s->nnz, hipMemcpyDeviceToDevice, st));
    if (searcher_upload_tree(s, hyperplanes, offsets, children, tree_indices)) return 1;
    S_HIP(hipStreamSynchronize(st));  // the caller's buffers are free again, and the searcher's own stream may read what was written
    return 0;
}

// what the two create entries share: the argument and device checks, and the searcher with its scalars set (nullptr: g_serr says why)
static nnd_searcher_s *searcher_new(const char *who, bool args_ok, int32_t device, int64_t n, int32_t dim, int32_t metric, int64_t nnz,
                                    bool tree_ok, int64_t n_nodes, float min_distance, int32_t n_neighbors, const int64_t *rng_state) {
    auto fail = [&](const char *msg) -> nnd_searcher_s * {
        snprintf(g_serr, sizeof(g_serr), "%s: %s", who, msg);
        return nullptr;
    };
    if (!args_ok || n < 1 || dim < 1 || nnz < 0) return fail("bad arguments");
    if (metric < NND_METRIC_SQEUCLIDEAN || metric > NND_METRIC_YULE || metric == NND_METRIC_PROXY_INNER_PRODUCT + 1) return fail("unknown metric");
    if (nnd_metric_bool(metric) && dim >= (1 << 23)) return fail("the boolean metrics need dim < 2^23");
    if (n_nodes > 0 && !tree_ok) return fail("tree arrays missing");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail("device out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("this build targets gfx950 (MI355X) only");
    nnd_searcher_s *s = new nnd_searcher_s();
    s->device = device;
    s->n = n;
    s->nnz = nnz;
    s->n_nodes = n_nodes;
    s->d = dim;
    s->dp = (dim + 3) & ~3;
    s->metric = metric;
    s->n_neighbors = n_neighbors;
    s->min_distance = min_distance;
    s->seed = rng_state ? nnd_mix32((uint32_t)rng_state[0] ^ nnd_mix32((uint32_t)rng_state[1] + 0x9E3779B9u) ^ nnd_mix32((uint32_t)rng_state[2] + 0x7F4A7C15u)) : 1u;
    return s;
}
static int searcher_filled(const char *who, nnd_searcher_s *s, int rc, nnd_searcher_t *out) {
    if (rc) {
        snprintf(g_serr, sizeof(g_serr), "%s: %s", who, s->err);
        nnd_searcher_destroy(s);
        return 1;
    }
    *out = s;
    return 0;
}

extern "C" int32_t nnd_searcher_create(nnd_searcher_t *out, int32_t device, int64_t n, int32_t dim, int32_t metric, const float *data,
                                       const int32_t *indptr, const int32_t *indices, int64_t nnz, const float *hyperplanes,
                                       const float *offsets, const int32_t *children, const int32_t *tree_indices, int64_t n_nodes,
                                       float min_distance, int32_t n_neighbors, const int64_t *rng_state) {
    nnd_searcher_s *s = searcher_new("nnd_searcher_create", out && data && indptr && indices, device, n, dim, metric, nnz,
                                     hyperplanes && offsets && children && tree_indices, n_nodes, min_distance, n_neighbors, rng_state);
    if (!s) return 1;
    return searcher_filled("nnd_searcher_create", s, searcher_fill(s, data, indptr, indices, hyperplanes, offsets, children, tree_indices), out);
}

extern "C" int32_t nnd_searcher_create_device(nnd_searcher_t *out, int32_t device, int64_t n, int32_t dim, int32_t metric, const void *rows_dev,
                                              int32_t dtype, const int32_t *order_dev, const int32_t *indptr_dev, const int32_t *indices_dev,
                                              int64_t nnz, const float *hyperplanes, const float *offsets, const int32_t *children,
                                              const int32_t *tree_indices, int64_t n_nodes, float min_distance, int32_t n_neighbors,
                                              const int64_t *rng_state, void *hip_stream) {
    const bool args_ok = out && rows_dev && indptr_dev && (indices_dev || nnz == 0) && dtype >= NND_DTYPE_FLOAT32 && dtype <= NND_DTYPE_FLOAT64;
    nnd_searcher_s *s = searcher_new("nnd_searcher_create_device", args_ok, device, n, dim, metric, nnz,
                                     hyperplanes && offsets && children && tree_indices, n_nodes, min_distance, n_neighbors, rng_state);
    if (!s) return 1;
    return searcher_filled("nnd_searcher_create_device", s,
                           searcher_fill_device(s, rows_dev, dtype, order_dev, indptr_dev, indices_dev, hyperplanes, offsets, children, tree_indices,
                                                (hipStream_t)hip_stream), out);
}

// ---- quantization="uint8" (pynndescent_.py:2191-2225, 2309-2364) ----
// the two 256-entry tables: the walk's codebook (entries past n_values = the last value; the reference reads past its
// array there, DESIGN.md "Quantized search") and the search table (+inf past n_values)
static int quant_tables(nnd_searcher_s *s, const char *who, const float *values, int32_t n_values) {
    if (s->metric != NND_METRIC_SQEUCLIDEAN && s->metric != NND_METRIC_ALT_COSINE && s->metric != NND_METRIC_ALT_DOT) {
        s->set_error("%s: uint8 quantization supports the sqeuclidean, alternative cosine and alternative dot metrics (metric %d)", who, s->metric);
        return 1;
    }
    if (!values || n_values < 1 || n_values > 256) { s->set_error("%s: the codebook must have 1..256 values (got %d)", who, n_values); return 1; }
    S_HIP(hipSetDevice(s->device));
    S_HIP(hipStreamSynchronize(s->stream));  // no kernel or copy of an earlier call still uses the tables
    float *tab = s->tab_host;
    for (int i = 0; i < 256; i++) {
        tab[i] = values[i < n_values ? i : n_values - 1];
        tab[256 + i] = i < n_values ? values[i] : INFINITY;
    }
    s->dcs = (s->d + 15) & ~15;
    if (!s->lut) S_ALLOC(&s->lut, 512);
    if (!s->codes) S_ALLOC(&s->codes, (size_t)s->n * s->dcs);
    if (!s->cn2 && s->metric != NND_METRIC_SQEUCLIDEAN) S_ALLOC(&s->cn2, (size_t)s->n);
    // queued on the searcher's stream, so the kernels that read the tables are ordered after it (the stream is
    // non-blocking: it does not wait for copies on the null stream); tab_host outlives the copy (next call syncs first)
    S_HIP(hipMemcpyAsync(s->lut, tab, sizeof(float) * 512, hipMemcpyHostToDevice, s->stream));
    return 0;
}

static int quant_launch(nnd_searcher_s *s, const float *x, int64_t xstride) {
    const int64_t blocks = (s->n + 3) / 4 < 4096 ? (s->n + 3) / 4 : 4096;
    hipLaunchKernelGGL(k_quantize_u8, dim3((unsigned)blocks), dim3(256), 0, s->stream, x, xstride, s->n, s->d, s->dcs, (const float *)s->lut,
                       (const float *)(s->lut + 256), s->codes, s->cn2);
    S_HIP(hipGetLastError());
    return 0;
}

extern "C" int32_t nnd_searcher_quantize_u8(nnd_searcher_t s, const float *rows, const float *values, int32_t n_values, uint8_t *codes_out) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_quantize_u8: null searcher"); return 1; }
    if (quant_tables(s, "nnd_searcher_quantize_u8", values, n_values)) return 1;
    nnd_scratch tmp;  // released on return, behind the synchronise below
    float *drows = nullptr;
    if (rows) {
        if (!(drows = tmp.get<float>(s, (size_t)s->n * s->d))) return 1;
        if (hipMemcpyAsync(drows, rows, sizeof(float) * (size_t)s->n * s->d, hipMemcpyHostToDevice, s->stream) != hipSuccess) {
            s->set_error("nnd_searcher_quantize_u8: H2D of the rows failed");
            return 1;
        }
    }
    int rc = rows ? quant_launch(s, drows, s->d) : quant_launch(s, s->x, s->dp);
    if (!rc && codes_out &&
        hipMemcpy2DAsync(codes_out, (size_t)s->d, s->codes, (size_t)s->dcs, (size_t)s->d, (size_t)s->n, hipMemcpyDeviceToHost, s->stream) != hipSuccess) {
        s->set_error("nnd_searcher_quantize_u8: D2H of the codes failed");
        rc = 1;
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess && !rc) {
        s->set_error("nnd_searcher_quantize_u8: kernel failed: %s", hipGetErrorString(hipGetLastError()));
        rc = 1;
    }
    return rc;
}

extern "C" int32_t nnd_searcher_set_codes_u8(nnd_searcher_t s, const float *values, int32_t n_values, const uint8_t *codes) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_set_codes_u8: null searcher"); return 1; }
    if (!codes) { s->set_error("nnd_searcher_set_codes_u8: codes missing"); return 1; }
    if (quant_tables(s, "nnd_searcher_set_codes_u8", values, n_values)) return 1;
    S_HIP(hipMemsetAsync(s->codes, 0, (size_t)s->n * s->dcs, s->stream));
    S_HIP(hipMemcpy2DAsync(s->codes, (size_t)s->dcs, codes, (size_t)s->d, (size_t)s->d, (size_t)s->n, hipMemcpyHostToDevice, s->stream));
    if (s->cn2 && quant_launch(s, nullptr, 0)) return 1;
    S_HIP(hipStreamSynchronize(s->stream));
    return 0;
}
